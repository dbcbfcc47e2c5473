"""Product and review embeddings built on the GPU: text in, searchable index (and the reference's files) out.

Stands in for nlp/11_build_product_embeddings.py:46-92 (`SentenceTransformer.encode(texts, normalize_embeddings=True)`
over `normalize_text(agg_text)`), the builder of product_emb.npy / product_emb_meta.parquet.  Per chunk of documents:

    UTF-8 bytes + offsets in pinned memory -> one copy to the device
    rr_wp_encode_dev          WordPiece ids, packed            (csrc/rr_wordpiece.hip, on a stream of its own)
    rr_ce_forward_dev         12 layers, CLS rows              (csrc/rr_ce.hip)
    rr_index_store_rows_dev   x / max(||x||, 1e-12) into the index's rows

with no host hop between the three: the host reads back two integers per chunk (tokens, longest sequence: what the forward
call takes as arguments) and the needs_host flags, and prepares chunk i + 1 while chunk i runs.  The tokenizer takes UTF-8
(Unicode text through the table of wp_unicode.py); the few documents it flags (a hard code point, a mapped text beyond
its buffers: wp_unicode.model_tokenize) are tokenised by wordpiece.py and encoded in one small pass at the end, scattered into
their rows.

Review embeddings (nlp/11...:95-169, the builder of reviews_with_embeddings.parquet) take the same chain behind three more
device stages (csrc/rr_textprep.hip, textprep.py), because the reference cleans review text before the model sees it:

    raw UTF-8 bytes, in row blocks through pinned staging -> the device
    rr_textprep_clean_dev     normalize_text, the length filter, looks_spammy: text in place, length and status per row
    (the few rows the kernel flags are cleaned by normalize_text / looks_spammy below and written into their slots)
    rr_textprep_dedup_dev     drop_duplicates(subset=["sku", "__txt"]): byte-compared, first row in file order survives
    rr_textprep_compact_dev   the survivors' texts back to back + offsets: what rr_wp_encode_dev reads, still on the device

and from there chunk by chunk through the tokenizer, the encoder and the row store (`build_review_embeddings`).

Product text that the products builder left on the device (products.DeviceProductText) needs no strings at all:
`build_product_embeddings_device` cuts normalize_text's heads there (rr_textprep_head_measure_dev /
rr_textprep_head_write_dev) and feeds them to the same chain (`--target product --reviews FILE`).
"""
from __future__ import annotations

import argparse
import ctypes as C
import re
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .index import ProductIndex
from .wordpiece import WordPieceTokenizer

MIN_TEXT_LEN = 10       # nlp/11_build_product_embeddings.py:22-23
MAX_TEXT_LEN = 4000
NORMALIZE_EPS = 1e-12   # torch.nn.functional.normalize's eps (normalize_embeddings=True)
META_COLUMNS = ("sku", "n_reviews", "avg_stars", "last_ts", "agg_text")     # nlp/11...:86-89
_WS = re.compile(r"\s+")
REVIEW_COLUMNS = ("id", "sku", "ts", "stars", "text")                       # nlp/11...:103
REVIEW_INPUT = "data/processed/reviews_merged.parquet"                      # nlp/11...:14
PRODUCT_INPUT = "data/processed/products.parquet"
URL_RE = re.compile(r"https?://\S+|www\.\S+", re.IGNORECASE)               # nlp/11...:25-27
PROMO_RE = re.compile(r"(discount code|use code|sponsored|i received this.*free)", re.IGNORECASE)
REPEAT_RE = re.compile(r"(.)\1{9,}")
MAX_TEXT_BYTES = 8 << 30        # review text kept on the device until it is encoded (dedup must see all of it)
STAGE_BYTES = 64 << 20          # one of the two pinned staging buffers the raw text passes through
RESUME_REFUSED = ("--resume is not supported: the reference reopens reviews_with_embeddings.parquet with a fresh writer, "
                  "which truncates the rows it claims to keep; run the build again without --resume")


def normalize_text(s) -> str:
    """nlp/11_build_product_embeddings.py:32-36."""
    if not isinstance(s, str):
        s = "" if s is None else str(s)
    s = s.replace("\r", " ").replace("\n", " ").strip()
    s = _WS.sub(" ", s)
    return s[:MAX_TEXT_LEN]


def looks_spammy(s: str) -> bool:
    """nlp/11_build_product_embeddings.py:38-39."""
    return (len(URL_RE.findall(s)) >= 2) or bool(PROMO_RE.search(s)) or bool(REPEAT_RE.search(s))


def filter_products(products, text_col: str = "agg_text"):
    """(meta, texts) as nlp/11...:58-62 and :86-89 make them: rows whose normalised text is shorter than MIN_TEXT_LEN go,
    order stays; meta = sku, n_reviews, avg_stars, last_ts, agg_text with missing columns NaN and agg_text the RAW column
    (after fillna("").astype(str)); texts = the normalised strings the model sees."""
    import pandas as pd
    if "sku" not in products.columns:
        raise ValueError("the product table must have 'sku'")
    if text_col not in products.columns:
        raise ValueError(f"the product table has no text column {text_col!r}")
    df = products.copy()
    df[text_col] = df[text_col].fillna("").astype(str)
    txt = df[text_col].map(normalize_text)
    keep = (txt.str.len() >= MIN_TEXT_LEN).values
    if not keep.any():
        raise RuntimeError("No products left after filtering.")
    df, txt = df[keep], txt[keep]
    meta = pd.DataFrame({"sku": df["sku"].values})
    for c in ("n_reviews", "avg_stars", "last_ts"):
        meta[c] = df[c].values if c in df.columns else np.nan
    meta["agg_text"] = df[text_col].values
    return meta.reset_index(drop=True), txt.tolist()


# ---------------------------------------------------------------------------------- the piece table
def piece_arrays(vocab: Dict[str, int]) -> Tuple[np.ndarray, np.ndarray]:
    """(bytes, offsets) of rr_wp_create_utf8: piece i = the vocabulary string with id i, empty where no string has that id."""
    n = max(vocab.values()) + 1
    pieces: List[bytes] = [b""] * n
    for s, i in vocab.items():
        if i < 0:
            raise ValueError(f"vocabulary id {i} of {s!r} is negative")
        pieces[i] = s.encode("utf-8")
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(p) for p in pieces], out=off[1:])
    blob = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy() if off[-1] else np.zeros(1, dtype=np.uint8)
    return blob, off


def build_piece_table(vocab: Dict[str, int], max_chars_per_word: int = 100):
    """The open-addressing table the device matches against, built by the library ON THE HOST (rr_wp_build_table_utf8; no GPU
    needed): (slots [n_slots][4] int32 = hash, first byte, length in bytes | ## form << 16, id or -1; piece bytes; pieces
    kept).  max_chars_per_word counts code points."""
    lib = _lib.load()
    blob, off = piece_arrays(vocab)
    n_slots, kept = C.c_int32(), C.c_int32()
    _lib.check(lib.rr_wp_table_slots(len(off) - 1, C.byref(n_slots)), "rr_wp_table_slots")
    slots = np.empty((n_slots.value, 4), dtype=np.int32)
    _lib.check(lib.rr_wp_build_table_utf8(_lib.ptr(blob), _lib.ptr(off), len(off) - 1, max_chars_per_word, n_slots.value,
                                          _lib.ptr(slots), C.byref(kept)), "rr_wp_build_table_utf8")
    return slots, blob, kept.value


class DeviceWordPiece:
    """`WordPieceTokenizer` for single texts on one GPU (csrc/rr_wordpiece.hip): UTF-8 text over the per-code-point table of
    wp_unicode.unicode_tables(); it leaves to the host only what wp_unicode.model_tokenize flags."""

    def __init__(self, tokenizer: WordPieceTokenizer, device: int = 0):
        if not tokenizer.do_lower_case:
            raise ValueError("the device tokenizer lower-cases (uncased vocabularies); this tokenizer does not")
        import torch
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the device tokenizer runs on the device only")
        from .wp_unicode import unicode_tables
        self._torch, self.tokenizer, self.device = torch, tokenizer, device
        self._dev = torch.device("cuda", device)
        blob, off = piece_arrays(tokenizer.vocab)
        t = unicode_tables()
        st1, st2, pool = t["stage1"], t["stage2"], t["pool"]
        h = C.c_void_p()
        _lib.check(_lib.load().rr_wp_create_utf8(device, _lib.ptr(blob), _lib.ptr(off), len(off) - 1, tokenizer.unk_id,
                                                 tokenizer.cls_id, tokenizer.sep_id, tokenizer.max_chars_per_word,
                                                 _lib.ptr(st1), len(st1), _lib.ptr(st2), len(st2), _lib.ptr(pool), len(pool),
                                                 C.byref(h)), "rr_wp_create_utf8")
        self._h = h

    @property
    def handle(self):
        return self._h

    def queue(self, docs: Sequence[bytes], max_length: int, capacity: Optional[int] = None):
        """Queues one batch on torch's CURRENT stream and returns without waiting: (packed, info, n, cap, keepalive).  `packed` is one
        int32 device tensor [tok cap | typ cap | pos cap | cu n + 1 | needs_host n | max_len 1]; `info` its tail from cu[n] on
        (tokens, needs_host flags, longest sequence) on its way to pinned host memory; `keepalive` the staged text (pinned,
        device), to be held until the batch has run."""
        torch = self._torch
        n = len(docs)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(d) for d in docs], out=off[1:])
        nbytes = int(off[-1])
        stage = torch.empty(8 * (n + 1) + nbytes + 8, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        host[:8 * (n + 1)] = off.view(np.uint8)
        host[8 * (n + 1):8 * (n + 1) + nbytes] = np.frombuffer(b"".join(docs), dtype=np.uint8)
        with torch.cuda.device(self._dev):
            d_in = stage.to(self._dev, non_blocking=True)       # [offsets int64 (n + 1)] [text]
        packed, info, n, cap, _ = self.queue_dev(d_in.data_ptr() + 8 * (n + 1), nbytes, d_in[:8 * (n + 1)].view(torch.int64),
                                                 max_length, capacity)
        return packed, info, n, cap, (stage, d_in)

    def queue_dev(self, d_text: int, text_bytes: int, d_off, max_length: int, capacity: Optional[int] = None):
        """`queue` for text that is ALREADY on the device: d_text = address of the first byte, d_off = int64 device tensor of
        n + 1 offsets relative to it (text_bytes = the last one, a host integer below 2^31).  Same return value; the
        keepalive holds d_off, the text stays the caller's."""
        torch = self._torch
        n = int(d_off.numel()) - 1
        cap = int(capacity) if capacity else n * int(max_length)
        with torch.cuda.device(self._dev):
            packed = torch.empty(3 * cap + 2 * n + 2, dtype=torch.int32, device=self._dev)
            base, st = packed.data_ptr(), torch.cuda.current_stream(self._dev).cuda_stream
            _lib.check(_lib.load().rr_wp_encode_dev(
                self._h, C.c_void_p(d_text), int(text_bytes), C.c_void_p(d_off.data_ptr()), n, int(max_length), cap,
                C.c_void_p(base), C.c_void_p(base + 4 * cap), C.c_void_p(base + 8 * cap), C.c_void_p(base + 12 * cap),
                C.c_void_p(base + 4 * (3 * cap + n + 1)), C.c_void_p(base + 4 * (3 * cap + 2 * n + 1)), C.c_void_p(st)),
                "rr_wp_encode_dev")
            info = torch.empty(n + 2, dtype=torch.int32, pin_memory=True)
            info.copy_(packed[3 * cap + n:], non_blocking=True)
        return packed, info, n, cap, (None, d_off)

    @staticmethod
    def views(packed, n: int, cap: int, total: int):
        """(tok, typ, pos, cu) views of `packed` once the host knows `total` = cu[n]."""
        return (packed[:total], packed[cap:cap + total], packed[2 * cap:2 * cap + total], packed[3 * cap:3 * cap + n + 1])

    def encode_dev(self, texts: Sequence[str], max_length: int):
        """The packed device tensors of `texts` (what `forward_packed_dev` takes) and the documents left to the host:
        (tok, typ, pos, cu_seqlens, max_len, needs_host) -- int32 device tensors, the longest sequence, and the indices of
        the documents that were NOT tokenised (malformed UTF-8, a hard code point, a mapped text beyond the buffers, or
        longer than the kernel's window and not answerable from it): their sequences are the placeholder [CLS] [SEP].
        Waits for the result (the sizes are host integers)."""
        torch = self._torch
        packed, info, n, cap, _keep = self.queue([t.encode("utf-8") for t in texts], max_length)
        torch.cuda.current_stream(self._dev).synchronize()
        self.check()
        h = info.numpy()
        tok, typ, pos, cu = self.views(packed, n, cap, int(h[0]))
        return tok, typ, pos, cu, int(h[n + 1]), np.flatnonzero(h[1:n + 1]).tolist()

    def check(self) -> None:
        """Raises ValueError when a batch since the last check had offsets that decrease or leave the text (waits for the device)."""
        bad = C.c_int32()
        _lib.check(_lib.load().rr_wp_status(self._h, C.byref(bad)), "rr_wp_status")

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_wp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------- text -> rows of an index
def _plan_chunks(docs_len: Sequence[int], max_length: int, chunk_tokens: int) -> List[Tuple[int, int]]:
    """Consecutive documents per chunk: a document of b bytes gives at most min(max_length, b + 2) tokens."""
    chunks, a, tot = [], 0, 0
    for i, b in enumerate(docs_len):
        t = min(max_length, b + 2)
        if i > a and tot + t > chunk_tokens:
            chunks.append((a, i))
            a, tot = i, 0
        tot += t
    if a < len(docs_len):
        chunks.append((a, len(docs_len)))
    return chunks


def embed_texts_into(index: ProductIndex, texts: Sequence[str], encoder, *, first_row: int = 0,
                     chunk_tokens: int = 131072, keep_rows: bool = False, stats: Optional[dict] = None) -> Optional[np.ndarray]:
    """Encodes `texts` AS THEY ARE (no normalize_text, no length filter: build_product_embeddings does those) into rows
    [first_row, first_row + len(texts)) of `index` (local rows), l2-normalised with eps 1e-12.  `encoder` is a QueryEncoder
    with a vocabulary.  keep_rows: also return the normalised fp32 rows on the host (what a bf16 index cannot give back).
    stats: a dict that receives "host_docs", the documents (indices into `texts`) the device tokenizer left to the host pass.

    The forward call gets the EXACT longest sequence of its chunk (read back with the token count, which it needs anyway),
    not the bound max_length."""
    lens = [len(t.encode("utf-8")) for t in texts]

    def queue_docs(wp, a, b, L, cap):
        return wp.queue([t.encode("utf-8") for t in texts[a:b]], L, cap)

    return _embed_into(index, lens, queue_docs, lambda i: texts[i], encoder, first_row=first_row, chunk_tokens=chunk_tokens,
                       keep_rows=keep_rows, stats=stats)


def _embed_into(index: ProductIndex, lens: Sequence[int], queue_docs, host_text, encoder, *, first_row: int, chunk_tokens: int,
                keep_rows: bool, stats: Optional[dict]) -> Optional[np.ndarray]:
    """`embed_texts_into` for any source of documents: lens = their lengths in bytes; queue_docs(wp, a, b, max_length,
    capacity) queues documents [a, b) on the current stream as DeviceWordPiece.queue does (host text) or queue_dev (text on
    the device); host_text(i) = document i as a str, asked only for what the tokenizer leaves to the host."""
    import torch
    if encoder.tokenizer is None:
        raise ValueError("no vocabulary was loaded: the builder tokenises text")
    n = len(lens)
    hidden = encoder.model.hidden                     # the encoder's width = the rows' width
    if first_row < 0 or first_row + n > index.n_rows or index.dim != hidden:
        raise ValueError(f"{n} rows of dim {hidden} from row {first_row} do not fit an index of {index.n_rows} x {index.dim}")
    model, L = encoder.model, encoder.max_length
    out_mode = encoder.out_mode                       # OUT_CLS or OUT_MEAN: the encoder's pooling, one row per document either way
    dev = torch.device("cuda", model.device)
    wp = getattr(encoder, "_device_wp", None)
    if wp is None:
        wp = encoder._device_wp = DeviceWordPiece(encoder.tokenizer, model.device)
    lib = _lib.load()
    kept = np.empty((n, hidden), dtype=np.float32) if keep_rows else None
    fp32 = model.precision == "fp32"
    host_docs: List[int] = []
    with torch.cuda.device(dev):
        main = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        scratch: List[Optional[ProductIndex]] = [None]

        def store(out, first, ids=None):
            _lib.check(lib.rr_index_store_rows_dev(index.handle, C.c_void_p(out.data_ptr()), out.shape[0], first,
                                                   C.c_void_p(ids.data_ptr()) if ids is not None else None, NORMALIZE_EPS,
                                                   C.c_void_p(main.cuda_stream)), "rr_index_store_rows_dev")

        def keep(out, where):
            # the normalised fp32 rows of this chunk through a small fp32 index: the same kernel, so the same bits
            if scratch[0] is None or scratch[0].n_rows < out.shape[0]:
                scratch[0] = ProductIndex(None, n_rows=max(out.shape[0], 256), dim=hidden, device=model.device)
            _lib.check(lib.rr_index_store_rows_dev(scratch[0].handle, C.c_void_p(out.data_ptr()), out.shape[0], 0, None,
                                                   NORMALIZE_EPS, C.c_void_p(main.cuda_stream)), "rr_index_store_rows_dev")
            kept[where] = scratch[0].download_rows(0, out.shape[0])

        def queue_tok(a, b):
            # On the side stream, with no wait for `main`: the buffers are allocated while `side` is current, so the
            # allocator hands out blocks of the side stream's own pool (record_stream below covers their use on `main`),
            # and the tokenizer's scratch is only ever touched on `side`.  The copy and the kernels of chunk i + 1 so run
            # while chunk i's layers do.
            with torch.cuda.stream(side):
                q = queue_docs(wp, a, b, L, max(chunk_tokens, L, 2 * (b - a)))
                ev = torch.cuda.Event()
                ev.record(side)
            for t in (q[0], q[4][1]):
                t.record_stream(main)
            return q, ev

        def forward(job):
            (packed, info, nd, cap, _), _, a, b = job
            h = info.numpy()
            tok, typ, pos, cu = wp.views(packed, nd, cap, int(h[0]))
            narrow = fp32 and not model.wide_range      # which kernels THIS launch runs: decides its redo, whatever comes later
            out = model.forward_packed_dev(tok, typ, pos, cu, nd, int(h[nd + 1]), out_mode)
            store(out, first_row + a)
            flag = None
            if narrow:                      # an out-of-range pass leaves NaN in every pooled row of its call (include/rr_hip.h)
                flag = torch.empty(1, dtype=torch.bool, pin_memory=True)
                flag.copy_(torch.isnan(out[:, 0]).any().reshape(1), non_blocking=True)
            done = torch.cuda.Event()
            done.record(main)
            return out, flag, done

        def settle(job, res):
            """Once the NEXT chunk is queued: this chunk's range flag, the rows to keep.  The flag belongs to the chunk and
            to the kernels it was LAUNCHED on: a chunk queued on the fp16-pair kernels before an earlier chunk's flag was
            read is redone on its own flag, although the handle has switched by then."""
            out, flag, done = res
            done.synchronize()
            if flag is not None and bool(flag[0]):
                if not model.wide_range:
                    model.set_wide_range(True)   # as forward_ids: the handle continues on the wide-range kernels
                out, _, done = forward(job)
                done.synchronize()
            if keep_rows:
                keep(out, slice(job[2], job[3]))

        chunks = _plan_chunks(lens, L, int(chunk_tokens))
        nxt = None
        if chunks:
            nxt = queue_tok(*chunks[0]) + chunks[0]
        prev = None
        for ci in range(len(chunks)):
            job = nxt
            job[1].synchronize()                 # (queued beside the previous chunk's forward pass: normally long done)
            main.wait_event(job[1])
            host_docs += [job[2] + int(i) for i in np.flatnonzero(job[0][1].numpy()[1:job[0][2] + 1])]
            res = forward(job)
            if ci + 1 < len(chunks):
                nxt = queue_tok(*chunks[ci + 1]) + chunks[ci + 1]
            if prev is not None:
                settle(*prev)
            prev = (job, res)
        if prev is not None:
            settle(*prev)
        wp.check()

        # the documents the device left to the host (wp_unicode.model_tokenize's reasons): one small pass, scattered into
        # their rows
        at = 0
        while at < len(host_docs):
            part, tot = [], 0
            while at < len(host_docs) and (not part or tot + L <= chunk_tokens):
                part.append(host_docs[at])
                tot += L
                at += 1
            seqs = [encoder.tokenizer.encode_pair(host_text(i), None, L) for i in part]
            sl = np.array([len(s[0]) for s in seqs], dtype=np.int64)
            cu = np.zeros(len(part) + 1, dtype=np.int32)
            np.cumsum(sl, out=cu[1:])
            T = int(cu[-1])
            ids = np.concatenate([s[0] for s in seqs]).astype(np.int32)
            if ids.min() < 0 or ids.max() >= model.vocab:
                raise ValueError("token id outside the embedding table")
            pos = (np.arange(T, dtype=np.int32) - np.repeat(cu[:-1], sl)).astype(np.int32)
            d = torch.from_numpy(np.concatenate([ids, np.zeros(T, np.int32), pos, cu])).to(dev)
            rows = torch.from_numpy(np.asarray(part, dtype=np.int64) + first_row).to(dev)
            args = (d[:T], d[T:2 * T], d[2 * T:3 * T], d[3 * T:], len(part), int(sl.max()), out_mode)
            out = model.forward_packed_dev(*args)
            if fp32 and not model.wide_range and model.out_of_range():
                model.set_wide_range(True)
                out = model.forward_packed_dev(*args)
            store(out, 0, rows)
            if keep_rows:
                keep(out, np.asarray(part))
        main.synchronize()
        if scratch[0] is not None:
            scratch[0].close()
    if stats is not None:
        stats["host_docs"] = list(host_docs)
    return kept


def build_product_embeddings(products, encoder, *, text_col: str = "agg_text", rows: Optional[Tuple[int, int]] = None,
                             dtype: str = "f32", chunk_tokens: int = 131072, data_dir=None, stats: Optional[dict] = None):
    """nlp/11_build_product_embeddings.py:50-92 on the GPU -> (ProductIndex, meta, emb or None).

    The product table is filtered as the reference does (`filter_products`), its normalised texts are encoded into a new index
    on the encoder's device (`embed_texts_into`), rows l2-normalised (eps 1e-12) like `normalize_embeddings=True`.
    rows=(lo, hi): one row shard of the FILTERED table, created with row_offset=lo (what sharded.py expects); meta is that
    shard's.  With `data_dir`, product_emb.npy and product_emb_meta.parquet are written there (artifacts.save_artifacts) and
    `emb` is the float32 matrix that went into the file: read back from an f32 index, the fp32 rows before rounding for a
    bf16 one."""
    meta, texts = filter_products(products, text_col)
    lo, hi = (0, len(texts)) if rows is None else (int(rows[0]), int(rows[1]))
    if not (0 <= lo < hi <= len(texts)):
        raise ValueError(f"rows=({lo}, {hi}) outside the {len(texts)} products left after filtering")
    meta, texts = meta.iloc[lo:hi].reset_index(drop=True), texts[lo:hi]
    index = ProductIndex(None, n_rows=hi - lo, dim=encoder.model.hidden, device=encoder.model.device, row_offset=lo, dtype=dtype)
    emb = embed_texts_into(index, texts, encoder, chunk_tokens=chunk_tokens,
                           keep_rows=data_dir is not None and dtype != "f32", stats=stats)
    if data_dir is not None:
        from .artifacts import save_artifacts
        if emb is None:
            emb = index.download_rows(0, index.n_rows)
        save_artifacts(data_dir, meta, emb)
    return index, meta, emb


def build_product_embeddings_device(products, text, encoder, *, rows: Optional[Tuple[int, int]] = None, dtype: str = "f32",
                                    chunk_tokens: int = 131072, data_dir=None, stats: Optional[dict] = None,
                                    head_bytes: int = 256 << 20):
    """`build_product_embeddings` for agg_text that is ALREADY on the device (`text`: a products.DeviceProductText, as
    ``build_products(..., keep_device=True)`` leaves it; `products`: its frame, row for row) -> (ProductIndex, meta, emb or
    None, kept).  No string of the text column is made on the host:

        rr_textprep_head_measure_dev   normalize_text's head (4000 code points) of every product: length, status word
        (the lengths and status words come back: they are the chunk plan and the length filter)
        rr_textprep_head_write_dev     the heads of the kept rows, back to back, in row blocks of at most `head_bytes`
        DeviceWordPiece.queue_dev      ... and from there as `embed_texts_into` (`_embed_into`)

    kept = the product rows whose normalised text has at least MIN_TEXT_LEN characters, in order (with rows=(lo, hi): rows
    [lo, hi) of that list, one row shard of the FILTERED table as in `build_product_embeddings`).  The documents the head
    kernel leaves to the host (malformed UTF-8 inside the head: ``stats["host_clean_docs"]``) are fetched, cleaned by
    `normalize_text` and written into their slots.  meta = the rows `kept` of `products` with the columns sku, n_reviews,
    avg_stars, last_ts; the agg_text column is fetched from the device and added ONLY with `data_dir`
    (product_emb_meta.parquet holds it), otherwise meta has no agg_text.  stats also receives "host_docs" (kept rows the
    tokenizer left to the host, whose heads are copied back) and "seconds"."""
    import time
    import pandas as pd
    import torch
    from . import textprep as T
    seconds: Dict[str, float] = {}
    clock = [time.perf_counter()]

    def lap(name):
        now = time.perf_counter()
        seconds[name] = seconds.get(name, 0.0) + now - clock[0]
        clock[0] = now

    if stats is not None:
        stats["seconds"] = seconds
    if "sku" not in products.columns:
        raise ValueError("the product table must have 'sku'")
    n = int(text.n)
    if len(products) != n:
        raise ValueError(f"{len(products)} products for the text of {n}")
    if encoder.tokenizer is None:
        raise ValueError("no vocabulary was loaded: the builder tokenises text")
    model = encoder.model
    if n and int(text.device) != int(model.device):
        raise ValueError(f"the text lives on GPU {text.device}, the encoder on GPU {model.device}")
    if not 1 <= int(head_bytes) < 2 ** 31:
        raise ValueError("head_bytes must lie in [1, 2^31): the tokenizer's offsets per call are below 2^31")
    if n == 0:
        raise RuntimeError("No products left after filtering.")
    dev = torch.device("cuda", model.device)
    tp = T.TextPrep(model.device)
    try:
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            st_ptr = main.cuda_stream
            p_text = text.d_text.data_ptr() if text.text_bytes else None
            d_len = torch.empty(n, dtype=torch.int32, device=dev)
            d_st = torch.empty(n, dtype=torch.int32, device=dev)
            tp.head_measure(p_text, text.text_bytes, text.d_off.data_ptr(), n, None, n, MAX_TEXT_LEN, True, MIN_TEXT_LEN,
                            d_len.data_ptr(), d_st.data_ptr(), st_ptr)
            lens, status = d_len.cpu().numpy().astype(np.int64), d_st.cpu().numpy()
            tp.check()
            lap("measure_heads")

            host_clean = np.flatnonzero(status & T.NEEDS_HOST)
            cleaned: Dict[int, bytes] = {}
            if len(host_clean):
                off = text.d_off.cpu().numpy()
                for i in host_clean.tolist():
                    raw = text.d_text[int(off[i]):int(off[i + 1])].cpu().numpy().tobytes()
                    t = normalize_text(raw.decode("utf-8", "surrogatepass"))
                    cleaned[i] = t.encode("utf-8", "surrogatepass")
                    lens[i] = len(cleaned[i])
                    status[i] = T.SHORT if len(t) < MIN_TEXT_LEN else 0
            kept = np.flatnonzero(status == 0)
            if stats is not None:
                stats.update(host_clean_docs=host_clean.tolist(), host_docs=[])
            if len(kept) == 0:
                raise RuntimeError("No products left after filtering.")
            lo, hi = (0, len(kept)) if rows is None else (int(rows[0]), int(rows[1]))
            if not (0 <= lo < hi <= len(kept)):
                raise ValueError(f"rows=({lo}, {hi}) outside the {len(kept)} products left after filtering")
            kept = kept[lo:hi]
            m = len(kept)
            lens_k = lens[kept]
            lap("host_clean")

            index = ProductIndex(None, n_rows=m, dim=model.hidden, device=model.device, row_offset=lo, dtype=dtype)
            keep_rows = data_dir is not None and dtype != "f32"
            emb_parts: List[np.ndarray] = []
            host_docs: List[int] = []
            d_kept = torch.from_numpy(kept.astype(np.int32)).to(dev)
            d_len_k, d_st_k = d_len[d_kept.long()], d_st[d_kept.long()]      # (the device's own status: a host-cleaned row writes nothing)
            ends = np.cumsum(lens_k)
            d_heads = None
            r0 = 0
            while r0 < m:
                before = int(ends[r0 - 1]) if r0 else 0
                r1 = max(r0 + 1, int(np.searchsorted(ends, before + int(head_bytes), side="right")))
                nb = r1 - r0
                boff = np.zeros(nb + 1, dtype=np.int64)
                np.cumsum(lens_k[r0:r1], out=boff[1:])
                nbytes = int(boff[-1])
                if nbytes >= 2 ** 31:
                    raise ValueError(f"the head of product row {int(kept[r0])} alone has {nbytes} bytes")
                if d_heads is None or d_heads.numel() < nbytes + 16:
                    d_heads = None
                    d_heads = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
                d_boff = torch.from_numpy(boff).to(dev)
                tp.head_write(p_text, text.text_bytes, text.d_off.data_ptr(), n, d_kept.data_ptr() + 4 * r0, nb, MAX_TEXT_LEN, True,
                              MIN_TEXT_LEN, d_len_k.data_ptr() + 4 * r0, d_st_k.data_ptr() + 4 * r0, d_heads.data_ptr(), nbytes,
                              d_boff.data_ptr(), st_ptr)
                mine = [j for j in range(nb) if int(kept[r0 + j]) in cleaned]
                _write_host_rows(d_heads, boff, mine, [cleaned[int(kept[r0 + j])] for j in mine])
                tp.check()                            # (waits: the tokenizer's stream reads what this one wrote)
                lap("write_heads")

                def queue_docs(wp, a, b, L, cap):
                    return wp.queue_dev(d_heads.data_ptr() + int(boff[a]), int(boff[b] - boff[a]), d_boff[a:b + 1] - int(boff[a]), L, cap)

                def host_text(i):
                    return d_heads[int(boff[i]):int(boff[i + 1])].cpu().numpy().tobytes().decode("utf-8", "surrogatepass")

                blk: dict = {}
                part = _embed_into(index, lens_k[r0:r1].tolist(), queue_docs, host_text, encoder, first_row=r0,
                                   chunk_tokens=chunk_tokens, keep_rows=keep_rows, stats=blk)
                host_docs += [r0 + i for i in blk["host_docs"]]
                if keep_rows:
                    emb_parts.append(part)
                lap("tokenize_encode_store")
                r0 = r1
            if stats is not None:
                stats["host_docs"] = host_docs
    finally:
        tp.close()

    meta = pd.DataFrame({"sku": products["sku"].values[kept]})
    for c in ("n_reviews", "avg_stars", "last_ts"):
        meta[c] = products[c].values[kept] if c in products.columns else np.nan
    emb = np.concatenate(emb_parts) if emb_parts else None
    if data_dir is not None:
        from .artifacts import save_artifacts
        agg = text.agg_text()
        meta["agg_text"] = np.asarray([agg[int(i)] for i in kept], dtype=object)
        if emb is None:
            emb = index.download_rows(0, index.n_rows)
        save_artifacts(data_dir, meta, emb)
        lap("write_files")
    return index, meta, emb, kept


def prepare_reviews(reviews):
    """nlp/11_build_product_embeddings.py:99-108: the five columns, id / sku / text as str, stars numeric, ts a UTC time."""
    import pandas as pd
    miss = {"id", "sku", "text"} - set(reviews.columns)
    if miss:
        raise ValueError(f"review table missing {sorted(miss)}")
    miss = {"ts", "stars"} - set(reviews.columns)
    if miss:                                      # (the reference dies on these with a KeyError)
        raise ValueError(f"review table missing {sorted(miss)}")
    df = reviews[list(REVIEW_COLUMNS)].copy()
    df["id"] = df["id"].astype(str)
    df["sku"] = df["sku"].astype(str)
    df["text"] = df["text"].fillna("").astype(str)
    df["stars"] = pd.to_numeric(df["stars"], errors="coerce")
    df["ts"] = pd.to_datetime(df["ts"], utc=True, errors="coerce")
    return df


def _utf8_column(texts) -> Tuple[np.ndarray, np.ndarray]:
    """(bytes, int64 offsets [n + 1]) of a column of str, without a Python loop where every row has a UTF-8 form."""
    import pyarrow as pa
    try:
        arr = pa.array(texts, type=pa.large_string())
        _, off, data = arr.buffers()
        off = np.frombuffer(off, dtype=np.int64)[arr.offset:arr.offset + len(arr) + 1]
        raw = np.frombuffer(data, dtype=np.uint8) if data is not None else np.zeros(0, dtype=np.uint8)
        return raw, off
    except (pa.ArrowInvalid, UnicodeEncodeError):  # a lone surrogate: three bytes the kernel calls malformed, so the host cleans the row
        docs = [t.encode("utf-8", "surrogatepass") for t in texts]
        off = np.zeros(len(docs) + 1, dtype=np.int64)
        np.cumsum([len(d) for d in docs], out=off[1:])
        return np.frombuffer(b"".join(docs), dtype=np.uint8), off


def _stage_rows(raw: np.ndarray, off: np.ndarray, d_text, main, stage_bytes: int, on_rows) -> None:
    """The text column `raw` (rows at `off`, int64 [n + 1]) copied to `d_text` on stream `main` in row blocks of about
    `stage_bytes` through two pinned buffers (a longer row goes through in pieces); on_rows(a, b) is called once rows
    [a, b) are queued, to queue what reads them.  Does not wait for the last block."""
    import torch
    n, total = len(off) - 1, int(off[-1])
    blk = max(1, min(int(stage_bytes), max(total, 1)))
    stage = [torch.empty(blk, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    busy: List[Optional[object]] = [None, None]
    turn = 0
    a = 0
    while a < n:
        b = int(np.searchsorted(off, off[a] + blk, side="right")) - 1
        b = min(n, max(b, a + 1))
        for lo in range(int(off[a]), int(off[b]), blk):
            hi = min(int(off[b]), lo + blk)
            if busy[turn] is not None:
                busy[turn].synchronize()
            stage[turn].numpy()[:hi - lo] = raw[lo:hi]
            d_text[lo:hi].copy_(stage[turn][:hi - lo], non_blocking=True)
            busy[turn] = torch.cuda.Event()
            busy[turn].record(main)
            turn ^= 1
        on_rows(a, b)
        a = b


def _write_host_rows(d_text, off: np.ndarray, rows, cleaned) -> None:
    """The texts `cleaned` (bytes, each no longer than its raw text) written into the slots of `rows` of `d_text`: two
    copies and one scatter, not a copy per row."""
    import torch
    parts = [np.frombuffer(t, dtype=np.uint8) for t in cleaned]
    for i, tb in zip(rows, parts):
        assert len(tb) <= off[i + 1] - off[i]
    if parts and sum(len(x) for x in parts):
        where = [np.arange(int(off[i]), int(off[i]) + len(tb), dtype=np.int64) for i, tb in zip(rows, parts)]
        d_text.index_copy_(0, torch.from_numpy(np.concatenate(where)).to(d_text.device),
                           torch.from_numpy(np.concatenate(parts)).to(d_text.device))


def build_review_embeddings(reviews, encoder, *, no_spam: bool = False, no_dedup: bool = False, chunk_tokens: int = 131072,
                            data_dir=None, product_skus=None, stats: Optional[dict] = None, max_text_bytes: int = MAX_TEXT_BYTES,
                            stage_bytes: int = STAGE_BYTES, log=None):
    """nlp/11_build_product_embeddings.py:99-165 on the GPU -> (table, emb, ReviewIndex or None).

    table = the surviving rows of id, sku, ts, stars, text (the RAW text) in file order, emb = their float32 (m, hidden) rows (hidden = the encoder's width),
    l2-normalised with eps 1e-12.  The raw text goes to the device in row blocks through two pinned buffers of `stage_bytes`;
    rr_textprep_clean_dev normalises it in place and answers a length and a status word per row; the rows it flags
    (textprep.model_clean says which) are cleaned by `normalize_text` / `looks_spammy` here and written into their slots
    (a normalised text is never longer than its raw text); rr_textprep_dedup_dev marks duplicates per sku; the survivors are
    compacted on the device and tokenised, encoded and stored from there, chunk by chunk (`_embed_into`).
    The cleaned text of the WHOLE table stays on the device until it is encoded, because dedup must see all of it:
    more than `max_text_bytes` (default 8 GiB) of raw text is refused.  With `product_skus` the rows become a ReviewIndex
    without leaving the device (rr_reviews_create_dev); with `data_dir`, reviews_with_embeddings.parquet is written there.
    stats receives "short", "spam", "duplicate" (rows dropped, counted as the reference logs them), "host_clean_docs" and
    "host_docs" (table rows the clean stage / survivors the tokenizer left to the host) and "seconds", the wall clock of the
    phases (each ends at a point where the host waits for the device anyway).  log: a callable that receives the
    reference's `[review] ...` lines where the reference prints them (the counts before the encoding starts)."""
    import time
    import pandas as pd
    import torch
    from . import textprep as T
    seconds: Dict[str, float] = {}
    clock = [time.perf_counter()]

    def lap(name):
        now = time.perf_counter()
        seconds[name] = seconds.get(name, 0.0) + now - clock[0]
        clock[0] = now

    if stats is not None:
        stats["seconds"] = seconds
    df = prepare_reviews(reviews)
    n = len(df)
    if n == 0:
        raise RuntimeError("No reviews left after filtering.")
    texts = df["text"].tolist()
    lap("prepare_columns")
    raw, off = _utf8_column(texts)
    total = int(off[-1])
    lap("utf8_bytes")
    if total > int(max_text_bytes):
        raise ValueError(f"{total:,} bytes of review text exceed max_text_bytes = {int(max_text_bytes):,}: the cleaned text of the "
                         "whole table stays on the device until it is encoded.  Split the table by sku and build the parts one "
                         "after the other: duplicates are dropped per sku, so the result is the same.")
    if encoder.tokenizer is None:
        raise ValueError("no vocabulary was loaded: the builder tokenises text")
    model, L = encoder.model, encoder.max_length
    dev = torch.device("cuda", model.device)
    tp = T.TextPrep(model.device)
    try:
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            st_ptr = main.cuda_stream
            d_text = torch.empty(total + 16, dtype=torch.uint8, device=dev)
            d_off = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
            d_len = torch.empty(n, dtype=torch.int32, device=dev)
            d_st = torch.empty(n, dtype=torch.int32, device=dev)
            _stage_rows(raw, off, d_text, main, stage_bytes,
                        lambda a, b: tp.clean(d_text.data_ptr(), total, d_off.data_ptr() + 8 * a, b - a, not no_spam, d_text.data_ptr(),
                                              d_len.data_ptr() + 4 * a, d_st.data_ptr() + 4 * a, st_ptr))
            main.synchronize()
            tp.check()
            status, lens = d_st.cpu().numpy(), d_len.cpu().numpy()
            lap("copy_and_clean")

            # the rows the kernel left to the host: the reference's own functions, into the rows' slots
            host_clean = np.flatnonzero(status & T.NEEDS_HOST)
            cleaned = []
            for i in host_clean.tolist():
                t = normalize_text(texts[i])
                tb = t.encode("utf-8", "surrogatepass")
                cleaned.append(tb)
                lens[i] = len(tb)
                status[i] = (T.SHORT if len(t) < MIN_TEXT_LEN else 0) | (T.SPAM if not no_spam and looks_spammy(t) else 0)
            _write_host_rows(d_text, off, host_clean.tolist(), cleaned)
            if len(host_clean):
                d_len.copy_(torch.from_numpy(lens))
                d_st.copy_(torch.from_numpy(status))
            n_short = int(np.count_nonzero(status & T.SHORT))
            n_spam = int(np.count_nonzero((status & (T.SHORT | T.SPAM)) == T.SPAM))
            lap("host_clean")

            if not no_dedup:
                group = torch.from_numpy(pd.factorize(df["sku"])[0].astype(np.int32)).to(dev)
                tp.dedup(d_text.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), group.data_ptr(), d_st.data_ptr(), n, 64, st_ptr)
                status = d_st.cpu().numpy()
                lap("dedup")
            keep = np.flatnonzero(status == 0)
            m = len(keep)
            n_dup = int(np.count_nonzero(status & T.DUP))
            if log is not None:                       # nlp/11...:115,118,124
                if not no_spam:
                    log(f"[review] spam filtered {n_spam:,} rows")
                if not no_dedup:
                    log(f"[review] dedup removed {n_dup:,}")
            if stats is not None:
                stats.update(short=n_short, spam=n_spam, duplicate=n_dup, host_clean_docs=host_clean.tolist(), host_docs=[])
            if m == 0:
                raise RuntimeError("No reviews left after filtering.")

            if log is not None:
                log(f"[review] rows={m:,}  chunk_tokens={int(chunk_tokens):,}")
            lens_k = lens[keep].astype(np.int64)
            coff = np.zeros(m + 1, dtype=np.int64)
            np.cumsum(lens_k, out=coff[1:])
            cbytes = int(coff[-1])
            d_ctext = torch.empty(cbytes + 16, dtype=torch.uint8, device=dev)
            d_coff = torch.empty(n + 1, dtype=torch.int64, device=dev)
            d_src = torch.empty(n, dtype=torch.int32, device=dev)
            d_count = torch.empty(2, dtype=torch.int64, device=dev)
            tp.compact(d_text.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), n, d_ctext.data_ptr(), cbytes,
                       d_coff.data_ptr(), d_src.data_ptr(), d_count.data_ptr(), st_ptr)
            count = d_count.cpu().numpy()             # (waits: the tokenizer's stream reads what this one wrote)
            tp.check()
            if int(count[0]) != m or int(count[1]) != cbytes:
                raise _lib.HipLibraryError(f"compaction kept {count.tolist()}, the host counts {[m, cbytes]}")
            del d_text
            lap("compact")

            def queue_docs(wp, a, b, L, cap):
                return wp.queue_dev(d_ctext.data_ptr() + int(coff[a]), int(coff[b] - coff[a]), d_coff[a:b + 1] - int(coff[a]), L, cap)

            index = ProductIndex(None, n_rows=m, dim=model.hidden, device=model.device)
            tok_stats: dict = {}
            _embed_into(index, lens_k.tolist(), queue_docs, lambda i: normalize_text(texts[int(keep[i])]), encoder, first_row=0,
                        chunk_tokens=chunk_tokens, keep_rows=False, stats=tok_stats)
            if stats is not None:
                stats["host_docs"] = tok_stats["host_docs"]
            lap("tokenize_encode_store")
            table = df.iloc[keep].reset_index(drop=True)
            emb = index.download_rows(0, m)
            review_index = None
            if product_skus is not None:
                from .reviews import ReviewIndex
                d_rows = torch.empty((m, model.hidden), dtype=torch.float32, device=dev)
                _lib.check(_lib.load().rr_index_copy_rows_dev(index.handle, 0, m, C.c_void_p(d_rows.data_ptr()), C.c_void_p(st_ptr)),
                           "rr_index_copy_rows_dev")
                review_index = ReviewIndex.from_device_rows(table, d_rows, product_skus, device=model.device)
            index.close()
    finally:
        tp.close()
    lap("table_and_rows")
    if data_dir is not None:
        from .artifacts import save_reviews
        save_reviews(data_dir, table, emb)
        lap("write_file")
    return table, emb, review_index


# ---------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m review_recommender_amd.embed",
                                 description="Build product or review embeddings on the GPU (nlp/11_build_product_embeddings.py's flags).")
    ap.add_argument("--target", choices=["product", "review"], required=True)
    ap.add_argument("--input", type=str, default="", help=f"default: {PRODUCT_INPUT} (product), {REVIEW_INPUT} (review)")
    ap.add_argument("--reviews", type=str, default="",
                    help="product target only: build from reviews_merged.parquet instead of --input -- products.load_reviews, "
                         "build_products with agg_text kept on the device, build_product_embeddings_device; writes the same "
                         "two files.  Not together with --input")
    ap.add_argument("--text-col", type=str, default="")
    ap.add_argument("--model", type=str, required=True, help="LOCAL model directory (weights + vocab.txt); nothing is fetched")
    ap.add_argument("--device", type=str, default="0", help="GPU ordinal (0, cuda:0)")
    ap.add_argument("--batch", type=int, default=256, help="documents per chunk at 512 tokens each (chunk = batch x 512 tokens)")
    ap.add_argument("--shard-rows", type=int, default=20000,
                    help="accepted for compatibility with the reference's command line and ignored: the build is chunked by "
                         "tokens (--batch), not by rows")
    ap.add_argument("--out-dir", type=str, default="data/processed")
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32", help="encoder arithmetic")
    ap.add_argument("--pooling", choices=["auto", "cls", "mean"], default="auto",
                    help="the sentence vector: auto = what the model directory's 1_Pooling/config.json says (cls without one; "
                         "any pooling but cls / mean is refused), cls = last_hidden_state[:, 0], mean = the mean over the tokens")
    # review-only options
    ap.add_argument("--no-spam", action="store_true", help="disable spam filter")
    ap.add_argument("--no-dedup", action="store_true", help="disable (sku,text) dedup")
    ap.add_argument("--resume", action="store_true",
                    help="refused (exit status 2): the reference's resume reopens the output with a fresh writer and so "
                         "truncates the rows it claims to keep; reproducing that would lose data")
    args = ap.parse_args(argv)
    if args.reviews and args.input:
        ap.error("--input and --reviews exclude each other: the product table is either read or built")
    if args.reviews and args.target != "product":
        ap.error("--reviews belongs to --target product (review embeddings read the review table with --input)")
    return args


def _main_product_from_reviews(args) -> int:
    from . import products as P
    from .cross_encoder import QueryEncoder
    device = int(str(args.device).split(":")[-1])
    reviews = P.load_reviews(args.reviews)
    products, _, text = P.build_products(reviews, device=device, keep_device=True)
    encoder = QueryEncoder.from_pretrained_dir(args.model, device=device, precision=args.precision, pooling=args.pooling)
    index, meta, emb, _ = build_product_embeddings_device(products, text, encoder, chunk_tokens=max(1, args.batch) * 512,
                                                          data_dir=args.out_dir)
    print(f"[product] rows={len(meta):,}  batch={args.batch}", flush=True)
    print(f"[ok] wrote {args.out_dir}/product_emb.npy shape={emb.shape}", flush=True)
    print(f"[ok] wrote {args.out_dir}/product_emb_meta.parquet rows={len(meta):,}", flush=True)
    return 0


def main(argv=None) -> int:
    args = parse_args(argv)
    if args.target == "review":
        return _main_review(args)
    if args.reviews:
        return _main_product_from_reviews(args)
    import pandas as pd
    from .cross_encoder import QueryEncoder
    df = pd.read_parquet(args.input or PRODUCT_INPUT)
    text_col = args.text_col or ("agg_text" if "agg_text" in df.columns else None)
    if not text_col:
        raise ValueError("Provide --text-col for product text (e.g., agg_text).")
    device = int(str(args.device).split(":")[-1])
    encoder = QueryEncoder.from_pretrained_dir(args.model, device=device, precision=args.precision, pooling=args.pooling)
    index, meta, emb = build_product_embeddings(df, encoder, text_col=text_col, chunk_tokens=max(1, args.batch) * 512,
                                                data_dir=args.out_dir)
    print(f"[product] rows={len(meta):,}  batch={args.batch}", flush=True)
    print(f"[ok] wrote {args.out_dir}/product_emb.npy shape={emb.shape}", flush=True)
    print(f"[ok] wrote {args.out_dir}/product_emb_meta.parquet rows={len(meta):,}", flush=True)
    return 0


def _main_review(args) -> int:
    import pandas as pd
    from .artifacts import REVIEWS_FILE
    from .cross_encoder import QueryEncoder
    if args.resume:
        print(RESUME_REFUSED, file=sys.stderr)
        return 2
    src = args.input or REVIEW_INPUT
    df = pd.read_parquet(src)
    try:
        prepare_reviews(df.iloc[:0])
    except ValueError as e:                     # e.g. a product table: say so instead of a traceback
        print(f"{src} {str(e).split('review table ', 1)[-1]}: review embeddings are not built here from a table without "
              "id, sku, ts, stars and text", file=sys.stderr)
        return 2
    device = int(str(args.device).split(":")[-1])
    encoder = QueryEncoder.from_pretrained_dir(args.model, device=device, precision=args.precision, pooling=args.pooling)
    table, emb, _ = build_review_embeddings(df, encoder, no_spam=args.no_spam, no_dedup=args.no_dedup,
                                            chunk_tokens=max(1, args.batch) * 512, data_dir=args.out_dir,
                                            log=lambda line: print(line, flush=True))
    print(f"[ok] wrote {args.out_dir}/{REVIEWS_FILE} total rows={len(table):,}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
