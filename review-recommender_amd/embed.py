"""Product embeddings built on the GPU: text in, searchable index (and the reference's files) out.

Stands in for nlp/11_build_product_embeddings.py:46-92 (`SentenceTransformer.encode(texts, normalize_embeddings=True)`
over `normalize_text(agg_text)`), the builder of product_emb.npy / product_emb_meta.parquet.  Per chunk of documents:

    UTF-8 bytes + offsets in pinned memory -> one copy to the device
    rr_wp_encode_dev          WordPiece ids, packed            (csrc/rr_wordpiece.hip, on a stream of its own)
    rr_ce_forward_dev         12 layers, CLS rows              (csrc/rr_ce.hip)
    rr_index_store_rows_dev   x / max(||x||, 1e-12) into the index's rows

with no host hop between the three: the host reads back two integers per chunk (tokens, longest sequence: what the forward
call takes as arguments) and the needs_host flags, and prepares chunk i + 1 while chunk i runs.  The tokenizer is the UTF-8
kernel (Unicode text through the table of wp_unicode.py); the few documents it flags (a hard code point, a mapped text beyond
its buffers: wp_unicode.model_tokenize) are tokenised by wordpiece.py and encoded in one small pass at the end, scattered into
their rows.  RR_WP_ASCII=1 in the environment restores the ASCII kernel, which flags every document with a byte >= 0x80.  Review embeddings
(nlp/11...:95-169) are not built here.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .cross_encoder import HIDDEN, OUT_CLS
from .index import ProductIndex
from .wordpiece import WordPieceTokenizer

MIN_TEXT_LEN = 10       # nlp/11_build_product_embeddings.py:22-23
MAX_TEXT_LEN = 4000
NORMALIZE_EPS = 1e-12   # torch.nn.functional.normalize's eps (normalize_embeddings=True)
META_COLUMNS = ("sku", "n_reviews", "avg_stars", "last_ts", "agg_text")     # nlp/11...:86-89
_WS = re.compile(r"\s+")


def normalize_text(s) -> str:
    """nlp/11_build_product_embeddings.py:32-36."""
    if not isinstance(s, str):
        s = "" if s is None else str(s)
    s = s.replace("\r", " ").replace("\n", " ").strip()
    s = _WS.sub(" ", s)
    return s[:MAX_TEXT_LEN]


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
    """(bytes, offsets) of rr_wp_create: piece i = the vocabulary string with id i, empty where no string has that id."""
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


def build_piece_table(vocab: Dict[str, int], max_chars_per_word: int = 100, unicode: bool = False):
    """The open-addressing table the device matches against, built by the library ON THE HOST (rr_wp_build_table; no GPU
    needed): (slots [n_slots][4] int32 = hash, first byte, length in bytes | ## form << 16, id or -1; piece bytes; pieces
    kept).  unicode=True: the table of a UTF-8 handle (rr_wp_build_table_utf8), which keeps pieces with bytes >= 0x80 and
    counts max_chars_per_word in code points."""
    lib = _lib.load()
    blob, off = piece_arrays(vocab)
    n_slots, kept = C.c_int32(), C.c_int32()
    _lib.check(lib.rr_wp_table_slots(len(off) - 1, C.byref(n_slots)), "rr_wp_table_slots")
    slots = np.empty((n_slots.value, 4), dtype=np.int32)
    fn, name = (lib.rr_wp_build_table_utf8, "rr_wp_build_table_utf8") if unicode else (lib.rr_wp_build_table, "rr_wp_build_table")
    _lib.check(fn(_lib.ptr(blob), _lib.ptr(off), len(off) - 1, max_chars_per_word, n_slots.value, _lib.ptr(slots), C.byref(kept)),
               name)
    return slots, blob, kept.value


class DeviceWordPiece:
    """`WordPieceTokenizer` for single texts on one GPU (csrc/rr_wordpiece.hip).  unicode=False: the ASCII kernel, which leaves
    every document with a byte >= 0x80 to the host.  unicode=True: the UTF-8 kernel over the per-code-point table of
    wp_unicode.unicode_tables(); it leaves to the host only what wp_unicode.model_tokenize flags."""

    def __init__(self, tokenizer: WordPieceTokenizer, device: int = 0, unicode: bool = False):
        if not tokenizer.do_lower_case:
            raise ValueError("the device tokenizer lower-cases (uncased vocabularies); this tokenizer does not")
        import torch
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the device tokenizer runs on the device only")
        self._torch, self.tokenizer, self.device, self.unicode = torch, tokenizer, device, bool(unicode)
        self._dev = torch.device("cuda", device)
        blob, off = piece_arrays(tokenizer.vocab)
        h = C.c_void_p()
        if unicode:
            from .wp_unicode import unicode_tables
            t = unicode_tables()
            st1, st2, pool = t["stage1"], t["stage2"], t["pool"]
            _lib.check(_lib.load().rr_wp_create_utf8(device, _lib.ptr(blob), _lib.ptr(off), len(off) - 1, tokenizer.unk_id,
                                                     tokenizer.cls_id, tokenizer.sep_id, tokenizer.max_chars_per_word,
                                                     _lib.ptr(st1), len(st1), _lib.ptr(st2), len(st2), _lib.ptr(pool), len(pool),
                                                     C.byref(h)), "rr_wp_create_utf8")
        else:
            _lib.check(_lib.load().rr_wp_create(device, _lib.ptr(blob), _lib.ptr(off), len(off) - 1, tokenizer.unk_id,
                                                tokenizer.cls_id, tokenizer.sep_id, tokenizer.max_chars_per_word, C.byref(h)),
                       "rr_wp_create")
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
        cap = int(capacity) if capacity else n * int(max_length)
        stage = torch.empty(8 * (n + 1) + nbytes + 8, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        host[:8 * (n + 1)] = off.view(np.uint8)
        host[8 * (n + 1):8 * (n + 1) + nbytes] = np.frombuffer(b"".join(docs), dtype=np.uint8)
        with torch.cuda.device(self._dev):
            d_in = stage.to(self._dev, non_blocking=True)
            packed = torch.empty(3 * cap + 2 * n + 2, dtype=torch.int32, device=self._dev)
            base, st = packed.data_ptr(), torch.cuda.current_stream(self._dev).cuda_stream
            _lib.check(_lib.load().rr_wp_encode_dev(
                self._h, C.c_void_p(d_in.data_ptr() + 8 * (n + 1)), nbytes, C.c_void_p(d_in.data_ptr()), n, int(max_length), cap,
                C.c_void_p(base), C.c_void_p(base + 4 * cap), C.c_void_p(base + 8 * cap), C.c_void_p(base + 12 * cap),
                C.c_void_p(base + 4 * (3 * cap + n + 1)), C.c_void_p(base + 4 * (3 * cap + 2 * n + 1)), C.c_void_p(st)),
                "rr_wp_encode_dev")
            info = torch.empty(n + 2, dtype=torch.int32, pin_memory=True)
            info.copy_(packed[3 * cap + n:], non_blocking=True)
        return packed, info, n, cap, (stage, d_in)

    @staticmethod
    def views(packed, n: int, cap: int, total: int):
        """(tok, typ, pos, cu) views of `packed` once the host knows `total` = cu[n]."""
        return (packed[:total], packed[cap:cap + total], packed[2 * cap:2 * cap + total], packed[3 * cap:3 * cap + n + 1])

    def encode_dev(self, texts: Sequence[str], max_length: int):
        """The packed device tensors of `texts` (what `forward_packed_dev` takes) and the documents left to the host:
        (tok, typ, pos, cu_seqlens, max_len, needs_host) -- int32 device tensors, the longest sequence, and the indices of
        the documents that were NOT tokenised (ASCII handle: a byte >= 0x80; UTF-8 handle: malformed UTF-8, a hard code point
        or a mapped text beyond the buffers; both: longer than the kernel's window and not answerable from it): their sequences are the placeholder [CLS] [SEP].  Waits for the result (the sizes are host integers)."""
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
    import torch
    if encoder.tokenizer is None:
        raise ValueError("no vocabulary was loaded: the builder tokenises text")
    n = len(texts)
    if first_row < 0 or first_row + n > index.n_rows or index.dim != HIDDEN:
        raise ValueError(f"{n} rows of dim {HIDDEN} from row {first_row} do not fit an index of {index.n_rows} x {index.dim}")
    model, L = encoder.model, encoder.max_length
    dev = torch.device("cuda", model.device)
    wp = getattr(encoder, "_device_wp", None)
    if wp is None:
        wp = encoder._device_wp = DeviceWordPiece(encoder.tokenizer, model.device,
                                                  unicode=os.environ.get("RR_WP_ASCII") != "1")
    lib = _lib.load()
    kept = np.empty((n, HIDDEN), dtype=np.float32) if keep_rows else None
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
                scratch[0] = ProductIndex(None, n_rows=max(out.shape[0], 256), dim=HIDDEN, device=model.device)
            _lib.check(lib.rr_index_store_rows_dev(scratch[0].handle, C.c_void_p(out.data_ptr()), out.shape[0], 0, None,
                                                   NORMALIZE_EPS, C.c_void_p(main.cuda_stream)), "rr_index_store_rows_dev")
            kept[where] = scratch[0].download_rows(0, out.shape[0])

        def queue_tok(a, b):
            # On the side stream, with no wait for `main`: the buffers are allocated while `side` is current, so the
            # allocator hands out blocks of the side stream's own pool (record_stream below covers their use on `main`),
            # and the tokenizer's scratch is only ever touched on `side`.  The copy and the kernels of chunk i + 1 so run
            # while chunk i's layers do.
            docs = [t.encode("utf-8") for t in texts[a:b]]
            with torch.cuda.stream(side):
                q = wp.queue(docs, L, max(chunk_tokens, L, 2 * (b - a)))
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
            out = model.forward_packed_dev(tok, typ, pos, cu, nd, int(h[nd + 1]), OUT_CLS)
            store(out, first_row + a)
            flag = None
            if narrow:                      # an out-of-range pass leaves NaN in every CLS row of its call (include/rr_hip.h)
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

        lens = [len(t.encode("utf-8")) for t in texts] if n else []
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

        # the documents the device left to the host (wp_unicode.model_tokenize's reasons; with RR_WP_ASCII=1 every byte
        # >= 0x80): one small pass, scattered into their rows
        at = 0
        while at < len(host_docs):
            part, tot = [], 0
            while at < len(host_docs) and (not part or tot + L <= chunk_tokens):
                part.append(host_docs[at])
                tot += L
                at += 1
            seqs = [encoder.tokenizer.encode_pair(texts[i], None, L) for i in part]
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
            args = (d[:T], d[T:2 * T], d[2 * T:3 * T], d[3 * T:], len(part), int(sl.max()), OUT_CLS)
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
    index = ProductIndex(None, n_rows=hi - lo, dim=HIDDEN, device=encoder.model.device, row_offset=lo, dtype=dtype)
    emb = embed_texts_into(index, texts, encoder, chunk_tokens=chunk_tokens,
                           keep_rows=data_dir is not None and dtype != "f32", stats=stats)
    if data_dir is not None:
        from .artifacts import save_artifacts
        if emb is None:
            emb = index.download_rows(0, index.n_rows)
        save_artifacts(data_dir, meta, emb)
    return index, meta, emb


# ---------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m review_recommender_amd.embed",
                                 description="Build product embeddings on the GPU (nlp/11_build_product_embeddings.py's flags).")
    ap.add_argument("--target", choices=["product", "review"], required=True)
    ap.add_argument("--input", type=str, default="data/processed/products.parquet")
    ap.add_argument("--text-col", type=str, default="")
    ap.add_argument("--model", type=str, required=True, help="LOCAL model directory (weights + vocab.txt); nothing is fetched")
    ap.add_argument("--device", type=str, default="0", help="GPU ordinal (0, cuda:0)")
    ap.add_argument("--batch", type=int, default=256, help="documents per chunk at 512 tokens each (chunk = batch x 512 tokens)")
    ap.add_argument("--shard-rows", type=int, default=20000,
                    help="accepted for compatibility with the reference's command line and ignored: the build is chunked by "
                         "tokens (--batch), not by rows")
    ap.add_argument("--out-dir", type=str, default="data/processed")
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32", help="encoder arithmetic")
    return ap.parse_args(argv)


def main(argv=None) -> int:
    args = parse_args(argv)
    if args.target == "review":
        print("review embeddings are not built here (product embeddings only)", file=sys.stderr)
        return 2
    import pandas as pd
    from .cross_encoder import QueryEncoder
    df = pd.read_parquet(args.input)
    text_col = args.text_col or ("agg_text" if "agg_text" in df.columns else None)
    if not text_col:
        raise ValueError("Provide --text-col for product text (e.g., agg_text).")
    device = int(str(args.device).split(":")[-1])
    encoder = QueryEncoder.from_pretrained_dir(args.model, device=device, precision=args.precision)
    index, meta, emb = build_product_embeddings(df, encoder, text_col=text_col, chunk_tokens=max(1, args.batch) * 512,
                                                data_dir=args.out_dir)
    print(f"[product] rows={len(meta):,}  batch={args.batch}", flush=True)
    print(f"[ok] wrote {args.out_dir}/product_emb.npy shape={emb.shape}", flush=True)
    print(f"[ok] wrote {args.out_dir}/product_emb_meta.parquet rows={len(meta):,}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
