"""The reranker's pairs on the GPU (csrc/rr_pairs.hip), and the plane's and the two kernels' model on the CPU.

Stands in for what `CrossEncoder.predict` does in front of the model as run_search calls it (app/app_product_search.py:272-278,
app/test.py:223-225): the pairs ``(query, agg_text[:2000])`` through the model's BertTokenizer, `[CLS] query [SEP] text [SEP]`
truncated `longest_first` to ``max_length``.

`RerankText` is the token plane of an index on the device: per product the WordPiece ids of ``agg_text[:2000]`` -- the cut is
in code points and is made BEFORE tokenising, so a word cut in half is tokenised as the half -- of which the first
``max_length - 3`` are kept (no longer text side survives the truncation), uint16, back to back.  It is tokenised once per
index (embed.DeviceWordPiece; what that hands back, by wordpiece.py), from a column of str (`from_texts`) or from agg_text
already on the device (`from_device`, over the raw heads of csrc/rr_textprep.hip); per batch `RerankText.scores` assembles the packed
sequences of the candidates on the device (rr_pairs_measure_dev / rr_pairs_write_dev), runs `forward_packed_dev` on them and
leaves the scores on the device.  `pack_queries` turns a batch's query ids into the arrays the kernels read.  `model_plane` /
`model_pairs` state in numpy what the plane and the two kernels hold, as gate.model_gate_plane / model_gate_hits do for theirs.

The plane holds ``min(n_b, avail)`` text tokens, ``avail = max_length - 3``, not ``n_b``.  `keep_lengths` (the rule of
`WordPieceTokenizer.encode_pair`) answers the same for both whenever the query has ``n_a <= avail`` tokens
(tests/test_rerank_model.py sweeps it) and differs for some longer queries: those are `PackedQueries.host_queries`, scored
through the host `predict`.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

MAX_CHARS = 2000            # app/app_product_search.py:276, app/test.py:224: agg_text[:2000]
MAX_VOCAB = 1 << 16         # the plane's ids are uint16
CHUNK_DOCS = 8192           # documents per call of the device tokenizer while the plane is built
STAGE_BYTES = 64 << 20


# ---------------------------------------------------------------------------------- the models
def keep_lengths(n_a: int, n_b: int, max_length: int) -> Tuple[int, int]:
    """(query tokens, text tokens) a pair keeps: `longest_first` as `WordPieceTokenizer.encode_pair` states it."""
    avail = max(int(max_length) - 3, 0)
    if n_a + n_b > avail:
        swap = n_a > n_b                           # (a tie: the text is the longer side)
        n1, n2 = (n_b, n_a) if swap else (n_a, n_b)
        n2 = n1 if n1 > avail else max(n1, avail - n1)
        if n1 + n2 > avail:
            n1 = avail // 2
            n2 = n1 + avail % 2
        n_a, n_b = (n2, n1) if swap else (n1, n2)
    return n_a, n_b


def model_plane(texts: Sequence[str], tokenizer, max_length: int, max_chars: int = MAX_CHARS) -> List[np.ndarray]:
    """What `RerankText.from_texts` holds per document: the ids of ``text[:max_chars]``, the first ``max_length - 3``."""
    keep = max(int(max_length) - 3, 0)
    return [np.asarray(tokenizer.text_ids(str(t)[:max_chars])[:keep], dtype=np.uint16) for t in texts]


def model_pairs(plane: Sequence[np.ndarray], rows, pool: int, rr_k: int, q_ids: Sequence[Sequence[int]], max_length: int,
                cls: int, sep: int, first_pair: int, n_pairs: int, row_offset: int = 0):
    """What rr_pairs_measure_dev / rr_pairs_write_dev make of the pairs [first_pair, first_pair + n_pairs) of a batch:
    (tok, typ, pos, cu) int32.  ``rows``: (B, pool) global rows, ``q_ids``: the B queries' ids.  A row outside the plane
    gives ``[CLS] query [SEP] [SEP]``."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, pool)
    avail = max(int(max_length) - 3, 0)
    tok: List[int] = []
    typ: List[int] = []
    pos: List[int] = []
    cu = [0]
    for p in range(first_pair, first_pair + n_pairs):
        b, j = divmod(p, rr_k)
        r = int(rows[b, j]) - row_offset
        text = [int(t) for t in plane[r][:avail]] if 0 <= r < len(plane) else []
        q = [int(t) for t in q_ids[b]]
        ka, kb = keep_lengths(len(q), len(text), max_length)
        ids = [cls] + q[:ka] + [sep] + text[:kb] + [sep]
        tok += ids
        typ += [0] * (ka + 2) + [1] * (kb + 1)
        pos += list(range(len(ids)))
        cu.append(len(tok))
    a = lambda x: np.asarray(x, dtype=np.int32)
    return a(tok), a(typ), a(pos), a(cu)


class PackedQueries:
    """A batch's query ids as the kernels read them (include/rr_hip.h: rr_pairs_measure_dev): ``ids`` int32, ``off`` int32
    [B + 1].  ``host_queries``: the queries of more than ``max_length - 3`` tokens; they are packed with no ids and their
    rows must be scored through the host `predict`."""

    def __init__(self, ids, off, host_queries, max_length):
        self.ids, self.off, self.host_queries, self.max_length = ids, off, list(host_queries), int(max_length)
        self.n_queries = len(off) - 1

    def buffer(self):
        """(one int32 array: the offsets, then the ids (at least one element), offset of the ids)."""
        n_off = len(self.off)
        buf = np.zeros(n_off + max(len(self.ids), 1), dtype=np.int32)
        buf[:n_off] = self.off
        buf[n_off:n_off + len(self.ids)] = self.ids
        return buf, n_off


def pack_queries(id_lists: Sequence[Sequence[int]], max_length: int) -> PackedQueries:
    """id_lists[q] = ``tokenizer.text_ids(query)``."""
    avail = max(int(max_length) - 3, 0)
    host = [q for q, ids in enumerate(id_lists) if len(ids) > avail]
    kept = [np.zeros(0, dtype=np.int32) if len(ids) > avail else np.asarray(ids, dtype=np.int32).reshape(-1) for ids in id_lists]
    off = np.zeros(len(kept) + 1, dtype=np.int32)
    np.cumsum([len(k) for k in kept], out=off[1:])
    flat = np.concatenate(kept) if off[-1] else np.zeros(0, dtype=np.int32)
    return PackedQueries(flat, off, host, max_length)


def _narrow(ids):
    """int32 / int64 ids 0..65535 (a torch tensor) as the int16 tensor with the same low 16 bits."""
    import torch
    return ((ids.to(torch.int32) + 32768) % 65536 - 32768).to(torch.int16)


def join_planes(toks, offs):
    """[ids of plane r (its n_tokens, any integer dtype)], [offsets of plane r, int64 [n_r + 1]] -> (ids, offsets) of the
    planes back to back: plane r's offsets without their leading 0, rebased by the tokens in front of it.  torch tensors on
    any one device (the GPU for `RerankText.concat`, the host in the collective's CPU test)."""
    import torch
    if len(toks) != len(offs) or not toks:
        raise ValueError("join_planes: one id tensor and one offset tensor per plane")
    parts, base = [offs[0][:1].to(torch.int64)], 0
    for t, o in zip(toks, offs):
        if int(o.numel()) < 1:
            raise ValueError("join_planes: an offset tensor holds at least the leading 0")
        parts.append(o[1:].to(torch.int64) + base)
        base += int(t.numel())
    return torch.cat(list(toks)), torch.cat(parts)


# ---------------------------------------------------------------------------------- the plane on the device
class RerankText:
    """The token plane of one index on one GPU: ``d_tok`` the ids back to back (uint16 in memory; held in a torch.int16
    tensor, `tokens()` gives them as numpy uint16), ``d_off`` int64 [n + 1], ``n`` documents, ``n_tokens``; document i is the
    product of global row ``row_offset + i``.  ``max_length``: the cross-encoder's, which decided the cap of ``max_length - 3``
    ids per document."""

    def __init__(self, device: int = 0, row_offset: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the token plane lives on the device only")
        self.device = getattr(device, "index", device) or 0
        self.row_offset = int(row_offset)
        h = C.c_void_p()
        _lib.check(_lib.load().rr_pairs_create(self.device, C.byref(h)), "rr_pairs_create")
        self._h = h
        self.d_tok = self.d_off = None
        self.n = self.n_tokens = self.max_length = 0
        self.cls_id = self.sep_id = self.vocab_size = 0
        self.host_docs: List[int] = []

    # ------------------------------------------------------------------ building
    @staticmethod
    def _check_build(tokenizer, max_length: int, chunk_docs: int) -> None:
        """What a plane cannot be built for, said before anything touches the device."""
        L = int(max_length)
        if L < 3:
            raise ValueError(f"max_length {L} leaves no room for [CLS] [SEP] [SEP]")
        vocab_size = max(tokenizer.vocab.values()) + 1
        if vocab_size > MAX_VOCAB:
            raise ValueError(f"a vocabulary of {vocab_size} pieces does not fit the plane's uint16 ids: use rerank=\"host\"")
        if int(chunk_docs) < 1:
            raise ValueError("chunk_docs must be at least 1")

    def _begin(self, tokenizer, max_length: int, n: int, max_bytes: Optional[int]) -> None:
        self.max_length, self.vocab_size = int(max_length), max(tokenizer.vocab.values()) + 1
        self.cls_id, self.sep_id = int(tokenizer.cls_id), int(tokenizer.sep_id)
        self._parts, self._lens_all, self._done, self._max_bytes, self.n = [], np.zeros(n, dtype=np.int64), 0, max_bytes, int(n)
        self._room(0)

    def _room(self, tokens: int) -> None:
        need = 2 * max(tokens, 1) + 8 * (self.n + 1)
        if self._max_bytes is not None and need > self._max_bytes:
            raise MemoryError(f"the token plane of {self.n} products needs {need} bytes of device memory or more, more than the "
                              f"{self._max_bytes} allowed: use rerank=\"host\" (or raise rerank_max_bytes)")

    def _block(self, wp, tokenizer, d_text: int, text_bytes: int, d_off, c0: int, host_head, also_host: Sequence[int] = ()) -> None:
        """Documents [c0, c0 + nd) of the plane: their heads lie on the device at `d_text` (address of the first byte) with
        the int64 offsets `d_off` [nd + 1] relative to it.  Tokenised by `wp` ([CLS], the first max_length - 3 pieces,
        [SEP]), narrowed to uint16 and appended; what the device tokenizer hands back, and the documents `also_host` (whose
        heads on the device are empty), are tokenised from ``host_head(i)`` (document i of the block as a str) and placed at
        their own offsets."""
        import torch
        dev = torch.device("cuda", self.device)
        L, keep, nd = self.max_length, self.max_length - 3, int(d_off.numel()) - 1
        packed, info, _, cap, _keep = wp.queue_dev(d_text, int(text_bytes), d_off, L - 1)
        torch.cuda.current_stream(dev).synchronize()
        h = info.numpy()
        tok, _, pos, cu = wp.views(packed, nd, cap, int(h[0]))
        cu_h = cu.cpu().numpy().astype(np.int64)
        lens = cu_h[1:] - cu_h[:-1] - 2                     # (a handed-back document: the placeholder, 0)
        host = sorted(set(np.flatnonzero(h[1:nd + 1]).tolist()) | set(int(i) for i in also_host))
        host_ids = [np.asarray(tokenizer.text_ids(host_head(i))[:keep], dtype=np.int64) for i in host]
        for i, ids in zip(host, host_ids):
            lens[i] = len(ids)
        new_off = np.zeros(nd + 1, dtype=np.int64)
        np.cumsum(lens, out=new_off[1:])
        m = int(new_off[-1])
        self._room(self._done + m)
        out = torch.empty(m, dtype=torch.int16, device=dev)
        if m:
            # the pieces without [CLS] / [SEP], each to its document's new offset + its place in the document
            is_piece = pos > 0
            is_piece[(cu[1:] - 1).long()] = False
            doc = torch.repeat_interleave(torch.arange(nd, device=dev), (cu[1:] - cu[:-1]).long(), output_size=int(h[0]))
            where = torch.from_numpy(new_off).to(dev)[doc[is_piece]] + pos[is_piece].long() - 1
            out[where] = _narrow(tok[is_piece])
            for i, ids in zip(host, host_ids):
                if len(ids):
                    out[int(new_off[i]):int(new_off[i + 1])] = _narrow(torch.from_numpy(ids).to(dev))
        self._parts.append(out)
        self._lens_all[c0:c0 + nd] = lens
        self._done += m
        self.host_docs += [c0 + i for i in host]

    def _finish(self) -> "RerankText":
        import torch
        dev = torch.device("cuda", self.device)
        plane_off = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self._lens_all, out=plane_off[1:])
        self.d_tok = torch.cat(self._parts) if self._done else torch.zeros(1, dtype=torch.int16, device=dev)
        self.d_off = torch.from_numpy(plane_off).to(dev)
        self.n_tokens = int(self._done)
        self._parts = None
        torch.cuda.current_stream(dev).synchronize()
        return self

    @classmethod
    def from_texts(cls, texts: Sequence[str], tokenizer, max_length: int, device: int = 0, *, max_chars: int = MAX_CHARS,
                   max_bytes: Optional[int] = None, row_offset: int = 0, chunk_docs: int = CHUNK_DOCS,
                   stage_bytes: int = STAGE_BYTES) -> "RerankText":
        """From a column of str.  The first ``max_chars`` characters of every text are uploaded as UTF-8 (in row blocks through
        two pinned buffers, embed._stage_rows) and tokenised ``chunk_docs`` documents at a time by the device tokenizer
        (``[CLS]``, the first ``max_length - 3`` pieces, ``[SEP]``); the pieces are narrowed to uint16 and appended.  What
        the device tokenizer hands back (a hard code point, malformed bytes, more than 4 096 bytes of text without enough
        pieces in them or of mapped text: ``host_docs``) is tokenised by ``tokenizer.text_ids`` and placed at its own
        offsets: the plane is dense and in row order.  The raw heads are dropped once the plane stands.
        ``max_bytes``: refuse (MemoryError) a plane that needs more device memory than this -- up to about 1 KB per
        product: 10M products of about 450 tokens are about 9 GB."""
        import torch
        from .embed import DeviceWordPiece, _stage_rows, _utf8_column
        cls._check_build(tokenizer, max_length, chunk_docs)
        self = cls(device, row_offset)
        heads = [str(t)[:max_chars] for t in texts]
        raw, off = _utf8_column(heads)
        n, total = len(off) - 1, int(off[-1])
        self._begin(tokenizer, max_length, n, max_bytes)
        dev = torch.device("cuda", self.device)
        wp = DeviceWordPiece(tokenizer, self.device)
        try:
            with torch.cuda.device(dev):
                main = torch.cuda.current_stream(dev)
                d_text = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
                d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)

                def on_rows(a: int, b: int) -> None:
                    for c0 in range(a, b, int(chunk_docs)):
                        c1, base = min(b, c0 + int(chunk_docs)), int(off[c0])
                        self._block(wp, tokenizer, d_text.data_ptr() + base, int(off[c1]) - base, d_off[c0:c1 + 1] - base, c0,
                                    lambda i: heads[c0 + i])

                _stage_rows(raw, off, d_text, main, stage_bytes, on_rows)
                wp.check()
                self._finish()
        finally:
            wp.close()
        return self

    @classmethod
    def from_device(cls, text, tokenizer, max_length: int, *, rows=None, max_chars: int = MAX_CHARS,
                    max_bytes: Optional[int] = None, row_offset: int = 0, chunk_docs: int = CHUNK_DOCS) -> "RerankText":
        """From a products.DeviceProductText (agg_text where rr_products_concat_dev wrote it): the plane `from_texts` builds
        from ``text.agg_text()``, with no host copy of the text.  ``rows``: the product rows the plane holds, in order
        (int array, e.g. the ``kept`` of embed.build_product_embeddings_device; None = all).  ``chunk_docs`` documents at a
        time: rr_textprep_head_measure_dev / rr_textprep_head_write_dev cut the raw heads (``str[:max_chars]``, read
        through ``rows`` without a copy of the text) into a block buffer, and the block goes through the step `from_texts`
        runs.  What the tokenizer hands back is read back from that buffer; a document whose head holds malformed UTF-8 has
        no head on the device, and its bytes are fetched from the text."""
        import torch
        from . import textprep as T
        from .embed import DeviceWordPiece
        cls._check_build(tokenizer, max_length, chunk_docs)
        self = cls(text.device, row_offset)
        n_src = int(text.n)
        rows = np.arange(n_src, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        n = len(rows)
        if n and (rows.min() < 0 or rows.max() >= n_src):
            raise ValueError(f"rows outside the {n_src} products of the text")
        self._begin(tokenizer, max_length, n, max_bytes)
        dev = torch.device("cuda", self.device)
        wp = DeviceWordPiece(tokenizer, self.device)
        tp = T.TextPrep(self.device)
        try:
            with torch.cuda.device(dev):
                main = torch.cuda.current_stream(dev)
                st = main.cuda_stream
                p_text = text.d_text.data_ptr() if text.text_bytes else None
                d_rows = torch.from_numpy(rows if n else np.zeros(1, dtype=np.int32)).to(dev)
                src_off = None
                for c0 in range(0, n, int(chunk_docs)):
                    nd = min(n, c0 + int(chunk_docs)) - c0
                    d_len = torch.empty(nd, dtype=torch.int32, device=dev)
                    d_st = torch.empty(nd, dtype=torch.int32, device=dev)
                    d_off = torch.empty(nd + 1, dtype=torch.int64, device=dev)
                    args = (p_text, text.text_bytes, text.d_off.data_ptr(), n_src, d_rows.data_ptr() + 4 * c0, nd, int(max_chars),
                            False, 0, d_len.data_ptr(), d_st.data_ptr())
                    tp.head_measure(*args, st)
                    tp.head_offsets(d_len.data_ptr(), d_st.data_ptr(), nd, d_off.data_ptr(), st)
                    nbytes = int(d_off[nd].item())             # sizes the block buffer
                    if nbytes >= 2 ** 31:
                        raise ValueError(f"{nbytes} bytes of heads in one block: lower chunk_docs")
                    d_heads = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
                    tp.head_write(*args, d_heads.data_ptr(), nbytes, d_off.data_ptr(), st)
                    left = np.flatnonzero(d_st.cpu().numpy()).tolist()
                    tp.check()
                    off_h = d_off.cpu().numpy()

                    def host_head(i):                              # (called inside this block's step only)
                        nonlocal src_off
                        if i in left:                          # malformed inside the head: no head on the device
                            if src_off is None:
                                src_off = text.d_off.cpu().numpy()
                            r = int(rows[c0 + i])
                            raw = text.d_text[int(src_off[r]):int(src_off[r + 1])].cpu().numpy().tobytes()
                            return raw.decode("utf-8", "surrogatepass")[:max_chars]
                        return d_heads[int(off_h[i]):int(off_h[i + 1])].cpu().numpy().tobytes().decode("utf-8", "surrogatepass")

                    self._block(wp, tokenizer, d_heads.data_ptr(), nbytes, d_off, c0, host_head, left)
                wp.check()
                self._finish()
        finally:
            wp.close()
            tp.close()
        return self

    @classmethod
    def concat(cls, planes: Sequence["RerankText"]) -> "RerankText":
        """The planes of consecutive row shards, in rank order, as ONE plane with the first shard's ``row_offset``: the ids
        appended, the offsets rebased, all on the device (`join_planes`) -- bitwise the plane `from_texts` builds from all
        the texts at once (a document's ids do not depend on its neighbours).  The planes must live on one GPU."""
        if not planes:
            raise ValueError("no planes to join")
        first = planes[0]
        at = first.row_offset
        for p in planes:
            if p.row_offset != at:
                raise ValueError(f"the planes are not consecutive row shards: one begins at row {p.row_offset}, expected {at}")
            if (p.max_length, p.cls_id, p.sep_id, p.vocab_size, p.device) != (first.max_length, first.cls_id, first.sep_id,
                                                                               first.vocab_size, first.device):
                raise ValueError("the planes were cut for different models or live on different GPUs")
            at += p.n
        tok, off = join_planes([p.d_tok[:p.n_tokens] for p in planes], [p.d_off for p in planes])
        host_docs = [p.row_offset - first.row_offset + i for p in planes for i in p.host_docs]
        return cls.from_arrays(tok, off, first, host_docs)

    @classmethod
    def from_arrays(cls, tok, off, like: "RerankText", host_docs: Sequence[int] = ()) -> "RerankText":
        """A plane over ready device tensors (``tok`` int16 ids back to back, ``off`` int64 [n + 1]) with the model constants,
        the device and the row offset of ``like``."""
        import torch
        self = cls(like.device, like.row_offset)
        self.max_length, self.vocab_size, self.cls_id, self.sep_id = like.max_length, like.vocab_size, like.cls_id, like.sep_id
        dev = torch.device("cuda", self.device)
        self.n, self.n_tokens = int(off.numel()) - 1, int(tok.numel())
        self.d_tok = tok.to(dev).contiguous() if self.n_tokens else torch.zeros(1, dtype=torch.int16, device=dev)
        self.d_off = off.to(dev).contiguous()
        self.host_docs = list(host_docs)
        return self

    def tokens(self) -> List[np.ndarray]:
        """The plane on the host: per document its uint16 ids (tests)."""
        flat = self.d_tok[:self.n_tokens].cpu().numpy().view(np.uint16)
        off = self.d_off.cpu().numpy()
        return [flat[off[i]:off[i + 1]] for i in range(self.n)]

    def check_model(self, ce) -> None:
        """Raises ValueError unless ``ce`` (a cross_encoder.CrossEncoder) can score this plane's ids."""
        if self.vocab_size > ce.model.vocab:
            raise ValueError(f"the tokenizer's vocabulary ({self.vocab_size} pieces) is larger than the model's embedding table "
                             f"({ce.model.vocab} rows)")
        if ce.max_length != self.max_length:
            raise ValueError(f"the plane was cut for max_length {self.max_length}, the cross-encoder has {ce.max_length}")
        if ce.model.n_labels != 1:
            raise ValueError(f"the device rerank path scores single-label models; this one has {ce.model.n_labels} labels")
        if ce.model.device != self.device:
            raise ValueError(f"the plane lives on GPU {self.device}, the cross-encoder on GPU {ce.model.device}")

    # ------------------------------------------------------------------ per batch
    def upload(self, packed: PackedQueries):
        """The packed queries on the device: (int32 tensor, offset of the ids).  One copy."""
        import torch
        buf, at = packed.buffer()
        return torch.from_numpy(buf).to(torch.device("cuda", self.device)), at

    def _check_rows(self, rows, rr_k: int, packed: PackedQueries):
        import torch
        B, pool = rows.shape
        if B != packed.n_queries:
            raise ValueError(f"{packed.n_queries} packed queries for {B} rows of candidates")
        if not rows.is_contiguous() or rows.dtype != torch.int64:
            raise ValueError("rows must be a contiguous int64 tensor")
        if packed.max_length != self.max_length:
            raise ValueError(f"queries packed for max_length {packed.max_length}, the plane was cut for {self.max_length}")
        return B, pool

    def pairs(self, rows, rr_k: int, packed: PackedQueries, first_pair: int = 0, n_pairs: Optional[int] = None, staged=None):
        """rr_pairs_measure_dev, the read-back of the token count, rr_pairs_write_dev, on the current stream: the packed
        sequences of the pairs [first_pair, first_pair + n_pairs) of ``rows`` ((B, pool) int64 device tensor of global rows,
        the first ``rr_k`` of every query) -> (tok, typ, pos, cu) int32 device tensors, as `forward_packed_dev` takes them."""
        import torch
        B, pool = self._check_rows(rows, rr_k, packed)
        n_pairs = B * int(rr_k) - int(first_pair) if n_pairs is None else int(n_pairs)
        lib = _lib.load()
        d_q, at = staged if staged is not None else self.upload(packed)
        p = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
        keep = torch.empty((max(n_pairs, 1), 2), dtype=torch.int32, device=rows.device)
        cu = torch.empty(max(n_pairs, 0) + 1, dtype=torch.int32, device=rows.device)
        _lib.check(lib.rr_pairs_measure_dev(self._h, p(self.d_off), self.n, self.row_offset, p(rows), pool, int(rr_k), p(d_q), B,
                                            self.max_length, int(first_pair), n_pairs, p(keep), p(cu), st), "rr_pairs_measure_dev")
        n_tokens = int(cu[n_pairs].item())                 # the only number read back: it sizes the three id arrays
        ids = torch.empty(3 * max(n_tokens, 1), dtype=torch.int32, device=rows.device)
        tok, typ, pos = ids[:n_tokens], ids[n_tokens:2 * n_tokens], ids[2 * n_tokens:3 * n_tokens]
        _lib.check(lib.rr_pairs_write_dev(self._h, p(self.d_tok), p(self.d_off), self.n, self.row_offset, p(rows), pool, int(rr_k),
                                          C.c_void_p(d_q.data_ptr() + 4 * at), p(d_q), B, self.cls_id, self.sep_id, int(first_pair),
                                          n_pairs, p(keep), p(cu), n_tokens, p(ids), C.c_void_p(ids.data_ptr() + 4 * n_tokens),
                                          C.c_void_p(ids.data_ptr() + 8 * n_tokens), st), "rr_pairs_write_dev")
        return tok, typ, pos, cu

    def scores(self, ce, rows, rr_k: int, packed: PackedQueries, first_pair: int = 0, n_pairs: Optional[int] = None,
               staged=None):
        """The reranker's scores of the first ``rr_k`` candidates of every query: (B, rr_k) float32 on the device, what
        ``ce.predict`` gives for the pairs ``(query, agg_text[:2000])``.  The pairs go through the model in chunks of
        ``n_pairs * max_length <= min(ce.model.max_tokens_per_call, FP32_MAX_TOKENS)`` (a bound that needs no lengths on the
        host); per chunk `pairs` and `forward_packed_dev`.  A pass of the fp32 mode that leaves the fp16 range poisons its
        call's logits with NaN (include/rr_hip.h): after all chunks ONE ``isnan`` over the scores decides whether the handle
        switches to the wide-range kernels and the chunks run again, once.  The rows of ``packed.host_queries`` hold the
        scores of the EMPTY query: the caller overwrites them (HybridSearcher.search_batch does).
        ``first_pair`` / ``n_pairs``: only the range [first_pair, first_pair + n_pairs) of the flattened B x rr_k pair list
        (a rank's share, sharded.split_pairs; it may begin and end inside a query) -> a flat (n_pairs,) tensor.  An empty
        range launches nothing and returns an empty tensor.  ``staged``: the packed queries already on the device, as `pairs`
        takes them (then ``packed`` is asked for its sizes only)."""
        import torch
        from .cross_encoder import FP32_MAX_TOKENS, OUT_LOGITS
        self.check_model(ce)
        B, pool = self._check_rows(rows, rr_k, packed)
        rr_k = int(rr_k)
        if not 1 <= rr_k <= pool:
            raise ValueError(f"rr_k {rr_k} outside 1..pool = {pool}")
        L = self.max_length
        whole = n_pairs is None and int(first_pair) == 0
        first = int(first_pair)
        total = B * rr_k - first if n_pairs is None else int(n_pairs)
        if first < 0 or total < 0 or first + total > B * rr_k:
            raise ValueError(f"pairs [{first}, {first + total}) outside the batch's {B * rr_k}")
        if total == 0:
            return torch.empty(0, dtype=torch.float32, device=rows.device)
        step = max(1, min(int(ce.model.max_tokens_per_call), FP32_MAX_TOKENS) // L)
        with torch.cuda.device(rows.device):
            staged = staged if staged is not None else self.upload(packed)
            out = torch.empty(total, dtype=torch.float32, device=rows.device)

            def run():
                for a in range(0, total, step):
                    m = min(step, total - a)
                    tok, typ, pos, cu = self.pairs(rows, rr_k, packed, first + a, m, staged)
                    out[a:a + m] = ce.model.forward_packed_dev(tok, typ, pos, cu, m, L, OUT_LOGITS)[:, 0]

            run()
            if bool(torch.isnan(out).any()):
                if ce.model.precision != "fp32" or ce.model.wide_range:
                    raise _lib.HipLibraryError("the cross-encoder answered NaN scores")
                ce.model.set_wide_range(True)              # as forward_ids: the handle continues on the wide-range kernels
                run()
                if bool(torch.isnan(out).any()):
                    raise _lib.HipLibraryError("the cross-encoder answered NaN scores on the wide-range kernels")
            self.check()
            if ce.activation == "sigmoid":                 # CrossEncoder._post: float64, rounded once to float32
                out = (1.0 / (1.0 + torch.exp(-out.to(torch.float64)))).to(torch.float32)
        return out.view(B, rr_k) if whole else out

    def check(self) -> None:
        """Raises ValueError when a call since the last check met a candidate row outside the plane or refused a pair
        (waits for the device)."""
        bad = C.c_int32()
        _lib.check(_lib.load().rr_pairs_status(self._h, C.byref(bad)), "rr_pairs_status")

    @property
    def nbytes(self) -> int:
        """Device memory the plane holds."""
        return 0 if self.d_tok is None else int(2 * self.d_tok.numel() + 8 * self.d_off.numel())

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_pairs_destroy(self._h)
            self._h = None
        self.d_tok = self.d_off = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
