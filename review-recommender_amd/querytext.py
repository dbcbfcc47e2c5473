"""The query text of a batch on the GPU (csrc/rr_query.hip), and the kernels' model on the CPU.

Stands in for what `SearchEngine.run_search_batch` does per query in Python before the kernels run: `text.tokenize_query` +
`BM25Index.term_ids`, `text.build_gate_groups` + `gate.pack_groups`, `tokenizer.text_ids` + `rerank.pack_queries`.

`QueryText` is the per-index object: the BM25 vocabulary as an open-addressing table, the stop words and the static gate groups
of text.py (uploaded once; the kernel source holds no word list) and, with a reranker, the device WordPiece tokenizer of the
cross-encoder's vocabulary.  `QueryText.front(queries, penalty)` stages the batch's bytes with ONE upload, queues the kernels
on the current stream and returns a `QueryFront`: device buffers in the layouts `rr_bm25_scores_at_dev`, `rr_gate_factors_dev`
and `rr_pairs_*_dev` read, and the ``needs_host`` flags, which travel to the host with the batch's answer (nothing is read back
before it).  A flagged query (FLAG_*) has no ids, no groups and no reranker ids on the device and is served by the host
functions.  `model_front` states in plain Python, without ``re``, what the kernels compute for one query, as
doctok.model_tokenize does for the document tokenizer.

With a `QueryEncoder` the front also makes the query VECTORS K1 reads (`QueryFront.qvecs`): the device WordPiece tokenizer
of the encoder's vocabulary over the same staged bytes, the forward with the encoder's pooled output (CLS rows or token means) and `rr_query_vectors_dev`, which
normalises the rows with numpy's float32 roundings, bit for bit.  `model_query_vectors` states that kernel in plain Python,
the pairwise order of the additions written out.

The byte rules are doctok.py's (tests/test_doctok_model.py proves them against ``str.lower()`` and ``re``) with the query-time
stop list, one-byte tokens kept and no cap; the colour groups are substring matches against the gate plane's byte image of
the query (gate.model_gate_plane), in which an ASCII string occurs exactly when it occurs in ``query.lower()``.
"""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, text
from .gate import MAX_GROUPS, MAX_TERM_BYTES, MAX_TERMS, QUERY_TERM_BYTES, _utf8, factor_table, model_gate_plane
from .vocabtable import model_hash, model_slot, table_lookup  # noqa: F401  (the walk of build_vocab_table's table)

MAX_QUERY_BYTES = 1024      # rr_query_limits (QueryText checks these against the library): bytes of a query,
MAX_TOKEN_BYTES = 64        # of a token,
MAX_STOP_BYTES = 8          # of a stop word the kernels hold
FLAG_QUERY, FLAG_TOKEN, FLAG_RERANK, FLAG_WP, FLAG_SPAN = 1, 2, 4, 8, 16     # needs_host bits (include/rr_hip.h)
FLAG_ENCODER = 32           # needs_host bit: the QUERY ENCODER's WordPiece kernel handed the query back (rr_query_flag_dev)

# alnums and the apostrophe stay, everything else (NUL and every byte >= 0x80 included) is a separator
_MAP = bytes(c if (48 <= c <= 57 or 97 <= c <= 122 or c == 39) else 32 for c in range(256))

FrontModel = namedtuple("FrontModel", "tokens ids groups terms rerank_ids flag")


# ---------------------------------------------------------------------------------- the static tables
@functools.lru_cache(maxsize=None)
def static_tables():
    """text.py's word lists as `rr_query_create` takes them: (stop words, groups, n_colors, keys) -- the groups are the colour
    groups in COLORS order, then the synonym groups in SYNONYMS order, each a SORTED list of terms; keys = SYNONYMS' keys."""
    groups = [sorted(g) for g in text.COLORS.values()] + [sorted(g) for g in text.SYNONYMS.values()]
    return sorted(text.QUERY_STOP_WORDS), groups, len(text.COLORS), list(text.SYNONYMS)


def _strings(items: Sequence[str], dtype=np.int32) -> Tuple[np.ndarray, np.ndarray]:
    blobs = [s.encode("utf-8") for s in items]
    off = np.zeros(len(blobs) + 1, dtype=dtype)
    np.cumsum([len(b) for b in blobs], out=off[1:])
    data = np.frombuffer(b"".join(blobs), dtype=np.uint8).copy() if off[-1] else np.zeros(1, dtype=np.uint8)
    return data, off


def vocab_arrays(vocab: Dict[str, int]) -> Tuple[np.ndarray, np.ndarray]:
    """(bytes, int64 offsets) of the vocabulary in id order; an id no string has is an empty entry."""
    n = max(vocab.values()) + 1 if vocab else 0
    entries = [""] * n
    for s, i in vocab.items():
        if i < 0:
            raise ValueError(f"vocabulary id {i} of {s!r} is negative")
        entries[i] = s
    return _strings(entries, np.int64)


def build_vocab_table(vocab: Dict[str, int]):
    """The open-addressing table the device looks tokens up in, built by the library ON THE HOST (rr_query_build_table; no
    GPU needed): (slots [n_slots][4] int32 = hash, first byte, length, id or -1; vocabulary bytes; entries kept).
    `table_lookup` (vocabtable.py) is the kernel's walk through it."""
    lib = _lib.load()
    blob, off = vocab_arrays(vocab)
    n_slots, kept = C.c_int32(), C.c_int32()
    _lib.check(lib.rr_query_table_slots(len(off) - 1, C.byref(n_slots)), "rr_query_table_slots")
    slots = np.empty((n_slots.value, 4), dtype=np.int32)
    _lib.check(lib.rr_query_build_table(_lib.ptr(blob), _lib.ptr(off), len(off) - 1, n_slots.value, _lib.ptr(slots),
                                        C.byref(kept)), "rr_query_build_table")
    return slots, blob, kept.value


# ---------------------------------------------------------------------------------- the model
def model_tokens(image: bytes) -> List[bytes]:
    """The tokens of a query's image, stop words included: doctok.model_tokenize's walk."""
    out: List[bytes] = []
    for chunk in image.translate(_MAP).split():    # maximal pieces of alnums and apostrophes
        runs = chunk.split(b"'")                   # an empty run = two apostrophes in a row, or one at either end
        i = 0
        while i < len(runs):
            if not runs[i]:
                i += 1
            elif i + 1 < len(runs) and runs[i + 1]:  # one apostrophe, then a run: the token takes both
                out.append(runs[i] + b"'" + runs[i + 1])
                i += 2
            else:
                out.append(runs[i])
                i += 1
    return out


@functools.lru_cache(maxsize=None)
def _model_tables():
    """static_tables() as bytes: (stop words, groups, n_colors, keys)."""
    stop, groups, n_colors, keys = static_tables()
    return (frozenset(s.encode("ascii") for s in stop), [[w.encode("ascii") for w in g] for g in groups], n_colors,
            [k.encode("ascii") for k in keys])


def model_front(query_bytes, vocab: Dict[str, int], *, rerank_tokenizer=None, max_length: int = 512) -> FrontModel:
    """What rr_query_front_dev / rr_query_strip_dev answer for one query (a str, or its UTF-8 bytes): ``tokens`` (str),
    ``ids`` (vocabulary ids, -1 = unknown), ``groups`` (each a sorted list of terms), ``terms`` ((group, bytes) in packing
    order), ``rerank_ids`` (None without a tokenizer) and ``flag`` (FLAG_* bits).  A flagged query has nothing but its flag."""
    raw = _utf8(query_bytes)
    stop_b, static, n_colors, key_b = _model_tables()
    flag = 0
    toks: List[bytes] = []
    image = b""
    if len(raw) > MAX_QUERY_BYTES:
        flag |= FLAG_QUERY
    else:
        image = model_gate_plane(raw, max_chars=len(raw) + 1)          # (no cut: a query is taken whole)
        every = model_tokens(image)
        if any(len(t) > MAX_TOKEN_BYTES for t in every):
            flag |= FLAG_TOKEN
        toks = [t for t in every if t not in stop_b]
    rr: Optional[List[int]] = None
    if rerank_tokenizer is not None:
        from .wp_unicode import model_tokenize
        ids, needs_host, _ = model_tokenize(bytes(raw), rerank_tokenizer, int(max_length))
        if needs_host:
            flag |= FLAG_WP
            rr = []
        else:
            rr = [int(t) for t in ids[1:-1]]
            if len(rr) > int(max_length) - 3:
                flag |= FLAG_RERANK
    if flag:
        return FrontModel([], [], [], [], None if rr is None else [], flag)
    ids_out = [vocab.get(t.decode("ascii"), -1) for t in toks]
    groups: List[List[bytes]] = []
    for g in static[:n_colors]:                                        # a substring of the image, not a token
        if any(w in image for w in g):
            groups.append(g)
    for t in toks:
        if t in key_b:
            groups.append(static[n_colors + key_b.index(t)])
        elif len(t) >= text.MIN_KEYWORD_LEN:
            groups.append([t])
    unique: List[List[bytes]] = []
    for g in groups:                                                   # (sorted lists of distinct terms: equal as sets = equal)
        if g not in unique:
            unique.append(g)
    unique = unique[:text.MAX_GATE_GROUPS]
    terms = [(i, w) for i, g in enumerate(unique) for w in g]
    return FrontModel([t.decode("ascii") for t in toks], ids_out, [[w.decode("ascii") for w in g] for g in unique], terms, rr,
                      flag)


# ---------------------------------------------------------------------------------- the model of the query vectors
PAIRWISE_BLOCK = 128        # numpy's pairwise sum: a piece of at most this many terms is summed on eight accumulators
VECTOR_EPS = 1e-12          # QueryEncoder.encode_ids: e / maximum(norm, 1e-12)


def model_pairwise_leaves(n: int) -> List[Tuple[int, int, int]]:
    """The pieces numpy's pairwise sum cuts ``n`` terms into, left to right: (first term, terms, depth).  A piece of more
    than PAIRWISE_BLOCK terms is split at ``n2 = n // 2 - (n // 2) % 8``; two neighbours of one depth are the halves of one
    split (the tree is full), so the list states the whole order of the additions."""
    out: List[Tuple[int, int, int]] = []
    todo = [(0, int(n), 0)]
    while todo:
        first, m, depth = todo.pop()
        while m > PAIRWISE_BLOCK:
            n2 = m // 2
            n2 -= n2 % 8
            todo.append((first + n2, m - n2, depth + 1))
            m, depth = n2, depth + 1
        out.append((first, m, depth))
    return out


def _model_leaf_sum(a: Sequence[np.float32]) -> np.float32:
    n = len(a)
    if n < 8:
        res = np.float32(0.0)
        for v in a:
            res = res + v
        return res
    r = list(a[:8])
    body = n - n % 8
    for i in range(8, body, 8):
        for j in range(8):
            r[j] = r[j] + a[i + j]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[body:]:
        res = res + v
    return res


def model_pairwise_sum(a: Sequence[np.float32]) -> np.float32:
    """``np.add.reduce`` of float32 terms that lie contiguous in memory, one float32 rounding per addition: the leaves of
    `model_pairwise_leaves`, folded in the order of the splits (left + right)."""
    stack: List[Tuple[np.float32, int]] = []
    for first, m, depth in model_pairwise_leaves(len(a)):
        s = _model_leaf_sum(a[first:first + m])
        while stack and stack[-1][1] == depth:             # the left half of the same split is waiting
            left, _ = stack.pop()
            s, depth = left + s, depth - 1
        stack.append((s, depth))
    return stack[0][0]


def model_query_vectors(rows, eps: float = VECTOR_EPS) -> np.ndarray:
    """What rr_query_vectors_dev answers: row q = rows[q] / maximum(norm(rows[q]), float32(eps)), every operation rounded to
    float32 once -- ``(e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), eps)).astype(np.float32)`` bit for bit
    (tests/test_query_vectors_model.py, every width class of the split).  Each square is rounded before it is summed, the
    sum runs in numpy's pairwise order, the square root and the quotients are correctly rounded, and the maximum keeps a NaN
    norm (numpy's ``maximum``, not C's fmaxf)."""
    e = np.ascontiguousarray(rows, dtype=np.float32)
    if e.ndim != 2 or e.shape[1] < 1:
        raise ValueError(f"rows must be (n, dim >= 1); got {e.shape}")
    out = np.empty_like(e)
    eps32 = np.float32(eps)
    with np.errstate(all="ignore"):
        for q in range(e.shape[0]):
            row = [np.float32(v) for v in e[q]]
            norm = np.sqrt(model_pairwise_sum([v * v for v in row]))
            d = norm if (norm != norm or norm > eps32) else eps32
            for i, v in enumerate(row):
                out[q, i] = v / d
    return out


# ---------------------------------------------------------------------------------- the batch on the device
class QueryFront:
    """One batch's query text on the device (QueryText.front).  ``terms``: an engine.StagedTerms (``n_ids`` is an upper
    bound); ``gate_staged``: ``(buffer, offsets)`` as `GateText.factors(staged=)` takes them; ``rerank_staged``: ``(int32
    tensor, offset of the ids)`` as `RerankText.pairs(staged=)` takes them, or None; ``needs_host``: int32 (B,) device tensor
    of FLAG_* bits.  It also stands where a gate.PackedGroups / rerank.PackedQueries is asked only for its sizes:
    ``n_queries``, ``max_length``, and ``host_queries`` (empty: the flags are not known on the host before the answer).
    ``qvecs``: with a query encoder, the (B, dim) float32 device tensor of the queries' unit vectors (zeros where a query is
    flagged), which `HybridSearcher.search_batch(None, ..., query_front=)` hands to K1."""

    def __init__(self, n_queries, terms, gate_staged, rerank_staged, needs_host, max_length, keep, qvecs=None):
        self.n_queries, self.terms, self.gate_staged, self.rerank_staged = int(n_queries), terms, gate_staged, rerank_staged
        self.needs_host, self.max_length, self._keep = needs_host, int(max_length), keep
        self.host_queries: List[int] = []
        # (B, dim) float32 device tensor: the queries' unit vectors as K1 reads them (QueryText with an encoder), else None;
        # zeros in the rows of flagged queries
        self.qvecs = qvecs

    def _i32(self, name: str, count: int):
        buf, where = self._keep["buf"], self._keep["where"]
        import torch
        return buf[where[name]:where[name] + 4 * count].view(torch.int32)

    def host_arrays(self) -> dict:
        """The device-made arrays on the host, cut to their lengths (tests; waits for the device)."""
        B = self.n_queries
        out = {"needs_host": self.needs_host.cpu().numpy(), "ids_off": self._i32("ids_off", B + 1).cpu().numpy(),
               "q_term": self._i32("q_term", B + 1).cpu().numpy(), "q_groups": self._i32("q_groups", B).cpu().numpy()}
        out["ids"] = self._i32("ids", int(out["ids_off"][B])).cpu().numpy()
        T = int(out["q_term"][B])
        out["term_off"] = self._i32("term_off", T + 1).cpu().numpy()
        out["term_group"] = self._i32("term_group", T).cpu().numpy()
        buf, where = self._keep["buf"], self._keep["where"]
        out["term_bytes"] = buf[where["term_bytes"]:where["term_bytes"] + int(out["term_off"][T])].cpu().numpy()
        if self.rerank_staged is not None:
            out["rr_off"] = self._i32("rr_off", B + 1).cpu().numpy()
            out["rr_ids"] = self._i32("rr_ids", int(out["rr_off"][B])).cpu().numpy()
        return out


class QueryText:
    """The query front end of one index on one GPU.  ``vocab``: the BM25 vocabulary (token -> id; {} when the index has no
    BM25 leg); ``rerank_tokenizer``: the cross-encoder's WordPieceTokenizer when the reranker's query ids are wanted too,
    with the cross-encoder's ``max_length``.  ``encoder``: a cross_encoder.QueryEncoder with a (lower-casing) tokenizer, on
    this device, when the query VECTORS are wanted too: every front then also tokenises the staged bytes with the encoder's
    vocabulary (truncated to ``encoder.max_length`` as ``encode_pair(s, None, max_length)`` truncates), runs the forward and
    normalises the pooled rows (CLS or mean, the encoder's `out_mode`) as numpy does (rr_query_vectors_dev) into ``QueryFront.qvecs`` -- bit for bit the rows of
    ``encoder.encode(queries, normalize_embeddings=True)``.  A query the encoder's tokenizer kernel hands back carries
    FLAG_ENCODER; its sequence is the placeholder [CLS] [SEP].  The row of every flagged query is zeros."""

    def __init__(self, vocab: Optional[Dict[str, int]], *, rerank_tokenizer=None, max_length: int = 512, device: int = 0,
                 encoder=None):
        import torch
        if vocab is None:
            raise ValueError("this corpus was built from integer ids; pass ids directly")
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the query front end runs on the device only")
        lib = _lib.load()
        lim = [C.c_int32() for _ in range(4)]
        _lib.check(lib.rr_query_limits(*[C.byref(v) for v in lim]), "rr_query_limits")
        if tuple(v.value for v in lim) != (MAX_QUERY_BYTES, MAX_TOKEN_BYTES, MAX_GROUPS, MAX_STOP_BYTES) \
                or MAX_TOKEN_BYTES != MAX_TERM_BYTES or text.MAX_GATE_GROUPS > MAX_GROUPS:
            raise _lib.HipLibraryError("querytext.py, gate.py and csrc/rr_query.hip disagree on the kernels' limits")
        self.device = getattr(device, "index", device) or 0
        self.max_length = int(max_length)
        stop, groups, n_colors, keys = static_tables()
        v_bytes, v_off = vocab_arrays(vocab)
        s_bytes, s_off = _strings(stop)
        t_bytes, t_off = _strings([w for g in groups for w in g])
        g_off = np.zeros(len(groups) + 1, dtype=np.int32)
        np.cumsum([len(g) for g in groups], out=g_off[1:])
        k_bytes, k_off = _strings(keys)
        # what a query can need of the gate's arrays: max_groups groups, each a static group or one token
        self.terms_per_query = text.MAX_GATE_GROUPS * max([len(g) for g in groups] + [1])
        self.term_bytes_per_query = text.MAX_GATE_GROUPS * max([sum(len(w) for w in g) for g in groups] + [MAX_TOKEN_BYTES])
        if self.terms_per_query > MAX_TERMS or self.term_bytes_per_query > QUERY_TERM_BYTES:
            raise ValueError("text.py's gate groups do not fit the gate kernel's limits")
        h = C.c_void_p()
        _lib.check(lib.rr_query_create(self.device, _lib.ptr(v_bytes), _lib.ptr(v_off), len(v_off) - 1, _lib.ptr(s_bytes),
                                       _lib.ptr(s_off), len(stop), _lib.ptr(t_bytes), _lib.ptr(t_off), _lib.ptr(g_off), n_colors,
                                       len(groups) - n_colors, _lib.ptr(k_bytes), _lib.ptr(k_off), text.MAX_GATE_GROUPS,
                                       text.MIN_KEYWORD_LEN, C.byref(h)), "rr_query_create")
        self._h = h
        self.wp = None
        if rerank_tokenizer is not None:
            if self.max_length < 3:
                raise ValueError(f"max_length {self.max_length} leaves no room for [CLS] [SEP] [SEP]")
            from .embed import DeviceWordPiece
            self.wp = DeviceWordPiece(rerank_tokenizer, self.device)
        self.encoder, self.enc_wp = None, None
        if encoder is not None:
            from .cross_encoder import QueryEncoder
            from .embed import DeviceWordPiece
            if not isinstance(encoder, QueryEncoder) or encoder.tokenizer is None:
                raise ValueError("the query vectors need this package's QueryEncoder with a tokenizer")
            if encoder.model.device != self.device:
                raise ValueError(f"the encoder is on device {encoder.model.device}, the query front on {self.device}")
            if encoder.max_length < 2:
                raise ValueError(f"encoder.max_length {encoder.max_length} leaves no room for [CLS] [SEP]")
            if max(encoder.tokenizer.vocab.values()) >= encoder.model.vocab:
                raise ValueError("the tokenizer's vocabulary has ids beyond the encoder's embedding table")
            self.enc_wp = DeviceWordPiece(encoder.tokenizer, self.device)
            self.encoder = encoder

    def front(self, queries: Sequence, penalty=0.5, vectors: bool = True) -> QueryFront:
        """Queues the front end of ``queries`` (str, or UTF-8 bytes) on the current stream: one pinned buffer with the
        offsets, the gate's factor table (``penalty``: one, or one per query) and the bytes, ONE copy to the device, the
        WordPiece kernels (with a reranker), rr_query_front_dev and rr_query_strip_dev.  Nothing is read back.

        With an encoder (and ``vectors``) the query vectors are queued as well: the encoder's WordPiece kernels FIRST, so that
        the two host integers the forward's launch needs -- the token count and the longest sequence -- travel back while
        the kernels above run; they are waited for once (the only wait), then come the forward, rr_query_flag_dev and
        rr_query_vectors_dev.  The fp32-mode forward writes NaN rows when an activation leaves fp16's range: ask
        `redo_vectors(front)` once the batch has been waited for."""
        raws = [_utf8(q) for q in queries]
        B = len(raws)
        if B < 1:
            raise ValueError("no queries")
        pens = [float(penalty)] * B if np.isscalar(penalty) else [float(p) for p in penalty]
        if len(pens) != B:
            raise ValueError(f"{len(pens)} penalties for {B} queries")
        off = np.zeros(B + 1, dtype=np.int64)
        np.cumsum([len(r) for r in raws], out=off[1:])
        return self.front_bytes(np.frombuffer(b"".join(raws), dtype=np.uint8), off, pens, vectors)

    def front_bytes(self, raw: np.ndarray, off: np.ndarray, penalties: Sequence[float], vectors: bool = True) -> QueryFront:
        """`front` for bytes and int64 offsets that are already packed (the offsets are the kernel's to check)."""
        import torch
        from .engine import StagedTerms
        B, total = len(off) - 1, int(raw.size)
        L = self.max_length
        cap_ids = max((total + B) // 2, 1)
        cap_terms, cap_tb = B * self.terms_per_query, B * self.term_bytes_per_query
        cap_rr = max(min(total, B * max(L - 3, 0)), 1) if self.wp is not None else 1
        where, at = {}, 0
        for name, nbytes in (("text_off", 8 * (B + 1)), ("factor", 4 * B * (MAX_GROUPS + 1)), ("text", total),
                             ("counts", 16 * B), ("needs_host", 4 * B), ("ids_off", 4 * (B + 1)), ("ids", 4 * cap_ids),
                             ("term_off", 4 * (cap_terms + 1)), ("term_group", 4 * cap_terms), ("q_term", 4 * (B + 1)),
                             ("q_groups", 4 * B), ("term_bytes", cap_tb), ("rr_off", 4 * (B + 1)), ("rr_ids", 4 * cap_rr)):
            where[name] = at
            at += (max(nbytes, 1) + 15) // 16 * 16
            if name == "text":
                n_in = at
        dev = torch.device("cuda", self.device)
        stage = torch.empty(n_in, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        host[:8 * (B + 1)] = np.ascontiguousarray(off, dtype=np.int64).view(np.uint8)
        factor = np.stack([factor_table(p) for p in penalties]) if len(set(penalties)) > 1 else \
            np.broadcast_to(factor_table(penalties[0]), (B, MAX_GROUPS + 1))
        host[where["factor"]:where["factor"] + 4 * B * (MAX_GROUPS + 1)] = np.ascontiguousarray(factor, dtype=np.float32).view(np.uint8).reshape(-1)
        host[where["text"]:where["text"] + total] = raw
        lib = _lib.load()
        with torch.cuda.device(dev):
            buf = torch.empty(at, dtype=torch.uint8, device=dev)
            buf[:n_in].copy_(stage, non_blocking=True)
            base = buf.data_ptr()
            p = lambda name: C.c_void_p(base + where[name])
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            d_off = buf[:8 * (B + 1)].view(torch.int64)
            enc = None
            if self.encoder is not None and vectors:
                Le = self.encoder.max_length
                e_packed, e_info, _, e_cap, _ = self.enc_wp.queue_dev(base + where["text"], total, d_off, Le,
                                                                      min(B * Le, total + 2 * B))
                e_ready = torch.cuda.Event()
                e_ready.record(torch.cuda.current_stream(dev))
                enc = {"packed": e_packed, "info": e_info, "cap": e_cap}
            wp_out = None
            if self.wp is not None:
                cap = min(B * L, total + 2 * B)
                packed, _info, _, cap, _ = self.wp.queue_dev(base + where["text"], total, d_off, L, cap)
                wp_out = packed
                wp_cu, wp_needs = C.c_void_p(packed.data_ptr() + 12 * cap), C.c_void_p(packed.data_ptr() + 4 * (3 * cap + B + 1))
            else:
                wp_cu = wp_needs = None
            _lib.check(lib.rr_query_front_dev(self._h, p("text"), total, p("text_off"), B, wp_cu, wp_needs, L, p("counts"),
                                              p("needs_host"), p("ids"), p("ids_off"), cap_ids, p("term_off"), p("term_group"),
                                              p("q_term"), p("q_groups"), p("term_bytes"), cap_terms, cap_tb, st),
                       "rr_query_front_dev")
            rerank_staged = None
            if self.wp is not None:
                _lib.check(lib.rr_query_strip_dev(self._h, C.c_void_p(packed.data_ptr()), wp_cu, cap, B, p("counts"), p("rr_off"),
                                                  p("rr_ids"), cap_rr, st), "rr_query_strip_dev")
                rerank_staged = (buf[where["rr_off"]:where["rr_ids"] + 4 * cap_rr].view(torch.int32),
                                 (where["rr_ids"] - where["rr_off"]) // 4)
            i32 = lambda name, count: buf[where[name]:where[name] + 4 * count].view(torch.int32)
            terms = StagedTerms(i32("ids", cap_ids), i32("ids_off", B + 1), None, cap_ids if total else 0)
            qvecs = None
            if enc is not None:
                e_ready.synchronize()                  # the one read-back: the token count and the longest sequence
                h = enc["info"].numpy()
                enc["n_tokens"], enc["max_len"] = int(h[0]), int(h[B + 1])
                _lib.check(lib.rr_query_flag_dev(C.c_void_p(e_packed.data_ptr() + 4 * (3 * e_cap + B + 1)), B, FLAG_ENCODER,
                                                 p("needs_host"), st), "rr_query_flag_dev")
                qvecs = self._vectors(enc, B, i32("needs_host", B))
        return QueryFront(B, terms, (buf, where), rerank_staged, i32("needs_host", B), L,
                          {"buf": buf, "where": where, "stage": stage, "wp": wp_out, "enc": enc}, qvecs)

    def _vectors(self, enc: dict, B: int, needs_host, out=None):
        """The forward over the encoder's packed ids and numpy's normalisation, queued on the current stream.  ``narrow``
        records which kernels THIS launch ran on (embed._embed_into does the same): it decides the redo."""
        model = self.encoder.model
        tok, typ, pos, cu = self.enc_wp.views(enc["packed"], B, enc["cap"], enc["n_tokens"])
        enc["narrow"] = model.precision == "fp32" and not model.wide_range
        rows = self.encoder.encode_dev(tok, typ, pos, cu, B, enc["max_len"])
        out = rows if out is None else out             # (in place: a row is read in full before it is written)
        import torch
        _lib.check(_lib.load().rr_query_vectors_dev(C.c_void_p(rows.data_ptr()), B, rows.shape[1], VECTOR_EPS,
                                                    C.c_void_p(needs_host.data_ptr()), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)),
                   "rr_query_vectors_dev")
        return out

    def redo_vectors(self, front: QueryFront) -> bool:
        """After the batch of ``front`` has been waited for: when its forward ran on the fp16-pair kernels and met an
        activation beyond fp16's range (``encoder.model.out_of_range()``; its pooled rows, and so ``front.qvecs``, are NaN), the
        handle is switched to the wide-range kernels as `BertEncoderGPU.forward_ids` switches it (``set_wide_range``), the
        forward and the normalisation are queued again INTO ``front.qvecs`` and True is returned: the caller searches the
        batch again.  False (and nothing queued) otherwise."""
        enc = front._keep.get("enc")
        if enc is None or not enc["narrow"] or not self.encoder.model.out_of_range():
            return False
        self.encoder.model.set_wide_range(True)
        import torch
        with torch.cuda.device(front.qvecs.device):
            self._vectors(enc, front.n_queries, front.needs_host, out=front.qvecs)
        return True

    def check(self) -> None:
        """Raises ValueError when a batch since the last check had offsets that decrease or leave the text, or a store that
        did not fit its buffer (waits for the device)."""
        bad = C.c_int32()
        _lib.check(_lib.load().rr_query_status(self._h, C.byref(bad)), "rr_query_status")
        if self.wp is not None:
            self.wp.check()
        if self.enc_wp is not None:
            self.enc_wp.check()

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_query_destroy(self._h)
            self._h = None
        if getattr(self, "wp", None) is not None:
            self.wp.close()
            self.wp = None
        if getattr(self, "enc_wp", None) is not None:
            self.enc_wp.close()
            self.enc_wp = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
