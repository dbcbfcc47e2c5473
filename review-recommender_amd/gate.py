"""The attribute gate on the GPU (csrc/rr_gate.hip), and the two kernels' model on the CPU.

Stands in for `calculate_gate_factor` as run_search calls it (app/app_product_search.py:297-302, app/test.py:292-297): a
group of terms hits when any of its terms occurs in ``agg_text[:6000].lower()``, the factor is ``penalty ** groups missed``.

`GateText` is the gate plane of an index on the device: per product the byte image of its first 6000 code points in which
every ASCII string occurs exactly when it occurs in ``text[:6000].lower()``.  `pack_groups` turns a batch's gate groups into
the arrays the match kernel reads, and the factor table.  `model_gate_plane` / `model_gate_hits` state in plain Python what
the two kernels compute, as textprep.model_clean and products.model_build_products do for theirs.

The image, byte by byte over the UTF-8 text: A-Z -> a-z; C4 B0 (U+0130) -> 69 B0, because lower() gives 'i' + U+0307;
E2 84 AA (U+212A KELVIN SIGN) -> 6B, because lower() gives 'k'; every other byte stays (the bytes of every other non-ASCII
character are >= 0x80).  FOLDS_TO_ASCII names the two: the only code points outside ASCII whose lower() holds an ASCII
character (tests/test_gate_model.py derives the list from this Python's str.lower()).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _lib

MAX_CHARS = 6000            # app/app_product_search.py:299, app/test.py:294: agg_text[:6000]
PLANE_STEP = 4096           # rr_gate_limits (GateText checks these against the library): bytes of a document per step of the
MATCH_STEP = 1024           # plane kernels, bytes of an image per step of a wave of the match,
PER_THREAD = 16             # consecutive bytes per thread,
MAX_TERM_BYTES = 64         # the longest term,
QUERY_TERM_BYTES = 1024     # term bytes per query,
MAX_TERMS = 64              # terms per query,
SLACK = 16                  # readable bytes behind the plane's last image
MAX_GROUPS = 6              # text.MAX_GATE_GROUPS: the factor table has MAX_GROUPS + 1 entries
STAGE_BYTES = 64 << 20
FOLDS_TO_ASCII = {0x130: "i\u0307", 0x212A: "k"}

_KELVIN, _IDOT = b"\xe2\x84\xaa", b"\xc4\xb0"            # U+212A, U+0130
_LOWER = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))
_IS_LEAD = bytes(0 if (c & 0xC0) == 0x80 else 1 for c in range(256))


def _utf8(text) -> bytes:
    return bytes(text) if isinstance(text, (bytes, bytearray)) else str(text).encode("utf-8", "surrogatepass")


def model_gate_plane(text, max_chars: int = MAX_CHARS) -> bytes:
    """What rr_gate_measure_dev / rr_gate_write_dev make of one document (a str, or its UTF-8 bytes)."""
    raw = _utf8(text)
    if len(raw) > max_chars:                       # the first byte of code point max_chars + 1, if there is one
        leads = np.flatnonzero(np.frombuffer(raw.translate(_IS_LEAD), dtype=np.uint8))
        if len(leads) > max_chars:
            raw = raw[:int(leads[max_chars])]
    return raw.replace(_KELVIN, b"k").replace(_IDOT, b"i\xb0").translate(_LOWER)


def _term_bytes(term: str) -> bytes:
    b = _utf8(term)
    if not b:
        raise ValueError("a gate term of length zero")
    return b


def model_gate_hits(plane: bytes, groups: Sequence[Sequence[str]]) -> int:
    """What rr_gate_factors_dev answers in d_hits for one candidate: bit g is set when a term of group g occurs in the
    image.  The terms are ASCII (the kernel's contract: only for those does the image decide what lower() would)."""
    hits = 0
    for g, terms in enumerate(groups):
        for t in terms:
            b = _term_bytes(t)
            if max(b) >= 0x80:
                raise ValueError(f"gate term {t!r} is not ASCII: the host function decides it")
            if b in plane:
                hits |= 1 << g
                break
    return hits


def factor_table(penalty: float, dtype=np.float32) -> np.ndarray:
    """[MAX_GROUPS + 1]: entry m = the factor of m missed groups, with calculate_gate_factor's own arithmetic (a Python
    float, ``factor *= penalty`` left to right), then ONE cast to float32: what the frame's `_gate` column holds.
    dtype=np.float64 keeps the Python floats."""
    out = np.empty(MAX_GROUPS + 1, dtype=dtype)
    factor = 1.0
    for m in range(MAX_GROUPS + 1):
        out[m] = factor
        factor *= penalty
    return out


class PackedGroups:
    """A batch's gate groups as the match kernel reads them (include/rr_hip.h: rr_gate_factors_dev): ``term_bytes`` uint8,
    ``term_off`` int32 [T + 1], ``term_group`` int32 [T], ``q_term`` int32 [B + 1], ``q_groups`` int32 [B], ``factor``
    float32 (B, 7).  ``host_queries``: the queries that exceed a limit of the kernel (more than MAX_GROUPS groups, MAX_TERMS
    terms or QUERY_TERM_BYTES term bytes, a term longer than MAX_TERM_BYTES or not ASCII); they are packed with no groups
    and must be gated by the host function.  ``any_groups``: whether the kernel has anything to match."""

    def __init__(self, term_bytes, term_off, term_group, q_term, q_groups, factor, host_queries):
        self.term_bytes, self.term_off, self.term_group = term_bytes, term_off, term_group
        self.q_term, self.q_groups, self.factor, self.host_queries = q_term, q_groups, factor, list(host_queries)
        self.n_queries = len(q_groups)
        self.any_groups = bool(q_groups.any())

    _FIELDS = ("term_off", "term_group", "q_term", "q_groups", "factor", "term_bytes")

    def buffer(self):
        """(one uint8 array with the six arrays, 16-byte aligned each, {name: offset})."""
        at, where = 0, {}
        for name in self._FIELDS:
            where[name] = at
            at += (max(getattr(self, name).nbytes, 1) + 15) // 16 * 16
        buf = np.zeros(at, dtype=np.uint8)
        for name in self._FIELDS:
            a = np.ascontiguousarray(getattr(self, name)).view(np.uint8).reshape(-1)
            buf[where[name]:where[name] + a.size] = a
        return buf, where


def pack_groups(groups_per_query: Sequence[Sequence[Sequence[str]]], penalties) -> PackedGroups:
    """groups_per_query[q] = the query's gate groups (text.build_gate_groups: sets of terms; a set's terms are packed in
    sorted order), penalties = one gate penalty or one per query.  A zero-length term is refused (ValueError)."""
    B = len(groups_per_query)
    pens = [float(penalties)] * B if np.isscalar(penalties) else [float(p) for p in penalties]
    if len(pens) != B:
        raise ValueError(f"{len(pens)} penalties for {B} queries")
    blobs: List[bytes] = []
    lens: List[int] = []
    tgroup: List[int] = []
    q_term = np.zeros(B + 1, dtype=np.int32)
    q_groups = np.zeros(B, dtype=np.int32)
    factor = np.empty((B, MAX_GROUPS + 1), dtype=np.float32)
    host: List[int] = []
    for q, groups in enumerate(groups_per_query):
        factor[q] = factor_table(pens[q])
        terms = [(g, _term_bytes(t)) for g, grp in enumerate(groups) for t in sorted(grp)]
        over = (len(groups) > MAX_GROUPS or len(terms) > MAX_TERMS or sum(len(b) for _, b in terms) > QUERY_TERM_BYTES
                or any(len(b) > MAX_TERM_BYTES or max(b) >= 0x80 for _, b in terms))
        if over:
            host.append(q)
        else:
            q_groups[q] = len(groups)
            for g, b in terms:
                blobs.append(b)
                lens.append(len(b))
                tgroup.append(g)
        q_term[q + 1] = len(lens)
    term_off = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=term_off[1:])
    return PackedGroups(np.frombuffer(b"".join(blobs), dtype=np.uint8), term_off, np.asarray(tgroup, dtype=np.int32), q_term,
                        q_groups, factor, host)


class GateText:
    """The gate plane of one index on one GPU: ``d_plane`` uint8 (the images back to back + SLACK bytes), ``d_off`` int64
    [n + 1], ``n`` documents, ``plane_bytes``; document i is the product of global row ``row_offset + i``."""

    def __init__(self, device: int = 0, row_offset: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the gate plane lives on the device only")
        lib = _lib.load()
        lim = [C.c_int32() for _ in range(7)]
        _lib.check(lib.rr_gate_limits(*[C.byref(v) for v in lim]), "rr_gate_limits")
        if tuple(v.value for v in lim) != (PLANE_STEP, MATCH_STEP, PER_THREAD, MAX_TERM_BYTES, QUERY_TERM_BYTES, MAX_TERMS, SLACK):
            raise _lib.HipLibraryError("gate.py and csrc/rr_gate.hip disagree on the kernels' limits")
        self.device = getattr(device, "index", device) or 0
        self.row_offset = int(row_offset)
        h = C.c_void_p()
        _lib.check(lib.rr_gate_create(self.device, C.byref(h)), "rr_gate_create")
        self._h = h
        self.d_plane = self.d_off = None
        self.n = self.plane_bytes = 0

    # ------------------------------------------------------------------ building
    def _build(self, d_text, text_bytes: int, d_off, n: int, max_chars: int, max_bytes: Optional[int]) -> "GateText":
        import torch
        lib = _lib.load()
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            p_text = C.c_void_p(d_text.data_ptr() if text_bytes else None)
            self.d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            d_total = torch.zeros(1, dtype=torch.int64, device=dev)
            _lib.check(lib.rr_gate_measure_dev(self._h, p_text, int(text_bytes), C.c_void_p(d_off.data_ptr()), n, int(max_chars),
                                               C.c_void_p(self.d_off.data_ptr()), C.c_void_p(d_total.data_ptr()), st),
                       "rr_gate_measure_dev")
            total = int(d_total.item())                    # the only number read back: it sizes the plane
            if max_bytes is not None and total + SLACK > max_bytes:
                raise MemoryError(f"the gate plane of {n} products needs {total + SLACK} bytes of device memory, more than the "
                                  f"{max_bytes} allowed: use gate=\"host\" (or raise max_bytes)")
            self.d_plane = torch.empty(total + SLACK, dtype=torch.uint8, device=dev)
            self.d_plane[total:].zero_()
            _lib.check(lib.rr_gate_write_dev(self._h, p_text, int(text_bytes), C.c_void_p(d_off.data_ptr()), n, int(max_chars),
                                             C.c_void_p(self.d_off.data_ptr()), C.c_void_p(self.d_plane.data_ptr()), total, st),
                       "rr_gate_write_dev")
            self.n, self.plane_bytes = int(n), total
            self.check()                                   # (waits: the text may be dropped after this)
        return self

    @classmethod
    def from_texts(cls, texts: Sequence[str], device: int = 0, *, stage_bytes: int = STAGE_BYTES, max_chars: int = MAX_CHARS,
                   max_bytes: Optional[int] = None, row_offset: int = 0) -> "GateText":
        """From a column of str.  Only the first ``max_chars`` characters of a text are encoded and uploaded (in row blocks
        through two pinned buffers, embed._stage_rows); the raw heads are dropped once the plane is written.
        ``max_bytes``: refuse (MemoryError) a plane that needs more device memory than this -- up to 4 bytes per character,
        6 KB per product of ASCII text: 60 GB at 10M products."""
        import torch
        from .embed import _stage_rows, _utf8_column
        self = cls(device, row_offset)
        raw, off = _utf8_column([t[:max_chars] for t in texts])
        n, total = len(off) - 1, int(off[-1])
        if max_bytes is not None and total > 3 * max_bytes:    # (an image is never shorter than a third of its text)
            raise MemoryError(f"{total} bytes of text cannot give a gate plane of at most {max_bytes} bytes: use gate=\"host\"")
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_text = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)
            _stage_rows(raw, off, d_text, torch.cuda.current_stream(dev), stage_bytes, lambda a, b: None)
            return self._build(d_text, total, d_off, n, max_chars, max_bytes)

    @classmethod
    def from_device(cls, text, *, max_chars: int = MAX_CHARS, max_bytes: Optional[int] = None, row_offset: int = 0) -> "GateText":
        """From a products.DeviceProductText (agg_text where rr_products_concat_dev wrote it): no host copy."""
        self = cls(text.device, row_offset)
        return self._build(text.d_text, text.text_bytes, text.d_off, text.n, max_chars, max_bytes)

    # ------------------------------------------------------------------ matching
    def upload(self, packed: PackedGroups):
        """The packed groups on the device: (uint8 tensor, offsets of its arrays).  One copy."""
        import torch
        buf, where = packed.buffer()
        return torch.from_numpy(buf).to(torch.device("cuda", self.device)), where

    def factors(self, rows, packed: PackedGroups, staged=None, want_hits: bool = False, out=None):
        """rr_gate_factors_dev on the current stream: ``rows`` (B, pool) int64 device tensor of global rows ->
        float32 (B, pool) gate factors on the device (and the int32 hit masks with ``want_hits``).  ``staged``: what
        `upload(packed)` returned, when the caller uploaded ahead of the kernels in front of this one.  ``out``: a contiguous
        float32 (B, pool) device tensor to write the factors into (e.g. the gate column of a shard payload)."""
        import torch
        B, pool = rows.shape
        if B != packed.n_queries:
            raise ValueError(f"{packed.n_queries} packed queries for {B} rows of candidates")
        if not rows.is_contiguous() or rows.dtype != torch.int64:
            raise ValueError("rows must be a contiguous int64 tensor")
        d_buf, where = staged if staged is not None else self.upload(packed)
        if out is not None and (out.shape != rows.shape or out.dtype != torch.float32 or not out.is_contiguous()
                                or out.device != rows.device):
            raise ValueError("out must be a contiguous float32 tensor of the rows' shape, on their device")
        gate = out if out is not None else torch.empty((B, pool), dtype=torch.float32, device=rows.device)
        hits = torch.empty((B, pool), dtype=torch.int32, device=rows.device) if want_hits else None
        at = lambda name: C.c_void_p(d_buf.data_ptr() + where[name])
        _lib.check(_lib.load().rr_gate_factors_dev(
            self._h, C.c_void_p(self.d_plane.data_ptr()), C.c_void_p(self.d_off.data_ptr()), self.plane_bytes, self.n,
            self.row_offset, C.c_void_p(rows.data_ptr()), B, pool, at("term_bytes"), at("term_off"), at("term_group"),
            at("q_term"), at("q_groups"), at("factor"), C.c_void_p(gate.data_ptr()),
            C.c_void_p(hits.data_ptr()) if want_hits else None,
            C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)), "rr_gate_factors_dev")
        return (gate, hits) if want_hits else gate

    def gate(self, rows, packed: PackedGroups, gate_host=None, staged=None, out=None):
        """`factors`, and for the queries the kernel cannot hold (``packed.host_queries``) their rows of the gate tensor from
        ``gate_host(b, rows[b] as numpy) -> (pool,) float32``: only then are the candidate rows copied to the host."""
        import torch
        gate = self.factors(rows, packed, staged, out=out)
        if packed.host_queries:
            if gate_host is None:
                raise ValueError(f"queries {packed.host_queries} exceed the gate kernel's limits and no gate_host was given")
            rows_h = rows.cpu().numpy()
            for b in packed.host_queries:
                g = np.ascontiguousarray(gate_host(b, rows_h[b]), dtype=np.float32).reshape(rows.shape[1])
                gate[b].copy_(torch.from_numpy(g))
        return gate

    def check(self) -> None:
        """Raises ValueError when a call since the last check refused a document, a candidate row or a query's packing
        (waits for the device)."""
        bad = C.c_int32()
        _lib.check(_lib.load().rr_gate_status(self._h, C.byref(bad)), "rr_gate_status")

    @property
    def nbytes(self) -> int:
        """Device memory the plane holds."""
        return 0 if self.d_plane is None else int(self.d_plane.numel() + 8 * self.d_off.numel())

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_gate_destroy(self._h)
            self._h = None
        self.d_plane = self.d_off = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
