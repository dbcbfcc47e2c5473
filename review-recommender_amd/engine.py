"""The drop-in search engine: the reference's Python call boundary over the HIP kernels.

Boundary kept:
  cosine_similarity_search(query_vector, embeddings_matrix, top_k)   utils.py:111-124
  run_search(query, k, rerank_k, w_dense, w_bm25, w_rerank, w_prior, w_best, prior_C,
             use_snips, max_scan, min_reviews, gate_penalty)
             -> (DataFrame, snips, dbg)                 app/app_product_search.py:245-317
  search(query, k, alpha)                               north-star sugar over run_search
  CLI flavour (pool floor 100, no trust factor)         app/test.py:228-342

Per query batch the device does K1 (dense scan + exact top-pool), K2 (BM25 at the
pool), K3 (min-max, priors, trust, blend, gate, top-k) back to back on one HIP stream;
the host only tokenises and builds the result frame.  The attribute gate is matched on the device between K2 and K3
(gate="device": gate.py, csrc/rr_gate.hip) or, by default, by the host function between the two; the reranker's pairs are
assembled and scored on the device (rerank="device": rerank.py, csrc/rr_pairs.hip) or, by default, by `predict` on the host.
torch is used for device buffers and streams only.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _lib, text
from .bm25 import BM25Corpus, BM25Index, build_bm25_index_ids, factorize_corpus
from .index import MAX_POOL, ProductIndex

APP_POOL_FLOOR = 150    # app/app_product_search.py:253
CLI_POOL_FLOOR = 100    # app/test.py:238
APP_TRUST_SAT = 80      # app/app_product_search.py:303
COLUMN_NAMES = ("_dense", "_bm25", "_prior", "_rerank", "_best", "_gate", "_trust", "_final")
_FLOAT32_COLUMNS = {"_dense", "_bm25", "_best", "_gate", "_trust", "_final"}


@dataclass
class FusionWeights:
    """run_search's scoring parameters (defaults: config.py:64-72, prior_C app/...:402)."""
    w_dense: float = 0.55
    w_bm25: float = 0.20
    w_rerank: float = 0.20
    w_prior: float = 0.20
    w_best: float = 0.10
    prior_C: float = 20.0
    min_reviews: int = 8
    gate_penalty: float = 0.5
    trust_sat: int = APP_TRUST_SAT
    apply_trust: bool = True


@dataclass
class BatchResult:
    """Raw result of one query batch (numpy, host)."""
    pool_rows: np.ndarray      # (B, pool) global rows in pool order (dense desc, row asc)
    columns: np.ndarray        # (B, 8, pool) float64: COLUMN_NAMES
    order: np.ndarray          # (B, k) pool positions of the top-k, best first
    dense_raw: np.ndarray      # (B, pool) float32 raw cosine scores
    bm25_raw: np.ndarray       # (B, pool) float32 raw BM25 scores
    pool: int
    k: int
    best_ids: Optional[np.ndarray] = None    # (B, pool) best review id per candidate, -1 = none
    best_raw: Optional[np.ndarray] = None    # (B, pool) its raw score
    needs_host: Optional[np.ndarray] = None  # (B,) with query_front: the queries the front end handed back (querytext.FLAG_*)

    def topk_rows(self) -> np.ndarray:
        return np.take_along_axis(self.pool_rows, self.order.astype(np.int64), axis=1)

    def topk_column(self, name: str) -> np.ndarray:
        c = self.columns[:, COLUMN_NAMES.index(name), :]
        return np.take_along_axis(c, self.order.astype(np.int64), axis=1)


@dataclass
class DeviceBatch:
    """One query batch's answer where the kernels left it (HybridSearcher.search_batch_dev): BatchResult's fields as tensors
    on the searcher's device.  Nothing has been waited for."""
    device: object
    pool_rows: object          # (B, pool) int64
    columns: object            # (B, 8, pool) float64
    order: object              # (B, k) int32
    dense_raw: object          # (B, pool) float32
    bm25_raw: object           # (B, pool) float32
    pool: int
    k: int
    best_ids: object = None    # (B, pool) int32, with reviews
    best_raw: object = None    # (B, pool) float32, with reviews
    needs_host: object = None  # (B,) int32, with a query front

    def download(self) -> BatchResult:
        """The copy to the host `search_batch` ends with."""
        with _torch().cuda.device(self.device):
            res = BatchResult(self.pool_rows.cpu().numpy(), self.columns.cpu().numpy(), self.order.cpu().numpy(),
                              self.dense_raw.cpu().numpy(), self.bm25_raw.cpu().numpy(), self.pool, self.k)
            if self.best_ids is not None:
                res.best_ids, res.best_raw = self.best_ids.cpu().numpy(), self.best_raw.cpu().numpy()
            if self.needs_host is not None:
                res.needs_host = self.needs_host.cpu().numpy()
        return res


def _torch():
    import torch
    return torch


# RR_NO_KERNEL_COPY=1 (A/B): the batch's small transfers as copy commands (hipMemcpyAsync) instead of through
# rr_copy_segments_dev / K1 reading pinned queries
_KERNEL_COPIES = os.environ.get("RR_NO_KERNEL_COPY") is None


class StagedTerms:
    """Token ids of a batch already on the device (HybridSearcher.stage_batch)."""
    __slots__ = ("ids", "off", "slot", "n_ids")

    def __init__(self, ids, off, slot, n_ids):
        self.ids, self.off, self.slot, self.n_ids = ids, off, slot, int(n_ids)


class StagedBatch:
    """One batch's inputs on the device: ``q`` (B, dim) float32, ``terms`` (StagedTerms or None), ``ready`` (event)."""
    __slots__ = ("q", "terms", "ready", "slot")

    def __init__(self, q, terms, ready, slot):
        self.q, self.terms, self.ready, self.slot = q, terms, ready, slot


def check_columns(B: int, w: FusionWeights, gate_text, rerank_text, gate_fn, gate_groups, gate_host, rerank_fn, rerank_pairs,
                  query_front=None):
    """The checks of a batch's gate / rerank arguments against the searcher's planes, before any launch or collective (on row
    shards every rank computes the same tests on the same batch, so no rank is left waiting in a collective the others never
    join).  ``gate_text``: the gate plane of the searcher's own rows; ``rerank_text``: the token plane of every row a merged
    pool can hold (sharded.exchange_plane on row shards).  Returns the batch's gate.PackedGroups, or None when there is
    nothing to match (no gate, as with gate_fn=None).  ``query_front`` (a querytext.QueryFront): the batch's groups and
    packed queries are already on the device; its sizes are checked and it is returned in the PackedGroups' place when the
    searcher has a gate plane and no gate_fn was given (which of its queries have groups is not known on the host)."""
    packed = None
    if query_front is not None:
        if gate_groups is not None or (rerank_pairs is not None and rerank_pairs[1] is not None):
            raise ValueError("pass either query_front or gate_groups / packed queries in rerank_pairs")
        if query_front.n_queries != B:
            raise ValueError(f"a query front of {query_front.n_queries} queries for {B} queries")
        if gate_text is not None and gate_fn is None:
            packed = query_front
    if gate_groups is not None:
        from .gate import pack_groups
        if gate_fn is not None:
            raise ValueError("pass either gate_fn or gate_groups")
        if gate_text is None:
            raise ValueError("gate_groups need the gate plane of the searcher's rows: HybridSearcher(..., gate_text=GateText...)")
        if len(gate_groups) != B:
            raise ValueError(f"{len(gate_groups)} gate groups for {B} queries")
        packed = pack_groups(gate_groups, w.gate_penalty)
        if packed.host_queries and gate_host is None:
            raise ValueError(f"queries {packed.host_queries} exceed the gate kernel's limits and no gate_host was given")
        if not packed.any_groups and not packed.host_queries:
            packed = None
    if rerank_pairs is not None:
        if rerank_fn is not None:
            raise ValueError("pass either rerank_fn or rerank_pairs")
        if rerank_text is None:
            raise ValueError("rerank_pairs need the token plane of the whole corpus: HybridSearcher(..., rerank_text=RerankText...), "
                             "on row shards ShardedSearcher(..., rerank_text=exchange_plane(...))")
        _, rr_queries, rerank_host = rerank_pairs
        if rr_queries is None:
            rr_queries = query_front
            if rr_queries is None or rr_queries.rerank_staged is None:
                raise ValueError("rerank_pairs without packed queries need a query_front made with a reranker's tokenizer")
        if rr_queries.n_queries != B:
            raise ValueError(f"{rr_queries.n_queries} packed queries for {B} queries")
        if rr_queries.host_queries and rerank_host is None:
            raise ValueError(f"queries {rr_queries.host_queries} exceed the pair kernel's limit and no rerank_host was given")
    return packed


class HybridSearcher:
    """K1 -> K2 -> K3 on one GPU over a ProductIndex (+ optional BM25Index)."""

    def __init__(self, index: ProductIndex, bm25: Optional[BM25Index] = None, gate_text=None, rerank_text=None):
        """``gate_text``: a gate.GateText over the index's rows, for ``search_batch(gate_groups=...)``.
        ``rerank_text``: a rerank.RerankText over the index's rows, for ``search_batch(rerank_pairs=...)``."""
        if not index.has_meta:
            raise ValueError("the index needs metadata (ProductIndex.set_meta) before searching")
        self.index, self.bm25, self.gate_text, self.rerank_text = index, bm25, gate_text, rerank_text
        self.lib = _lib.load()
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the search path runs on the device only")
        self.device = torch.device("cuda", index.device)
        self._stage_slots = [{"host": None, "dev": None, "event": None, "consumed": None} for _ in range(8)]
        self._stage_next = 0
        self._q_slots = [{"dev": None, "free": None} for _ in range(4)]
        self._q_next = 0
        self._in = None                       # input stream of stage_batch (created on first use)
        # the staging rings are shared Python state: one searcher serves every Streamlit session thread (frontend.py), and
        # the C library's per-handle mutex does not cover slot selection / the pinned buffers
        self._ring_lock = threading.RLock()

    # -------------------------------------------------------------- device steps
    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def copy_segments(self, pairs) -> None:
        """ONE kernel launch on the current stream that copies ``src`` into ``dst`` for every (dst, src) pair of tensors
        (at most four; same shape and dtype; contiguous, or 2-D with contiguous rows).  Either side may be a PINNED host
        tensor: the bytes then cross PCIe as the kernel's own loads / stores (rr_copy_segments_dev) instead of as one
        copy command per tensor -- a batch's token ids in, its rows / order / final scores out."""
        segs = (_lib.CopySeg * len(pairs))()
        for i, (dst, src) in enumerate(pairs):
            if dst.shape != src.shape or dst.dtype != src.dtype:
                raise ValueError("copy_segments: shape / dtype mismatch")
            for t in (dst, src):
                if not t.is_cuda and not t.is_pinned():
                    raise ValueError("copy_segments: host tensors must be pinned")
            esz = dst.element_size()
            if dst.is_contiguous() and src.is_contiguous():
                rows, row_bytes, dp, sp = 1, dst.numel() * esz, dst.numel() * esz, dst.numel() * esz
            else:
                if dst.dim() != 2 or dst.stride(1) != 1 or src.stride(1) != 1:
                    raise ValueError("copy_segments: tensors must be contiguous or 2-D with contiguous rows")
                rows, row_bytes = dst.shape[0], dst.shape[1] * esz
                dp, sp = dst.stride(0) * esz, src.stride(0) * esz
            segs[i] = _lib.CopySeg(dst.data_ptr(), src.data_ptr(), row_bytes, rows, dp, sp)
        _lib.check(self.lib.rr_copy_segments_dev(segs, len(pairs), self.device.index, self._stream()), "rr_copy_segments_dev")

    def _pool_pair(self, B: int, pool: int):
        """K1's output pair: fresh (rows int64 (B, pool), scores float32 (B, pool)) device tensors."""
        torch = _torch()
        return (torch.empty((B, pool), dtype=torch.int64, device=self.device),
                torch.empty((B, pool), dtype=torch.float32, device=self.device))

    def dense_pool(self, q_dev, pool: int, out=None, slot: int = 0):
        """K1 on device tensors: (rows int64 (B,pool), scores float32 (B,pool)).  ``q_dev``: (B, dim) float32 on the
        device -- or in PINNED host memory (K1's first kernel then reads the queries over PCIe itself: no copy command).
        ``out`` = (rows, scores) tensors to write into (e.g. views of a shard payload).  ``slot``: the scan slot whose state
        the call uses (rr_dense_topk_slot_dev; 0 unless other batches have scans parked)."""
        B = q_dev.shape[0]
        rows, dense = out if out is not None else self._pool_pair(B, pool)
        _lib.check(self.lib.rr_dense_topk_slot_dev(self.index.handle, int(slot), C.c_void_p(q_dev.data_ptr()), B, pool,
                                                   C.c_void_p(rows.data_ptr()), C.c_void_p(dense.data_ptr()),
                                                   self._stream()), "rr_dense_topk_dev")
        return rows, dense

    def dense_scan(self, q_dev, pool: int, kth: int):
        """Phase 1 of the two-phase K1 of row shards (rr_dense_scan_dev): the scan without its selection.  Returns a
        float32 (B,) device tensor -- per query a lower bound of the score of this shard's kth-best row -- or None when
        the call cannot be split (then use dense_pool)."""
        torch = _torch()
        B = q_dev.shape[0]
        bound = torch.empty((B,), dtype=torch.float32, device=self.device)      # (written in full whenever `applied`)
        applied = C.c_int32(0)
        _lib.check(self.lib.rr_dense_scan_dev(self.index.handle, C.c_void_p(q_dev.data_ptr()), B, pool, int(kth),
                                              C.c_void_p(bound.data_ptr()), C.byref(applied), self._stream()),
                   "rr_dense_scan_dev")
        return bound if applied.value else None

    def dense_select(self, q_dev, pool: int, floor, out=None):
        """Phase 2 (rr_dense_select_dev): the selection of the scan dense_scan left behind, with the floor the shards
        agreed on (float32 (B,) device tensor).  Lists of `pool` rows: see include/rr_hip.h."""
        B = q_dev.shape[0]
        rows, dense = out if out is not None else self._pool_pair(B, pool)
        _lib.check(self.lib.rr_dense_select_dev(self.index.handle, C.c_void_p(q_dev.data_ptr()), B, pool,
                                                C.c_void_p(floor.data_ptr()), C.c_void_p(rows.data_ptr()),
                                                C.c_void_p(dense.data_ptr()), self._stream()), "rr_dense_select_dev")
        return rows, dense

    def dense_scan_slot(self, slot: int, q_dev, pool: int, kth: int = 0, bound_out=None):
        """Phase 1 of the pipelined K1 (rr_dense_scan_slot_dev) on the CURRENT stream: the scan of ``q_dev`` into scan slot
        ``slot`` (0 .. 2).  ``kth`` > 0 (row shards): also the per-query bound of dense_scan, returned as a float32 (B,)
        tensor (``bound_out`` if given); ``kth`` = 0: returns True.  None when the call cannot be split (then use dense_pool)."""
        torch = _torch()
        B = q_dev.shape[0]
        bound = None
        if kth > 0:
            bound = bound_out if bound_out is not None else torch.empty((B,), dtype=torch.float32, device=self.device)
        applied = C.c_int32(0)
        _lib.check(self.lib.rr_dense_scan_slot_dev(self.index.handle, int(slot), C.c_void_p(q_dev.data_ptr()), B, pool, int(kth),
                                                   C.c_void_p(bound.data_ptr()) if kth > 0 else None, C.byref(applied),
                                                   self._stream()), "rr_dense_scan_slot_dev")
        if not applied.value:
            return None
        return bound if kth > 0 else True

    SELECT_LIST, SELECT_RESCORE, SELECT_ORDER = 1, 2, 4        # include/rr_hip.h: RR_SELECT_*

    def dense_select_slot(self, slot: int, B: int, pool: int, floor=None, out=None, parts: int = 7):
        """Phase 2 (rr_dense_select_part_dev) on the CURRENT stream -- which may be another one than the scan's, and another
        one per part (SELECT_LIST | SELECT_RESCORE | SELECT_ORDER): the library orders them with events.  Returns
        (rows, dense) when SELECT_ORDER is among the parts, else None."""
        rows = dense = None
        if parts & self.SELECT_ORDER:
            rows, dense = out if out is not None else self._pool_pair(B, pool)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.lib.rr_dense_select_part_dev(self.index.handle, int(slot), int(parts), B, pool, p(floor), p(rows), p(dense),
                                                     self._stream()), "rr_dense_select_part_dev")
        return (rows, dense) if parts & self.SELECT_ORDER else None

    def bm25_at(self, term_id_lists: Sequence[Sequence[int]], rows_dev, mode: str = "forward", out=None):
        """K2 on device tensors: float32 (B, pool) raw BM25 at the candidate rows."""
        torch = _torch()
        B, pool = rows_dev.shape
        staged = isinstance(term_id_lists, StagedTerms)
        flat_form = isinstance(term_id_lists, tuple) and len(term_id_lists) == 2 and isinstance(term_id_lists[1], np.ndarray)
        empty = (term_id_lists.n_ids == 0) if staged else \
            (len(term_id_lists[0]) == 0) if flat_form else not any(len(t) for t in term_id_lists)
        if self.bm25 is None or empty:
            # no index / no tokens -> zeros (app/app_product_search.py:202,204)
            if out is None:
                return torch.zeros((B, pool), dtype=torch.float32, device=self.device)
            out.zero_()
            return out
        if out is None:
            out = torch.empty((B, pool), dtype=torch.float32, device=self.device)
        ids_dev, off_dev = (term_id_lists.ids, term_id_lists.off) if staged else self._stage_terms(term_id_lists)[:2]
        _lib.check(self.lib.rr_bm25_scores_at_dev(
            self.bm25.handle, C.c_void_p(ids_dev.data_ptr()), C.c_void_p(off_dev.data_ptr()), B,
            C.c_void_p(rows_dev.data_ptr()), pool, {"forward": 0, "postings": 1}[mode],
            C.c_void_p(out.data_ptr()), self._stream()), "rr_bm25_scores_at_dev")
        return out

    def _stage_terms(self, term_id_lists):
        """Token ids of a batch as device arrays (flat ids + offsets), uploaded on every call through a
        small ring of pinned host buffers (one async copy per batch; nothing is cached across calls, so a
        caller may reuse and mutate its lists).  ``term_id_lists`` is a sequence of per-query id
        sequences, or an already flattened ``(ids int32, offsets int32[B+1])`` pair of numpy arrays."""
        torch = _torch()
        if isinstance(term_id_lists, tuple) and len(term_id_lists) == 2 and isinstance(term_id_lists[1], np.ndarray):
            flat = np.ascontiguousarray(term_id_lists[0], dtype=np.int32).reshape(-1)
            off = np.ascontiguousarray(term_id_lists[1], dtype=np.int32).reshape(-1)
        else:
            B = len(term_id_lists)
            off = np.zeros(B + 1, dtype=np.int32)
            np.cumsum([len(t) for t in term_id_lists], out=off[1:])
            flat = (np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for t in term_id_lists])
                    if off[-1] else np.zeros(0, dtype=np.int32))
        n_off, n_ids = off.shape[0], flat.shape[0]
        need = n_off + max(n_ids, 1)
        with self._ring_lock:
            return self._stage_terms_locked(off, flat, n_off, n_ids, need)

    def _stage_terms_locked(self, off, flat, n_off, n_ids, need):
        torch = _torch()
        slot = self._stage_slots[self._stage_next % len(self._stage_slots)]
        self._stage_next += 1
        if slot["host"] is None or slot["host"].numel() < need:
            # (pinning host memory is slow and synchronises: every slot of the ring is sized at once, on first use)
            cap = max(2 * need, 16384)
            torch.cuda.synchronize(self.device)      # (buffers change hands between streams only when nothing is in flight)
            for sl in self._stage_slots:
                if sl["host"] is None or sl["host"].numel() < need:
                    if sl["event"] is not None:
                        sl["event"].synchronize()
                    sl["host"] = torch.empty(cap, dtype=torch.int32).pin_memory()
                    sl["dev"] = torch.empty(cap, dtype=torch.int32, device=self.device)
                    sl["event"] = torch.cuda.Event()
        else:
            slot["event"].synchronize()          # the copy that last used this pinned buffer has finished
        h = slot["host"].numpy()
        h[:n_off] = off
        h[n_off:n_off + n_ids] = flat
        cur = torch.cuda.current_stream(self.device)
        if slot["consumed"] is not None:         # (input stream: the K2 launch that read this device buffer last)
            cur.wait_event(slot["consumed"])
            slot["consumed"] = None
        if _KERNEL_COPIES:
            self.copy_segments([(slot["dev"][:need], slot["host"][:need])])
        else:
            slot["dev"][:need].copy_(slot["host"][:need], non_blocking=True)
        slot["event"].record(cur)
        return slot["dev"][n_off:n_off + max(n_ids, 1)], slot["dev"][:n_off], slot, n_ids

    def stage_batch(self, q_host, term_id_lists=None) -> "StagedBatch":
        """Uploads one batch's inputs on the searcher's INPUT stream: the query vectors (``q_host``: pinned float32
        (B, dim) tensor) into a device buffer of a small ring, the token ids through the pinned staging ring.  The
        caller makes its compute stream wait for ``.ready``, runs the batch with ``.q`` / ``.terms`` and then calls
        ``release(batch)`` (records when the buffers may be overwritten).  With the answer copied back on a third
        stream, batch i + 1's uploads and batch i - 1's downloads run under batch i's kernels instead of between
        them (~90 us per 256-query batch on one stream)."""
        torch = _torch()
        with self._ring_lock:
            return self._stage_batch_locked(q_host, term_id_lists)

    def _stage_batch_locked(self, q_host, term_id_lists):
        torch = _torch()
        if self._in is None:
            self._in = torch.cuda.Stream(device=self.device)
        slot = self._q_slots[self._q_next % len(self._q_slots)]
        self._q_next += 1
        if slot["dev"] is None or slot["dev"].shape != q_host.shape:
            # a fresh block of the caching allocator may still be read by kernels queued on the compute stream (it is
            # free in THAT stream's order only): the input stream must not write it before they have run
            slot["dev"] = torch.empty(tuple(q_host.shape), dtype=torch.float32, device=self.device)
            slot["free"] = torch.cuda.Event()
            slot["free"].record(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._in):
            if slot["free"] is not None:
                self._in.wait_event(slot["free"])
            slot["dev"].copy_(q_host, non_blocking=True)
            terms = None
            if term_id_lists is not None:
                ids, off, tslot, n_ids = self._stage_terms(term_id_lists)
                terms = StagedTerms(ids, off, tslot, n_ids)
            ready = torch.cuda.Event()
            ready.record(self._in)
        return StagedBatch(slot["dev"], terms, ready, slot)

    def release(self, batch: "StagedBatch") -> None:
        """After the batch's kernels are enqueued on the current stream: its buffers are free once they have run."""
        torch = _torch()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        batch.slot["free"] = ev
        if batch.terms is not None:
            batch.terms.slot["consumed"] = ev

    def fuse(self, params: "_lib.FuseParams", B: int, rows, dense, bm25, meta=None,
             rerank=None, best=None, gate=None):
        """K3 on device tensors -> (out_rows (B,pool), cols (B,8,pool) f64, order (B,k))."""
        torch = _torch()
        pool, k = params.pool, params.k
        out_rows = torch.empty((B, pool), dtype=torch.int64, device=self.device)
        cols = torch.empty((B, 8, pool), dtype=torch.float64, device=self.device)
        order = torch.empty((B, k), dtype=torch.int32, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        n, avg, l1p = meta if meta is not None else (None, None, None)
        _lib.check(self.lib.rr_fuse_topk_dev(
            self.index.handle, C.byref(params), B, p(rows), p(dense), p(bm25), p(n), p(avg), p(l1p),
            p(rerank), p(best), p(gate), p(out_rows), p(cols), p(order), self._stream()),
            "rr_fuse_topk_dev")
        return out_rows, cols, order

    # -------------------------------------------------------------- one batch
    @staticmethod
    def make_params(w: FusionWeights, k: int, pool: int, n_candidates: int, rerank_k: int,
                    cand_per_rank: int = 0, stride_bytes: int = 0, bm25_f64: bool = False) -> "_lib.FuseParams":
        return _lib.FuseParams(
            w_dense=w.w_dense, w_bm25=w.w_bm25, w_rerank=w.w_rerank, w_prior=w.w_prior,
            w_best=w.w_best, prior_C=w.prior_C, min_reviews=int(w.min_reviews),
            trust_sat=int(w.trust_sat), apply_trust=int(bool(w.apply_trust)),
            rerank_active=int(rerank_k > 0), rerank_k=int(rerank_k), k=int(k),
            n_candidates=int(n_candidates), pool=int(pool), cand_per_rank=int(cand_per_rank),
            bm25_f64=int(bool(bm25_f64)), cand_rank_stride_bytes=int(stride_bytes))

    def search_batch(self, qvecs: np.ndarray, term_id_lists: Optional[Sequence[Sequence[int]]],
                     k: int, rerank_k: int = 0, weights: Optional[FusionWeights] = None,
                     pool_floor: int = APP_POOL_FLOOR,
                     gate_fn: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                     rerank_fn: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                     bm25_mode: str = "forward", reviews=None, max_scan: int = 0,
                     bm25_f64: bool = False, gate_groups=None,
                     gate_host: Optional[Callable[[int, np.ndarray], np.ndarray]] = None,
                     rerank_pairs: Optional[Tuple] = None, query_front=None,
                     on_queued: Optional[Callable[[], None]] = None) -> BatchResult:
        """qvecs (B, dim) float32: a numpy array (uploaded here), a float32 torch tensor on the searcher's device (read where it
        is), or None with a ``query_front`` that carries ``qvecs`` (QueryText with an encoder): K1 and the best-review pick
        then read that tensor.  term_id_lists: per-query BM25 token ids (None = no BM25).
        gate_fn / rerank_fn map the (B, pool) pool rows to (B, pool) float32 gate factors /
        (B, rr_k) raw reranker scores; they run on the host between K2 and K3.
        ``gate_groups`` (instead of gate_fn): per query its gate groups (text.build_gate_groups); they are matched against
        the searcher's ``gate_text`` on the device (rr_gate_factors_dev, queued between K2 and K3; the penalty is
        ``weights.gate_penalty``) and the rows stay on the device.  A query over a limit of that kernel (gate.pack_groups:
        ``host_queries``) gets its row of the gate tensor from ``gate_host(b, rows[b]) -> (pool,) float32`` instead; only
        then are the rows copied to the host.
        ``rerank_pairs`` (instead of rerank_fn): ``(cross_encoder, packed_queries, rerank_host)`` -- the pairs of the first
        rr_k candidates of every query are assembled from the searcher's ``rerank_text`` and scored on the device
        (RerankText.scores); the (B, pool) rerank tensor, zeros beyond rr_k, goes straight into K3: no row leaves the device
        and no score is uploaded.  A query of more than max_length - 3 tokens (rerank.pack_queries: ``host_queries``) gets
        its rr_k scores from ``rerank_host(b, rows[b, :rr_k]) -> (rr_k,) float32`` instead; only then are the rows copied to
        the host.
        ``query_front`` (instead of term_id_lists, gate_groups and the packed queries of rerank_pairs -- pass
        ``rerank_pairs=(cross_encoder, None, rerank_host)``): a querytext.QueryFront, the batch's query text already on the
        device.  K2 reads its ids, the gate match its groups (when the searcher has a gate plane and no gate_fn is given),
        the pair kernels its query ids.  Its ``needs_host`` flags come back in ``BatchResult.needs_host`` with the answer:
        the rows of a flagged query were computed from an EMPTY query text and are the caller's to replace.
        ``on_queued``: called once when every kernel of the batch is queued, before the answer is waited for.
        ``bm25_f64``: the CLI flavour without a BM25 artefact (float64 zeros column, app/test.py:252)."""
        dev = self.search_batch_dev(qvecs, term_id_lists, k, rerank_k, weights, pool_floor, gate_fn, rerank_fn, bm25_mode,
                                    reviews, max_scan, bm25_f64, gate_groups, gate_host, rerank_pairs, query_front, on_queued)
        return dev.download()

    def search_batch_dev(self, qvecs, term_id_lists, k: int, rerank_k: int = 0, weights: Optional[FusionWeights] = None,
                         pool_floor: int = APP_POOL_FLOOR, gate_fn=None, rerank_fn=None, bm25_mode: str = "forward",
                         reviews=None, max_scan: int = 0, bm25_f64: bool = False, gate_groups=None, gate_host=None,
                         rerank_pairs: Optional[Tuple] = None, query_front=None, on_queued=None,
                         shared: Optional[dict] = None) -> DeviceBatch:
        """`search_batch` up to the download: every kernel of the batch queued, the answer left in device tensors
        (`DeviceBatch`; ``download()`` makes the BatchResult `search_batch` returns).
        ``shared``: a dict that lives as long as ONE batch of queries is searched under several configurations
        (SearchEngine.evaluate).  A stage whose inputs the dict has seen is not run again but read from it: K1 and K2 per
        pool, the best-review column per (pool, max_scan), the gate factors per (pool, gate_penalty), the reranker's scores per
        (pool, rerank_k).  The keys hold everything of THIS call's arguments the stage reads, on the understanding that the
        caller passes the same queries, ``bm25_mode``, ``reviews`` and the same gate / rerank functions with every call that
        shares the dict; K3 always runs.  With None nothing is kept."""
        torch = _torch()
        w = weights or FusionWeights()
        memo = shared if shared is not None else {}
        q = q_dev = None
        if qvecs is None:
            q_dev = getattr(query_front, "qvecs", None)
            if q_dev is None:
                raise ValueError("qvecs=None needs a query_front that carries the query vectors (QueryText with an encoder)")
        elif isinstance(qvecs, torch.Tensor):
            if qvecs.device != self.device or qvecs.dtype != torch.float32:
                raise ValueError(f"a tensor as qvecs must be float32 on {self.device}; got {qvecs.dtype} on {qvecs.device}")
            q_dev = qvecs.contiguous()
        else:
            q = np.ascontiguousarray(qvecs, dtype=np.float32)
        shape = tuple(q.shape if q is not None else q_dev.shape)
        if len(shape) != 2 or shape[1] != self.index.dim:
            raise ValueError(f"qvecs must be (B, {self.index.dim}); got {shape}")
        B = shape[0]
        if k < 1:
            raise ValueError("k must be >= 1")
        pool = min(max(k, rerank_k, pool_floor), self.index.n_rows)
        if pool > MAX_POOL:
            raise ValueError(f"pool {pool} exceeds the kernels' limit {MAX_POOL}")
        k_eff = min(k, pool)
        rr_k = min(rerank_k, pool)
        if query_front is not None and term_id_lists is not None:
            raise ValueError("pass either query_front or term_id_lists")
        packed = check_columns(B, w, self.gate_text, self.rerank_text, gate_fn, gate_groups, gate_host, rerank_fn, rerank_pairs,
                               query_front)

        def once(key, make):
            if key not in memo:
                memo[key] = make()
            return memo[key]

        with torch.cuda.device(self.device):
            if q_dev is None:
                q_dev = once(("q",), lambda: torch.from_numpy(q).to(self.device))
            staged_groups = None
            if ("gate", pool, w.gate_penalty) not in memo:
                if packed is query_front:
                    staged_groups = query_front.gate_staged if packed is not None else None
                else:
                    staged_groups = self.gate_text.upload(packed) if packed is not None else None    # (ahead of the kernels)

            def k1_k2():
                rows, dense = self.dense_pool(q_dev, pool)
                tl = term_id_lists if term_id_lists is not None else [[] for _ in range(B)]
                if query_front is not None and self.bm25 is not None:
                    tl = query_front.terms
                return rows, dense, self.bm25_at(tl, rows, bm25_mode)

            rows, dense, bm = once(("pool", pool), k1_k2)
            gate = rerank = best = None
            best_ids = None
            rows_host = lambda: once(("rows_h", pool), lambda: rows.cpu().numpy())
            if reviews is not None:
                # best review per candidate (csrc/rr_reviews.hip), the whole batch in one call; the
                # reference's iloc[:max_rows] cut is evaluated per query on the device
                def best_review():
                    best = torch.empty((B, pool), dtype=torch.float32, device=self.device)
                    best_ids = torch.empty((B, pool), dtype=torch.int32, device=self.device)
                    _lib.check(self.lib.rr_reviews_best_cut_dev(
                        reviews.handle, C.c_void_p(q_dev.data_ptr()), B, C.c_void_p(rows.data_ptr()), pool,
                        self.index.row_offset, int(max_scan), C.c_void_p(best.data_ptr()),
                        C.c_void_p(best_ids.data_ptr()), self._stream()), "rr_reviews_best_cut_dev")
                    return best, best_ids
                best, best_ids = once(("best", pool, int(max_scan)), best_review)
            if packed is not None:
                gate = once(("gate", pool, w.gate_penalty), lambda: self.gate_text.gate(rows, packed, gate_host, staged_groups))
            if gate_fn is not None:
                def host_gate():
                    g = np.ascontiguousarray(gate_fn(rows_host()), dtype=np.float32)
                    return torch.from_numpy(g).to(self.device)
                gate = once(("gate", pool, w.gate_penalty), host_gate)
            if rerank_fn is not None and rr_k > 0:
                def host_rerank():
                    r = np.zeros((B, pool), dtype=np.float32)
                    r[:, :rr_k] = np.asarray(rerank_fn(rows_host()[:, :rr_k]), dtype=np.float32)
                    return torch.from_numpy(r).to(self.device)
                rerank = once(("rerank", pool, rr_k), host_rerank)
            if rerank_pairs is not None and rr_k > 0:
                def device_rerank():
                    rr_ce, rr_queries, rerank_host = rerank_pairs
                    rerank = torch.zeros((B, pool), dtype=torch.float32, device=self.device)
                    if rr_queries is None:
                        rr_queries = query_front
                        rerank[:, :rr_k] = self.rerank_text.scores(rr_ce, rows, rr_k, rr_queries, staged=query_front.rerank_staged)
                    else:
                        rerank[:, :rr_k] = self.rerank_text.scores(rr_ce, rows, rr_k, rr_queries)
                    if rr_queries.host_queries:
                        rows_h = rows_host()
                        for b in rr_queries.host_queries:
                            r = np.ascontiguousarray(rerank_host(b, rows_h[b, :rr_k]), dtype=np.float32).reshape(rr_k)
                            rerank[b, :rr_k].copy_(torch.from_numpy(r))
                    return rerank
                rerank = once(("rerank", pool, rr_k), device_rerank)
            params = self.make_params(w, k_eff, pool, pool, rr_k, bm25_f64=bm25_f64 and self.bm25 is None)
            out_rows, cols, order = self.fuse(params, B, rows, dense, None if params.bm25_f64 else bm, None,
                                              rerank, best, gate)
            if on_queued is not None:
                on_queued()
        return DeviceBatch(self.device, out_rows, cols, order, dense, bm, pool, k_eff, best_ids, best if best_ids is not None else None,
                           query_front.needs_host if query_front is not None else None)


class SearchEngine:
    """The reference's search API over one GPU.

    meta: DataFrame with ``sku, n_reviews, avg_stars, agg_text`` (+ any other column),
    row-aligned with ``embeddings`` (product_emb_meta.parquet / product_emb.npy).
    bm25_blob: the ``{"skus", "corpus"}`` dict of product_bm25.pkl, or None.
    encoder: object with ``encode([query], normalize_embeddings=True)`` (SentenceTransformer API).
    cross_encoder: object with ``predict(pairs, batch_size=64, show_progress_bar=False)``.
    bm25_build: "device" builds the BM25 index on the GPU (bm25.build_bm25_index), "host" with
    BM25Corpus.from_corpus; the two give bitwise the same index.
    gate: "host" (the default) matches the gate terms with `text.calculate_gate_factor` between K2 and K3; "device" builds a
    gate plane of ``meta["agg_text"]`` on the GPU (gate.GateText, up to 6 KB of device memory per product; ``gate_max_bytes``
    refuses a larger one) and matches there (csrc/rr_gate.hip).  The two give bitwise the same frames.
    rerank: "host" (the default) builds the reranker's pairs as strings and scores them with ``cross_encoder.predict``;
    "device" builds a token plane of ``meta["agg_text"]`` on the GPU (rerank.RerankText, up to about 1 KB of device memory per
    product; ``rerank_max_bytes`` refuses a larger one), assembles the pairs there (csrc/rr_pairs.hip) and leaves the scores
    on the device.  It needs a ``cross_encoder`` that is this package's `CrossEncoder` with a tokenizer.
    query_text: "host" (the default) tokenises the queries, looks their BM25 ids up, builds and packs their gate groups and
    their reranker ids in Python, query by query; "device" stages the batch's bytes once and does all of that on the GPU
    (querytext.QueryText, csrc/rr_query.hip) for the consumers that are on the device (K2; the gate with gate="device"; the
    pairs with rerank="device").  The queries the kernels hand back are searched again through the host functions.  The two
    give bitwise the same frames, snips and dbg.
    query_vectors: "host" (the default) encodes the queries with ``encoder.encode`` (Python WordPiece per query, ids up, pooled
    rows down, numpy's l2 normalisation, vectors up again); "device" makes them in the query front from the staged bytes
    (device WordPiece of the encoder's vocabulary, the forward, rr_query_vectors_dev) and K1 reads them where they are.  It
    needs query_text="device" and an ``encoder`` that is this package's `QueryEncoder` with a tokenizer.  The queries the
    front hands back are encoded with ``encoder.encode``, those only.  The two give bitwise the same frames, snips and dbg.
    """

    def __init__(self, meta: pd.DataFrame, embeddings: np.ndarray, bm25_blob: Optional[dict] = None,
                 *, encoder=None, cross_encoder=None, device: int = 0, normalize: bool = True,
                 flavour: str = "app", dtype: str = "f32", reviews: Optional[Tuple] = None,
                 bm25_build: str = "device", index: Optional[ProductIndex] = None, bm25_ids: Optional[Tuple] = None,
                 gate: str = "host", gate_max_bytes: Optional[int] = None, rerank: str = "host",
                 rerank_max_bytes: Optional[int] = None, query_text: str = "host", query_vectors: str = "host"):
        """``index``: a ready ProductIndex (embed.build_product_embeddings) to use instead of uploading ``embeddings``
        (then None); it is taken as it is -- ``normalize`` and ``dtype`` describe an upload only.
        ``bm25_ids``: ``(skus, tok, doc_off, vocab)`` instead of ``bm25_blob`` -- the corpus as token ids (numpy arrays or
        tensors on ``device``, doctok.DeviceDocTokenizer): what ``factorize_corpus(bm25_blob["corpus"])`` gives."""
        if flavour not in ("app", "cli"):
            raise ValueError("flavour must be 'app' or 'cli'")
        if bm25_build not in ("device", "host"):
            raise ValueError("bm25_build must be 'device' or 'host'")
        if gate not in ("device", "host"):
            raise ValueError("gate must be 'device' or 'host'")
        if rerank not in ("device", "host"):
            raise ValueError("rerank must be 'device' or 'host'")
        if query_text not in ("device", "host"):
            raise ValueError("query_text must be 'device' or 'host'")
        if rerank == "device":
            from .cross_encoder import CrossEncoder
            if not isinstance(cross_encoder, CrossEncoder) or cross_encoder.tokenizer is None:
                raise ValueError("rerank=\"device\" needs a cross_encoder that is this package's CrossEncoder with a tokenizer "
                                 "(its ids are what the token plane holds); any other object is served by rerank=\"host\"")
        if query_vectors not in ("device", "host"):
            raise ValueError("query_vectors must be 'device' or 'host'")
        if query_vectors == "device":
            from .cross_encoder import QueryEncoder
            if query_text != "device":
                raise ValueError("query_vectors=\"device\" needs query_text=\"device\" (the vectors are made from the bytes the "
                                 "query front stages); with query_text=\"host\" the queries are encoded by query_vectors=\"host\"")
            if not isinstance(encoder, QueryEncoder) or encoder.tokenizer is None:
                raise ValueError("query_vectors=\"device\" needs an encoder that is this package's QueryEncoder with a tokenizer "
                                 "(its ids are what the forward reads); any other object is served by query_vectors=\"host\"")
        if (index is None) == (embeddings is None):
            raise ValueError("pass either an embedding matrix or a ready index")
        n_emb = embeddings.shape[0] if index is None else index.n_rows
        if len(meta) != n_emb:
            # app/app_product_search.py:104-107, app/test.py:141-142: hard error
            raise ValueError(f"metadata has {len(meta)} rows but embeddings have "
                             f"{n_emb} rows")
        if "sku" not in meta.columns or "agg_text" not in meta.columns:
            raise ValueError("metadata must have 'sku' and 'agg_text' columns")  # app/test.py:138-139
        from .cross_encoder import QueryEncoder as _QueryEncoder
        idx_dim = embeddings.shape[1] if index is None else index.dim
        if isinstance(encoder, _QueryEncoder) and encoder.hidden != idx_dim:
            raise ValueError(f"the query encoder makes vectors of width {encoder.hidden} but the index has dim {idx_dim}")
        self.flavour = flavour
        self.meta = meta.reset_index(drop=True)
        self.encoder, self.cross_encoder = encoder, cross_encoder
        # chunked upload: the matrix may be a memory-mapped product_emb.npy (app/test.py:140)
        self.index = index if index is not None else ProductIndex.from_rows(embeddings, device=device, normalize=normalize,
                                                                            dtype=dtype)
        nan = pd.Series([np.nan] * len(self.meta))
        n = pd.to_numeric(self.meta.get("n_reviews", nan), errors="coerce").fillna(0).values
        r = pd.to_numeric(self.meta.get("avg_stars", nan), errors="coerce").values
        self.index.set_meta(n, r)
        self._texts = self.meta["agg_text"].astype(str)
        self._bm25_corpus: Optional[BM25Corpus] = None
        self._bm25_source = None
        bm25_index = None
        if bm25_ids is not None:
            if bm25_blob:
                raise ValueError("pass either bm25_blob or bm25_ids")
            if bm25_build != "device":
                raise ValueError("bm25_ids are indexed by the GPU builder: bm25_build must be 'device'")
            skus, tok, off, vocab = bm25_ids
            order = self._align_bm25([str(s) for s in skus])
            bm25_index = build_bm25_index_ids(tok, off, len(vocab), device=device, order=order, vocab=vocab)
            if not isinstance(tok, np.ndarray):            # kept for bm25_corpus on the HOST, as the blob path keeps them:
                tok, off = tok.cpu().numpy(), off.cpu().numpy()    # 4 B per token of device memory is given back
            self._bm25_source = (tok, off, vocab)
        elif bm25_blob:
            order = self._align_bm25([str(s) for s in bm25_blob["skus"]])
            if bm25_build == "device":       # the index built on the GPU (csrc/rr_bm25_build.hip): the same arrays
                # kept for bm25_corpus: the ids (4 B per token, no reference to the blob's token lists)
                tok, off, vocab = factorize_corpus(bm25_blob["corpus"])
                self._bm25_source = (tok, off, vocab)
                bm25_index = build_bm25_index_ids(tok, off, len(vocab), device=device, order=order, vocab=vocab)
            else:
                self._bm25_corpus = BM25Corpus.from_corpus(bm25_blob["corpus"])
                bm25_index = self._bm25_corpus.select(order).to_device(device)
        self.gate = gate
        gate_text = None
        if gate == "device":
            from .gate import GateText
            gate_text = GateText.from_texts(self._texts.tolist(), self.index.device, max_bytes=gate_max_bytes,
                                            row_offset=self.index.row_offset)
        self.rerank = rerank
        rerank_text = None
        if rerank == "device":
            from .rerank import RerankText
            rerank_text = RerankText.from_texts(self._texts.tolist(), cross_encoder.tokenizer, cross_encoder.max_length,
                                                self.index.device, max_bytes=rerank_max_bytes, row_offset=self.index.row_offset)
            rerank_text.check_model(cross_encoder)
        self.searcher = HybridSearcher(self.index, bm25_index, gate_text, rerank_text)
        self.query_text = query_text
        self._query_text = None
        if query_text == "device":
            from .querytext import QueryText
            vocab = {} if bm25_index is None else bm25_index.corpus.vocab      # (None: refused with term_ids' message)
            self._query_text = QueryText(vocab, rerank_tokenizer=cross_encoder.tokenizer if rerank == "device" else None,
                                         max_length=cross_encoder.max_length if rerank == "device" else 512,
                                         device=self.index.device, encoder=encoder if query_vectors == "device" else None)
        self.query_vectors = query_vectors
        # reviews = (frame with sku/text/stars, (n_reviews, dim) embeddings): reviews_with_embeddings.parquet
        self.reviews = None
        if reviews is not None:
            from .reviews import ReviewIndex
            self.reviews = ReviewIndex(reviews[0], reviews[1], self.meta["sku"].astype(str).tolist(), device=device)

    @property
    def bm25_corpus(self) -> Optional[BM25Corpus]:
        """The blob's corpus on the host, in blob order.  When the index was built on the GPU it is made on first use
        from the token ids kept at load (BM25Corpus.from_ids: the arrays from_corpus makes), which are then dropped."""
        if self._bm25_corpus is None and self._bm25_source is not None:
            tok, off, vocab = self._bm25_source
            self._bm25_corpus = BM25Corpus.from_ids(tok, off, len(vocab), vocab=vocab)
            self._bm25_source = None
        return self._bm25_corpus

    @classmethod
    def from_artifacts(cls, data_dir, **kw) -> "SearchEngine":
        """Loads product_emb.npy / product_emb_meta.parquet / product_bm25.pkl from ``data_dir``
        (the reference's data/processed layout, app/test.py:21-26) and l2-normalises the rows on
        the GPU like the reference's loaders do on the host (app/test.py:144)."""
        from .artifacts import load_artifacts, load_reviews
        meta, emb, blob = load_artifacts(data_dir)
        kw.setdefault("normalize", True)
        if "reviews" not in kw:
            kw["reviews"] = load_reviews(data_dir)     # None when reviews_with_embeddings.parquet is absent
        return cls(meta, emb, blob, **kw)

    @classmethod
    def from_products(cls, products, encoder, *, text_col: str = "agg_text", dtype: str = "f32", chunk_tokens: int = 131072,
                      bm25: bool = True, data_dir=None, bm25_tokenize: str = "device", **kw) -> "SearchEngine":
        """The engine straight from a product table (sku, agg_text, ...), no files in between: embeddings by
        embed.build_product_embeddings on the encoder's GPU (nlp/11_build_product_embeddings.py), the BM25 corpus tokenised
        as nlp/12_product_prep.py:80-89 does and indexed by the GPU builder.  ``encoder`` (a QueryEncoder with a vocabulary)
        also becomes the engine's query encoder.  With ``data_dir`` the two embedding files are written as well.
        bm25_tokenize: "device" tokenises ``agg_text`` and numbers the vocabulary on the GPU (doctok.DeviceDocTokenizer),
        "host" with ``build_bm25_blob`` + ``factorize_corpus``; the two give bitwise the same index.  The device tokenizer
        feeds the GPU index builder only: with ``bm25_build="host"`` (the index built by BM25Corpus.from_corpus, which reads
        token lists) the corpus is tokenised on the host whatever ``bm25_tokenize`` says.

        The same engine, bit for bit, as `from_artifacts` on the files this build writes: the loaders l2-normalise the
        stored unit rows once more (app/test.py:144), so this does too (`index.l2_normalize()` after the build).
        dtype="bf16": the order is NORMALISE AGAIN, THEN ROUND, the one `from_artifacts(dtype="bf16")` produces (fp32 rows
        normalised at the build, normalised again at load, rounded once to bf16); the fp32 rows pass through the host once
        for it."""
        from .artifacts import build_bm25_blob
        from .embed import build_product_embeddings
        if bm25_tokenize not in ("device", "host"):
            raise ValueError("bm25_tokenize must be 'device' or 'host'")
        index, meta, _ = build_product_embeddings(products, encoder, text_col=text_col, dtype="f32",
                                                  chunk_tokens=chunk_tokens, data_dir=data_dir)
        if dtype == "f32":
            index.l2_normalize()
        else:
            rows = index.download_rows()
            index.close()
            index = ProductIndex.from_rows(rows, device=encoder.model.device, normalize=True, dtype=dtype)
        kw.setdefault("device", encoder.model.device)
        if bm25 and bm25_tokenize == "device" and kw.get("bm25_build", "device") == "device":   # (the host builder reads token lists)
            from .doctok import DeviceDocTokenizer
            dt = DeviceDocTokenizer(kw["device"])
            try:                                           # build_bm25_blob's column: fillna("").astype(str)
                tok, off, vocab = dt.tokenize(meta["agg_text"].fillna("").astype(str).tolist())
            finally:
                dt.close()
            return cls(meta, None, None, encoder=encoder, index=index,
                       bm25_ids=(meta["sku"].astype(str).tolist(), tok, off, vocab), **kw)
        blob = build_bm25_blob(meta) if bm25 else None
        return cls(meta, None, blob, encoder=encoder, index=index, **kw)

    # app: sku -> last position, missing -> 0.0 score (app/app_product_search.py:207-208)
    # cli: same map, but if ANY meta sku is missing the scores are used unpermuted
    #      (ensure_same_order returns None, app/test.py:159-173)
    def _align_bm25(self, bm25_skus: List[str]) -> np.ndarray:
        pos = {s: i for i, s in enumerate(bm25_skus)}
        meta_skus = self.meta["sku"].astype(str).tolist()
        order = np.array([pos.get(s, -1) for s in meta_skus], dtype=np.int64)
        if self.flavour == "cli" and (order < 0).any():
            if len(bm25_skus) < len(meta_skus):
                raise IndexError("BM25 corpus is shorter than the metadata and cannot be used unpermuted")
            order = np.arange(len(meta_skus), dtype=np.int64)
        return order

    # ------------------------------------------------------------------ pieces
    def encode(self, query: str) -> np.ndarray:
        if self.encoder is None:
            raise ValueError("no query encoder was given; use search_by_vector / pass qvec")
        return np.asarray(self.encoder.encode([query], normalize_embeddings=True)[0], dtype=np.float32)

    def _gate_rows(self, groups, penalty: float, rows: np.ndarray) -> np.ndarray:
        """The host gate: float32 (len(rows),) factors of one query's groups at these rows."""
        if not groups:
            return np.ones(len(rows), dtype=np.float32)
        texts = self._texts.iloc[rows].str.slice(0, 6000).tolist()
        return np.array([text.calculate_gate_factor(t, groups, penalty)[0] for t in texts], dtype=np.float32)

    def _gate_args(self, groups_per_query, penalty: float) -> dict:
        """search_batch's gate arguments for these queries' groups: the device match when the engine has a gate plane,
        else the host function, each query's groups on its own row of the pool."""
        if not any(groups_per_query):
            return {}
        if self.searcher.gate_text is not None:
            return {"gate_groups": groups_per_query,
                    "gate_host": lambda b, rows: self._gate_rows(groups_per_query[b], penalty, rows)}
        return {"gate_fn": lambda rows: np.stack([self._gate_rows(g, penalty, r) for g, r in zip(groups_per_query, rows)])}

    def _rerank_args(self, queries: Sequence[str], rerank_k: int) -> dict:
        """search_batch's rerank arguments for these queries: the device pairs when the engine has a token plane (the B
        queries are tokenised here, B short strings), else the host function over all of them."""
        if rerank_k <= 0:
            return {}
        if self.searcher.rerank_text is not None:
            from .rerank import pack_queries
            ce = self.cross_encoder
            packed = pack_queries([ce.tokenizer.text_ids(str(q)) for q in queries], ce.max_length)
            return {"rerank_pairs": (ce, packed, lambda b, rows: self._rerank_fn(queries[b:b + 1])(rows[None, :])[0])}
        return {"rerank_fn": self._rerank_fn(queries)}

    def _rerank_fn(self, queries: Sequence[str]):
        if self.cross_encoder is None:
            return None   # model missing -> zeros (app/app_product_search.py:275)

        def fn(rows: np.ndarray) -> np.ndarray:
            # the (query, text[:2000]) pairs of EVERY query of the batch in ONE predict call: the packed forward has no use
            # for per-query mini-batches (app/app_product_search.py:272-278 builds the pairs the same way, per query)
            texts = self._texts.iloc[rows.reshape(-1)].str.slice(0, 2000).tolist()
            pairs = [(queries[i // rows.shape[1]], t) for i, t in enumerate(texts)]
            scores = np.asarray(self.cross_encoder.predict(pairs, batch_size=64, show_progress_bar=False), dtype=np.float32)
            return scores.reshape(rows.shape)
        return fn

    # ------------------------------------------------------------------ API
    def run_search(self, query: str, k: int, rerank_k: int, w_dense: float, w_bm25: float,
                   w_rerank: float, w_prior: float, w_best: float, prior_C: float,
                   use_snips: bool = False, max_scan: int = 0, min_reviews: int = 8,
                   gate_penalty: float = 0.5, *, qvec: Optional[np.ndarray] = None
                   ) -> Tuple[pd.DataFrame, Dict, Dict]:
        """Same positional / keyword signature and return triple as the reference's
        run_search (app/app_product_search.py:245-248, 312-317); ``qvec`` lets a caller
        supply the query embedding when no encoder is loaded.  With ``use_snips`` and a review
        index (``reviews=`` of the constructor) ``snips`` and ``_best`` are filled like
        _best_snippets does (app/app_product_search.py:285-294, 320-370); otherwise ``snips`` is {}
        and ``_best`` zeros, as in the reference when the review file is absent."""
        qv = self.encode(query) if qvec is None else np.asarray(qvec, dtype=np.float32)
        return self.run_search_batch([query], k, rerank_k, w_dense, w_bm25, w_rerank, w_prior, w_best, prior_C, use_snips,
                                     max_scan, min_reviews, gate_penalty, qvecs=qv[None, :])[0]

    def run_search_batch(self, queries: Sequence[str], k: int, rerank_k: int, w_dense: float, w_bm25: float,
                         w_rerank: float, w_prior: float, w_best: float, prior_C: float,
                         use_snips: bool = False, max_scan: int = 0, min_reviews: int = 8,
                         gate_penalty: float = 0.5, *, qvecs: Optional[np.ndarray] = None
                         ) -> List[Tuple[pd.DataFrame, Dict, Dict]]:
        """`run_search` for a batch of queries with the same parameters: per query the triple `run_search` returns.
        The queries are encoded in ONE encoder call (unless ``qvecs`` (B, dim) is given; with query_vectors="device" in the
        query front on the GPU, and nothing is encoded on the host but the queries the front hands back), searched in one `search_batch`
        -- with gate="device" the gate terms of all of them are matched in one kernel launch -- and the reranker pairs of
        all of them go through one `predict` (with rerank="device": through the pair kernels and the packed forward)."""
        app = self.flavour == "app"
        queries = list(queries)
        if not queries:
            return []
        if qvecs is None:
            if self.encoder is None:
                raise ValueError("no query encoder was given; pass qvecs")
            # query_vectors="device": nothing is encoded here -- the query front makes the vectors (qv stays None)
            qv = None if self.query_vectors == "device" else \
                np.asarray(self.encoder.encode(queries, normalize_embeddings=True), dtype=np.float32)
        else:
            qv = np.asarray(qvecs, dtype=np.float32)
        if qv is not None and qv.shape[0] != len(queries):
            raise ValueError(f"{qv.shape[0]} query vectors for {len(queries)} queries")
        w = FusionWeights(w_dense, w_bm25, w_rerank, w_prior, w_best, prior_C, min_reviews,
                          gate_penalty, APP_TRUST_SAT, app)
        floor = APP_POOL_FLOOR if app else CLI_POOL_FLOOR
        common = dict(pool_floor=floor, reviews=self.reviews if use_snips else None, max_scan=max_scan, bm25_f64=not app)

        def host_text(qs):
            return [text.tokenize_query(q) for q in qs], [text.build_gate_groups(q) for q in qs]

        def search_host(qs, vecs, toks, groups):
            term_ids = None
            if self.searcher.bm25 is not None:
                term_ids = [self.searcher.bm25.term_ids(t) for t in toks]
            return self.searcher.search_batch(vecs, term_ids, k, rerank_k, w, **common, **self._rerank_args(qs, rerank_k),
                                              **self._gate_args(groups, gate_penalty))

        if self._query_text is None:
            toks, groups = host_text(queries)
            res = search_host(queries, qv, toks, groups)
        else:
            res, toks, groups = self._search_device_text(queries, qv, k, rerank_k, w, gate_penalty, common, host_text, search_host)
        out = []
        for b in range(len(queries)):
            frame = self._frame(res, b, rerank_k > 0)
            snips = {}
            if res.best_ids is not None:
                skus = self.meta["sku"].astype(str).iloc[res.pool_rows[b]].tolist()
                snips = self.reviews.snippets(skus, res.best_ids[b], res.best_raw[b], 600 if app else 400)
            dbg = {"bm25_active": self.searcher.bm25 is not None, "tokens": toks[b],
                   "groups": [list(g) for g in groups[b]], "pool": max(k, rerank_k, floor)}
            out.append((frame, snips, dbg))
        return out

    def evaluate(self, test_queries, method_configs: Dict[str, Dict], *, qvecs: Optional[np.ndarray] = None,
                 batch: int = 1024):
        """The reference's ``evaluate_ranking_methods(run_search, test_queries, method_configs)`` as a device operation
        (evals.py, csrc/rr_evals.hip).  ``test_queries``: the evals dicts (``id``, ``query``, ``relevant_items``, optional
        ``relevance_scores``), the app tab's JSONL entries (``query``, ``relevant``), or a ready `evals.LabelSet`;
        ``method_configs``: method -> `run_search` keyword arguments, as in BENCHMARK_CONFIGS; ``qvecs`` (Q, dim): the query
        embeddings when no encoder is loaded.  Returns an `evals.EvalReport`: ``summary`` (methods x the seven metrics),
        ``detailed(method)`` (per query, downloaded on demand), ``metrics_dev[method]`` ((Q, 8) float64 on the device).

        The queries go through in batches of at most ``batch`` (<= RR_MAX_BATCH).  Per batch every configuration ranks
        exactly as `run_search_batch` does with its arguments, but the stages the fusion weights do not touch run once for
        all configurations that read the same thing -- the query front per gate penalty (the query vectors once), K1 and K2
        per pool, the best-review column per (pool, max_scan), the gate match per (pool, gate_penalty), the reranker per
        (pool, rerank_k) -- and only K3 and rr_ir_metrics_dev run per configuration.  Pool rows, columns and orders stay on
        the device and no frame is built; what is read back is the front's flags (the queries it hands back are searched
        again through the host functions, as in `run_search_batch`) and, when asked for, the metrics."""
        from .evals import evaluate_engine
        return evaluate_engine(self, test_queries, method_configs, qvecs=qvecs, batch=batch)

    def _search_device_text(self, queries, qv, k, rerank_k, w, gate_penalty, common, host_text, search_host):
        """One batch with query_text="device": the bytes are staged once and the front end is queued ahead of K1; the
        consumers that are on the device read its buffers, a host gate / host reranker keeps its host function.  The dbg
        lists (tokens, groups) are built while the kernels run.  The queries the front end flags are searched again through
        the host functions, in one batch of their own, and their results put in place."""
        qs = [str(q) for q in queries]
        front = self._query_text.front(qs, gate_penalty, vectors=qv is None)
        made = {}
        args = {}
        if self.searcher.gate_text is None:                    # the host gate reads the groups: they are built first
            made["toks"], made["groups"] = host_text(queries)
            args.update(self._gate_args(made["groups"], gate_penalty))
        if rerank_k > 0:
            if self.searcher.rerank_text is not None:
                args["rerank_pairs"] = (self.cross_encoder, None,
                                        lambda b, rows: self._rerank_fn(queries[b:b + 1])(rows[None, :])[0])
            else:
                args.update(self._rerank_args(queries, rerank_k))

        def on_queued():
            if not made:
                made["toks"], made["groups"] = host_text(queries)

        res = self.searcher.search_batch(qv, None, k, rerank_k, w, **common, query_front=front, on_queued=on_queued, **args)
        self._query_text.check()
        if qv is None and self._query_text.redo_vectors(front):
            # the forward left fp16's range (NaN vectors went into K1): the vectors were made again on the wide-range
            # kernels, as the host path's forward_ids does, and the batch is searched again with them
            res = self.searcher.search_batch(None, None, k, rerank_k, w, **common, query_front=front, **args)
        flagged = np.flatnonzero(res.needs_host)
        if len(flagged):
            # (query_vectors="device": the host encoder for the queries the front handed back, those only)
            sub_qv = qv[flagged] if qv is not None else \
                np.asarray(self.encoder.encode([qs[i] for i in flagged], normalize_embeddings=True), dtype=np.float32)
            sub = search_host([queries[i] for i in flagged], sub_qv, [made["toks"][i] for i in flagged],
                              [made["groups"][i] for i in flagged])
            for name in ("pool_rows", "columns", "order", "dense_raw", "bm25_raw", "best_ids", "best_raw"):
                if getattr(res, name) is not None:
                    getattr(res, name)[flagged] = getattr(sub, name)
        return res, made["toks"], made["groups"]

    def _frame(self, res: BatchResult, b: int, rerank_active: bool = False) -> pd.DataFrame:
        top = res.order[b].astype(np.int64)
        out = self.meta.iloc[res.pool_rows[b][top]].reset_index(drop=True).copy()
        for j, name in enumerate(COLUMN_NAMES):
            col = res.columns[b, j, top]
            if name == "_trust" and self.flavour == "cli":
                continue   # the CLI has no trust column (app/test.py:308)
            # `_rerank` is the float32 array z when rerank_k > 0, else the float64 scalar column 0.0
            # (app/app_product_search.py:279-282); `_bm25` is float64 zeros in the CLI without an artefact
            f32 = name in _FLOAT32_COLUMNS or (name == "_rerank" and rerank_active)
            if name == "_bm25" and self.flavour == "cli" and self.searcher.bm25 is None:
                f32 = False
            out[name] = col.astype(np.float32) if f32 else col
        return out

    def search(self, query: str, k: int = 10, alpha: float = 0.5, *,
               qvec: Optional[np.ndarray] = None) -> Tuple[pd.DataFrame, Dict, Dict]:
        """search(query, k, alpha) of BASELINE.json: dense weight alpha, BM25 weight
        1 - alpha, no rerank / prior / best, gate off."""
        return self.run_search(query, k, 0, alpha, 1.0 - alpha, 0.0, 0.0, 0.0, 20.0, False, 0,
                               8, 1.0, qvec=qvec)

    def search_by_vector(self, qvec: np.ndarray, query: str = "", k: int = 10, alpha: float = 0.5):
        return self.search(query, k, alpha, qvec=qvec)

    def cosine_similarity_search(self, query_vector: np.ndarray, top_k: int):
        rows, scores = self.index.dense_topk(np.asarray(query_vector, dtype=np.float32)[None, :], top_k)
        return rows[0], scores[0]


def cosine_similarity_search(query_vector: np.ndarray, embeddings_matrix: np.ndarray,
                             top_k: int, device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """utils.py:111-124 with the matrix copied to the GPU for this call; use
    ProductIndex / SearchEngine to keep it resident across calls."""
    ix = ProductIndex(np.asarray(embeddings_matrix, dtype=np.float32), device=device)
    try:
        rows, scores = ix.dense_topk(np.asarray(query_vector, dtype=np.float32)[None, :], top_k)
    finally:
        ix.close()
    return rows[0], scores[0]


def cli_rows(frame: pd.DataFrame, snips: Optional[Dict] = None) -> List[Dict]:
    """The CLI's JSON row schema (app/test.py:312-328), 4-dp rounding; ``snips`` is run_search's
    second return value (sku -> best review)."""
    rows = []
    for _, r in frame.iterrows():
        n = r.get("n_reviews", np.nan)
        a = r.get("avg_stars", np.nan)
        snip = snips.get(str(r["sku"])) if snips else None
        rows.append({
            "sku": str(r["sku"]), "score": round(float(r["_final"]), 4),
            "dense": round(float(r["_dense"]), 4), "bm25": round(float(r["_bm25"]), 4),
            "rerank": round(float(r["_rerank"]), 4), "prior": round(float(r["_prior"]), 4),
            "bestrev": round(float(r["_best"]), 4),
            "n_reviews": int(n) if pd.notna(n) else 0,
            "avg_stars": round(float(a), 2) if pd.notna(a) else None,
            "snippet_stars": float(snip["stars"]) if snip and snip.get("stars") is not None else None,
            "snippet": snip["text"] if snip else None})
    return rows
