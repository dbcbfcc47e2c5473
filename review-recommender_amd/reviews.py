"""Best review per candidate product: the device-resident replacement of
``_best_snippets`` (app/app_product_search.py:320-370) / ``best_review_snippets``
(app/test.py:181-215).

The reference re-reads reviews_with_embeddings.parquet on every query, keeps the reviews whose sku
is among the candidates, cuts them to ``max_rows`` in file order, l2-normalises their embeddings,
scores them against the query and keeps the best review per sku.  Here the review embeddings are
uploaded and normalised once, grouped by product row, and a query only touches the reviews of its
candidates (csrc/rr_reviews.hip).

On row shards (sharded.py) every rank holds the reviews of its own products only (``ReviewIndex.shard``): review ids
inside the index are local, a map turns them into GLOBAL ids (positions in the whole table), and the ``iloc[:max_rows]``
cut, an order statistic over ids that live on different ranks, is found by rounds of 256-way narrowing whose counts the
ranks sum (``model_cut`` states the rule in numpy; the ``cut_*`` methods are its steps on the device).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import pandas as pd

from . import _lib


CUT_WAYS = 256       # thresholds per round of the cut across shards (csrc/rr_reviews.hip)


def cut_rounds(n_total: int) -> int:
    """Rounds of 256-way narrowing that bring [0, n_total) down to one id: the smallest R >= 1 with 256^R >= n_total."""
    r, span = 1, CUT_WAYS
    while span < n_total:
        r, span = r + 1, span * CUT_WAYS
    return r


def cut_thresholds(lo: int, hi: int) -> np.ndarray:
    """T_j = lo + ((j+1)(hi-lo+1) + 255)/256 - 1, j = 0..255: the interval [lo, hi] in 256 parts (T_255 = hi)."""
    j = np.arange(1, CUT_WAYS + 1, dtype=np.int64)
    return lo + (j * (hi - lo + 1) + (CUT_WAYS - 1)) // CUT_WAYS - 1


def cut_narrow(lo: int, hi: int, sums: np.ndarray, max_rows: int, first: bool, n_total: int):
    """One narrowing of [lo, hi] from the ranks' summed counts (what rr_reviews_cut_narrow_dev does per query)."""
    if lo >= n_total:                                  # parked by round 1: keep all
        return lo, hi
    if first and int(sums[CUT_WAYS - 1]) <= max_rows:
        return n_total, n_total
    hit = np.flatnonzero(sums >= max_rows)
    if len(hit) == 0:
        return lo, hi
    T = cut_thresholds(lo, hi)
    js = int(hit[0])
    return (lo if js == 0 else int(T[js - 1]) + 1), int(T[js])


def model_cut(rank_lists, max_rows: int, n_total: int) -> int:
    """The numpy statement of the cut across shards.  ``rank_lists``: per rank the GLOBAL ids of the reviews of the merged
    pool's candidates that rank owns (one array, or a list of arrays; a rank that owns nothing: empty).  Returns the largest
    review id inside the reference's ``iloc[:max_rows]`` cut over the union: -1 for max_rows <= 0, ``n_total`` when the
    union is not longer than max_rows, else the max_rows-th smallest id -- found as the device finds it: R = cut_rounds
    rounds; in each, every rank counts its ids <= T_j for the 256 thresholds of the current interval, the counts are summed
    over the ranks, and the interval narrows to the part that holds the max_rows-th id."""
    if max_rows <= 0:
        return -1
    flat = lambda L: np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in L] + [np.zeros(0, dtype=np.int64)])
    ranks = [np.sort(flat(L) if isinstance(L, (list, tuple)) else flat([L])) for L in rank_lists]
    lo, hi = 0, n_total - 1
    for r in range(cut_rounds(n_total)):
        T = cut_thresholds(lo, hi)
        sums = np.zeros(CUT_WAYS, dtype=np.int64)
        for ids in ranks:
            sums += np.searchsorted(ids, T, side="right")
        lo, hi = cut_narrow(lo, hi, sums, max_rows, r == 0, n_total)
    assert lo == hi
    return lo


def pool_reviews_bound(top_counts: np.ndarray, pool: int) -> int:
    """The most reviews the candidates of any pool of ``pool`` distinct products can have: the sum of the ``pool`` largest
    per-product review counts (``top_counts``: counts that include the `pool` largest of the corpus, any order).  A
    ``max_scan`` at or above it can never cut (sharded.py: the rounds are skipped)."""
    c = np.sort(np.asarray(top_counts, dtype=np.int64))[::-1]
    return int(c[:pool].sum())


class ReviewIndex:
    def __init__(self, reviews: pd.DataFrame, embeddings: np.ndarray, product_skus: Sequence[str],
                 device: int = 0, eps: float = 1e-12):
        """reviews: frame with ``sku``, ``text`` and optionally ``stars`` (file order = row order);
        embeddings: (n_reviews, dim) float32, row-aligned; product_skus: the metadata's sku column."""
        if "sku" not in reviews.columns:
            raise ValueError("review table lacks a 'sku' column")      # app/app_product_search.py:328-330
        emb = np.ascontiguousarray(embeddings, dtype=np.float32)
        if emb.ndim != 2 or emb.shape[0] != len(reviews):
            raise ValueError("embeddings must be (n_reviews, dim), row-aligned with the review table")
        self._group(reviews, product_skus, emb.shape)
        h = C.c_void_p()
        _lib.check(_lib.load().rr_reviews_create(_lib.ptr(emb), self.n_reviews, self.dim, self.n_products,
                                                 _lib.ptr(self.indptr), _lib.ptr(self.ids), device, eps,
                                                 C.byref(h)), "rr_reviews_create")
        self._h, self.device = h, device

    @classmethod
    def from_device_rows(cls, reviews: pd.DataFrame, rows, product_skus: Sequence[str], device: int = 0,
                         eps: float = 1e-12) -> "ReviewIndex":
        """The same index from embeddings that are already on the GPU: `rows` = a contiguous float32 (n_reviews, dim) torch
        tensor on `device` (rr_reviews_create_dev copies it; what a builder left there needs no trip through the host)."""
        import torch
        if "sku" not in reviews.columns:
            raise ValueError("review table lacks a 'sku' column")
        if (rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[0] != len(reviews) or not rows.is_contiguous()
                or not rows.is_cuda or rows.device.index != device):
            raise ValueError("rows must be a contiguous float32 (n_reviews, dim) tensor on the index's GPU, row-aligned with "
                             "the review table")
        self = cls.__new__(cls)
        self._group(reviews, product_skus, tuple(rows.shape))
        h = C.c_void_p()
        _lib.check(_lib.load().rr_reviews_create_dev(C.c_void_p(rows.data_ptr()), self.n_reviews, self.dim, self.n_products,
                                                     _lib.ptr(self.indptr), _lib.ptr(self.ids), device, eps,
                                                     C.byref(h)), "rr_reviews_create_dev")
        self._h, self.device = h, device
        return self

    @classmethod
    def shard(cls, reviews: pd.DataFrame, embeddings, product_skus: Sequence[str], lo: int, hi: int, device: int = 0,
              eps: float = 1e-12) -> "ReviewIndex":
        """The index of ONE ROW SHARD: only the reviews whose sku is one of product rows [lo, hi) of ``product_skus``, in
        file order; only their embeddings are uploaded, the CSR is over the local product rows 0 .. hi-lo.  ``reviews`` and
        ``embeddings`` are the WHOLE table ((n_total, dim) float32: a numpy array, a memory map, or a contiguous float32
        torch tensor on ``device`` whose rows are then gathered there).  ``global_ids`` (host) / ``d_global_ids`` (device)
        map a local review id to its GLOBAL id, the position in the whole table; cuts and best ids of this index are global
        ids, ``texts`` / ``stars`` stay the host table of the whole file, so ``snippets`` works unchanged on every rank.
        A review's score does not depend on the shard it sits in: every answer equals the whole index's bit for bit."""
        import torch
        if "sku" not in reviews.columns:
            raise ValueError("review table lacks a 'sku' column")
        n_total = len(reviews)
        if n_total >= 1 << 31:
            raise ValueError(f"a review table of {n_total} rows does not fit the kernels' int32 review ids")
        if not (0 <= lo < hi <= len(product_skus)):
            raise ValueError(f"rows [{lo}, {hi}) are not a range of the {len(product_skus)} products")
        on_device = isinstance(embeddings, torch.Tensor)
        if len(embeddings.shape) != 2 or embeddings.shape[0] != n_total:
            raise ValueError("embeddings must be (n_reviews, dim), row-aligned with the review table")
        if on_device and (embeddings.dtype != torch.float32 or not embeddings.is_contiguous() or not embeddings.is_cuda
                          or embeddings.device.index != device):
            raise ValueError("a tensor of embeddings must be contiguous float32 on the index's GPU")
        self = cls.__new__(cls)
        self._group(reviews, product_skus, tuple(embeddings.shape), lo, hi)
        gids = self.global_ids if len(self.global_ids) else np.zeros(1, dtype=np.int32)    # (a shard without reviews: one
        n_local = len(gids)                                                                # unused zero row, an empty CSR)
        lib, h = _lib.load(), C.c_void_p()
        if on_device:
            rows = embeddings[torch.from_numpy(gids.astype(np.int64)).to(embeddings.device)].contiguous()
            if not len(self.global_ids):
                rows.zero_()
            _lib.check(lib.rr_reviews_create_dev(C.c_void_p(rows.data_ptr()), n_local, self.dim, self.n_products,
                                                 _lib.ptr(self.indptr), _lib.ptr(self.ids), device, eps, C.byref(h)),
                       "rr_reviews_create_dev")
        else:
            emb = np.ascontiguousarray(embeddings[gids], dtype=np.float32)
            if not len(self.global_ids):
                emb[:] = 0
            _lib.check(lib.rr_reviews_create(_lib.ptr(emb), n_local, self.dim, self.n_products, _lib.ptr(self.indptr),
                                             _lib.ptr(self.ids), device, eps, C.byref(h)), "rr_reviews_create")
        self._h, self.device = h, device
        _lib.check(lib.rr_reviews_set_global_ids(h, _lib.ptr(gids), n_total), "rr_reviews_set_global_ids")
        self.d_global_ids = torch.from_numpy(self.global_ids).to(torch.device("cuda", device))
        return self

    def _group(self, reviews: pd.DataFrame, product_skus: Sequence[str], shape, lo: int = 0, hi: Optional[int] = None) -> None:
        """Texts, stars and the CSR product row -> review ids (file order inside a product).  ``hi``: a shard -- only the
        reviews of product rows [lo, hi) are kept and numbered 0.. in file order (``global_ids``: their positions in the
        table), the CSR is over the local rows."""
        self.texts = reviews["text"].astype(str).tolist() if "text" in reviews.columns else [""] * len(reviews)
        self.stars = (pd.to_numeric(reviews["stars"], errors="coerce").to_numpy(dtype=np.float64)
                      if "stars" in reviews.columns else np.full(len(reviews), np.nan))
        row_of = {str(s): i for i, s in enumerate(product_skus)}
        prod = np.array([row_of.get(str(s), -1) for s in reviews["sku"].tolist()], dtype=np.int64)
        self.n_total, self.row_lo, self.row_hi = int(shape[0]), lo, len(product_skus) if hi is None else hi
        self.global_ids = self.d_global_ids = None             # (None: local = global)
        n_reviews = int(shape[0])
        if hi is not None:
            self.global_ids = np.ascontiguousarray(np.nonzero((prod >= lo) & (prod < hi))[0], dtype=np.int32)
            prod = prod[self.global_ids] - lo                  # local reviews -> local product rows
            n_reviews = len(self.global_ids)
        known = np.nonzero(prod >= 0)[0]
        order = known[np.argsort(prod[known], kind="stable")]          # by product, file order inside
        n_products = self.row_hi - lo
        self.indptr = np.zeros(n_products + 1, dtype=np.int64)
        np.cumsum(np.bincount(prod[known], minlength=n_products), out=self.indptr[1:])
        self.ids = np.ascontiguousarray(order, dtype=np.int32)
        self.n_reviews, self.dim, self.n_products = n_reviews, int(shape[1]), n_products

    def top_counts(self, n: int) -> np.ndarray:
        """The ``n`` largest per-product review counts of this index, descending, zero-padded (int64): what the ranks exchange
        once for the rule that skips the cut's rounds (pool_reviews_bound)."""
        out = np.zeros(n, dtype=np.int64)
        c = np.sort(np.diff(self.indptr))[::-1][:n]
        out[:len(c)] = c
        return out

    # ------------------------------------------------------------------ the cut across shards, step by step
    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    @staticmethod
    def _stream(t):
        import torch
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def cut_begin(self, n_queries: int):
        """The rounds' state: (n_queries, 2) int64 on the device, every interval [0, n_total - 1]."""
        import torch
        state = torch.empty((n_queries, 2), dtype=torch.int64, device=self._dev())
        _lib.check(_lib.load().rr_reviews_cut_begin_dev(self._h, n_queries, C.c_void_p(state.data_ptr()), self._stream(state)),
                   "rr_reviews_cut_begin_dev")
        return state

    def cut_counts(self, state, rows, max_rows: int, row_offset: int = 0, sums=None, first: bool = False, out=None):
        """One round on this index: (B, 256) int64 counts of the reviews with global id <= T_j among the candidates
        ``rows`` (B, pool) int64 global product rows that this index owns.  ``sums``: the ranks' summed counts of the
        PREVIOUS round -- the launch then narrows ``state`` with them first (``first``: they are round 1's)."""
        import torch
        B, pool = rows.shape
        counts = out if out is not None else torch.empty((B, CUT_WAYS), dtype=torch.int64, device=rows.device)
        _lib.check(_lib.load().rr_reviews_cut_count_dev(
            self._h, B, C.c_void_p(rows.data_ptr()), pool, int(row_offset), int(max_rows),
            C.c_void_p(sums.data_ptr()) if sums is not None else None, int(bool(first)), C.c_void_p(state.data_ptr()),
            C.c_void_p(counts.data_ptr()), self._stream(rows)), "rr_reviews_cut_count_dev")
        return counts

    def cut_narrow(self, state, sums, max_rows: int, first: bool = False, cuts=None):
        """Narrows ``state`` with the summed counts of a round, as a launch of its own; ``cuts``: an int32 (B,) tensor that
        also receives every interval's lower end."""
        B = state.shape[0]
        _lib.check(_lib.load().rr_reviews_cut_narrow_dev(
            self._h, B, int(max_rows), C.c_void_p(sums.data_ptr()), int(bool(first)), C.c_void_p(state.data_ptr()),
            C.c_void_p(cuts.data_ptr()) if cuts is not None else None, self._stream(state)), "rr_reviews_cut_narrow_dev")
        return state

    def cut_end(self, state, sums, max_rows: int, first: bool = False):
        """Behind the last round: narrows with its sums and returns the cuts, int32 (B,) global review ids."""
        import torch
        cuts = torch.empty((state.shape[0],), dtype=torch.int32, device=state.device)
        self.cut_narrow(state, sums, max_rows, first, cuts)
        return cuts

    def best_at(self, q_dev, rows, cuts, row_offset: int = 0, out=None):
        """Best review per (query, candidate) under per-query cuts in device memory: (score float32, id int32), both
        (B, pool); ids are global ids; a row this index does not own gives (0, -1)."""
        import torch
        B, pool = rows.shape
        score, rid = out if out is not None else (torch.empty((B, pool), dtype=torch.float32, device=rows.device),
                                                  torch.empty((B, pool), dtype=torch.int32, device=rows.device))
        _lib.check(_lib.load().rr_reviews_best_at_dev(
            self._h, C.c_void_p(q_dev.data_ptr()), B, C.c_void_p(rows.data_ptr()), pool, int(row_offset),
            C.c_void_p(cuts.data_ptr()), C.c_void_p(score.data_ptr()), C.c_void_p(rid.data_ptr()), self._stream(rows)),
            "rr_reviews_best_at_dev")
        return score, rid

    @property
    def handle(self):
        return self._h

    def cut_for(self, rows: np.ndarray, max_rows: int) -> int:
        """Largest review id still inside the reference's ``iloc[:max_rows]`` cut
        (app/app_product_search.py:342-345) for the candidate product rows ``rows``."""
        if max_rows <= 0:
            return -1
        rows = np.asarray(rows) - self.row_lo              # (a shard: its own candidates, as global ids)
        rows = np.unique(rows[(rows >= 0) & (rows < self.n_products)])
        counts = self.indptr[rows + 1] - self.indptr[rows]
        if int(counts.sum()) <= max_rows:
            return int(self.n_total)                       # nothing is cut
        sel = np.concatenate([self.ids[self.indptr[r]:self.indptr[r + 1]] for r in rows])
        cut = int(np.partition(sel, max_rows - 1)[max_rows - 1])
        return cut if self.global_ids is None else int(self.global_ids[cut])

    def snippets(self, skus: Sequence[str], best_id: np.ndarray, best_score: np.ndarray,
                 text_cut: int = 600) -> Dict[str, Dict]:
        """The reference's ``{sku: {"score", "text", "stars"}}`` for candidates that have a review."""
        out: Dict[str, Dict] = {}
        for sku, rid, sc in zip(skus, best_id.tolist(), best_score.tolist()):
            if rid >= 0:
                out[str(sku)] = {"score": float(sc), "text": self.texts[rid][:text_cut],
                                 "stars": float(self.stars[rid])}
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_reviews_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
