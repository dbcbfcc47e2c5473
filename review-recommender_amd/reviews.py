"""Best review per candidate product: the device-resident replacement of
``_best_snippets`` (app/app_product_search.py:320-370) / ``best_review_snippets``
(app/test.py:181-215).

The reference re-reads reviews_with_embeddings.parquet on every query, keeps the reviews whose sku
is among the candidates, cuts them to ``max_rows`` in file order, l2-normalises their embeddings,
scores them against the query and keeps the best review per sku.  Here the review embeddings are
uploaded and normalised once, grouped by product row, and a query only touches the reviews of its
candidates (csrc/rr_reviews.hip).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import numpy as np
import pandas as pd

from . import _lib


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
        self._h = h

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
        self._h = h
        return self

    def _group(self, reviews: pd.DataFrame, product_skus: Sequence[str], shape) -> None:
        """Texts, stars and the CSR product row -> review ids (file order inside a product)."""
        self.texts = reviews["text"].astype(str).tolist() if "text" in reviews.columns else [""] * len(reviews)
        self.stars = (pd.to_numeric(reviews["stars"], errors="coerce").to_numpy(dtype=np.float64)
                      if "stars" in reviews.columns else np.full(len(reviews), np.nan))
        row_of = {str(s): i for i, s in enumerate(product_skus)}
        prod = np.array([row_of.get(str(s), -1) for s in reviews["sku"].tolist()], dtype=np.int64)
        known = np.nonzero(prod >= 0)[0]
        order = known[np.argsort(prod[known], kind="stable")]          # by product, file order inside
        n_products = len(product_skus)
        self.indptr = np.zeros(n_products + 1, dtype=np.int64)
        np.cumsum(np.bincount(prod[known], minlength=n_products), out=self.indptr[1:])
        self.ids = np.ascontiguousarray(order, dtype=np.int32)
        self.n_reviews, self.dim, self.n_products = int(shape[0]), int(shape[1]), n_products

    @property
    def handle(self):
        return self._h

    def cut_for(self, rows: np.ndarray, max_rows: int) -> int:
        """Largest review id still inside the reference's ``iloc[:max_rows]`` cut
        (app/app_product_search.py:342-345) for the candidate product rows ``rows``."""
        if max_rows <= 0:
            return -1
        rows = np.unique(rows[(rows >= 0) & (rows < self.n_products)])
        counts = self.indptr[rows + 1] - self.indptr[rows]
        if int(counts.sum()) <= max_rows:
            return int(self.n_reviews)                     # nothing is cut
        sel = np.concatenate([self.ids[self.indptr[r]:self.indptr[r + 1]] for r in rows])
        return int(np.partition(sel, max_rows - 1)[max_rows - 1])

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
