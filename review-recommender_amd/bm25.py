"""BM25 index of the hot path: host-side CSR construction + the device scorer.

Stands in for ``rank_bm25.BM25Okapi`` as the reference uses it
(``BM25Okapi(blob["corpus"])`` app/app_product_search.py:142, app/test.py:156;
``.get_scores(tokens)`` app/app_product_search.py:206, app/test.py:170), with the
package's default parameters k1=1.5, b=0.75, epsilon=0.25.

Host side (this file): vocabulary in first-appearance order, per-document term
frequencies, document lengths, avgdl, idf with the epsilon floor -- computed once
at load, in float64 with ``math.log`` per term and a running sum in vocabulary
order, like the package.  ``build_bm25_index`` builds the same CSR arrays on the
GPU instead (csrc/rr_bm25_build.hip); only the vocabulary ids and idf stay on the
host.  Device side (csrc/rr_bm25.hip): every per-query operation.
The corpus is stored twice on the device, 8 bytes per posting each way:
postings (term -> ascending docs) for ``get_scores`` and a forward list
(doc -> ascending terms) for scoring a candidate pool.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib


def idf_with_floor(df: np.ndarray, n_docs: int, epsilon: float = 0.25) -> np.ndarray:
    """idf[t] = ln(N - df + 0.5) - ln(df + 0.5); negatives -> epsilon * mean(idf).

    ``df`` is in vocabulary order; the mean is a left-to-right float64 sum in that
    order divided by the vocabulary size (rank_bm25 ``_calc_idf``)."""
    out = np.empty(len(df), dtype=np.float64)
    total = 0.0
    log = math.log
    for i, f in enumerate(df.tolist()):
        v = log(n_docs - f + 0.5) - log(f + 0.5)
        out[i] = v
        total += v
    if len(df):
        floor = epsilon * (total / len(df))
        out[out < 0] = floor
    return out


class BM25Corpus:
    """Host-side integer-id corpus: forward CSR + corpus-wide statistics.

    ``doc_terms`` ascend within each document.  ``idf`` / ``avgdl``
    always describe the corpus the statistics were taken over, also after
    ``select`` / ``slice`` (a shard scores with corpus-wide statistics).
    """

    def __init__(self, doc_indptr, doc_terms, doc_tf, doc_len, n_terms: int, *,
                 idf: Optional[np.ndarray] = None, avgdl: Optional[float] = None,
                 k1: float = 1.5, b: float = 0.75, epsilon: float = 0.25,
                 vocab: Optional[Dict[str, int]] = None):
        self.doc_indptr = np.ascontiguousarray(doc_indptr, dtype=np.int64)
        self.doc_terms = np.ascontiguousarray(doc_terms, dtype=np.int32)
        self.doc_tf = np.ascontiguousarray(doc_tf, dtype=np.int32)
        self.doc_len = np.ascontiguousarray(doc_len, dtype=np.int32)
        self.n_docs, self.n_terms = len(self.doc_len), int(n_terms)
        if len(self.doc_indptr) != self.n_docs + 1:
            raise ValueError("doc_indptr must have n_docs + 1 entries")
        self.nnz = int(self.doc_indptr[-1])
        if len(self.doc_terms) != self.nnz or len(self.doc_tf) != self.nnz:
            raise ValueError("doc_terms / doc_tf length does not match doc_indptr[-1]")
        self.k1, self.b, self.epsilon, self.vocab = float(k1), float(b), float(epsilon), vocab
        if avgdl is None:
            avgdl = int(self.doc_len.astype(np.int64).sum()) / self.n_docs
        self.avgdl = float(avgdl)
        if idf is None:
            df = np.bincount(self.doc_terms, minlength=self.n_terms).astype(np.int64)
            idf = idf_with_floor(df, self.n_docs, epsilon)
        self.idf = np.ascontiguousarray(idf, dtype=np.float64)
        if len(self.idf) != self.n_terms:
            raise ValueError("idf must have one entry per vocabulary term")

    @classmethod
    def from_corpus(cls, corpus: Sequence[Sequence[str]], **kw) -> "BM25Corpus":
        """``corpus`` = list of token lists, the ``blob["corpus"]`` of product_bm25.pkl
        (nlp/12_product_prep.py:85-89).  Vocabulary ids follow first appearance, the
        order rank_bm25's dicts iterate in."""
        vocab: Dict[str, int] = {}
        indptr = np.zeros(len(corpus) + 1, dtype=np.int64)
        terms: List[np.ndarray] = []
        tfs: List[np.ndarray] = []
        doc_len = np.zeros(len(corpus), dtype=np.int32)
        for d, doc in enumerate(corpus):
            doc_len[d] = len(doc)
            counts: Dict[int, int] = {}
            for w in doc:
                t = vocab.get(w)
                if t is None:
                    t = vocab[w] = len(vocab)
                counts[t] = counts.get(t, 0) + 1
            ids = np.fromiter(counts.keys(), dtype=np.int32, count=len(counts))
            cnt = np.fromiter(counts.values(), dtype=np.int32, count=len(counts))
            o = np.argsort(ids, kind="stable")
            terms.append(ids[o])
            tfs.append(cnt[o])
            indptr[d + 1] = indptr[d] + len(counts)
        cat = (lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int32))
        return cls(indptr, cat(terms), cat(tfs), doc_len, len(vocab), vocab=vocab, **kw)

    @classmethod
    def from_ids(cls, tok, doc_off, n_terms: int, **kw) -> "BM25Corpus":
        """The corpus of an integer-id token stream (``factorize_corpus``): the arrays ``from_corpus`` makes
        from the token lists the ids came from, computed with numpy (a sort by (doc, term) and run lengths)."""
        tok = np.asarray(tok, dtype=np.int64)
        off = np.asarray(doc_off, dtype=np.int64)
        n_docs = len(off) - 1
        doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(off))
        keys, tf = np.unique(doc * max(int(n_terms), 1) + tok, return_counts=True)
        e_doc = keys // max(int(n_terms), 1)
        indptr = np.zeros(n_docs + 1, dtype=np.int64)
        np.cumsum(np.bincount(e_doc, minlength=n_docs), out=indptr[1:])
        return cls(indptr, (keys - e_doc * max(int(n_terms), 1)).astype(np.int32), tf.astype(np.int32),
                   np.diff(off).astype(np.int32), int(n_terms), **kw)

    def _derive(self, indptr, terms, tf, doc_len) -> "BM25Corpus":
        return BM25Corpus(indptr, terms, tf, doc_len, self.n_terms, idf=self.idf,
                          avgdl=self.avgdl, k1=self.k1, b=self.b, epsilon=self.epsilon,
                          vocab=self.vocab)

    def select(self, order: np.ndarray) -> "BM25Corpus":
        """Document j of the result is document order[j] of this corpus; -1 gives an
        empty document (scores 0.0 -- the ``by_sku.get(sku, 0.0)`` miss of
        app/app_product_search.py:208)."""
        order = np.asarray(order, dtype=np.int64)
        safe = np.where(order >= 0, order, 0)
        counts = np.where(order >= 0, np.diff(self.doc_indptr)[safe], 0)
        indptr = np.zeros(len(order) + 1, dtype=np.int64)
        np.cumsum(counts, out=indptr[1:])
        starts = self.doc_indptr[safe]
        # gather index: for every output entry, its position in the source arrays
        src = np.repeat(starts - indptr[:-1], counts) + np.arange(indptr[-1], dtype=np.int64)
        doc_len = np.where(order >= 0, self.doc_len[safe], 0)
        return self._derive(indptr, self.doc_terms[src], self.doc_tf[src], doc_len)

    def slice(self, lo: int, hi: int) -> "BM25Corpus":
        s, e = int(self.doc_indptr[lo]), int(self.doc_indptr[hi])
        return self._derive(self.doc_indptr[lo:hi + 1] - s, self.doc_terms[s:e],
                            self.doc_tf[s:e], self.doc_len[lo:hi])

    def term_ids(self, tokens: Sequence[str]) -> np.ndarray:
        """Vocabulary ids of query tokens; -1 for a token the corpus never saw
        (``idf.get(q) or 0`` in the package)."""
        if self.vocab is None:
            raise ValueError("this corpus was built from integer ids; pass ids directly")
        return np.array([self.vocab.get(t, -1) for t in tokens], dtype=np.int32)

    def to_device(self, device: int = 0, row_offset: int = 0) -> "BM25Index":
        return BM25Index(self, device=device, row_offset=row_offset)


class BM25Index:
    """A BM25Corpus resident on one GPU (postings + forward lists)."""

    def __init__(self, corpus: BM25Corpus, device: int = 0, row_offset: int = 0):
        c = corpus
        self.corpus = c
        self.n_docs, self.n_terms, self.nnz = c.n_docs, c.n_terms, c.nnz
        self.row_offset, self.device = int(row_offset), int(device)
        # postings = forward entries stably sorted by term (docs stay ascending per term)
        order = np.argsort(c.doc_terms, kind="stable")
        doc_of_entry = np.repeat(np.arange(c.n_docs, dtype=np.int32), np.diff(c.doc_indptr))
        post_docs = np.ascontiguousarray(doc_of_entry[order])
        post_tf = np.ascontiguousarray(c.doc_tf[order])
        post_indptr = np.zeros(c.n_terms + 1, dtype=np.int64)
        np.cumsum(np.bincount(c.doc_terms, minlength=c.n_terms), out=post_indptr[1:])
        lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(lib.rr_bm25_create(
            device, c.n_docs, c.n_terms, c.nnz, _lib.ptr(post_indptr), _lib.ptr(post_docs),
            _lib.ptr(post_tf), _lib.ptr(c.doc_indptr), _lib.ptr(c.doc_terms), _lib.ptr(c.doc_tf),
            _lib.ptr(c.doc_len), _lib.ptr(c.idf), c.avgdl, c.k1, c.b, self.row_offset,
            C.byref(handle)), "rr_bm25_create")
        self._h = handle

    @classmethod
    def _adopt(cls, handle, corpus: Optional[BM25Corpus], sizes, df: np.ndarray, device: int,
               row_offset: int) -> "BM25Index":
        """An index over the arrays rr_bm25_build left on the device (no second upload)."""
        self = cls.__new__(cls)
        self._h = handle
        self.corpus = corpus
        self.n_docs, self.n_terms, self.nnz = int(sizes[0]), int(sizes[1]), int(sizes[2])
        self.n_src, self.length_sum = int(sizes[3]), int(sizes[4])
        self.df = df
        self.row_offset, self.device = int(row_offset), int(device)
        return self

    def copy_csr(self, out: Optional[dict] = None) -> dict:
        """The device arrays copied to host numpy arrays (``out``: the subset of them to copy, preallocated)."""
        n, t, z = self.n_docs, self.n_terms, self.nnz
        o = out or {"doc_indptr": np.empty(n + 1, np.int64), "doc_terms": np.empty(z, np.int32),
                    "doc_tf": np.empty(z, np.int32), "doc_len": np.empty(n, np.int32),
                    "post_indptr": np.empty(t + 1, np.int64), "post_docs": np.empty(z, np.int32),
                    "post_tf": np.empty(z, np.int32)}
        names = ("doc_indptr", "doc_terms", "doc_tf", "doc_len", "post_indptr", "post_docs", "post_tf")
        _lib.check(_lib.load().rr_bm25_copy_csr(self._h, *[_lib.ptr(o[k]) if k in o else None for k in names]),
                   "rr_bm25_copy_csr")
        return o

    def term_ids(self, tokens: Sequence[str]) -> np.ndarray:
        return self.corpus.term_ids(tokens)

    def get_scores_ids(self, term_ids: Sequence[int]) -> np.ndarray:
        ids = np.ascontiguousarray(term_ids, dtype=np.int32)
        out = np.empty(self.n_docs, dtype=np.float64)
        _lib.check(_lib.load().rr_bm25_get_scores(self._h, _lib.ptr(ids), len(ids), _lib.ptr(out)),
                   "rr_bm25_get_scores")
        return out

    def scores_at_ids(self, term_id_lists: Sequence[Sequence[int]], rows: np.ndarray,
                      mode: str = "forward") -> np.ndarray:
        """BM25 of query q at rows[q, :] (global rows).  float32, shape of ``rows``."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 2 or rows.shape[0] != len(term_id_lists):
            raise ValueError("rows must be (n_queries, pool)")
        off = np.zeros(len(term_id_lists) + 1, dtype=np.int32)
        for i, t in enumerate(term_id_lists):
            off[i + 1] = off[i] + len(t)
        flat = (np.concatenate([np.asarray(t, dtype=np.int32) for t in term_id_lists])
                if off[-1] else np.zeros(1, dtype=np.int32))
        flat = np.ascontiguousarray(flat, dtype=np.int32)
        out = np.zeros(rows.shape, dtype=np.float32)
        if rows.shape[1] == 0:
            return out
        _lib.check(_lib.load().rr_bm25_scores_at(
            self._h, _lib.ptr(flat), _lib.ptr(off), rows.shape[0], _lib.ptr(rows), rows.shape[1],
            {"forward": 0, "postings": 1}[mode], _lib.ptr(out)), "rr_bm25_scores_at")
        return out

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_bm25_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def doc_offsets(corpus: Sequence[Sequence]) -> np.ndarray:
    """doc_off[n + 1] (int64) of the flattened token stream: document d is tokens [doc_off[d], doc_off[d + 1])."""
    off = np.zeros(len(corpus) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, corpus), dtype=np.int64, count=len(corpus)), out=off[1:])
    return off


def factorize_corpus(corpus: Sequence[Sequence[str]]):
    """-> (tok int32[T], doc_off int64[n + 1], vocab): vocabulary ids in first-appearance order, the ids
    ``BM25Corpus.from_corpus`` gives.  ``pd.factorize`` does the hashing; a token that is not a ``str``
    (factorize takes None / NaN for missing values) sends the corpus through the dict loop instead."""
    import itertools
    import pandas as pd
    off = doc_offsets(corpus)
    T = int(off[-1])
    flat = np.fromiter(itertools.chain.from_iterable(corpus), dtype=object, count=T)
    codes, uniques = pd.factorize(flat, sort=False)
    if not (codes < 0).any() and all(type(u) is str for u in uniques):
        vocab = {u: i for i, u in enumerate(uniques)}
        return np.ascontiguousarray(codes, dtype=np.int32), off, vocab
    vocab: Dict = {}
    tok = np.empty(T, dtype=np.int32)
    for i, w in enumerate(flat.tolist()):
        t = vocab.get(w)
        if t is None:
            t = vocab[w] = len(vocab)
        tok[i] = t
    return tok, off, vocab


def build_bm25_index(corpus: Sequence[Sequence[str]], *, device: int = 0, order=None, rows=None,
                     row_offset: int = 0, k1: float = 1.5, b: float = 0.75, epsilon: float = 0.25,
                     host_copy: bool = True) -> BM25Index:
    """``BM25Corpus.from_corpus(corpus).select(order).slice(lo, hi).to_device(row_offset=...)`` with the
    index built on the GPU (csrc/rr_bm25_build.hip): vocabulary ids on the host (factorize_corpus),
    everything else on the device.  ``rows = (lo, hi)`` of the selected rows; idf and avgdl stay those
    of the whole corpus."""
    tok, off, vocab = factorize_corpus(corpus)
    return build_bm25_index_ids(tok, off, len(vocab), device=device, order=order, rows=rows,
                                row_offset=row_offset, k1=k1, b=b, epsilon=epsilon, vocab=vocab,
                                host_copy=host_copy)


def build_bm25_index_ids(tok, doc_off, n_terms: int, *, device: int = 0, order=None, rows=None,
                         row_offset: int = 0, k1: float = 1.5, b: float = 0.75, epsilon: float = 0.25,
                         vocab: Optional[Dict[str, int]] = None, host_copy: bool = True) -> BM25Index:
    """The same from integer ids: ``tok`` int32[T] in document order, ``doc_off`` int64[n_src + 1], as numpy
    arrays or tensors on ``device``.  ``host_copy=False`` leaves ``.corpus`` None (no copy of the
    arrays back to host memory)."""
    import torch
    if isinstance(order, np.ndarray) and len(order) == len(doc_off) - 1 and np.array_equal(order, np.arange(len(order))):
        order = None                                              # (the identity: no second build)
    on_dev = any(isinstance(a, torch.Tensor) and a.device.type == "cuda" for a in (tok, doc_off, order))
    keep = []                                                     # (the buffers the call reads)

    def arg(a, np_dtype, t_dtype):
        if a is None:
            return None, 0
        if on_dev:
            t = torch.as_tensor(a).to(device=f"cuda:{device}", dtype=t_dtype).contiguous()
            keep.append(t)
            return C.c_void_p(t.data_ptr() if t.numel() else 0), t.numel()
        h = np.ascontiguousarray(a, dtype=np_dtype)
        keep.append(h)
        return (_lib.ptr(h) if h.size else None), h.size

    p_tok, T = arg(tok, np.int32, torch.int32)
    p_off, n_off = arg(doc_off, np.int64, torch.int64)
    p_ord, n_ord = arg(order, np.int64, torch.int64)
    n_src = n_off - 1
    n_rows = n_ord if order is not None else n_src
    lo, hi = (0, n_rows) if rows is None else (int(rows[0]), int(rows[1]))
    lib = _lib.load()
    handle = C.c_void_p()
    # device inputs (and the conversions above) are queued on torch's current stream: the build waits for that stream
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if on_dev else None
    _lib.check(lib.rr_bm25_build(device, int(on_dev), p_tok, T, p_off, n_src, int(n_terms), p_ord, n_ord, lo, hi,
                                 float(k1), float(b), int(row_offset), stream, C.byref(handle)), "rr_bm25_build")
    try:
        sizes = np.zeros(5, dtype=np.int64)
        df = np.empty(int(n_terms), dtype=np.int64)
        _lib.check(lib.rr_bm25_build_stats(handle, _lib.ptr(df), _lib.ptr(sizes)), "rr_bm25_build_stats")
        idf = idf_with_floor(df, int(sizes[3]), epsilon)          # the host's float64 sum order
        avgdl = int(sizes[4]) / int(sizes[3])                     # BM25Corpus.__init__
        _lib.check(lib.rr_bm25_set_idf(handle, _lib.ptr(idf), avgdl), "rr_bm25_set_idf")
    except Exception:
        lib.rr_bm25_destroy(handle)
        raise
    index = BM25Index._adopt(handle, None, sizes, df, device, row_offset)
    if host_copy:
        a = index.copy_csr({"doc_indptr": np.empty(index.n_docs + 1, np.int64),
                            "doc_terms": np.empty(index.nnz, np.int32), "doc_tf": np.empty(index.nnz, np.int32),
                            "doc_len": np.empty(index.n_docs, np.int32)})
        index.corpus = BM25Corpus(a["doc_indptr"], a["doc_terms"], a["doc_tf"], a["doc_len"], int(n_terms),
                                  idf=idf, avgdl=avgdl, k1=k1, b=b, epsilon=epsilon, vocab=vocab)
    return index


def build_bm25_index_texts(texts, *, device: int = 0, order=None, rows=None, row_offset: int = 0, k1: float = 1.5,
                           b: float = 0.75, epsilon: float = 0.25, host_copy: bool = True) -> BM25Index:
    """``build_bm25_index([text.tokenize_document(t) for t in texts], ...)`` with the tokens and the vocabulary ids made on
    the GPU as well (csrc/rr_doctok.hip): raw text in, the same index out, bit for bit."""
    from .doctok import DeviceDocTokenizer
    dt = DeviceDocTokenizer(device)
    try:
        tok, off, vocab = dt.tokenize(texts)
        return build_bm25_index_ids(tok, off, len(vocab), device=device, order=order, rows=rows, row_offset=row_offset,
                                    k1=k1, b=b, epsilon=epsilon, vocab=vocab, host_copy=host_copy)
    finally:
        dt.close()


class BM25Okapi:
    """Drop-in for ``rank_bm25.BM25Okapi`` on the calls the reference makes:
    ``BM25Okapi(corpus)`` and ``get_scores(tokens) -> float64[N]``."""

    def __init__(self, corpus: Sequence[Sequence[str]], tokenizer=None, k1: float = 1.5,
                 b: float = 0.75, epsilon: float = 0.25, device: int = 0, build: str = "device"):
        """build: "device" = the index built on the GPU (build_bm25_index), "host" = BM25Corpus.from_corpus
        + upload; the two give bitwise the same index."""
        if tokenizer is not None:
            corpus = [tokenizer(doc) for doc in corpus]
        if build == "device":
            self.index = build_bm25_index(corpus, device=device, k1=k1, b=b, epsilon=epsilon)
        elif build == "host":
            self.index = BM25Corpus.from_corpus(corpus, k1=k1, b=b, epsilon=epsilon).to_device(device)
        else:
            raise ValueError("build must be 'device' or 'host'")
        self._adopt(k1, b, epsilon)

    def _adopt(self, k1: float, b: float, epsilon: float) -> None:
        """The attributes rank_bm25 exposes, from ``self.index``."""
        self.corpus_size = self.index.n_docs
        self.avgdl = self.index.corpus.avgdl
        self.k1, self.b, self.epsilon = k1, b, epsilon

    @classmethod
    def from_texts(cls, texts, k1: float = 1.5, b: float = 0.75, epsilon: float = 0.25, device: int = 0) -> "BM25Okapi":
        """``BM25Okapi([text.tokenize_document(t) for t in texts])`` from the raw texts, tokenised on the GPU."""
        self = cls.__new__(cls)
        self.index = build_bm25_index_texts(texts, device=device, k1=k1, b=b, epsilon=epsilon)
        self._adopt(k1, b, epsilon)
        return self

    @property
    def idf(self) -> Dict[str, float]:
        c = self.index.corpus
        return {w: float(c.idf[i]) for w, i in c.vocab.items()}

    def get_scores(self, query: Sequence[str]) -> np.ndarray:
        return self.index.get_scores_ids(self.index.term_ids(query))

    def get_batch_scores(self, query: Sequence[str], doc_ids: Sequence[int]) -> List[float]:
        rows = np.asarray(doc_ids, dtype=np.int64)[None, :]
        return self.index.scores_at_ids([self.index.term_ids(query)], rows)[0].astype(
            np.float64).tolist()
