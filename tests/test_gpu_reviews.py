"""best review per candidate (use_snips) against the oracle's restatement of
_best_snippets (app/app_product_search.py:320-370)."""
import numpy as np
import pandas as pd
import pytest

from oracle.bm25 import BM25OkapiOracle
from oracle.pipeline import run_search_oracle
from review_recommender_amd import synth
from review_recommender_amd.engine import SearchEngine

pytestmark = pytest.mark.gpu


def make(n=3000, n_rev=20000, seed=3):
    V = synth.unit_rows(n, 384, seed)
    n_r, stars = synth.metadata(n, seed + 1)
    texts = synth.text_corpus(n, seed + 2, 20)
    meta = pd.DataFrame({"sku": synth.skus(n), "n_reviews": n_r, "avg_stars": stars, "agg_text": texts})
    rng = np.random.default_rng(seed + 3)
    owner = rng.integers(0, n + 200, n_rev)                         # some reviews belong to unknown skus
    E = (rng.standard_normal((n_rev, 384)) * rng.uniform(0.5, 3.0, (n_rev, 1))).astype(np.float32)
    # reviews resemble their product so best scores are well separated
    known = owner < n
    E[known] = (V[owner[known]] * 4 + E[known] * 0.05).astype(np.float32)
    reviews = pd.DataFrame({"sku": [f"B{o:09d}" for o in owner],
                            "text": [f"review {i} " + "x" * (i % 900) for i in range(n_rev)],
                            "stars": rng.integers(1, 6, n_rev).astype(np.float64)})
    return meta, V, reviews, E


@pytest.mark.parametrize("flavour,max_scan", [("app", 300000), ("app", 150), ("cli", 1000000), ("app", 0)])
def test_snippets_and_best_column(flavour, max_scan):
    meta, V, reviews, E = make()
    corpus = [t.split() for t in meta["agg_text"]]
    blob = {"skus": meta["sku"].tolist(), "corpus": corpus}
    engine = SearchEngine(meta, V, blob, normalize=False, flavour=flavour, reviews=(reviews, E))
    ora = BM25OkapiOracle(corpus)
    cfg = dict(k=10, rerank_k=0, w_dense=0.5, w_bm25=0.2, w_rerank=0.0, w_prior=0.1, w_best=0.2, prior_C=20.0,
               min_reviews=8, gate_penalty=1.0)
    for seed, query in ((41, "wireless mug"), (42, "cat socks")):
        qv = synth.unit_rows(1, 384, seed)[0]
        want, want_snips, _, cand = run_search_oracle(query=query, qvec=qv, meta=meta, V=V, bm25=ora,
                                                      bm25_skus=blob["skus"], flavour=flavour, use_snips=True,
                                                      max_scan=max_scan, reviews=(reviews, E), **cfg)
        got, snips, _ = engine.run_search(query, cfg["k"], 0, 0.5, 0.2, 0.0, 0.1, 0.2, 20.0, True, max_scan, 8, 1.0,
                                          qvec=qv)
        assert set(snips) == set(want_snips)
        if max_scan > 0:
            assert len(snips) > 20
        for sku, w in want_snips.items():
            g = snips[sku]
            assert g["text"] == w["text"] and g["stars"] == w["stars"]
            assert abs(g["score"] - w["score"]) < 1e-5
            assert len(g["text"]) <= (600 if flavour == "app" else 400)
        assert got["sku"].tolist() == want["sku"].tolist()
        np.testing.assert_allclose(got["_final"].values, want["_final"].values, atol=1e-5, rtol=0)
        np.testing.assert_allclose(got["_best"].values, want["_best"].values, atol=1e-5, rtol=0)


def test_no_review_index_means_empty_snips():
    meta, V, _, _ = make(500, 10)
    engine = SearchEngine(meta, V, None, normalize=False)
    qv = synth.unit_rows(1, 384, 5)[0]
    got, snips, _ = engine.run_search("mug", 5, 0, 1.0, 0, 0, 0, 0.5, 20.0, True, 1000, 8, 1.0, qvec=qv)
    assert snips == {} and np.all(got["_best"] == 0)


@pytest.mark.parametrize("max_scan", [300000, 150, 37, 1, 0])
def test_batched_snippets_with_the_per_query_cut_on_the_device(max_scan):
    """One rr_reviews_best_cut_dev call for a whole batch (no host round trip for the iloc[:max_rows] cut):
    per query the snippets must be the ones the oracle's _best_snippets finds for that query alone."""
    from oracle.dense import cosine_similarity_search
    from oracle.pipeline import best_snippets_oracle
    from review_recommender_amd.engine import FusionWeights
    meta, V, reviews, E = make(2500, 15000, seed=9)
    engine = SearchEngine(meta, V, None, normalize=False, reviews=(reviews, E))
    Q = synth.unit_rows(9, 384, 77)
    w = FusionWeights(0.6, 0.0, 0.0, 0.0, 0.4, gate_penalty=1.0)
    res = engine.searcher.search_batch(Q, None, 10, 0, w, reviews=engine.reviews, max_scan=max_scan)
    skus = meta["sku"].astype(str)
    for b in range(9):
        rows_o, _ = cosine_similarity_search(Q[b], V, 150)
        assert np.array_equal(rows_o, res.pool_rows[b])
        want = best_snippets_oracle(reviews, E, Q[b], skus.iloc[rows_o].tolist(), max_rows=max_scan)
        got = engine.reviews.snippets(skus.iloc[res.pool_rows[b]].tolist(), res.best_ids[b], res.best_raw[b])
        assert set(got) == set(want)
        for s_, w_ in want.items():
            assert got[s_]["text"] == w_["text"] and abs(got[s_]["score"] - w_["score"]) < 1e-5


def test_best_review_pick_is_the_first_maximum_in_file_order(hip):
    """rr_reviews_best_dev / rr_reviews_best_cut_dev against np.argmax over each product's reviews in file order.
    Embeddings and queries are small integers times 2^-4, so every dot product is exact in any summation order and
    ties stay ties.  Products hold 0, 1, 2, 5, 15, 16, 17, 33, 64 and 300 reviews; for query 0 two copies of the best
    possible review sit in different waves or different 16-review steps of the kernel; the review-id cut falls inside
    the 300-review list; max_rows is the union size, one more, one less and 0."""
    import ctypes as C
    import torch
    from review_recommender_amd import _lib
    from review_recommender_amd.reviews import ReviewIndex
    rng = np.random.default_rng(21)
    dim, B, off = 384, 3, 100
    sizes = np.array([1, 15, 16, 17, 300, 0, 2, 5, 33, 64, 16, 17] * 3)
    n_prod = len(sizes)
    owner = np.concatenate([np.repeat(np.arange(n_prod), sizes), np.full(40, -1)])   # 40 reviews of unknown skus
    owner = owner[rng.permutation(len(owner))]                                        # file order
    Ei = rng.integers(-3, 4, (len(owner), dim))
    Qi = rng.integers(-3, 4, (B, dim))
    lists = [np.flatnonzero(owner == p) for p in range(n_prod)]
    pairs = {2: (0, 1), 15: (3, 12), 16: (1, 5), 17: (2, 16), 33: (7, 30), 64: (4, 60), 300: (5, 290)}
    for p, L in enumerate(lists):                   # (a, b): wave (position // 4) % 4 or step position // 16 differ
        if len(L) in pairs and p % 3 != 2:
            a, b = pairs[len(L)]
            Ei[L[a]] = Ei[L[b]] = 3 * np.sign(Qi[0])
    S = Ei @ Qi.T                                   # exact: the kernel's float32 sums times 2^8
    reviews = pd.DataFrame({"sku": [f"B{o:09d}" if o >= 0 else "X" for o in owner], "text": "t"})
    ri = ReviewIndex(reviews, (Ei * 0.0625).astype(np.float32), synth.skus(n_prod), eps=0.0)
    assert all(np.array_equal(ri.ids[ri.indptr[p]:ri.indptr[p + 1]], lists[p]) for p in range(n_prod))
    tied = [p for p, L in enumerate(lists) if len(L) > 1 and np.sum(S[L, 0] == S[L, 0].max()) > 1]
    assert len(tied) >= 16 and all(np.argmax(S[lists[p], 0]) != len(lists[p]) - 1 - np.argmax(S[lists[p], 0][::-1])
                                   for p in tied)   # a "last maximum" rule would pick another review
    rows = np.stack([np.concatenate([rng.permutation(n_prod), [-1, n_prod, n_prod + 50]]) + off for _ in range(B)])
    pool = rows.shape[1]
    q_dev = torch.from_numpy((Qi * 0.0625).astype(np.float32)).cuda()
    r_dev = torch.from_numpy(rows.astype(np.int64)).cuda()

    def run(cut=None, max_rows=None):
        score = torch.empty((B, pool), dtype=torch.float32, device="cuda")
        rid = torch.empty((B, pool), dtype=torch.int32, device="cuda")
        args = (ri.handle, C.c_void_p(q_dev.data_ptr()), B, C.c_void_p(r_dev.data_ptr()), pool, off)
        outs = (C.c_void_p(score.data_ptr()), C.c_void_p(rid.data_ptr()), None)
        torch.cuda.synchronize()
        if max_rows is None:
            _lib.check(hip.rr_reviews_best_dev(*args, cut, *outs), "rr_reviews_best_dev")
        else:
            _lib.check(hip.rr_reviews_best_cut_dev(*args, max_rows, *outs), "rr_reviews_best_cut_dev")
        torch.cuda.synchronize()
        return score.cpu().numpy(), rid.cpu().numpy()

    def expect(cut):
        score, rid = np.zeros((B, pool), np.float32), np.full((B, pool), -1, np.int32)
        for q in range(B):
            for c in range(pool):
                p = rows[q, c] - off
                if not 0 <= p < n_prod:
                    continue
                L = lists[p][lists[p] <= cut]
                if len(L):
                    j = int(np.argmax(S[L, q]))
                    score[q, c], rid[q, c] = np.float32(S[L[j], q] * 2.0 ** -8), L[j]
        return score, rid

    inside = int(lists[4][150])                     # a cut inside the 300-review list
    for cut in (len(owner), inside):
        got, want = run(cut=cut), expect(cut)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), cut
    union = np.sort(np.concatenate(lists))
    U = len(union)
    for max_rows, cut in ((U, len(owner)), (U + 1, len(owner)), (U - 1, int(union[U - 2])), (0, -1)):
        got, want = run(max_rows=max_rows), expect(cut)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), max_rows
    ri.close()
