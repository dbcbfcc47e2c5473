"""The best-review column (`_best`, snippets) on row shards (reviews.py, sharded.py, DESIGN.md sections 4 K4 and 5), on one
GPU: every shard holds the reviews of its own products, the `iloc[:max_rows]` cut is found across the shards by rounds of
256-way narrowing whose counts the test sums with torch, every shard picks the best review of the merged rows it owns, and
the picks are combined by owner.  Cuts, scores, ids, the eight columns and the order must equal the unsharded
`rr_reviews_best_cut_dev` / `HybridSearcher.search_batch(reviews=..., max_scan=...)` over the whole index bit for bit."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from review_recommender_amd import _lib, synth
from review_recommender_amd import text as T
from review_recommender_amd.engine import FusionWeights, HybridSearcher
from review_recommender_amd.gate import GateText
from review_recommender_amd.index import MAX_POOL, ProductIndex
from review_recommender_amd.reviews import ReviewIndex, cut_narrow, cut_rounds, cut_thresholds, model_cut
from review_recommender_amd.sharded import (ShardedSearcher, pack_picks, select_by_owner, shard_bounds, unpack_picks)
from test_gpu_reviews import make

pytestmark = pytest.mark.gpu

WORLDS = (2, 3, 8)


# ---------------------------------------------------------------------------------------------- 1. cut and pick
def exact_table(sizes, dim, n_unknown, seed, B=3):
    """The construction of test_best_review_pick_is_the_first_maximum_in_file_order: entries are small integers x 2^-4 (every
    dot product exact in any order, ties stay ties), file order shuffled, reviews of unknown skus among them, two copies
    of the best possible review for query 0 planted in the longer lists."""
    rng = np.random.default_rng(seed)
    n_prod = len(sizes)
    owner = np.concatenate([np.repeat(np.arange(n_prod), sizes), np.full(n_unknown, -1)])
    owner = owner[rng.permutation(len(owner))]
    Ei = rng.integers(-3, 4, (len(owner), dim))
    Qi = rng.integers(-3, 4, (B, dim))
    lists = [np.flatnonzero(owner == p) for p in range(n_prod)]
    pairs = {2: (0, 1), 15: (3, 12), 16: (1, 5), 17: (2, 16), 33: (7, 30), 64: (4, 60), 300: (5, 290)}
    for p, L in enumerate(lists):
        if len(L) in pairs and p % 3 != 2:
            a, b = pairs[len(L)]
            Ei[L[a]] = Ei[L[b]] = 3 * np.sign(Qi[0])
    reviews = pd.DataFrame({"sku": [f"B{o:09d}" if o >= 0 else "X" for o in owner], "text": "t"})
    E = (Ei * 0.0625).astype(np.float32)
    skus = synth.skus(n_prod)
    whole = ReviewIndex(reviews, E, skus, eps=0.0)
    shards = {w: [ReviewIndex.shard(reviews, E, skus, *shard_bounds(n_prod, w, r), eps=0.0) for r in range(w)] for w in WORLDS}
    q_dev = torch.from_numpy((Qi * 0.0625).astype(np.float32)).cuda()
    return dict(n_prod=n_prod, lists=lists, whole=whole, shards=shards, q_dev=q_dev, rng=rng, n_total=len(owner), B=B)


@pytest.fixture(scope="module")
def small():
    t = exact_table(np.array([1, 15, 16, 17, 300, 0, 2, 5, 33, 64, 16, 17] * 3), 384, 40, 21)
    assert t["n_total"] > 256 and cut_rounds(t["n_total"]) == 2
    return t


@pytest.fixture(scope="module")
def large():
    rng = np.random.default_rng(5)
    sizes = rng.multinomial(66_000 - 40, np.ones(600) / 600)
    sizes[[7, 300]] = 0
    t = exact_table(sizes, 32, 66_000 - int(sizes.sum()), 22)
    assert t["n_total"] == 66_000 and cut_rounds(t["n_total"]) == 3
    return t


def whole_best(hip, t, rows, max_rows):
    B, pool = rows.shape
    score = torch.empty((B, pool), dtype=torch.float32, device="cuda")
    rid = torch.empty((B, pool), dtype=torch.int32, device="cuda")
    _lib.check(hip.rr_reviews_best_cut_dev(t["whole"].handle, C.c_void_p(t["q_dev"].data_ptr()), B, C.c_void_p(rows.data_ptr()),
                                           pool, 0, max_rows, C.c_void_p(score.data_ptr()), C.c_void_p(rid.data_ptr()), None),
               "rr_reviews_best_cut_dev")
    torch.cuda.synchronize()
    return score.cpu().numpy(), rid.cpu().numpy()


def played_cuts(shards, rows, max_rows, n_prod, fused=True, model=None):
    """The rounds on every shard of a played world, the sums formed with torch: int32 (B,) cuts, the same on every shard.
    ``fused``: the narrowing rides in front of the next round's counting (the product's form); otherwise it is a launch
    of its own.  ``model``: per query the candidates' id lists -- every round's sums and narrowed interval are then also
    checked against the numpy statement."""
    B = rows.shape[0]
    if max_rows <= 0:
        return torch.full((B,), -1, dtype=torch.int32, device="cuda")
    los = [shard_bounds(n_prod, len(shards), r)[0] for r in range(len(shards))]
    n_total = shards[0].n_total
    states = [sh.cut_begin(B) for sh in shards]
    assert all(st.cpu().tolist() == [[0, n_total - 1]] * B for st in states)
    R, sums = cut_rounds(n_total), None
    expect = [(0, n_total - 1)] * B

    def narrowed(first):                                    # every shard's interval = the numpy narrowing of the last one
        sums_h = sums.cpu().numpy()
        want = [cut_narrow(lo, hi, sums_h[q], max_rows, first, n_total) for q, (lo, hi) in enumerate(expect)]
        assert all(st.cpu().tolist() == [list(x) for x in want] for st in states), first
        return want

    for r in range(R):
        if fused or r == 0:
            counts = [sh.cut_counts(st, rows, max_rows, lo, sums=sums, first=r == 1) for sh, st, lo in zip(shards, states, los)]
        else:
            for sh, st in zip(shards, states):
                sh.cut_narrow(st, sums, max_rows, first=r == 1)
            counts = [sh.cut_counts(st, rows, max_rows, lo) for sh, st, lo in zip(shards, states, los)]
        assert all(c.dtype == torch.int64 and c.shape == (B, 256) for c in counts)
        if model is not None:
            if r > 0:
                expect = narrowed(r == 1)
            total = torch.stack(counts).sum(0).cpu().numpy()
            for q in range(B):                              # the summed counts at the model's thresholds
                Tq = cut_thresholds(*expect[q])
                assert np.array_equal(total[q], sum(np.searchsorted(L, Tq, side="right") for L in model[q])), (r, q)
        sums = torch.stack(counts).sum(0)
    cuts = [sh.cut_end(st, sums, max_rows, first=R == 1) for sh, st in zip(shards, states)]
    if model is not None:
        narrowed(R == 1)
    assert all(torch.equal(c, cuts[0]) for c in cuts) and all(torch.equal(st, states[0]) for st in states)
    assert torch.equal(states[0][:, 0], states[0][:, 1]) and torch.equal(states[0][:, 0].to(torch.int32), cuts[0])
    return cuts[0]


def played_picks(shards, q_dev, rows, cuts, n_prod):
    los = [shard_bounds(n_prod, len(shards), r)[0] for r in range(len(shards))]
    words = torch.stack([pack_picks(*sh.best_at(q_dev, rows, cuts, lo)) for sh, lo in zip(shards, los)])
    raw, ids = unpack_picks(select_by_owner(words, rows, n_prod))
    torch.cuda.synchronize()
    return raw.cpu().numpy(), ids.cpu().numpy()


def candidate_rows(t):
    """Every product in random order plus rows -1 and beyond the corpus; the last query sees only half of the products."""
    n_prod, rng = t["n_prod"], np.random.default_rng(3)
    rows = np.stack([np.concatenate([rng.permutation(n_prod), [-1, n_prod, n_prod + 50]]) for _ in range(t["B"])])
    rows[-1, : n_prod // 2] = -1
    return rows.astype(np.int64)


def check_world(hip, t, size, rows, max_rows, fused=True, model=False):
    shards, n_prod, lists = t["shards"][size], t["n_prod"], t["lists"]
    r_dev = torch.from_numpy(rows).cuda()
    per_query = [[lists[p] for p in rows[q] if 0 <= p < n_prod] for q in range(rows.shape[0])]
    cuts = played_cuts(shards, r_dev, max_rows, n_prod, fused, per_query if model else None).cpu().numpy()
    for q, cand in enumerate(per_query):
        union = np.sort(np.concatenate(cand))
        want = t["whole"].cut_for(rows[q], max_rows)
        assert np.array_equal(union <= cuts[q], union <= want), (size, max_rows, q, cuts[q], want)   # the same kept set
        ranks = [[lists[p] for p in rows[q] if lo <= p < hi] for lo, hi in (shard_bounds(n_prod, size, r) for r in range(size))]
        assert cuts[q] == model_cut(ranks, max_rows, t["n_total"]), (size, max_rows, q)
    got = played_picks(shards, t["q_dev"], r_dev, torch.from_numpy(cuts).cuda(), n_prod)
    want = whole_best(hip, t, r_dev, max_rows)
    assert np.array_equal(got[1], want[1]), (size, max_rows)
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (size, max_rows)
    assert (got[1][:, -3:] == -1).all() and not got[0][:, -3:].any(), "rows -1 and rows beyond the corpus have no review"
    return cuts, got


@pytest.mark.parametrize("size", WORLDS)
def test_cut_and_pick_across_shards_equal_the_whole_index_bitwise(hip, small, size):
    t = small
    n_prod, lists = t["n_prod"], t["lists"]
    rows = candidate_rows(t)
    union = np.sort(np.concatenate(lists))
    U = len(union)
    inside = int(np.searchsorted(union, lists[4][150])) + 1                      # the cut falls inside the 300-review list
    ends = [shard_bounds(n_prod, size, r)[1] - 1 for r in range(size)]
    last = next(p for p in ends if len(lists[p]) and lists[p][-1] != union[-1])  # the last review of a shard's last product
    at_end = int(np.searchsorted(union, lists[last][-1])) + 1
    seen_cut, seen_all = False, False
    for max_rows in (U, U + 1, U - 1, 1, 0, inside, at_end):
        cuts, (raw, ids) = check_world(hip, t, size, rows, max_rows, model=True)
        if max_rows == inside:
            assert cuts[0] == lists[4][150]
        if max_rows == at_end:
            assert cuts[0] == lists[last][-1]
        if max_rows == U:
            assert (cuts == t["n_total"]).all() and (ids[:, :n_prod] >= 0).sum() > n_prod
        if max_rows == 0:
            assert (cuts == -1).all() and (ids == -1).all()
        seen_cut |= bool((cuts < t["n_total"]).any() and (cuts >= 0).any())
        seen_all |= bool((cuts == t["n_total"]).any())
    assert seen_cut and seen_all
    # the narrowing as a launch of its own gives the same rounds
    check_world(hip, t, size, rows, inside, fused=False, model=True)


@pytest.mark.parametrize("size", WORLDS)
def test_three_rounds_over_a_table_of_66000_reviews(hip, large, size):
    t = large
    rows = candidate_rows(t)
    lists = t["lists"]
    union = np.sort(np.concatenate(lists))
    U = len(union)
    for max_rows in (U, U - 1, 1, U // 3, 65_537):
        cuts, _ = check_world(hip, t, size, rows, max_rows, model=max_rows == U // 3)
        if max_rows == U // 3:
            assert cuts[0] == union[max_rows - 1]


# ---------------------------------------------------------------------------------------------- 2. end to end
W_BEST = FusionWeights(w_dense=0.5, w_bm25=0.0, w_rerank=0.0, w_prior=0.1, w_best=0.4, gate_penalty=1.0)
K, POOL, BATCH = 10, 150, 9


def searcher(V, n_rev, stars, lo, hi, gate_texts=None):
    ix = ProductIndex(V[lo:hi], row_offset=lo)
    ix.set_meta(n_rev[lo:hi], stars[lo:hi])
    gt = GateText.from_texts(gate_texts[lo:hi], 0, row_offset=lo) if gate_texts is not None else None
    return HybridSearcher(ix, None, gate_text=gt)


@pytest.fixture(scope="module")
def corpus():
    meta, V, reviews, E = make()                   # 3 000 products, 20 000 reviews: a shard of eight still holds >= 150 rows
    n = len(meta)
    skus = meta["sku"].astype(str).tolist()
    n_rev, stars = meta["n_reviews"].to_numpy(np.float64), meta["avg_stars"].to_numpy(np.float64)
    c = dict(n=n, V=V, skus=skus, reviews=reviews, E=E, n_rev=n_rev, stars=stars, texts=meta["agg_text"].tolist())
    c["whole"] = searcher(V, n_rev, stars, 0, n, c["texts"])
    c["whole_reviews"] = ReviewIndex(reviews, E, skus)
    c["Q"] = synth.unit_rows(BATCH, 384, 77)
    c["worlds"] = {}
    return c


def world_of(c, size):
    """The played shards of one world size, their payloads of the batch gathered, and pass A's merged rows."""
    if size not in c["worlds"]:
        n, shards = c["n"], []
        for r in range(size):
            lo, hi = shard_bounds(n, size, r)
            rv = ReviewIndex.shard(c["reviews"], c["E"], c["skus"], lo, hi)
            shards.append(ShardedSearcher(searcher(c["V"], c["n_rev"], c["stars"], lo, hi), n, r, size, reviews=rv))
        tops = np.concatenate([sh.reviews.top_counts(MAX_POOL) for sh in shards])
        for sh in shards:
            assert sh.review_tops is None, "no process group: the test supplies what the ranks would have exchanged"
            sh.review_tops = tops
        q_dev = torch.from_numpy(c["Q"]).cuda()
        lay, bufs = None, []
        for sh in shards:
            lay, buf = sh.local_payload(q_dev, [[] for _ in range(BATCH)], POOL)
            bufs.append(buf)
        gathered = torch.stack(bufs)
        merged, _, _ = shards[0].merge(lay, gathered, BATCH, POOL, POOL, POOL, W_BEST)
        c["worlds"][size] = (shards, q_dev, lay, gathered, merged)
    return c["worlds"][size]


def played_best(shards, q_dev, rows, max_scan, n):
    """ShardedSearcher.best_column with the collectives played: sums by torch, picks stacked as the all-gather leaves them."""
    B, pool = rows.shape
    plans = {sh.review_plan(pool, max_scan) for sh in shards}
    assert len(plans) == 1
    plan = plans.pop()
    if plan == "none":
        return plan, torch.zeros((B, pool), dtype=torch.float32, device="cuda"), torch.full((B, pool), -1, dtype=torch.int32,
                                                                                            device="cuda")
    if plan == "rounds":
        # every shard's review_cuts in lock step: the reduction of round r is the sum of all shards' round-r counts
        cuts = [played_cuts([sh.reviews for sh in shards], rows, max_scan, n)] * len(shards)
    else:
        cuts = [torch.full((B,), sh.reviews.n_total, dtype=torch.int32, device="cuda") for sh in shards]
    words = torch.stack([sh.best_local(q_dev, rows, c_) for sh, c_ in zip(shards, cuts)])
    raw, ids = unpack_picks(select_by_owner(words, rows, n))
    return plan, raw, ids


@pytest.mark.parametrize("max_scan", [300000, 150, 37, 1, 0])
@pytest.mark.parametrize("size", WORLDS)
def test_played_shards_equal_the_unsharded_search_with_reviews_bitwise(corpus, size, max_scan):
    c = corpus
    ref = c["whole"].search_batch(c["Q"], None, K, 0, W_BEST, reviews=c["whole_reviews"], max_scan=max_scan)
    plain = c["whole"].search_batch(c["Q"], None, K, 0, W_BEST)
    assert ref.pool == POOL
    if max_scan > 1:
        assert not np.array_equal(ref.columns[:, 7], plain.columns[:, 7]), "_best changes _final"
        assert not np.array_equal(ref.order, plain.order), "... and the order"
        assert (ref.best_ids >= 0).sum() > BATCH * 10
    shards, q_dev, lay, gathered, merged = world_of(c, size)
    assert np.array_equal(merged.cpu().numpy(), ref.pool_rows)
    plan, raw, ids = played_best(shards, q_dev, merged, max_scan, c["n"])
    assert plan == {300000: "skip", 150: "rounds", 37: "rounds", 1: "rounds", 0: "none"}[max_scan]
    rows, cols, order = [t.cpu().numpy() for t in shards[0].merge(lay, gathered, BATCH, K, POOL, POOL, W_BEST, best=raw)]
    raw, ids = raw.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(ids, ref.best_ids)
    assert np.array_equal(raw.view(np.int32), ref.best_raw.view(np.int32))
    assert np.array_equal(rows, ref.pool_rows)
    assert np.array_equal(cols, ref.columns, equal_nan=True)
    assert np.array_equal(order, ref.order)
    for b in (0, BATCH - 1):                     # texts / stars are the whole table's on every rank: global ids index them
        skus = [c["skus"][r] for r in rows[b]]
        want = c["whole_reviews"].snippets(skus, ref.best_ids[b], ref.best_raw[b])
        assert shards[-1].reviews.snippets(skus, ids[b], raw[b]) == want
        assert len(want) > 20 or max_scan < 150


# ---------------------------------------------------------------------------------------------- 3. one rank
N_BIG, POOL_BIG = 20_000, 37


@pytest.fixture(scope="module")
def big():
    """A corpus large enough for the two-phase K1 at pool 37 (test_gpu_sharded_gate.py): plain batches stay in the pipeline."""
    n, n_r = N_BIG, 30_000
    V = synth.unit_rows(n, 384, 71)
    near = V[7] + 0.05 * V[:40]                                              # products 0 .. 39 side by side: one query's pool
    V[:40] = near / np.linalg.norm(near, axis=1, keepdims=True)
    n_rev, stars = synth.metadata(n, 72, nan_fraction=0.0)
    rng = np.random.default_rng(73)
    owner = rng.integers(0, n + 500, n_r)
    owner[rng.integers(0, n_r, 3000)] = rng.integers(0, 40, 3000)            # a few products with many reviews
    E = rng.standard_normal((n_r, 384)).astype(np.float32)
    reviews = pd.DataFrame({"sku": [f"B{o:09d}" for o in owner], "text": [f"r{i}" for i in range(n_r)],
                            "stars": rng.integers(1, 6, n_r).astype(np.float64)})
    skus = synth.skus(n)
    Qs = [synth.unit_rows(b, 384, 80 + i) for i, b in enumerate((8, 5, 8))]
    for Q in Qs:
        Q[0] = V[7]                                                          # ... with ~75 reviews each: the cut bites
    s = searcher(V, n_rev.astype(np.float64), stars, 0, n)
    return dict(n=n, s=s, whole=ReviewIndex(reviews, E, skus), shard=ReviewIndex.shard(reviews, E, skus, 0, n), Qs=Qs)


def test_one_rank_payload_path_submit_finish_and_the_overlapped_pipeline(big):
    b = big
    sh = ShardedSearcher(b["s"], b["n"], 0, 1, reviews=b["shard"])
    assert sh.review_tops is not None and len(b["shard"].global_ids) < b["whole"].n_reviews, "local ids differ from global ids"
    kw = dict(pool_floor=POOL_BIG, reviews=True, max_scan=60)
    refs = [b["s"].search_batch(Q, None, K, 0, W_BEST, pool_floor=POOL_BIG, reviews=b["whole"], max_scan=60) for Q in b["Qs"]]
    assert any((r.best_ids >= 0).sum(axis=1).max() > 5 for r in refs)

    def same(res, out, ref):
        rows, cols, order = [t.cpu().numpy() for t in res]
        assert np.array_equal(rows, ref.pool_rows) and np.array_equal(cols, ref.columns, equal_nan=True)
        assert np.array_equal(order, ref.order)
        assert np.array_equal(out["best_ids"].cpu().numpy(), ref.best_ids)
        assert np.array_equal(out["best_raw"].cpu().numpy().view(np.int32), ref.best_raw.view(np.int32))

    q_devs = [torch.from_numpy(Q).cuda() for Q in b["Qs"]]
    for force in (True, False):
        sh.force_payload = force
        rounds = sh.review_rounds_run
        for q, ref in zip(q_devs, refs):
            out = {}
            same(sh.search_batch_dev(q, None, K, W_BEST, best_out=out, **kw), out, ref)
        assert (sh.review_rounds_run > rounds) == force, "the payload path runs the rounds, the straight path the bisection"
    sh.force_payload = True
    outs = [{} for _ in q_devs]
    tickets = [sh.submit(q, None, K, W_BEST, best_out=o, **kw) for q, o in zip(q_devs, outs)]
    assert all(t.two_pass and t.slot < 0 for t in tickets)
    for t, o, ref in zip(tickets, outs, refs):
        same(sh.finish(t), o, ref)
    # max_scan large: the rounds are skipped; max_scan 0: nothing is scored
    for max_scan, plan in ((300000, "skip"), (0, "none")):
        assert sh.review_plan(POOL_BIG, max_scan) == plan
        rounds, out = sh.review_rounds_run, {}
        ref = b["s"].search_batch(b["Qs"][0], None, K, 0, W_BEST, pool_floor=POOL_BIG, reviews=b["whole"], max_scan=max_scan)
        same(sh.search_batch_dev(q_devs[0], None, K, W_BEST, pool_floor=POOL_BIG, reviews=True, max_scan=max_scan, best_out=out),
             out, ref)
        assert sh.review_rounds_run == rounds
    assert sh.review_plan(POOL_BIG, 60) == "rounds"

    plain = [[t.cpu().numpy() for t in sh.search_batch_dev(q, None, K, W_BEST, pool_floor=POOL_BIG)] for q in q_devs]
    assert sh.enable_overlap(160)
    try:
        pins = [torch.from_numpy(Q).pin_memory() for Q in b["Qs"]]
        out = {}
        t0 = sh.submit(pins[0], None, K, W_BEST, pool_floor=POOL_BIG)
        t1 = sh.submit(pins[1], None, K, W_BEST, best_out=out, **kw)
        t2 = sh.submit(pins[2], None, K, W_BEST, pool_floor=POOL_BIG)
        assert t0.slot >= 0 and t2.slot >= 0, "plain batches stay in the pipeline"
        assert t1.slot < 0 and t1.two_pass, "a batch with reviews leaves it, in order"
        got0 = [t.cpu().numpy() for t in sh.finish(t0)]
        same(sh.finish(t1), out, refs[1])
        got2 = [t.cpu().numpy() for t in sh.finish(t2)]
        assert all(np.array_equal(a, p, equal_nan=True) for a, p in zip(got0, plain[0]))
        assert all(np.array_equal(a, p, equal_nan=True) for a, p in zip(got2, plain[2]))
    finally:
        sh.disable_overlap()


# ---------------------------------------------------------------------------------------------- 4. with other columns
def test_reviews_with_a_reranker_and_gate_groups_equal_the_unsharded_batch(corpus):
    c = corpus
    wts = FusionWeights(w_dense=0.3, w_bm25=0.0, w_rerank=0.3, w_prior=0.1, w_best=0.3, gate_penalty=0.5)
    rr_k = 20
    groups = [T.build_gate_groups(q) for q in ("wireless yellow cat socks", "red blue wireless keyboard", "dog design pattern")] * 3
    score = lambda qi, rows: (np.sin(rows * 0.001) + qi * 0.1).astype(np.float32)
    ref = c["whole"].search_batch(c["Q"], None, K, rr_k, wts, gate_groups=groups, reviews=c["whole_reviews"], max_scan=150,
                                  rerank_fn=lambda rows: score(np.arange(rows.shape[0])[:, None], rows))
    assert (ref.columns[:, 3, :rr_k] != 0).any() and (ref.columns[:, 4] != 0).any() and (ref.columns[:, 5] != 1.0).any()
    sh = ShardedSearcher(c["whole"], c["n"], 0, 1, reviews=ReviewIndex.shard(c["reviews"], c["E"], c["skus"], 0, c["n"]))
    q_dev = torch.from_numpy(c["Q"]).cuda()
    for force in (True, False):
        sh.force_payload = force
        out = {}
        rows, cols, order = [t.cpu().numpy() for t in sh.search_batch_dev(
            q_dev, None, K, wts, rerank_k=rr_k, rerank_fn=score, gate_groups=groups, reviews=True, max_scan=150, best_out=out)]
        assert np.array_equal(rows, ref.pool_rows), force
        assert np.array_equal(cols, ref.columns, equal_nan=True), force
        assert np.array_equal(order, ref.order), force
        assert np.array_equal(out["best_ids"].cpu().numpy(), ref.best_ids), force
    c["whole"].gate_text.check()


# ---------------------------------------------------------------------------------------------- 5. argument errors
def test_review_argument_errors_are_raised_before_anything_runs(corpus):
    c = corpus
    n = c["n"]
    q_dev = torch.from_numpy(c["Q"]).cuda()
    lo, hi = shard_bounds(n, 2, 1)
    part = ReviewIndex.shard(c["reviews"], c["E"], c["skus"], lo, hi)
    with pytest.raises(ValueError, match="review index is over rows"):
        ShardedSearcher(c["whole"], n, 0, 1, reviews=part)
    bare = ShardedSearcher(c["whole"], n, 0, 1)
    wrong = ShardedSearcher(c["whole"], n, 0, 1, reviews=c["whole_reviews"])
    wrong.reviews = part                        # (an index swapped in after construction)

    def launches(s):
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(s.s.lib.rr_index_scan_stats(s.s.index.handle, C.byref(ms), C.byref(cnt)), "rr_index_scan_stats")
        return cnt.value

    torch.cuda.synchronize()
    launches(bare)
    for force in (False, True):
        bare.force_payload = wrong.force_payload = force
        with pytest.raises(ValueError, match="needs the review index"):
            bare.search_batch_dev(q_dev, None, K, W_BEST, reviews=True, max_scan=150)
        with pytest.raises(ValueError, match="needs the review index"):
            bare.submit(q_dev, None, K, W_BEST, reviews=True, max_scan=150)
        with pytest.raises(ValueError, match="not this rank's"):
            wrong.search_batch_dev(q_dev, None, K, W_BEST, reviews=True, max_scan=150)
    played = ShardedSearcher(searcher(c["V"], c["n_rev"], c["stars"], lo, hi), n, 1, 2, reviews=part)
    with pytest.raises(ValueError, match="have not been exchanged"):
        played._plan(q_dev, None, K, W_BEST, 150, 0, None, None, None, None, None, True)
    torch.cuda.synchronize()
    assert launches(bare) == 0
