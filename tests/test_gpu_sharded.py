"""The multi-GPU data path on ONE GPU: the corpus is cut into row shards that all live on
cuda:0, every shard builds its payload exactly as a rank would (K1 + K2 + metadata gather into
the packed buffer), the buffers are laid out as the all-gather would leave them, and K3 merges
+ fuses with the [rank][query][pool] addressing.  The result must equal the unsharded result
bit for bit.  The collective itself is covered on CPU (gloo) in
tests/test_sharded_gloo.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from review_recommender_amd import _lib, synth
from review_recommender_amd.bm25 import BM25Corpus
from review_recommender_amd.engine import FusionWeights, HybridSearcher
from review_recommender_amd.index import ProductIndex
from review_recommender_amd.sharded import PayloadLayout, ShardedSearcher, shard_bounds

pytestmark = pytest.mark.gpu


def build(V, n_rev, stars, corpus, lo, hi):
    ix = ProductIndex(V[lo:hi], row_offset=lo)
    ix.set_meta(n_rev[lo:hi], stars[lo:hi])
    bm = corpus.slice(lo, hi).to_device(row_offset=lo)
    return HybridSearcher(ix, bm)


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("batch", [1, 5, 20])
def test_sharded_equals_unsharded_bitwise(world, batch):
    n, vocab = 40_000, 3000
    V = synth.unit_rows(n, 384, 61)
    V[1000] = V[39_000]                       # an exact tie across shards: the smaller row must win
    n_rev, stars = synth.metadata(n, 62, nan_fraction=0.01)
    ip, terms, tf, dl = synth.bm25_forward_csr(n, vocab, 30, 63)
    corpus = BM25Corpus(ip, terms, tf, dl, vocab)
    Q = synth.unit_rows(batch, 384, 64)
    Q[0] = V[1000]
    tl = synth.query_terms(batch, vocab, 65, np.bincount(terms, minlength=vocab))
    w = FusionWeights(w_dense=0.5, w_bm25=0.3, w_rerank=0.0, w_prior=0.2, w_best=0.0, gate_penalty=1.0)
    k, pool = 100, 150

    whole = build(V, n_rev.astype(np.float64), stars, corpus, 0, n)
    ref = ShardedSearcher(whole, n, 0, 1)
    q_dev = torch.from_numpy(Q).cuda()
    want_rows, want_cols, want_order = [t.cpu().numpy() for t in ref.search_batch_dev(q_dev, tl, k, w)]

    shards = []
    for r in range(world):
        lo, hi = shard_bounds(n, world, r)
        shards.append(ShardedSearcher(build(V, n_rev.astype(np.float64), stars, corpus, lo, hi), n, r, world))
    lay = PayloadLayout(batch, pool)
    gathered = torch.empty((world, lay.nbytes), dtype=torch.uint8, device="cuda")
    for r, sh in enumerate(shards):
        _, buf = sh.local_payload(q_dev, tl, pool)
        gathered[r].copy_(buf)
    s0 = shards[0].s
    params = HybridSearcher.make_params(w, k, pool, world * pool, 0, cand_per_rank=pool, stride_bytes=lay.nbytes)
    out_rows = torch.empty((batch, pool), dtype=torch.int64, device="cuda")
    cols = torch.empty((batch, 8, pool), dtype=torch.float64, device="cuda")
    order = torch.empty((batch, k), dtype=torch.int32, device="cuda")
    base = gathered.data_ptr()
    p = lambda off: C.c_void_p(base + off)
    _lib.check(s0.lib.rr_fuse_topk_dev(
        s0.index.handle, C.byref(params), batch, p(lay.off_rows), p(lay.off_dense), p(lay.off_bm25),
        p(lay.off_n), p(lay.off_avg), p(lay.off_l1p), None, None, None, C.c_void_p(out_rows.data_ptr()),
        C.c_void_p(cols.data_ptr()), C.c_void_p(order.data_ptr()), s0._stream()), "rr_fuse_topk_dev")
    torch.cuda.synchronize()
    assert np.array_equal(out_rows.cpu().numpy(), want_rows)
    assert np.array_equal(cols.cpu().numpy(), want_cols, equal_nan=True)
    assert np.array_equal(order.cpu().numpy(), want_order)
    # ShardedSearcher.merge (what finish runs) on the same gathered buffer: the raw call's three arrays, bit for bit
    for got, raw in zip(shards[0].merge(lay, gathered, batch, k, pool, pool, w), (out_rows, cols, order)):
        assert got.dtype == raw.dtype and got.shape == raw.shape and got.data_ptr() != raw.data_ptr()
        assert got.cpu().numpy().tobytes() == raw.cpu().numpy().tobytes()
    r0 = want_rows[0].tolist()
    assert r0.index(1000) + 1 == r0.index(39_000)      # tie: ascending global row


def test_eight_shards_merge_up_to_the_candidate_limit_and_refuse_more():
    """K3 merges at most RR_MAX_CANDIDATES = 4096 candidates per query, world x pool of them on row shards: 8 shards
    at pool 512 (the limit exactly) merge bit for bit to the unsharded answer; pool 513 is refused with a ValueError
    naming the limit before anything runs -- no scan is launched, and no collective is entered."""
    n, vocab, world, batch, pool = 40_000, 3000, 8, 3, 512
    V = synth.unit_rows(n, 384, 61)
    n_rev, stars = synth.metadata(n, 62, nan_fraction=0.01)
    ip, terms, tf, dl = synth.bm25_forward_csr(n, vocab, 30, 63)
    corpus = BM25Corpus(ip, terms, tf, dl, vocab)
    Q = synth.unit_rows(batch, 384, 66)
    tl = synth.query_terms(batch, vocab, 67, np.bincount(terms, minlength=vocab))
    w = FusionWeights(w_dense=0.5, w_bm25=0.3, w_rerank=0.0, w_prior=0.2, w_best=0.0, gate_penalty=1.0)
    q_dev = torch.from_numpy(Q).cuda()
    whole = ShardedSearcher(build(V, n_rev.astype(np.float64), stars, corpus, 0, n), n, 0, 1)
    want = [t.cpu().numpy() for t in whole.search_batch_dev(q_dev, tl, pool, w)]
    shards = [ShardedSearcher(build(V, n_rev.astype(np.float64), stars, corpus, *shard_bounds(n, world, r)), n, r, world)
              for r in range(world)]

    def launches(sh):
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(sh.s.lib.rr_index_scan_stats(sh.s.index.handle, C.byref(ms), C.byref(cnt)), "rr_index_scan_stats")
        return cnt.value

    launches(shards[0])
    with pytest.raises(ValueError, match="4096"):
        shards[0].search_batch_dev(q_dev, tl, pool + 1, w)
    with pytest.raises(ValueError, match="4096"):
        shards[0].submit(q_dev, tl, 10, w, rerank_k=pool + 1)
    torch.cuda.synchronize()
    assert launches(shards[0]) == 0
    lay = PayloadLayout(batch, pool)
    gathered = torch.empty((world, lay.nbytes), dtype=torch.uint8, device="cuda")
    for r, sh in enumerate(shards):
        _, buf = sh.local_payload(q_dev, tl, pool)
        gathered[r].copy_(buf)
    out_rows, cols, order = shards[0].merge(lay, gathered, batch, pool, pool, pool, w)
    torch.cuda.synchronize()
    assert np.array_equal(out_rows.cpu().numpy(), want[0])
    assert np.array_equal(cols.cpu().numpy(), want[1], equal_nan=True)
    assert np.array_equal(order.cpu().numpy(), want[2])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_config4_shape_bf16_batch_256_sharded_equals_unsharded(dtype):
    """BASELINE config 4's shape on one GPU: batch 256 (two 128-query filter-scan launches per shard), bf16 or
    fp32 storage, 8 shards: merged answer == unsharded answer, bit for bit."""
    n, vocab, world, batch, k, pool = 640_000, 5000, 8, 256, 100, 150
    V = synth.unit_rows(n, 384, 71)
    n_rev, stars = synth.metadata(n, 72, nan_fraction=0.0)
    ip, terms, tf, dl = synth.bm25_forward_csr(n, vocab, 20, 73)
    corpus = BM25Corpus(ip, terms, tf, dl, vocab)
    Q = synth.unit_rows(batch, 384, 74)
    tl = synth.query_terms(batch, vocab, 75, np.bincount(terms, minlength=vocab))
    w = FusionWeights(w_dense=0.5, w_bm25=0.5, w_rerank=0.0, w_prior=0.0, w_best=0.0, gate_penalty=1.0)

    def build_t(lo, hi):
        ix = ProductIndex.from_rows(V[lo:hi], row_offset=lo, dtype=dtype)
        ix.set_meta(n_rev[lo:hi].astype(np.float64), stars[lo:hi])
        return HybridSearcher(ix, corpus.slice(lo, hi).to_device(row_offset=lo))

    q_dev = torch.from_numpy(Q).cuda()
    whole = ShardedSearcher(build_t(0, n), n, 0, 1)
    want = [t.cpu().numpy() for t in whole.search_batch_dev(q_dev, tl, k, w)]
    lay = PayloadLayout(batch, pool)
    gathered = torch.empty((world, lay.nbytes), dtype=torch.uint8, device="cuda")
    first = None
    for r in range(world):
        lo, hi = shard_bounds(n, world, r)
        sh = ShardedSearcher(build_t(lo, hi), n, r, world)
        _, buf = sh.local_payload(q_dev, tl, pool)
        gathered[r].copy_(buf)
        torch.cuda.synchronize()
        first = first or sh
    out_rows, cols, order = first.merge(lay, gathered, batch, k, pool, pool, w)
    torch.cuda.synchronize()
    assert np.array_equal(out_rows.cpu().numpy(), want[0])
    assert np.array_equal(cols.cpu().numpy(), want[1], equal_nan=True)
    assert np.array_equal(order.cpu().numpy(), want[2])


def test_gate_and_rerank_columns_travel_through_the_payload_path():
    """configs with gate_penalty < 1 or rerank_k > 0 on the sharded path.  The payload + merge
    path (forced on one rank) with host gate / rerank callables over the MERGED pool must equal the straight
    K1 -> K2 -> K3 path with the same callables, bit for bit; the rerank callable sees exactly its rank's share."""
    n, vocab, batch, k, rr_k = 60_000, 3000, 6, 20, 200
    V = synth.unit_rows(n, 384, 81)
    n_rev, stars = synth.metadata(n, 82)
    ip, terms, tf, dl = synth.bm25_forward_csr(n, vocab, 25, 83)
    corpus = BM25Corpus(ip, terms, tf, dl, vocab)
    Q = synth.unit_rows(batch, 384, 84)
    tl = synth.query_terms(batch, vocab, 85, np.bincount(terms, minlength=vocab))
    w = FusionWeights(w_dense=0.4, w_bm25=0.2, w_rerank=0.3, w_prior=0.1, w_best=0.0, gate_penalty=0.5)
    seen = []

    def gate_fn(rows):
        return np.where(rows % 3 == 0, 0.5, 1.0).astype(np.float32)

    def rerank_fn(qi, rows):
        seen.append((qi.copy(), rows.copy()))
        return (np.sin(rows * 0.001) + qi * 0.1).astype(np.float32)

    q_dev = torch.from_numpy(Q).cuda()
    sh = ShardedSearcher(build(V, n_rev.astype(np.float64), stars, corpus, 0, n), n, 0, 1)
    a = [t.cpu().numpy() for t in sh.search_batch_dev(q_dev, tl, k, w, rerank_k=rr_k, gate_fn=gate_fn, rerank_fn=rerank_fn)]
    sh.force_payload = True
    b = [t.cpu().numpy() for t in sh.search_batch_dev(q_dev, tl, k, w, rerank_k=rr_k, gate_fn=gate_fn, rerank_fn=rerank_fn)]
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    pool = a[0].shape[1]
    assert pool == 200 and a[1].shape == (batch, 8, pool)
    assert all(len(qi) == batch * rr_k for qi, _ in seen)                 # world 1: the whole pair list
    assert np.array_equal(seen[0][1].reshape(batch, rr_k), a[0][:, :rr_k])  # pairs are the pool's first rr_k rows, in order
    gate_col, rr_col = a[1][:, 5], a[1][:, 3]
    assert np.array_equal(gate_col, gate_fn(a[0]).astype(np.float64))
    assert np.all(rr_col.max(axis=1) > 0.999) and np.all(rr_col.min(axis=1) == 0)   # min-max of the reranker scores
    no_gate = [t.cpu().numpy() for t in sh.search_batch_dev(q_dev, tl, k, w, rerank_k=rr_k, rerank_fn=rerank_fn)]
    assert not np.array_equal(no_gate[1][:, 7], a[1][:, 7])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_shards_select_against_a_corpus_wide_floor(dtype):
    """Two-phase K1 of row shards (include/rr_hip.h: rr_dense_scan_dev / rr_dense_select_dev): every
    shard scans and reports, per query, a lower bound of the score of its ceil(pool / shards)-th best row; the minimum over
    the shards is a lower bound of the corpus-wide pool-th best score, and every shard then opens only what can reach it.
    8 shards played in one process: the merged answer equals the unsharded one bit for bit, and the shards rescored a
    fraction of the M-tiles their own thresholds would have opened."""
    n, vocab, world, batch, k, pool = 640_000, 5000, 8, 256, 100, 150
    V = synth.unit_rows(n, 384, 71)
    n_rev, stars = synth.metadata(n, 72, nan_fraction=0.0)
    ip, terms, tf, dl = synth.bm25_forward_csr(n, vocab, 20, 73)
    corpus = BM25Corpus(ip, terms, tf, dl, vocab)
    Q = synth.unit_rows(batch, 384, 74)
    tl = synth.query_terms(batch, vocab, 75, np.bincount(terms, minlength=vocab))
    w = FusionWeights(w_dense=0.5, w_bm25=0.5, w_rerank=0.0, w_prior=0.0, w_best=0.0, gate_penalty=1.0)

    def build_t(lo, hi):
        ix = ProductIndex.from_rows(V[lo:hi], row_offset=lo, dtype=dtype)
        ix.set_meta(n_rev[lo:hi].astype(np.float64), stars[lo:hi])
        return HybridSearcher(ix, corpus.slice(lo, hi).to_device(row_offset=lo))

    q_dev = torch.from_numpy(Q).cuda()
    whole = ShardedSearcher(build_t(0, n), n, 0, 1)
    want = [t.cpu().numpy() for t in whole.search_batch_dev(q_dev, tl, k, w)]
    shards = [ShardedSearcher(build_t(*shard_bounds(n, world, r)), n, r, world) for r in range(world)]
    # plain per-shard selection first: how many M-tiles each shard opens on its own threshold
    own = []
    for sh in shards:
        sh.local_payload(q_dev, tl, pool, floor=False)
        torch.cuda.synchronize()
        own.append(sh.s.index.select_trace()[2])
    bounds = [sh.local_scan(q_dev, pool) for sh in shards]
    assert all(b is not None for b in bounds), "a 256-query batch on an 80 000-row shard takes the filter path"
    floor = torch.stack(bounds).min(dim=0).values
    assert torch.isfinite(floor).all()
    lay = PayloadLayout(batch, pool)
    gathered = torch.empty((world, lay.nbytes), dtype=torch.uint8, device="cuda")
    opened = []
    for r, sh in enumerate(shards):
        _, buf = sh.local_payload(q_dev, tl, pool, floor=floor)
        gathered[r].copy_(buf)
        torch.cuda.synchronize()
        assert sh.s.index.select_trace()[0] == 2
        opened.append(sh.s.index.select_trace()[2])
    assert sum(opened) * 3 < sum(own), (opened, own)              # (query 0's M-tile lists: ~1/8 expected)
    out_rows, cols, order = shards[0].merge(lay, gathered, batch, k, pool, pool, w)
    torch.cuda.synchronize()
    assert np.array_equal(out_rows.cpu().numpy(), want[0])
    assert np.array_equal(cols.cpu().numpy(), want[1], equal_nan=True)
    assert np.array_equal(order.cpu().numpy(), want[2])
    # a phase 2 without its phase 1 is an error, and a plain search in between voids the parked scan
    shards[0].local_scan(q_dev, pool)
    shards[0].s.dense_pool(q_dev[:3], pool)
    with pytest.raises(Exception):
        shards[0].s.dense_select(q_dev, pool, floor)


def test_pipelined_submit_finish_equals_the_straight_path_bitwise():
    """ShardedSearcher.submit / finish (batch i + 1's K1 enqueued before batch i's merge) on the payload path of
    one GPU: three batches in flight give bit for bit what search_batch_dev gives one at a time -- also with the queries
    read from PINNED host memory by K1's first kernel and the answer written to pinned memory by one copy kernel."""
    n, vocab, batch = 60_000, 3000, 200
    V = synth.unit_rows(n, 384, 71)
    n_rev, stars = synth.metadata(n, 72)
    ip, terms, tf, dl = synth.bm25_forward_csr(n, vocab, 30, 73)
    corpus = BM25Corpus(ip, terms, tf, dl, vocab)
    sh = ShardedSearcher(build(V, n_rev.astype(np.float64), stars, corpus, 0, n), n, 0, 1)
    sh.force_payload = True
    w = FusionWeights(w_dense=0.5, w_bm25=0.5, w_rerank=0.0, w_prior=0.0, w_best=0.0, gate_penalty=1.0)
    df = np.bincount(terms, minlength=vocab)
    Qs = [synth.unit_rows(batch, 384, 80 + i) for i in range(3)]
    tls = [synth.query_terms(batch, vocab, 90 + i, df) for i in range(3)]
    want = [[t.cpu().numpy() for t in sh.search_batch_dev(torch.from_numpy(Q).cuda(), tl, 100, w)] for Q, tl in zip(Qs, tls)]
    pins = [torch.from_numpy(Q).pin_memory() for Q in Qs]
    outs = []
    ticket = sh.submit(pins[0], tls[0], 100, w)
    for i in range(1, 3):
        nxt = sh.submit(pins[i], tls[i], 100, w)
        outs.append(sh.finish(ticket))
        ticket = nxt
    outs.append(sh.finish(ticket))
    for (rows, cols, order), (wr, wc, wo) in zip(outs, want):
        p_rows = torch.empty(rows.shape, dtype=rows.dtype).pin_memory()
        p_final = torch.empty((batch, cols.shape[2]), dtype=cols.dtype).pin_memory()
        sh.s.copy_segments([(p_rows, rows), (p_final, cols[:, 7, :])])
        torch.cuda.synchronize()
        assert np.array_equal(p_rows.numpy(), wr) and np.array_equal(p_final.numpy(), wc[:, 7, :])
        assert np.array_equal(cols.cpu().numpy(), wc, equal_nan=True) and np.array_equal(order.cpu().numpy(), wo)
    with pytest.raises(ValueError):
        sh.s.copy_segments([(torch.empty(4), torch.empty(4, device="cuda"))])      # pageable host memory is refused


@pytest.mark.parametrize("scan_cus", [160, 224])
def test_overlapped_shard_pipeline_equals_the_straight_path_bitwise(scan_cus):
    """ShardedSearcher.enable_overlap: scan(i + 1) on a stream masked to `scan_cus` CUs beside payload(i) and merge(i - 1) on a
    stream masked to the rest, two tickets in flight behind the one being submitted -- every answer bit for bit the straight
    path's; a batch the pipeline does not take (3 queries: K1 cannot be split) goes through in order; more than three
    unfinished tickets are refused."""
    n, vocab = 200_000, 3000
    V = synth.unit_rows(n, 384, 71)
    n_rev, stars = synth.metadata(n, 72)
    ip, terms, tf, dl = synth.bm25_forward_csr(n, vocab, 30, 73)
    corpus = BM25Corpus(ip, terms, tf, dl, vocab)
    sh = ShardedSearcher(build(V, n_rev.astype(np.float64), stars, corpus, 0, n), n, 0, 1)
    sh.force_payload = True
    w = FusionWeights(w_dense=0.5, w_bm25=0.5, w_rerank=0.0, w_prior=0.0, w_best=0.0, gate_penalty=1.0)
    df = np.bincount(terms, minlength=vocab)
    sizes = (256, 200, 256, 3, 37, 256, 128)
    Qs = [synth.unit_rows(b, 384, 80 + i) for i, b in enumerate(sizes)]
    tls = [synth.query_terms(b, vocab, 90 + i, df) for i, b in enumerate(sizes)]
    want = [[t.cpu().numpy() for t in sh.search_batch_dev(torch.from_numpy(Q).cuda(), tl, 100, w)] for Q, tl in zip(Qs, tls)]
    assert not sh.enable_overlap()                        # off unless asked for
    assert sh.enable_overlap(scan_cus) and sh.enable_overlap()
    try:
        pins = [torch.from_numpy(Q).pin_memory() for Q in Qs]
        got, inflight = [], []
        for i in range(len(Qs)):
            inflight.append(sh.submit(pins[i], tls[i], 100, w))
            while len(inflight) > 2:
                got.append([t.cpu().numpy() for t in sh.finish(inflight.pop(0))])
        while inflight:
            got.append([t.cpu().numpy() for t in sh.finish(inflight.pop(0))])
        for i, ((rows, cols, order), (wr, wc, wo)) in enumerate(zip(got, want)):
            assert np.array_equal(rows, wr) and np.array_equal(cols, wc, equal_nan=True) and np.array_equal(order, wo), i
        # search_batch_dev on the overlapped searcher = submit + finish at once
        again = [t.cpu().numpy() for t in sh.search_batch_dev(pins[0], tls[0], 100, w)]
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again, want[0]))
        tickets = [sh.submit(pins[0], tls[0], 100, w) for _ in range(3)]
        with pytest.raises(RuntimeError, match="three batches deep"):
            sh.submit(pins[0], tls[0], 100, w)
        for t in tickets:
            sh.finish(t)
    finally:
        sh.disable_overlap()
    # and off again: the straight path still answers the same
    back = [t.cpu().numpy() for t in sh.search_batch_dev(torch.from_numpy(Qs[1]).cuda(), tls[1], 100, w)]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(back, want[1]))


def test_hot_shard_whose_groups_all_reach_the_floor_selects_on_its_own_threshold():
    """the corpus-wide floor is the MINIMUM of the shards' bounds.  With unequal, clustered shards the emptiest one
    sets it far below a hot shard's own pool-th best row: every selection group of the hot shard reaches it and the list of
    opened groups (4096) overflows.  The hot shard must then search its own threshold (a valid, higher cut: its rows of the
    corpus-wide top-pool are among its own top-pool) instead of flagging every query for the exact fallback; the merged
    answer stays bit for bit the unsharded one."""
    n_hot, n_cold, batch, pool = 2_400_000, 600_000, 16, 150
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    c0 = torch.randn((1, 384), generator=g, device="cuda")
    c0 /= c0.norm()
    mat = torch.empty((n_hot + n_cold, 384), device="cuda")
    for s0 in range(0, n_hot, 600_000):                     # the hot shard: one broad cloud around c0 (scores 0.31 +- 0.035)
        blk = c0 + 1.5 / 384 ** 0.5 * torch.randn((600_000, 384), generator=g, device="cuda")
        mat[s0:s0 + 600_000] = blk / blk.norm(dim=1, keepdim=True)
    cold = torch.randn((n_cold, 384), generator=g, device="cuda")
    mat[n_hot:] = cold / cold.norm(dim=1, keepdim=True)     # the cold shard: nothing near the queries (best rows ~0.25)
    q = c0 + 1.5 / 384 ** 0.5 * torch.randn((batch, 384), generator=g, device="cuda")
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    n = n_hot + n_cold
    ones = np.ones(n)

    def searcher(lo, hi):
        ix = ProductIndex(None, n_rows=hi - lo, dim=384, row_offset=lo, device_ptr=mat[lo:hi].data_ptr(), keepalive=mat)
        ix.set_meta(ones[lo:hi], ones[lo:hi])
        return HybridSearcher(ix, None)

    whole = searcher(0, n)
    want_rows, want_dense = [t.cpu().numpy() for t in whole.dense_pool(q, pool)]
    # (ShardedSearcher cuts the rows evenly; the unequal cut is the point here: the two-phase K1 is driven directly, with
    #  local_scan's kth for two shards)
    shards = [searcher(0, n_hot), searcher(n_hot, n)]
    kth = max((pool + 1) // 2, (pool + 7) // 8 + 1)
    bounds = [sh.dense_scan(q, pool, kth) for sh in shards]
    assert all(b is not None for b in bounds)
    floor = torch.stack(bounds).min(dim=0).values
    # the cold shard sets the floor, far below the hot shard's own bound
    assert (bounds[1] < bounds[0] - 0.1).all() and torch.equal(floor, bounds[1])
    # ... so far that most ROWS of the hot shard reach it: all of its ~4 900 selection groups (2.4M rows = 37 500 tiles in
    # 256 runs of groups of 8 tiles) would be listed -- more than the 4 096 the list holds
    assert int((mat[:n_hot] @ q[0] >= floor[0]).sum()) > n_hot // 2
    got_rows, got_dense = [], []
    for sh in shards:
        rows, dense = sh.dense_select(q, pool, floor)
        torch.cuda.synchronize()
        tr = sh.index.select_trace()
        assert tr[0] == 2, "the two-pass path served query 0 (no exact fallback)"
        assert tr[1] <= 4096
        got_rows.append(rows.cpu().numpy())
        got_dense.append(dense.cpu().numpy())
    for b in range(batch):                                  # the merge K3 does: (dense desc, row asc), first `pool`
        r = np.concatenate([got_rows[0][b], got_rows[1][b]])
        d = np.concatenate([got_dense[0][b], got_dense[1][b]])
        keep = np.lexsort((r, -d.astype(np.float64)))[:pool]
        assert np.array_equal(r[keep], want_rows[b]) and np.array_equal(d[keep], want_dense[b]), b
