"""The attribute gate BEFORE the shard merge (sharded.py), on one GPU: every shard matches its own
candidates against the gate plane of its own rows, the factor travels in the payload, K3 (rr_fuse_topk_cand_dev) reads it
through the merge.  The merged answer must equal the unsharded `HybridSearcher.search_batch(gate_groups=...)` over a
whole-corpus plane bit for bit, and the `_gate` column must be `text.calculate_gate_factor` of every pool row."""
import ctypes as C

import numpy as np
import pytest
import torch

from review_recommender_amd import _lib, synth
from review_recommender_amd import text as T
from review_recommender_amd.bm25 import BM25Corpus
from review_recommender_amd.engine import FusionWeights, HybridSearcher
from review_recommender_amd.gate import GateText, pack_groups
from review_recommender_amd.index import ProductIndex
from review_recommender_amd.sharded import PayloadLayout, ShardedSearcher, shard_bounds

pytestmark = pytest.mark.gpu

N, VOCAB, K, POOL = 40_000, 3000, 100, 150
PENALTY = 0.5
W = FusionWeights(w_dense=0.5, w_bm25=0.3, w_rerank=0.0, w_prior=0.2, w_best=0.0, gate_penalty=PENALTY)
WORLDS = (2, 3, 8)
TERMS = sorted({t for grp in list(T.SYNONYMS.values()) + list(T.COLORS.values()) for t in grp} - {"wireless", "bluetooth"})
FILLER = ["lorem", "ipsum", "item", "great", "value", "pack", "size", "soft", "daily", "use", "gift", "home", "set", "new"]


def make_texts(n, seed, distinct=2000):
    """n texts of a few hundred bytes: `distinct` different ones, repeated (words of the gate's groups among filler)."""
    rng = np.random.default_rng(seed)
    words = np.array(TERMS + ["wireless", "bluetooth"] + FILLER * 8)
    base = [" ".join(words[rng.integers(0, len(words), rng.integers(20, 60))]) for _ in range(distinct)]
    pick = rng.integers(0, distinct, n)
    return [base[i] for i in pick]


def boundary_rows(n):
    return sorted({shard_bounds(n, w, r)[0] for w in WORLDS for r in range(1, w)})


def host_factors(texts, groups, rows):
    return np.array([np.float32(T.calculate_gate_factor(texts[int(i)][:6000], groups, PENALTY)[0]) for i in rows], dtype=np.float32)


GROUPS = [
    T.build_gate_groups("wireless yellow cat socks"),                                   # 5 groups; query 0 looks at the planted rows
    [],                                                                                 # no group: factor 1, no text read
    T.build_gate_groups("red blue wireless keyboard dog design pattern"),               # 6 groups
    [{"café", "sock"}, {"kitten"}],                                                # a term outside ASCII: the host gates it
    T.build_gate_groups("noise cancelling headphones in black"),
]


assert [len(g) for g in GROUPS[:3]] == [5, 0, T.MAX_GATE_GROUPS]


def groups_for(batch):
    rng = np.random.default_rng(batch)
    pool = list(T.SYNONYMS.values()) + list(T.COLORS.values())
    out = [GROUPS[i] if i < len(GROUPS) else [pool[j] for j in rng.permutation(len(pool))[:rng.integers(1, 5)]] for i in range(batch)]
    return out


@pytest.fixture(scope="module")
def world():
    """The corpus of test_sharded_equals_unsharded_bitwise with texts, the planted documents near query 0, the whole-corpus
    searcher with its plane, and a cache of the shards per world size."""
    V = synth.unit_rows(N, 384, 61)
    V[1000] = V[39_000]
    texts = make_texts(N, 5)
    planted = {7: "lorem " * 1100 + "wireless yellow cat socks",                       # > 6000 code points: the only hits are cut
               1000: "WIRELESS Yellow CAT SOCKS",                                      # upper case
               39_000: "socK Kitten wirelessİ İyellow",              # U+212A -> k (sock, kitten), U+0130 beside terms
               11: "",                                                                 # an empty text
               12: "yellİow kİtty bluetoKth"}                             # U+0130 -> i + U+0307: no hit
    for lo in boundary_rows(N):                # `...wire` | `less...`: a match must not run into the neighbouring document
        planted[lo - 1] = "yellow gift item wire"
        planted[lo] = "less value cat pack"
    rng = np.random.default_rng(9)
    for r, t in planted.items():
        texts[r] = t
        if r not in (1000, 39_000):            # every planted row into query 0's pool
            v = V[1000] + 0.3 / np.sqrt(384) * rng.standard_normal(384).astype(np.float32)
            V[r] = v / np.linalg.norm(v)
    n_rev, stars = synth.metadata(N, 62, nan_fraction=0.01)
    ip, terms, tf, dl = synth.bm25_forward_csr(N, VOCAB, 30, 63)
    corpus = BM25Corpus(ip, terms, tf, dl, VOCAB)
    w = dict(V=V, texts=texts, planted=planted, n_rev=n_rev.astype(np.float64), stars=stars, corpus=corpus,
             df=np.bincount(terms, minlength=VOCAB), shards={})

    def build(lo, hi, gate=True):
        ix = ProductIndex(V[lo:hi], row_offset=lo)
        ix.set_meta(w["n_rev"][lo:hi], stars[lo:hi])
        gt = GateText.from_texts(texts[lo:hi], 0, row_offset=lo) if gate else None
        return HybridSearcher(ix, corpus.slice(lo, hi).to_device(row_offset=lo), gate_text=gt)

    w["build"] = build
    w["whole"] = build(0, N)
    return w


def shards_of(w, size):
    if size not in w["shards"]:
        w["shards"][size] = [ShardedSearcher(w["build"](*shard_bounds(N, size, r)), N, r, size) for r in range(size)]
    return w["shards"][size]


def batch_of(w, batch):
    Q = synth.unit_rows(batch, 384, 64)
    Q[0] = w["V"][1000]
    return Q, synth.query_terms(batch, VOCAB, 65, w["df"]), groups_for(batch)


def merge(shards, lay, bufs, weights, k, batch, pool):
    """The gathered payloads as the all-gather leaves them, and K3 with the gate column: (rows, cols, order) numpy."""
    size = len(shards)
    gathered = torch.empty((size, lay.nbytes), dtype=torch.uint8, device="cuda")
    for r, buf in enumerate(bufs):
        gathered[r].copy_(buf)
    assert lay.gate
    out_rows, cols, order = shards[0].merge(lay, gathered, batch, k, pool, pool, weights)
    torch.cuda.synchronize()
    return out_rows.cpu().numpy(), cols.cpu().numpy(), order.cpu().numpy()


@pytest.mark.parametrize("size", WORLDS)
@pytest.mark.parametrize("batch", [1, 5, 20])
def test_gate_before_the_merge_equals_the_unsharded_device_gate_bitwise(world, size, batch):
    w = world
    texts = w["texts"]
    Q, tl, groups = batch_of(w, batch)
    ref = w["whole"].search_batch(Q, tl, K, weights=W, gate_groups=groups,
                                  gate_host=lambda b, rows: host_factors(texts, groups[b], rows))
    plain = w["whole"].search_batch(Q, tl, K, weights=W)
    assert ref.pool == POOL and not np.array_equal(ref.columns[:, 7], plain.columns[:, 7]), "the gate changes _final"
    assert not np.array_equal(ref.order, plain.order), "... and the order"
    for b in range(batch):                      # the unsharded reference itself is the host function's, row by row
        assert np.array_equal(ref.columns[b, 5], host_factors(texts, groups[b], ref.pool_rows[b]).astype(np.float64)), b
    if batch >= 5:
        row0 = ref.pool_rows[0].tolist()
        assert all(r in row0 for r in w["planted"]), "every planted document is a candidate of query 0"

    shards = shards_of(w, size)
    packed = pack_groups(groups, PENALTY)
    assert packed.host_queries == ([3] if batch > 3 else [])
    q_dev = torch.from_numpy(Q).cuda()
    seen, bufs, lay = [], [], None
    for r, sh in enumerate(shards):
        def gate_host(b, rows, r=r):
            seen.append((r, b, rows.copy()))
            return host_factors(texts, groups[b], rows)
        lay, buf = sh.local_payload(q_dev, tl, POOL, gate=packed, gate_host=gate_host)
        assert lay == PayloadLayout(batch, POOL, gate=True) and buf.numel() == lay.nbytes
        bufs.append(buf)
    rows, cols, order = merge(shards, lay, bufs, W, K, batch, POOL)
    for sh in shards:
        sh.s.gate_text.check()                  # no candidate row outside its shard's plane
    assert np.array_equal(rows, ref.pool_rows)
    assert np.array_equal(cols, ref.columns, equal_nan=True)
    assert np.array_equal(order, ref.order)
    for b in range(batch):
        assert np.array_equal(cols[b, 5], host_factors(texts, groups[b], rows[b]).astype(np.float64)), b
    if batch > 3:
        assert sorted(r for r, _, _ in seen) == list(range(size)) and all(b == 3 for _, b, _ in seen)
        for r, _, got in seen:                  # the over-limit query is gated on the rank's own rows only
            lo, hi = shard_bounds(N, size, r)
            assert got.shape == (POOL,) and got.min() >= lo and got.max() < hi, (r, lo, hi)
    else:
        assert not seen


@pytest.fixture(scope="module")
def floor_world():
    """A corpus large enough for the two-phase K1 at pool 37 (a shard needs 64 x 8 x pool rows), with texts."""
    n = 160_000
    V = synth.unit_rows(n, 384, 71)
    n_rev, stars = synth.metadata(n, 72, nan_fraction=0.0)
    ip, terms, tf, dl = synth.bm25_forward_csr(n, VOCAB, 10, 73)
    texts = make_texts(n, 6)
    return dict(n=n, V=V, n_rev=n_rev.astype(np.float64), stars=stars, corpus=BM25Corpus(ip, terms, tf, dl, VOCAB), texts=texts,
                df=np.bincount(terms, minlength=VOCAB), planes={})


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_eight_shards_under_a_corpus_wide_floor_gate_their_own_rows(floor_world, dtype):
    """The form of test_shards_select_against_a_corpus_wide_floor: with the floor a shard's list is filled up with other
    rescored rows (scores below the cut, -inf among them).  Those fill entries are rows of the shard too: the gate reads
    them from the shard's own plane, rr_gate_status stays clean, and the merged answer is the unsharded one bit for bit."""
    f = floor_world
    n, size, batch, k, pool = f["n"], 8, 8, 20, 37
    texts = f["texts"]

    def plane(lo, hi):
        if (lo, hi) not in f["planes"]:
            f["planes"][(lo, hi)] = GateText.from_texts(texts[lo:hi], 0, row_offset=lo)
        return f["planes"][(lo, hi)]

    def build_t(lo, hi):
        ix = ProductIndex.from_rows(f["V"][lo:hi], row_offset=lo, dtype=dtype)
        ix.set_meta(f["n_rev"][lo:hi], f["stars"][lo:hi])
        return HybridSearcher(ix, f["corpus"].slice(lo, hi).to_device(row_offset=lo), gate_text=plane(lo, hi))

    Q = synth.unit_rows(batch, 384, 74)
    tl = synth.query_terms(batch, VOCAB, 75, f["df"])
    groups = groups_for(batch)
    groups[3] = groups[4]                       # (every query on the kernel here)
    ref = build_t(0, n).search_batch(Q, tl, k, weights=W, pool_floor=pool, gate_groups=groups)
    assert ref.pool == pool
    shards = [ShardedSearcher(build_t(*shard_bounds(n, size, r)), n, r, size) for r in range(size)]
    q_dev = torch.from_numpy(Q).cuda()
    bounds = [sh.local_scan(q_dev, pool) for sh in shards]
    assert all(b is not None for b in bounds), "an 8-query batch on a 20 000-row shard takes the filter path at pool 37"
    floor = torch.stack(bounds).min(dim=0).values
    assert torch.isfinite(floor).all()
    packed = pack_groups(groups, PENALTY)
    bufs, lay, filled = [], None, 0
    for sh in shards:
        lay, buf = sh.local_payload(q_dev, tl, pool, floor=floor, gate=packed)
        torch.cuda.synchronize()
        v = lay.views(buf)
        lo, hi = sh.s.index.row_offset, sh.s.index.row_offset + sh.s.index.n_rows
        rows_h, dense_h = v["rows"].cpu().numpy(), v["dense"].cpu().numpy()
        assert rows_h.min() >= lo and rows_h.max() < hi, "K1's fill entries are rows of the shard"
        filled += int((dense_h < floor.cpu().numpy()[:, None]).sum())
        bufs.append(buf)
        sh.s.gate_text.check()
    assert filled > 0, "some lists were filled up with rows below the floor"
    rows, cols, order = merge(shards, lay, bufs, W, k, batch, pool)
    assert np.array_equal(rows, ref.pool_rows)
    assert np.array_equal(cols, ref.columns, equal_nan=True)
    assert np.array_equal(order, ref.order)
    for b in range(batch):
        assert np.array_equal(cols[b, 5], host_factors(texts, groups[b], rows[b]).astype(np.float64)), b


def pipeline_batches(w):
    sizes = (20, 8, 20)
    Qs = [synth.unit_rows(b, 384, 80 + i) for i, b in enumerate(sizes)]
    tls = [synth.query_terms(b, VOCAB, 90 + i, w["df"]) for i, b in enumerate(sizes)]
    gs = [groups_for(b) for b in sizes]
    return Qs, tls, gs


def test_submit_finish_with_gate_groups_three_batches_in_flight(world):
    w, texts = world, world["texts"]
    sh = ShardedSearcher(w["whole"], N, 0, 1)
    sh.force_payload = True
    Qs, tls, gs = pipeline_batches(w)
    host = lambda g: (lambda b, rows: host_factors(texts, g[b], rows))
    want = [[t.cpu().numpy() for t in sh.search_batch_dev(torch.from_numpy(Q).cuda(), tl, 20, W, pool_floor=37, gate_groups=g,
                                                          gate_host=host(g))] for Q, tl, g in zip(Qs, tls, gs)]
    for (Q, tl, g), (wr, wc, wo) in zip(zip(Qs, tls, gs), want):       # the payload path = the unsharded answer
        ref = w["whole"].search_batch(Q, tl, 20, weights=W, pool_floor=37, gate_groups=g, gate_host=host(g))
        assert np.array_equal(wr, ref.pool_rows) and np.array_equal(wc, ref.columns, equal_nan=True) and np.array_equal(wo, ref.order)
        assert (wc[:, 5] != 1.0).any()
    pins = [torch.from_numpy(Q).pin_memory() for Q in Qs]
    tickets = [sh.submit(pins[i], tls[i], 20, W, pool_floor=37, gate_groups=gs[i], gate_host=host(gs[i])) for i in range(3)]
    assert all(t.lay.gate and t.packed is not None for t in tickets)
    for t, (wr, wc, wo) in zip(tickets, want):
        rows, cols, order = [x.cpu().numpy() for x in sh.finish(t)]
        assert np.array_equal(rows, wr) and np.array_equal(cols, wc, equal_nan=True) and np.array_equal(order, wo)
    # one rank without the payload path: K1 -> K2 -> gate -> K3 straight through, a pool-aligned gate and one pass
    sh.force_payload = False
    for (Q, tl, g), (wr, wc, wo) in zip(zip(Qs, tls, gs), want):
        rows, cols, order = [x.cpu().numpy() for x in sh.search_batch_dev(torch.from_numpy(Q).cuda(), tl, 20, W, pool_floor=37,
                                                                           gate_groups=g, gate_host=host(g))]
        assert np.array_equal(rows, wr) and np.array_equal(cols, wc, equal_nan=True) and np.array_equal(order, wo)
    w["whole"].gate_text.check()


@pytest.mark.parametrize("scan_cus", [160, 224])
def test_overlapped_pipeline_takes_gated_batches(world, scan_cus):
    w, texts = world, world["texts"]
    sh = ShardedSearcher(w["whole"], N, 0, 1)
    sh.force_payload = True
    Qs, tls, gs = pipeline_batches(w)
    host = lambda g: (lambda b, rows: host_factors(texts, g[b], rows))
    kw = lambda i: dict(pool_floor=37, gate_groups=gs[i], gate_host=host(gs[i]))
    want = [[t.cpu().numpy() for t in sh.search_batch_dev(torch.from_numpy(Qs[i]).cuda(), tls[i], 20, W, **kw(i))] for i in range(3)]
    plain = [t.cpu().numpy() for t in sh.search_batch_dev(torch.from_numpy(Qs[0]).cuda(), tls[0], 20, W, pool_floor=37)]
    assert sh.enable_overlap(scan_cus)
    try:
        pins = [torch.from_numpy(Q).pin_memory() for Q in Qs]
        order_of = (0, 1, 2, 0, 2)
        tickets, got = [], []
        for i in order_of:
            tickets.append(sh.submit(pins[i], tls[i], 20, W, **kw(i)))
            assert tickets[-1].slot >= 0 and tickets[-1].lay.gate, "a gated batch stays in the pipeline"
            while len(tickets) > 2:
                got.append([t.cpu().numpy() for t in sh.finish(tickets.pop(0))])
        # an ungated batch between gated ones has the other layout, hence ring buffers of its own
        tickets.append(sh.submit(pins[0], tls[0], 20, W, pool_floor=37))
        assert tickets[-1].slot >= 0 and not tickets[-1].lay.gate
        while tickets:
            got.append([t.cpu().numpy() for t in sh.finish(tickets.pop(0))])
        for i, res in zip(order_of, got):
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(res, want[i])), i
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[-1], plain))
        # a host gate still leaves the pipeline
        t = sh.submit(pins[1], tls[1], 20, W, pool_floor=37, gate_fn=lambda rows: np.ones(rows.shape, np.float32))
        assert t.slot < 0
        sh.finish(t)
    finally:
        sh.disable_overlap()
    w["whole"].gate_text.check()


def test_gate_groups_with_a_host_reranker_equal_the_host_gate_bitwise(world):
    """gate_groups + rerank_fn: two passes (the merge, then K3 with the rerank column and the payload's gate column), bit for
    bit what gate_fn + rerank_fn gave for the same factors."""
    w, texts = world, world["texts"]
    batch, k, rr_k = 5, 10, 20
    Q, tl, groups = batch_of(w, batch)
    wts = FusionWeights(w_dense=0.4, w_bm25=0.2, w_rerank=0.3, w_prior=0.1, w_best=0.0, gate_penalty=PENALTY)
    gate_fn = lambda rows: np.stack([host_factors(texts, groups[b], rows[b]) for b in range(rows.shape[0])])
    rerank_fn = lambda qi, rows: (np.sin(rows * 0.001) + qi * 0.1).astype(np.float32)
    host = lambda b, rows: host_factors(texts, groups[b], rows)
    sh = ShardedSearcher(w["whole"], N, 0, 1)
    sh.force_payload = True
    q_dev = torch.from_numpy(Q).cuda()
    a = [t.cpu().numpy() for t in sh.search_batch_dev(q_dev, tl, k, wts, pool_floor=37, rerank_k=rr_k, gate_fn=gate_fn,
                                                      rerank_fn=rerank_fn)]
    b = [t.cpu().numpy() for t in sh.search_batch_dev(q_dev, tl, k, wts, pool_floor=37, rerank_k=rr_k, gate_groups=groups,
                                                      gate_host=host, rerank_fn=rerank_fn)]
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    assert (a[1][:, 5] != 1.0).any() and (a[1][:, 3] != 0.0).any()
    sh.force_payload = False                    # and straight through
    c = [t.cpu().numpy() for t in sh.search_batch_dev(q_dev, tl, k, wts, pool_floor=37, rerank_k=rr_k, gate_groups=groups,
                                                      gate_host=host, rerank_fn=rerank_fn)]
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, c))


def test_gate_argument_errors_are_raised_before_anything_runs(world):
    w = world
    Q, tl, groups = batch_of(w, 5)
    q_dev = torch.from_numpy(Q).cuda()
    host = lambda b, rows: np.ones(len(rows), np.float32)
    sh = ShardedSearcher(w["whole"], N, 0, 1)
    bare = ShardedSearcher(w["build"](0, N, gate=False), N, 0, 1)

    def launches(s):
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(s.s.lib.rr_index_scan_stats(s.s.index.handle, C.byref(ms), C.byref(cnt)), "rr_index_scan_stats")
        return cnt.value

    launches(sh), launches(bare)
    for force in (False, True):
        sh.force_payload = bare.force_payload = force
        with pytest.raises(ValueError, match="either gate_fn or gate_groups"):
            sh.search_batch_dev(q_dev, tl, K, W, gate_fn=lambda rows: np.ones(rows.shape, np.float32), gate_groups=groups,
                                gate_host=host)
        with pytest.raises(ValueError, match="gate plane"):
            bare.search_batch_dev(q_dev, tl, K, W, gate_groups=groups, gate_host=host)
        with pytest.raises(ValueError, match="gate plane"):
            bare.submit(q_dev, tl, K, W, gate_groups=groups, gate_host=host)
        with pytest.raises(ValueError, match="no gate_host"):
            sh.search_batch_dev(q_dev, tl, K, W, gate_groups=groups)
    torch.cuda.synchronize()
    assert launches(sh) == 0 and launches(bare) == 0
