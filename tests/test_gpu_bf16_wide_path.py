"""bf16 storage at embedding widths other than 384 (csrc/rr_dense_bf16w.hip, csrc/rr_dense_fltw.hip), through ProductIndex.

The oracle is the one of tests/test_gpu_bf16.py: the reference's fp32 matvec + argpartition, and the float64 yardstick, over
the matrix rounded once to bf16 and widened back (oracle.dense.round_to_bf16).  Every batch of two or more must be served by
rr_scan_fltw on the index's own rows (last_scan_info family 5, variant 16, 2 bytes per element; select_trace word 0 = 2), a
single query by rr_scan_bf16_generic (family 2); every query of a batch gets the answer it gets alone -- rows and score BITS
-- and the single-query scores are bit for bit the CPU model of the chain (fltw_bf16_model.chain_wb) on the returned rows.

Seeds.  The documented rule (tau~ = pool-th largest group maximum of the bf16 products s~; candidate rows s~ >= tau~ - 2.05 eps;
caps 4096 rows and 16384 M-tiles) replayed in numpy on the ROUNDED rows (row delta 0 in eps) for every (dim, n_rows) below and
all 256 queries, one 64-row tile per group, gives at most
    dim 64: 31 rows / 31 M-tiles    dim 100: 30 / 30    dim 192: 32 / 32    dim 320: 34 / 33    dim 768: 40 / 40
    dim 1000: 43 / 42               dim 1024: 43 / 43   (dim 350, 40 queries: 37 / 37)
candidates for the worst query: about 100x under the caps, so no query is flagged by the data.  In the equal-rows batches the
same replay gives 6000 candidate rows for exactly the queries placed next to the block and at most 39 for any other.

Run on the parent commit every test of this file fails at its first line that builds an index: rr_index_create refuses
"bf16 storage is built for dim 384 only" (dim 350 included: the check tested dim, not dim_pad).
"""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import fltw_bf16_model as WB
from oracle import dense as OD
from parity import assert_topk_matches, min_gap
from review_recommender_amd import synth
from review_recommender_amd.index import ProductIndex

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)
POOL = 20
BATCHES = (1, 2, 9, 33, 64, 65, 130, 256)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _padded(a):
    n, dim = a.shape
    out = np.zeros((n, (dim + 63) // 64 * 64), dtype=np.float32)
    out[:, :dim] = a
    return out


class _Oracle:
    """The float64 yardstick and the reference-order oracle of every query over the rounded rows, computed once per index."""

    def __init__(self, Vb, Q, pool):
        self.pool = pool
        self.ref64 = Vb.astype(np.float64) @ Q.astype(np.float64).T
        self.ref = [OD.cosine_similarity_search(q, Vb, pool) for q in Q]
        self.gap = [min_gap(self.ref64[:, i], pool) for i in range(len(Q))]

    def check(self, rows, scores, first=0):
        pool = self.pool
        assert rows.shape[1:] == (pool,) and rows.dtype == np.int64 and scores.dtype == np.float32
        for i in range(len(rows)):
            assert_topk_matches(rows[i], scores[i], self.ref64[:, first + i], pool)
            o_rows, o_sims = self.ref[first + i]
            if self.gap[first + i] > 4e-7:
                assert np.array_equal(rows[i], o_rows), "IDs must be bit-exact"
            np.testing.assert_allclose(scores[i], o_sims[:pool], atol=1e-5, rtol=0)


@pytest.mark.parametrize("n_rows", [12000, 12005])
@pytest.mark.parametrize("dim", [64, 100, 192, 320, 768, 1000, 1024])
def test_batches_take_the_wide_filter_path_and_keep_the_single_query_answer(dim, n_rows):
    V = synth.unit_rows(n_rows, dim, 1000 + dim)
    Vb = OD.round_to_bf16(V)
    Q = synth.unit_rows(256, dim, 2000 + dim)
    Vp, Qp = _padded(Vb), _padded(Q)
    ix = ProductIndex.from_rows(V, dtype="bf16")
    oracle = _Oracle(Vb, Q, POOL)
    try:
        assert ix.dim_padded == Vp.shape[1]
        for b in BATCHES:
            rows, scores = ix.dense_topk(Q[:b], POOL)
            info, trace = ix.last_scan_info(), ix.select_trace()
            if b >= 2:
                assert info[:2] == (5, 16) and info[4] == 2, (b, info)   # rr_scan_fltw over the 2-byte rows themselves
                assert trace[0] == 2, (b, trace[:4])
            else:
                assert info[0] == 2, (b, info)                           # rr_scan_bf16_generic
            assert len(rows) == b
            oracle.check(rows, scores)
            for i in sorted({b - 1, b // 2}):
                r1, s1 = ix.dense_topk(Q[i:i + 1], POOL)
                assert ix.last_scan_info()[0] == 2
                assert np.array_equal(rows[i], r1[0]), (b, i)
                assert np.array_equal(_bits(scores[i]), _bits(s1[0])), (b, i)
                assert np.array_equal(_bits(s1[0]), _bits(WB.chain_wb(Vp[r1[0]], Qp[i]))), (b, i)
    finally:
        ix.close()


def test_dim_350_pads_to_384_and_is_served_by_the_384_kernels():
    dim, n = 350, 12000
    V = synth.unit_rows(n, dim, 1350)
    Vb = OD.round_to_bf16(V)
    Q = synth.unit_rows(40, dim, 2350)
    ix = ProductIndex.from_rows(V, dtype="bf16")
    oracle = _Oracle(Vb, Q, POOL)
    try:
        assert ix.dim_padded == 384
        for b in (1, 8, 40):
            rows, scores = ix.dense_topk(Q[:b], POOL)
            info = ix.last_scan_info()
            assert info[0] == (2 if b == 1 else 5) and info[1] != 16, (b, info)
            oracle.check(rows, scores)
            for i in sorted({b - 1, b // 2}):
                r1, s1 = ix.dense_topk(Q[i:i + 1], POOL)
                assert np.array_equal(rows[i], r1[0]) and np.array_equal(_bits(scores[i]), _bits(s1[0])), (b, i)
    finally:
        ix.close()


def test_all_rows_equal_every_query_is_flagged_and_served_by_the_listed_passes():
    """12 000 copies of one row, 40 queries: every candidate list overflows, five listed passes of eight serve the batch.  The
    answer is rows 0..19 (equal scores order by row) and bit for bit the single-query answer."""
    dim = 768
    v = synth.unit_rows(1, dim, 5)
    V = np.repeat(v, 12000, axis=0)
    Q = synth.unit_rows(40, dim, 6)
    ix = ProductIndex.from_rows(V, dtype="bf16")
    try:
        rows, scores = ix.dense_topk(Q, POOL)
        assert ix.last_scan_info()[:2] == (5, 16)
        vb = OD.round_to_bf16(v)
        for i in range(40):
            assert rows[i].tolist() == list(range(POOL)), (i, rows[i])
            r1, s1 = ix.dense_topk(Q[i:i + 1], POOL)
            assert np.array_equal(rows[i], r1[0]) and np.array_equal(_bits(scores[i]), _bits(s1[0])), i
            assert np.all(_bits(s1[0]) == _bits(WB.chain_wb(vb, Q[i]))[0]), i
    finally:
        ix.close()


def _child(code: str, timeout: int = 300, env=None, args=()):
    p = subprocess.run([sys.executable, "-c", code.replace("@ROOT@", repr(ROOT)), *args], capture_output=True, text=True,
                       timeout=timeout, env=env)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


NEAR = r"""
import os, sys
os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, @ROOT@)
import ctypes as C
import numpy as np
from review_recommender_amd import _lib, synth
from review_recommender_amd.index import ProductIndex
lib = _lib.load()
dim, pool = 768, 20
V = synth.unit_rows(12000, dim, 11)
v = V[0].copy()
V[:6000] = v                                      # rows 0 .. 5999: copies of one unit vector
ix = ProductIndex.from_rows(V, dtype="bf16")
def near(seed):                                   # a unit query within 1e-3 of v
    d = synth.unit_rows(1, dim, seed)[0]
    q = v + np.float32(5e-4) * d
    q = (q / np.linalg.norm(q)).astype(np.float32)
    assert np.linalg.norm(q - v) < 1e-3
    return q
for tag, where in (("three", (3, 17, 39)), ("twelve", (0, 1, 2, 5, 8, 13, 20, 21, 22, 30, 38, 39))):
    Q = synth.unit_rows(40, dim, 12 + len(where))
    for k, i in enumerate(where):
        Q[i] = near(100 + k)
    rows, scores = ix.dense_topk(Q, pool)
    info = ix.last_scan_info()
    tr = (C.c_int32 * (16 * 40))()
    _lib.check(lib.rr_debug_select_traces(ix.handle, 40, tr), "rr_debug_select_traces")
    flagged = [q for q in range(40) if tr[16 * q] != 2]
    same = True
    for i in range(40):
        r1, s1 = ix.dense_topk(Q[i:i + 1], pool)
        same = same and np.array_equal(rows[i], r1[0]) and np.array_equal(scores[i].view(np.uint32), s1[0].view(np.uint32))
    top = all(rows[i].tolist() == list(range(pool)) for i in where)
    print(f"NEAR|{tag}|info={info[0]},{info[1]}|flagged={flagged}|want={list(where)}|bitwise={same}|rows0to19={top}", flush=True)
"""


def test_a_block_of_equal_rows_flags_exactly_the_queries_next_to_it():
    """The 6 000-equal-rows block of tests/test_gpu_fltw_path.py in a bf16 index, with 3 queries next to it (one listed pass)
    and with 12 (two passes).  Per-query path traces (rr_debug_select_traces, harness library): exactly those queries left the
    filter tail; all 40 answers are bit for bit the single-query answers."""
    from review_recommender_amd.build import DEBUG_LIB_PATH
    assert DEBUG_LIB_PATH.exists(), "librr_hip_dbg.so is built by build()"
    out = _child(NEAR)
    lines = [l.split("|") for l in out.splitlines() if l.startswith("NEAR|")]
    assert len(lines) == 2, out[-2000:]
    for l in lines:
        assert l[2] == "info=5,16", l
        assert l[3].split("=")[1] == l[4].split("=")[1], l
        assert l[5] == "bitwise=True" and l[6] == "rows0to19=True", l


def test_an_inf_element_sends_the_batch_to_the_valu_scans_and_a_nan_score_ranks_last():
    """Row 5 holds +inf in column 3, row 7 a NaN: no finite row-norm bound, the batched path declines (RR_FLT_NO_BOUND) and the
    batch is served by rr_scan_bf16_generic eight queries per pass (family 2, variant 8).  Every answer is bitwise the
    single-query answer.  Queries 0 .. 9 are 0 in column 3: inf x 0 = NaN, the row's score is NaN and ranks last (it is not
    among the top 20, whose scores are all finite); the other queries see +inf (first) or -inf there.  Row 7 never shows."""
    dim, n = 768, 12000
    V = synth.unit_rows(n, dim, 71)
    V[5, 3] = np.inf
    V[7, 2] = np.nan
    Q = synth.unit_rows(40, dim, 72)
    Q[:10, 3] = 0.0
    ix = ProductIndex.from_rows(V, dtype="bf16")
    try:
        rows, scores = ix.dense_topk(Q, POOL)
        assert ix.last_scan_info()[:2] == (2, 8), ix.last_scan_info()
        assert not np.isnan(scores).any() and not (rows == 7).any()
        for i in range(40):
            r1, s1 = ix.dense_topk(Q[i:i + 1], POOL)
            assert np.array_equal(rows[i], r1[0]) and np.array_equal(_bits(scores[i]), _bits(s1[0])), i
            if i < 10:
                assert 5 not in rows[i] and np.isfinite(scores[i]).all(), i
            elif Q[i, 3] > 0:
                assert rows[i, 0] == 5 and scores[i, 0] == np.inf, i
            else:
                assert 5 not in rows[i], i
    finally:
        ix.close()


SWITCH = r"""
import sys
sys.path.insert(0, @ROOT@)
import numpy as np
from review_recommender_amd import synth
from review_recommender_amd.index import ProductIndex
V = synth.unit_rows(12000, 768, 1768)
Q = synth.unit_rows(64, 768, 2768)
ix = ProductIndex.from_rows(V, dtype="bf16")
rows, scores = ix.dense_topk(Q, 20)
print("FAMILY|%d" % ix.last_scan_info()[0], flush=True)
np.savez(sys.argv[1], rows=rows, scores=scores)
"""


def test_the_switch_restores_the_valu_route_with_the_same_bits(tmp_path):
    """RR_NO_WIDE_FLT=1 (read once per process: a child): family 2, the bf16 VALU scans, and for one batch of 64 at 768 the rows
    and score bits of the default route."""
    V = synth.unit_rows(12000, 768, 1768)
    Q = synth.unit_rows(64, 768, 2768)
    ix = ProductIndex.from_rows(V, dtype="bf16")
    rows, scores = ix.dense_topk(Q, POOL)
    assert ix.last_scan_info()[:2] == (5, 16)
    ix.close()
    out_file = str(tmp_path / "valu.npz")
    out = _child(SWITCH, env=dict(os.environ, RR_NO_WIDE_FLT="1"), args=(out_file,))
    assert "FAMILY|2" in out, out
    got = np.load(out_file)
    assert np.array_equal(got["rows"], rows)
    assert np.array_equal(_bits(got["scores"]), _bits(scores))


def test_the_row_norm_bound_follows_rows_uploaded_after_a_batched_search(hip):
    """tests/test_gpu_bf16.py's test of the cached bound, at 768: small rows, one batched search caches their bound, larger rows
    are uploaded over them, and the batch must still equal the single-query scan."""
    from review_recommender_amd import _lib
    n, dim = 12000, 768
    small = (synth.unit_rows(n, dim, 41) * 0.05).astype(np.float32)
    big = (synth.unit_rows(n, dim, 42) * 3.0).astype(np.float32)
    Q = synth.unit_rows(40, dim, 43)
    ix = ProductIndex.from_rows(small, dtype="bf16")
    try:
        ix.dense_topk(Q, POOL)
        assert ix.last_scan_info()[:2] == (5, 16)
        _lib.check(hip.rr_index_upload_rows_f32(ix.handle, 0, n, _lib.ptr(big), 0.0), "upload")
        rows_b, scores_b = ix.dense_topk(Q, POOL)
        assert ix.last_scan_info()[:2] == (5, 16)
        ref64 = OD.round_to_bf16(big).astype(np.float64) @ Q.astype(np.float64).T
        for i in range(0, 40, 7):
            r1, s1 = ix.dense_topk(Q[i:i + 1], POOL)
            assert np.array_equal(rows_b[i], r1[0]) and np.array_equal(_bits(scores_b[i]), _bits(s1[0])), i
            assert_topk_matches(rows_b[i], scores_b[i], ref64[:, i], POOL, score_tol=3e-5)
    finally:
        ix.close()


def test_rows_enter_through_every_door_with_the_same_bits():
    """dim 100 (pads to 128): the host upload, the device store (contiguous, and scattered by row ids) and an adopted matrix of
    n x 128 bf16 hold the same rows, so one batch gives the same rows and score bits through all four.  Then the adopted
    matrix is overwritten with rows 60 times larger behind the index's back: after matrix_changed() the batch still equals the
    single-query scan (the cached bound was reset)."""
    import torch
    n, dim = 12000, 100
    V = synth.unit_rows(n, dim, 81)
    Q = synth.unit_rows(33, dim, 82)
    dev = torch.device("cuda", 0)
    Vd = torch.from_numpy(V).to(dev)
    a = ProductIndex.from_rows(V, dtype="bf16")
    want = a.dense_topk(Q, POOL)
    assert a.last_scan_info()[:2] == (5, 16)
    a.close()

    def same(ix):
        got = ix.dense_topk(Q, POOL)
        assert ix.last_scan_info()[:2] == (5, 16)
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))

    b = ProductIndex(None, n_rows=n, dim=dim, dtype="bf16")
    b.store_rows_dev(Vd, normalize=False)
    torch.cuda.synchronize()
    same(b)
    b.close()
    c = ProductIndex(None, n_rows=n, dim=dim, dtype="bf16")
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(83)).to(dev)
    c.store_rows_dev(Vd[perm].contiguous(), row_ids=perm, normalize=False)
    torch.cuda.synchronize()
    same(c)
    c.close()
    mat = torch.zeros((n, 128), dtype=torch.bfloat16, device=dev)
    mat[:, :dim] = Vd.to(torch.bfloat16)                       # (round to nearest even, as the index's own stores)
    d = ProductIndex(None, n_rows=n, dim=dim, device_ptr=mat.data_ptr(), keepalive=mat, dtype="bf16")
    same(d)
    mat[:, :dim] = (Vd.flip(0) * 60.0).to(torch.bfloat16)
    torch.cuda.synchronize()
    d.matrix_changed()
    rows, scores = d.dense_topk(Q, POOL)
    assert d.last_scan_info()[:2] == (5, 16)
    for i in range(0, 33, 4):
        r1, s1 = d.dense_topk(Q[i:i + 1], POOL)
        assert np.array_equal(rows[i], r1[0]) and np.array_equal(_bits(scores[i]), _bits(s1[0])), i
    d.close()


def test_bf16_is_refused_above_1024_with_a_message_that_says_so():
    with pytest.raises(Exception, match="1024"):
        ProductIndex(None, n_rows=64, dim=1025, dtype="bf16")
