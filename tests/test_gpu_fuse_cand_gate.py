"""rr_fuse_topk_cand_dev (csrc/rr_fuse.hip): K3 with a CANDIDATE-aligned gate column that survives the shard merge.

The reference is the two-pass form the sharded path ran before: pass A (k = pool, no gate) fixes the pool order, the
factors are permuted on the host into that order by row, pass B takes them as the pool-aligned d_gate.  One pass with
d_cand_gate must give the same pool rows, the same 8 columns and the same order, bit for bit -- in contiguous and in gathered
([rank][query][pool]) addressing, through the binary-search merge of ordered lists and through the bitonic fallback."""
import ctypes as C

import numpy as np
import pytest
import torch

from review_recommender_amd import _lib, synth
from review_recommender_amd.engine import FusionWeights, HybridSearcher
from review_recommender_amd.index import ProductIndex
from review_recommender_amd.sharded import PayloadLayout

pytestmark = pytest.mark.gpu

W = FusionWeights(w_dense=0.45, w_bm25=0.25, w_rerank=0.0, w_prior=0.2, w_best=0.0, gate_penalty=0.5)
FACTORS = np.array([1.0, 1.0, 1.0, 0.5, 0.5, 0.25, 0.125, 0.0, 0.3, 0.77, 1.5, 3.0e-5], dtype=np.float32)


@pytest.fixture(scope="module")
def index():
    n = 512
    ix = ProductIndex(synth.unit_rows(n, 384, 7), row_offset=0)
    n_rev, stars = synth.metadata(n, 8, nan_fraction=0.05)
    ix.set_meta(n_rev.astype(np.float64), stars)
    return ix


def candidates(rng, B, world, pool, ordered=True, tie=False):
    """Per rank and query `pool` candidates with rows unique inside a query: dict of (world, B, pool) arrays.  Every rank's
    list is in K1's order (dense desc, row asc) unless ``ordered`` is False (rank 1's lists are shuffled).  ``tie``: the best
    candidate of rank 0 and of rank 1 share one dense score, above every other, and carry different factors.  Returns the
    dict and, per query, the two tied rows."""
    x = dict(rows=np.empty((world, B, pool), np.int64), dense=rng.uniform(-0.2, 0.9, (world, B, pool)).astype(np.float32),
             bm25=(rng.exponential(3.0, (world, B, pool)) * (rng.random((world, B, pool)) < 0.7)).astype(np.float32),
             n=np.floor(rng.lognormal(2.5, 1.5, (world, B, pool))).clip(0, 5000),
             avg=np.round(rng.uniform(1, 5, (world, B, pool)), 3),
             gate=rng.choice(FACTORS, (world, B, pool)))
    x["avg"][rng.random((world, B, pool)) < 0.03] = np.nan
    for r in range(world):
        for b in range(B):
            x["rows"][r, b] = 100_000 * r + rng.permutation(90_000)[:pool]
    if tie:
        x["dense"][0, :, 0] = x["dense"][1, :, 0] = np.float32(0.95)
        x["gate"][0, :, 0], x["gate"][1, :, 0] = np.float32(0.25), np.float32(1.0)
    tied = (x["rows"][0, :, 0].copy(), x["rows"][min(1, world - 1), :, 0].copy())
    for r in range(world):
        for b in range(B):
            o = np.lexsort((x["rows"][r, b], -x["dense"][r, b].astype(np.float64)))
            if not ordered and r == min(1, world - 1):
                o = rng.permutation(pool)
            for c in x:
                x[c][r, b] = x[c][r, b][o]
    x["l1p"] = np.log1p(x["n"])
    return x, tied


class Case:
    """The candidates on the device, gathered (cand_per_rank = pool, one payload block per rank) or contiguous
    ([query][world x pool], cand_per_rank = 0), and the three ways to call K3 on them."""

    def __init__(self, index, x, B, world, pool, gathered, k=None):
        self.ix, self.x, self.B, self.world, self.pool, self.k = index, x, B, world, pool, k or min(pool, 20)
        self.lib = _lib.load()
        if gathered:
            lay = PayloadLayout(B, pool, gate=True)
            host = torch.zeros((world, lay.nbytes), dtype=torch.uint8)
            for r in range(world):
                v = lay.views(host[r])
                for c in ("rows", "n", "avg", "l1p", "dense", "bm25", "gate"):
                    v[c].copy_(torch.from_numpy(x[c][r]))
            self.buf = host.cuda()
            base = self.buf.data_ptr()
            self.ptr = {c: base + getattr(lay, "off_" + c) for c in ("rows", "n", "avg", "l1p", "dense", "bm25", "gate")}
            self.geom = dict(cand_per_rank=pool, stride_bytes=lay.nbytes)
        else:
            self.t = {c: torch.from_numpy(np.ascontiguousarray(x[c].transpose(1, 0, 2).reshape(B, world * pool))).cuda() for c in x}
            self.ptr = {c: t.data_ptr() for c, t in self.t.items()}
            self.geom = dict(cand_per_rank=0, stride_bytes=0)

    def factor_of_row(self, b):
        return dict(zip(self.x["rows"][:, b].reshape(-1).tolist(), self.x["gate"][:, b].reshape(-1).tolist()))

    def run(self, k, gate=None, cand_gate=False, entry="cand", fill=None):
        B, pool = self.B, self.pool
        params = HybridSearcher.make_params(W, k, pool, self.world * pool, 0, **self.geom)
        mk = (lambda shape, dt: torch.full(shape, fill, dtype=dt, device="cuda")) if fill is not None else \
            (lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda"))
        out = mk((B, pool), torch.int64), mk((B, 8, pool), torch.float64), mk((B, k), torch.int32)
        p = self.ptr
        vp = lambda a: C.c_void_p(a) if a is not None else None
        head = [self.ix.handle, C.byref(params), B, vp(p["rows"]), vp(p["dense"]), vp(p["bm25"]), vp(p["n"]), vp(p["avg"]),
                vp(p["l1p"]), None, None, vp(gate.data_ptr() if gate is not None else None)]
        tail = [vp(t.data_ptr()) for t in out] + [C.c_void_p(torch.cuda.current_stream().cuda_stream)]
        if entry == "cand":
            rc = self.lib.rr_fuse_topk_cand_dev(*head, vp(p["gate"] if cand_gate else None), *tail)
        else:
            rc = self.lib.rr_fuse_topk_dev(*head, *tail)
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy() for t in out]

    def two_pass(self):
        rc, (rows_a, _, _) = self.run(self.pool, entry="plain")
        assert rc == 0
        gate = np.empty((self.B, self.pool), np.float32)
        for b in range(self.B):
            f = self.factor_of_row(b)
            gate[b] = [f[r] for r in rows_a[b].tolist()]
        rc, out = self.run(self.k, gate=torch.from_numpy(gate).cuda(), entry="plain")
        assert rc == 0
        return out, gate


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


CASES = [  # (name, B, world, pool, gathered, ordered, tie)
    ("no_merge_150", 5, 1, 150, False, True, False),
    ("no_merge_37_b1", 1, 1, 37, False, True, False),
    ("no_merge_gathered_one_rank", 5, 1, 37, True, True, False),
    ("world2_150", 5, 2, 150, True, True, False),
    ("world3_150_b1", 1, 3, 150, True, True, False),
    ("world8_150", 5, 8, 150, True, True, False),
    ("world3_37", 5, 3, 37, True, True, False),
    ("world8_37_b1", 1, 8, 37, True, True, False),
    ("unordered_list_bitonic_150", 5, 3, 150, True, False, False),
    ("unordered_list_bitonic_37", 5, 2, 37, True, False, False),
    ("contiguous_merge_bitonic", 5, 2, 37, False, True, False),
    ("dense_tie_across_ranks", 5, 2, 150, True, True, True),
    ("dense_tie_across_ranks_bitonic", 5, 2, 37, True, False, True),
]


@pytest.mark.parametrize("name,B,world,pool,gathered,ordered,tie", CASES, ids=[c[0] for c in CASES])
def test_one_pass_with_candidate_gate_equals_the_two_pass_form_bitwise(index, name, B, world, pool, gathered, ordered, tie):
    rng = np.random.default_rng(1000 + len(name) + 7 * world + pool)
    x, tied = candidates(rng, B, world, pool, ordered, tie)
    case = Case(index, x, B, world, pool, gathered)
    want, gate = case.two_pass()
    rc, got = case.run(case.k, cand_gate=True)
    assert rc == 0
    assert np.array_equal(got[0], want[0]), "pool rows"
    assert np.array_equal(got[1], want[1], equal_nan=True), "columns"
    assert np.array_equal(got[2], want[2]), "order"
    assert np.array_equal(got[1][:, 5], gate.astype(np.float64)), "the _gate column is the factor of the row in that place"
    # the gate decides something here: the ungated answer differs
    rc, plain = case.run(case.k)
    assert rc == 0 and not np.array_equal(plain[1][:, 7], got[1][:, 7], equal_nan=True)
    if tie:
        for b in range(B):
            r = got[0][b].tolist()
            i, j = r.index(int(tied[0][b])), r.index(int(tied[1][b]))
            assert (i, j) == (0, 1), "equal scores: the smaller global row first"
            assert got[1][b, 5, i] == 0.25 and got[1][b, 5, j] == 1.0, "the factor followed its row"


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("world,pool,B", [(1, 150, 5), (3, 37, 5), (8, 150, 1)])
def test_null_candidate_gate_is_rr_fuse_topk_dev_bitwise(index, gathered, world, pool, B):
    rng = np.random.default_rng(77 + world + pool)
    case = Case(index, candidates(rng, B, world, pool)[0], B, world, pool, gathered)
    rc_a, a = case.run(case.k, entry="plain")
    rc_b, b = case.run(case.k, entry="cand")
    assert rc_a == 0 and rc_b == 0 and same(a, b)
    gate = torch.from_numpy(rng.choice(FACTORS, (B, pool))).cuda()           # and with the pool-aligned column
    rc_a, a = case.run(case.k, gate=gate, entry="plain")
    rc_b, b = case.run(case.k, gate=gate, entry="cand")
    assert rc_a == 0 and rc_b == 0 and same(a, b)


def test_both_gate_columns_are_refused_and_nothing_is_written(index):
    rng = np.random.default_rng(5)
    B, world, pool = 3, 2, 37
    case = Case(index, candidates(rng, B, world, pool)[0], B, world, pool, True)
    gate = torch.ones((B, pool), dtype=torch.float32, device="cuda")
    rc, out = case.run(case.k, gate=gate, cand_gate=True, fill=-7)
    assert rc == -1                                                          # RR_E_INVALID
    assert b"not both" in case.lib.rr_last_error()
    assert all((t == -7).all() for t in out), "outputs untouched"
    with pytest.raises(ValueError):
        _lib.check(rc, "rr_fuse_topk_cand_dev")
