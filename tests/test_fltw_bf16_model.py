"""The CPU model of a bf16 index's per-row chain at a runtime width (tests/fltw_bf16_model.py), on the CPU.

1. At D = 384 the runtime-width chain is the 384 chain: chain_wb == rescore_model.chain_bf16 bit for bit (unit rows, rows of
   norm 0.01 .. 30, an all-zero row, rows with a NaN and with +-inf elements).
2. At D in {64, 192, 320, 768, 1024}, bf16 rows and fp32 queries: what rr_scan_fltw estimates -- the bf16 products a~_k bf16(q)_k,
   summed here in float64 -- stays within fltw_model.eps_wide of the chain.  eps_wide is evaluated on the ROUNDED rows, so its
   first term (max ||a - bf16(a)||) is exactly 0: the bound a bf16 index runs with (rr_row_norm_max<true> reports delta 0).
   The real scan adds D products in fp32 in its own order; that error is inside the same c(D) ||a|| ||q|| the bound sets aside
   (tests/test_fltw_bound.py), so the float64 sum is the sharper test of the two remaining terms.
"""
import numpy as np
import pytest

import fltw_bf16_model as WB
import fltw_model as W
import rescore_model as RM


def _rows(n, dim, seed, norms=None):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, dim)).astype(np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True).astype(np.float32)
    if norms is not None:
        m *= np.exp(rng.uniform(np.log(norms[0]), np.log(norms[1]), (n, 1))).astype(np.float32)
    return RM.round_to_bf16(m)


def test_at_384_the_runtime_width_chain_is_the_384_chain():
    V = np.concatenate([_rows(300, 384, 1), _rows(300, 384, 2, (0.01, 30.0))])
    V[7] = 0
    V[50, 5] = np.nan
    V[60, 200] = np.inf
    V[61, 383] = -np.inf
    rng = np.random.default_rng(3)
    for norm in (1.0, 7.5):
        q = rng.standard_normal(384).astype(np.float32)
        q *= np.float32(norm / np.linalg.norm(q))
        a, b = WB.chain_wb(V, q), RM.chain_bf16(V, q)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isnan(WB.chain_wb(V, q)[50]) and np.isneginf(WB.stored_scores(V, q)[50])


@pytest.mark.parametrize("dim", [64, 192, 320, 768, 1024])
def test_the_scan_estimate_stays_within_eps_of_the_chain(dim):
    for seed, norms, qnorm in ((10, None, 1.0), (11, (0.01, 30.0), 7.5)):
        V = _rows(2000, dim, seed + dim, norms)
        assert np.array_equal(RM.round_to_bf16(V).view(np.uint32), V.view(np.uint32))          # the rows ARE bf16 values
        rng = np.random.default_rng(seed + 1000)
        Q = rng.standard_normal((6, dim)).astype(np.float32)
        Q *= (qnorm / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
        Q[1] = V[17] * np.float32(qnorm / np.linalg.norm(V[17]))                               # a query that is a row
        eps = W.eps_wide(V, Q)
        # the delta term of the bound is 0 on rounded rows: eps is its two other terms
        row_norm = np.linalg.norm(V.astype(np.float64), axis=1).max()
        Q64, Qr = Q.astype(np.float64), W.bf16(Q).astype(np.float64)
        want = 1.01 * (row_norm * np.linalg.norm(Q64 - Qr, axis=1) + W.acc_coef(dim) * row_norm * np.linalg.norm(Q64, axis=1))
        assert np.array_equal(eps, want)
        est = V.astype(np.float64) @ Qr.T                                                      # [n, nq]
        for j in range(len(Q)):
            chain = WB.chain_wb(V, Q[j]).astype(np.float64)
            err = np.abs(est[:, j] - chain).max()
            assert err <= eps[j], (dim, j, err, eps[j])
