"""The error bound of the runtime-width filter path (csrc/rr_dense_fltw.hip: rr_fltw_prep_queries), checked in numpy at
D = 64, 768, 1024 on the row kinds of tests/test_filter_bound.py:

    eps = 1.01 (max||a - a~|| ||q~|| + max||a|| ||q - q~|| + c(D) max||a|| ||q||),   c(D) = 2^-14 max(D, 384) / 384

must bound |s~ - s| for the float64 products of the bf16 operands, and |s~32 - chain32| for a float32 accumulation of those
products in two adversarial orders (ascending and descending magnitude: one loses the small terms last, the other first)
against the 16-lane fmaf chain at nf = D / 64 that defines the answer; and the containment argument built on it must hold:
the exact top-pool of the chain scores lies among the rows with s~ >= tau~ - 2 eps."""
import numpy as np
import pytest

import fltw_model as W


def test_the_python_constant_is_the_one_in_the_source():
    coef, dim, formula = W.acc_coef_from_source()
    assert np.float32(coef) == np.float32(W.ACC_COEF) and dim == W.ACC_DIM and formula
    # 2^-14 is 2 gamma_384 with a margin of 1.33; c(D) keeps that margin over 2 gamma_D at every width from 384 up
    for D in (384, 448, 768, 1024):
        assert 1.33 < W.acc_coef(D) / (2 * W.gamma(D)) < 1.3334
    assert W.acc_coef(64) == W.ACC_COEF and W.acc_coef(1024) == W.ACC_COEF * 1024 / 384


def _rows(kind, D, n=5000):
    rng = np.random.default_rng(7 + D)
    V = rng.standard_normal((n, D)).astype(np.float32)
    q = rng.standard_normal(D).astype(np.float32)
    if kind == "unit":
        V /= np.linalg.norm(V, axis=1, keepdims=True)
        q /= np.linalg.norm(q)
    elif kind == "scaled":
        V *= rng.uniform(0.01, 30.0, (len(V), 1)).astype(np.float32)
        q *= np.float32(7.5)
    else:   # rows proportional to the query, every product of one sign, mantissas that round badly
        V = (np.abs(q)[None, :] * rng.uniform(0.5, 1.5, (len(V), 1))).astype(np.float32) * np.float32(1 + 2 ** -9)
        q = np.abs(q)
    return V, q


def _f32_sum(prod):
    """sequential float32 accumulation along axis 1"""
    acc = np.zeros(prod.shape[0], dtype=np.float32)
    for k in range(prod.shape[1]):
        acc = acc + prod[:, k]
    return acc


@pytest.mark.parametrize("kind", ["unit", "scaled", "aligned"])
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_wide_filter_scores_stay_within_the_bound(D, kind):
    V, q = _rows(kind, D)
    eps = W.eps_wide(V, q[None, :])[0]
    Vr, qr = W.bf16(V), W.bf16(q)
    s = V.astype(np.float64) @ q.astype(np.float64)
    s_approx = Vr.astype(np.float64) @ qr.astype(np.float64)
    assert np.abs(s_approx - s).max() <= eps
    chain = W.chain_w(V, q).astype(np.float64)
    prod = Vr * qr[None, :]                                   # a bf16 x bf16 product is exact in float32 (16 significant bits)
    order = np.argsort(np.abs(prod), axis=1)
    asc = np.take_along_axis(prod, order, axis=1)
    approx32 = {"ascending": _f32_sum(asc), "descending": _f32_sum(asc[:, ::-1])}
    pool = 20
    top = set(np.lexsort((np.arange(len(chain)), -chain))[:pool].tolist())
    for name, s32 in list(approx32.items()) + [("float64", s_approx)]:
        s32 = s32.astype(np.float64)
        assert np.abs(s32 - chain).max() <= eps, (name, np.abs(s32 - chain).max(), eps)
        # containment: tau~ = the pool-th largest approximate score (the kernel uses a lower bound of it)
        tau = np.sort(s32)[-pool]
        cand = set(np.nonzero(s32 >= tau - 2 * eps)[0].tolist())
        assert top <= cand, name
        assert (chain[list(top)] >= tau - eps).all(), name    # the row cut after rescoring keeps them
