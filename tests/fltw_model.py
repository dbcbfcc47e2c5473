"""CPU models of the runtime-width filter path (csrc/rr_dense_fltw.hip), plain numpy.  Nothing here reads a kernel's output:
tests/test_fltw_bound.py checks the bound on the CPU, tests/test_gpu_fltw_kernels.py holds the kernels against the models.

    acc_coef(D)         c(D), the accumulation coefficient of the error bound, from ONE Python constant pair
    eps_wide            rr_fltw_prep_queries' eps in float64 (the 1.0001 of the cached row bounds left out: a smaller eps)
    gamma(D)            gamma_D = D u / (1 - D u): what flt_words_model calls GAMMA_384, at width D
    chain_w             rr_rescore_chain_w / rr_scan_f32_generic: lane j of 16 takes floats 4 (j + 16 i) .. + 3, i < nf = D / 64,
                        one fmaf chain from 0 in ascending order, then rr_row16_sum (rescore_model.fma32 / row16_sum)
"""
import os
import re

import numpy as np

import rescore_model as RM

ACC_COEF = 2.0 ** -14          # RR_FLTW_ACC_COEF
ACC_DIM = 384                  # RR_FLTW_ACC_DIM
U = 2.0 ** -24
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "review-recommender_amd", "csrc", "rr_dense_fltw.hip")


def acc_coef(dim_pad):
    return ACC_COEF * max(dim_pad, ACC_DIM) / ACC_DIM


def acc_coef_from_source():
    """(coefficient, dimension) of the #defines, and whether the formula beside them is max(D, dim) / dim."""
    text = open(_SRC).read()
    coef = float(re.search(r"#define\s+RR_FLTW_ACC_COEF\s+([0-9.eE+-]+)f", text).group(1))
    dim = int(re.search(r"#define\s+RR_FLTW_ACC_DIM\s+(\d+)", text).group(1))
    formula = re.search(r"return RR_FLTW_ACC_COEF \* \(float\)\(dim_pad > RR_FLTW_ACC_DIM \? dim_pad : RR_FLTW_ACC_DIM\) / \(float\)RR_FLTW_ACC_DIM;",
                        text) is not None
    return coef, dim, formula


def gamma(n):
    return n * U / (1 - n * U)


def bf16(x):
    return RM.round_to_bf16(x)


def eps_wide(V, Q):
    """eps per query of Q [nq, D] against the rows V [n, D] (D a multiple of 64), float64."""
    V64, Q64 = V.astype(np.float64), Q.astype(np.float64)
    Vr, Qr = bf16(V).astype(np.float64), bf16(Q).astype(np.float64)
    row_norm = np.linalg.norm(V64, axis=1).max()
    row_delta = np.linalg.norm(V64 - Vr, axis=1).max()
    return 1.01 * (row_delta * np.linalg.norm(Qr, axis=1) + row_norm * np.linalg.norm(Q64 - Qr, axis=1) +
                   acc_coef(V.shape[1]) * row_norm * np.linalg.norm(Q64, axis=1))


def chain_w(rows, q):
    """float32 scores of fp32 rows [n, D] against q [D], D = 64 nf: bit for bit the per-row chain of the GPU."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, D = rows.shape
    nf = D // 64
    assert D == 64 * nf
    r = rows.reshape(n, nf, 16, 4)
    qq = np.asarray(q, dtype=np.float32).reshape(nf, 16, 4)
    acc = np.zeros((n, 16), dtype=np.float32)
    for i in range(nf):
        for k in range(4):
            acc = RM.fma32(r[:, i, :, k], qq[i, :, k][None, :], acc)
    return RM.row16_sum(acc)


def stored_scores(rows, q):
    """what rr_rescore_chain_w stores for these rows: the chain, NaN -> -inf"""
    s = chain_w(rows, q)
    return np.where(np.isnan(s), np.float32(-np.inf), s).astype(np.float32)
