"""CPU model of the per-row chain of a bf16 index at a runtime width (csrc/rr_dense_bf16w.hip: rr_scan_bf16_generic and its listed
form; csrc/rr_dense_fltw.hip: rr_rescore_chain_wb), plain numpy.  Nothing here reads a kernel's output.

    chain_wb        rows [n, D] float32 that ARE bf16 values, D a multiple of 64.  A row is D / 8 chunks of 8 elements; lane j of
                    16 takes chunks c = j + 16 i, i < ceil(D / 128); a chunk with 8 c >= D does not exist and adds nothing
                    (D = 64, 192, 320, ..: the last round is half full).  Per chunk eight fma32 in memory order onto the lane's
                    one accumulator, which starts at 0; then row16_sum (rescore_model.fma32 / row16_sum).
    stored_scores   what the scan and the rescoring store for these rows: the chain, NaN -> -inf
"""
import numpy as np

import rescore_model as RM


def chain_wb(rows, q):
    """float32 scores of bf16 rows [n, D] against the fp32 q [D]: bit for bit the per-row chain of the GPU."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, D = rows.shape
    assert D % 64 == 0 and D >= 64
    units = D // 8
    nr = (units + 15) // 16
    r = np.zeros((n, nr * 16, 8), dtype=np.float32)
    r[:, :units] = rows.reshape(n, units, 8)
    qq = np.zeros((nr * 16, 8), dtype=np.float32)
    qq[:units] = np.asarray(q, dtype=np.float32).reshape(units, 8)
    r, qq = r.reshape(n, nr, 16, 8), qq.reshape(nr, 16, 8)
    acc = np.zeros((n, 16), dtype=np.float32)
    for i in range(nr):
        exists = (np.arange(16) + 16 * i) < units
        new = acc
        for k in range(8):
            new = RM.fma32(r[:, i, :, k], qq[i, :, k][None, :], new)
        acc = np.where(exists[None, :], new, acc)          # a chunk that does not exist adds nothing
    return RM.row16_sum(acc)


def stored_scores(rows, q):
    s = chain_wb(rows, q)
    return np.where(np.isnan(s), np.float32(-np.inf), s).astype(np.float32)
