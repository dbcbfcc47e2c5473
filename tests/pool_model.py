"""What the mean-pooling tests share (tests/test_pool_model.py on the CPU, tests/test_gpu_k5_pool_kernel.py and
tests/test_gpu_k5_pool_forward.py on the GPU): seeded rows, and the error of a pooled row against float64 beside numpy
float32's own on the same rows -- the yardstick of the bar (twice numpy's, the rule of tests/test_gpu_k5_x3_kernels.py)."""
import numpy as np

F32, F64 = np.float32, np.float64


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def rows_of(hidden, data, lengths, seed=0):
    """(rows (sum of lengths, hidden) float32, cu_seqlens): N(0, 1) ("normal") or 1e4 + N(0, 1) ("offset": a common offset
    shows accumulation error)."""
    rng = np.random.default_rng([seed, hidden, len(lengths)])
    x = rng.standard_normal((int(np.sum(lengths)), hidden))
    if data == "offset":
        x = x + 1e4
    cu = np.zeros(len(lengths) + 1, dtype=np.int32)
    np.cumsum(lengths, out=cu[1:])
    return x.astype(F32), cu


def pool_errors(got, rows, cu):
    """(worst error of `got`, worst error of numpy float32's own mean) over every sequence and column, against the float64
    mean of the same float32 rows.  Error of a value = |value - float64 mean| / (the mean of |row| over the sequence, per
    column): what one rounding of the sum is relative to."""
    worst, worst_np = 0.0, 0.0
    for s in range(len(cu) - 1):
        r = rows[cu[s]:cu[s + 1]]
        want = r.astype(F64).mean(axis=0)
        scale = np.abs(r.astype(F64)).mean(axis=0)
        worst = max(worst, float((np.abs(got[s].astype(F64) - want) / scale).max()))
        worst_np = max(worst_np, float((np.abs(np.mean(r, axis=0, dtype=F32).astype(F64) - want) / scale).max()))
    return worst, worst_np
