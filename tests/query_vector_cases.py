"""The rows and the reference the query-vector tests share (the model on the CPU, the kernel on the GPU)."""
import functools

import numpy as np

# every branch of numpy's pairwise split and its tails: below 8, the eight-accumulator block (8 .. 128) with and without a
# tail, one split with equal and unequal halves, two splits (384 = four pieces of 96), uneven pieces, six splits
WIDTHS = [1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 255, 256, 257, 383, 384, 385, 1000, 1024, 8192]


@functools.lru_cache(maxsize=None)
def _rows_of(dim: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + dim)
    base = rng.standard_normal((9, dim)).astype(np.float32)
    e = np.empty((9, dim), dtype=np.float32)
    with np.errstate(over="ignore"):
        e[0], e[1], e[2] = base[0] * np.float32(1e-3), base[1], base[2] * np.float32(30)      # random at three scales
        e[3] = 0                                                                            # a zero row
        e[4] = base[4] * np.float32(1e-25)       # squares denormal or zero, norm below eps
        e[5] = base[5] * np.float32(1e25)        # squares overflow
        e[6] = base[6]
        e[6, dim // 2] = np.nan                  # one NaN
        e[7] = base[7]
        e[7, (2 * dim) // 3] = np.inf            # one +Inf
        e[8] = np.abs(base[8]) * np.where(np.arange(dim) % 2 == 0, 1, -1).astype(np.float32)   # alternating signs
    e.setflags(write=False)
    return e


def rows_of(dim: int) -> np.ndarray:
    """(9, dim) float32, read-only: random rows at scales 1e-3, 1 and 30, a zero row, a row whose squares are denormal, a row
    whose squares overflow, a row with one NaN, a row with one +Inf, a row of alternating signs."""
    return _rows_of(dim)


def batch_of(dim: int, n: int) -> np.ndarray:
    """(n, dim) float32: the rows of `rows_of` first, then random rows at the three scales in turn."""
    e = np.empty((n, dim), dtype=np.float32)
    head = rows_of(dim)[:n]
    e[:len(head)] = head
    if n > len(head):
        rng = np.random.default_rng(7 * dim + n)
        scale = np.array([1e-3, 1.0, 30.0], dtype=np.float32)[np.arange(n - len(head)) % 3]
        e[len(head):] = rng.standard_normal((n - len(head), dim)).astype(np.float32) * scale[:, None]
    return e


def numpy_vectors(e: np.ndarray) -> np.ndarray:
    """QueryEncoder.encode_ids' normalisation (cross_encoder.py), the reference of every query-vector test."""
    with np.errstate(all="ignore"):
        return (e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)).astype(np.float32)


def assert_bitwise(got: np.ndarray, want: np.ndarray) -> None:
    """Equal as uint32 bit patterns; where the reference is NaN the other must be NaN (any payload)."""
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere((g != w) & ~nan)
    assert len(bad) == 0, f"{len(bad)} element(s) differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
