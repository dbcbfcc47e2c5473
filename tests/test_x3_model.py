"""CPU checks of tests/x3_model.py, the numpy model tests/test_gpu_x3_scan_kernels.py holds the split-operand dense scans to:
the split's exactness and its domain, what it makes of inf / NaN, the plane orders, and -- what keeps the GPU cases from being
vacuous -- that on every input family with a bar the model alone stays inside the bar while every defect (each kept term
dropped in turn, the two-term split, a wrong plane order) leaves it, by 4x where the bar is a number.
"""
import numpy as np
import pytest

import x3_model as M


def _sum3(t):
    return t[0].astype(np.float64) + t[1].astype(np.float64) + t[2].astype(np.float64)


def _random_f32(rng, n, lo, hi):
    m = rng.integers(0, 1 << 23, size=n, dtype=np.uint32)
    return M.signs(rng, n) * np.ldexp(M.from_bits(np.uint32(0x3F800000) | m), rng.integers(lo, hi + 1, size=n)).astype(np.float32)


def test_split_is_exact_and_every_term_is_a_bf16_number():
    rng = np.random.default_rng(1)
    x = _random_f32(rng, 1_000_000, -100, 99)
    t = M.split3(x)
    assert (_sum3(t) == x.astype(np.float64)).all()
    for term in t:                                            # each term fits the 16 bits an MFMA operand keeps
        assert ((M.bits(term) & np.uint32(0xFFFF)) == 0).all()
    assert (_sum3(M.split3_stored(x)) == x.astype(np.float64)).all()
    # the terms do not overlap: |x2| < 2^-7 |x1|, |x3| < 2^-15 |x1|
    assert (np.abs(t[1]) < np.abs(t[0]) * 2.0 ** -7).all() and (np.abs(t[2]) < np.abs(t[0]) * 2.0 ** -15).all()


def test_split_domain_ends_at_two_to_the_minus_110():
    """Exact for |x| >= 2^-110: the third term is then at least 2^-126 in its lowest set bit, a normal number or a subnormal
    whose low 16 bits are clear.  Below, the third term is an fp32 subnormal whose low 16 bits the planes cut: the stored sum
    misses less than 2^-133 -- harmless in size, but outside the "exact sum" claim."""
    rng = np.random.default_rng(2)
    m = rng.integers(0, 1 << 23, size=200_000, dtype=np.uint32) | np.uint32(1)          # lowest bit set: x3 reaches bit 0
    for e in (-110, -109, -100, 0, 100, 127):
        x = np.ldexp(M.from_bits(np.uint32(0x3F800000) | m), e).astype(np.float32)
        assert (_sum3(M.split3_stored(x)) == x.astype(np.float64)).all(), e
    x = np.ldexp(M.from_bits(np.uint32(0x3F800000) | m), -111).astype(np.float32)
    miss = np.abs(_sum3(M.split3_stored(x)) - x.astype(np.float64))
    assert (_sum3(M.split3(x)) == x.astype(np.float64)).all()            # the fp32 terms are still exact ...
    assert miss.max() > 0 and miss.max() < 2.0 ** -133                    # ... their 16-bit images are not
    # zeros and subnormal inputs: no NaN, nothing larger than the input
    z = np.float32([0.0, -0.0, 1e-45, -1e-40, 1.1754942e-38])
    assert np.isfinite(_sum3(M.split3_stored(z))).all() and (np.abs(_sum3(M.split3_stored(z))) <= np.abs(z)).all()


def test_split_of_inf_and_nan():
    """+-inf -> (+-inf, NaN, NaN): x - x1 is inf - inf.  So a row with an inf element scores NaN in these scans (-inf after
    rr_x3_canon), also in bf16 storage, where inf * q2 with q2 = 0 is NaN; the per-row chain gives +-inf."""
    for v in (np.inf, -np.inf):
        t = M.split3(np.float32([v]))
        assert t[0][0] == v and np.isnan(t[1][0]) and np.isnan(t[2][0])
    assert all(np.isnan(t[0]) for t in M.split3(np.float32([np.nan])))
    A = np.zeros((2, M.DIM), dtype=np.float32)
    A[0, 3], A[1, 3] = np.inf, 1.0
    Q = np.zeros((1, M.DIM), dtype=np.float32)
    Q[0, 3] = 0.5                                             # a bf16 number: q2 = q3 = 0
    for bf16 in (False, True):
        s = M.kept_sum(A, Q, bf16)
        assert np.isnan(s[0, 0]) and s[0, 1] == 0.5
        assert M.canon(s)[0, 0] == -np.inf
    assert (Q.astype(np.float64) @ A.astype(np.float64).T)[0, 0] == np.inf


def test_plane_orders_are_permutations_of_each_32_dim_group():
    for order in (M.ORDER_NATURAL, M.ORDER_PAIR64, M.ORDER_WIDE_BF16):
        src = M.plane_src(order)
        assert sorted(src.tolist()) == list(range(M.DIM))
        assert ((src >> 5) == (np.arange(M.DIM) >> 5)).all()
    assert (M.plane_src(M.ORDER_NATURAL) == np.arange(M.DIM)).all()
    # PAIR64: slot (kg, j) = dim 4kg + j | 16 + 4kg + (j - 4); WIDE_BF16: K-step v, slot (h, j) = dim 16h + 8v + j
    assert M.plane_src(M.ORDER_PAIR64)[:16].tolist() == [0, 1, 2, 3, 16, 17, 18, 19, 4, 5, 6, 7, 20, 21, 22, 23]
    assert M.plane_src(M.ORDER_WIDE_BF16)[:32].tolist() == list(range(0, 8)) + list(range(16, 24)) + list(range(8, 16)) + list(range(24, 32))


def test_planes_check_tells_the_orders_apart():
    rng = np.random.default_rng(3)
    Q = M.signs(rng, (5, M.DIM)) * M.mantissas(rng, (5, M.DIM))
    got = {o: M.planes(Q, 16, o) for o in (M.ORDER_NATURAL, M.ORDER_PAIR64, M.ORDER_WIDE_BF16)}
    assert (got[0] != got[1]).any() and (got[0] != got[2]).any() and (got[1] != got[2]).any()
    p = got[0].astype(np.uint32) << 16
    assert (p.view(np.float32).astype(np.float64).sum(axis=0)[:5] == Q.astype(np.float64)).all()
    assert (got[0][:, 5:] == 0).all()                          # zero queries fill the slots


FILLS = {"i": M.fill_i, "ii": M.fill_ii, "iii": M.fill_iii}


def _stored(A, bf16):
    return M.round_to_bf16(A) if bf16 else A


@pytest.mark.parametrize("fill,bf16", [("i", False), ("i", True), ("ii", False), ("iii", False), ("iii", True)],
                         ids=["i-fp32", "i-bf16", "ii-fp32", "iii-fp32", "iii-bf16"])      # (ii: full-mantissa rows, fp32 storage only)
def test_bitwise_fills_are_exact_and_every_pinned_defect_changes_bits(fill, bf16):
    """Case a: the model's score is an fp32 number (so any order of the exact partial sums gives its bits), equals the plain
    product, and each fill changes bits under the defects it is said to pin; together the fills pin every kept term."""
    A, Q = FILLS[fill](17, 40)
    S = _stored(A, bf16)
    m = M.kept_sum(S, Q, bf16)
    assert np.isfinite(m).all() and (m.astype(np.float32).astype(np.float64) == m).all()
    assert (m == Q.astype(np.float64) @ S.astype(np.float64).T).all()
    hot = np.arange(len(A)) % M.DIM
    assert (m != 0).all() and (np.abs(m) >= 2.0 ** -100).all()            # every product normal, none zero
    if fill == "iii" and not bf16:
        assert (m == 1 + 2.0 ** -8 + 2.0 ** -18).all()
    pinned = {"i": ["no a1q1", "no a1q2", "no a1q3", "two-term split"], "ii": ["no a1q1", "no a2q1", "no a3q1", "two-term split"],
              "iii": ["no a1q1", "no a1q2"] if bf16 else ["no a1q1", "no a1q2", "no a2q1", "no a2q2"]}[fill]
    for name in pinned:
        d = M.kept_sum(S, Q, bf16, **M.defects(bf16)[name])
        changed = d.astype(np.float32).view(np.uint32) != m.astype(np.float32).view(np.uint32)
        assert changed.all(), (fill, name, int((~changed).sum()))
    # a wrong k order: the planes permuted inside a 32-dim group move every product to another dim's row.  Fill i's job
    # (full-mantissa queries: two dims never hold the same value); in ii and iii the query values repeat across dims.
    for wrong in (M.ORDER_PAIR64, M.ORDER_WIDE_BF16) if fill == "i" else ():
        src = M.plane_src(wrong)
        d = M.kept_sum(S, Q[:, src], bf16)
        moved = src[hot] != hot
        assert (d[:, moved].astype(np.float32).view(np.uint32) != m[:, moved].astype(np.float32).view(np.uint32)).all()
        assert moved.sum() >= len(A) // 2


def test_the_fills_pin_every_kept_term():
    pinned32 = {"no a1q1", "no a1q2", "no a1q3", "no a2q1", "no a3q1", "no a2q2", "two-term split"}
    assert pinned32 == set(M.defects(False))
    assert {"no a1q1", "no a1q2", "no a1q3", "two-term split"} == set(M.defects(True))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_one_product_bar_holds_for_the_model_and_no_defect_comes_within_4x(bf16):
    """Case b.  The model's own distance from the exact product is the dropped terms (< 2^-21); the accumulator's share of
    the bar (6 x 2^-24) is left to the kernel.  Every defect is at least 4 bars away on EVERY product."""
    worst_model, least_defect = 0.0, np.inf
    for seed in range(4):
        A, Q = M.fill_b(64, 100 + seed)
        S = _stored(A, bf16)
        exact = Q.astype(np.float64) @ S.astype(np.float64).T
        assert (exact != 0).all() and np.isfinite(exact.astype(np.float32)).all() and (np.abs(exact) > 2.0 ** -90).all()
        m = M.kept_sum(S, Q, bf16)
        worst_model = max(worst_model, float((np.abs(m - exact) / np.abs(exact)).max()))
        for name, kw in M.defects(bf16).items():
            d = M.kept_sum(S, Q, bf16, **kw)
            least_defect = min(least_defect, float((np.abs(d - exact) / np.abs(exact)).min()))
    print(f"one-product: model {worst_model:.3e}, bar {M.ONE_PRODUCT_BAR:.3e}, least defect {least_defect:.3e}")
    assert worst_model < 2.0 ** -21 <= M.ONE_PRODUCT_BAR - 6 * 2.0 ** -24
    assert (worst_model == 0.0) == bf16                                   # bf16 rows drop nothing
    assert least_defect >= 4 * M.ONE_PRODUCT_BAR


@pytest.mark.parametrize("kind", M.DENSE_KINDS)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_dense_sets_model_inside_the_bar_of_four_float32_errors(kind, bf16):
    """Case c.  The bar is 4 x the error of numpy's float32 product on the same data; the model (dropped terms only) is far
    inside.  The two-term defect is NOT reliably outside on dense data (printed): the one-product cases catch it."""
    Q = M.dense_queries(64, 3)
    A = _stored(M.dense_rows(kind, 1000, Q, 3), bf16)
    f32_err = M.rel_error(M.f32_matvec(A, Q), A, Q)
    model = M.rel_error(M.kept_sum(A, Q, bf16), A, Q)
    two = M.rel_error(M.kept_sum(A, Q, bf16, two_term=True), A, Q)
    print(f"{kind} {'bf16' if bf16 else 'fp32'}: model {model:.3e}, float32 {f32_err:.3e}, bar {4 * f32_err:.3e}, two-term {two:.3e}")
    assert np.isfinite(A).all() and 0 < f32_err < 1e-5
    assert 4 * model < 4 * f32_err
    if kind == "cancelling":
        A64, Q64 = A.astype(np.float64), Q.astype(np.float64)
        r = np.arange(len(A))
        own = np.abs((Q64[r % 64] * A64).sum(axis=1)) / np.abs(Q64[r % 64] * A64).sum(axis=1)
        assert own.max() < 1e-6 and not bf16 or bf16


def test_maxima_plants_and_lists_reach_what_they_are_meant_to():
    Q = M.dense_queries(5, 9)
    A0 = M.maxima_matrix()
    n_tiles = (M.MAXIMA_ROWS + 63) // 64
    for C in (2, 4):
        A, rows = M.maxima_plants(A0, Q, C)
        s = M.canon(M.kept_sum(A, Q, False).astype(np.float32))
        for q, rr in rows.items():
            assert set(np.argsort(-s[q])[:len(rr)].tolist()) == set(rr)
        assert rows[0][0] // 64 == C and rows[0][0] % 64 < 16               # first M-tile of group 1's run
        assert rows[1][0] // 64 == C - 1 and rows[1][0] % 64 >= 48          # last M-tile of group 0's run
        assert rows[2][0] // 16 == (M.MAXIMA_ROWS - 1) // 16 and M.MAXIMA_ROWS % 16 != 0
        assert rows[3][0] // 16 != rows[3][1] // 16 and rows[3][0] // (64 * C) == rows[3][1] // (64 * C)
        assert M.bits(s[3, rows[3][0]]) == M.bits(s[3, rows[3][1]])
    assert n_tiles == 32
    mt, count, fb = M.rescore_lists(M.MAXIMA_ROWS, 17)
    n_mt = (M.MAXIMA_ROWS + 15) // 16
    assert mt[0, 0] == n_mt - 1 and {0, 1} <= set(mt[0, :count[0]].tolist()) and count[2] == 0 and fb[3] == 1
    assert len(set(mt[1, :count[1]].tolist())) < count[1] and count[4] == mt.shape[1]
    assert all((mt[q, :count[q]] < n_mt).all() for q in range(17))


def test_nonfinite_matrix_has_every_kind_in_full_and_ragged_tiles():
    A, rows = M.nonfinite_matrix()
    n = len(A)
    last_tile = (n - 1) // 64
    assert n % 64 != 0 and n <= 2048
    for k, rr in rows.items():
        assert any(r // 64 == last_tile for r in rr) and any(r // 64 < last_tile for r in rr), k
    assert np.isnan(A[rows["nan"]]).any(axis=1).all()
    assert (A[rows["+inf"]] == np.inf).any(axis=1).all() and (A[rows["-inf"]] == -np.inf).any(axis=1).all()
    assert ((A[rows["+-inf"]] == np.inf).any(axis=1) & (A[rows["+-inf"]] == -np.inf).any(axis=1)).all()
    assert np.isfinite(A[rows["overflow"]]).all()
    Q = M.nonfinite_queries(4)
    with np.errstate(over="ignore", invalid="ignore"):
        prod = A[rows["overflow"]][:, None, :] * Q[None]                                          # float32 products
    assert np.isinf(prod).any(axis=2).all() and not np.isnan(prod).any()
    assert {np.sign(A[r, 0]) for r in rows["overflow"]} == {1.0, -1.0}
    special = sorted(r for rr in rows.values() for r in rr)
    assert len(set(special)) == len(special)
    assert np.isfinite(np.delete(A, special, axis=0)).all()
