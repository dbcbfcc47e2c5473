"""tests/rescore_model.py on the CPU: its float32 fused multiply-add against the C library's fmaf, both row chains against
the float64 dot product within the derived bound, the selection model against a brute-force sort, and the conditions under
which tests/test_gpu_rescore_kernels.py is not vacuous -- computed from the model alone, on the very inputs that file uses."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import rescore_model as M

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _fmaf(a, b, c):
    return np.array([_libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want):
    # bit for bit; any NaN equals any NaN (the kernels only ask "is it a NaN")
    g, w = _bits(got), _bits(want)
    return (g == w) | (np.isnan(got) & np.isnan(want))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_fma32_repairs_the_double_rounding_ties(sign):
    """a = +-24929, b = 673, c = +-k 2^-40: the float64 sum is exactly halfway between two float32 values and the addend decides.
    "float64, then cast" is wrong on all 2000 of them."""
    k = np.arange(1, 2001, dtype=np.float32)
    a, b = np.full(2000, np.float32(sign * 24929.0)), np.full(2000, np.float32(673.0))
    c = (np.float32(sign) * np.float32(2.0 ** -40) * k).astype(np.float32)
    want = _fmaf(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert int((_bits(naive) != _bits(want)).sum()) == 2000
    assert _same(M.fma32(a, b, c), want).all()


def test_fma32_equals_fmaf_on_random_and_extreme_triples():
    rng = np.random.default_rng(0)
    n = 150_000
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
    assert _same(M.fma32(a, b, c), _fmaf(a, b, c)).all()
    # a product that is an exact half ulp of c, or just beside it
    m = 20_000
    c2 = (np.float32(1.0) + np.float32(2.0 ** -23) * rng.integers(0, 1000, m).astype(np.float32)).astype(np.float32)
    a2 = np.full(m, np.float32(2.0 ** -12))
    b2 = (np.float32(2.0 ** -12) * (1 + rng.integers(-1, 2, m) * np.float32(2.0 ** -20))).astype(np.float32)
    for s in (1, -1):
        assert _same(M.fma32(s * a2, b2, c2), _fmaf(s * a2, b2, c2)).all()
    # near the overflow threshold and in the subnormal range (results that round to inf, to subnormals, to zero)
    big = (np.float32(3.0e38) * rng.uniform(0.5, 1.13, m)).astype(np.float32)
    x = rng.uniform(0.5, 2.0, m).astype(np.float32)
    y = (rng.uniform(-1.0, 1.0, m) * 3.0e38).astype(np.float32)
    assert _same(M.fma32(big, x, y), _fmaf(big, x, y)).all()
    tiny = (np.float32(2.0 ** -126) * rng.uniform(0.0, 4.0, m)).astype(np.float32)
    z = (np.float32(2.0 ** -140) * rng.integers(-4096, 4096, m).astype(np.float32)).astype(np.float32)
    w = rng.uniform(-1.0, 1.0, m).astype(np.float32)
    assert _same(M.fma32(tiny, w, z), _fmaf(tiny, w, z)).all()
    t2 = (np.float32(2.0 ** -75) * rng.uniform(1.0, 2.0, m)).astype(np.float32)
    assert _same(M.fma32(t2, t2 * w, z), _fmaf(t2, t2 * w, z)).all()
    sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0], dtype=np.float32)
    A, B, C = (g.ravel() for g in np.meshgrid(sp, sp, sp))
    assert _same(M.fma32(A, B, C), _fmaf(A, B, C)).all()


def test_keys_are_the_kernels_ordered_keys():
    f = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], dtype=np.float32)
    k = M.f2key(f)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert (_bits(M.key2f(k)) == _bits(f)).all()
    assert k[0] == 0x007FFFFF and k[-1] == 0xFF800000 and k[4] == 0x7FFFFFFF and k[5] == 0x80000000


@pytest.fixture(scope="module")
def scored():
    """The finite matrix and queries of the GPU tests with every model score: computed once, read-only."""
    V, Q = M.rescore_matrix(), M.rescore_queries()
    Vb = M.round_to_bf16(V)
    exact = np.stack([M.chain_f32(V, q) for q in Q])
    est = np.stack([M.chain_bf16(Vb, q) for q in Q])
    for a in (V, Q, Vb, exact, est):
        a.setflags(write=False)
    return V, Q, Vb, exact, est


def test_both_chains_stay_within_the_derived_bound_of_the_float64_dot_product(scored):
    V, Q, Vb, exact, est = scored
    for rows, got in ((V, exact), (Vb, est)):
        want = rows.astype(np.float64) @ Q.astype(np.float64).T
        mag = np.abs(rows.astype(np.float64)) @ np.abs(Q.astype(np.float64)).T
        assert (np.abs(got.T.astype(np.float64) - want) <= M.GAMMA_28 * mag).all()
    assert (exact[:, M.ZERO_ROW] == 0).all() and (_bits(exact[:, M.TWIN_ROWS[0]]) == _bits(exact[:, M.TWIN_ROWS[1]])).all()
    assert (exact != est).any()
    # the lane layout matters: another order of the same 384 products gives other bits on these rows
    other = np.stack([M.row16_sum(M._chain(V, q, 8)) for q in Q])
    assert (_bits(other) != _bits(exact)).mean() > 0.2


def test_special_values_end_as_minus_infinity_or_stay_infinite():
    V, Q = M.rescore_matrix(special=True), M.rescore_queries()
    exact = np.stack([M.chain_f32(V, q) for q in Q])
    est = np.stack([M.chain_bf16(M.round_to_bf16(V), q) for q in Q])
    assert np.isnan(exact[:, M.NAN_ROW]).all() and np.isnan(est[:, M.NAN_ROW]).all()
    assert np.isinf(exact[:, M.INF_ROW]).all() and np.isinf(exact[:, M.INF_ROW + 1]).all()
    stored = M.row_scores(exact[0], est[0], M.f2key(np.float32([0.5]))[0], np.float32(0.25))
    assert stored[M.NAN_ROW] == -np.inf and not np.isnan(stored).any()
    # a NaN bound, an infinite one and the key 0 ("not a score") send every row through the exact chain
    for tau, eps in ((M.f2key(np.float32([0.5]))[0], np.nan), (M.f2key(np.float32([0.5]))[0], np.inf), (np.uint32(0), 0.0)):
        assert M.takes_exact_chain(est[0], tau, np.float32(eps)).all()
    assert not M.takes_exact_chain(est[0][np.isfinite(est[0])], M.f2key(np.float32([np.inf]))[0], np.float32(0)).any()


def test_the_splitting_cut_skips_between_a_tenth_and_nine_tenths_of_the_listed_rows(scored):
    """Non-vacuity of the plane test: with tau = key of the 150th largest exact score and eps = 1.01 x the filter bound,
    between 10 % and 90 % of the rows of every list of 64 M-tiles or more (and of the whole matrix) take no exact chain,
    for every query whose flag is down."""
    V, Q, Vb, exact, est = scored
    for q in range(M.RESCORE_NQ - 1):
        tau, eps = M.split_cut(exact[q], V, Q[q])
        need = M.takes_exact_chain(est[q], tau, eps)
        assert need.sum() >= M.POOL and 0.1 <= 1 - need.mean() <= 0.9, (q, need.mean())
        top = np.argsort(-exact[q].astype(np.float64), kind="stable")[:M.POOL]
        assert need[top].all()                                   # (test_filter_bound.py's statement, on these rows)
        for c in M.RESCORE_COUNTS:
            mt, count, fb = M.rescore_lists(c)
            if count[q] < 64:
                continue
            rows = (mt[q, :count[q]].astype(np.int64)[:, None] * 8 + np.arange(8)).ravel()
            rows = rows[rows < M.RESCORE_ROWS]
            assert 0.1 <= 1 - need[rows].mean() <= 0.9, (q, c, need[rows].mean())


def test_the_lists_hold_what_the_gpu_tests_say_they_hold():
    for c in M.RESCORE_COUNTS:
        mt, count, fb = M.rescore_lists(c)
        assert mt.shape == (M.RESCORE_NQ, max(c, 1)) and mt.max() < M.RESCORE_TILES and fb.tolist() == [0, 0, 0, 0, 1]
        assert count.tolist() == [c, c, c, max(c - 2, 0), c]
        if c:
            assert mt[0, 0] == M.RAGGED and mt[1, c // 2] == M.RAGGED and mt[2, c - 1] == M.RAGGED
        if c >= 3:
            assert (mt[3, :count[3]] == M.RAGGED).sum() >= 1
        if c <= M.RESCORE_TILES - 1:
            assert all(len(set(mt[q, :c].tolist())) == c for q in (0, 1, 2))
    mt, count, fb = M.rescore_lists(600)
    assert (mt[3, 255:count[3]] == M.RAGGED).all() and len(set(mt[0].tolist())) < 600      # repeats; the ragged tile as padding
    # grid passes: a workgroup takes 16 M-tiles per pass with a plane or bf16 rows and 8 without; grids of 16 and 4 workgroups
    per_pass = sorted({g * 4 * u for g in (16, 4) for u in (4, 2)})
    assert per_pass == [32, 64, 128, 256]
    for p in per_pass:
        assert p in M.RESCORE_COUNTS and p + 1 in M.RESCORE_COUNTS and any(c < p for c in M.RESCORE_COUNTS)


def _brute(mtiles, count, fb, tau, sc, pool, rpm, floor_mode, n_rows, off):
    if fb:
        return 1, None, None
    half = M.rcap_of(pool) // 2
    items = []
    for s in range(count):
        for r in range(rpm):
            row = int(mtiles[s]) * rpm + r
            if row < n_rows:
                items.append((int(M.f2key(sc[s, r:r + 1])[0]), row))
    fill = floor_mode and count * rpm <= half
    cand = items if fill else [it for it in items if it[0] >= int(tau)]
    if len(cand) > half or len(cand) < pool:
        return 1, len(cand), None
    cand.sort(key=lambda it: (-it[0], it[1]))
    return 0, len(cand), cand[:pool]


def test_selection_model_against_a_brute_force_sort_with_ties():
    rng = np.random.default_rng(5)
    for trial in range(60):
        rpm, floor_mode = int(rng.choice([8, 16])), int(rng.integers(0, 2))
        pool = int(rng.choice([1, 7, 150, 512, 513, 700]))
        n_rows = int(rng.integers(300, 9000))
        n_tiles = (n_rows + rpm - 1) // rpm
        count = int(rng.integers(0, min(n_tiles, 1024) + 1))
        mt = rng.permutation(n_tiles)[:count].astype(np.uint32)
        sc = rng.choice(np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, 0.5, 1.0, 2.0, np.inf], dtype=np.float32), (count, rpm))
        tau = M.f2key(rng.choice(np.array([-np.inf, -0.0, 0.0, 0.5, 1.0], dtype=np.float32), 1))[0]
        fb = int(trial % 11 == 0)
        got = M.select_rescored(mt, count, fb, tau, sc, pool, rpm, floor_mode, n_rows, 1000)
        wfb, wn, wtop = _brute(mt, count, fb, tau, sc, pool, rpm, floor_mode, n_rows, 1000)
        assert got["fb"] == wfb and got["n_cand"] == wn
        if wtop is None:
            assert got["rows"] is None and got["scores"] is None
        else:
            assert got["rows"].tolist() == [r + 1000 for _, r in wtop]
            assert M.f2key(got["scores"]).tolist() == [k for k, _ in wtop]


def test_the_selection_cases_reach_the_branches_they_are_named_for():
    """Non-vacuity of the selection tests: from the model alone, every case has the candidate count it names, the flag it
    expects, a sort on the side of the 1024-key threshold it names, ties that cross M-tiles, and -- where it keeps its
    answer -- +inf scores in unlisted slots and rows past the end that must stay out."""
    seen = set()
    for key, cases in M.selection_launches().items():
        pool, rpm, floor_mode = key
        half = M.rcap_of(pool) // 2
        mt, count, fb, tau, sc = M.selection_launch_arrays(key, cases)
        assert len(cases) <= M.RR_SEL_MAXQ and mt.shape[1] <= M.RR_X3_MCAP
        n_mtiles = (M.SELECT_ROWS + rpm - 1) // rpm
        for i, case in enumerate(cases):
            assert len(set(mt[i, :count[i]].tolist())) == count[i] and (n_mtiles - 1) in mt[i, :count[i]]
            assert np.isinf(sc[i, count[i]:]).all() and (sc[i, count[i]:] > 0).all()
            r = M.select_rescored(mt[i], count[i], fb[i], tau[i], sc[i], pool, rpm, floor_mode, M.SELECT_ROWS, M.SELECT_OFFSET)
            if case["fb"]:
                assert r["n_cand"] is None and r["rows"] is None
                continue
            n1 = count[i] * rpm
            filled = floor_mode and n1 <= half
            assert r["n_cand"] == (count[i] * rpm - (n_mtiles * rpm - M.SELECT_ROWS) if filled else case["n_cand"])
            assert r["fb"] == int(case["expect_flag"]), case
            if r["fb"]:
                seen.add(("flag", "few" if r["n_cand"] < pool else "many", floor_mode, n1 <= half))
                continue
            seen.add(("rank" if r["n_cand"] <= M.RR_SEL_THREADS else "bitonic", half, rpm, floor_mode))
            assert np.isfinite(r["scores"]).all() and (r["rows"] < M.SELECT_ROWS + M.SELECT_OFFSET).all() and (r["rows"] >= M.SELECT_OFFSET).all()
            k = M.f2key(r["scores"]).astype(np.int64)
            assert (np.diff(k) <= 0).all() and (np.diff(r["rows"])[np.diff(k) == 0] > 0).all()
            if pool > 1:
                tie = np.diff(k) == 0
                assert tie.any() and ((r["rows"][1:] - M.SELECT_OFFSET) // rpm != (r["rows"][:-1] - M.SELECT_OFFSET) // rpm)[tie].any()
            if filled and case["n_cand"] < pool:
                assert (k < int(tau[i])).any()                      # rows below the cut fill the list up
    for want in (("flag", "few", 0, False), ("flag", "many", 0, False), ("flag", "few", 1, True), ("flag", "few", 1, False),
                 ("rank", 4096, 8, 0), ("bitonic", 4096, 8, 0), ("rank", 6144, 8, 0), ("bitonic", 6144, 8, 0), ("rank", 4096, 16, 0),
                 ("bitonic", 4096, 16, 0), ("bitonic", 6144, 16, 0), ("rank", 4096, 8, 1), ("bitonic", 4096, 8, 1)):
        assert want in seen, (want, sorted(seen, key=str))
    zero = [c for cs in M.selection_launches().values() for c in cs if c["cut"] == 0.0]
    assert len(zero) == 2
