"""The numpy model of the filter scans' tile word (flt_words_model.py) against itself: words built by the model from random
unit rows pass check_words(); each of seven ways a scan kernel could get a word wrong is then applied to those words and
check_words() has to name it -- property, tile, query, direction.  No GPU: test_gpu_flt_words.py holds the kernels against
the same check."""
import numpy as np
import pytest

import flt_words_model as M

N_ROWS = 64 * 40 + 5             # a ragged end: 32-row tile 80 has 5 real rows (three of its M-tiles have none), tile 81 none
NQ = 32
SENTINEL = 0x5A5A7FC1


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(11)
    a = rng.standard_normal((N_ROWS, 384)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    q = rng.standard_normal((NQ, 384)).astype(np.float32)
    q *= 7.5 / np.linalg.norm(q, axis=1, keepdims=True)
    q[3] = 7.5 * a[N_ROWS - 1]                   # a query that is a row: the matrix's LAST row (what a pad row would repeat)
    q[7] = 7.5 * a[1000]
    ab, qb = M.bf16_rne(a), M.bf16_rne(q)
    n_tiles = (N_ROWS + 63) // 64
    # runs of 8 tiles in groups of 2; the last run holds one tile: three groups without any
    geom = {"n_rows": N_ROWS, "n_tiles": n_tiles, "tiles_per_wave": 8, "n_waves": (n_tiles + 7) // 8, "gpw": 4, "tiles_per_group": 2}
    M8, delta = M.reference_m8(ab, qb, 2 * n_tiles)
    # the kernel's own bound, per query: 1.01 (row_delta ||q~|| + row_norm ||q - q~|| + 2^-14 row_norm ||q||)
    row_norm = np.linalg.norm(a.astype(np.float64), axis=1).max()
    row_delta = np.linalg.norm(a.astype(np.float64) - ab, axis=1).max()
    eps = (1.01 * (row_delta * np.linalg.norm(qb.astype(np.float64), axis=1) + row_norm * np.linalg.norm(q.astype(np.float64) - qb, axis=1)
                   + 2.0 ** -14 * row_norm * np.linalg.norm(q.astype(np.float64), axis=1))).astype(np.float32)
    m8_f32 = M8.astype(np.float32)               # a scan without summation error
    words = M.encode_words(m8_f32, eps)
    ng = geom["n_waves"] * geom["gpw"]
    keys = np.zeros((ng, NQ), dtype=np.uint32)
    for gi in range(ng):
        lo, hi = M.group_tiles(geom, gi)
        if hi > lo:
            keys[gi] = M.f2key(m8_f32[lo:hi].max(axis=(0, 1)))
    return {"a": ab, "q": qb, "geom": geom, "M8": M8, "delta": delta, "eps": eps, "words": words, "keys": keys, "m8": m8_f32}


def run(w, words=None, keys=None, **kw):
    return M.check_words(w["words"] if words is None else words, w["keys"] if keys is None else keys, w["geom"], w["M8"],
                         w["delta"], w["eps"], sentinel=SENTINEL, **kw)


def test_number_formats_and_codes():
    x = np.array([1.0, 1.0 + 2.0 ** -9, -1.0 - 2.0 ** -9, 0.0, np.inf, -np.inf, 3.0e-40], dtype=np.float32)
    up = M.bf16_val(M.bf16_up_bits(x))
    assert np.all(up >= x) and up[1] == np.float32(1.0 + 2.0 ** -7) and up[2] == np.float32(-1.0) and up[4] == np.inf and up[5] == -np.inf
    assert M.bf16_up(np.float64(1.0) + 1e-12) == 1.0 + 2.0 ** -7 and M.f32_up(np.float64(1.0) + 1e-12) == np.float32(1.0 + 2.0 ** -23)
    k = M.f2key(x)
    assert np.array_equal(M.key2f(k).view(np.uint32), x.view(np.uint32)) and np.all(np.diff(k[[5, 2, 3, 6, 0, 1, 4]].astype(np.int64)) > 0)
    # the gap encoder: codes 0..7 one step each, 8..15 two steps each, the 0.9999 factor keeps an exact multiple below its
    # code, the clamp, inf - inf; the decoder
    step = np.float32(0.25)
    inv = M.inv_step_of(step)
    gaps = np.array([0, 0.99, 1.0, 1.01, 7.5, 8.01, 9.99, 10.01, 21.9, 22.01, 23.9, 24.5, 1000.0], dtype=np.float32) * step
    codes = M.gap_code(np.float32(5.0), np.float32(5.0) - gaps, inv)
    assert codes.tolist() == [0, 0, 0, 1, 7, 8, 8, 9, 14, 15, 15, 15, 15]
    assert M.gap_code(np.float32(-np.inf), np.float32(-np.inf), inv) == 15 and M.gap_code(np.float32(1.0), np.float32(-np.inf), inv) == 15
    assert M.gap_code(np.float32(1.0), np.float32(0.5), M.inv_step_of(0.0)) == 0
    assert M.gap_steps(np.arange(16)).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22]
    assert M.gap_step(np.array([0.0, np.inf, 0.5, 0.25, np.nan], dtype=np.float32)) == np.float32(0.125)
    assert M.gap_step(np.array([0.0, np.inf], dtype=np.float32)) == 0


def test_derived_delta_sits_inside_the_kernels_own_budget(world):
    """gamma_384 sum |a~ q~| (any fp32 summation order) is below the 2^-14 ||a|| ||q|| the kernel's eps sets aside for the
    scan's and the chain's accumulations together."""
    budget = 2.0 ** -14 * np.linalg.norm(world["a"].astype(np.float64), axis=1).max() * np.linalg.norm(world["q"].astype(np.float64), axis=1)
    assert np.all(world["delta"].max(axis=(0, 1)) < budget)
    assert np.all(world["delta"].max(axis=(0, 1)) < 0.05 * M.gap_step(world["eps"]))      # ... and far below one step


def test_model_words_pass_every_property(world):
    bad, st = run(world)
    assert not bad, M.describe(bad, st)
    assert st["words"] == world["words"].size and st["keys"] == world["keys"].size and st["far"] > 0
    assert 0 < st["tight_steps"] < 3.5 and st["safe_delta"] <= 0.0, st
    # the query that is a row: its tile maximum is ||row||^2 * 7.5 in bf16 operands, the word's maximum covers it
    t, r = divmod(1000, 32)
    assert M.bf16_val(world["words"][t, 7] & 0xFFFF) >= world["M8"][t, r // 8, 7] > 7.0


def names(bad):
    return {(v["prop"], v["direction"]) for v in bad}


def test_mutation_maximum_rounded_down(world):
    w = world["words"].copy()
    down = M.bf16_val(M.bf16_up_bits(world["m8"].max(axis=1))) > world["m8"].max(axis=1)     # words the round-up moved
    w[down] -= 1                                                                              # (positive maxima: one bf16 ulp down)
    assert down[:, 3].any() and np.all(world["m8"].max(axis=1)[down] > 0)
    bad, st = run(world, words=w)
    assert ("P1", "low") in names(bad), M.describe(bad, st)
    assert 0.9 * down.sum() < st["counts"][("P1", "low")] <= down.sum()      # (all but the maxima within delta of a bf16 value)
    v = next(v for v in bad if v["prop"] == "P1")
    assert down[v["tile"], v["query"]] and v["sub"] is None and v["got"] < v["limit"]


def test_mutation_gap_code_rounded_up(world):
    w = world["words"].copy()
    g = 2
    code = (w >> np.uint32(16 + 4 * g)) & np.uint32(15)
    hit = code < 15
    w[hit] += np.uint32(1 << (16 + 4 * g))
    bad, st = run(world, words=w)
    assert names(bad) == {("P2", "low")}, M.describe(bad, st)
    assert all(v["sub"] == g and hit[v["tile"], v["query"]] and v["got"] < v["limit"] for v in bad)
    assert st["safe_delta"] > 1.0


def test_mutation_two_sub_tiles_swapped(world):
    w = world["words"].copy()
    c0, c1 = (w >> np.uint32(16)) & np.uint32(15), (w >> np.uint32(20)) & np.uint32(15)
    w = (w & np.uint32(0xFF00FFFF)) | (c1 << np.uint32(16)) | (c0 << np.uint32(20))
    bad, st = run(world, words=w)
    assert ("P2", "low") in names(bad) and ("P4", "high") in names(bad), M.describe(bad, st)
    assert all(v["sub"] in (0, 1) for v in bad if v["prop"] in ("P2", "P4"))
    differ = c0 != c1
    assert all(differ[v["tile"], v["query"]] for v in bad)


def test_mutation_queries_c_and_c_plus_16_swapped(world):
    w = world["words"].copy()
    c = 5
    w[:, [c, c + 16]] = w[:, [c + 16, c]]
    bad, st = run(world, words=w, max_report=10_000)
    assert {v["query"] for v in bad} == {c, c + 16}, M.describe(bad, st)
    assert ("P1", "low") in names(bad) and ("P3", "high") in names(bad)


def test_mutation_words_written_one_tile_late(world):
    w = world["words"].copy()
    lo, hi = 32, 48                              # the 32-row tiles of one wave's run
    w[lo + 1:hi] = world["words"][lo:hi - 1]
    bad, st = run(world, words=w, max_report=10_000)
    assert bad and {v["tile"] for v in bad} <= set(range(lo + 1, hi)), M.describe(bad, st)
    assert ("P1", "low") in names(bad) and len({v["tile"] for v in bad}) == hi - lo - 1


def test_mutation_a_row_past_the_end_counted(world):
    # what the scans' loads deliver for rows >= n_rows: the matrix's last row again (the addresses are clamped)
    T = world["words"].shape[0]
    a_pad = np.concatenate([world["a"], np.repeat(world["a"][-1:], T * 32 - N_ROWS, axis=0)])
    m8_bad, _ = M.reference_m8(a_pad, world["q"], T)
    w = M.encode_words(m8_bad.astype(np.float32), world["eps"])
    bad, st = run(world, words=w, max_report=10_000)
    last = (N_ROWS - 1) // 32
    assert ("P6", "high") in names(bad) and names(bad) <= {("P6", "high"), ("P3", "high")}, M.describe(bad, st)
    assert {v["tile"] for v in bad} <= {last, last + 1} and any(v["tile"] == last and v["query"] == 3 and v["sub"] in (1, 2, 3) for v in bad)
    assert any(v["tile"] == last + 1 and v["sub"] is None for v in bad)          # a tile without real rows has a maximum


def test_mutation_a_word_left_at_the_sentinel(world):
    w = world["words"].copy()
    w[17, 9] = SENTINEL
    bad, st = run(world, words=w)
    assert [(v["prop"], v["direction"], v["tile"], v["query"]) for v in bad] == [("P6", "sentinel", 17, 9)], M.describe(bad, st)
    ok = np.zeros(w.shape, dtype=bool)
    ok[17, 9] = True
    bad, st = run(world, words=w, may_skip=ok)           # a word the store prefilter may skip
    assert not bad and st["sentinel_words"] == 1
    w[17, 9] = 0x00007FC0                                 # a NaN maximum that is not the sentinel
    bad, st = run(world, words=w)
    assert [(v["prop"], v["direction"]) for v in bad] == [("P6", "nan")]


def test_group_keys_are_checked(world):
    k = world["keys"].copy()
    k[2, 4] -= 20000                               # a group maximum below its tiles'
    k[3, 6] += 20000                               # ... and above
    k[-1, 0] = M.f2key(np.array([0.5], dtype=np.float32))[0]          # the last wave's run is short: its last groups hold no tile
    k[0, 1] = 0xFFC00001
    assert M.group_tiles(world["geom"], len(k) - 1) == (0, 0)
    bad, st = run(world, keys=k)
    got = {(v["prop"], v["direction"], v["tile"], v["query"]) for v in bad}
    assert got == {("P5", "low", 2, 4), ("P5", "high", 3, 6), ("P5", "high", len(k) - 1, 0), ("P5", "nan", 0, 1)}, M.describe(bad, st)
