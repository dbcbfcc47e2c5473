"""The numpy model of the two-set scan's own store prefilter (fltq_prefilter_model.py) against itself, and the inputs of
test_gpu_fltq_prefilter.py against the branches they are named for -- no GPU: the geometry rule replayed at 256 runs says
which shapes take the pair, which runs have one group, where the four-body loop is entered in launch B and where the
masks stop fitting; the adversarial layout flags its query in the model; a line the model stores or drops wrongly is named."""
import numpy as np
import pytest

import flt_words_model as M
import fltq_prefilter_model as F

R = 256
POOL = 150
SENTINEL = 0x5A5A7FC1
PLANTED_POOL = 48


def test_shapes_reach_the_branches_they_are_named_for():
    S = F.shapes(R)
    g = F.fltq_geom(S["groups-of-4"], R)
    assert 290_000 < g["n_rows"] < 310_000 and 2 * g["tiles_per_group"] == 4 and g["gpw"] >= 5 and g["n_waves"] == R
    assert F.pair_taken(g, forced=True) and not F.pair_taken(g) and F.masks_fit(g)
    # launch A (group 0: four M-tiles) runs on the C++ bodies alone, launch B enters the generated loop and leaves it at every group's end
    assert F.loop_iterations(g, 0, 1) == [] and set(F.loop_iterations(g, 1, g["gpw"])) == {1} and len(F.loop_iterations(g, 1, g["gpw"])) >= 4
    g = F.fltq_geom(S["short-last-M-tile"], R)
    assert g["n_rows"] % 64 == 64 - 27 and g["n_rows"] % 32 == 5 and g["n_waves"] == R and g["gpw"] >= 5
    g = F.fltq_geom(S["one-group-run"], R)
    last = g["n_tiles"] - (g["n_waves"] - 1) * g["tiles_per_wave"]
    assert g["n_waves"] == R and g["gpw"] >= 5 and 0 < last <= g["tiles_per_group"]         # the last run: group 0 only
    assert M.group_tiles(g, (R - 1) * g["gpw"] + 1) in ((0, 0), (2 * g["n_tiles"], 2 * g["n_tiles"])) or \
        M.group_tiles(g, (R - 1) * g["gpw"] + 1)[1] <= M.group_tiles(g, (R - 1) * g["gpw"] + 1)[0]
    g = F.fltq_geom(S["one-group-everywhere"], R)
    assert g["gpw"] == 1 and not F.pair_taken(g, forced=True)
    g = F.fltq_geom(S["fewer-tiles-than-runs"], R)
    assert g["n_waves"] < R and g["gpw"] == 1 and not F.pair_taken(g, forced=True)
    # the product's own switch-on size and the benchmark's: the pair with masks; masks stop fitting above ~16.8M rows
    g = F.fltq_geom(2_200_000, R)
    assert F.pair_taken(g) and F.masks_fit(g) and g["gpw"] >= 16
    g = F.fltq_geom(10_000_000, R)
    assert F.pair_taken(g) and F.masks_fit(g) and g["gpw"] == 31 and g["tiles_per_group"] == 20 and F.sigma_m(g, POOL) == 36
    assert F.masks_fit(F.fltq_geom(16_700_000, R)) and not F.masks_fit(F.fltq_geom(17_000_000, R))      # (mask off)
    assert F.pair_taken(F.fltq_geom(17_000_000, R))


@pytest.fixture(scope="module")
def world():
    # 64 runs of 16 tiles in groups of 2 (the model's geometry is a dict: any consistent one serves)
    rng = np.random.default_rng(5)
    runs, tpw, tpg = 64, 16, 2
    n = runs * tpw * 64 - 27
    geom = {"n_rows": n, "n_tiles": (n + 63) // 64, "tiles_per_wave": tpw, "n_waves": runs, "gpw": tpw // tpg, "tiles_per_group": tpg}
    a = rng.standard_normal((n, 384)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    nq = 40
    q = rng.standard_normal((nq, 384)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    # the adversarial layout: query 3's best rows all sit in first groups (group 0 of run r = its first two 64-row tiles)
    for i in range(120):
        row = (i % runs) * tpw * 64 + 5 + 9 * (i // runs)
        v = q[3] * (0.9 - 0.002 * i) + 0.3 * rng.standard_normal(384).astype(np.float32) / np.sqrt(384)
        a[row] = v / np.linalg.norm(v)
    ab, qb = M.bf16_rne(a), M.bf16_rne(q)
    T = 2 * geom["n_tiles"]
    M8, delta = M.reference_m8(ab, qb, T)
    eps = np.full(128, np.inf, dtype=np.float32)
    eps[:nq] = 0.004
    m8 = M8.astype(np.float32)
    words = np.full((T, 128), SENTINEL, dtype=np.uint32)
    words[:, :nq] = M.encode_words(m8, eps[:nq])
    ng = runs * geom["gpw"]
    keys = np.zeros((ng, 128), dtype=np.uint32)
    for gi in range(ng):
        lo, hi = M.group_tiles(geom, gi)
        keys[gi, :nq] = M.f2key(m8[lo:hi].max(axis=(0, 1)))
    return {"geom": geom, "nq": nq, "M8": M8, "delta": delta, "eps": eps, "m8": m8, "words": words, "keys": keys}


def test_sigma_rule_and_the_flagged_query(world):
    g, nq, pool = world["geom"], world["nq"], PLANTED_POOL
    m = F.sigma_m(g, pool)
    assert m == 16 + 24 and m < pool             # (what lets a query whose best rows all sit in first groups overshoot)
    sg = F.sigma_model(g, world["keys"], world["eps"], nq, pool)
    assert np.all(np.isposinf(sg[nq:])) and np.all(np.isfinite(sg[:nq]))
    first = M.key2f(world["keys"][0::g["gpw"], :nq])
    assert np.array_equal(sg[:nq], (np.sort(first, axis=0)[-m] - np.float32(2.05) * world["eps"][:nq]).astype(np.float32))
    # fewer real keys than m, a key of 0, no finite eps
    k = world["keys"].copy()
    k[g["gpw"] * (m - 1)::g["gpw"], 0] = 0
    e = world["eps"].copy()
    e[1] = np.inf
    sg2 = F.sigma_model(g, k, e, nq, pool)
    assert np.isneginf(sg2[0]) and np.isneginf(sg2[1]) and np.array_equal(sg2[2:nq], sg[2:nq])
    # the flagged query: its sigma sits above what the selection opens down to (the pool-th largest group maximum - 2.05 eps)
    gmax = M.key2f(world["keys"][:, :nq])
    open_f = np.sort(gmax, axis=0)[-pool] - 2.05 * world["eps"][:nq]
    flagged = sg[:nq] > open_f
    assert flagged[3] and flagged.sum() == 1, np.flatnonzero(flagged)


def test_model_lines_pass_and_wrong_lines_are_named(world):
    g, nq = world["geom"], world["nq"]
    sg = F.sigma_model(g, world["keys"], world["eps"], nq, PLANTED_POOL)
    m32 = np.full((world["m8"].shape[0], 128), -np.inf, dtype=np.float32)
    m32[:, :nq] = world["m8"].max(axis=1)
    stored = F.stored_model(g, m32, sg, nq)
    assert 0.02 < stored.mean() < 0.9
    masks = F.masks_from_stored(g, stored)
    marked = F.marked_lines(g, masks)
    assert np.array_equal(marked, stored) and F.marked_lines(g, masks, with_masks=False) is None
    w = np.where(np.repeat(stored, 32, axis=1), world["words"], np.uint32(SENTINEL))
    assert F.check_lines(g, w, marked, world["M8"], world["delta"], sg, nq, SENTINEL) == []
    bad, st = M.check_words(w[:, :nq], world["keys"][:, :nq], g, world["M8"], world["delta"], world["eps"][:nq], sentinel=SENTINEL,
                            may_skip=~np.repeat(marked, 32, axis=1)[:, :nq])
    assert not bad, M.describe(bad, st)
    # a dropped line that a query could use; a marked line that was not stored; a stale word in an unmarked line; group 0
    t, l = np.argwhere(stored & (np.arange(stored.shape[0])[:, None] % (2 * g["tiles_per_wave"]) >= 2 * g["tiles_per_group"]))[0]
    m2 = marked.copy(); m2[t, l] = False
    w2 = w.copy(); w2[t, 32 * l:32 * l + 32] = SENTINEL
    assert any("usable word" in p for p in F.check_lines(g, w2, m2, world["M8"], world["delta"], sg, nq, SENTINEL))
    assert any("still the sentinel" in p for p in F.check_lines(g, w2, marked, world["M8"], world["delta"], sg, nq, SENTINEL))
    t, l = np.argwhere(~stored)[0]
    w3 = w.copy(); w3[t, 32 * l] = 0x00007F80
    assert any("not the sentinel" in p for p in F.check_lines(g, w3, marked, world["M8"], world["delta"], sg, nq, SENTINEL))
    m4 = marked.copy(); m4[0, 1] = False
    assert any("group 0" in p for p in F.check_lines(g, w, m4, world["M8"], world["delta"], sg, nq, SENTINEL))
