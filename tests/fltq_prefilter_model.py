"""numpy restatement of the two-set filter scan's own store prefilter (csrc/rr_dense_flt.hip: rr_flt_launch_fltq_prefiltered,
rr_fltq_sigma, the masks of rr_scan_fltq) -- a library for test_fltq_prefilter_model.py (no GPU) and
test_gpu_fltq_prefilter.py.  Words, keys and geometry are flt_words_model's.

    launch A   group 0 of every run, every word stored
    sigma      per query: key2f(m-th largest of the <= 256 first-group keys that are not 0) - 2.05 eps, in float32, with
               m = 16 + ceil(4 pool / gpw); fewer than m such keys or no finite eps: -inf; slots past the set's queries: +inf
    launch B   groups 1 .. gpw - 1: a line (one 32-row tile x 32 queries) is stored iff some query of it has its tile
               maximum >= its sigma (a NaN maximum counts as stored); bit j of mask[group][line] = tile j of the group stored
"""
import numpy as np

import flt_words_model as M

MASK_SENTINEL = 0xA5A5A5A5A5A5A5A5


def sigma_m(geom, pool):
    return 16 + -(-4 * pool // geom["gpw"])


def sigma_model(geom, keys, eps, nq, pool):
    """keys[group, 128] (uint32) and eps[128] (float32) of ONE set with nq queries -> sigma[128] float32, bit for bit."""
    m, gpw, runs = sigma_m(geom, pool), geom["gpw"], geom["n_waves"]
    out = np.full(128, np.inf, dtype=np.float32)
    first = keys[0:runs * gpw:gpw]                    # the first group of every run
    for q in range(nq):
        out[q] = -np.inf
        e = np.float32(eps[q])
        k = first[:, q]
        k = np.sort(k[k != 0])
        if runs > 256 or not (e >= 0 and e < np.float32(3.0e38)) or len(k) < m:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            out[q] = np.float32(M.key2f(k[-m:len(k) - m + 1])[0]) - np.float32(np.float32(2.05) * e)
    return out


def marked_lines(geom, masks, with_masks=True):
    """masks[group, 4] (uint64) of ONE set -> marked[32-row tile, 4 lines] (bool): group 0 of a run counts as fully marked,
    as rr_select_mtiles takes it; with_masks=False (no masks written): None."""
    if not with_masks:
        return None
    T = 2 * geom["n_tiles"]
    out = np.zeros((T, 4), dtype=bool)
    for gi in range(geom["n_waves"] * geom["gpw"]):
        lo, hi = M.group_tiles(geom, gi)
        if hi <= lo:
            continue
        if gi % geom["gpw"] == 0:
            out[lo:hi] = True
            continue
        assert hi - lo <= 64
        bits = (masks[gi][None, :] >> np.arange(hi - lo, dtype=np.uint64)[:, None]) & np.uint64(1)
        out[lo:hi] = bits.astype(bool)
    return out


def stored_model(geom, m32, sigma, nq):
    """Lines a scan without rounding would store: m32[32-row tile, query] (the scan's float32 tile maxima), sigma[128]
    -> stored[tile, 4 lines]; group 0 of a run: everything."""
    T = m32.shape[0]
    hit = np.zeros((T, 128), dtype=bool)
    with np.errstate(invalid="ignore"):
        hit[:, :nq] = ~(m32[:, :nq] < sigma[None, :nq])
    out = hit.reshape(T, 4, 32).any(axis=2)
    for r in range(geom["n_waves"]):
        lo, hi = M.group_tiles(geom, r * geom["gpw"])
        out[lo:hi] = True
    return out


def masks_from_stored(geom, stored):
    """stored[tile, 4 lines] -> masks[group, 4] uint64 as launch B writes them (group 0 and absent groups: the sentinel)."""
    ng = geom["n_waves"] * geom["gpw"]
    out = np.full((ng, 4), MASK_SENTINEL, dtype=np.uint64)
    for gi in range(ng):
        lo, hi = M.group_tiles(geom, gi)
        if hi <= lo or gi % geom["gpw"] == 0:
            continue
        w = (stored[lo:hi].astype(np.uint64) << np.arange(hi - lo, dtype=np.uint64)[:, None]).sum(axis=0, dtype=np.uint64)
        out[gi] = w
    return out


def check_lines(geom, words, marked, M8, delta, sigma, nq, sentinel):
    """What the masks promise about the words of ONE set.  words[tile, 128]; marked[tile, 4]; M8 / delta[tile, 4, nq].
    -> list of problems (str): a marked line holds a sentinel for a real query, an unmarked line holds anything but the
    sentinel, an unmarked line has a real query whose float64 tile maximum minus delta is above its sigma, group 0 is not
    fully marked.  (P1..P6 of the marked words: flt_words_model.check_words with may_skip = ~marked.)"""
    T = words.shape[0]
    problems = []
    line_of = np.repeat(marked, 32, axis=1)                       # [tile, 128]
    real = np.arange(128)[None, :] < nq
    bad = line_of & real & (words == np.uint32(sentinel))
    if bad.any():
        t, q = np.argwhere(bad)[0]
        problems.append(f"marked line, word still the sentinel: tile {t} query {q} ({int(bad.sum())} such)")
    bad = ~line_of & (words != np.uint32(sentinel))
    if bad.any():
        t, q = np.argwhere(bad)[0]
        problems.append(f"unmarked line, word {int(words[t, q]):#x} is not the sentinel: tile {t} query {q} ({int(bad.sum())} such)")
    low = (M8 - delta).max(axis=1)                                # [tile, nq]: what the tile maximum is at least
    with np.errstate(invalid="ignore"):
        above = ~line_of[:, :nq] & (low > sigma[None, :nq].astype(np.float64))
    if above.any():
        t, q = np.argwhere(above)[0]
        problems.append(f"unmarked line with a usable word: tile {t} query {q}: M32 - delta = {low[t, q]!r} > sigma = {sigma[q]!r} ({int(above.sum())} such)")
    for r in range(geom["n_waves"]):
        lo, hi = M.group_tiles(geom, r * geom["gpw"])
        if not marked[lo:hi].all():
            problems.append(f"group 0 of run {r} is not fully marked")
            break
    return problems


def fltq_geom(n_rows, runs=256, max_groups=8192):
    """rr_fltq_geom (one run per compute unit, up to 32 selection groups per run, an even number of 64-row tiles per group)."""
    n_tiles = (n_rows + 63) // 64
    tpw = -(-n_tiles // runs)
    n_waves = -(-n_tiles // tpw)
    gpw = min(32, max(1, max_groups // n_waves))
    gpw = min(gpw, tpw)
    tpg = -(-tpw // gpw)
    if tpg < 8 and n_waves * (-(-tpw // 8)) > 2048:
        tpg = 8
    tpg += tpg & 1
    gpw = -(-tpw // tpg)
    return {"n_rows": n_rows, "n_tiles": n_tiles, "tiles_per_wave": tpw, "n_waves": n_waves, "gpw": gpw, "tiles_per_group": tpg}


def pair_taken(geom, forced=False):
    """rr_fltq_prefilter_wanted, for a plain call (no shard exchange)."""
    return geom["gpw"] >= 2 and (forced or geom["n_rows"] >= 2_000_000)


def masks_fit(geom):
    return 2 * geom["tiles_per_group"] <= 64


def loop_iterations(geom, g0, g1):
    """Iterations of rr_scan_fltq's four-body loop per entry, for a full run of a launch over groups [g0, g1)."""
    cg2 = 2 * geom["tiles_per_group"]
    T = 2 * (min(g1 * geom["tiles_per_group"], geom["tiles_per_wave"]) - min(g0 * geom["tiles_per_group"], geom["tiles_per_wave"]))
    it, out = 0, []
    while it < T:
        n_it = 0
        if it >= 5 and (it & 3) == 1 and (cg2 & 3) == 0:
            flush = (it + cg2 - 1) // cg2 * cg2
            n_it = (min(flush + 1, T) - it) // 4
        if n_it > 0:
            out.append(n_it)
            it += 4 * n_it
        else:
            it += 1
    return out


def shapes(runs):
    """Row counts of test_gpu_fltq_prefilter.py from the number of runs R the device reports (the rule of the rr_scan_fltq
    tests: R k tiles of 64 rows): name -> n_rows."""
    return {"groups-of-4": runs * 18 * 64,                          # ~300 000 rows at R = 256: nine 4-M-tile groups per run
            "short-last-M-tile": runs * 18 * 64 - 27,
            "one-group-run": (runs - 1) * 18 * 64 + 2 * 64 - 27,    # the last run holds one group: launch B has nothing to do there
            "one-group-everywhere": runs * 2 * 64 - 27,             # gpw = 1: the product takes the single launch
            "fewer-tiles-than-runs": 64 * (runs // 3) + 5}
