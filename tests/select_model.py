"""A CPU model of the three kernels of csrc/rr_dense.hip that turn a scan's output into an answer -- rr_select, rr_group_kth,
rr_select_mtiles -- plain numpy, and the inputs tests/test_gpu_select_kernels.py runs them on.  Nothing here reads a kernel's
output: tests/test_select_model.py checks the model and the inputs on the CPU, the GPU tests hold the kernels against it.

None of the three kernels reads a matrix.  They read LEVELS: the score of every row, the maximum of every 64-row tile (or
of every 16-row M-tile) and the ordered key of the maximum of every wave's run of tiles (a "group").  levels() /
mtile_levels() build them for any geometry as a scan leaves them; the expected answer is exact -- integer keys, ordered
by (key descending, row ascending).

    levels              scores, tile maxima and group keys of `nq` queries, plain and in the two device layouts
    kth_largest_reg     integer for integer what rr_kth_largest_reg returns
    select              the exact answer of ONE query + the trace rr_select must leave, stage by stage, + the door it takes
    group_kth           tau and the float64 value of the bound rr_group_kth writes
    select_mtiles       open / tau / flag / the listed set of ONE query of rr_select_mtiles (mm_pairs 0 or 1)

Test inputs hold no NaN and no -0.0: the scans store neither (every chain starts from +0.0 and a NaN score is stored as
-inf), and the order is the KEY's, under which -0.0 < +0.0 -- so -0.0 is kept out and not modelled.
"""
import os
import re

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "review-recommender_amd", "csrc")


def _define(name, fname):
    return int(re.search(r"#define\s+" + name + r"\s+\(?(-?(?:0x[0-9A-Fa-f]+|\d+))", open(os.path.join(_CSRC, fname)).read()).group(1), 0)


RR_SEL_LCAP = _define("RR_SEL_LCAP", "rr_dense.hip")
RR_SEL_GCAP = _define("RR_SEL_GCAP", "rr_dense.hip")
RR_SEL_CCAP = _define("RR_SEL_CCAP", "rr_dense.hip")
RR_SEL_SORTCAP = _define("RR_SEL_SORTCAP", "rr_dense.hip")
RR_SEL_RK = _define("RR_SEL_RK", "rr_dense.hip")
RR_SEL_THREADS = _define("RR_SEL_THREADS", "rr_dense.hip")
RR_SEL_LISTED = _define("RR_SEL_LISTED", "rr_dense.h")
RR_X3_MCAP = _define("RR_X3_MCAP", "rr_dense.h")
RR_MAX_SCAN_WAVES = _define("RR_MAX_SCAN_WAVES", "rr_dense.h")
RR_MFMA_MAXQ = _define("RR_MFMA_MAXQ", "rr_dense.h")
RR_FLT_MAXQ = _define("RR_FLT_MAXQ", "rr_dense.h")
RR_SEL_MAXQ = _define("RR_SEL_MAXQ", "rr_dense.h")
ROW_SENTINEL = np.int64(_define("RR_DEBUG_SEL_ROW_SENTINEL", "rr_dense.hip"))
SCORE_SENTINEL = np.uint32(_define("RR_DEBUG_SEL_SCORE_SENTINEL", "rr_dense.hip"))
WORD_SENTINEL = np.int32(_define("RR_DEBUG_SEL_WORD_SENTINEL", "rr_dense.hip"))

STEPS = 7                                   # two-bit bisection steps every caller of rr_kth_largest_reg asks for
KEY_NEG_INF = 0x007FFFFF                    # rr_f2key(-inf): the smallest key a score has
NEG_INF_BITS = np.uint32(0xFF800000)
POOL = 150
BIG_OFFSET = 4_290_000_000                  # row_offset of the index whose answers pass 2^31
F32 = np.float32


def f2key(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _key1(f):
    return int(f2key(np.float32([f]))[0])


def _f1(k):
    return key2f(np.uint32([k]))[0]


# ------------------------------------------------------------------ levels
def levels(scores, n_rows, tiles_per_wave, qs=0):
    """scores [nq][n_rows] float32 (no NaN, no -0.0) -> the three levels as a scan leaves them.  Rows past the end are -inf; a
    group is one wave's run of `tiles_per_wave` tiles, the last run may be short.  Plain arrays per query: sims [nq][n_pad],
    gmax [nq][n_tiles], keys [nq][n_waves]; device() packs them in the layout rr_scan_geom::qs documents."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    assert scores.ndim == 2 and scores.shape[1] == n_rows and not np.isnan(scores).any()
    assert not ((scores == 0) & np.signbit(scores)).any(), "-0.0 is kept out of the inputs"
    nq = scores.shape[0]
    n_tiles = (n_rows + 63) // 64
    n_pad = 64 * n_tiles
    n_waves = (n_tiles + tiles_per_wave - 1) // tiles_per_wave
    sims = np.full((nq, n_pad), -np.inf, dtype=np.float32)
    sims[:, :n_rows] = scores
    gmax = sims.reshape(nq, n_tiles, 64).max(axis=2)
    padded = np.full((nq, n_waves * tiles_per_wave), -np.inf, dtype=np.float32)
    padded[:, :n_tiles] = gmax
    keys = f2key(padded.reshape(nq, n_waves, tiles_per_wave).max(axis=2)).reshape(nq, n_waves)
    return dict(n_rows=n_rows, n_tiles=n_tiles, n_pad=n_pad, n_waves=n_waves, tiles_per_wave=tiles_per_wave, qs=qs, nq=nq,
                sims=sims, gmax=gmax, keys=keys)


def device(L, slots=None):
    """The levels in the device layout: qs == 0 -> sims [slots][n_pad], gmax [slots][n_tiles], keys [slots][n_waves]; qs > 0 ->
    sims [n_pad / 16][qs][16], gmax [n_tiles][qs], keys [n_waves][qs].  Slots no query uses hold +inf everywhere (a kernel that
    read a neighbour's slot would return its rows)."""
    qs, nq = L["qs"], L["nq"]
    slots = (qs if qs else nq) if slots is None else slots
    assert nq <= slots and (qs == 0 or slots == qs)
    sims = np.full((slots, L["n_pad"]), np.inf, dtype=np.float32)
    gmax = np.full((slots, L["n_tiles"]), np.inf, dtype=np.float32)
    keys = np.full((slots, L["n_waves"]), _key1(np.inf), dtype=np.uint32)
    sims[:nq], gmax[:nq], keys[:nq] = L["sims"], L["gmax"], L["keys"]
    if qs == 0:
        return sims, gmax, keys
    return (np.ascontiguousarray(sims.reshape(slots, L["n_pad"] // 16, 16).transpose(1, 0, 2)), np.ascontiguousarray(gmax.T),
            np.ascontiguousarray(keys.T))


# ------------------------------------------------------------------ rr_kth_largest_reg
def kth_largest_reg(keys, k, max_steps=STEPS):
    """What rr_kth_largest_reg returns for these keys (uint32; 0 = padding): a lower bound of the k-th largest, resolved
    two bits per step from the highest bit in which the largest and the smallest NON-ZERO key differ (zeros join the
    spread only when fewer than k keys are non-zero)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32).astype(np.int64)
    mx = int(keys.max())
    nz = keys[keys != 0]
    mn = int(nz.min()) if len(nz) else 0xFFFFFFFF
    if len(nz) < k:
        mn = 0
    if mx == mn:
        return mx
    bit = (mx ^ mn).bit_length() - 1
    prefix = 0 if bit == 31 else (mx >> (bit + 1)) << (bit + 1)
    step = 0
    while bit >= 0 and step < max_steps:
        lo = bit - 1 if bit >= 1 else 0
        t1, t2, t3 = prefix | (1 << lo), prefix | (1 << bit), prefix | (1 << bit) | (1 << lo)
        s1, s2, s3 = (int((keys >= t).sum()) for t in (t1, t2, t3))
        if bit >= 1:
            if s3 >= k:
                prefix = t3
            elif s2 >= k:
                prefix = t2
            elif s1 >= k:
                prefix = t1
        elif s2 >= k:
            prefix = t2
        bit = lo - 1
        step += 1
    return prefix


def kth_largest_exact(keys, k):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    return int(np.partition(keys, len(keys) - k)[len(keys) - k])


# ------------------------------------------------------------------ rr_select
def exact_top(sims_q, n_rows, pool, row_offset=0):
    """rows (int64, + row_offset) and score bits of the top `pool` by (key descending, row ascending)."""
    k = f2key(sims_q[:n_rows]).astype(np.int64)
    order = np.lexsort((np.arange(n_rows), -k))[:pool]
    return order.astype(np.int64) + np.int64(row_offset), key2f(k[order].astype(np.uint32)).view(np.uint32)


def select(L, q, pool, row_offset=0, keys=None):
    """One query of one rr_select launch: the exact answer, trace words 0..3 (fast | groups opened | tiles opened | rows kept:
    counts keep counting past a cap, a stage after a failed one stays 0), words 11..13 of the debug build (sentinels on the fast
    path) and word 14 (1 rank sort, 2 bitonic sort; the sentinel on the slow path), the door it leaves the fast path through (None | "groups" | "tiles" | "rows" | "few"), the sort ("rank" |
    "bitonic") or the slow sub-branch ("listed" | "all": by overflow or because n_tiles <= pool) and whether step 3b ran.
    `keys`: other group keys than the levels' (stale keys: the only way to fewer than `pool` rows)."""
    n_rows, n_tiles, C = L["n_rows"], L["n_tiles"], L["tiles_per_wave"]
    gk = (L["keys"][q] if keys is None else np.ascontiguousarray(keys, dtype=np.uint32)).astype(np.int64)
    tk = f2key(L["gmax"][q]).astype(np.int64)
    rk = f2key(L["sims"][q]).astype(np.int64)
    ng = len(gk)
    assert ng <= RR_SEL_RK * RR_SEL_THREADS
    tau = kth_largest_reg(gk, pool) if ng > pool else 1
    tau = tau or 1
    c0 = int((gk >= tau).sum())
    c1 = c2 = 0
    door = sort = None
    if c0 > RR_SEL_LCAP:
        door = "groups"
    else:
        tiles = (np.flatnonzero(gk >= tau)[:, None] * C + np.arange(C)[None, :]).ravel()
        tiles = tiles[tiles < n_tiles]
        tiles = tiles[tk[tiles] >= tau]
        c1 = len(tiles)
        if c1 > RR_SEL_GCAP:
            door = "tiles"
        else:
            rows = (tiles[:, None] * 64 + np.arange(64)[None, :]).ravel()
            rows = rows[rows < n_rows]
            c2 = int((rk[rows] >= tau).sum())
            if c2 > RR_SEL_CCAP // 2:
                door = "rows"
            elif c2 < pool:
                door = "few"
            else:
                sort = "rank" if c2 <= RR_SEL_THREADS else "bitonic"
    out = dict(tau=tau, trace=[0 if door else 1, c0, c1, c2], door=door, sort=sort, sub=None, step3b=None,
               slow=[int(WORD_SENTINEL)] * 3, sort_word={None: int(WORD_SENTINEL), "rank": 1, "bitonic": 2}[sort])
    if door:
        tau_key, all_tiles = 0, n_tiles <= pool
        if not all_tiles:
            tau_key = int(np.partition(tk, n_tiles - pool)[n_tiles - pool])
            listed = np.flatnonzero(tk >= tau_key)
            all_tiles = len(listed) > RR_SEL_GCAP
        if all_tiles:
            listed = np.arange(n_tiles)
        rows = (listed[:, None] * 64 + np.arange(64)[None, :]).ravel()
        rows = rows[rows < n_rows]
        n_cand = int((rk[rows] >= tau_key).sum())
        out.update(sub="all" if all_tiles else "listed", step3b=n_cand > RR_SEL_SORTCAP,
                   slow=[len(listed), n_cand, int(n_cand > RR_SEL_SORTCAP)])
    out["rows"], out["bits"] = exact_top(L["sims"][q], n_rows, pool, row_offset)
    return out


# ------------------------------------------------------------------ rr_group_kth
def group_kth(keys, kth, eps):
    """keys [ng] of one query, eps float32 -> (tau or None, the float64 value of key2f(tau) - 1.01f * eps or -inf)."""
    ng = len(keys)
    if not (ng > kth and ng <= RR_SEL_RK * RR_SEL_THREADS):
        return None, -np.inf
    tau = kth_largest_reg(keys, kth)
    e = F32(eps)
    if tau > KEY_NEG_INF and e >= 0 and e < F32(3.0e38):
        return tau, float(_f1(tau)) - float(F32(1.01)) * float(e)
    return tau, -np.inf


# ------------------------------------------------------------------ rr_select_mtiles
def mtile_levels(mt, n_rows, tiles_per_wave, gpw, tiles_per_group, qs):
    """mt [nq][ceil(n_rows / 16)] float32: the maximum of every 16-row M-tile -> M-tile maxima [nq][4 n_tiles] (M-tiles past
    the end -inf) and group keys [nq][n_waves gpw]: group g = wave * gpw + k covers tiles k * tiles_per_group .. of the wave's
    run; a group without tiles (the short last run) has key 0."""
    mt = np.ascontiguousarray(mt, dtype=np.float32)
    nq = mt.shape[0]
    n_tiles = (n_rows + 63) // 64
    assert mt.shape[1] == (n_rows + 15) // 16 and gpw * tiles_per_group >= tiles_per_wave
    n_waves = (n_tiles + tiles_per_wave - 1) // tiles_per_wave
    mm = np.full((nq, 4 * n_tiles), -np.inf, dtype=np.float32)
    mm[:, :mt.shape[1]] = mt
    tmax = mm.reshape(nq, n_tiles, 4).max(axis=2)
    keys = np.zeros((nq, n_waves * gpw), dtype=np.uint32)
    group_tiles = []
    for g in range(n_waves * gpw):
        w, k = divmod(g, gpw)
        j = np.arange(tiles_per_group)
        in_run = k * tiles_per_group + j
        t = w * tiles_per_wave + in_run
        t = t[(in_run < tiles_per_wave) & (t < n_tiles)]
        group_tiles.append(t)
        if len(t):
            keys[:, g] = f2key(tmax[:, t].max(axis=1))
    return dict(n_rows=n_rows, n_tiles=n_tiles, n_waves=n_waves, tiles_per_wave=tiles_per_wave, gpw=gpw, tiles_per_group=tiles_per_group,
                qs=qs, nq=nq, mm=mm, keys=keys, group_tiles=group_tiles)


def mtile_device(L, mm_pairs):
    """mm_pairs 0: [tile][qs][4]; 1: [32-row tile][qs][2]; keys [group][qs].  Unused slots hold +inf."""
    qs, nq, n_tiles = L["qs"], L["nq"], L["n_tiles"]
    mm = np.full((qs, 4 * n_tiles), np.inf, dtype=np.float32)
    mm[:nq] = L["mm"]
    keys = np.full((qs, L["keys"].shape[1]), _key1(np.inf), dtype=np.uint32)
    keys[:nq] = L["keys"]
    if mm_pairs == 0:
        m = mm.reshape(qs, n_tiles, 4).transpose(1, 0, 2)
    else:
        m = mm.reshape(qs, 2 * n_tiles, 2).transpose(1, 0, 2)
    return np.ascontiguousarray(m), np.ascontiguousarray(keys.T)


def _sub32(key, factor, e):
    """rr_f2key(rr_key2f(key) - factor * e), float32 with one rounding per operation."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _key1(_f1(key) - F32(factor) * F32(e))


def select_mtiles(L, q, pool, eps=None, floor=None):
    """One query of one rr_select_mtiles launch (one set, no sigma): open, tau (keys), fb, count, the listed M-tiles (a set),
    trace words 1 and 2 (groups / M-tiles counted, past the caps too) and the branch ("small" | "no eps" | "own" | "floor" |
    "hot")."""
    gk = L["keys"][q].astype(np.int64)
    ng = len(gk)
    out = dict(open=1, tau=1, fb=1, count=0, listed=set(), c0=0, c1=0, branch="small")
    if not (ng <= RR_SEL_RK * RR_SEL_THREADS and ng > pool):
        return out
    e = None if eps is None else F32(eps)
    if e is not None and not (e >= 0 and e < F32(3.0e38)):
        out["branch"] = "no eps"
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        fl = F32(floor) - F32(1.05) * e if (floor is not None and e is not None) else F32(-np.inf)
    if fl > F32(-3.0e38):
        opn = _key1(fl) or 1
        c0 = int((gk >= opn).sum())
        tau = _key1(floor)
        branch = "floor"
        if c0 > RR_SEL_LCAP:
            branch = "hot"
            own = kth_largest_reg(gk, pool) or 1
            thr = max(_sub32(own, 2.05, e) or 1, opn)
            opn = thr
            c0 = int((gk >= thr).sum())
            tau = max(_sub32(own, 1.02, e), tau)
    else:
        branch = "own"
        own = kth_largest_reg(gk, pool) or 1
        if e is None:
            opn = tau = own
        else:
            opn = _sub32(own, 2.05, e) or 1
            tau = _sub32(own, 1.02, e)
        c0 = int((gk >= opn).sum())
    tau = tau or 1
    out.update(open=opn, tau=tau, c0=c0, branch=branch)
    if c0 > RR_SEL_LCAP:
        return out
    groups = np.flatnonzero(gk >= opn)
    tiles = np.concatenate([L["group_tiles"][g] for g in groups]) if len(groups) else np.zeros(0, dtype=np.int64)
    ids = (tiles[:, None] * 4 + np.arange(4)[None, :]).ravel()
    ids = ids[f2key(L["mm"][q][ids]).astype(np.int64) >= opn]
    out["c1"] = len(ids)
    if len(ids) > RR_X3_MCAP:
        return out
    out.update(fb=0, count=len(ids), listed=set(int(i) for i in ids))
    return out


# ------------------------------------------------------------------ inputs: rr_select
TOP = F32(0.9)              # the tied value: above every base score, so tau (within 2^-14 of the spread below it) still separates


def _base(n_rows, seed):
    return np.random.default_rng(seed).uniform(-1.0, 0.5, n_rows).astype(np.float32)


def tied_rows(n_tied, n_tiles_used, n_tiles, tile_step=1, n_rows=None):
    """n_tied rows spread round-robin over tiles 0, tile_step, 2 tile_step .. (n_tiles_used of them): row r of the tie sits in
    slot r // n_tiles_used of its tile."""
    i = np.arange(n_tied)
    rows = (i % n_tiles_used) * tile_step * 64 + i // n_tiles_used
    assert (i // n_tiles_used).max() < 64 and (n_tiles_used - 1) * tile_step < n_tiles and len(set(rows.tolist())) == n_tied
    return rows


def _tied_case(n_groups, tiles_per_wave, n_tied, n_tiles_used, tile_step=1, above=0, seed=1, n_rows=None):
    n_tiles = n_groups * tiles_per_wave
    n_rows = n_tiles * 64 if n_rows is None else n_rows
    s = _base(n_rows, seed)
    rows = tied_rows(n_tied, n_tiles_used, n_tiles, tile_step)
    s[rows] = TOP
    if above:                                    # distinct scores above the tie: the cut runs inside the tie
        s[rows[-above:]] = TOP + F32(0.01) * np.arange(1, above + 1, dtype=np.float32)
    return s


def select_cases():
    """name -> dict(scores [n_rows], n_rows, tiles_per_wave, pool, want): `want` is what the MODEL must say about the input (the
    door it is named after); tests/test_select_model.py asserts it on the CPU."""
    cases = {}

    def add(name, scores, tiles_per_wave, pool=POOL, keys=None, **want):
        cases[name] = dict(scores=np.ascontiguousarray(scores, dtype=np.float32), n_rows=len(scores), tiles_per_wave=tiles_per_wave,
                           pool=pool, keys=keys, want=want)

    rng = np.random.default_rng(7)
    for ng in (1000, 2000, 4000, 8000):          # one RK instance each (ng <= 1024, 2048, 4096, 8192); ragged last tile
        add(f"fast rank, {ng} groups", rng.standard_normal(ng * 64 - 37).astype(np.float32), 1, door=None, sort="rank")
    add("ng <= pool, 96 groups", rng.standard_normal(96 * 64).astype(np.float32), 1, door=None, sort="bitonic", tau=1, trace=[1, 96, 96, 6144])
    add("ng <= pool, 100 groups", rng.standard_normal(100 * 64).astype(np.float32), 1, door="rows", sub="all", step3b=False, tau=1,
        trace=[0, 100, 100, 6400])
    add("n_cand 1024: the last rank sort", _tied_case(1000, 1, 1024, 500), 1, door=None, sort="rank", trace=[1, 500, 500, 1024])
    for n in (1025, 3000, 6144):
        add(f"fast bitonic, n_cand {n}", _tied_case(1000, 1, n, 500), 1, door=None, sort="bitonic", trace=[1, 500, 500, n])
    add("door 3: n_cand 6145", _tied_case(1000, 1, 6145, 500), 1, door="rows", sub="listed", step3b=False, trace=[0, 500, 500, 6145],
        slow=[500, 6145, 0])
    add("4096 groups stay fast", _tied_case(8000, 1, 4096, 4096), 1, door=None, sort="bitonic", trace=[1, 4096, 4096, 4096])
    add("door 1: 4097 groups", _tied_case(8000, 1, 4097, 4097), 1, door="groups", sub="all", step3b=False, trace=[0, 4097, 0, 0],
        slow=[8000, 4097, 0])
    add("4096 tiles stay fast", _tied_case(4000, 2, 4096, 4096), 2, door=None, sort="bitonic", trace=[1, 2048, 4096, 4096])
    add("door 2: 4097 tiles", _tied_case(4000, 2, 4097, 4097), 2, door="tiles", sub="all", step3b=False, trace=[0, 2049, 4097, 0],
        slow=[8000, 4097, 0])
    for n in (7000, 8192):
        add(f"slow, listed tiles, n_cand {n}", _tied_case(1000, 1, n, 500), 1, door="rows", sub="listed", step3b=False, slow=[500, n, 0])
    add("slow, step 3b, n_cand 8193", _tied_case(1000, 1, 8193, 500), 1, door="rows", sub="listed", step3b=True, slow=[500, 8193, 1])
    add("slow, step 3b, 20000 tied at the cut", _tied_case(1000, 1, 20000, 500, above=50), 1, door="rows", sub="listed", step3b=True,
        slow=[500, 20000, 1])
    add("slow, all tiles by overflow", _tied_case(4000, 2, 5000, 5000), 2, door="tiles", sub="all", step3b=False, slow=[8000, 5000, 0])
    add("n_tiles <= pool: pool 2048 over 150 tiles", rng.standard_normal(9600).astype(np.float32), 1, pool=2048, door="rows", sub="all",
        step3b=True, tau=1, slow=[150, 9600, 1])
    # stale group keys (every group claims 0.99, no row has it): the only way to fewer than `pool` candidates
    add("door 4: fewer rows than pool", _base(64000, 3), 1, keys=np.full(1000, _key1(0.99), dtype=np.uint32), door="few", sub="listed",
        step3b=False, trace=[0, 1000, 0, 0])

    # ---- edges of the data
    n_rows = 64 * 999 + 17                       # the tie straddles the ragged end: its last 17 rows are the last 17 rows
    s = _base(n_rows, 11)
    s[np.concatenate([tied_rows(283, 283, 999), np.arange(64 * 999, n_rows)])] = TOP
    add("ragged last tile, tie across the end", s, 1, door=None, sort="rank", trace=[1, 284, 284, 300])
    n_rows = 64 * 1000 - 5                       # 1000 tiles in runs of 3: the last run holds one tile, and the tie is in it
    s = _base(n_rows, 12)
    s[np.concatenate([tied_rows(7000, 500, 1000), np.arange(64 * 999, n_rows)])] = TOP
    add("short last run, tie across the end", s, 3, door="rows", sub="listed", step3b=False, slow=[501, 7000 + 59, 0])
    s = rng.standard_normal(100).astype(np.float32)
    s[rng.permutation(100)[:40]] = -np.inf
    add("-inf rows, pool == n_rows == 100", s, 1, pool=100, door=None, sort="rank", tau=1, trace=[1, 2, 2, 100])
    s = rng.standard_normal(2000).astype(np.float32)
    s[rng.permutation(2000)[:700]] = -np.inf
    add("-inf rows, pool == n_rows == 2000", s, 1, pool=2000, door=None, sort="bitonic", tau=1, trace=[1, 32, 32, 2000])
    s = rng.standard_normal(64000).astype(np.float32)
    s[rng.permutation(64000)[:5]] = np.inf
    add("+inf scores, five rows", s, 1, door=None, sort="rank")
    add("+inf scores, 7000 rows tied", np.where(_tied_case(1000, 1, 7000, 500) == TOP, F32(np.inf), _base(64000, 1)), 1, door="rows",
        sub="listed", step3b=False, slow=[500, 7000, 0])
    for pool in (1, 256, 257, 2048):
        add(f"pool {pool}", rng.standard_normal(4000 * 64 - 1).astype(np.float32), 1, pool=pool, door=None,
            sort="rank" if pool < 1000 else "bitonic")
    return cases


# which cases share one launch: name of the launch -> (qs, names); all of a launch have one geometry and one pool
def select_launches():
    c = select_cases()
    launches = {name: (0, [name]) for name in c}
    # several queries per launch, each on a different door, in every layout
    launches["doors, qs 0"] = (0, ["fast bitonic, n_cand 3000", "door 3: n_cand 6145", "n_cand 1024: the last rank sort",
                                   "slow, step 3b, n_cand 8193", "slow, listed tiles, n_cand 7000"])
    for qs in (16, 32, 64):
        launches[f"doors, qs {qs}"] = (qs, launches["doors, qs 0"][1])
    launches["doors at 8000 groups, qs 16"] = (16, ["4096 groups stay fast", "door 1: 4097 groups"])
    launches["doors at 8000 tiles, qs 0"] = (0, ["4096 tiles stay fast", "door 2: 4097 tiles", "slow, all tiles by overflow"])
    return launches


def launch_levels(names, qs, cases=None):
    c = select_cases() if cases is None else cases
    geo = {(c[n]["n_rows"], c[n]["tiles_per_wave"], c[n]["pool"]) for n in names}
    assert len(geo) == 1, geo
    n_rows, tpw, pool = geo.pop()
    L = levels(np.stack([c[n]["scores"] for n in names]), n_rows, tpw, qs)
    for i, n in enumerate(names):
        if c[n]["keys"] is not None:
            L["keys"][i] = c[n]["keys"]
    return L, pool


# ------------------------------------------------------------------ inputs: rr_group_kth
def kth_key_sets():
    """name -> (keys [ng] uint32, k): random and adversarial sets for kth_largest_reg, and the sets rr_group_kth runs on."""
    rng = np.random.default_rng(21)
    sets = {}
    for ng in (300, 1024, 1025, 2048, 3000, 4096, 5000, 8192):
        sets[f"random scores, {ng}"] = (f2key(rng.standard_normal(ng).astype(np.float32)), 38)
    sets["all equal"] = (np.full(2000, _key1(0.5), dtype=np.uint32), 38)
    two = np.full(2000, _key1(0.25), dtype=np.uint32)
    two[rng.permutation(2000)[:37]] = _key1(0.75)
    sets["two values, 37 high of k = 38"] = (two.copy(), 38)
    two[0] = _key1(0.75) if two[0] != _key1(0.75) else two[0]
    two[np.flatnonzero(two == _key1(0.25))[0]] = _key1(0.75)
    sets["two values, 38 high of k = 38"] = (two, 38)
    z = f2key(rng.uniform(0.2, 0.9, 1500).astype(np.float32))
    z[rng.permutation(1500)[:1470]] = 0
    sets["30 non-zero keys of k = 38 (padding)"] = (z, 38)
    z = f2key(rng.uniform(0.2, 0.9, 1500).astype(np.float32))
    z[rng.permutation(1500)[:1000]] = 0
    sets["500 non-zero keys, 1000 padding"] = (z, 38)
    sets["spread in bit 31"] = (f2key(np.concatenate([rng.uniform(-1, -0.1, 600), rng.uniform(0.1, 1, 600)]).astype(np.float32)), 38)
    sets["spread in bit 31, k-th below zero"] = (f2key(np.concatenate([rng.uniform(-1, -0.1, 1190), rng.uniform(0.1, 1, 10)]).astype(np.float32)), 38)
    sets["-inf and finite"] = (f2key(np.concatenate([np.full(1000, -np.inf), rng.uniform(0.1, 1, 20)]).astype(np.float32)), 38)
    sets["k = 1"] = (f2key(rng.standard_normal(700).astype(np.float32)), 1)
    sets["k = ng - 1"] = (f2key(rng.standard_normal(700).astype(np.float32)), 699)
    return sets


# ------------------------------------------------------------------ inputs: rr_select_mtiles
MT_POOL = 150
MT_GAP = 8                  # keys every group key and M-tile maximum keeps away from the model's `open` when eps is given


def mtile_scores(n_rows, seed, n_hot=0, hot=0.9):
    """M-tile maxima: a base in (-0.5, 0.5), `n_hot` M-tiles (one per 64-row tile, tiles 0 ..) at `hot`."""
    n_mt = (n_rows + 15) // 16
    s = np.random.default_rng(seed).uniform(-0.5, 0.5, n_mt).astype(np.float32)
    s[4 * np.arange(n_hot) + 1] = F32(hot) + F32(1e-4) * np.random.default_rng(seed + 1).uniform(0, 1, n_hot).astype(np.float32)
    return s


def keep_gap(L, q, opn, gap=MT_GAP):
    """Moves every M-tile maximum of query q that lies within `gap` keys of `opn` away from it (up), then rebuilds the levels;
    returns the new levels.  (The threshold arithmetic may differ from the model by 2 keys: the listed sets stay exact.)"""
    mm = L["mm"].copy()
    k = f2key(mm[q]).astype(np.int64)
    near = np.abs(k - opn) < gap
    mm[q][near] = key2f((k[near] + 2 * gap).astype(np.uint32))
    n_mt = (L["n_rows"] + 15) // 16
    return mtile_levels(mm[:, :n_mt], L["n_rows"], L["tiles_per_wave"], L["gpw"], L["tiles_per_group"], L["qs"])


def gap_ok(L, q, opn, gap=MT_GAP):
    k = np.concatenate([f2key(L["mm"][q]).astype(np.int64), L["keys"][q].astype(np.int64)])
    return bool((np.abs(k - opn) >= gap).all())


def _plant(n_rows, seed, tiles, value, jitter=0.0, per_tile=1, base=(-0.5, 0.5)):
    """M-tile maxima [ceil(n_rows / 16)]: a uniform base, and in each of `tiles` (64-row tiles) `per_tile` M-tiles at `value`
    (+ a uniform jitter in [0, jitter))."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(base[0], base[1], (n_rows + 15) // 16).astype(np.float32)
    ids = (np.asarray(tiles)[:, None] * 4 + np.arange(per_tile)[None, :]).ravel()
    s[ids] = F32(value) + (rng.uniform(0, jitter, len(ids)).astype(np.float32) if jitter else F32(0))
    return s


def mtile_cases():
    """name -> dict(L, pool, eps [nq] | None, floor [nq] | None, want [nq] of dict(branch, fb, ...)): one launch each (run with
    mm_pairs 0 and 1).  With eps every key keeps MT_GAP keys from the model's `open` (gap_ok, asserted on the CPU)."""
    cases = {}
    inf = np.inf

    def add(name, mt, n_rows, tpw, gpw, tpg, qs, eps=None, floor=None, want=(), pool=MT_POOL):
        L = mtile_levels(np.stack(mt), n_rows, tpw, gpw, tpg, qs)
        if eps is not None:
            for q in range(L["nq"]):
                for _ in range(3):
                    L = keep_gap(L, q, select_mtiles(L, q, pool, eps[q], None if floor is None else floor[q])["open"])
        cases[name] = dict(L=L, pool=pool, eps=None if eps is None else np.asarray(eps, dtype=np.float32),
                           floor=None if floor is None else np.asarray(floor, dtype=np.float32), want=list(want))

    # ---- without eps: the split-operand use.  3000 tiles (the last one ragged) in runs of 3, two groups per run (2 + 1 tiles)
    n = 3000 * 64 - 20
    rng = np.random.default_rng(31)
    inf_q = _plant(n, 3, np.arange(0, 3000, 17), inf)
    add("no eps", [rng.standard_normal((n + 15) // 16).astype(np.float32), _plant(n, 2, np.arange(200) * 3, 0.9, 1e-3, 2), inf_q], n, 3, 2, 2, 16,
        want=[dict(branch="own", fb=0)] * 3)
    add("no eps, 150 groups = pool", [_plant(150 * 64, 4, np.arange(20), 0.9)], 150 * 64, 1, 1, 1, 16, want=[dict(branch="small", fb=1)])
    add("no eps, 151 groups", [_plant(151 * 64, 4, np.arange(20), 0.9)], 151 * 64, 1, 1, 1, 16, want=[dict(branch="own", fb=0)])
    n = 8000 * 64
    add("no eps, 4096 / 4097 groups reach tau", [_plant(n, 5, np.arange(4096), 0.9), _plant(n, 5, np.arange(4097), 0.9)], n, 1, 1, 1, 16,
        want=[dict(branch="own", fb=0, c0=4096, count=4096), dict(branch="own", fb=1, c0=4097, count=0)])
    a = _plant(n, 6, np.arange(4096), 0.9, 0, 4)
    b = a.copy()
    b[4 * 4096] = F32(0.9)
    add("no eps, 16384 / 16385 M-tiles reach tau", [a, b], n, 2, 1, 2, 32,
        want=[dict(branch="own", fb=0, c0=2048, c1=RR_X3_MCAP, count=RR_X3_MCAP), dict(branch="own", fb=1, c0=2049, c1=RR_X3_MCAP + 1, count=0)])

    # ---- with eps, no floor
    n = 3000 * 64 - 20
    mts = [rng.standard_normal((n + 15) // 16).astype(np.float32) * F32(0.3), _plant(n, 8, np.arange(200) * 3, 0.9, 2e-2, 2)]
    add("eps, no floor", mts + [mts[0], mts[0], mts[0], mts[0]], n, 3, 2, 2, 16, eps=[0.01, 0.005, np.nan, -1.0, inf, 3.0e38],
        want=[dict(branch="own", fb=0)] * 2 + [dict(branch="no eps", fb=1)] * 4)

    # ---- with a floor
    add("floor", [mts[1], mts[1], mts[1], mts[0]], n, 3, 2, 2, 16, eps=[0.01, 0.01, np.nan, 0.01], floor=[0.6, -inf, 0.6, -0.05],
        want=[dict(branch="floor", fb=0, tau=_key1(0.6)), dict(branch="own", fb=0), dict(branch="no eps", fb=1),
              dict(branch="floor", fb=0, tau=_key1(-0.05))])
    # hot shards: 8000 groups of one tile; more than 4096 reach the floor's `open`
    n, e = 8000 * 64, 0.01
    spread = _plant(n, 9, np.arange(5000), 0.5, 0.4)                    # own threshold far above the floor: its tau wins
    probe = mtile_levels(np.stack([_plant(n, 10, np.arange(160), 0.9, 0.01)]), n, 1, 1, 1, 16)
    own = _f1(kth_largest_reg(probe["keys"][0], MT_POOL))
    band = _plant(n, 10, np.arange(160), 0.9, 0.01)                     # same seed: the same base and the same 160 hot tiles
    band[4 * np.arange(160, 4660)] = own - F32(2.055 * e)                # 4500 groups between the floor's `open` and the shard's own
    fl = own - F32(1.01 * e)                                            # above the shard's own row cut: the floor's tau wins
    add("hot shard", [spread, band, spread], n, 1, 1, 1, 16, eps=[0.001, e, 0.001], floor=[0.3, fl, -0.49],
        want=[dict(branch="hot", fb=0, tau_is="own"), dict(branch="hot", fb=0, tau=_key1(fl), c0=160), dict(branch="hot", fb=0, tau_is="own")])
    return cases


# ------------------------------------------------------------------ inputs: rr_group_kth
def group_kth_cases():
    """name -> dict(n_waves, gpw, qs, kth, nq_a, nq_b, keys [sets][ng][qs], eps [RR_SEL_MAXQ], per [nq] of (set, slot),
    want [nq] of "-inf" | "value")."""
    rng = np.random.default_rng(41)
    cases = {}

    def add(name, n_waves, gpw, qs, kth, sets, want):
        # sets: per set a list of (keys [ng], eps)
        ng = n_waves * gpw
        keys = np.full((len(sets), ng, qs), _key1(np.inf), dtype=np.uint32)
        eps = np.zeros(RR_SEL_MAXQ, dtype=np.float32)
        per = []
        for s, qq in enumerate(sets):
            for i, (k, e) in enumerate(qq):
                assert len(k) == ng
                keys[s, :, i] = k
                eps[RR_FLT_MAXQ * s + i] = e
                per.append((s, i))
        cases[name] = dict(n_waves=n_waves, gpw=gpw, qs=qs, kth=kth, nq_a=len(sets[0]), nq_b=len(sets[1]) if len(sets) > 1 else 0, keys=keys,
                           eps=eps, per=per, want=list(want))

    sc = lambda ng, lo=-1.0, hi=1.0: f2key(rng.uniform(lo, hi, ng).astype(np.float32))
    k300 = sc(300)
    add("RK 1, eps edges", 100, 3, 16, 38,
        [[(k300, 0.01), (np.full(300, KEY_NEG_INF, dtype=np.uint32), 0.01), (k300, np.nan), (k300, -0.5), (k300, np.inf), (k300, 3.0e38),
          (k300, 0.0), (sc(300, 0.5, 0.5001), 0.25), (np.where(np.arange(300) < 290, KEY_NEG_INF, k300).astype(np.uint32), 0.01)]], 
        ["value", "-inf", "-inf", "-inf", "-inf", "-inf", "value", "value", "-inf"])
    z_few, z_many, z_most = sc(1500, 0.1, 0.9), sc(1500, 0.1, 0.9), sc(1500, 0.1, 0.9)
    z_few[rng.permutation(1500)[:10]] = 0
    z_many[rng.permutation(1500)[:1000]] = 0
    z_most[rng.permutation(1500)[:1470]] = 0
    add("RK 2, padding keys", 500, 3, 32, 38, [[(z_few, 0.01), (z_many, 0.01), (z_most, 0.01), (sc(1500), 0.02)]], ["value", "value", "-inf", "value"])
    add("RK 4, two sets", 3000, 1, 64, 38, [[(sc(3000), 0.01) for _ in range(5)], [(sc(3000), 0.03), (sc(3000), np.nan), (sc(3000, 0.2, 0.9), 0.5)]],
        ["value"] * 5 + ["value", "-inf", "value"])
    add("RK 8", 8192, 1, 16, 38, [[(sc(8192), 0.01), (sc(8192, -1e-3, 1e-3), 1e-5)]], ["value", "value"])
    add("kth 1", 300, 1, 16, 1, [[(k300, 0.01), (sc(300), 0.0)]], ["value", "value"])
    add("kth = ng - 1", 300, 1, 16, 299, [[(k300, 0.01), (sc(300), 0.0)]], ["value", "value"])
    add("ng = kth", 38, 1, 16, 38, [[(sc(38), 0.01)]], ["-inf"])
    add("ng = kth + 1", 39, 1, 16, 38, [[(sc(39), 0.01)]], ["value"])
    return cases
