"""A CPU model of the batch tail's last two launches (csrc/rr_dense_flt.hip: rr_rescore_chain; csrc/rr_dense.hip:
rr_select_rescored), plain numpy, and the inputs tests/test_gpu_rescore_kernels.py runs them on.  Nothing here reads a
kernel's output: tests/test_rescore_model.py checks the model on the CPU, the GPU tests hold the kernels against it.

Arithmetic
    fma32           one float32 fused multiply-add: the float64 product of two float32 is exact (48 bits), the float64 sum
                    p + c is rounded once and its TwoSum residual is exact.  Casting that sum to float32 rounds a second
                    time, which is wrong exactly where the float64 sum sits halfway between two float32 values and the
                    residual is not zero: the result must go to the neighbour on the residual's side.  The model makes
                    the float64 sum "sticky" first -- where the residual is not zero and the sum's last bit is even, it
                    moves one float64 step towards the residual (rounding to odd) -- and casts then: a halfway sum with a
                    residual is no longer halfway and lands on the residual's side, any other sum keeps its float32
                    neighbour (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums", 2008: 53 >= 24 + 2 bits).
    chain_f32       a 16-lane row of an fp32 matrix: lane j takes floats 4 (j + 16 i) .. + 3, i = 0..5, one chain of 24
                    fma32 in ascending order from 0
    chain_bf16      a 16-lane row of a bf16 matrix (or plane): lane j takes elements 8 (j + 16 i) .. + 7, i = 0..2
    row16_sum       the 16 partial sums in rr_row16_sum's order: partners xor 1, xor 2, xor 4, xor 8, float32 additions
Decisions
    rescore_expected    what ONE rr_rescore_chain launch leaves in sc, bit for bit (plane pre-scoring included)
    select_rescored     what ONE rr_select_rescored launch leaves for one query
"""
import os
import re

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "review-recommender_amd", "csrc")


def _define(name, fname):
    return int(re.search(r"#define\s+" + name + r"\s+\(?(-?(?:0x[0-9A-Fa-f]+|\d+))", open(os.path.join(_CSRC, fname)).read()).group(1), 0)


RR_X3_MCAP = _define("RR_X3_MCAP", "rr_dense.h")
RR_SEL_MAXQ = _define("RR_SEL_MAXQ", "rr_dense.h")
RR_SEL_RCAP = _define("RR_SEL_RCAP", "rr_dense.hip")
RR_SEL_CCAP = _define("RR_SEL_CCAP", "rr_dense.hip")
RR_SEL_THREADS = _define("RR_SEL_THREADS", "rr_dense.hip")
SC_SENTINEL = np.uint32(_define("RR_DEBUG_SC_SENTINEL", "rr_dense_flt.hip"))
ROW_SENTINEL = np.int64(_define("RR_DEBUG_ROW_SENTINEL", "rr_dense_flt.hip"))
NCAND_SENTINEL = np.int32(_define("RR_DEBUG_NCAND_SENTINEL", "rr_dense_flt.hip"))

U = 2.0 ** -24
GAMMA_28 = 28 * U / (1 - 28 * U)          # 24 chain steps + 4 additions of the row sum
NEG_INF_BITS = np.uint32(0xFF800000)


def rcap_of(pool):
    return RR_SEL_RCAP if pool <= 512 else RR_SEL_CCAP


# ------------------------------------------------------------------ arithmetic
def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, on float32 arrays (the module docstring says how)."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)            # exact
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)                            # TwoSum: s + e == p + c exactly (NaN where s is not finite)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where((e != 0) & (e == e) & even & np.isfinite(s), np.nextafter(s, toward), s)
        return s.astype(np.float32)


def row16_sum(p):
    """[..., 16] float32 partial sums -> [...] in rr_row16_sum's order."""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(4):                   # partners xor 1, then 2, 4, 8: neighbours of what is left
            p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def _chain(rows, q, per):
    # rows [n, 384] float32 (bf16 values widened for per = 8), q [384] float32; lane j: elements per (j + 16 i) .. + per - 1
    n = rows.shape[0]
    r = rows.reshape(n, 384 // (16 * per), 16, per)
    qq = np.asarray(q, dtype=np.float32).reshape(384 // (16 * per), 16, per)
    acc = np.zeros((n, 16), dtype=np.float32)
    for i in range(r.shape[1]):
        for k in range(per):
            acc = fma32(r[:, i, :, k], qq[i, :, k][None, :], acc)
    return acc


def chain_f32(rows, q):
    """Scores of fp32 rows [n, 384] against q [384]: rr_rescore_chain's exact chain (= rr_scan_f32<6, 1>)."""
    return row16_sum(_chain(np.ascontiguousarray(rows, dtype=np.float32), q, 4))


def chain_bf16(rows_bf16, q):
    """Scores of bf16 rows (float32 values that ARE bf16 values) [n, 384] against the fp32 q: the bf16 index's chain
    (= rr_scan_bf16<1>) and the plane pre-scoring of an fp32 index."""
    return row16_sum(_chain(np.ascontiguousarray(rows_bf16, dtype=np.float32), q, 8))


def round_to_bf16(x):
    """float32 -> nearest-even bf16, widened back (NaN stays NaN, whatever its payload)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = (((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r)


def f2key(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------ rr_rescore_chain
def pre_threshold(tau_key, eps):
    """pre_thr = key2f(tau) - 1.01f * eps in float32, one rounding per operation (-ffp-contract=off); NaN -> -inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = key2f(np.asarray(tau_key, dtype=np.uint32)) - np.float32(1.01) * np.asarray(eps, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    return np.where(np.isnan(t), np.float32(-np.inf), t).astype(np.float32)


def takes_exact_chain(est, tau_key, eps):
    """The plane pre-scoring decision of every row, from its plane score `est`."""
    with np.errstate(invalid="ignore"):
        return (est >= pre_threshold(tau_key, eps)) | np.isnan(est)


def row_scores(exact, est=None, tau_key=None, eps=None):
    """What the kernel stores for every row of the matrix: the exact chain where it runs (NaN -> -inf), -inf elsewhere."""
    out = np.where(np.isnan(exact), np.float32(-np.inf), exact).astype(np.float32)
    if est is not None:
        out = np.where(takes_exact_chain(est, tau_key, eps), out, np.float32(-np.inf)).astype(np.float32)
    return out


def rescore_expected(stored, n_rows, mtiles, count, fb, cap):
    """sc[nq][cap][8] as uint32 bit patterns after one launch.  stored[q][row]: row_scores of query q; mtiles [nq][cap]."""
    nq = len(count)
    out = np.full((nq, cap, 8), SC_SENTINEL, dtype=np.uint32)
    for q in range(nq):
        if fb[q]:
            continue
        n = int(count[q])
        rows = mtiles[q, :n].astype(np.int64)[:, None] * 8 + np.arange(8)[None, :]
        val = np.where(rows < n_rows, stored[q][np.minimum(rows, n_rows - 1)], np.float32(-np.inf)).astype(np.float32)
        out[q, :n] = val.view(np.uint32)
    return out


# ------------------------------------------------------------------ rr_select_rescored
def select_rescored(mtiles, count, fb, tau_key, sc, pool, rows_per_mtile, floor_mode, n_rows, row_offset):
    """One query of one launch.  mtiles [cap], sc [cap][rows_per_mtile] float32.  -> dict(fb, n_cand, rows, scores): rows /
    scores None where the kernel writes none (the outputs keep their sentinels), n_cand None where it writes no trace."""
    if fb:
        return dict(fb=1, n_cand=None, rows=None, scores=None)
    half = rcap_of(pool) // 2
    n1 = int(count) * rows_per_mtile
    rows = (mtiles[:count].astype(np.uint32)[:, None] * np.uint32(rows_per_mtile) + np.arange(rows_per_mtile, dtype=np.uint32)[None, :]).ravel()
    keys = f2key(np.asarray(sc, dtype=np.float32)[:count].ravel())
    live = rows.astype(np.int64) < n_rows
    all_rows = bool(floor_mode) and n1 <= half
    pick = np.zeros(n1, dtype=bool) if all_rows else live & (keys >= np.uint32(tau_key))
    if all_rows or (floor_mode and pick.sum() < pool and n1 <= half):
        pick = live                               # under a corpus-wide floor: the best of ALL rescored rows, when they fit
    n_cand = int(pick.sum())
    if n_cand > half or n_cand < pool:
        return dict(fb=1, n_cand=n_cand, rows=None, scores=None)
    k64 = (keys[pick].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rows[pick].astype(np.uint64))
    top = np.sort(k64)[::-1][:pool]               # key descending, then row ascending
    out_rows = (np.uint64(0xFFFFFFFF) - (top & np.uint64(0xFFFFFFFF))).astype(np.int64) + row_offset
    return dict(fb=0, n_cand=n_cand, rows=out_rows, scores=key2f((top >> np.uint64(32)).astype(np.uint32)))


# ------------------------------------------------------------------ inputs of tests/test_gpu_rescore_kernels.py
RESCORE_ROWS = 2043                  # 255 full 8-row M-tiles + one of 3 rows; <= 2048: one single-query search returns every row
RESCORE_TILES = (RESCORE_ROWS + 7) // 8
RAGGED = RESCORE_TILES - 1
ZERO_ROW, TWIN_ROWS, NAN_ROW, INF_ROW, QUERY_ROW = 77, (500, 1501), 300, 1300, 1700
RESCORE_COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 256, 257, 600)
RESCORE_NQ = 5                       # query 4 enters with fb = 1
POOL = 150


def rescore_matrix(special=False):
    """[2043, 384] float32: rows 0..1023 unit, rows 1024.. of norm 0.01 .. 30 (log-uniform), an all-zero row, two identical
    rows; special: also one row with a NaN element and one with an inf element."""
    rng = np.random.default_rng(2043)
    m = rng.standard_normal((RESCORE_ROWS, 384)).astype(np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True).astype(np.float32)
    m[1024:] *= np.exp(rng.uniform(np.log(0.01), np.log(30.0), (RESCORE_ROWS - 1024, 1))).astype(np.float32)
    m[ZERO_ROW] = 0
    m[TWIN_ROWS[1]] = m[TWIN_ROWS[0]]
    if special:
        m[NAN_ROW, 5] = np.nan
        m[INF_ROW, 200] = np.inf
        m[INF_ROW + 1, 201] = -np.inf
    return np.ascontiguousarray(m)


def rescore_queries():
    """[5, 384] float32 of norm 7.5; query 1 is a scaled row."""
    rng = np.random.default_rng(75)
    q = rng.standard_normal((RESCORE_NQ, 384)).astype(np.float32)
    q[1] = rescore_matrix()[QUERY_ROW]
    q *= (7.5 / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(q)


def rescore_lists(c):
    """mtiles [5][max(c, 1)], count [5], fb [5] of the launch with `c` listed M-tiles: a permutation of the matrix's M-tiles
    (past 256: repeats) with the ragged M-tile first (query 0), in the middle (1), last (2), and as the repeated padding (3,
    which lists two fewer); query 4 enters flagged."""
    cap = max(c, 1)
    mt = np.zeros((RESCORE_NQ, cap), dtype=np.uint32)
    count = np.full(RESCORE_NQ, c, dtype=np.int32)
    count[3] = max(c - 2, 0)
    fb = np.zeros(RESCORE_NQ, dtype=np.int32)
    fb[4] = 1
    for q in range(RESCORE_NQ):
        rng = np.random.default_rng(1000 * c + q)
        perm = rng.permutation(RESCORE_TILES - 1).astype(np.uint32)           # (without the ragged one)
        lst = np.concatenate([perm, rng.integers(0, RESCORE_TILES - 1, max(c - len(perm), 0)).astype(np.uint32)])[:c]
        if c:
            at = {0: 0, 1: c // 2, 2: c - 1}.get(q)
            if at is not None:
                lst[at] = RAGGED
            elif q == 3:
                lst[max(c - 2, 1) // 3] = RAGGED
                lst[RESCORE_TILES - 1:] = RAGGED                                 # the padding of the long lists repeats it
        mt[q, :c] = lst
    return mt, count, fb


def filter_eps(V, q):
    """The float64 bound of tests/test_filter_bound.py::_eps (max ||a - a~|| ||q~|| + max ||a|| ||q - q~||) times 1.01."""
    Vr, qr = round_to_bf16(V).astype(np.float64), round_to_bf16(q[None, :])[0].astype(np.float64)
    V64, q64 = V.astype(np.float64), q.astype(np.float64)
    return 1.01 * (np.linalg.norm(V64 - Vr, axis=1).max() * np.linalg.norm(qr) + np.linalg.norm(V64, axis=1).max() * np.linalg.norm(q64 - qr))


def split_cut(exact_q, V, q):
    """tau (key) and eps (float32) of the splitting case of one query: the key of the 150th largest exact score, the filter
    bound."""
    s = np.sort(np.where(np.isnan(exact_q), np.float32(-np.inf), exact_q))[::-1]
    return np.uint32(f2key(s[POOL - 1:POOL])[0]), np.float32(filter_eps(V, q))


# ---- selection: synthetic scores on an index of 8189 zero rows, row_offset 1000
SELECT_ROWS, SELECT_OFFSET = 8189, 1000


def selection_case(name, pool, rpm, floor_mode, n_cand, count=None, levels=None, cut=1.0, fb=0, expect_flag=False):
    return dict(name=name, pool=pool, rpm=rpm, floor_mode=floor_mode, n_cand=n_cand, count=count, levels=levels, cut=cut, fb=fb,
                expect_flag=expect_flag)


def selection_cases():
    c = selection_case
    out = []
    for pool, counts in ((150, (149, 150, 151, 1023, 1024, 1025, 1500, 4096, 4097)), (1, (0, 1, 2, 1024, 1025, 4096, 4097)),
                         (512, (511, 512, 513, 1023, 1024, 1025, 1500, 4096, 4097)),
                         (513, (512, 513, 514, 1023, 1024, 1025, 1500, 6144, 6145)), (2048, (2047, 2048, 2049, 6144, 6145))):
        half = rcap_of(pool) // 2
        for n in counts:
            out.append(c(f"n_cand={n}", pool, 8, 0, n, expect_flag=n < pool or n > half))
    out += [c("one run of equal keys", 150, 8, 0, 1500, levels=1), c("cut at +0.0 over -0.0", 150, 8, 0, 1100, cut=0.0),
            c("two levels", 512, 8, 0, 3000, levels=2), c("enters flagged", 150, 8, 0, 1500, fb=1),
            c("enters flagged, too few", 512, 8, 0, 100, fb=1)]
    for pool, counts in ((150, (149, 150, 1024, 1025, 4096, 4097)), (2048, (2047, 2048, 6144, 6145))):
        half = rcap_of(pool) // 2
        for n in counts:
            out.append(c(f"n_cand={n}", pool, 16, 0, n, expect_flag=n < pool or n > half))
    out.append(c("cut at +0.0 over -0.0", 150, 16, 0, 700, cut=0.0))
    # floor_mode = 1: n_cand is the count of rows at or above the cut; n1 = 8 count rows were rescored
    out += [c("floor: filled up", 150, 8, 1, 100, count=300), c("floor: filled up although enough reach the cut", 150, 8, 1, 400, count=512),
            c("floor: fewer than pool rows in all", 150, 8, 1, 20, count=18, expect_flag=True),
            c("floor: too many rescored rows to fill up", 150, 8, 1, 100, count=600, expect_flag=True),
            c("floor: too many rescored rows, enough at the cut", 150, 8, 1, 200, count=600),
            c("floor: one more row than fits", 150, 8, 1, 100, count=513, expect_flag=True)]
    return out


def selection_inputs(case, seed):
    """-> mtiles [cap], count, tau key, sc [cap][rpm] of one case: `count` distinct M-tiles in random order, the ragged last
    one among them; exactly case["n_cand"] of their real rows at or above the cut, on `levels` score levels (ties across
    tiles); below the cut -inf, -0.0 and negative scores; +inf in the rows past n_rows."""
    rng = np.random.default_rng(seed)
    rpm, n = case["rpm"], case["n_cand"]
    n_tiles = (SELECT_ROWS + rpm - 1) // rpm
    count = case["count"] if case["count"] is not None else n_tiles
    tiles = rng.permutation(n_tiles - 1)[:count - 1].astype(np.uint32)
    tiles = np.insert(tiles, int(rng.integers(0, count)), n_tiles - 1)       # the ragged one somewhere
    rows = (tiles.astype(np.int64)[:, None] * rpm + np.arange(rpm)[None, :]).ravel()
    live = np.nonzero(rows < SELECT_ROWS)[0]
    assert n <= len(live)
    cut = np.float32(case["cut"])
    below = np.array([-np.inf, -0.0, -1.0, -2.5e-3, np.nextafter(cut, np.float32(-np.inf)) if cut != 0 else -0.0], dtype=np.float32)
    sc = below[rng.integers(0, len(below), rows.size)]
    levels = case["levels"] or max(2, n // 20)
    step = np.float32(2.0 ** -10)
    sc[rng.permutation(live)[:n]] = (cut + step * rng.integers(0, levels, n).astype(np.float32)).astype(np.float32)
    sc[rows >= SELECT_ROWS] = np.inf
    return tiles, count, np.uint32(f2key(np.array([cut], dtype=np.float32))[0]), sc.reshape(count, rpm).astype(np.float32)


def selection_launches():
    """The cases grouped into launches: {(pool, rpm, floor_mode): [case, ...]}, one query per case."""
    out = {}
    for case in selection_cases():
        out.setdefault((case["pool"], case["rpm"], case["floor_mode"]), []).append(case)
    return out


def selection_launch_arrays(key, cases):
    """Host arrays of one launch: mtiles [nq][cap], count, fb, tau, sc [nq][cap][rpm]; slots past a query's count hold M-tile 0
    and +inf scores."""
    pool, rpm, floor_mode = key
    parts = [selection_inputs(case, 7919 * pool + 31 * rpm + 1000 * floor_mode + i) for i, case in enumerate(cases)]
    cap = max(p[1] for p in parts) + 1                                           # (one slot past every count)
    nq = len(cases)
    mt = np.zeros((nq, cap), dtype=np.uint32)
    sc = np.full((nq, cap, rpm), np.inf, dtype=np.float32)
    count = np.array([p[1] for p in parts], dtype=np.int32)
    tau = np.array([p[2] for p in parts], dtype=np.uint32)
    fb = np.array([case["fb"] for case in cases], dtype=np.int32)
    for i, (tiles, n, _, s) in enumerate(parts):
        mt[i, :n], sc[i, :n] = tiles, s
    return mt, count, fb, tau, sc
