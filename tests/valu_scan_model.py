"""CPU model of ONE VALU dense scan launch (csrc/rr_dense.hip: rr_scan_f32, rr_scan_f32_generic and their listed forms;
csrc/rr_dense_bf16.hip: rr_scan_bf16; csrc/rr_dense_bf16w.hip: rr_scan_bf16_generic and its listed form), plain numpy, and the
named inputs tests/test_gpu_valu_scan_kernels.py runs the kernels on.  Nothing here reads a kernel's output:
tests/test_valu_scan_model.py checks the model on the CPU, the GPU test holds the kernels against it.

Levels
    chain               the per-row fmaf chain of a storage dtype and width: rescore_model.chain_f32 / chain_bf16 at 384,
                        fltw_model.chain_w / fltw_bf16_model.chain_wb at any other width (at 384 they agree bit for bit)
    expected_levels     what a launch leaves: sims [NB][n_pad] (NaN and rows past n_rows are -inf; a slot past the call's queries
                        holds the zero query's scores), gmax [NB][n_tiles], smax [NB][n_waves] keys.  A maximum is taken BY KEY
                        (rr_f2key), so where a tile holds +0.0 and -0.0 and nothing above, the model says +0.0; mixed_zero marks
                        those tiles and runs, where the GPU test compares values and records which zero the kernel reported
    f64_bound           gamma_k sum |a_i q_i|, k = dim_pad / 16 + 4 (a lane chains dim_pad / 16 fmaf, the row sum adds four times),
                        u = 2^-24: at 384 rescore_model.GAMMA_28.  The gamma bound is the one of normal arithmetic; a product that
                        underflows is rounded to a multiple of 2^-149 instead, an ABSOLUTE error of at most 2^-150 per fmaf
                        (sums of denormals are exact), so dim_pad 2^-150 = 3.6e-43 at most is added: the rows planted to
                        underflow (special_rows) are held to the bound like every other row, none is left out
Lists
    flagged_list        rr_flagged_list: the first NB flagged queries; count 0 when MORE than NB flags are up
    flagged_slice       rr_flagged_slice: the flagged queries ranked [skip, skip + NB)
Geometry
    geom_of             n_tiles, n_pad, n_waves of n_rows rows in runs of tiles_per_wave tiles
    pick_tiles          from one probe of a grid (a matrix of t_probe tiles came back with runs of c_probe tiles): a tile count
                        at which EVERY grid that answers the probe that way gives runs of >= 3 tiles and a shorter last run
"""
import numpy as np

import fltw_bf16_model as FB
import fltw_model as FW
import rescore_model as RM

SC_SENTINEL = np.uint32(RM._define("RR_DEBUG_SC_SENTINEL", "rr_debug.h"))
KEY_SENTINEL = np.uint32(RM._define("RR_DEBUG_KEY_SENTINEL", "rr_debug.h"))
RR_SEL_LISTED = RM._define("RR_SEL_LISTED", "rr_dense.h")
RR_SEL_MAXQ = RM._define("RR_SEL_MAXQ", "rr_dense.h")
RR_MAX_SCAN_WAVES = RM._define("RR_MAX_SCAN_WAVES", "rr_dense.h")
RR_FLT_MAXQ = RM._define("RR_FLT_MAXQ", "rr_dense.h")
NEG_INF_BITS = np.uint32(0xFF800000)
NEG_ZERO_BITS = np.uint32(0x80000000)
KEY_NEG_INF = np.uint32(0x007FFFFF)
U = 2.0 ** -24
F32 = np.float32
DTYPES = ("f32", "bf16")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------ geometry and routing
def nb_of(nq):
    """query slots of the plain launch that serves nq queries (rr_valu_nb, rr_dense.h)"""
    assert 1 <= nq <= 8
    return 1 if nq <= 1 else 2 if nq <= 2 else 4 if nq <= 4 else 8


def kernel_id(dtype, dim_pad, listed=False):
    """geom[6] of rr_debug_valu_scan: rr_scan_note's 1 / 2, + 10 at a runtime width, + 100 listed"""
    return (2 if dtype == "bf16" else 1) + (10 if dim_pad != 384 else 0) + (100 if listed else 0)


def dim_pad_of(dim):
    return (dim + 63) // 64 * 64


def geom_of(n_rows, tiles_per_wave=1):
    n_tiles = (n_rows + 63) // 64
    return {"n_rows": n_rows, "n_tiles": n_tiles, "n_pad": 64 * n_tiles, "tiles_per_wave": tiles_per_wave,
            "n_waves": (n_tiles + tiles_per_wave - 1) // tiles_per_wave}


def geom_problems(g, n_rows):
    """what is wrong with a launch's geometry (item 1 of the GPU test)"""
    out = []
    if g["n_rows"] != n_rows:
        out.append(f"n_rows {g['n_rows']}")
    if g["n_tiles"] != (n_rows + 63) // 64 or g["n_pad"] != 64 * g["n_tiles"]:
        out.append(f"n_tiles {g['n_tiles']} / n_pad {g['n_pad']}")
    C, W, T = g["tiles_per_wave"], g["n_waves"], g["n_tiles"]
    if not (C >= 1 and W >= 1 and W * C >= T > (W - 1) * C and W <= RR_MAX_SCAN_WAVES):
        out.append(f"{W} waves x {C} tiles for {T} tiles")
    return out


def grids_of_probe(t_probe, c_probe):
    """the resident grids (in waves) that split t_probe tiles into runs of c_probe"""
    return [w for w in range(1, RR_MAX_SCAN_WAVES + 1) if (t_probe + w - 1) // w == c_probe]


def multi_tile_ok(n_tiles, max_waves):
    c = (n_tiles + max_waves - 1) // max_waves
    w = (n_tiles + c - 1) // c
    return c >= 3 and w >= 2 and n_tiles - (w - 1) * c < c


def pick_tiles(t_probe, c_probes, at_least=1):
    """smallest tile count >= at_least at which every grid consistent with every probe (c_probes: runs of the probes of
    several kernels on the same t_probe tiles) gives runs of three tiles or more and a shorter last run"""
    grids = sorted({w for c in c_probes for w in grids_of_probe(t_probe, c)})
    assert grids and grids[-1] < RR_MAX_SCAN_WAVES, (t_probe, c_probes)
    for t in range(max(at_least, 3 * grids[0] - 1), 4 * grids[-1] + at_least + 64):
        if all(multi_tile_ok(t, w) for w in grids):
            return t
    raise AssertionError(f"no tile count serves grids {grids}")


# ------------------------------------------------------------------ storage and queries
def stored_rows(V, dtype):
    """[n, dim] caller rows -> the [n, dim_pad] float32 VALUES the index stores (zero padded; bf16: rounded once)"""
    V = np.ascontiguousarray(V, dtype=np.float32)
    n, dim = V.shape
    S = np.zeros((n, dim_pad_of(dim)), dtype=np.float32)
    S[:, :dim] = V
    return RM.round_to_bf16(S).astype(np.float32) if dtype == "bf16" else S


def bf16_words(stored):
    """the 16-bit patterns of stored bf16 rows (their float32 values have an empty low half)"""
    u = bits(stored)
    nan = np.isnan(stored)
    assert ((u & np.uint32(0xFFFF)) == 0)[~nan].all()
    return np.where(nan, np.uint32(0x7FC0), u >> np.uint32(16)).astype(np.uint16)


def pad_queries(Q, dim_pad, slots):
    """rr_pad_queries: [nq, dim] -> [slots, dim_pad], zero filled"""
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    P = np.zeros((slots, dim_pad), dtype=np.float32)
    P[:len(Q), :Q.shape[1]] = Q
    return P


def chain(stored, q, dtype):
    """float32 chain scores (NaN kept) of stored rows [n, dim_pad] against the padded q [dim_pad]"""
    D = stored.shape[1]
    if dtype == "bf16":
        return RM.chain_bf16(stored, q) if D == 384 else FB.chain_wb(stored, q)
    return RM.chain_f32(stored, q) if D == 384 else FW.chain_w(stored, q)


def stored_scores(stored, q, dtype):
    s = chain(stored, q, dtype)
    return np.where(np.isnan(s), F32(-np.inf), s).astype(np.float32)


# ------------------------------------------------------------------ levels
def levels_of_scores(S, geom):
    """S [NB][n_rows] float32 stored scores (no NaN) -> bits of sims [NB][n_pad], gmax [NB][n_tiles], keys smax [NB][n_waves]"""
    S = np.ascontiguousarray(S, dtype=np.float32)
    NB, n = S.shape
    assert n == geom["n_rows"] and not np.isnan(S).any()
    T, C, W = geom["n_tiles"], geom["tiles_per_wave"], geom["n_waves"]
    sims = np.full((NB, geom["n_pad"]), -np.inf, dtype=np.float32)
    sims[:, :n] = S
    keys = RM.f2key(sims).reshape(NB, T, 64)
    tkey = keys.max(axis=2)                                   # the maximum BY KEY: +0.0 above -0.0
    gmax = bits(RM.key2f(tkey)).reshape(NB, T)
    padded = np.full((NB, W * C), KEY_NEG_INF, dtype=np.uint32)
    padded[:, :T] = tkey
    smax = padded.reshape(NB, W, C).max(axis=2)
    return bits(sims).reshape(NB, -1), gmax, smax


def expected_levels(stored, queries_padded, geom, dtype, cache=None):
    """what one launch with these query slots leaves.  cache: a dict the caller keeps per matrix -- a query's scores do not
    depend on its slot, its launch or the geometry, which is the property under test, so the chain runs once per query"""
    rows = []
    for q in np.ascontiguousarray(queries_padded, dtype=np.float32):
        key = q.tobytes()
        if cache is None or key not in cache:
            s = stored_scores(stored, q, dtype)
            if cache is not None:
                cache[key] = s
        else:
            s = cache[key]
        rows.append(s)
    return levels_of_scores(np.stack(rows), geom)


def mixed_zero(sims_bits, geom):
    """tiles [NB][n_tiles] and runs [NB][n_waves] whose maximum is zero and that hold BOTH +0.0 and -0.0"""
    NB = sims_bits.shape[0]
    T, C, W = geom["n_tiles"], geom["tiles_per_wave"], geom["n_waves"]
    s = from_bits(sims_bits).reshape(NB, T, 64)
    u = np.ascontiguousarray(sims_bits, dtype=np.uint32).reshape(NB, T, 64)
    tmax, pos, neg = s.max(axis=2), (u == 0).any(axis=2), (u == NEG_ZERO_BITS).any(axis=2)
    tiles = (tmax == 0) & pos & neg

    def runs(a, fill, how):
        p = np.full((NB, W * C), fill, dtype=a.dtype)
        p[:, :T] = a
        return how(p.reshape(NB, W, C), axis=2)
    wmax = runs(tmax, F32(-np.inf), np.max)
    return tiles, (wmax == 0) & runs(pos, False, np.any) & runs(neg, False, np.any)


def gamma(k):
    return k * U / (1 - k * U)


def f64_bound(stored, q, dim_pad):
    """[n] float64: gamma_k sum |a_i q_i| (+ the underflow term, see the module docstring); NaN where the sum is"""
    assert stored.shape[1] == dim_pad and dim_pad % 64 == 0
    k = dim_pad // 16 + 4
    with np.errstate(invalid="ignore", over="ignore"):
        mag = np.abs(stored.astype(np.float64) * np.asarray(q, dtype=np.float64)[None, :]).sum(axis=1)
    return gamma(k) * mag + dim_pad * 2.0 ** -150


def f64_scores(stored, q):
    with np.errstate(invalid="ignore", over="ignore"):
        return (stored.astype(np.float64) * np.asarray(q, dtype=np.float64)[None, :]).sum(axis=1)


def f64_excess(sims_bits_q, stored, q):
    """item 3 of the GPU test for one query slot: (rows checked, rows outside the bound, worst |error| / bound)"""
    n, D = stored.shape
    s = from_bits(sims_bits_q)[:n].astype(np.float64)
    fin = np.isfinite(s)
    ref, bound = f64_scores(stored, q), f64_bound(stored, q, D)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(s[fin] - ref[fin]) / bound[fin]
    bad = ~(ratio <= 1.0)                                     # (a NaN reference beside a finite score counts)
    return int(fin.sum()), int(bad.sum()), float(np.nanmax(ratio)) if ratio.size else 0.0


# ------------------------------------------------------------------ the flagged lists
def _listed(idx, NB):
    lst = np.zeros(NB, dtype=np.int32)
    n = len(idx)
    lst[:n] = idx
    if 0 < n < NB:
        lst[n:] = lst[n - 1]
    return lst


def flagged_list(flags, NB=RR_SEL_LISTED):
    """(count, list[NB]) of rr_flagged_list: the first NB flagged queries in query order, slots past the count repeat the last;
    MORE than NB flags up: count 0 (the slots still name the first NB)"""
    idx = np.flatnonzero(np.asarray(flags) != 0)
    return (0 if len(idx) > NB else len(idx)), _listed(idx[:NB], NB)


def flagged_slice(flags, skip, NB=RR_SEL_LISTED):
    """(count, list[NB]) of rr_flagged_slice: the flagged queries ranked [skip, skip + NB)"""
    idx = np.flatnonzero(np.asarray(flags) != 0)[skip:skip + NB]
    return len(idx), _listed(idx, NB)


def list_words(count, lst):
    return np.concatenate([[count], lst]).astype(np.int32)


def flag_patterns(nq):
    """name -> flags[nq] of the listed cases of a call of nq queries (the 384 form serves <= 8 flags; `skip` forms slice 20)"""
    def at(*qs):
        f = np.zeros(nq, dtype=np.int32)
        f[[q for q in qs if q < nq]] = 1
        return f
    spread = np.unique(np.linspace(0, nq - 1, 8).astype(int)) if nq >= 8 else np.arange(nq)
    out = {"none": at(), "q0": at(0), "last": at(nq - 1), "eight": at(*spread)}
    if nq > 63:
        out["q63"] = at(63)
    if nq > 64:
        out["q64"] = at(64)
    if nq >= 9:
        out["nine"] = at(*np.unique(np.linspace(0, nq - 1, 9).astype(int)))
    if nq >= 20:
        out["twenty"] = at(*np.unique(np.linspace(0, nq - 1, 20).astype(int)))
    return out


# ------------------------------------------------------------------ named inputs
def ragged(n_rows, dim, seed=1):
    """random rows of about unit norm"""
    return (np.random.default_rng(seed).standard_normal((n_rows, dim)) / np.sqrt(dim)).astype(np.float32)


def queries(nq, dim, seed=2):
    return (np.random.default_rng(1000 + seed).standard_normal((nq, dim)) / np.sqrt(dim)).astype(np.float32)


C_INF, C_ZERO, C_NAN = 5, 7, 11          # columns of the planted inf / the query's zero component / the planted NaN
TINY_Q = F32(2.0 ** -20)                 # |component| of the underflow query
TINY_A = F32(2.0 ** -133)                # the smallest bf16 denormal: TINY_A TINY_Q = 2^-153 < 2^-150 rounds to a zero
SPECIAL_NQ = 3


def special_queries(dim, seed=3):
    """[3, dim]: q_full (no zero component, |q_i| in [0.5, 1.5] / sqrt(dim)); q_zero (q_full with component C_ZERO zero);
    q_tiny (every component +-2^-20: every product with a row of +-2^-133 underflows)"""
    rng = np.random.default_rng(2000 + seed)
    sgn = np.where(rng.random(dim) < 0.5, -1.0, 1.0)
    full = (sgn * rng.uniform(0.5, 1.5, dim) / np.sqrt(dim)).astype(np.float32)
    zero = full.copy()
    zero[C_ZERO] = 0.0
    tiny = (np.where(rng.random(dim) < 0.5, -1.0, 1.0) * TINY_Q).astype(np.float32)
    return np.stack([full, zero, tiny])


def negzero_reaches(dim, dtype):
    """whether special_rows' `negzero` row scores -0.0 against q_tiny at this width and storage (see special_rows)"""
    return dim % 64 == 0 and (dtype == "f32" or dim % 128 == 0)


def special_layout(n_tiles, runs=(1,)):
    """where special_rows plants by tile, for launches whose runs are `runs` tiles long: the tie seam is a run seam of the
    longest run, the zero region is every run (of any length in `runs`) that holds the zero tile"""
    cm = max(runs)
    seam = 2 * cm                      # (run 0 holds the +-inf scores)
    tz = 3 * cm + 1
    lo = min(tz // c * c for c in runs)
    hi = max(tz // c * c + c for c in runs)
    nan_tile = hi + 1
    assert nan_tile + 1 < n_tiles, f"{n_tiles} tiles are too few for runs of {runs}"
    return {"seam": seam, "zero_tile": tz, "zero_region": (lo, hi), "nan_tile": nan_tile}


def special_rows(n_rows, dim, runs=(1,), seed=4):
    """-> V [n_rows, dim] (random, with the plants), Q [3, dim] (special_queries), plants: name -> rows.
        nan         a NaN element                                              -> -inf for every query
        pinf, ninf  a +inf / -inf element against a non-zero component         -> +-inf
        inf_zero    a +inf element in column C_ZERO                            -> NaN = -inf for q_zero, +-inf for the others
        overflow    every element 3e38 with q_full's sign                      -> the chain overflows to +inf for q_full
        zero        an all-zero row                                            -> +0.0
        negzero     every element -sign(q_tiny_i) 2^-133, same tile as `zero`  -> every product underflows to -0.0: the row scores
                                                                                  -0.0 for q_tiny where EVERY lane's chain ends on such
                                                                                  a product (negzero_reaches: a pad column, or a lane
                                                                                  without a chunk, adds +0.0 and the row sum is +0.0)
        the zero region's other rows score < 0 for q_tiny: the tile and the run of `zero` have maximum zero of both signs
        nan_tile    a whole tile of rows with a NaN element                    -> tile maximum -inf
        ties        the same row on both sides of a run seam, q_full's best    -> the same bits in two tiles and two runs"""
    n_tiles = (n_rows + 63) // 64
    L = special_layout(n_tiles, runs)
    V = ragged(n_rows, dim, seed)
    Q = special_queries(dim)
    full, tiny = Q[0], Q[2]
    lo, hi = L["zero_region"]
    region = np.arange(64 * lo, min(64 * hi, n_rows))
    V[region] = -np.sign(tiny)[None, :] * np.abs(V[region])              # negative against q_tiny
    z0 = 64 * L["zero_tile"]
    plants = {"nan": [17], "pinf": [20], "ninf": [35], "inf_zero": [42], "overflow": [50], "zero": [z0 + 9], "negzero": [z0 + 30],
              "nan_tile": list(range(64 * L["nan_tile"], 64 * L["nan_tile"] + 64)), "ties": [64 * L["seam"] - 1, 64 * L["seam"]]}
    V[17, C_NAN] = np.nan
    V[20, C_INF] = np.inf
    V[35, C_INF] = -np.inf
    V[42, C_ZERO] = np.inf
    V[50] = np.sign(full) * F32(3e38)
    V[z0 + 9] = 0.0
    V[z0 + 30] = -np.sign(tiny) * TINY_A
    for r in plants["nan_tile"]:
        V[r, (7 * r) % dim] = np.nan
    V[plants["ties"]] = (2.0 * full / np.dot(full.astype(np.float64), full.astype(np.float64))).astype(np.float32)[None, :]
    assert max(r for rr in plants.values() for r in rr) < n_rows
    return V, Q, plants


def maxima_plants(V, Q, geom, avoid=()):
    """plants into V (in place), for each query slot b of Q, the maximum of one run in the run's first tile, of another in its
    last tile, of a third in a middle tile -- at row b of the tile, at row 63 - b, at row 31 + b, so slot 0 has a tile maximum
    at row 0 and one at row 63 -- as the row (4 + b) q_b / |q_b|^2 (score 4 + b against q_b, far above everything unplanted).
    The three runs of a slot differ; runs that hold a tile of `avoid` and the ragged last run are passed over.
    -> {(slot, where): (run, tile, row)}"""
    C, W = geom["tiles_per_wave"], geom["n_waves"]
    free = [w for w in range(W - 1) if not any(w * C <= t < (w + 1) * C for t in avoid)]
    assert len(free) >= 3, (geom, avoid)
    out = {}
    for b, q in enumerate(np.ascontiguousarray(Q, dtype=np.float32)):
        nrm = float(np.dot(q.astype(np.float64), q.astype(np.float64)))
        if nrm == 0.0:
            continue
        for j, (where, tile_in_run, row_in_tile) in enumerate((("first", 0, b), ("last", C - 1, 63 - b), ("middle", C // 2, 31 + b))):
            w = free[(3 * b + j) % len(free)]
            tile = w * C + tile_in_run
            row = 64 * tile + row_in_tile
            V[row] = ((4.0 + b) * q[:V.shape[1]] / nrm).astype(np.float32)
            out[(b, where)] = (w, tile, row)
    return out
