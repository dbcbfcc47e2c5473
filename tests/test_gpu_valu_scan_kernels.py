"""The VALU dense scans -- rr_scan_f32<6, NB>, rr_scan_f32<6, 8, true> (listed), rr_scan_f32_generic<NB>,
rr_scan_f32_generic_listed<8>, rr_scan_bf16<NB>, rr_scan_bf16_generic<NB>, rr_scan_bf16_generic_listed<8> -- ONE launch at a time
against tests/valu_scan_model.py (librr_hip_dbg.so: rr_debug_valu_scan, which pads the queries, sizes the scratch and launches
through the helpers the product calls, and copies the raw levels back).  These kernels' per-row fmaf chain is what every other
dense path is held against ("bit for bit the single-query answer"); tests/test_valu_scan_model.py has shown on the CPU that
the model equals float64 brute force within its bound and that every named input reaches its door.

Every launch (a line `L|...` of a child process; the parent asserts on the lines) is held to all of:
 1  the geometry is self-consistent, and the kernel id and NB are the ones the product routes this index and nq to;
 2  sims equals the model BIT FOR BIT in every slot and every row, pad rows and zero-query slots included;
 3  every finite score is within valu_scan_model.f64_bound of the float64 product of the STORED rows with the fp32 query;
 4  gmax[b][t] is the maximum of that slot's 64 sims of tile t and smax[b][w] the key of the maximum of wave w's run, compared as
    bits -- with one exception: a tile or run whose maximum is zero and which holds +0.0 and -0.0 is compared by value, and
    whether the kernel reported the -0.0 is recorded (field negzero);
 5  every word outside what the launch owns (sims past NB n_pad, gmax past NB n_tiles, smax past NB n_waves; everything, for a
    listed launch that returns early) still holds its sentinel;
 6  list_out equals the list model (written also when the count is 0), and a plain launch leaves it alone;
 7  (INV lines) one query leaves the same sims bits in slot 0 of an NB = 1 launch, in slots 1, 2, 7 of NB = 2, 4, 8 launches and
    as a listed query, under the default geometry and under runs of several tiles.

The -0.0 question.  On an MI355X no launch reported the -0.0: in every launch with a tile and a run that hold both zeros and
nothing above (special_rows' zero tile against q_tiny; fp32 and bf16 rows, NB = 4 and 8, both geometries) gmax and the key in
smax came back as +0.0 (negzero = 0 in every line), i.e. fmaxf in rr_wave_max and in the carry of `gm` orders -0.0 below +0.0
as rr_f2key does, and every maximum equals the model's maximum BY KEY bit for bit.  It matters: rr_select opens a group, then a
tile, when its key is >= tau, and tau (about the pool-th largest group key) can be the key of +0.0 when `pool` groups hold a
row scoring >= +0.0; a tile whose +0.0 row was reported as -0.0 would then be skipped although that row ties with the cut and
wins the tie by its row number -- a lost row.  So a reported -0.0 is a problem here (the comparison is bitwise against the
maximum by key), not merely recorded.
The denormal question.  Neither side flushes: special_rows' negzero row (every product 2^-153, below half the smallest
denormal) scores -0.0 against q_tiny and a denormal ~1e-40 against the normal queries, the kernels' bits equal
rescore_model.fma32's, which rounds such a product to a signed zero and keeps denormal sums, and the scores stay within
f64_bound with its underflow term.  No model or kernel change was needed.

Measured on an MI355X: 0 problems in every launch (no kernel bug found); the worst |score - float64| was 0.177 of f64_bound.
The file runs 391 launches (180 plain, 101 at runs of several tiles, 110 listed and refused) in three child processes, 17 s
in all.  With one CU's share of the grid the kernels came back with runs of 3, 5 and 7 tiles (384 wide, 3301 / 2149 rows)
and 3, 4 and 5 tiles (other widths, 4261 rows).

Kernel-side mutations, each applied to a copy of the tree, built into the debug library alone and run against this file:
    (a) two adjacent fmaf of rr_dot_rows swapped            test_scan_384_one_tile_per_wave[f32], test_runs_..[f32] and
                                                            test_listed_forms[f32-384] fail from the first launch: "f32 dim 384 n 1
                                                            nq 1 .. 1 scores differ from the model, first slot 0 row 0: kernel
                                                            0x3b705308, model 0x3b705310" (inside the float64 bound: only the bits tell)
    (b) rr_finish_tile stores gmax from lane 0's own v      8 of 10 tests fail (all but rr_scan_bf16's, which has its own tile end):
                                                            "f32 dim 384 n 63 nq 1 .. 1 tile maxima differ, first slot 0 tile 0:
                                                            kernel 0x3b705310, maximum of its scores 0x7f800000"
    (c) the `valid` mask dropped from rr_finish_tile        the same 8 tests: "f32 dim 384 n 1 nq 1 .. 63 scores differ from the model,
                                                            first slot 0 row 1: kernel 0x3b705310, model 0xff800000 ; pad rows are not -inf"
    (d) rr_flagged_list returns n when total > NB           test_listed_forms[f32-384]: "call of 9 nine skip 0 .. list_out [8, 0, 1, ..],
                                                            model [0, 0, 1, ..] ; 8448 words outside the launch's own were written"
    (e) rr_bf16w_scan_rows starts pf_i at 1 for waves > 0   test_scan_generic_one_tile_per_wave[bf16], test_runs_..[bf16],
                                                            test_listed_forms[bf16-768]: "bf16 dim 64 n 1000 nq 1 .. 816 scores differ
                                                            from the model, first slot 0 row 68 (tile 1, run 1)" (wave 0's tile is right)
((a) was run when rr_dot_rows held its own four fmaf.)  The chain step of each storage type is now ONE function (rr_dense.h) that
every scan and every rescoring kernel calls.  Two adjacent fmaf swapped inside it, run against this file,
test_gpu_rescore_kernels.py, test_gpu_fltw_kernels.py and test_gpu_bf16_wide_kernels.py (18 tests):
    (f) rr_f32_chunk: the x and y products swapped          8 fail, every fp32 chain and no other: here test_scan_384_..[f32],
                                                            test_scan_generic_..[f32], test_runs_..[f32], test_listed_forms[f32-384] and
                                                            [f32-768]; test_rescoring_of_fp32_rows_with_and_without_the_plane and
                                                            test_rescoring_of_rows_with_nan_and_inf_elements (rr_rescore_chain, both
                                                            fp32 branches); test_gpu_fltw_kernels' test_rescored_rows_are_the_chain_bit_
                                                            for_bit (rr_rescore_chain_w)
    (g) rr_bf16_chunk: the first two products swapped       6 fail, every bf16 chain and no other: here test_scan_384_..[bf16],
                                                            test_scan_generic_..[bf16], test_runs_..[bf16], test_listed_forms[bf16-768];
                                                            test_rescoring_of_bf16_rows (rr_rescore_chain); test_gpu_bf16_wide_kernels'
                                                            test_rescored_bf16_rows_are_the_chain_bit_for_bit (rr_rescore_chain_wb):
                                                            "bf16 dim 384 n 1 nq 1 .. 1 scores differ from the model, first slot 0 row 0
                                                            (tile 0, run 0): kernel 0x3b801170, model 0x3b80116c"
"""
import pathlib
import subprocess
import sys

import pytest

import valu_scan_model as M

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)

COMMON = r"""
import os, sys, time
os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, @ROOT@); sys.path.insert(0, os.path.join(@ROOT@, "tests"))
import ctypes as C
import numpy as np, torch
import valu_scan_model as M
import rescore_model as RM
from review_recommender_amd import _lib
from review_recommender_amd.index import ProductIndex
lib = _lib.load()
dev = torch.device("cuda", 0)
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
HOST_FILL = np.uint32(0x11111111)
SLOTS = 8                                      # rr_ensure_scratch(ix, 8) on an index no search has touched
GN = ("n_rows", "n_tiles", "n_pad", "tiles_per_wave", "n_waves", "NB", "kernel", "sims_words", "gmax_words", "smax_words")
T0 = time.time()
N_LAUNCH = [0]

def make_index(V, dtype):
    # -> the index over V [n, dim] (adopted device memory, padded) and the rows it stores, as float32 values [n, dim_pad]
    stored = M.stored_rows(V, dtype)
    host = M.bf16_words(stored).view(np.int16) if dtype == "bf16" else stored
    t = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    ix = ProductIndex(None, n_rows=len(V), dim=V.shape[1], device_ptr=t.data_ptr(), keepalive=t, dtype=dtype)
    assert ix.dim_padded == stored.shape[1]
    return ix, stored

def raw_launch(ix, Q, form, flags, skip, caps):
    nq = len(Q)
    dq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    torch.cuda.synchronize()
    sims, gmax, smax = (np.full(c, HOST_FILL, dtype=np.uint32) for c in caps)
    lst = np.full(1 + M.RR_SEL_LISTED, -7, dtype=np.int32)
    geom = np.zeros(10, dtype=np.int64)
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.int32)
    rc = lib.rr_debug_valu_scan(ix.handle, C.c_void_p(dq.data_ptr()), nq, form, P(fl), skip, P(geom), P(sims), len(sims), P(gmax), len(gmax),
                                P(smax), len(smax), P(lst))
    return rc, dict(zip(GN, geom.tolist())), sims, gmax, smax, lst

def caps_of(n_rows):
    T = (n_rows + 63) // 64
    return (SLOTS * 64 * T, SLOTS * 4 * T + M.RR_MAX_SCAN_WAVES * M.RR_FLT_MAXQ, 2 * SLOTS * M.RR_MAX_SCAN_WAVES)

def launch(ix, Q, form=0, flags=None, skip=0):
    caps = caps_of(ix.n_rows)
    rc, g, sims, gmax, smax, lst = raw_launch(ix, Q, form, flags, skip, caps)
    _lib.check(rc, "rr_debug_valu_scan")
    N_LAUNCH[0] += 1
    assert (g["sims_words"], g["gmax_words"], g["smax_words"]) == caps, (g, caps)       # every word of the three buffers came back
    return g, sims, gmax, smax, lst

def check_launch(tag, ix, stored, dtype, Q, cache, form=0, flags=None, skip=0, want_multi=False):
    # one launch held to items 1..6; -> (geometry, the sims bits [NB][n_pad] or None when the launch returned early)
    n, D = stored.shape
    nq = len(Q)
    g, sims, gmax, smax, lst = launch(ix, Q, form, flags, skip)
    pr = M.geom_problems(g, n)
    NB = M.RR_SEL_LISTED if form == 1 else M.nb_of(nq)
    if g["NB"] != NB or g["kernel"] != M.kernel_id(dtype, D, form == 1):
        pr.append(f"NB {g['NB']} kernel {g['kernel']}, the product routes to NB {NB} kernel {M.kernel_id(dtype, D, form == 1)}")
    T, W, C, n_pad = g["n_tiles"], g["n_waves"], g["tiles_per_wave"], g["n_pad"]
    if want_multi and not (C >= 3 and T - (W - 1) * C < C and n % 64 != 0):
        pr.append(f"runs of {C} tiles, last run {T - (W - 1) * C}, n_rows % 64 = {n % 64}: not the geometry this case is about")
    count = NB
    QP = M.pad_queries(Q, D, NB) if form == 0 else None
    if form == 1:
        count, want_list = M.flagged_list(flags, NB) if D == 384 else M.flagged_slice(flags, skip, NB)
        if lst.tolist() != M.list_words(count, want_list).tolist():
            pr.append(f"list_out {lst.tolist()}, model {M.list_words(count, want_list).tolist()}")
        QP = M.pad_queries(Q, D, nq)[want_list]
    own = (NB * n_pad, NB * T, NB * W) if count > 0 else (0, 0, 0)
    outside = int((sims[own[0]:] != M.SC_SENTINEL).sum() + (gmax[own[1]:] != M.SC_SENTINEL).sum() + (smax[own[2]:] != M.KEY_SENTINEL).sum())
    if outside:
        pr.append(f"{outside} words outside the launch's own were written")
    fields = dict(NB=NB, kernel=g["kernel"], rows=n, tpw=C, waves=W, count=count, outside=outside)
    S = None
    if count > 0:
        S = sims[:own[0]].reshape(NB, n_pad)
        e_sims = M.expected_levels(stored, QP, g, dtype, cache)[0]   # (with equal scores the model's maxima are those of k_gmax / k_smax below)
        bad = np.argwhere(S != e_sims)
        if len(bad):
            b, r = bad[0]
            pr.append(f"{len(bad)} scores differ from the model, first slot {b} row {r} (tile {r // 64}, run {r // 64 // C}): kernel {S[b, r]:#010x}, model {e_sims[b, r]:#010x}")
        checked = worst = n_bad = 0
        for b in range(NB):
            c, nb_, w_ = M.f64_excess(S[b], stored, QP[b])
            checked, n_bad, worst = checked + c, n_bad + nb_, max(worst, w_)
        if n_bad:
            pr.append(f"{n_bad} finite scores outside the float64 bound (worst {worst:.3f} bounds)")
        # the maxima of the kernel's OWN scores, by key; mixed zeros by value
        k_sims, k_gmax, k_smax = M.levels_of_scores(M.from_bits(S)[:, :n], g)
        if (k_sims != S).any():
            pr.append("pad rows are not -inf")
        tiles, runs = M.mixed_zero(S, g)
        G, K = gmax[:own[1]].reshape(NB, T), smax[:own[2]].reshape(NB, W)
        bad_g = (G != k_gmax) & ~(tiles & (M.from_bits(G) == 0))
        bad_k = (K != k_smax) & ~(runs & (RM.key2f(K) == 0))
        negzero = int((G[tiles] == M.NEG_ZERO_BITS).sum() + (K[runs] == RM.f2key(np.float32(-0.0))).sum())
        if bad_g.any():
            b, t = np.argwhere(bad_g)[0]
            pr.append(f"{int(bad_g.sum())} tile maxima differ, first slot {b} tile {t}: kernel {G[b, t]:#010x}, maximum of its scores {k_gmax[b, t]:#010x}")
        if bad_k.any():
            b, w = np.argwhere(bad_k)[0]
            pr.append(f"{int(bad_k.sum())} group keys differ, first slot {b} run {w}: kernel {K[b, w]:#010x}, key of its maximum {k_smax[b, w]:#010x}")
        if negzero:
            pr.append(f"{negzero} maxima of a tile or run holding +0.0 and -0.0 came back as -0.0")
        nan_tiles = int((k_gmax == M.NEG_INF_BITS).sum())
        fields.update(bad_sims=len(bad), f64_rows=checked, f64_bad=n_bad, f64_worst=f"{worst:.3f}", bad_gmax=int(bad_g.sum()), bad_smax=int(bad_k.sum()),
                      mixed=int(tiles.sum() + runs.sum()), negzero=negzero, neg_inf_tiles=nan_tiles)
    if form == 0 and (lst.view(np.uint32) != M.KEY_SENTINEL).any():
        pr.append(f"a plain launch wrote the flagged list: {lst.tolist()}")
    print(f"L|{tag}|" + "|".join(f"{k}={v}" for k, v in fields.items()) + f"|problems={len(pr)}|" + " ; ".join(pr), flush=True)
    return g, S

Q8_CACHE = {}
def queries8(dim):
    # three special queries + five random ones
    if dim not in Q8_CACHE:
        Q8_CACHE[dim] = np.concatenate([M.special_queries(dim), M.queries(5, dim, dim)])
    return Q8_CACHE[dim]

def done():
    print(f"LAUNCHES|{N_LAUNCH[0]}|seconds={time.time() - T0:.1f}", flush=True)
    print("DONE", flush=True)
"""

PLAIN = r"""
# one tile per wave (the default geometry): n_rows 1, 63, 64, 65, 1000 as prefixes of ONE matrix with the special rows
KINDS, NQS_ALL, ALL_AT = @KINDS@, (1, 2, 3, 5, 8), @ALL_AT@
for dtype, dim in KINDS:
    V, _, plants = M.special_rows(1000, dim)
    Q8 = queries8(dim)
    for n in (1, 63, 64, 65, 1000):
        ix, stored = make_index(V[:n], dtype)
        cache = {}
        for nq in (NQS_ALL if dim in ALL_AT else (1, 8)):
            check_launch(f"{dtype} dim {dim} n {n} nq {nq}", ix, stored, dtype, Q8[:nq], cache)
        ix.close()
done()
"""

RUNS = r"""
# runs of several tiles (a grid of one CU's share): the special rows, the planted maxima, and one query in every slot, every
# launch form and both geometries
T_PROBE = 97
for dtype, dim, nqs, listed in @KINDS@:
    D = M.dim_pad_of(dim)
    Q8 = queries8(dim)
    probe, _ = make_index(np.zeros((64 * T_PROBE - 27, dim), dtype=np.float32), dtype)
    _lib.check(lib.rr_index_set_scan_cus(probe.handle, 1), "rr_index_set_scan_cus")
    c_probe = {}
    for nq in nqs:
        c_probe[nq] = launch(probe, Q8[:nq])[0]["tiles_per_wave"]
    if listed:
        c_probe["listed"] = launch(probe, Q8, 1, np.ones(8, dtype=np.int32), 0)[0]["tiles_per_wave"]
    probe.close()
    grids = sorted({w for c in c_probe.values() for w in M.grids_of_probe(T_PROBE, c)})
    at_least = 1
    while True:
        T = M.pick_tiles(T_PROBE, list(c_probe.values()), at_least)
        runs = tuple(sorted({(T + w - 1) // w for w in grids}))
        try:
            M.special_layout(T, runs)
            break
        except AssertionError:
            at_least = T + 1
    n = 64 * (T - 1) + 37
    print(f"GEOM|{dtype} dim {dim}|probe={c_probe}|grids={grids}|tiles={T}|runs={runs}|rows={n}", flush=True)

    # ---- the special rows
    V, _, plants = M.special_rows(n, dim, runs)
    ix, stored = make_index(V, dtype)
    _lib.check(lib.rr_index_set_scan_cus(ix.handle, 1), "rr_index_set_scan_cus")
    cache, geoms = {}, {}
    for nq in nqs:
        geoms[nq], _ = check_launch(f"special|{dtype} dim {dim} nq {nq}", ix, stored, dtype, Q8[:nq], cache, want_multi=True)

    # ---- one query (q_full) in slot 0 of NB = 1, slot 1 / 2 / 7 of NB = 2 / 4 / 8, and listed; runs of several tiles, then the default geometry
    seen = {}
    for cus, geo in ((1, "runs"), (0, "default")):
        _lib.check(lib.rr_index_set_scan_cus(ix.handle, cus), "rr_index_set_scan_cus")
        for nq, slot in ((1, 0), (2, 1), (3, 2), (8, 7)):
            if nq not in nqs:
                continue
            Q = Q8[:nq].copy()
            Q[[0, slot]] = Q[[slot, 0]]
            g, S = check_launch(f"slot|{dtype} dim {dim} {geo} nq {nq} slot {slot}", ix, stored, dtype, Q, cache, want_multi=cus == 1)
            seen[(geo, f"NB {g['NB']} slot {slot}", g["tiles_per_wave"])] = S[slot]
        if listed:
            Q = np.concatenate([M.queries(64, dim, 77), Q8[:1]])                 # a call of 65 queries, the flag up at query 64
            flags = np.zeros(65, dtype=np.int32)
            flags[64] = 1
            g, S = check_launch(f"slot|{dtype} dim {dim} {geo} listed query 64", ix, stored, dtype, Q, cache, 1, flags, 0, want_multi=cus == 1)
            seen[(geo, "listed", g["tiles_per_wave"])] = S[0]
            if not (S[1:] == S[0]).all():
                print(f"L|repeat|{dtype} dim {dim} {geo}|problems=1|slots past the count do not repeat the listed query's scores", flush=True)
    first = next(iter(seen.values()))
    diff = [k for k, s in seen.items() if (s != first).any()]
    tpws = ",".join(map(str, sorted({k[2] for k in seen})))
    print(f"INV|{dtype} dim {dim}|forms={len(seen)}|tpw={tpws}|problems={len(diff)}|" + " ; ".join(map(str, diff)), flush=True)
    ix.close()

    # ---- planted maxima: one matrix per run length the launches came back with
    R8 = M.queries(8, dim, 5)
    for Cr in sorted({g["tiles_per_wave"] for g in geoms.values()}):
        g0 = M.geom_of(n, Cr)
        V = M.ragged(n, dim, 11)
        planted = M.maxima_plants(V, R8, g0)
        ix, stored = make_index(V, dtype)
        _lib.check(lib.rr_index_set_scan_cus(ix.handle, 1), "rr_index_set_scan_cus")
        cache = {}
        for nq in [q for q in nqs if geoms[q]["tiles_per_wave"] == Cr]:
            g, S = check_launch(f"maxima|{dtype} dim {dim} runs of {Cr} nq {nq}", ix, stored, dtype, R8[:nq], cache, want_multi=True)
            Sf = M.from_bits(S)
            at_max = sum(int(np.argmax(Sf[b, 64 * Cr * w:64 * Cr * (w + 1)])) + 64 * Cr * w == row for (b, _), (w, _, row) in planted.items() if b < nq)
            print(f"PLANTS|{dtype} dim {dim} runs of {Cr} nq {nq}|planted={3 * nq}|at_max={at_max}|same_geom={int(g['tiles_per_wave'] == Cr and g['n_waves'] == g0['n_waves'])}", flush=True)
        ix.close()
done()
"""

LISTED = r"""
# the listed forms: calls of 9, 64, 65 and 256 queries on the 1000-row matrix with the special rows
for dtype, dim in @KINDS@:
    D = M.dim_pad_of(dim)
    V, _, plants = M.special_rows(1000, dim)
    ix, stored = make_index(V, dtype)
    cache = {}
    QALL = np.concatenate([queries8(dim), M.queries(M.RR_SEL_MAXQ - 8, dim, 31)])
    for nq in (9, 64, 65, 256):
        Q = QALL[:nq]
        for name, flags in M.flag_patterns(nq).items():
            skips = (0,) if D == 384 else (0, 8) if name == "nine" else (0, 8, 16, 24) if name == "twenty" else (0,)
            if D == 384 and name == "twenty":
                continue
            for skip in skips:
                check_launch(f"{dtype} dim {dim} call of {nq} {name} skip {skip}", ix, stored, dtype, Q, cache, 1, flags, skip)
    ix.close()
done()
"""

REFUSALS = r"""
# a bad argument gives RR_E_INVALID, names the entry, launches nothing (the host arrays keep their fill)
V = M.ragged(200, 384, 1)
ix, stored = make_index(V, "f32")
ixb, _ = make_index(V, "bf16")
ixw, _ = make_index(M.ragged(200, 100, 1), "f32")
Q = M.queries(9, 384)
Qw = M.queries(9, 100)
caps = caps_of(200)
f9 = np.ones(9, dtype=np.int32)
def refuse(name, ix_, Q_, form, flags, skip, caps_):
    rc, g, sims, gmax, smax, lst = raw_launch(ix_, Q_, form, flags, skip, caps_)
    untouched = int((sims == HOST_FILL).all() and (gmax == HOST_FILL).all() and (smax == HOST_FILL).all() and (lst == -7).all() and not any(g.values()))
    print(f"REFUSE|{name}|rc={rc}|untouched={untouched}", flush=True)
launch(ix, Q[:1]); launch(ixb, Q[:1]); launch(ixw, Qw[:1])       # (the scratch exists: what is refused below is the argument)
refuse("nq 9 plain", ix, Q, 0, None, 0, caps)
refuse("plain with flags", ix, Q[:8], 0, f9[:8], 0, caps)
refuse("plain with skip", ix, Q[:8], 0, None, 8, caps)
refuse("listed without flags", ix, Q, 1, None, 0, caps)
refuse("form 2", ix, Q[:8], 2, None, 0, caps)
refuse("skip at 384", ix, Q, 1, f9, 8, caps)
refuse("negative skip", ixw, Qw, 1, f9, -1, caps)
refuse("listed bf16 384", ixb, Q, 1, f9, 0, caps)
refuse("sims cap", ix, Q[:8], 0, None, 0, (caps[0] + 1, caps[1], caps[2]))
refuse("gmax cap", ix, Q[:8], 0, None, 0, (caps[0], caps[1] + 1, caps[2]))
refuse("smax cap", ix, Q[:8], 0, None, 0, (caps[0], caps[1], caps[2] + 1))
for i in (ix, ixb, ixw):
    i.close()
done()
"""



GROUPS = {"plain": (PLAIN, 420), "runs": (RUNS, 540), "listed": (LISTED.replace("done()", "") + REFUSALS, 300)}
_OUT = {}


def _child(group: str, **subst) -> str:
    """the output of a group's child process (one process per group and set of kinds, run once per session)"""
    key = (group, repr(sorted(subst.items())))
    if key in _OUT:
        return _OUT[key]
    from review_recommender_amd.build import DEBUG_LIB_PATH
    assert DEBUG_LIB_PATH.exists(), "librr_hip_dbg.so not built (python review-recommender_amd/build.py --debug)"
    body, timeout = GROUPS[group]
    src = (COMMON + body).replace("@ROOT@", repr(ROOT))
    for k, v in subst.items():
        src = src.replace("@" + k + "@", repr(v))
    p = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "DONE" in p.stdout
    _OUT[key] = p.stdout
    return p.stdout


def _lines(out: str, tag: str):
    return [l.split("|")[1:] for l in out.splitlines() if l.startswith(tag + "|")]


def _field(line, name):
    return [f.split("=", 1)[1] for f in line if f.startswith(name + "=")][0]


def _no_problems(lines):
    bad = [l for l in lines if _field(l, "problems") != "0"]
    assert not bad, "\n".join("|".join(l) for l in bad[:12])


def _of(lines, dtype, dim=None):
    # the L lines of one storage dtype (and width): the tag's last part starts "<dtype> dim <dim> ..."
    def kind(l):
        w = [p for p in l if " dim " in p][0].split()
        return w[0], int(w[2])
    return [l for l in lines if kind(l)[0] == dtype and (dim is None or kind(l)[1] == dim)]


WIDE = {"f32": (64, 100, 320, 768, 1000),       # dim_pad 64, 128, 320, 768, 1024
        "bf16": (64, 192, 100, 768, 1000)}      # dim_pad 64 and 192 (last ring round half full), 128, 768, 1024
PLAIN_KINDS = tuple((dt, d) for dt in M.DTYPES for d in (384,) + WIDE[dt])


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_scan_384_one_tile_per_wave(dtype):
    """rr_scan_f32<6, NB> / rr_scan_bf16<NB>, NB = 1, 2, 4, 8 reached with nq = 1, 2, 3, 5, 8 (zero slots occur), n_rows 1, 63,
    64, 65, 1000; the 1000-row matrix carries every plant of special_rows."""
    L = _of(_lines(_child("plain", KINDS=PLAIN_KINDS, ALL_AT=(384, 100)), "L"), dtype, 384)
    assert len(L) == 25
    _no_problems(L)
    assert {_field(l, "NB") for l in L} == {"1", "2", "4", "8"} and {_field(l, "kernel") for l in L} == {str(M.kernel_id(dtype, 384))}
    assert {_field(l, "tpw") for l in L} == {"1"}
    big = [l for l in L if _field(l, "rows") == "1000"]
    assert all(int(_field(l, "neg_inf_tiles")) >= 1 for l in big)                       # the NaN tile
    assert all(int(_field(l, "mixed")) >= 2 for l in big if int(_field(l, "NB")) >= 4)     # q_tiny's zero tile and run


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_scan_generic_one_tile_per_wave(dtype):
    """rr_scan_f32_generic<NB> / rr_scan_bf16_generic<NB>: NB = 1 and 8 at every width (dim 100 and 1000 are no multiple of 64),
    all four NB at dim 100."""
    out = _child("plain", KINDS=PLAIN_KINDS, ALL_AT=(384, 100))
    L = [l for l in _of(_lines(out, "L"), dtype) if l not in _of(_lines(out, "L"), dtype, 384)]
    assert len(L) == 5 * (4 * 2 + 5)
    _no_problems(L)
    assert {_field(l, "NB") for l in L} == {"1", "2", "4", "8"} and {_field(l, "kernel") for l in L} == {str(M.kernel_id(dtype, 64))}
    assert _launches(out) == 2 * (25 + 65)


def _launches(out):
    return int(_lines(out, "LAUNCHES")[0][0])


RUN_KINDS = (("f32", 384, (1, 2, 3, 5, 8), True), ("f32", 100, (1, 8), True), ("f32", 768, (1, 8), True),
             ("bf16", 384, (1, 2, 3, 5, 8), False), ("bf16", 192, (1, 8), True), ("bf16", 768, (1, 8), True))


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_runs_of_several_tiles_and_batch_invariance(dtype):
    """A grid of one CU's share (rr_index_set_scan_cus(ix, 1)): one probe per kernel, then n_rows chosen from it so that every
    launch comes back with tiles_per_wave >= 3, a shorter last run and n_rows % 64 != 0 (asserted from the returned geometry
    in check_launch: a launch that misses it is a problem, not a skip).  special_rows and maxima_plants at that geometry; then
    q_full in slot 0 / 1 / 2 / 7 of NB = 1 / 2 / 4 / 8 and as the listed query 64 of a call of 65, under runs of several tiles
    and under the default geometry: the same sims bits everywhere (INV)."""
    out = _child("runs", KINDS=RUN_KINDS)
    kinds = [k for k in RUN_KINDS if k[0] == dtype]
    L = _of(_lines(out, "L"), dtype)
    _no_problems(L)
    assert len(_of(_lines(out, "GEOM"), dtype)) == 3
    inv = _of(_lines(out, "INV"), dtype)
    assert len(inv) == 3
    _no_problems(inv)
    for l, kind in zip(inv, kinds):
        assert int(_field(l, "forms")) == 2 * (len([q for q in kind[2] if q in (1, 2, 3, 8)]) + int(kind[3])), l
        tpw = [int(c) for c in _field(l, "tpw").split(",")]
        assert tpw[0] == 1 and tpw[-1] >= 3, l                                             # both geometries were compared
    special = [l for l in L if l[0] == "special"]
    assert len(special) == sum(len(k[2]) for k in kinds)
    assert all(int(_field(l, "tpw")) >= 3 and int(_field(l, "neg_inf_tiles")) >= 1 for l in special)
    for dt, dim, _, _ in kinds:
        if M.negzero_reaches(dim, dt):                                                     # q_tiny's zero tile and its run
            assert all(int(_field(l, "mixed")) >= 2 for l in _of(special, dt, dim) if int(_field(l, "NB")) >= 4)
    plants = _of(_lines(out, "PLANTS"), dtype)
    assert len(plants) == len(special)
    for l in plants:
        assert _field(l, "same_geom") == "1" and _field(l, "at_max") == _field(l, "planted"), l


LISTED_KINDS = (("f32", 384), ("f32", 768), ("bf16", 768))


@pytest.mark.parametrize("kind", LISTED_KINDS, ids=lambda k: f"{k[0]}-{k[1]}")
def test_listed_forms(kind):
    """rr_scan_f32<6, 8, true>, rr_scan_f32_generic_listed<8>, rr_scan_bf16_generic_listed<8> in calls of 9, 64, 65 and 256
    queries: no flag (count 0: the list is written, the levels keep their sentinels); one flag at query 0, 63, 64 and the last;
    eight flags over several ballot words; nine flags (384: count 0, nothing written; the `skip` forms: eight, then one); twenty
    flags with skip 0, 8, 16 (a slice of four, the last repeated) and 24 (empty)."""
    L = _of(_lines(_child("listed", KINDS=LISTED_KINDS), "L"), *kind)
    _no_problems(L)
    wide = int(kind[1] != 384)
    # patterns per call: none, q0, last, eight, nine (+ q63, q64, twenty where the call is long enough)
    want = {9: 5 + wide, 64: 6 + wide + 4 * wide, 65: 7 + wide + 4 * wide, 256: 7 + wide + 4 * wide}
    assert len(L) == sum(want.values())
    counts = [int(_field(l, "count")) for l in L]
    assert 0 in counts and 1 in counts and 8 in counts and (not wide or 4 in counts)
    assert all(_field(l, "outside") == "0" for l in L)


def test_bad_arguments_are_refused_before_any_launch():
    """every refused call: RR_E_INVALID, no word of any output array written, no launch"""
    ref = _lines(_child("listed", KINDS=LISTED_KINDS), "REFUSE")
    assert len(ref) == 11
    for l in ref:
        assert l[1] == "rc=-1" and l[2] == "untouched=1", "|".join(l)
