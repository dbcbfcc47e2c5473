"""The split-operand dense scans -- rr_scan_mfma_x3 (5..16 queries), rr_scan_x3w<1|2> (17..64), their rescoring kernels
rr_rescore_x3 / rr_rescore_x3w, rr_split_queries and the in-kernel query split of the fallback launches -- ONE launch at a
time against tests/x3_model.py (librr_hip_dbg.so: rr_debug_x3_scan, rr_debug_x3_rescore; both launch through the helpers the
product calls).  fp32 and bf16 storage, each at nq = 5, 16, 17, 32, 33, 64: both ends of every kernel's range.  The kernel cases
run in one child process that prints one line per launch; the tests assert on the lines.  tests/test_x3_model.py shows on the
CPU that the model alone passes each check and that every single-term loss, the two-term split and a wrong plane order fail.

a  bitwise, one product per output (467 one-hot rows: every dim, every row position of a tile, ragged 16/32/64-row tiles):
   every stored score equals the model's bits, rows past n are -inf, the planes equal the model's, and nothing outside
   [0, n_pad) x the launch's query slots (scores), the maxima and the keys of the launch is written.
b  one product per output, full mantissas on both sides, exponents over +-40: |score - a q| / |a q| <= ONE_PRODUCT_BAR
   (x3_model.py: 2^-21 for the dropped terms + 6 accumulator roundings of 2^-24 = 8.37e-7; every defect is >= 4.1e-6).
c  dense data against float64, max |score - float64| / sum |a_k q_k| per data set, n in {64, 65, 79, 80, 127, 129, 1000}.  Bar:
   4 x the error of numpy's float32 product on the same data (per data set).  Measured on an MI355X, worst over shapes and
   query counts -- kernel | float32 | two-term defect (least):
                     fp32 rows                              bf16 rows
       unit          2.77e-7 | 2.27e-7 | 5.08e-6            1.97e-7 | 2.47e-7 | 2.88e-6
       wide          2.45e-7 | 2.73e-7 | 5.38e-6            1.56e-7 | 2.74e-7 | 3.18e-6
       cancelling    4.67e-7 | 6.28e-7 | 1.12e-5            3.05e-7 | 5.43e-7 | 6.73e-6
   The two-term defect is at least 2.9 bars out on every data set (5.0 on fp32 rows); the single-term losses are not all that
   far out on dense data (a lost a1q3 is ~8e-7 on unit rows): case b is what catches those.  Case b measured 4.77e-7 (fp32
   rows) and 1.13e-7 (bf16 rows) against the bar of 8.37e-7.
d  maxima and groups (2013 rows, a grid of one CU's share: tiles_per_wave >= 2, asserted): the maximum of a group planted in
   the first / the last M-tile of a run, in the ragged last tile, a tie between two M-tiles; every M-tile maximum (both
   layouts), every tile maximum and every group key, in mode 0 and in mode 1, equals the maximum of the mode-1 stored scores
   over its rows bit for bit; mode 2 stores mode 1's bits for flagged queries and writes nothing when no flag is up.
e  rescoring: lists with the ragged last M-tile, both halves of 32-row tiles, repeats, count = 0, a flagged query: sc equals
   the mode-1 stored scores bit for bit, -inf past n, the sentinel everywhere else.
f  non-finite rows (a NaN, +inf, -inf, +inf and -inf, an overflowing product; full and ragged tiles), kernel level: the mode-0
   maxima are the maxima of the scores the rescoring returns (tau is a lower bound), and through the public API (no child
   process): the head (+inf) and the tail (-inf) of every query's ranking hold the same rows in batches of 1, 4, 5, 16, 17,
   64 as alone, the finite rows between satisfy assert_topk_matches against float64.  With pool = n <= 2048 the product
   serves every batch by the per-row-chain scans (too few tiles per pool row for anything else); the second public case
   (8205 rows, pool 16) is the one a batch reaches the matrix-core path with.  There a matrix with an infinite row norm used to
   take the split-operand scans, which give an fp32 row with an inf element -inf whatever its sign (the KINDS lines of the
   kernel-level case record exactly that), while alone the row scores +-inf; such matrices now take the VALU scans.
"""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import x3_model as M
from parity import assert_topk_matches
from review_recommender_amd.index import ProductIndex

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)

CHILD = r"""
import os, sys
os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, @ROOT@); sys.path.insert(0, os.path.join(@ROOT@, "tests"))
import ctypes as C
import numpy as np, torch
import x3_model as M
from review_recommender_amd import _lib
from review_recommender_amd.index import ProductIndex
lib = _lib.load()
dev = torch.device("cuda", 0)
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
HOST_FILL = np.uint32(0x11111111)
DT = ((False, "fp32"), (True, "bf16"))

def make_index(V, bf16):
    # -> the index (scratch allocated by one 64-query search) and the rows it stores, as float32 values
    t = torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32)).to(dev)
    if bf16:
        tb = t.to(torch.bfloat16).contiguous()
        ix = ProductIndex(None, n_rows=len(V), dim=384, device_ptr=tb.data_ptr(), keepalive=tb, dtype="bf16")
        stored = tb.float().cpu().numpy()
        fin = np.isfinite(V)
        assert (stored.view(np.uint32)[fin] == M.round_to_bf16(V).view(np.uint32)[fin]).all()
    else:
        ix, stored = ProductIndex(V), np.ascontiguousarray(V, dtype=np.float32)
    ix.dense_topk(np.zeros((64, 384), dtype=np.float32), 1)
    return ix, stored

def scan(ix, Q, mode, flags=None, full=True):
    # one launch; full: every word of the three buffers comes back, else only what the launch may write
    nq = len(Q)
    dq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    torch.cuda.synchronize()
    n_tiles = (ix.n_rows + 63) // 64
    QN = M.slots_of(nq, mode == 2)
    caps = (64 * 64 * n_tiles, 128 * n_tiles * 4 + 8192 * 128, 2 * 128 * 8192) if full else (QN * 64 * n_tiles, QN * 4 * n_tiles, QN * 8192)
    sims, gmax, smax = (np.full(c, HOST_FILL, dtype=np.uint32) for c in caps)
    planes = np.full((3, QN, 384), 0x1111, dtype=np.uint16)
    geom = np.zeros(10, dtype=np.int64)
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.int32)
    _lib.check(lib.rr_debug_x3_scan(ix.handle, C.c_void_p(dq.data_ptr()), nq, mode, P(fl), P(geom), P(sims), len(sims), P(gmax), len(gmax),
                                    P(smax), len(smax), P(planes)), "rr_debug_x3_scan")
    g = dict(zip(("n_rows", "n_tiles", "tiles_per_wave", "n_waves", "qs", "mm_pairs", "sims_words", "gmax_words", "smax_words", "QN"),
                 geom.tolist()))
    assert g["QN"] == QN and g["qs"] == QN and g["n_tiles"] == n_tiles and g["n_rows"] == ix.n_rows
    if full:
        assert (g["sims_words"], g["gmax_words"], g["smax_words"]) == caps, (g, caps)
    return g, sims, gmax, smax, planes

def extents(g, mode):
    # words of (scores, maxima, keys) the launch writes
    QN, T = g["QN"], g["n_tiles"]
    return (0 if mode == 0 else QN * 64 * T, QN * 4 * T if mode == 0 else QN * T, QN * g["n_waves"])

def outside(g, mode, sims, gmax, smax):
    # words outside the launch's extents that are no longer the sentinel
    e = extents(g, mode)
    return int((sims[e[0]:] != M.SC_SENTINEL).sum() + (gmax[e[1]:] != M.SC_SENTINEL).sum() + (smax[e[2]:] != M.KEY_SENTINEL).sum())

def stored_scores(g, sims):
    return M.decode_sims(sims, 64 * g["n_tiles"], g["QN"])            # bits [QN][n_pad]

def plane_diff(g, planes, Q, bf16):
    return int((planes != M.planes(Q, g["QN"], M.order_of(g["QN"], bf16))).sum())

def bitwise_case(tag, ix, stored, Q, bf16):
    n, nq = len(stored), len(Q)
    g, sims, gmax, smax, planes = scan(ix, Q, 1)
    S = stored_scores(g, sims)
    exp = M.kept_sum(stored, Q, bf16).astype(np.float32).view(np.uint32)
    bad = int((S[:nq, :n] != exp).sum())
    pad = int((S[:, n:] != M.NEG_INF_BITS).sum())
    zero = int(((S[nq:, :n] & np.uint32(0x7FFFFFFF)) != 0).sum())     # the zero queries of the unused slots
    print(f"BIT|{tag}|nq={nq}|QN={g['QN']}|bad={bad}|pad_rows={pad}|zero_slots={zero}|outside={outside(g, 1, sims, gmax, smax)}|"
          f"planes={plane_diff(g, planes, Q, bf16)}|checked={exp.size}", flush=True)
    if bad:
        q, r = np.argwhere(S[:nq, :n] != exp)[0]
        print(f"FIRST|{tag}|nq={nq}|query {q} row {r}: kernel {S[q, r]:#010x}, model {exp[q, r]:#010x}", flush=True)

def run_a():
    for bf16, dt in DT:
        for name, fill in (("i", M.fill_i), ("ii", M.fill_ii), ("iii", M.fill_iii)):
            if name == "ii" and bf16:
                continue
            A, _ = fill(64, 40)
            ix, stored = make_index(A, bf16)
            for nq in M.NQS:
                bitwise_case(f"{name}|{dt}", ix, stored, fill(nq, 40 + nq)[1], bf16)
            if name == "i":                                            # the normal scan writes no score and only its maxima
                for nq in M.NQS:
                    Q = fill(nq, 40 + nq)[1]
                    g, sims, gmax, smax, planes = scan(ix, Q, 0)
                    e = extents(g, 0)
                    unwritten = int((gmax[:e[1]] == M.SC_SENTINEL).sum() + (smax[:e[2]] == M.KEY_SENTINEL).sum())
                    print(f"BIT0|{dt}|nq={nq}|outside={outside(g, 0, sims, gmax, smax)}|unwritten={unwritten}|"
                          f"planes={plane_diff(g, planes, Q, bf16)}", flush=True)
            ix.close()

def run_b():
    for bf16, dt in DT:
        A, _ = M.fill_b(64, 100)
        ix, stored = make_index(A, bf16)
        n = len(A)
        for nq in M.NQS:
            Q = M.fill_b(nq, 100 + nq)[1]
            g, sims, gmax, smax, planes = scan(ix, Q, 1, full=False)
            S = stored_scores(g, sims)[:nq, :n].view(np.float32).astype(np.float64)
            exact = Q.astype(np.float64) @ stored.astype(np.float64).T
            err = float((np.abs(S - exact) / np.abs(exact)).max())
            print(f"ONE|{dt}|nq={nq}|err={err:.4e}|bar={M.ONE_PRODUCT_BAR:.4e}|products={exact.size}", flush=True)
        ix.close()

def run_c():
    Q64 = M.dense_queries(64, 3)
    for bf16, dt in DT:
        for kind in M.DENSE_KINDS:
            for n in M.DENSE_SHAPES:
                A = M.dense_rows(kind, n, Q64, 3 + n)
                ix, stored = make_index(A, bf16)
                f32_err = M.rel_error(M.f32_matvec(stored, Q64), stored, Q64)        # the yardstick, once per data set
                two = M.rel_error(M.kept_sum(stored, Q64, bf16, two_term=True), stored, Q64)
                for nq in M.NQS:
                    Q = Q64[:nq]
                    g, sims, gmax, smax, planes = scan(ix, Q, 1, full=False)
                    S = stored_scores(g, sims)[:nq, :n].view(np.float32)
                    print(f"DENSE|{kind}|{dt}|n={n}|nq={nq}|kernel={M.rel_error(S, stored, Q):.4e}|float32={f32_err:.4e}|two_term={two:.4e}",
                          flush=True)
                ix.close()

def eq_count(got_bits, want_f32, nq):
    # bits for the launch's queries; values for the unused slots (a zero score may carry either sign)
    bad = int((got_bits[:nq] != want_f32[:nq].view(np.uint32)).sum())
    return bad + int((got_bits[nq:].view(np.float32) != want_f32[nq:]).sum())

def maxima_check(tag, g, mode, S1f, gmax, smax, nq):
    # S1f: the mode-1 stored scores [QN][n_pad] as float32 (slots of this launch)
    T, QN = g["n_tiles"], g["QN"]
    m16, m64, keys = M.maxima_of(S1f, T, g["tiles_per_wave"], g["n_waves"])
    if mode == 0:
        bad_m = eq_count(M.decode_mtile_max(gmax, T, QN, g["mm_pairs"]), m16, nq)
    else:
        bad_m = eq_count(M.decode_tile_max(gmax, T, QN), m64, nq)
    k = M.decode_keys(smax, g["n_waves"], QN)
    bad_k = int((k[:nq] != keys[:nq]).sum()) + int((k[nq:] == M.KEY_SENTINEL).sum())      # (unused slots: written)
    print(f"MAX|{tag}|mode={mode}|nq={nq}|tpw={g['tiles_per_wave']}|waves={g['n_waves']}|mm_pairs={g['mm_pairs']}|maxima={bad_m}|keys={bad_k}",
          flush=True)

def rescore(ix, Q, mt, count, fb):
    dq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    torch.cuda.synchronize()
    sc = np.full(mt.shape + (16,), HOST_FILL, dtype=np.uint32)
    _lib.check(lib.rr_debug_x3_rescore(ix.handle, C.c_void_p(dq.data_ptr()), len(Q), P(mt), mt.shape[1], P(count), P(fb), P(sc)),
               "rr_debug_x3_rescore")
    return sc

def run_de():
    Q64 = M.dense_queries(64, 9)
    A0 = M.maxima_matrix()
    n = len(A0)
    for bf16, dt in DT:
        for cls in ((5, 16), (17, 32), (33, 64)):
            base, _ = make_index(A0, bf16)
            _lib.check(lib.rr_index_set_scan_cus(base.handle, 1), "rr_index_set_scan_cus")
            C0 = scan(base, Q64[:cls[0]], 0, full=False)[0]["tiles_per_wave"]
            base.close()
            A, planted = M.maxima_plants(A0, Q64, C0)
            ix, stored = make_index(A, bf16)
            _lib.check(lib.rr_index_set_scan_cus(ix.handle, 1), "rr_index_set_scan_cus")
            for nq in cls:
                Q = Q64[:nq]
                tag = f"{dt}"
                g1, sims, gmax, smax, planes = scan(ix, Q, 1)
                S1 = stored_scores(g1, sims)
                S1f = S1.view(np.float32)
                print(f"GEOM|{tag}|nq={nq}|tpw={g1['tiles_per_wave']}|planted_for={C0}|outside={outside(g1, 1, sims, gmax, smax)}|"
                      f"planes={plane_diff(g1, planes, Q, bf16)}|err64={M.rel_error(S1f[:nq, :n], stored, Q):.3e}", flush=True)
                maxima_check(tag, g1, 1, S1f, gmax, smax, nq)
                # the plants: each is its query's best row, alone in its M-tile; the tie sits in two M-tiles with the same bits
                m16 = S1f.reshape(g1["QN"], -1, 16).max(axis=2)
                ok = all(S1f[q, r] == S1f[q].max() and m16[q, r // 16] == S1f[q, r] for q, rr in planted.items() for r in rr)
                tie = S1[3, planted[3][0]] == S1[3, planted[3][1]]
                print(f"PLANT|{tag}|nq={nq}|ok={int(ok)}|tie={int(tie)}", flush=True)
                g0, sims0, gmax0, smax0, planes0 = scan(ix, Q, 0)
                print(f"GEOM0|{tag}|nq={nq}|tpw={g0['tiles_per_wave']}|outside={outside(g0, 0, sims0, gmax0, smax0)}|"
                      f"planes={plane_diff(g0, planes0, Q, bf16)}", flush=True)
                maxima_check(tag, g0, 0, S1f, gmax0, smax0, nq)
                # mode 2: the fallback launch (flags + in-kernel split).  Its slots may be more (rr_scan_x3w at any count).
                flags = np.zeros(nq, dtype=np.int32)
                flags[[1, 3, nq - 1]] = 1
                g2, sims2, gmax2, smax2, planes2 = scan(ix, Q, 2, flags=flags)
                S2 = stored_scores(g2, sims2)
                up = np.flatnonzero(flags)
                S2f = S2.view(np.float32)
                # mode 1 of the same kernel: up to 16 queries the fallback is rr_scan_x3w<1> where mode 1 is rr_scan_mfma_x3
                # (another accumulation order), so mode 1 runs on the queries plus zero rows up to 17 -- a score depends
                # only on its own row and query
                S1w = S1 if nq > 16 else stored_scores(*scan(ix, np.concatenate([Q, np.zeros((17 - nq, 384), dtype=np.float32)]), 1, full=False)[:2])
                print(f"FALLBACK|{tag}|nq={nq}|QN={g2['QN']}|tpw={g2['tiles_per_wave']}|differ={int((S2[up] != S1w[up]).sum())}|"
                      f"outside={outside(g2, 1, sims2, gmax2, smax2)}|planes_touched={int((planes2 != M.PLANE_SENTINEL).sum())}", flush=True)
                maxima_check(tag + "|fallback", g2, 1, S2f, gmax2, smax2, nq)
                g3, sims3, gmax3, smax3, planes3 = scan(ix, Q, 2, flags=np.zeros(nq, dtype=np.int32))
                written = int((sims3 != M.SC_SENTINEL).sum() + (gmax3 != M.SC_SENTINEL).sum() + (smax3 != M.KEY_SENTINEL).sum())
                print(f"NOFLAG|{tag}|nq={nq}|written={written}", flush=True)
                # e: rescoring on caller lists
                mt, count, fb = M.rescore_lists(n, nq)
                sc = rescore(ix, Q, mt, count, fb)
                exp = M.rescore_expected(S1, n, mt, count, fb)
                print(f"RESCORE|{tag}|nq={nq}|differ={int((sc != exp).sum())}|listed={int((exp != M.SC_SENTINEL).sum())}|"
                      f"past_end={int((exp == M.NEG_INF_BITS).sum())}", flush=True)
                if (sc != exp).any():
                    q, s, r = np.argwhere(sc != exp)[0]
                    print(f"FIRST|rescore {tag}|nq={nq}|query {q} slot {s} (M-tile {mt[q, s]}) row {r}: kernel {sc[q, s, r]:#010x}, "
                          f"stored {exp[q, s, r]:#010x}", flush=True)
            ix.close()

def run_f():
    A, rows = M.nonfinite_matrix()
    n = len(A)
    n_mt = (n + 15) // 16
    for bf16, dt in DT:
        ix, stored = make_index(A, bf16)
        for nq in M.NQS:
            Q = M.nonfinite_queries(nq)
            mt = np.tile(np.arange(n_mt, dtype=np.uint32), (nq, 1))
            count, fb = np.full(nq, n_mt, dtype=np.int32), np.zeros(nq, dtype=np.int32)
            sc = rescore(ix, Q, mt, count, fb)                           # every row's rescored score: [nq][n_mt][16]
            g1, sims, gmax, smax, _ = scan(ix, Q, 1, full=False)
            S1 = stored_scores(g1, sims)
            same = int((sc.reshape(nq, -1)[:, :n] != S1[:nq, :n]).sum())
            nan = int(np.isnan(sc.view(np.float32)).sum())
            g0, sims0, gmax0, smax0, _ = scan(ix, Q, 0, full=False)
            scf = np.full((g0["QN"], 64 * g0["n_tiles"]), -np.inf, dtype=np.float32)
            scf[:nq, :16 * n_mt] = sc.view(np.float32).reshape(nq, -1)
            m16, m64, keys = M.maxima_of(scf, g0["n_tiles"], g0["tiles_per_wave"], g0["n_waves"])
            got = M.decode_mtile_max(gmax0, g0["n_tiles"], g0["QN"], g0["mm_pairs"])
            bad_m = int((got[:nq] != m16[:nq].view(np.uint32)).sum())
            bad_k = int((M.decode_keys(smax0, g0["n_waves"], g0["QN"])[:nq] != keys[:nq]).sum())
            kinds = "|".join(f"{k}={','.join(str(np.float32(sc.view(np.float32)[0].reshape(-1)[r])) for r in rr)}" for k, rr in rows.items())
            print(f"NONFINITE|{dt}|nq={nq}|rescored_vs_stored={same}|nan_scores={nan}|maxima={bad_m}|keys={bad_k}", flush=True)
            if nq == 5:
                print(f"KINDS|{dt}|{kinds}", flush=True)
        ix.close()

def refuse(name, call):
    try:
        call()
        print(f"REFUSE|{name}|accepted", flush=True)
    except ValueError as e:
        print(f"REFUSE|{name}|refused|{str(e)[:100]}", flush=True)

def run_refusals():
    A = M.unit_rows(200, 1)
    ix, _ = make_index(A, False)
    Q = M.dense_queries(17, 1)
    dq = torch.from_numpy(Q).to(dev)
    buf = np.zeros(16, dtype=np.uint32)
    pl = np.zeros((3, 64, 384), dtype=np.uint16)
    geom = np.zeros(10, dtype=np.int64)
    fl = np.zeros(17, dtype=np.int32)
    def sc(nq, mode, flags, cap=16):
        return lambda: _lib.check(lib.rr_debug_x3_scan(ix.handle, C.c_void_p(dq.data_ptr()), nq, mode, P(flags), P(geom), P(buf), cap, P(buf), 16,
                                                       P(buf), 16, P(pl)), "rr_debug_x3_scan")
    refuse("nq=4", sc(4, 0, None)); refuse("nq=65", sc(65, 0, None)); refuse("mode=3", sc(17, 3, None))
    refuse("mode 2 without flags", sc(17, 2, None)); refuse("mode 1 with flags", sc(17, 1, fl)); refuse("cap beyond the buffer", sc(17, 1, None, 1 << 40))
    mt = np.zeros((17, 4), dtype=np.uint32); cnt = np.ones(17, dtype=np.int32); fb0 = np.zeros(17, dtype=np.int32)
    out = np.zeros((17, 4, 16), dtype=np.uint32)
    def rs(mt_, cnt_):
        return lambda: _lib.check(lib.rr_debug_x3_rescore(ix.handle, C.c_void_p(dq.data_ptr()), 17, P(mt_), 4, P(cnt_), P(fb0), P(out)), "rr_debug_x3_rescore")
    bad_mt = mt.copy(); bad_mt[3, 0] = 13                                # 200 rows: M-tiles 0..12
    refuse("M-tile past the end", rs(bad_mt, cnt))
    bad_cnt = cnt.copy(); bad_cnt[2] = 5
    refuse("count beyond cap", rs(mt, bad_cnt))
    fresh = ProductIndex(A)                                              # no batched search yet: no scratch
    refuse("no scratch", lambda: _lib.check(lib.rr_debug_x3_scan(fresh.handle, C.c_void_p(dq.data_ptr()), 17, 0, None, P(geom), P(buf), 16, P(buf), 16,
                                                                P(buf), 16, P(pl)), "rr_debug_x3_scan"))
    fresh.close(); ix.close()

for part in (run_refusals, run_a, run_b, run_c, run_de, run_f):
    part()
    print(f"PART|{part.__name__}|done", flush=True)
print("DONE", flush=True)
"""


def _lines(out: str, tag: str):
    return [l.split("|")[1:] for l in out.splitlines() if l.startswith(tag + "|")]


def _f(line, name):
    return [f.split("=", 1)[1] for f in line if f.startswith(name + "=")][0]


def _zero(out, tag, names, n_lines):
    lines = _lines(out, tag)
    assert len(lines) == n_lines, (tag, len(lines), n_lines)
    first = "\n".join("|".join(l) for l in _lines(out, "FIRST")[:8])
    for l in lines:
        for name in names:
            assert _f(l, name) == "0", f"{tag}|" + "|".join(l) + "\n" + first
    return lines


@pytest.fixture(scope="module")
def kernels_out():
    from review_recommender_amd.build import DEBUG_LIB_PATH
    if not DEBUG_LIB_PATH.exists():
        pytest.skip("librr_hip_dbg.so not built (python review-recommender_amd/build.py --debug)")
    p = subprocess.run([sys.executable, "-c", CHILD.replace("@ROOT@", repr(ROOT))], capture_output=True, text=True, timeout=600)
    print(p.stdout[-20000:])
    assert p.returncode == 0 and "DONE" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


N_DT_NQ = 2 * len(M.NQS)


def test_x3_scans_one_product_per_output_bit_for_bit(kernels_out):
    lines = _zero(kernels_out, "BIT", ("bad", "pad_rows", "zero_slots", "outside", "planes"), 5 * len(M.NQS))
    assert {(l[0], l[1]) for l in lines} == {("i", "fp32"), ("ii", "fp32"), ("iii", "fp32"), ("i", "bf16"), ("iii", "bf16")}
    assert {(int(_f(l, "nq")), int(_f(l, "QN"))) for l in lines} == {(5, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64)}
    assert all(int(_f(l, "checked")) == int(_f(l, "nq")) * M.ONEHOT_ROWS for l in lines)
    _zero(kernels_out, "BIT0", ("outside", "unwritten", "planes"), N_DT_NQ)


def test_x3_scans_one_full_mantissa_product_per_output(kernels_out):
    """|score - a_k q_k| <= ONE_PRODUCT_BAR |a_k q_k|: derived in x3_model.py (dropped terms < 2^-21, six accumulator
    roundings of 2^-24), not measured; test_x3_model.py: no defect comes within 4x of it."""
    lines = _lines(kernels_out, "ONE")
    assert len(lines) == N_DT_NQ
    for l in lines:
        assert int(_f(l, "products")) == int(_f(l, "nq")) * M.ONEHOT_ROWS
        assert float(_f(l, "err")) <= M.ONE_PRODUCT_BAR, "|".join(l)
    print("worst one-product error:", {dt: max(float(_f(l, "err")) for l in lines if l[0] == dt) for dt in ("fp32", "bf16")})


def test_x3_scans_dense_data_against_float64(kernels_out):
    lines = _lines(kernels_out, "DENSE")
    assert len(lines) == len(M.DENSE_KINDS) * len(M.DENSE_SHAPES) * N_DT_NQ
    worst = {}
    for l in lines:
        k, f, t = float(_f(l, "kernel")), float(_f(l, "float32")), float(_f(l, "two_term"))
        w = worst.setdefault((l[0], l[1]), [0.0, 0.0, np.inf, np.inf])
        w[0], w[1], w[2], w[3] = max(w[0], k), max(w[1], f), min(w[2], t), min(w[3], t / (4 * f))
        assert 0 < f < 1e-5 and k <= 4 * f, "|".join(l)
    for key, w in sorted(worst.items()):
        print(f"{key[0]:10s} {key[1]}: kernel {w[0]:.3e} | float32 {w[1]:.3e} | two-term defect >= {w[2]:.3e} ({w[3]:.2f} bars)")


def test_x3_scans_maxima_groups_and_the_fallback_launch(kernels_out):
    for tag in ("GEOM", "GEOM0"):
        for l in _zero(kernels_out, tag, ("outside", "planes"), N_DT_NQ):
            assert int(_f(l, "tpw")) >= 2, "|".join(l)
    for l in _lines(kernels_out, "GEOM"):
        assert _f(l, "tpw") == _f(l, "planted_for") and float(_f(l, "err64")) < 1e-6, "|".join(l)
    lines = _zero(kernels_out, "MAX", ("maxima", "keys"), 3 * N_DT_NQ)
    assert {(_f(l, "mode"), _f(l, "mm_pairs")) for l in lines if "fallback" not in l} >= {("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")}
    assert all(int(_f(l, "tpw")) >= 2 for l in lines)
    for l in _lines(kernels_out, "PLANT"):
        assert _f(l, "ok") == "1" and _f(l, "tie") == "1", "|".join(l)
    assert len(_lines(kernels_out, "PLANT")) == N_DT_NQ
    _zero(kernels_out, "FALLBACK", ("differ", "outside", "planes_touched"), N_DT_NQ)
    assert {(int(_f(l, "nq")), int(_f(l, "QN"))) for l in _lines(kernels_out, "FALLBACK")} == {(5, 32), (16, 32), (17, 32), (32, 32), (33, 64), (64, 64)}
    _zero(kernels_out, "NOFLAG", ("written",), N_DT_NQ)


def test_x3_rescoring_repeats_the_stored_scores_bit_for_bit(kernels_out):
    for l in _zero(kernels_out, "RESCORE", ("differ",), N_DT_NQ):
        assert int(_f(l, "listed")) >= 16 * 38 and int(_f(l, "past_end")) >= 3 * 3, "|".join(l)


def test_x3_maxima_bound_the_rescored_scores_on_non_finite_rows(kernels_out):
    _zero(kernels_out, "NONFINITE", ("rescored_vs_stored", "nan_scores", "maxima", "keys"), N_DT_NQ)
    assert len(_lines(kernels_out, "KINDS")) == 2
    for l in _lines(kernels_out, "KINDS"):
        # fp32 rows: the split of an inf element is (inf, NaN, NaN), so every such row is -inf here, whatever its sign.  (bf16
        # rows: inf times the three query terms, NaN only where one of them is zero -- the line is a record.)
        if l[0] == "fp32":
            assert all(v == "-inf" for f in l[1:] if not f.startswith("overflow") for v in f.split("=", 1)[1].split(",")), "|".join(l)


def test_x3_harness_entries_refuse_bad_arguments(kernels_out):
    lines = _lines(kernels_out, "REFUSE")
    assert len(lines) == 9
    for l in lines:
        assert l[1] == "refused", "|".join(l)


# ---- f, through the public API
def _single(ix, Q, pool):
    out = [ix.dense_topk(Q[i:i + 1], pool) for i in range(len(Q))]
    return np.concatenate([r for r, _ in out]), np.concatenate([s for _, s in out])


def _ranking_reference(A_stored, Q, rows1, scores1):
    """float64 scores with +inf / -inf where the single-query search ranks a row first / last (its own arithmetic decides
    what overflows); -> ref [nq][n], head rows, tail rows per query."""
    n = len(A_stored)
    fin = np.isfinite(A_stored).all(axis=1)
    ref = np.full((len(Q), n), np.nan)
    ref[:, fin] = Q.astype(np.float64) @ A_stored[fin].astype(np.float64).T
    heads, tails = [], []
    for q in range(len(Q)):
        s = np.empty(n, dtype=np.float32)
        s[rows1[q]] = scores1[q]
        ref[q, s == np.inf], ref[q, s == -np.inf] = np.inf, -np.inf
        heads.append(set(np.flatnonzero(s == np.inf).tolist()))
        tails.append(set(np.flatnonzero(s == -np.inf).tolist()))
    assert not np.isnan(ref).any()
    return ref, heads, tails


def _reference_with_non_finite(stored, Q, kinds):
    """float64 scores [nq][n]; a row with non-finite elements: the IEEE sum of its products (inf - inf and NaN rank last: -inf);
    an overflow row: the sign of its +-3e38 element times inf (1.5 x 3e38 is beyond fp32)."""
    fin = np.isfinite(stored).all(axis=1)
    Q64 = Q.astype(np.float64)
    ref = np.full((len(Q), len(stored)), -np.inf)
    ref[:, fin] = Q64 @ stored[fin].astype(np.float64).T
    with np.errstate(invalid="ignore"):
        for r in np.flatnonzero(~fin):
            v = (Q64 * stored[r].astype(np.float64)[None, :]).sum(axis=1)
            ref[:, r] = np.where(np.isnan(v), -np.inf, v)
    for r in kinds.get("overflow", ()):
        ref[:, r] = np.sign(stored[r, 0]) * np.inf
    return ref


def _assert_finite_part(rows, scores, ref_q):
    """assert_topk_matches for the finite stretch of a ranking: the rows at +-inf are taken out of the reference."""
    r = np.where(np.isfinite(ref_q), ref_q, -np.inf)
    assert np.isfinite(r[rows]).all()
    assert_topk_matches(rows, scores, r, len(rows))


def _assert_head_then_finite(rows, scores, ref_q, pool):
    """The rows at +inf (fewer than the pool) lead in ascending row order, the rest of the pool satisfies assert_topk_matches."""
    head = np.flatnonzero(ref_q == np.inf)
    h = len(head)
    assert 0 < h < pool and rows[:h].tolist() == head.tolist() and (scores[:h] == np.inf).all(), (rows, scores, head)
    _assert_finite_part(rows[h:], scores[h:], ref_q)


def _make(A, dtype):
    # -> the index and the rows it stores, as float32 values
    if dtype == "bf16":
        return ProductIndex.from_rows(A, dtype="bf16"), M.round_to_bf16(A)
    return ProductIndex(A), A


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_non_finite_rows_rank_the_same_alone_and_in_any_batch(dtype):
    A, kinds = M.nonfinite_matrix()
    n = len(A)
    ix, stored = _make(A, dtype)
    Q = M.nonfinite_queries(64)
    rows1, scores1 = _single(ix, Q, n)
    ref, heads, tails = _ranking_reference(stored, Q, rows1, scores1)
    special = {r for rr in kinds.values() for r in rr}
    for q in range(64):
        assert len(heads[q]) >= 2 and len(tails[q]) >= len(kinds["nan"]) + 2 and (heads[q] | tails[q]) <= special
        assert set(kinds["nan"]) <= tails[q]
    for batch in (1, 4, 5, 16, 17, 64):
        rows, scores = ix.dense_topk(Q[:batch], n)
        for q in range(batch):
            h, t = len(heads[q]), len(tails[q])
            assert set(rows[q, :h].tolist()) == heads[q] and (scores[q, :h] == np.inf).all(), (batch, q)
            assert set(rows[q, n - t:].tolist()) == tails[q] and (scores[q, n - t:] == -np.inf).all(), (batch, q)
            assert np.isfinite(scores[q, h:n - t]).all()
            _assert_finite_part(rows[q, h:n - t], scores[q, h:n - t], ref[q])
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_inf_rows_lead_a_batch_that_reaches_the_matrix_cores(dtype):
    """8205 rows at pool 16 (129 tiles = 8 per pool row, the least the batched paths take): enough tiles per pool row for a batch of five or more to leave the per-row-chain scans.  A matrix
    with an infinite row norm has no filter bound; it must not take the split-operand scans either, where its inf rows score
    NaN and rank last (the kernel-level KINDS lines show it).  A matrix whose only non-finite rows are NaN rows stays on them."""
    pool = 16
    A, kinds = M.nonfinite_matrix(n=8192 + 13)
    ix, stored = _make(A, dtype)
    Q = M.nonfinite_queries(64)
    rows1, scores1 = _single(ix, Q, pool)
    assert (scores1[:, 0] == np.inf).all()
    n = len(A)
    ref = _reference_with_non_finite(stored, Q, kinds)
    for q in range(64):
        _assert_head_then_finite(rows1[q], scores1[q], ref[q], pool)
    for batch in (5, 16, 17, 64):
        rows, scores = ix.dense_topk(Q[:batch], pool)
        assert ix.last_scan_info()[0] in (1, 2), ix.last_scan_info()                          # the VALU scans
        for q in range(batch):
            _assert_head_then_finite(rows[q], scores[q], ref[q], pool)
            assert rows[q].tolist() == rows1[q].tolist() and (scores[q].view(np.uint32) == scores1[q].view(np.uint32)).all()
    ix.close()
    A2, kinds2 = M.nonfinite_matrix(kinds=("nan",), n=8192 + 13)
    ix2, stored2 = _make(A2, dtype)
    ref2 = _reference_with_non_finite(stored2, Q, kinds2)
    for batch in (5, 17, 64):
        rows, scores = ix2.dense_topk(Q[:batch], pool)
        assert ix2.last_scan_info()[0] in (3, 4), ix2.last_scan_info()                        # the split-operand scans
        for q in range(batch):
            assert_topk_matches(rows[q], scores[q], ref2[q], pool)
    ix2.close()
