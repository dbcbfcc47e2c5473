"""The filter scans (csrc/rr_dense_flt.hip: rr_scan_flt, rr_scan_flt16, the two-set rr_scan_fltq with the C++ bodies
and with the generated loop) one launch at a time against float64: EVERY tile word and EVERY group key a launch leaves is
decoded and held against properties P1..P6 of flt_words_model.check_words (safe and tight maximum, safe and tight gaps,
group maxima, ragged end / NaN / sentinel), then the product's selection (rr_select_mtiles) is run on those words and its
lists, thresholds and flags are held against the same reference.

Each group of cases runs in a child process on the harness library (librr_hip_dbg.so: rr_debug_flt_words,
rr_debug_flt_select, rr_debug_fltq_compare, rr_debug_select_traces), with its own timeout; M8 and delta come from torch
float64 on the device.  The children print one line per launch: kernel, words and keys checked, violations, the worst
tight margin (bound - M8) / step and the worst safe margin (M8 - bound) / delta.

rr_scan_fltq row counts follow the geometry the entry point reports (R runs): R k tiles of 64 rows minus 27 rows (a short
last M-tile) for k tiles per run with 2 k < 6 M-tiles (C++ bodies only), and k for which the four-body loop of a run is
entered with 0, 1 and 2 iterations (the child replays rr_scan_fltq's loop-entry rule on the reported geometry and asserts the
shape it meant to hit); one count with fewer tiles than R.

Worst margins on hardware (a record, not a bar: the bars are the derived ones), over all launches of a kernel -- words
checked, tight side (bound - M8) / step, safe side (M8 - bound) / delta (P2 allows 1):
    rr_scan_flt               5.6M words   2.580   0.002
    rr_scan_flt16            55.1M words   5.230   0.003
    rr_scan_fltq<false>      53.9M words   5.493   0.003
    rr_scan_fltq<true>       78.1M words   5.493   0.003
(the tight side is largest on bf16 storage with rows of norm 0.01 .. 30: one bf16 ulp of a large mx is several steps of the
launch's smallest eps.)  On the first run rr_scan_flt and rr_scan_flt16 left bit-identical words and keys (pinned below), as did
rr_scan_fltq's generated loop and its C++ bodies.

Kernel-side mutations, each applied to the debug library alone, run against one test and reverted:
    rr_flt_gap_code rounding up (8.0f -> 8.999f)      every-scan[f32-unit] fails: "10708 x P2 (low)" .. "68530 x P2 (low)"
    rr_scan_flt16 stores the word for mt, not mt - 1  every-scan[f32-unit] fails: "P1 (low) ; P2 (low) ; P4 (high)", tile 0 on
    prefilter reads sigma of 32-query group t + 1     prefilter test fails: "1085160 x P6 (sentinel)" (40 and 100 queries)
"""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)

COMMON = r"""
import os, sys
os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, @ROOT@); sys.path.insert(0, os.path.join(@ROOT@, "tests"))
import ctypes as C
import numpy as np, torch
import flt_words_model as M
from review_recommender_amd import _lib
from review_recommender_amd.index import ProductIndex
lib = _lib.load()
dev = torch.device("cuda", 0)
KERNEL = {0: "rr_scan_flt", 1: "rr_scan_flt16", 3: "rr_scan_fltq<false>", 4: "rr_scan_fltq<true>"}      # (2 was the two-set rr_scan_flt16)
GN = ["n_rows", "n_tiles", "tiles_per_wave", "n_waves", "gpw", "tiles_per_group", "stride", "words_per_set", "keys_per_set", "sets",
      "prefilter", "nq2", "word_sentinel", "key_sentinel", "word_set_stride", "key_set_stride"]
P = lambda a: a.ctypes.data_as(C.c_void_p)
import re
_csrc = os.path.join(@ROOT@, "review-recommender_amd", "csrc")
CAPS = {name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", open(os.path.join(_csrc, f)).read()).group(1))
        for name, f in (("RR_X3_MCAP", "rr_dense.h"), ("RR_SEL_LCAP", "rr_dense.hip"))}

def unit_rows(n, seed, lo=None, hi=None):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    m = torch.randn((n, 384), generator=g, device=dev)
    m /= m.norm(dim=1, keepdim=True)
    if lo is not None:                           # norms log-uniform in [lo, hi]
        m *= torch.exp(torch.rand((n, 1), generator=g, device=dev) * np.log(hi / lo) + np.log(lo))
    return m

def queries(nq, seed, mat, norm=7.5, rows=()):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    q = torch.randn((nq, 384), generator=g, device=dev)
    q *= norm / q.norm(dim=1, keepdim=True)
    for i, r in rows:                            # a query that is a row
        v = mat[r].float()
        q[i] = v * (norm / v.norm())
    return q.contiguous()

def make_index(mat, bf16):
    # -> index, its rows as bf16 (what every filter scan multiplies); .row_norm = float64 max ||a|| of the STORED rows
    if bf16:
        mb = mat.to(torch.bfloat16).contiguous()
        ix, stored = ProductIndex(None, n_rows=len(mb), dim=384, device_ptr=mb.data_ptr(), keepalive=mb, dtype="bf16"), mb
    else:
        ix, stored, mb = ProductIndex(None, n_rows=len(mat), dim=384, device_ptr=mat.data_ptr(), keepalive=mat), mat, mat.to(torch.bfloat16)
    mb.row_norm = max(float(stored[s:s + 262144].double().norm(dim=1).max()) for s in range(0, len(stored), 262144))
    return ix, mb

def warm(ix, pool=10):
    ix.dense_topk(np.random.default_rng(0).standard_normal((64, 384)).astype(np.float32), pool)     # (allocates the scratch)

def reference(a_bf16, q, T):
    # M8[tile, 4, query] and delta (flt_words_model's docstring) in float64 on the device, 8192 tiles of 32 rows at a time
    qb = q.to(torch.bfloat16).double()
    n, nq = len(a_bf16), len(q)
    M8, D = np.empty((T, 4, nq)), np.empty((T, 4, nq))
    for t0 in range(0, T, 8192):
        t1 = min(t0 + 8192, T)
        a = a_bf16[32 * t0:min(32 * t1, n)].double()
        sc = torch.full((32 * (t1 - t0), nq), -float("inf"), dtype=torch.float64, device=dev)
        mg = torch.zeros((32 * (t1 - t0), nq), dtype=torch.float64, device=dev)
        sc[:len(a)] = a @ qb.T
        mg[:len(a)] = a.abs() @ qb.abs().T
        M8[t0:t1] = sc.view(t1 - t0, 4, 8, nq).amax(dim=2).cpu().numpy()
        D[t0:t1] = (M.GAMMA_384 * mg.view(t1 - t0, 4, 8, nq).amax(dim=2)).cpu().numpy()
    return M8, D

def geometry(ix, nq_a, nq_b, scan):
    g = (C.c_int64 * 16)()
    _lib.check(lib.rr_debug_flt_words(ix.handle, None, nq_a, nq_b, scan, 0, 150, g, None, None, None, 0, None, 0), "rr_debug_flt_words")
    return dict(zip(GN, list(g)))

def scan_words(ix, q, nq_a, nq_b, scan, prefilter=0, pool=150):
    G = geometry(ix, nq_a, nq_b, scan)
    words = np.empty(G["sets"] * G["words_per_set"], dtype=np.uint32)
    keys = np.empty(G["sets"] * G["keys_per_set"], dtype=np.uint32)
    eps, sigma, g = np.empty(256, dtype=np.float32), np.empty(256, dtype=np.float32), (C.c_int64 * 16)()
    _lib.check(lib.rr_debug_flt_words(ix.handle, C.c_void_p(q.data_ptr()), nq_a, nq_b, scan, prefilter, pool, g, P(eps), P(sigma),
                                      P(words), words.size, P(keys), keys.size), "rr_debug_flt_words")
    G = dict(zip(GN, list(g)))
    return G, eps, sigma, words.reshape(G["sets"], 2 * G["n_tiles"], G["stride"]), keys.reshape(G["sets"], -1, G["stride"])

def check_launch(tag, ix, a_bf16, q, nq_a, nq_b, scan, prefilter=0, ref=None, pool=150):
    # one launch, every word and key of it; -> (G, eps, sigma, words, keys, ref, total violations)
    G, eps, sigma, words, keys = scan_words(ix, q, nq_a, nq_b, scan, prefilter, pool)
    T = 2 * G["n_tiles"]
    if ref is None:
        ref = reference(a_bf16, q, T)
    M8, D = ref
    # the derived delta sits inside the 2^-14 ||a|| ||q|| that eps sets aside for the accumulations of scan and chain
    budget = 2.0 ** -14 * a_bf16.row_norm * q.double().norm(dim=1).cpu().numpy()
    assert np.all(D.max(axis=(0, 1)) < budget), "delta exceeds the kernel's own accumulation budget"
    total = 0
    for s, (q0, n) in enumerate([(0, nq_a), (nq_a, nq_b)][:G["sets"]]):
        e = eps[128 * s:128 * s + n]
        w, k = words[s][:, :n], keys[s][:, :n]
        m8, d = M8[:, :, q0:q0 + n], D[:, :, q0:q0 + n]
        may = None
        if G["prefilter"]:
            # a word may stay at the sentinel only if EVERY query of its 32-query group has M32 <= sigma_q + delta
            sg = sigma[:G["stride"]].astype(np.float64)
            low = np.full((T, G["stride"]), True)
            low[:, :n] = (m8 - d).max(axis=1) <= sg[None, :n]
            may = np.repeat(low.reshape(T, -1, 32).all(axis=2), 32, axis=1)[:, :n]
            # (the first M-tile of a wave's run has nothing pending when its store slot comes up: the scans store "-inf, gaps 0"
            #  to the tile's own slot, and only a KEPT first tile overwrites it -- that word is the skip mark of such a tile)
            first = 2 * G["tiles_per_wave"] * np.arange(G["n_waves"])
            w = w.copy()
            w[first] = np.where(w[first] == 0x0000FF80, np.uint32(G["word_sentinel"]), w[first])
        bad, st = M.check_words(w, k, G, m8, d, e, sentinel=G["word_sentinel"], may_skip=may)
        nbad = sum(st["counts"].values())
        total += nbad
        print(f"LAUNCH|{tag}|{KERNEL[scan]}|nq2={G['nq2']}|set {s}|n_rows={G['n_rows']}|queries={n}|words={st['words']}|keys={st['keys']}|"
              f"skipped={st['sentinel_words']}|violations={nbad}|tight_steps={st['tight_steps']:.3f}|safe_delta={st['safe_delta']:.3f}", flush=True)
        if nbad:
            print("VIOLATIONS|" + tag + "|" + M.describe(bad, st).replace("\n", " ;; "), flush=True)
    return G, eps, sigma, words, keys, ref, total

def fltq_compare(tag):
    out = (C.c_int64 * 8)()
    _lib.check(lib.rr_debug_fltq_compare(ix.handle, out), "rr_debug_fltq_compare")
    print(f"COMPARE|{tag}|{out[0]}|{out[1]}|{out[2]}|{out[3]}|first word {out[4]}: {out[5]:#x} vs {out[6]:#x}", flush=True)

def select(ix, nq, pool, cap=16384):
    mt = np.empty((nq, cap), dtype=np.uint32)
    count, fb = np.empty(nq, dtype=np.int32), np.empty(nq, dtype=np.int32)
    tau, opn = np.empty(nq, dtype=np.uint32), np.empty(nq, dtype=np.uint32)
    _lib.check(lib.rr_debug_flt_select(ix.handle, pool, P(mt), cap, P(count), P(tau), P(opn), P(fb)), "rr_debug_flt_select")
    return mt, count, tau, opn, fb

def model_tau(G, m8, d, pool):
    # Where rr_sel_open_groups' tau~ must lie, from the model alone: tau~ is at most the pool-th largest group maximum and
    # at least that value with everything below the 14 bits under the highest bit in which the keys of the groups THAT HOLD
    # TILES differ cleared (rr_dense.hip: "within 2^-14 of the spread of the group maxima").  -> (lowest, highest, up_g)
    ng = G["n_waves"] * G["gpw"]
    lo_g, up_g = np.full(ng, -np.inf), np.full(ng, -np.inf)
    for gi in range(ng):
        a, b = M.group_tiles(G, gi)
        if b > a:
            lo_g[gi], up_g[gi] = (m8[a:b] - d[a:b]).max(), (m8[a:b] + d[a:b]).max()
    has = np.isfinite(up_g)
    assert has.sum() > pool
    f32_down = lambda v: -M.f32_up(-np.float64(v))
    kmax, kmin = int(M.f2key(M.f32_up(up_g[has].max()).reshape(1))[0]), int(M.f2key(f32_down(lo_g[has].min()).reshape(1))[0])
    drop = np.uint32(0xFFFFFFFF) << np.uint32(max((kmax ^ kmin).bit_length() - 1 - 13, 0))
    kth_lo = M.f2key(f32_down(np.sort(lo_g)[-pool]).reshape(1)) & drop
    return np.float64(M.key2f(kth_lo)[0]), np.float64(M.f32_up(np.sort(up_g)[-pool])), up_g

def check_selection(tag, G, eps, sigma, words, ref, nq_a, nq_b, pool, sel, tied=()):
    # rr_select_mtiles' lists, thresholds and flags against the reference, for every query.  `tied`: queries whose may-open
    # list cannot fit (their flag must be up); a query whose sigma sits above its open threshold must be flagged as well.
    mt, count, tau, opn, fb = sel
    M8, D = ref
    T, problems = 2 * G["n_tiles"], []
    for Q in range(nq_a + nq_b):
        s, q = (0, Q) if Q < nq_a else (1, Q - nq_a)
        e = np.float64(eps[128 * s + q])
        step = np.float64(M.gap_step(eps[128 * s:128 * s + (nq_b if s else nq_a)]))
        m8, d = M8[:, :, Q], D[:, :, Q]
        tau_lo, tau_up, up_g = model_tau(G, m8, d, pool)
        open_f, tau_f = np.float64(M.key2f(opn[Q:Q + 1])[0]), np.float64(M.key2f(tau[Q:Q + 1])[0])
        mx, codes, bound = M.decode_words(words[s][:, q:q + 1], step)
        # may-open: the P4 upper limit of the M-tile's decoded bound (a saturated code: the decoded bound itself; an M-tile
        # without real rows has nothing but its saturated code) reaches the threshold
        lim4 = M.gap_upper_limit(m8[:, :, None], d[:, :, None], (m8 - d)[:, :, None], (m8 + d).max(axis=1)[:, None], mx, codes, step)[:, :, 0]
        lim4 = np.fmax(np.where(np.isneginf(m8), -np.inf, lim4), np.where(codes[:, :, 0] == 15, bound[:, :, 0].astype(np.float64), -np.inf))
        lowest_open = tau_lo - 2.05 * e * (1 + 1e-5)
        may_count, n_groups = int((lim4 >= lowest_open).sum()), int((up_g >= lowest_open).sum())
        if Q in tied:
            if may_count <= CAPS["RR_X3_MCAP"] or fb[Q] != 1:
                problems.append(f"query {Q}: {may_count} M-tiles may open, flag {fb[Q]}: expected an overflowing list and the flag up")
            continue
        if sigma is not None and np.float64(sigma[128 * s + q]) > open_f:
            if fb[Q] != 1:
                problems.append(f"query {Q}: sigma {sigma[128 * s + q]!r} above the open threshold {open_f!r} and the flag is down")
            continue
        if not (may_count < CAPS["RR_X3_MCAP"] // 2 and n_groups < CAPS["RR_SEL_LCAP"] // 2):
            problems.append(f"query {Q}: precondition: model may-open {may_count} M-tiles, {n_groups} groups")
            continue
        if fb[Q] != 0:
            problems.append(f"query {Q}: fallback flag up (count {count[Q]})")
            continue
        # open = tau~ - 2.05 eps, row cut = tau~ - 1.02 eps (rr_select_mtiles); 1e-5: the fp32 roundings of that arithmetic
        if not (lowest_open <= open_f <= tau_up - 2.05 * e * (1 - 1e-5)):
            problems.append(f"query {Q}: open threshold {open_f!r} outside [{lowest_open!r}, {tau_up - 2.05 * e!r}]")
        if not (tau_lo - 1.02 * e * (1 + 1e-5) <= tau_f <= tau_up - 1.02 * e * (1 - 1e-5)):
            problems.append(f"query {Q}: row cut {tau_f!r} outside [{tau_lo - 1.02 * e!r}, {tau_up - 1.02 * e!r}]")
        ids = mt[Q, :count[Q]].astype(np.int64)
        if len(np.unique(ids)) != len(ids) or (len(ids) and ids.max() >= T * 4):
            problems.append(f"query {Q}: listed M-tiles repeat or run past the matrix")
            continue
        listed = np.zeros(T * 4, dtype=bool)
        listed[ids] = True
        listed = listed.reshape(T, 4)
        missing = ((m8 - d) >= tau_up - 2.0 * e) & ~listed       # tau~_model from above: M-tiles that must be opened
        if missing.any():
            t, g = np.argwhere(missing)[0]
            problems.append(f"query {Q}: must-open M-tile (tile {t}, sub-tile {g}) not listed: M8 - delta = {(m8 - d)[t, g]!r} >= {tau_up - 2 * e!r} ({int(missing.sum())} such)")
        extra = listed & ~(lim4 >= open_f)
        if extra.any():
            t, g = np.argwhere(extra)[0]
            problems.append(f"query {Q}: listed M-tile (tile {t}, sub-tile {g}) cannot reach the open threshold {open_f!r}: bound <= {lim4[t, g]!r}")
    print(f"SELECT|{tag}|queries={nq_a + nq_b}|flags={int(fb.sum())}|max_count={int(count.max())}|problems={len(problems)}", flush=True)
    for p in problems[:10]:
        print("PROBLEM|" + tag + "|" + p, flush=True)
"""


def _child(body: str, timeout: int) -> str:
    from review_recommender_amd.build import DEBUG_LIB_PATH
    if not DEBUG_LIB_PATH.exists():
        pytest.skip("librr_hip_dbg.so not built (python review-recommender_amd/build.py --debug)")
    p = subprocess.run([sys.executable, "-c", (COMMON + body).replace("@ROOT@", repr(ROOT))], capture_output=True, text=True,
                       timeout=timeout)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


def _lines(out: str, tag: str):
    return [l.split("|")[1:] for l in out.splitlines() if l.startswith(tag + "|")]


def _assert_clean(out: str, n_launches: int):
    launches = _lines(out, "LAUNCH")          # one line per set and per launch: exactly what the child's loops make
    assert len(launches) == n_launches, (len(launches), out[-2000:])
    bad = [l for l in launches if l[9] != "violations=0"]
    assert not bad, "\n".join("|".join(l) for l in bad) + "\n" + "\n".join("|".join(l) for l in _lines(out, "VIOLATIONS"))
    assert all(int(l[6].split("=")[1]) > 0 for l in launches)
    for c in _lines(out, "COMPARE"):
        assert c[1] == "0" and c[2] == "0" and int(c[3]) > 0, "asm loop vs C++ bodies: " + "|".join(c)
    for s in _lines(out, "SELECT"):
        assert s[4] == "problems=0", "|".join(s) + "\n" + "\n".join("|".join(l) for l in _lines(out, "PROBLEM"))


SINGLE = r"""
n = @N@
bf16 = @BF16@
mat = unit_rows(n, 31, *(@NORMS@))
mat[1000:1040] = mat[999]                        # a block of equal rows over a tile edge (row 1024)
mat[n - 10:] = mat[n - 11]                       # ... and over the ragged end
ix, a_b = make_index(mat, bf16)
warm(ix)
total = 0
for nq in (5, 32, 33, 64, 65, 128):
    q = queries(nq, 100 + nq, a_b, rows=[(1, n - 1), (2, 1003), (nq - 1, 77)])
    ref = None
    got = {}
    for scan in ([1] if bf16 else [0, 1]):
        G, eps, sigma, words, keys, ref, bad = check_launch("single", ix, a_b, q, nq, 0, scan, ref=ref)
        got[scan] = (words, keys)
        total += bad
    if not bf16:
        dw = int((got[0][0][0][:, :nq] != got[1][0][0][:, :nq]).sum())
        dk = int((got[0][1][0][:, :nq] != got[1][1][0][:, :nq]).sum()) if got[0][1].shape == got[1][1].shape else -1
        print(f"PAIR|rr_scan_flt vs rr_scan_flt16|nq={nq}|words differ={dw}|keys differ={dk}", flush=True)
for nq_b in (65, 128):
    q = queries(128 + nq_b, 300 + nq_b, a_b, rows=[(1, n - 1), (130, 1003), (128 + nq_b - 1, n - 1)])
    ref, got = None, {}
    for scan in (3, 4):
        G, eps, sigma, words, keys, ref, bad = check_launch("paired", ix, a_b, q, 128, nq_b, scan, ref=ref)
        got[scan] = words
        total += bad
    print(f"PAIR|rr_scan_fltq<false> vs <true>|nq=128+{nq_b}|words differ={int((got[3] != got[4]).sum())}", flush=True)
print("DONE", total)
"""


@pytest.mark.parametrize("bf16,norms", [(False, "()"), (True, "()"), (True, "(0.01, 30.0)"), (False, "(0.01, 30.0)")],
                         ids=["f32-unit", "bf16-unit", "bf16-norms", "f32-norms"])
def test_every_scan_at_the_smallest_filter_size(bf16, norms):
    """8 * 150 * 64 + 37 rows (the smallest matrix the filter path serves at pool 150): every selectable scan, query counts
    5, 32, 33, 64, 65, 128 alone and 193, 256 paired; a query that is the matrix's last row, equal rows over a tile edge and
    over the ragged end."""
    out = _child(SINGLE.replace("@N@", str(8 * 150 * 64 + 37)).replace("@BF16@", str(bf16)).replace("@NORMS@", norms), 900)
    _assert_clean(out, 14 if bf16 else 20)
    assert "DONE 0" in out
    pairs = _lines(out, "PAIR")
    # pinned from the first hardware run: on the same plane and queries rr_scan_flt and rr_scan_flt16 leave bit-identical
    # words and keys, and so do the generated loop and the C++ bodies of rr_scan_fltq
    for l in pairs:
        if l[0] in ("rr_scan_flt vs rr_scan_flt16", "rr_scan_fltq<false> vs <true>"):
            assert l[2] == "words differ=0" and (len(l) < 4 or l[3] == "keys differ=0"), "|".join(l)
    assert len(pairs) == (2 if bf16 else 8)
    assert not any("differ=-1" in f for l in pairs for f in l)


RAGGED = r"""
total = 0
for extra, norms in ((1, ()), (31, ()), (32, ()), (33, ()), (33, (0.01, 30.0))):
    n = 64 * 4700 + extra                        # about 300 000 rows
    mat = unit_rows(n, 40 + extra, *norms)
    tag = f"ragged+{extra}" + ("-norms" if norms else "")
    for bf16 in (False, True):
        ix, a_b = make_index(mat, bf16)
        warm(ix)
        for nq in ((5, 32, 33, 64, 65, 128) if norms else (33,)):
            q = queries(nq, 7 + nq, a_b, rows=[(0, n - 1), (nq - 1, n - 1)])
            ref = None
            for scan in ([1] if bf16 else [0, 1]):
                *_, ref, bad = check_launch(tag, ix, a_b, q, nq, 0, scan, ref=ref)
                total += bad
        for nq_b in ((65, 128) if norms else (128,)):
            q = queries(128 + nq_b, 8 + nq_b, a_b, rows=[(0, n - 1), (127 + nq_b, n - 1)])
            ref = None
            for scan in ((3, 4) if norms else (4,)):
                *_, ref, bad = check_launch(tag, ix, a_b, q, 128, nq_b, scan, ref=ref)
                total += bad
        ix.close()
print("DONE", total)
"""


def test_ragged_ends_at_300k_rows():
    """A multiple of 64 plus 1, 31, 32 and 33 rows, fp32 and bf16 storage; queries that are the last row (what a counted pad
    row would repeat).  At plus 33 also rows of norm 0.01 .. 30 with every query count and every selectable scan."""
    out = _child(RAGGED, 1500)
    _assert_clean(out, 62)
    assert "DONE 0" in out


FLTQ = r"""
probe = unit_rows(64 * 20000, 1)
ix, a_b = make_index(probe, False)
warm(ix)
R = geometry(ix, 128, 128, 4)["n_waves"]         # runs of a matrix with more tiles than compute units
ix.close(); del probe
def loop_iterations(G):
    # iterations of the four-body loop per entry, for a full run (rr_scan_fltq's host-visible rule)
    T, cg2, it, out = 2 * G["tiles_per_wave"], 2 * G["tiles_per_group"], 0, []
    while it < T:
        n_it = 0
        if it >= 5 and (it & 3) == 1 and (cg2 & 3) == 0:
            flush = (it + cg2 - 1) // cg2 * cg2
            n_it = (min(flush + 1, T) - it) // 4
        if n_it > 0:
            out.append(n_it); it += 4 * n_it
        else:
            it += 1
    return out
total, seen = 0, set()
for k, want in ((2, "short"), (4, "zero"), (5, "once"), (69, "twice"), (0, "few")):
    n = R * k * 64 - 27 if k else 64 * (R // 3) + 5
    mat = unit_rows(n, 60 + k)
    ix, a_b = make_index(mat, False)
    warm(ix)
    q = queries(256, 9, a_b, rows=[(3, n - 1), (200, n - 1), (77, 12345 % n)])
    ref = None
    for scan in (3, 4):
        G, eps, sigma, words, keys, ref, bad = check_launch(f"fltq-{want}", ix, a_b, q, 128, 128, scan, ref=ref)
        total += bad
    its = loop_iterations(G)
    print(f"SHAPE|{want}|n_rows={n}|runs={G['n_waves']}|M-tiles per run={2 * G['tiles_per_wave']}|loop iterations={its}", flush=True)
    ok = {"short": 2 * G["tiles_per_wave"] < 6 and not its, "zero": 2 * G["tiles_per_wave"] >= 6 and not its, "once": its and max(its) == 1 and 1 in its,
          "twice": 2 in its, "few": G["n_waves"] < R}[want]
    assert ok, (want, G, its)
    # the generated loop against the C++ bodies on the planes of a 256-query search (rr_debug_fltq_compare's contract)
    ix.dense_topk(q.cpu().numpy(), 10)
    fltq_compare(f"fltq-{want}")
    ix.close()
print("DONE", total)
"""


def test_fltq_run_shapes_and_the_generated_loop_against_the_cpp_bodies():
    """rr_scan_fltq<false> and <true> at run lengths chosen from the reported geometry: fewer than six M-tiles per run, the
    four-body loop entered with zero, one and two iterations, a short last M-tile, fewer runs than compute units; at each
    shape rr_debug_fltq_compare must find no differing word and no differing group maximum."""
    out = _child(FLTQ, 1200)
    _assert_clean(out, 20)
    assert len(_lines(out, "COMPARE")) == 5 and len(_lines(out, "SHAPE")) == 5
    assert "DONE 0" in out


PREFILTER = r"""
n, pool = 2_200_000, 150
mat = unit_rows(n, 77)
q_all = queries(128, 4711, mat, norm=1.0)
# the adversarial layout of test_store_prefilter_of_the_filter_scan_stays_exact: query 3's best rows sit in the sampled tiles
gi = torch.Generator(device="cuda"); gi.manual_seed(5)
for i in range(400):
    row = (64 * (i + 3) + 32) * 32 + (i % 32)
    v = q_all[3] * (0.9 - 0.0005 * i) + 0.3 * torch.randn(384, generator=gi, device=dev) / 384 ** 0.5
    mat[row] = v / v.norm()
total = 0
for bf16 in (False, True):
    ix, a_b = make_index(mat, bf16)
    warm(ix)
    for nq in (20, 40, 100):                     # rr_scan_flt16<1>, <2>, <4>
        q, ref = q_all[:nq].contiguous(), None
        for pre in (0, 1):
            tag = f"prefilter={pre} nq={nq}"
            G, eps, sigma, words, keys, ref, bad = check_launch(tag, ix, a_b, q, nq, 0, 1, prefilter=pre, ref=ref, pool=pool)
            total += bad
            assert G["prefilter"] == pre and G["nq2"] == {20: 1, 40: 2, 100: 4}[nq], G
            skipped = int((words[0][:, :nq] == G["word_sentinel"]).sum())
            assert (skipped > 0) == bool(pre), skipped
            print(f"SKIPPED|{tag}|{skipped} of {words[0][:, :nq].size} words left unwritten", flush=True)
            sel = select(ix, nq, pool)
            mt, count, tau, opn, fb = sel
            if pre:
                # query 3: its sampled threshold overshoots -- either sigma <= open after all, or the flag is up; and so for all
                open3 = float(M.key2f(opn[3:4])[0])
                print(f"ADVERSARIAL|nq={nq}|sigma={float(sigma[3])!r}|open={open3!r}|fb={int(fb[3])}", flush=True)
                for Q in range(nq):
                    assert fb[Q] == 1 or float(sigma[Q]) <= float(M.key2f(opn[Q:Q + 1])[0]), ("a silently skipped candidate tile", Q)
            check_selection(tag, G, eps, sigma if pre else None, words, ref, nq, 0, pool, sel)
    ix.close()
print("DONE", total)
"""


def test_store_prefilter_skips_only_what_no_query_can_want():
    """2.2M rows (the prefilter's threshold is 2M): rr_scan_flt16<1>, <2> and <4> (20, 40, 100 queries) with and without sigma
    on an fp32 and a bf16 index.  Every word still at the sentinel belongs to a (tile, 32-query group) all of whose queries have M32 <= sigma + delta; every
    written word passes P1..P6; for the adversarial query sigma <= open or its flag is up."""
    out = _child(PREFILTER, 1500)
    _assert_clean(out, 12)
    assert len(_lines(out, "ADVERSARIAL")) == 6 and len(_lines(out, "SELECT")) == 12 and "DONE 0" in out


BIG = r"""
n = 2_200_000 + 33
mat = unit_rows(n, 78)
mat[n - 40:] = mat[n - 41]                       # equal rows over the last tile edge and the ragged end
total = 0
for bf16 in (False, True):
    ix, a_b = make_index(mat, bf16)
    warm(ix)
    if not bf16:
        q = queries(65, 21, a_b, rows=[(0, n - 1)])
        *_, bad = check_launch("2.2M", ix, a_b, q, 65, 0, 0)
        total += bad
    nq_b = 65 if bf16 else 128
    q = queries(128 + nq_b, 22, a_b, rows=[(1, n - 1), (127 + nq_b, n - 1)])
    ref = None
    for scan in (3, 4):
        *_, ref, bad = check_launch("2.2M", ix, a_b, q, 128, nq_b, scan, ref=ref)
        total += bad
    ix.close()
print("DONE", total)
"""


def test_the_other_scans_at_two_million_rows():
    """2.2M + 33 rows: rr_scan_flt on the fp32 rows and rr_scan_fltq<false|true> with 256 queries
    (fp32 storage) and 193 (bf16 storage); rr_scan_flt16 alone at this size is the prefilter test's."""
    out = _child(BIG, 1500)
    _assert_clean(out, 9)
    assert "DONE 0" in out


SELECTION = r"""
n, pool = 300_037, 150
mat = unit_rows(n, 88)
total = 0
for bf16 in (False, True):
    ix, a_b = make_index(mat, bf16)
    warm(ix)
    for nq_a, nq_b, scan in ((64, 0, 1), (128, 128, 4), (128, 65, 4)):
        q = queries(nq_a + nq_b, 50 + nq_b, a_b, rows=[(1, n - 1)])
        G, eps, sigma, words, keys, ref, bad = check_launch("selection", ix, a_b, q, nq_a, nq_b, scan, pool=pool)
        total += bad
        check_selection(f"selection {KERNEL[scan]}", G, eps, None, words, ref, nq_a, nq_b, pool, select(ix, nq_a + nq_b, pool))
    ix.close()
# massive ties (test_filter_path_falls_back_per_query_on_massive_ties): 20 000 copies of row 3, query 0 is that row
mat = unit_rows(200_000, 91)
mat[::10] = mat[3]
ix, a_b = make_index(mat, False)
warm(ix)
q = queries(20, 92, a_b, norm=1.0, rows=[(0, 3)])
G, eps, sigma, words, keys, ref, bad = check_launch("ties", ix, a_b, q, 20, 0, 1, pool=pool)
total += bad
sel = select(ix, 20, pool)
print("TIES|" + "".join(str(int(f)) for f in sel[4]), flush=True)
check_selection("ties", G, eps, None, words, ref, 20, 0, pool, sel, tied={0})
print("DONE", total)
"""


def test_selection_on_the_words_lists_what_it_must_and_no_more():
    """rr_select_mtiles on the words of ordinary data (300 037 unit rows, both storages, one-set and two-set launches): for
    EVERY query the listed M-tiles contain every M-tile with M8 - delta >= tau~_model - 2 eps, contain none whose P4 upper
    bound stays below the reported open threshold, tau and open sit where rr_select_mtiles' comments put them relative to
    the model's pool-th largest group maximum, and the fallback flag is down -- under the asserted precondition that the
    model's may-open count stays below RR_X3_MCAP / 2 and its group count below RR_SEL_LCAP / 2.  With 20 000 copies of
    one row, the flag of the query that is that row is up and its neighbours' are down."""
    out = _child(SELECTION, 1500)
    _assert_clean(out, 11)
    assert len(_lines(out, "SELECT")) == 7
    ties = _lines(out, "TIES")[0][0]
    assert ties[0] == "1" and set(ties[1:]) == {"0"}, ties
    assert "DONE 0" in out
