"""The kernels of the runtime-width filter path on a bf16 INDEX, one launch at a time on the harness library (librr_hip_dbg.so:
rr_debug_fltw_words, rr_debug_flt_select, rr_debug_fltw_rescore), in child processes with their own timeouts.  Modelled on
tests/test_gpu_fltw_kernels.py; the index adopts a torch bf16 matrix, so the scan streams the index's own rows (no plane).

rr_scan_fltw on ix->d_matrix: EVERY tile word and group key of a launch is held against the properties of
flt_words_model.check_words (P1 / P2 of DESIGN.md among them) with M8 and delta from torch float64 on the device and
row_delta = 0: the launch's eps must be the two-term bound fltw_model.eps_wide gives on the rounded rows.  dim 64 (half-full
last round of the chain; one K-step pair per row in the scan), 320, 1024; 3 000 rows (pool 5) and 12 005 (a ragged last M-tile,
pool 20); 9 and 64 queries (both template instances); unit rows and rows of norm 0.01 .. 30; two queries equal to rows.  Then
the product's selection on that state: no flag up, every must-open M-tile listed.

rr_rescore_chain_wb: every stored score of caller lists -- the matrix's last, partial M-tile (rows past the end), repeats of
it, an empty list, a flagged query, and a row holding a NaN -- is bitwise fltw_bf16_model.chain_wb, at dim 64, 192, 320 (half-
full last rounds), 768 and 1024.

Worst margins on hardware (a record, not a bar), over all launches: words checked, tight side (bound - M8) / step, safe side
(M8 - bound) / delta (P2 allows 1):
    rr_scan_fltw on bf16 rows     0.2M words   7.048   0.000

On the parent commit both tests fail: the bf16 index cannot be created at these widths.
"""
import pathlib
import subprocess
import sys

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
import fltw_model as W
import fltw_bf16_model as WB
from review_recommender_amd import _lib
from review_recommender_amd.index import ProductIndex
lib = _lib.load()
dev = torch.device("cuda", 0)
GN = ["n_rows", "n_tiles", "tiles_per_wave", "n_waves", "gpw", "tiles_per_group", "stride", "words_per_set", "keys_per_set", "sets",
      "prefilter", "nq2", "word_sentinel", "key_sentinel", "word_set_stride", "key_set_stride"]
P = lambda a: a.ctypes.data_as(C.c_void_p)

def rows_of(n, dim, seed, lo=None, hi=None):
    # bf16 rows (rounded once, nearest even)
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    m = torch.randn((n, dim), generator=g, device=dev)
    m /= m.norm(dim=1, keepdim=True)
    if lo is not None:                           # norms log-uniform in [lo, hi]
        m *= torch.exp(torch.rand((n, 1), generator=g, device=dev) * np.log(hi / lo) + np.log(lo))
    return m.to(torch.bfloat16).contiguous()

def queries(nq, dim, seed, mat, norm=7.5, rows=()):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    q = torch.randn((nq, dim), generator=g, device=dev)
    q *= norm / q.norm(dim=1, keepdim=True)
    for i, r in rows:                            # a query that is a row
        v = mat[r].float()
        q[i] = v * (norm / v.norm())
    return q.contiguous()

def reference(a_bf16, q, T, dim):
    # M8[tile, 4, query] and delta[tile, 4, query] in float64 on the device; rows past the end: -inf / 0
    qb = q.to(torch.bfloat16).double()
    n, nq = len(a_bf16), len(q)
    a = a_bf16.double()
    sc = torch.full((32 * T, nq), -float("inf"), dtype=torch.float64, device=dev)
    mg = torch.zeros((32 * T, nq), dtype=torch.float64, device=dev)
    sc[:n] = a @ qb.T
    mg[:n] = a.abs() @ qb.abs().T
    M8 = sc.view(T, 4, 8, nq).amax(dim=2).cpu().numpy()
    D = (W.gamma(dim) * mg.view(T, 4, 8, nq).amax(dim=2)).cpu().numpy()
    return M8, D, (a @ qb.T).cpu().numpy()
"""

WORDS = r"""
total, worst_tight, worst_safe, n_words = 0, 0.0, 0.0, 0
for dim in (64, 320, 1024):
    for n, pool in ((3000, 5), (12005, 20)):
        for norms in ((), (0.01, 30.0)):
            mat = rows_of(n, dim, 31 + dim + n, *norms)
            mat[1000:1040] = mat[999]                        # a block of equal rows over a tile edge (row 1024)
            mat[n - 10:] = mat[n - 11]                       # ... and over the (ragged) end
            host = mat.float().cpu().numpy()
            row_norm = float(mat.double().norm(dim=1).max())
            ix = ProductIndex(None, n_rows=n, dim=dim, device_ptr=mat.data_ptr(), keepalive=mat, dtype="bf16")
            ix.dense_topk(np.random.default_rng(0).standard_normal((9, dim)).astype(np.float32), pool)      # (allocates the scratch)
            assert ix.last_scan_info()[:2] == (5, 16) and ix.last_scan_info()[4] == 2
            for nq in (9, 64):
                q = queries(nq, dim, 100 + nq, mat, rows=[(1, n - 1), (nq - 1, 1003)])
                g = (C.c_int64 * 16)()
                _lib.check(lib.rr_debug_fltw_words(ix.handle, None, nq, pool, g, None, None, 0, None, 0), "rr_debug_fltw_words")
                G = dict(zip(GN, list(g)))
                words = np.empty(G["words_per_set"], dtype=np.uint32)
                keys = np.empty(G["keys_per_set"], dtype=np.uint32)
                eps = np.empty(256, dtype=np.float32)
                _lib.check(lib.rr_debug_fltw_words(ix.handle, C.c_void_p(q.data_ptr()), nq, pool, g, P(eps), P(words), words.size, P(keys),
                                                   keys.size), "rr_debug_fltw_words")
                G = dict(zip(GN, list(g)))
                assert G["stride"] == (32 if nq <= 32 else 64) and G["nq2"] == G["stride"] // 32, G
                T = 2 * G["n_tiles"]
                words, keys = words.reshape(T, G["stride"]), keys.reshape(-1, G["stride"])
                M8, D, s_all = reference(mat, q, T, dim)
                # row_delta = 0: eps is the two-term bound of fltw_model on the rounded rows (the cached row norm carries 1.0001)
                qh = q.cpu().numpy()
                want = W.eps_wide(host, qh)
                rn = np.linalg.norm(host.astype(np.float64), axis=1).max()
                two = 1.01 * (rn * np.linalg.norm(qh.astype(np.float64) - W.bf16(qh).astype(np.float64), axis=1) +
                              W.acc_coef(dim) * rn * np.linalg.norm(qh.astype(np.float64), axis=1))
                assert np.array_equal(want, two), "the delta term of the model is not 0 on bf16 rows"
                assert np.all(eps[:nq] >= want * (1 - 1e-5)) and np.all(eps[:nq] <= want * 1.0002 * (1 + 1e-5)), (eps[:nq], want)
                budget = W.acc_coef(dim) * row_norm * q.double().norm(dim=1).cpu().numpy()
                assert np.all(D.max(axis=(0, 1)) < budget), "delta exceeds the kernel's own accumulation budget"
                e = eps[:nq]
                bad, st = M.check_words(words[:, :nq], keys[:, :nq], G, M8, D, e, sentinel=G["word_sentinel"], may_skip=None)
                nbad = sum(st["counts"].values())
                total += nbad
                worst_tight, worst_safe, n_words = max(worst_tight, st["tight_steps"]), max(worst_safe, st["safe_delta"]), n_words + st["words"]
                print(f"LAUNCH|dim={dim}|n_rows={n}|norms={bool(norms)}|queries={nq}|words={st['words']}|keys={st['keys']}|violations={nbad}|"
                      f"tight_steps={st['tight_steps']:.3f}|safe_delta={st['safe_delta']:.3f}", flush=True)
                if nbad:
                    print("VIOLATIONS|" + M.describe(bad, st).replace("\n", " ;; "), flush=True)
                assert not (words == G["word_sentinel"]).any()
                # ---- the product's selection on that state
                cap = 16384
                mt = np.empty((nq, cap), dtype=np.uint32)
                count, fb = np.empty(nq, dtype=np.int32), np.empty(nq, dtype=np.int32)
                tau, opn = np.empty(nq, dtype=np.uint32), np.empty(nq, dtype=np.uint32)
                _lib.check(lib.rr_debug_flt_select(ix.handle, pool, P(mt), cap, P(count), P(tau), P(opn), P(fb)), "rr_debug_flt_select")
                problems = []
                for Q in range(nq):
                    if fb[Q] != 0:
                        problems.append(f"query {Q}: flag up (count {count[Q]})")
                        continue
                    kth = np.sort(s_all[:, Q])[-pool]                   # the pool-th largest float64 filter score
                    must = (M8[:, :, Q] >= kth - np.float64(e[Q])).reshape(-1)
                    listed = np.zeros(T * 4, dtype=bool)
                    ids = mt[Q, :count[Q]].astype(np.int64)
                    if len(np.unique(ids)) != len(ids) or (len(ids) and ids.max() >= T * 4):
                        problems.append(f"query {Q}: listed M-tiles repeat or run past the matrix")
                        continue
                    listed[ids] = True
                    if (must & ~listed).any():
                        problems.append(f"query {Q}: {int((must & ~listed).sum())} must-open M-tiles not listed")
                print(f"SELECT|dim={dim}|n_rows={n}|queries={nq}|flags={int(fb.sum())}|max_count={int(count.max())}|problems={len(problems)}", flush=True)
                for p in problems[:5]:
                    print("PROBLEM|" + p, flush=True)
                total += len(problems)
            ix.close()
print(f"RECORD|{n_words / 1e6:.1f}M words   {worst_tight:.3f}   {worst_safe:.3f}", flush=True)
print("DONE", total)
"""

RESCORE = r"""
import rescore_model as RM
total = 0
for dim in (64, 192, 320, 768, 1024):
    n = 12005
    mat = rows_of(n, dim, 77 + dim, 0.01, 30.0)
    mat[4321, dim // 2] = float("nan")               # a row holding a NaN: its score is stored as -inf
    ix = ProductIndex(None, n_rows=n, dim=dim, device_ptr=mat.data_ptr(), keepalive=mat, dtype="bf16")
    nq, cap = 5, 64
    q = queries(nq, dim, 9, mat, rows=[(1, n - 1)])
    last = (n - 1) // 8                              # the matrix's last M-tile: rows 12000 .. 12004 and three past the end
    rng = np.random.default_rng(dim)
    mtiles = np.zeros((nq, cap), dtype=np.uint32)
    count = np.array([64, 1, 0, 37, 9], dtype=np.int32)
    fb = np.array([0, 0, 0, 1, 0], dtype=np.int32)   # query 3 is flagged: nothing of it is touched
    mtiles[0] = rng.integers(0, last + 1, cap)
    mtiles[0, :4] = (last, 4321 // 8, last, 0)       # the partial M-tile (twice), the NaN row's, the first
    mtiles[1, 0] = last
    mtiles[3, :37] = rng.integers(0, last + 1, 37)
    mtiles[4, :9] = (4321 // 8, last, 1, 2, 3, 1500, 1499, last - 1, last)     # odd count: the launch repeats the last tile
    sc = np.empty((nq, cap, 8), dtype=np.float32)
    _lib.check(lib.rr_debug_fltw_rescore(ix.handle, C.c_void_p(q.data_ptr()), nq, P(mtiles), cap, P(count), P(fb), P(sc)), "rr_debug_fltw_rescore")
    host, qh = mat.float().cpu().numpy(), q.cpu().numpy()
    want = np.full((nq, cap, 8), RM.SC_SENTINEL, dtype=np.uint32)
    for Q in range(nq):
        if fb[Q]:
            continue
        for s in range(count[Q]):
            r0 = int(mtiles[Q, s]) * 8
            real = min(8, n - r0)
            sc_rows = np.full(8, -np.inf, dtype=np.float32)
            sc_rows[:real] = WB.stored_scores(host[r0:r0 + real], qh[Q])
            want[Q, s] = sc_rows.view(np.uint32)
    diff = int((sc.view(np.uint32) != want).sum())
    nan_ok = bool(np.isneginf(sc[0, 1, 4321 % 8]))
    print(f"RESCORE|dim={dim}|scores={int(count[fb == 0].sum()) * 8}|differ={diff}|nan_row_is_neg_inf={nan_ok}", flush=True)
    total += diff + (0 if nan_ok else 1)
    ix.close()
print("DONE", total)
"""


def _child(body: str, timeout: int) -> str:
    from review_recommender_amd.build import DEBUG_LIB_PATH
    assert DEBUG_LIB_PATH.exists(), "librr_hip_dbg.so is built by build()"
    p = subprocess.run([sys.executable, "-c", (COMMON + body).replace("@ROOT@", repr(ROOT))], capture_output=True, text=True,
                       timeout=timeout)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


def _lines(out: str, tag: str):
    return [l.split("|")[1:] for l in out.splitlines() if l.startswith(tag + "|")]


def test_every_word_and_key_of_the_wide_scan_on_bf16_rows_and_the_selection_on_them():
    out = _child(WORDS, 600)
    launches, selects = _lines(out, "LAUNCH"), _lines(out, "SELECT")
    assert len(launches) == 24 and len(selects) == 24, (len(launches), len(selects), out[-2000:])
    bad = [l for l in launches if l[6] != "violations=0"]
    assert not bad, "\n".join("|".join(l) for l in bad) + "\n" + "\n".join("|".join(l) for l in _lines(out, "VIOLATIONS"))
    assert all(int(l[4].split("=")[1]) > 0 for l in launches)
    for s in selects:
        assert s[3] == "flags=0" and s[5] == "problems=0", "|".join(s) + "\n" + "\n".join("|".join(l) for l in _lines(out, "PROBLEM"))
    assert "DONE 0" in out


def test_rescored_bf16_rows_are_the_chain_bit_for_bit():
    out = _child(RESCORE, 300)
    res = _lines(out, "RESCORE")
    assert len(res) == 5, out[-2000:]
    for r in res:
        assert r[2] == "differ=0" and r[3] == "nan_row_is_neg_inf=True" and int(r[1].split("=")[1]) > 0, "|".join(r)
    assert "DONE 0" in out
