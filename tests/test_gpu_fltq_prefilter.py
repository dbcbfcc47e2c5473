"""The two-set filter scan with the store prefilter from its own first groups (csrc/rr_dense_flt.hip:
rr_flt_launch_fltq_prefiltered = rr_scan_fltq over group 0 of every run, rr_fltq_sigma, rr_scan_fltq over the other groups
with thresholds and masks; csrc/rr_dense.hip: rr_select_mtiles reading only the marked words), against float64 and
against the unfiltered scan.  fltq_prefilter_model.py restates the rule in numpy; test_fltq_prefilter_model.py shows
without a GPU that the shapes below reach the branches they are named for.

Children run on the harness library (rr_debug_fltq_prefiltered, rr_debug_flt_select, rr_debug_select_mlcap), one per
case, and print one line per launch.  Row counts follow the geometry the device reports (R runs), as the rr_scan_fltq
tests of test_gpu_flt_words.py take theirs.
"""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from test_gpu_flt_words import COMMON, ROOT, _lines      # noqa: E402  (the children's shared preamble: index, reference, selection)

pytestmark = pytest.mark.gpu

PAIR_COMMON = COMMON + r"""
import fltq_prefilter_model as F
POOL = 150
OPEN_ALL = 0x00007F80                            # a word that opens every M-tile: maximum +inf, gap codes 0

def runs_of_the_device():
    probe = unit_rows(64 * 20000, 1)
    ix, _ = make_index(probe, False)
    warm(ix)
    R = geometry(ix, 128, 128, 4)["n_waves"]
    ix.close()
    return R

def pair(ix, q, nq_b, flags, fill=0, pool=POOL):
    G0 = geometry(ix, 128, nq_b, 4)
    ng = G0["n_waves"] * G0["gpw"]
    words, keys = np.empty(2 * G0["words_per_set"], dtype=np.uint32), np.empty(2 * G0["keys_per_set"], dtype=np.uint32)
    masks = np.empty(2 * ng * 4, dtype=np.uint64)
    eps, sigma, g = np.empty(256, dtype=np.float32), np.empty(256, dtype=np.float32), (C.c_int64 * 16)()
    _lib.check(lib.rr_debug_fltq_prefiltered(ix.handle, C.c_void_p(q.data_ptr()), 128, nq_b, pool, flags, fill, g, P(eps), P(sigma),
                                             P(words), words.size, P(keys), keys.size, P(masks), masks.size), "rr_debug_fltq_prefiltered")
    G = dict(zip(GN, list(g)))
    return G, eps, sigma, words.reshape(2, 2 * G["n_tiles"], 128), keys.reshape(2, -1, 128), masks.reshape(2, ng, 4)

def marked_of(G, masks, s):
    # lines the selection may read: the masks where the pair wrote them, everything otherwise
    if G["prefilter"] == 3:
        return F.marked_lines(G, masks[s])
    return np.ones((2 * G["n_tiles"], 4), dtype=bool)

def lists(sel, nq):
    mt, count, tau, opn, fb = sel
    return [set(mt[Q, :count[Q]].tolist()) for Q in range(nq)]
"""

WORDS = r"""
bf16, nq_b = @BF16@, @NQB@
R = runs_of_the_device()
total = 0
for name, n in F.shapes(R).items():
    mat = unit_rows(n, 300 + len(name))
    ix, a_b = make_index(mat, bf16)
    warm(ix)
    nq = 128 + nq_b
    q = queries(nq, 17 + nq_b, a_b, rows=[(3, n - 1), (nq - 1, 12345 % n)])
    Gu, epsu, _, wu, ku = scan_words(ix, q, 128, nq_b, 4)                  # the unfiltered scan of the same data
    G, eps, sigma, words, keys, masks = pair(ix, q, nq_b, 1)
    Gc, epsc, sigc, wc, kc, mc = pair(ix, q, nq_b, 1 | 4)                 # the C++ bodies everywhere
    assert G["prefilter"] == (3 if F.pair_taken(G, forced=True) else 0), (name, G)
    assert F.pair_taken(G, forced=True) == (name in ("groups-of-4", "short-last-M-tile", "one-group-run")), (name, G)
    if name == "groups-of-4":
        assert 2 * G["tiles_per_group"] == 4 and F.loop_iterations(G, 0, 1) == [] and 1 in F.loop_iterations(G, 1, G["gpw"]), G
    if name == "one-group-run":
        last = G["n_tiles"] - (G["n_waves"] - 1) * G["tiles_per_wave"]
        assert 0 < last <= G["tiles_per_group"], G
    same = (np.array_equal(words, wc) and np.array_equal(keys, kc) and np.array_equal(masks, mc)
            and np.array_equal(sigma.view(np.uint32), sigc.view(np.uint32)))
    keys_equal = np.array_equal(keys, ku)
    M8, D = reference(a_b, q, 2 * G["n_tiles"])
    problems, nbad, sig_equal, skipped = [], 0, True, 0
    for s, (q0, ns) in enumerate([(0, 128), (128, nq_b)]):
        sg = sigma[128 * s:128 * s + 128]
        if G["prefilter"]:
            want = F.sigma_model(G, keys[s], eps[128 * s:128 * s + 128], ns, POOL)
            sig_equal = sig_equal and np.array_equal(want.view(np.uint32), sg.view(np.uint32))
        marked = marked_of(G, masks, s)
        m8, d = M8[:, :, q0:q0 + ns], D[:, :, q0:q0 + ns]
        problems += [f"set {s}: " + p for p in F.check_lines(G, words[s], marked, m8, d, sg, ns, G["word_sentinel"])]
        bad, st = M.check_words(words[s][:, :ns], keys[s][:, :ns], G, m8, d, eps[128 * s:128 * s + ns], sentinel=G["word_sentinel"],
                                may_skip=~np.repeat(marked, 32, axis=1)[:, :ns])
        nbad += sum(st["counts"].values())
        skipped += st["sentinel_words"]
        if bad:
            print("VIOLATIONS|" + name + "|" + M.describe(bad, st).replace("\n", " ;; "), flush=True)
    for p in problems[:6]:
        print("PROBLEM|" + name + "|" + p, flush=True)
    total += nbad + len(problems)
    stored = float(np.mean([marked_of(G, masks, s).mean() for s in (0, 1)]))
    print(f"PAIR|{name}|n_rows={n}|pair={G['prefilter']}|gpw={G['gpw']}|cg2={2 * G['tiles_per_group']}|asm==c++={same}|keys==unfiltered={keys_equal}|"
          f"sigma==model={sig_equal}|violations={nbad}|problems={len(problems)}|skipped_words={skipped}|lines_marked={stored:.3f}", flush=True)
    ix.close()
print("DONE", total)
"""


def _child(body: str, timeout: int, env=None) -> str:
    from review_recommender_amd.build import DEBUG_LIB_PATH
    if not DEBUG_LIB_PATH.exists():
        pytest.skip("librr_hip_dbg.so not built (python review-recommender_amd/build.py --debug)")
    e = dict(os.environ)
    e.pop("RR_NO_FLTQ_PREFILTER", None)
    e.update(env or {})
    p = subprocess.run([sys.executable, "-c", (PAIR_COMMON + body).replace("@ROOT@", repr(ROOT))], capture_output=True, text=True,
                       timeout=timeout, env=e)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


@pytest.mark.parametrize("nq_b", [1, 65, 128])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32-plane", "bf16"])
def test_words_masks_keys_and_sigma_of_the_prefiltered_pair(bf16, nq_b):
    """The pair forced below 2M rows at ~300 000 rows (4-M-tile groups, every entry and exit of the four-body loop in launch
    B), the same minus 27 rows, a last run of one group, one group per run and fewer tiles than runs (the last two take the
    single launch, as in the product).  Marked lines pass P1..P6 word by word; unmarked lines still hold the sentinel and
    no real query of them has M32 - delta above its sigma; group 0 is fully written; every group key equals the
    unfiltered scan's; sigma equals the numpy rule bit for bit; generated loop and C++ bodies agree on every word, mask,
    key and sigma."""
    out = _child(WORDS.replace("@BF16@", str(bf16)).replace("@NQB@", str(nq_b)), 600)
    pairs = _lines(out, "PAIR")
    assert len(pairs) == 5 and "DONE 0" in out, out[-3000:]
    for l in pairs:
        assert l[5] == "asm==c++=True" and l[6] == "keys==unfiltered=True" and l[7] == "sigma==model=True", "|".join(l)
        assert l[8] == "violations=0" and l[9] == "problems=0", "|".join(l)
    taken = {l[0]: l[2] for l in pairs}
    assert taken == {"groups-of-4": "pair=3", "short-last-M-tile": "pair=3", "one-group-run": "pair=3", "one-group-everywhere": "pair=0",
                     "fewer-tiles-than-runs": "pair=0"}
    # the prefilter did skip lines where it ran, and skipped none where it did not
    for l in pairs:
        assert (int(l[10].split("=")[1]) > 0) == (l[2] == "pair=3"), "|".join(l)


SELECTION = r"""
bf16 = @BF16@
R = runs_of_the_device()
nq_b, problems = 65, []
for name in ("groups-of-4", "short-last-M-tile"):
    n = F.shapes(R)[name]
    mat = unit_rows(n, 500 + len(name))
    ix, a_b = make_index(mat, bf16)
    warm(ix)
    nq = 128 + nq_b
    q = queries(nq, 23, a_b, rows=[(3, n - 1), (nq - 1, 12345 % n)])
    scan_words(ix, q, 128, nq_b, 4)
    unf = select(ix, nq, POOL)
    G, eps, sigma, words, keys, masks = pair(ix, q, nq_b, 1, fill=OPEN_ALL)          # stale words that would open everything
    sel = select(ix, nq, POOL)
    mt, count, tau, opn, fb = sel
    M8, D = reference(a_b, q, 2 * G["n_tiles"])
    got, base = lists(sel, nq), lists(unf, nq)
    assert G["prefilter"] == 3
    for Q in range(nq):
        s, qq = (0, Q) if Q < 128 else (1, Q - 128)
        open_f = float(M.key2f(opn[Q:Q + 1])[0])
        if float(sigma[128 * s + qq]) > open_f:
            if fb[Q] != 1:
                problems.append(f"{name} query {Q}: sigma above open and the flag is down")
            continue
        if fb[Q] != 0 or unf[4][Q] != 0:
            problems.append(f"{name} query {Q}: flagged ({fb[Q]}, unfiltered {unf[4][Q]})")
            continue
        if opn[Q] != unf[3][Q] or tau[Q] != unf[2][Q]:
            problems.append(f"{name} query {Q}: thresholds differ from the unfiltered scan's")
        marked = F.marked_lines(G, masks[s])
        ids = np.array(sorted(got[Q]), dtype=np.int64)
        if len(ids) and not marked[ids // 4, qq // 32].all():
            problems.append(f"{name} query {Q}: an M-tile of an unmarked line is listed")
        if not got[Q] <= base[Q]:
            problems.append(f"{name} query {Q}: {len(got[Q] - base[Q])} M-tiles listed that the unfiltered scan's selection does not list")
        must = np.flatnonzero(((M8[:, :, Q] - D[:, :, Q]) >= open_f).reshape(-1))
        if not set(must.tolist()) <= got[Q]:
            problems.append(f"{name} query {Q}: {len(set(must.tolist()) - got[Q])} M-tiles whose M8 - delta reaches open are not listed")
    # masks off (launch B only skips stores; untouched words are the NaN sentinel, which opens nothing) and the LDS list
    # overflowing (the loop over all words of the opened groups): the same sets
    pair(ix, q, nq_b, 1 | 2)
    off = select(ix, nq, POOL)
    lib.rr_debug_select_mlcap(8)
    G2, *_ = pair(ix, q, nq_b, 1)
    over = select(ix, nq, POOL)
    lib.rr_debug_select_mlcap(0)
    assert G2["prefilter"] == 3
    for tag, other in (("masks off", off), ("list overflow", over)):
        if lists(other, nq) != got or not np.array_equal(other[4], fb):
            problems.append(f"{name}: {tag}: lists or flags differ from the masked selection's")
    print(f"SELECT|{name}|queries={nq}|flags={int(fb.sum())}|max_count={int(count.max())}|unfiltered_max={int(unf[1].max())}", flush=True)
    ix.close()
for p in problems[:10]:
    print("PROBLEM|" + p, flush=True)
print("DONE", len(problems))
"""


@pytest.mark.parametrize("bf16", [False, True], ids=["f32-plane", "bf16"])
def test_selection_reads_only_marked_words(bf16):
    """The word scratch pre-filled with words that would open every M-tile (maximum +inf, codes 0): nothing from an unmarked
    line is listed; the M-tiles listed with masks are a subset of those listed from an unfiltered scan of the same data
    and contain every M-tile whose M8 - delta reaches `open`; thresholds equal the unfiltered scan's; with the masks off
    and with the LDS list overflowing the same sets come out."""
    out = _child(SELECTION.replace("@BF16@", str(bf16)), 600)
    assert len(_lines(out, "SELECT")) == 2 and "DONE 0" in out, out[-3000:]


END_TO_END = r"""
n, nq = 2_200_000, 256
mat = unit_rows(n, 77)
ix, _ = make_index(mat, False)
warm(ix)
G = geometry(ix, 128, 128, 4)
ix.close()
q = queries(nq, 4711, mat, norm=1.0)
# adversarial layout: the best rows of query ADV all sit in first groups (group 0 of run r = its first tiles_per_group tiles)
ADV = 5
gi = torch.Generator(device="cuda"); gi.manual_seed(5)
for i in range(400):
    row = (i % G["n_waves"]) * G["tiles_per_wave"] * 64 + 3 + 7 * (i // G["n_waves"])
    v = q[ADV] * (0.9 - 0.0005 * i) + 0.3 * torch.randn(384, generator=gi, device=dev) / 384 ** 0.5
    mat[row] = v / v.norm()
ix, a_b = make_index(mat, False)
qh = q.cpu().numpy()
out = {}
out["rows256"], out["scores256"] = ix.dense_topk(qh, POOL)
assert ix.last_scan_info()[:2] == (5, 9), ix.last_scan_info()
tr = np.zeros((nq, 16), dtype=np.int32)
_lib.check(lib.rr_debug_select_traces(ix.handle, nq, P(tr)), "rr_debug_select_traces")
out["filter_path"] = (tr[:, 0] == 2).astype(np.int32)
out["rows256b"], out["scores256b"] = ix.dense_topk(qh, POOL)
out["rows193"], out["scores193"] = ix.dense_topk(qh[:193], POOL)
for Q in (0, ADV, 130, 200, 255):
    out[f"rows1_{Q}"], out[f"scores1_{Q}"] = ix.dense_topk(qh[Q:Q + 1], POOL)
if not os.environ.get("RR_NO_FLTQ_PREFILTER"):
    # the same pair through the harness (the product's rule: on from 2M rows), and the product's selection on what it left
    Gp, eps, sigma, words, keys, masks = pair(ix, q, 128, 0)
    assert Gp["prefilter"] == 3, Gp
    mt, count, tau, opn, fb = select(ix, nq, POOL)
    open_f = M.key2f(opn)
    sg = np.concatenate([sigma[:128], sigma[128:256]])
    for s in (0, 1):
        want = F.sigma_model(Gp, keys[s], eps[128 * s:128 * s + 128], 128, POOL)
        assert np.array_equal(want.view(np.uint32), sigma[128 * s:128 * s + 128].view(np.uint32)), "sigma is not the numpy rule's"
    print(f"ADVERSARIAL|sigma={float(sg[ADV])!r}|open={float(open_f[ADV])!r}|fb={int(fb[ADV])}|other_flags={int(fb.sum()) - int(fb[ADV])}|"
          f"lines_marked={float(np.mean([F.marked_lines(Gp, masks[s]).mean() for s in (0, 1)])):.3f}", flush=True)
    out["adv"] = np.array([float(sg[ADV]) > float(open_f[ADV]), fb[ADV] == 1, fb.sum() == fb[ADV], np.all(sg[fb == 0] <= open_f[fb == 0])], dtype=np.int32)
np.savez(@OUT@, **out)
ix.close()
print("DONE 0")
"""


def test_end_to_end_bitwise_with_and_without_the_prefilter(tmp_path):
    """2.2M rows, where the product itself turns the prefilter on: 256 and 193 queries, rows and scores bitwise equal with and
    without RR_NO_FLTQ_PREFILTER=1 (a child process per setting), bitwise equal to single-query searches for a handful of
    queries, and the same batch twice gives the same bits.  One query's best rows all sit in first groups: it is flagged
    (sigma above its open threshold), the others stay on the filter path, and its answer is still the single-query scan's."""
    got = {}
    for tag, env in (("on", {}), ("off", {"RR_NO_FLTQ_PREFILTER": "1"})):
        path = str(tmp_path / f"{tag}.npz")
        out = _child(END_TO_END.replace("@OUT@", repr(path)), 600, env=env)
        assert "DONE 0" in out
        got[tag] = dict(np.load(path))
    on, off = got["on"], got["off"]
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    for k in off:
        assert np.array_equal(bits(on[k]), bits(off[k])) or k == "filter_path", k
    assert np.array_equal(on["rows256"], on["rows256b"]) and np.array_equal(bits(on["scores256"]), bits(on["scores256b"]))
    assert np.array_equal(on["rows193"], on["rows256"][:193]) and np.array_equal(bits(on["scores193"]), bits(on["scores256"][:193]))
    for Q in (0, 5, 130, 200, 255):
        assert np.array_equal(on[f"rows1_{Q}"][0], on["rows256"][Q]) and np.array_equal(bits(on[f"scores1_{Q}"][0]), bits(on["scores256"][Q])), Q
    assert on["adv"].tolist() == [1, 1, 1, 1], on["adv"]
    assert on["filter_path"][5] == 0 and on["filter_path"].sum() == 255 and off["filter_path"].sum() == 256
