"""The last two launches of the batch tail -- rr_rescore_chain (csrc/rr_dense_flt.hip) and rr_select_rescored
(csrc/rr_dense.hip) -- one launch at a time against tests/rescore_model.py, on caller lists placed in the selection scratch
(librr_hip_dbg.so: rr_debug_rescore_chain, rr_debug_select_rescored; both launch through the product's helpers,
rr_launch_rescore_chain and rr_launch_select_rescored).  EVERY word of every output is compared, so a wrong score outside
the final top-pool, a row wrongly set to -inf by the plane pre-scoring, a store past a list's end and a write into a flagged
query's outputs all show up at the launch that made them.

Each group of cases runs in a child process with its own timeout and prints one line per launch (CASE), per selection
case (SEL) and per refused call (REFUSE); the parent asserts on the lines.  The inputs come from rescore_model.py, where
tests/test_rescore_model.py checks on the CPU that they reach the branches they are meant to reach.

Rescoring (2043 rows = 255 M-tiles of 8 rows + one of 3): per launch five queries with lists of c M-tiles, c = 0 .. 600 (past
256 with repeats), the ragged M-tile first / in the middle / last / as the repeated padding, one query flagged on entry;
each c with 16 and with 4 workgroups per query.  Every score due an exact chain equals the model's bits AND the single-query
search's score of that row AND lies within gamma_28 sum |a_k q_k| of the float64 dot product; rows past the end and NaN
scores are -inf; slots past a list's end and the flagged query keep the sentinel; both grids leave the same bits.  With the
bf16 plane the per-row decision (exact chain or -inf) must be the model's, for tau = 0, eps = NaN, eps = inf (every row exact),
tau = the key of the 150th largest score with the filter bound as eps (44 % .. 64 % of the rows skipped) and tau = key(+inf)
(every row -inf).  One chained case: all 256 M-tiles in file order, then rr_select_rescored at pool 150 -- rows and score
bits of dense_topk(q, 150) of a batch of one.

Selection (8189 zero rows, row_offset 1000, synthetic scores): one query per case, one launch per (pool, rows per M-tile,
floor_mode); see rescore_model.selection_cases.  Rows, score bits, flag and candidate count equal the model's; flagged
queries keep their output sentinels.

Five indexes in all (each carries the selection scratch): fp32, bf16, fp32 with a NaN and two inf elements, the selection's,
and one of dimension 64 that both entries must refuse.

Worst |score - float64| / (gamma_28 sum |a_k q_k|) on hardware (a record, not a bar: the bar is 1), over all launches of a
form: fp32 rows 0.0210 (220 launches), bf16 rows 0.0201 (36), the index with NaN / inf elements 0.0210 (72).  On the first
run every launch equalled the model and the single-query search bit for bit, and the single-query search equalled the model
on all 5 x 2043 rows of each index.

Kernel-side mutations, each applied to the debug library alone (values and comparisons only), run against one test and
reverted:
    pre-threshold factor 1.01f -> 0.5f                      fp32 test fails at every "plane split" launch: "plane split|c=1|grid=16|
                                                            model=2|...|single=2|bound=2", "query 0 slot 0 (M-tile 255) row 0:
                                                            kernel 0xff800000, model 0x3b847caf" (a row skipped that the model scores)
    bf16 form stores without `row < n_rows`                 bf16 test fails: "bf16|c=1|grid=16|model=15|sentinel=0|past_end=15",
                                                            "(M-tile 255) row 3: kernel 0x3cb09625, model 0xff800000"
    row tie order reversed in rr_select_rescored's key      selection test fails in every kept case with more rows than one:
    (row instead of 0xFFFFFFFF - row, stored and decoded)   "pool=150|rpm=8|floor=0|n_cand=150|...|rows differ first at rank 0: 8586
                                                            (key 0x3f80c000), model 1134 (0x3f80c000)"
    `slot < RCAP / 2` -> `slot <= RCAP / 2`                 left out: the comparison guards the store `cand[slot] = ...` itself, so
                                                            the mutant writes cand[RCAP / 2] -- an address the kernel never writes
                                                            there -- and a mutation may not touch an address.  What the guard
                                                            protects is covered from outside: n_cand = RCAP / 2 keeps its answer and
                                                            n_cand = RCAP / 2 + 1 raises the flag, for both instances.
"""
import pathlib
import subprocess
import sys

import pytest

import rescore_model as M

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)

COMMON = r"""
import os, sys
os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, @ROOT@); sys.path.insert(0, os.path.join(@ROOT@, "tests"))
import ctypes as C
import numpy as np, torch
import rescore_model as M
from review_recommender_amd import _lib
from review_recommender_amd.index import ProductIndex
lib = _lib.load()
dev = torch.device("cuda", 0)
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
NQ, N = M.RESCORE_NQ, M.RESCORE_ROWS
HOST_FILL = np.uint32(0x11111111)              # what the host output arrays hold before a call
KEY_INF = M.f2key(np.float32([np.inf]))[0]

def make_index(V, bf16):
    # -> index, the rows it stores as float32 values, the device tensor the float64 reference reads
    t = torch.from_numpy(V).to(dev)
    if bf16:
        tb = t.to(torch.bfloat16).contiguous()
        ix = ProductIndex(None, n_rows=len(V), dim=384, device_ptr=tb.data_ptr(), keepalive=tb, dtype="bf16")
        stored = tb.float().cpu().numpy()
        assert (stored.view(np.uint32) == M.round_to_bf16(V).view(np.uint32)).all()      # the model's rounding is the index's
        return ix, stored, tb
    return ProductIndex(V), V, t

def reference64(a_dev, Q):
    # float64 dot products and sum |a_k q_k| on the device -> [NQ][N]
    with torch.no_grad():
        a, q = a_dev.double(), torch.from_numpy(Q).to(dev).double()
        return (q @ a.T).cpu().numpy(), (q.abs() @ a.abs().T).cpu().numpy()

def single_query_scores(ix, Q):
    # every row's score from the single-query search (an independent kernel): [NQ][N]; NaN scores come back as -inf
    out = np.empty((len(Q), N), dtype=np.float32)
    for q in range(len(Q)):
        rows, sc = ix.dense_topk(Q[q:q + 1], N)
        assert sorted(rows[0].tolist()) == list(range(N))
        out[q, rows[0]] = sc[0]
    return out

def rescore(ix, dq, mt, count, fb, tau, eps, grid_x, use_plane):
    cap = mt.shape[1]
    sc = np.full((len(count), cap, 8), HOST_FILL, dtype=np.uint32)
    torch.cuda.synchronize()
    _lib.check(lib.rr_debug_rescore_chain(ix.handle, C.c_void_p(dq.data_ptr()), len(count), grid_x, use_plane, P(mt), cap, P(count), P(fb),
                                          P(np.ascontiguousarray(tau, dtype=np.uint32)), P(np.ascontiguousarray(eps, dtype=np.float32)), P(sc)),
               "rr_debug_rescore_chain")
    return sc

def check_launch(tag, got, mt, count, fb, stored, exact_mask, single, ref64, mag64):
    # got [NQ][cap][8] uint32.  stored[q][row]: the model's stored score; exact_mask[q][row]: the row takes the exact chain
    cap = mt.shape[1]
    exp = M.rescore_expected(stored, N, mt, count, fb, cap)
    bad_model = int((got != exp).sum())
    sent = exp == M.SC_SENTINEL
    listed = np.zeros_like(sent)
    for q in range(NQ):
        if not fb[q]:
            listed[q, :count[q]] = True
    assert (sent == ~listed).all()                       # (no model score is the sentinel)
    bad_sentinel = int((got[sent] != M.SC_SENTINEL).sum())
    rows = mt.astype(np.int64)[:, :, None] * 8 + np.arange(8)[None, None, :]
    past = listed & (rows >= N)
    bad_past = int((got[past] != M.NEG_INF_BITS).sum())
    rr = np.minimum(rows, N - 1)
    qq = np.broadcast_to(np.arange(NQ)[:, None, None], rows.shape)
    due = listed & (rows < N) & exact_mask[qq, rr]
    skipped = listed & (rows < N) & ~exact_mask[qq, rr]
    bad_skip = int((got[skipped] != M.NEG_INF_BITS).sum())
    bad_single = int((got[due] != single.view(np.uint32)[qq, rr][due]).sum())
    g = got.view(np.float32)
    fin = due & np.isfinite(ref64[qq, rr]) & (mag64[qq, rr] > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.abs(g.astype(np.float64) - ref64[qq, rr]) / (M.GAMMA_28 * np.where(mag64[qq, rr] > 0, mag64[qq, rr], 1.0))
    bad_bound = int((~(ratio[fin] <= 1.0)).sum())
    worst = float(ratio[fin].max()) if fin.any() else 0.0
    zero = due & (mag64[qq, rr] == 0)
    bad_bound += int((g[zero] != 0).sum())
    nan_rows = listed & (rows < N) & np.isnan(ref64[qq, rr])
    bad_nan = int((got[nan_rows] != M.NEG_INF_BITS).sum())
    print(f"CASE|{tag}|model={bad_model}|sentinel={bad_sentinel}|past_end={bad_past}|skipped={bad_skip}|single={bad_single}|bound={bad_bound}|"
          f"nan={bad_nan}|due={int(due.sum())}|not_due={int(skipped.sum())}|worst={worst:.4f}", flush=True)
    if bad_model:
        q, s, r = np.argwhere(got != exp)[0]
        print(f"FIRST|{tag}|query {q} slot {s} (M-tile {mt[q, s]}) row {r}: kernel {got[q, s, r]:#010x}, model {exp[q, s, r]:#010x}", flush=True)

def run_counts(form, ix, dq, Q, stored, exact_mask, single, ref64, mag64, tau, eps, use_plane, counts=M.RESCORE_COUNTS):
    for c in counts:
        mt, count, fb = M.rescore_lists(c)
        got = {}
        for grid_x in (16, 4):
            got[grid_x] = rescore(ix, dq, mt, count, fb, tau, eps, grid_x, use_plane)
            check_launch(f"{form}|c={c}|grid={grid_x}", got[grid_x], mt, count, fb, stored, exact_mask, single, ref64, mag64)
        print(f"GRIDS|{form}|c={c}|differ={int((got[16] != got[4]).sum())}", flush=True)

def settings(exact, est, V, Q):
    # the plane cases: name -> (tau [NQ], eps [NQ]); query 4 (flagged) borrows query 0's
    cut = [M.split_cut(exact[q], V, Q[q]) for q in range(NQ)]
    tau, eps = np.array([c[0] for c in cut], dtype=np.uint32), np.array([c[1] for c in cut], dtype=np.float32)
    return {"tau=0": (np.zeros(NQ, dtype=np.uint32), eps), "eps=nan": (tau, np.full(NQ, np.nan, dtype=np.float32)),
            "eps=inf": (tau, np.full(NQ, np.inf, dtype=np.float32)), "split": (tau, eps),
            "tau=+inf": (np.full(NQ, KEY_INF, dtype=np.uint32), np.zeros(NQ, dtype=np.float32))}

def model_scores(rows_f32, Q, per):
    f = M.chain_f32 if per == 4 else M.chain_bf16
    return np.stack([f(rows_f32, q) for q in Q])
"""


def _child(body: str, timeout: int) -> str:
    from review_recommender_amd.build import DEBUG_LIB_PATH
    assert DEBUG_LIB_PATH.exists(), "librr_hip_dbg.so not built (python review-recommender_amd/build.py --debug)"
    p = subprocess.run([sys.executable, "-c", (COMMON + body).replace("@ROOT@", repr(ROOT))], capture_output=True, text=True,
                       timeout=timeout)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


def _lines(out: str, tag: str):
    return [l.split("|")[1:] for l in out.splitlines() if l.startswith(tag + "|")]


def _field(line, name):
    return [f.split("=", 1)[1] for f in line if f.startswith(name + "=")][0]


def _assert_rescoring(out: str, n_launches: int):
    cases, grids = _lines(out, "CASE"), _lines(out, "GRIDS")
    assert len(cases) == n_launches and len(grids) * 2 == n_launches, (len(cases), len(grids), out[-2000:])
    first = "\n".join("|".join(l) for l in _lines(out, "FIRST")[:10])
    for l in cases:
        for name in ("model", "sentinel", "past_end", "skipped", "single", "bound", "nan"):
            assert _field(l, name) == "0", "|".join(l) + "\n" + first
    for l in grids:
        assert _field(l, "differ") == "0", "|".join(l)
    assert "DONE" in out
    worst = max(float(_field(l, "worst")) for l in cases)
    print(f"worst |score - float64| / (gamma_28 sum |a q|) over {len(cases)} launches: {worst:.4f}")
    return cases


def _due(cases, form):
    # (rows due an exact chain, rows not due one) over the launches of a form
    sel = [l for l in cases if l[0] == form]
    assert sel, form
    return sum(int(_field(l, "due")) for l in sel), sum(int(_field(l, "not_due")) for l in sel)


F32 = r"""
V, Q = M.rescore_matrix(), M.rescore_queries()
ix, stored_rows, a_dev = make_index(V, False)
dq = torch.from_numpy(Q).to(dev).contiguous()
ref64, mag64 = reference64(a_dev, Q)
single = single_query_scores(ix, Q)
exact, est = model_scores(V, Q, 4), model_scores(M.round_to_bf16(V), Q, 8)
print(f"MODEL|single-query search vs model chain: {int((single.view(np.uint32) != M.row_scores(exact).view(np.uint32)).sum())} rows differ", flush=True)
every = np.ones((NQ, N), dtype=bool)
# no plane: the cut and the bound are not looked at (key(+inf) would reject every row)
run_counts("no-plane", ix, dq, Q, M.row_scores(exact), every, single, ref64, mag64, np.full(NQ, KEY_INF, dtype=np.uint32), np.zeros(NQ, dtype=np.float32), 0)
for name, (tau, eps) in settings(exact, est, V, Q).items():
    mask = np.stack([M.takes_exact_chain(est[q], tau[q], eps[q]) for q in range(NQ)])
    st = np.stack([M.row_scores(exact[q], est[q], tau[q], eps[q]) for q in range(NQ)])
    run_counts("plane " + name, ix, dq, Q, st, mask, single, ref64, mag64, tau, eps, 1)
# the plane is built now: use_plane = 0 must still take the no-plane form
run_counts("no-plane again", ix, dq, Q, M.row_scores(exact), every, single, ref64, mag64, np.zeros(NQ, dtype=np.uint32), np.zeros(NQ, dtype=np.float32), 0, counts=(33, 600))
# chained: all 256 M-tiles in file order -> rr_rescore_chain (plane, splitting cut) -> rr_select_rescored, pool 150
tau, eps = settings(exact, est, V, Q)["split"]
mt = np.ascontiguousarray(np.broadcast_to(np.arange(M.RESCORE_TILES, dtype=np.uint32), (NQ, M.RESCORE_TILES)))
count, fb = np.full(NQ, M.RESCORE_TILES, dtype=np.int32), np.array([0, 0, 0, 0, 1], dtype=np.int32)
sc = rescore(ix, dq, mt, count, fb, tau, eps, 16, 1)
rows, scores = np.full((NQ, M.POOL), -1, dtype=np.int64), np.full((NQ, M.POOL), HOST_FILL, dtype=np.uint32)
fbo, nc = np.full(NQ, -1, dtype=np.int32), np.full(NQ, -1, dtype=np.int32)
_lib.check(lib.rr_debug_select_rescored(ix.handle, NQ, M.POOL, 8, 0, P(mt), M.RESCORE_TILES, P(count), P(fb), P(tau), P(sc), P(rows), P(scores),
                                        P(fbo), P(nc)), "rr_debug_select_rescored")
for q in range(NQ):
    if fb[q]:
        ok = (rows[q] == M.ROW_SENTINEL).all() and (scores[q] == M.SC_SENTINEL).all() and fbo[q] == 1 and nc[q] == M.NCAND_SENTINEL
    else:
        r1, s1 = ix.dense_topk(Q[q:q + 1], M.POOL)
        ok = rows[q].tolist() == r1[0].tolist() and (scores[q] == s1[0].view(np.uint32)).all() and fbo[q] == 0 and nc[q] >= M.POOL
    print(f"CHAINED|query {q}|ok={int(ok)}|n_cand={nc[q]}|fb={fbo[q]}", flush=True)
print("DONE")
"""


def test_rescoring_of_fp32_rows_with_and_without_the_plane():
    """The fp32 index: the no-plane form, the five plane cases, and the chained case.  From the CASE lines: "split" skips some
    listed rows and keeps others, tau = 0 / eps = NaN / eps = inf skip none, tau = key(+inf) keeps none."""
    out = _child(F32, 600)
    n = len(M.RESCORE_COUNTS)
    cases = _assert_rescoring(out, 2 * n * 6 + 4)
    assert _lines(out, "MODEL")[0][0].endswith(": 0 rows differ"), _lines(out, "MODEL")
    for form in ("no-plane", "plane tau=0", "plane eps=nan", "plane eps=inf"):
        due, not_due = _due(cases, form)
        assert due > 0 and not_due == 0, (form, due, not_due)
    due, not_due = _due(cases, "plane split")
    assert 0.1 <= not_due / (due + not_due) <= 0.9, (due, not_due)
    assert _due(cases, "plane tau=+inf")[0] == 0
    chained = _lines(out, "CHAINED")
    assert len(chained) == 5 and all(l[1] == "ok=1" for l in chained), chained


BF16 = r"""
V, Q = M.rescore_matrix(), M.rescore_queries()
ix, stored_rows, a_dev = make_index(V, True)
dq = torch.from_numpy(Q).to(dev).contiguous()
ref64, mag64 = reference64(a_dev, Q)
single = single_query_scores(ix, Q)
exact = model_scores(stored_rows, Q, 8)
print(f"MODEL|single-query search vs model chain: {int((single.view(np.uint32) != M.row_scores(exact).view(np.uint32)).sum())} rows differ", flush=True)
run_counts("bf16", ix, dq, Q, M.row_scores(exact), np.ones((NQ, N), dtype=bool), single, ref64, mag64, np.full(NQ, KEY_INF, dtype=np.uint32),
           np.full(NQ, np.nan, dtype=np.float32), 0)
# a plane is an fp32 index's: refused here, nothing launched
mt, count, fb = M.rescore_lists(5)
sc = np.full((NQ, 5, 8), HOST_FILL, dtype=np.uint32)
z = np.zeros(NQ, dtype=np.uint32)
rc = lib.rr_debug_rescore_chain(ix.handle, C.c_void_p(dq.data_ptr()), NQ, 16, 1, P(mt), 5, P(count), P(fb), P(z), P(z.view(np.float32)), P(sc))
msg = lib.rr_last_error().decode()
print(f"REFUSE|rr_debug_rescore_chain|use_plane on a bf16 index|rc={rc}|named={int('rr_debug_rescore_chain' in msg)}|untouched={int((sc == HOST_FILL).all())}", flush=True)
print("DONE")
"""


def _assert_refusals(out: str, n: int):
    ref = _lines(out, "REFUSE")
    assert len(ref) == n, (len(ref), out[-3000:])
    for l in ref:
        assert l[2] == "rc=-1" and l[3] == "named=1" and l[4] == "untouched=1", "|".join(l)


def test_rescoring_of_bf16_rows():
    """The bf16 index: rr_rescore_chain<true>, whose 24-step chain over the bf16 row IS the score."""
    out = _child(BF16, 600)
    cases = _assert_rescoring(out, 2 * len(M.RESCORE_COUNTS))
    assert _lines(out, "MODEL")[0][0].endswith(": 0 rows differ"), _lines(out, "MODEL")
    due, not_due = _due(cases, "bf16")
    assert due > 0 and not_due == 0
    _assert_refusals(out, 1)


SPECIAL = r"""
V, Q = M.rescore_matrix(special=True), M.rescore_queries()
ix, stored_rows, a_dev = make_index(V, False)
dq = torch.from_numpy(Q).to(dev).contiguous()
ref64, mag64 = reference64(a_dev, Q)
single = single_query_scores(ix, Q)
exact, est = model_scores(V, Q, 4), model_scores(M.round_to_bf16(V), Q, 8)
print(f"MODEL|single-query search vs model chain: {int((single.view(np.uint32) != M.row_scores(exact).view(np.uint32)).sum())} rows differ", flush=True)
print(f"SPECIAL|nan scores={int(np.isnan(exact).sum())}|inf scores={int(np.isinf(exact).sum())}|nan plane scores={int(np.isnan(est).sum())}", flush=True)
every = np.ones((NQ, N), dtype=bool)
run_counts("no-plane", ix, dq, Q, M.row_scores(exact), every, single, ref64, mag64, np.zeros(NQ, dtype=np.uint32), np.zeros(NQ, dtype=np.float32), 0)
tau, eps = np.full(NQ, M.f2key(np.float32([0.5]))[0], dtype=np.uint32), np.full(NQ, 0.25, dtype=np.float32)
mask = np.stack([M.takes_exact_chain(est[q], tau[q], eps[q]) for q in range(NQ)])
st = np.stack([M.row_scores(exact[q], est[q], tau[q], eps[q]) for q in range(NQ)])
print(f"SPECIAL|nan row takes the exact chain={int(mask[:, M.NAN_ROW].all())}|stored={st[0, M.NAN_ROW]}", flush=True)
run_counts("plane", ix, dq, Q, st, mask, single, ref64, mag64, tau, eps, 1)
print("DONE")
"""


def test_rescoring_of_rows_with_nan_and_inf_elements():
    """A row with a NaN element (its plane score is NaN: the exact chain decides, and stores -inf) and rows with +inf / -inf
    elements (scores of +-inf are scores), in an index of their own so that the finite index keeps a finite bound."""
    out = _child(SPECIAL, 600)
    cases = _assert_rescoring(out, 4 * len(M.RESCORE_COUNTS))
    assert _lines(out, "MODEL")[0][0].endswith(": 0 rows differ"), _lines(out, "MODEL")
    sp = _lines(out, "SPECIAL")
    assert sp[0] == ["nan scores=5", "inf scores=10", "nan plane scores=5"], sp
    assert sp[1] == ["nan row takes the exact chain=1", "stored=-inf"], sp
    due, not_due = _due(cases, "plane")
    assert due > 0 and not_due > 0


SELECT = r"""
ix = ProductIndex(np.zeros((M.SELECT_ROWS, 384), dtype=np.float32), row_offset=M.SELECT_OFFSET)

def select(ix, pool, rpm, floor_mode, mt, count, fb, tau, sc, nq=None, cap=None, outs=None):
    nq = len(count) if nq is None else nq
    cap = mt.shape[1] if cap is None else cap
    if outs is None:
        outs = (np.full((max(nq, 1), max(pool, 1)), -1, dtype=np.int64), np.full((max(nq, 1), max(pool, 1)), HOST_FILL, dtype=np.uint32),
                np.full(max(nq, 1), -1, dtype=np.int32), np.full(max(nq, 1), -1, dtype=np.int32))
    rc = lib.rr_debug_select_rescored(ix.handle if ix is not None else None, nq, pool, rpm, floor_mode, P(mt), cap, P(count), P(fb), P(tau),
                                      P(sc), *[P(o) for o in outs])
    return rc, outs

n_launch = 0
for key, cases in M.selection_launches().items():
    pool, rpm, floor_mode = key
    mt, count, fb, tau, sc = M.selection_launch_arrays(key, cases)
    rc, (rows, scores, fbo, nc) = select(ix, pool, rpm, floor_mode, mt, count, fb, tau, sc)
    _lib.check(rc, "rr_debug_select_rescored")
    n_launch += 1
    for i, case in enumerate(cases):
        want = M.select_rescored(mt[i], count[i], fb[i], tau[i], sc[i], pool, rpm, floor_mode, M.SELECT_ROWS, M.SELECT_OFFSET)
        problems = []
        if fbo[i] != want["fb"]:
            problems.append(f"flag {fbo[i]}, model {want['fb']}")
        if nc[i] != (M.NCAND_SENTINEL if want["n_cand"] is None else want["n_cand"]):
            problems.append(f"n_cand {nc[i]}, model {want['n_cand']}")
        if want["rows"] is None:
            if not ((rows[i] == M.ROW_SENTINEL).all() and (scores[i] == M.SC_SENTINEL).all()):
                problems.append("a flagged query's outputs were written")
        else:
            if rows[i].tolist() != want["rows"].tolist():
                j = int(np.argmax(rows[i] != want["rows"]))
                problems.append(f"rows differ first at rank {j}: {rows[i][j]} (key {scores[i][j]:#010x}), model {want['rows'][j]} ({want['scores'].view(np.uint32)[j]:#010x})")
            if (scores[i] != want["scores"].view(np.uint32)).any():
                problems.append(f"{int((scores[i] != want['scores'].view(np.uint32)).sum())} score bit patterns differ")
        print(f"SEL|pool={pool}|rpm={rpm}|floor={floor_mode}|{case['name']}|n_cand={nc[i]}|fb={fbo[i]}|problems={len(problems)}|" + " ; ".join(problems), flush=True)
print(f"LAUNCHES|{n_launch}", flush=True)

# ---- refusals: RR_E_INVALID, the entry named, nothing written
small = ProductIndex(np.zeros((64, 64), dtype=np.float32))
dq = torch.zeros((4, 384), device=dev)
def refuse_select(what, ix=ix, nq=2, pool=150, rpm=8, floor_mode=0, cap=4, count=(2, 2), tile=None, null=None):
    big = max(cap, 4)
    a = dict(mt=np.zeros((4, big), dtype=np.uint32), count=np.array(list(count) + [0, 0], dtype=np.int32), fb=np.zeros(4, dtype=np.int32),
             tau=np.zeros(4, dtype=np.uint32), sc=np.zeros((4, big, 16), dtype=np.float32))
    if tile is not None:
        a["mt"][1, 1] = tile
    outs = [np.full((4, 2048), -1, dtype=np.int64), np.full((4, 2048), HOST_FILL, dtype=np.uint32), np.full(4, -1, dtype=np.int32), np.full(4, -1, dtype=np.int32)]
    keep = [o.copy() for o in outs]
    if null in a:
        a[null] = None
    if null is not None and null.startswith("out"):
        outs[int(null[3:])] = None
    rc, _ = select(ix, pool, rpm, floor_mode, a["mt"], a["count"], a["fb"], a["tau"], a["sc"], nq=nq, cap=cap, outs=outs)
    msg = lib.rr_last_error().decode()
    same = all(o is None or (o == k).all() for o, k in zip(outs, keep))
    print(f"REFUSE|rr_debug_select_rescored|{what}|rc={rc}|named={int('rr_debug_select_rescored' in msg)}|untouched={int(same)}", flush=True)

def refuse_rescore(what, ix=ix, nq=2, grid_x=16, use_plane=0, cap=4, count=(2, 2), tile=None, null=None):
    big = max(cap, 4)
    a = dict(dq=C.c_void_p(dq.data_ptr()), mt=np.zeros((4, big), dtype=np.uint32), count=np.array(list(count) + [0, 0], dtype=np.int32),
             fb=np.zeros(4, dtype=np.int32), tau=np.zeros(4, dtype=np.uint32), eps=np.zeros(4, dtype=np.float32))
    if tile is not None:
        a["mt"][1, 1] = tile
    sc = np.full((4, big, 8), HOST_FILL, dtype=np.uint32)
    if null in a:
        a[null] = None
    rc = lib.rr_debug_rescore_chain(ix.handle if ix is not None else None, a["dq"], nq, grid_x, use_plane, P(a["mt"]), cap, P(a["count"]), P(a["fb"]),
                                    P(a["tau"]), P(a["eps"]), None if null == "sc" else P(sc))
    msg = lib.rr_last_error().decode()
    print(f"REFUSE|rr_debug_rescore_chain|{what}|rc={rc}|named={int('rr_debug_rescore_chain' in msg)}|untouched={int((sc == HOST_FILL).all())}", flush=True)

MCAP, MAXQ = M.RR_X3_MCAP, M.RR_SEL_MAXQ
refuse_rescore("NULL index", ix=None)
for name in ("dq", "mt", "count", "fb", "tau", "eps", "sc"):
    refuse_rescore("NULL " + name, null=name)
refuse_rescore("nq = 0", nq=0)
refuse_rescore("nq = RR_SEL_MAXQ + 1", nq=MAXQ + 1)
refuse_rescore("cap = 0", cap=0, count=(0, 0))
refuse_rescore("cap = RR_X3_MCAP + 1", cap=MCAP + 1)
refuse_rescore("count = -1", count=(2, -1))
refuse_rescore("count = cap + 1", count=(5, 2))
refuse_rescore("M-tile id = number of M-tiles", tile=(M.SELECT_ROWS + 7) // 8)
refuse_rescore("dim_pad != 384", ix=small)
refuse_rescore("use_plane = 2", use_plane=2)
refuse_rescore("grid_x = 8", grid_x=8)
refuse_select("NULL index", ix=None)
for name in ("mt", "count", "fb", "tau", "sc", "out0", "out1", "out2", "out3"):
    refuse_select("NULL " + name, null=name)
refuse_select("nq = 0", nq=0)
refuse_select("nq = RR_SEL_MAXQ + 1", nq=MAXQ + 1)
refuse_select("cap = 0", cap=0, count=(0, 0))
refuse_select("cap = RR_X3_MCAP + 1", cap=MCAP + 1)
refuse_select("count = -1", count=(-1, 2))
refuse_select("count = cap + 1", count=(2, 5))
refuse_select("M-tile id = number of 8-row M-tiles", tile=(M.SELECT_ROWS + 7) // 8)
refuse_select("M-tile id = number of 16-row M-tiles", rpm=16, tile=(M.SELECT_ROWS + 15) // 16)
refuse_select("dim_pad != 384", ix=small, pool=10)
refuse_select("pool = 0", pool=0)
refuse_select("pool = RR_MAX_POOL + 1", pool=2049)
refuse_select("rows_per_mtile = 4", rpm=4)
refuse_select("floor_mode = 2", floor_mode=2)
# (a listed id just inside is taken: the 16-row id bound is half the 8-row one)
rc, _ = select(ix, 1, 8, 0, np.full((1, 1), (M.SELECT_ROWS + 7) // 8 - 1, dtype=np.uint32), np.ones(1, dtype=np.int32), np.zeros(1, dtype=np.int32),
               np.zeros(1, dtype=np.uint32), np.zeros((1, 1, 8), dtype=np.float32))
print(f"ACCEPT|last 8-row M-tile|rc={rc}", flush=True)
print("DONE")
"""


def test_selection_of_the_rescored_rows_and_what_both_entries_refuse():
    """Every case of rescore_model.selection_cases, one query each, against the model: candidate counts on both sides of
    pool, of the 1024-key sort threshold and of the key area's half (both instances), 8- and 16-row M-tiles, ties across
    M-tiles, -0.0 under +0.0, +inf where nothing may be read, the three floor_mode branches, queries flagged on entry.
    Then every invalid argument of both entries: RR_E_INVALID, the entry named in rr_last_error, outputs untouched."""
    out = _child(SELECT, 600)
    sel = _lines(out, "SEL")
    assert len(sel) == len(M.selection_cases()) and _lines(out, "LAUNCHES")[0][0] == str(len(M.selection_launches()))
    bad = [l for l in sel if _field(l, "problems") != "0"]
    assert not bad, "\n".join("|".join(l) for l in bad)
    _assert_refusals(out, 18 + 23)
    assert _lines(out, "ACCEPT")[0][1] == "rc=0" and "DONE" in out
