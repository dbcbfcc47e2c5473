"""`ce_pool_mean` (csrc/rr_ce_pool.hip: RR_CE_OUT_MEAN's kernel) ONE launch at a time on host-made rows, in one child process on
the harness library (librr_hip_dbg.so: rr_debug_ce_pool_mean), as tests/test_gpu_k5_x3_kernels.py runs its kernels.

Every output must be `cross_encoder.model_pool_mean` bit for bit -- the summation order is the contract -- and within the
float64 bar of tests/test_pool_model.py (tests/pool_model.py: twice numpy float32's own worst error on the same rows, computed here); rows behind
the output stay untouched; what the entry refuses it refuses with RR_E_INVALID before anything is launched."""
import pathlib
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)
HIDDEN = [128, 384, 1024]
DATA = ["normal", "offset"]

CHILD = r"""
import os, sys
os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, @ROOT@)
sys.path.insert(0, os.path.join(@ROOT@, "tests"))
import ctypes as C
import numpy as np, torch
from review_recommender_amd import _lib
from review_recommender_amd.cross_encoder import model_pool_mean
from pool_model import bits, pool_errors, rows_of
lib = _lib.load()
dev = torch.device("cuda", 0)
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
GUARD = 3                                        # rows behind every output that the kernel may not touch

def call(rows, cu, hidden, n_seqs=None, T=None, null=None):
    n = len(cu) - 1 if n_seqs is None else n_seqs
    out = torch.full((max(n, 1) + GUARD, hidden), float("nan"), dtype=torch.float32, device=dev)
    d_rows, d_cu = D(rows), D(np.asarray(cu, dtype=np.int32))
    args = {"rows": d_rows, "cu": d_cu, "out": out}
    if null:
        args[null] = None
    rc = lib.rr_debug_ce_pool_mean(ptr(args["rows"]), len(rows) if T is None else T, ptr(args["cu"]), n, hidden, ptr(args["out"]))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), n

for hidden in (128, 384, 1024):
    for data in ("normal", "offset"):
        for name, lengths in (("batch", [1, 2, 3, 4, 5, 63, 64, 65, 512]), ("single", [77])):
            rows, cu = rows_of(hidden, data, lengths, seed=11)
            rc, out, n = call(rows, cu, hidden)
            want = model_pool_mean(rows, cu)
            same = int(rc == 0 and np.array_equal(bits(out[:n]), bits(want)))
            err, err_np = pool_errors(out[:n], rows, cu) if rc == 0 and np.isfinite(out[:n]).all() else (float("inf"), 0.0)
            print(f"POOL|{hidden}|{data}|{name}|{rc}|{same}|{err:.6e}|{err_np:.6e}|{int(np.isnan(out[n:]).all())}", flush=True)

# refusals: RR_E_INVALID (-1), nothing launched, the output as it was
rows, cu = rows_of(384, "normal", [4, 3, 5], seed=12)
wide = np.zeros((12, 1152), dtype=np.float32)
cases = {"empty_sequence": dict(rows=rows, cu=[0, 4, 4, 12], hidden=384),
         "cu_short_of_T": dict(rows=rows, cu=[0, 4, 7, 11], hidden=384),
         "cu_not_from_0": dict(rows=rows, cu=[1, 4, 7, 12], hidden=384),
         "too_long": dict(rows=np.zeros((513, 128), dtype=np.float32), cu=[0, 513], hidden=128),
         "hidden_96": dict(rows=wide[:, :96], cu=cu, hidden=96),
         "hidden_1152": dict(rows=wide, cu=cu, hidden=1152),
         "null_rows": dict(rows=rows, cu=cu, hidden=384, null="rows"),
         "null_cu": dict(rows=rows, cu=cu, hidden=384, null="cu"),
         "null_out": dict(rows=rows, cu=cu, hidden=384, null="out"),
         "no_sequences": dict(rows=rows, cu=cu, hidden=384, n_seqs=0)}
for name, kw in cases.items():
    rc, out, _ = call(**kw)
    print(f"REFUSED|{name}|{rc}|{int(np.isnan(out).all())}|{lib.rr_last_error().decode()}", flush=True)
rc, out, n = call(rows, cu, 384)                 # ... and the handle-less entry still works after them
print(f"AFTER|{rc}|{int(np.array_equal(bits(out[:n]), bits(model_pool_mean(rows, cu))))}", flush=True)
"""


@pytest.fixture(scope="module")
def child():
    from review_recommender_amd.build import DEBUG_LIB_PATH
    if not DEBUG_LIB_PATH.exists():
        pytest.skip("librr_hip_dbg.so not built (python review-recommender_amd/build.py --debug)")
    p = subprocess.run([sys.executable, "-c", CHILD.replace("@ROOT@", repr(ROOT))], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    print(p.stdout)
    return p.stdout


def lines(out, tag):
    return [l.split("|")[1:] for l in out.splitlines() if l.startswith(tag + "|")]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("hidden", HIDDEN)
def test_pool_kernel_is_the_model_bit_for_bit_and_within_the_float64_bar(child, hidden, data):
    got = [l for l in lines(child, "POOL") if l[0] == str(hidden) and l[1] == data]
    assert [l[2] for l in got] == ["batch", "single"]
    for _, _, name, rc, same, err, err_np, untouched in got:
        print(f"hidden {hidden} {data} {name}: kernel {err}, numpy float32 {err_np}")
        assert rc == "0" and same == "1", (name, rc, same)
        assert float(err) <= 2 * float(err_np), (name, err, err_np)
        assert untouched == "1", name


def test_pool_entry_refuses_before_it_launches(child):
    got = {l[0]: l[1:] for l in lines(child, "REFUSED")}
    assert set(got) == {"empty_sequence", "cu_short_of_T", "cu_not_from_0", "too_long", "hidden_96", "hidden_1152", "null_rows", "null_cu",
                        "null_out", "no_sequences"}
    for name, (rc, untouched, msg) in got.items():
        assert rc == "-1" and untouched == "1", (name, rc, untouched, msg)          # RR_E_INVALID, the output as it was
        assert "rr_debug_ce_pool_mean" in msg, (name, msg)
    assert "has 0 tokens" in got["empty_sequence"][2] and "513 tokens" in got["too_long"][2]
    assert "not from 0 to 12" in got["cu_short_of_T"][2] and "hidden 96" in got["hidden_96"][2] and "hidden 1152" in got["hidden_1152"][2]
    assert lines(child, "AFTER") == [["0", "1"]]
