"""The fp32 mode's attention and LayerNorm kernels (csrc/rr_ce_h2.hip) one at a time against float64, the ce_gemm_h2
epilogue at row strides whose h2 image is larger than 4 GiB, and the attention's max_len guard.

Kernel-level checks run in a child process on the harness library (librr_hip_dbg.so: rr_debug_ce_h2_attention,
rr_debug_ce_h2_add_ln, rr_debug_ce_h2_gemm), as test_gpu_k5.py's GEMM test does.  Every accuracy case prints three errors
on the same data: the kernel's, an fp32 computation's (numpy float32: the yardstick the mode promises to match) and that of
the float64 computation on operands rounded to fp16 (what a plain fp16 kernel could reach at best).  A bar must sit within
4x the fp32 error and 10x below the fp16-operand one: a bar loose enough to let an fp16-grade defect through fails here."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from oracle import cross_encoder as OC
from review_recommender_amd import synth
from review_recommender_amd.cross_encoder import CrossEncoder

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)

# attention: max |ctx - float64| / max(sum_k p_k |v_k|, 2^-14) per score pattern (see test_h2_attention_against_float64)
ATT_BARS = {"normal": 1e-6, "dominant": 1e-6, "identical": 5e-7, "rising": 2.5e-6, "large": 1e-4, "tiny_v": 1e-6, "big_v": 1e-6}
# add-LN: max |out - float64| / max_c (|g_c xhat_c| + |b_c|) per row; "offset" = rows of 1e4 +- 1e-2, where fp32 itself
# carries only ~10 steps of the spread (ulp(1e4) = 2^-10) and its mean is off by a good part of one
LN_BARS = {"rows": 5e-7, "offset": 0.09}


def _child(src: str, timeout: int = 900) -> str:
    from review_recommender_amd.build import DEBUG_LIB_PATH
    if not DEBUG_LIB_PATH.exists():
        pytest.skip("librr_hip_dbg.so not built (python review-recommender_amd/build.py --debug)")
    p = subprocess.run([sys.executable, "-c", src.replace("@ROOT@", repr(ROOT))], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def _lines(out: str, tag: str):
    return [l.split("|")[1:] for l in out.splitlines() if l.startswith(tag + "|")]


KERNELS_CHILD = r"""
import os, sys
os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, @ROOT@)
import ctypes as C
import numpy as np, torch
from review_recommender_amd import _lib
lib = _lib.load()
dev = torch.device("cuda", 0)
QS = np.log2(np.e) / np.sqrt(32.0)               # what the QKV epilogue folds into Q
ptr = lambda t: C.c_void_p(t.data_ptr())
D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
PATTERNS = ["normal", "dominant", "identical", "rising", "large", "tiny_v", "big_v"]

# ------------------------------------------------------------------ attention
def make(pattern, S):
    # one sequence's qkv rows [S][1152] (Q scaled), a function of (pattern, S) only: the same sequence in every batch
    rng = np.random.default_rng((PATTERNS.index(pattern), S))
    q, k, v = (rng.standard_normal((S, 12, 32)) for _ in range(3))
    if pattern == "dominant":                    # one key per head 36.7 log2 units above the rest, for every query
        q[:, :, 0] = 12.0
        k[:, :, 0] = 0.0
        k[rng.integers(0, S, 12), np.arange(12), 0] = 12.0
    elif pattern == "identical":                 # every key the same: the output is the mean of V
        k[:] = k[rng.integers(0, S)]
    elif pattern == "rising":                    # scores rise 0.05 per key: a new maximum in every group, the last key's the largest
        q[:, :, 1:] *= 0.1
        k[:, :, 1:] *= 0.1
        q[:, :, 0] = 4.0
        k[:, :, 0] = np.arange(S)[:, None] * (0.05 / (4.0 * QS))
    elif pattern == "large":                     # scores of magnitude ~100: most 2^(s - m) underflow
        q *= 8.4
        k *= 8.4
    elif pattern == "tiny_v":                    # a tenth of V in and below fp16's subnormal range, some exact zeros
        tiny = rng.random(v.shape) < 0.1
        v[tiny] = 10.0 ** rng.uniform(-9, -4, tiny.sum()) * rng.choice([-1, 1], tiny.sum())
        v[rng.random(v.shape) < 0.01] = 0.0
    elif pattern == "big_v":                     # V near the top of fp16's range
        v = rng.uniform(5.5e4, 6.0e4, v.shape) * rng.choice([-1, 1], v.shape)
    return np.concatenate([q.reshape(S, 384) * QS, k.reshape(S, 384), v.reshape(S, 384)], axis=1).astype(np.float32)

def attend(x, cls, dt):
    # softmax_2(Q K^T) V in dtype dt -> ([rows][384] context, sum_k p_k |v_k|)
    S = len(x)
    q, k, v = (x[:, 384 * i:384 * (i + 1)].reshape(S, 12, 32).transpose(1, 0, 2).astype(dt) for i in range(3))
    if cls:
        q = q[:, :1]
    s = q @ k.transpose(0, 2, 1)
    p = np.exp2(s - s.max(-1, keepdims=True))
    l = p.sum(-1, keepdims=True)
    o, mag = (p @ v) / l, (p @ np.abs(v)) / l
    return o.transpose(1, 0, 2).reshape(-1, 384), mag.transpose(1, 0, 2).reshape(-1, 384)

REF = {}
def errors(pattern, S, cls, got):
    key = (pattern, S, cls)
    if key not in REF:
        x = make(pattern, S)
        ref, mag = attend(x, cls, np.float64)
        mag = np.maximum(mag, 2.0 ** -14)         # (below fp16's smallest normal an h2 value is held to 2^-36 absolute)
        f32 = attend(x, cls, np.float32)[0].astype(np.float64)
        f16 = attend(x.astype(np.float16).astype(np.float64), cls, np.float64)[0]
        REF[key] = (ref, mag, float((np.abs(f32 - ref) / mag).max()), float((np.abs(f16 - ref) / mag).max()))
    ref, mag, e32, e16 = REF[key]
    return float((np.abs(got - ref) / mag).max()), e32, e16

def run_att(x, cu, max_len, cls, kernel):
    n = len(cu) - 1
    out = torch.full((n if cls else len(x), 384), float("nan"), dtype=torch.float32, device=dev)
    dx, dcu = D(x), D(cu.astype(np.int32))
    flag = C.c_int32(-1)
    _lib.check(lib.rr_debug_ce_h2_attention(ptr(dx), len(x), ptr(dcu), n, max_len, cls, kernel, ptr(out), C.byref(flag)),
               "rr_debug_ce_h2_attention")
    return out.cpu().numpy(), flag.value

SEEN = {}                                        # (pattern, S, cls) -> bits of that sequence's context in the first run
def att_batch(name, pattern, lens, max_len=None, kernels=(0,)):
    xs = [make(pattern, S) for S in lens]
    x = np.concatenate(xs)
    cu = np.concatenate([[0], np.cumsum(lens)])
    max_len = max_len or max(lens)
    for cls in (0, 1):
        runs = {kern: run_att(x, cu, max_len, cls, kern) for kern in kernels}
        got, flag = runs[kernels[0]]
        same_kernels = all(np.array_equal(r[0].view(np.uint32), got.view(np.uint32)) for r in runs.values())
        same_seen, err, e32, e16 = True, 0.0, 0.0, 0.0
        for i, S in enumerate(lens):
            rows = got[i:i + 1] if cls else got[cu[i]:cu[i + 1]]
            bits = rows.view(np.uint32).copy()
            same_seen &= np.array_equal(SEEN.setdefault((pattern, S, cls), bits), bits)
            e, a, b = errors(pattern, S, cls, rows.astype(np.float64))
            err, e32, e16 = max(err, e), max(e32, a), max(e16, b)
        flags = [r[1] for r in runs.values()]
        print("ATT|%s|%s|%d|%s|%s|%.3e|%.3e|%.3e|%d|%d|%d" % (name, pattern, cls, ",".join(map(str, kernels)), ",".join(map(str, flags)),
              err, e32, e16, int(same_kernels), int(same_seen), int(np.isfinite(got).all())))

SMALL1 = list(range(1, 33)) + [7]                                       # max_len 32: one group per wave, 33 sequences
SMALL2 = list(range(33, 65)) + [1, 2, 17]                               # max_len 64: two groups per wave, 35 sequences
LARGE = list(range(65, 71)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 3]   # 21
P_SMALL = [1, 2, 16, 17, 31, 32, 33, 47, 48, 63, 64]
P_LARGE = [65, 97, 129, 200, 257, 385, 512]
att_batch("lengths 1-32", "normal", SMALL1, kernels=(0, 1))
att_batch("lengths 33-64", "normal", SMALL2, kernels=(0, 1))
att_batch("lengths 65-512", "normal", LARGE)
att_batch("lengths 1-70, max_len 512", "normal", list(range(1, 71)) + [33], max_len=512)
for pattern in PATTERNS:
    att_batch("short", pattern, P_SMALL, kernels=(0, 1))
    att_batch("long", pattern, P_LARGE)

# max_len below a sequence's length: that sequence's context is NaN, flag bit 2, the others as always
for name, lens, max_len, kernel in [("small kernel", [70, 5, 20], 64, 0), ("large kernel", [97, 5, 20], 96, 1)]:
    x = np.concatenate([make("normal", S) for S in lens])
    cu = np.concatenate([[0], np.cumsum(lens)])
    got, flag = run_att(x, cu, max_len, 0, kernel)
    rest = all(np.array_equal(got[cu[i]:cu[i + 1]].view(np.uint32), SEEN[("normal", lens[i], 0)]) for i in (1, 2))
    print("GUARD|%s|%d|%d|%d" % (name, flag, int(np.isnan(got[:lens[0]]).all()), int(rest)))

# ------------------------------------------------------------------ add + LayerNorm
def run_ln(y, h, g, b, eps):
    T = len(y)
    o32 = torch.full((T, 384), float("nan"), dtype=torch.float32, device=dev)
    oh = torch.full((T, 384), float("nan"), dtype=torch.float32, device=dev)
    dy, dh, dg, db = D(y), D(h), D(g), D(b)
    flag = C.c_int32(-1)
    _lib.check(lib.rr_debug_ce_h2_add_ln(ptr(dy), ptr(dh), T, ptr(dg), ptr(db), C.c_float(eps), ptr(o32), ptr(oh), C.byref(flag)),
               "rr_debug_ce_h2_add_ln")
    return o32.cpu().numpy(), oh.cpu().numpy(), flag.value

def ln(x, g, b, eps, dt):
    x = x.astype(dt)
    mu = x.mean(1, keepdims=True, dtype=dt)
    xc = x - mu
    xh = xc / np.sqrt((xc * xc).mean(1, keepdims=True, dtype=dt) + dt(eps))
    return xh * g.astype(dt) + b.astype(dt), xh

rng = np.random.default_rng(7)
def ln_case(name, T, kind, eps=1e-12, gscale=None):
    y = rng.standard_normal((T, 384)).astype(np.float32)
    h = rng.standard_normal((T, 384)).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(384)).astype(np.float32)
    b = (0.1 * rng.standard_normal(384)).astype(np.float32)
    const = np.zeros(T, bool)
    if kind == "offset":                         # a common offset of 1e4, a spread of 1e-2: a one-pass variance loses it all
        y *= np.float32(1e-2)
        h[:] = np.float32(1e4)
    elif kind == "constant":                     # rows of one value: (x - mean) = 0, the output must be b exactly
        const[::3] = True
        c = np.resize(np.array([3.0, -0.8125, 1234.5, 0.0, 1.0, -7.25], np.float32), const.sum())
        y[const] = (c - 0.5)[:, None]
        h[const] = 0.5
    if gscale is not None:
        g = (gscale * (1.0 + 0.1 * rng.standard_normal(384))).astype(np.float32)
    o32, oh, flag = run_ln(y, h, g, b, eps)
    x = y + h                                    # (fp32: the kernel's first operation, and the model's residual add)
    ref, xh = ln(x, g, b, eps, np.float64)
    den = (np.abs(g * xh) + np.abs(b)).max(1, keepdims=True)
    f32 = ln(x, g, b, eps, np.float32)[0].astype(np.float64)
    f16 = ln(x.astype(np.float16), g, b, eps, np.float64)[0]
    e = lambda a: float((np.abs(a - ref) / den).max())
    big = np.abs(o32) > 65504
    h2ok = bool((np.abs(oh.astype(np.float64) - o32)[~big] <= 2.0 ** -22 * np.abs(o32[~big]) + 2.0 ** -36).all())
    exact_b = bool((o32[const] == b[None, :]).all()) if const.any() else True
    print("LN|%s|%d|%d|%d|%.3e|%.3e|%.3e|%d|%d|%d" % (name, T, flag, int(big.any()), e(o32), e(f32), e(f16), int(h2ok), int(exact_b),
          int(np.isfinite(o32).all())))

for T in (1, 31, 32, 33, 1000, 4097):
    ln_case("N(0,1) rows", T, "normal")
for T in (33, 1000):
    ln_case("offset 1e4, spread 1e-2", T, "offset")
ln_case("constant rows", 33, "constant")
ln_case("constant rows", 4097, "constant")
ln_case("N(0,1) rows, eps 1e-5", 1000, "normal", eps=1e-5)
for gs in (1e4, 1.4e4, 2e4, 1e5):
    ln_case("g ~ %.1e" % gs, 1000, "range", gscale=gs)
"""


@pytest.fixture(scope="module")
def kernels_out():
    return _child(KERNELS_CHILD)


def test_h2_attention_against_float64(kernels_out):
    """ce_attention_h2 and ce_attention_h2_small by themselves on every length 1..70 and the query-tile / h2a_tiles edges
    (95-97, 127-129, 255-257, 383-385, 511, 512), batches of odd sequence counts (the last small-kernel workgroup partly
    empty), max_len far above the longest sequence, cls_only, and seven score / value patterns.  Error of each output
    element against sum_k p_k |v_k| of the float64 softmax (at least 2^-14: below fp16's smallest normal the h2 format
    holds a value to 2^-36 absolute, so a context element made of 1e-9-sized V alone is off by ~1e-11).
    First MI355X run -- kernel / fp32 (numpy float32) / fp16 operands, worst batch each:
      normal 5.5e-7 / 7.1e-7 / >= 3.9e-4;  dominant key (36.7 log2 units) 5.4e-7 / 6.5e-7 / 4.8e-4;
      identical keys 2.1e-7 / 1.8e-7 / 8.9e-5;  rising scores 1.3e-6 / 1.6e-6 / 4.6e-4;
      scores ~100 4.7e-5 / 6.9e-5 / 2.6e-2;  tiny V (relative to sum p|v|, before the 2^-14 floor: 9.3e-3 on 1- and
      2-token sequences, the format's absolute floor) 4.3e-7 on long ones / 8.2e-7 / 3.5e-4;  V near 6e4 3.7e-7 / 4.7e-7 / 2.7e-4."""
    rows = _lines(kernels_out, "ATT")
    assert len(rows) == 2 * (4 + 2 * len(ATT_BARS)), kernels_out
    by = {}
    for name, pattern, cls, kernels, flags, err, e32, e16, same_k, same_seen, finite in rows:
        print("%-28s %-9s cls %s kernels %-4s  kernel %s  fp32 %s  fp16 operands %s" % (name, pattern, cls, kernels, err, e32, e16))
        assert set(flags.split(",")) == {"0"} and finite == "1", (name, pattern, cls, flags)
        by.setdefault(pattern, []).append((float(err), float(e32), float(e16)))
    for pattern, bar in ATT_BARS.items():
        errs = np.array(by[pattern])
        assert errs[:, 0].max() < bar, (pattern, errs[:, 0].max(), bar)
        assert bar <= 4 * errs[:, 1].max(), (pattern, bar, errs[:, 1].max())
        assert 10 * bar <= errs[:, 2].min(), (pattern, bar, errs[:, 2].min())


def test_h2_attention_small_and_large_kernels_agree_bitwise(kernels_out):
    """For every batch with max_len <= 64 the per-wave kernel and ce_attention_h2 return the same bits, and a sequence's
    context is the same bits in every batch it appears in (alone or packed, either kernel, max_len 32, 64 or 512)."""
    rows = _lines(kernels_out, "ATT")
    small = [r for r in rows if r[3] == "0,1"]
    assert len(small) == 2 * (2 + len(ATT_BARS))
    for name, pattern, cls, kernels, flags, err, e32, e16, same_k, same_seen, finite in rows:
        assert same_k == "1", (name, pattern, cls)
        assert same_seen == "1", (name, pattern, cls)


def test_h2_attention_refuses_a_sequence_longer_than_max_len(kernels_out):
    """max_len below a sequence's length: that (sequence, every head) comes back NaN with flag bit 2 (not bit 1, the range
    bit), and every other sequence of the batch keeps its bits."""
    rows = _lines(kernels_out, "GUARD")
    assert len(rows) == 2
    for name, flag, nan, rest in rows:
        assert int(flag) & 2, name
        assert nan == "1" and rest == "1", name


def test_h2_add_ln_against_float64(kernels_out):
    """ce_h2_add_ln by itself: the fp32 rows against the float64 LayerNorm of the same fp32 sums (two-pass statistics: a
    1e4 offset with a 1e-2 spread keeps its shape), constant rows give b exactly, the h2 image is the fp32 rows to 2^-22,
    and the range flag is up exactly when an output exceeds 65504.  First MI355X run -- kernel / fp32 / fp16 input:
    N(0,1) and constant rows 2.5e-7 / 2.1e-7 / >= 2.3e-4; offset rows 6.9e-2 / 3.7e-2 / 1.0 (fp32's ulp at 1e4 is a
    tenth of the spread: the mean's rounding alone moves every output by a few per cent of its range)."""
    rows = _lines(kernels_out, "LN")
    assert len(rows) == 15, kernels_out
    flags, by = [], {}
    for name, T, flag, big, err, e32, e16, h2ok, exact_b, finite in rows:
        print("%-26s T %5s flag %s  kernel %s  fp32 %s  fp16 operands %s" % (name, T, flag, err, e32, e16))
        assert finite == "1" and h2ok == "1" and exact_b == "1", (name, T)
        assert int(flag) == int(big), (name, T, flag, big)
        flags.append(int(flag))
        if not name.startswith("g ~"):                      # (outputs beyond fp16's range: the flag cases)
            by.setdefault("offset" if name.startswith("offset") else "rows", []).append((float(err), float(e32), float(e16)))
    assert 0 in flags and 1 in flags
    for kind, bar in LN_BARS.items():
        errs = np.array(by[kind])
        assert errs[:, 0].max() < bar, (kind, errs[:, 0].max(), bar)
        assert bar <= 4 * errs[:, 1].max(), (kind, bar, errs[:, 1].max())
        assert 10 * bar <= errs[:, 2].min(), (kind, bar, errs[:, 2].min())


GEMM_WRAP_CHILD = r"""
import os, sys
os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, @ROOT@)
import ctypes as C
import numpy as np, torch
from scipy.special import erf
from review_recommender_amd import _lib
lib = _lib.load()
dev = torch.device("cuda", 0)
ptr = lambda t: C.c_void_p(t.data_ptr())
rng = np.random.default_rng(23)
K = 384
for name, epi, M, N, qcols in [("FFN-1 shape, GELU", 2, 1_400_000, 1536, 0), ("QKV shape, h2 out, Q scaled", 1, 1_870_000, 1152, 384)]:
    gen = torch.Generator(device=dev)
    gen.manual_seed(M)
    dx = torch.randn((M, K), generator=gen, device=dev)
    tiny = torch.rand((M, K), generator=gen, device=dev) < 0.1          # a tenth in and below fp16's subnormal range
    dx = torch.where(tiny, torch.pow(10.0, torch.rand((M, K), generator=gen, device=dev) * 5 - 9) * torch.sign(dx), dx)
    del tiny
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dw, db = torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=dev)
    flag = C.c_int32(-1)
    _lib.check(lib.rr_debug_ce_h2_gemm(epi, M, N, K, ptr(dx), ptr(dw), ptr(db), qcols, ptr(out), C.byref(flag)), "rr_debug_ce_h2_gemm")
    rows = np.unique(np.concatenate([[0, 1, M - 2, M - 1], rng.choice(M, 508, replace=False)]))
    ri = torch.from_numpy(rows).to(dev)
    got = out[ri].cpu().numpy().astype(np.float64)
    x = dx[ri].cpu().numpy().astype(np.float64)
    finite = bool(torch.isfinite(out).all())
    del out, dx
    torch.cuda.empty_cache()
    ref = x @ w.astype(np.float64).T + b
    mag = np.abs(x) @ np.abs(w).astype(np.float64).T + np.abs(b)
    ref[:, :qcols] *= 0.5
    mag[:, :qcols] *= 0.5
    if epi == 2:
        ref = 0.5 * ref * (1.0 + erf(ref / np.sqrt(2.0)))
    print("WRAP|%s|%d|%d|%.3e|%d" % (name, M, flag.value, float((np.abs(got - ref) / mag).max()), int(finite)))
"""


def test_h2_gemm_epilogue_past_4_gib_of_h2_image():
    """ce_gemm_h2's h2 stores at row strides whose image is larger than 4 GiB: the lo plane starts 2 N os bytes above the
    hi plane, 4.3 GB for FFN-1 at 1.4 M tokens and for QKV at 1.87 M (with 32-bit offsets both wrapped: every lo unit landed
    inside the hi plane).  512 rows -- the first, the last, random ones --, every column, against float64 at the bars of
    test_gpu_k5.py::test_h2_gemm_kernel_against_float64_products.  ~25 GB of device memory per case."""
    out = _child(GEMM_WRAP_CHILD)
    rows = _lines(out, "WRAP")
    assert len(rows) == 2, out
    for name, M, flag, err, finite in rows:
        print(name, "M", M, "error / sum|xw|:", err)
        assert int(flag) == 0 and finite == "1", name
        assert float(err) < (6e-7 if "GELU" in name else 3e-7), (name, err)


def _seqs(lens, seed, vocab=30522):
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        ids = rng.integers(0, vocab, n).astype(np.int32)
        ids[0] = 101
        out.append((ids, (np.arange(n) > n // 3).astype(np.int32)))
    return out


def test_fp32_forward_of_1_46m_tokens_in_one_call():
    """One fp32-mode call on 1.46 M tokens (the activation scratch's row stride past the FFN-1 image's 4 GiB): 671 copies
    of 8 sequences, every copy's logit the same bits as a fresh handle's on the 8 alone, and those within 2e-5 of the
    numpy oracle."""
    sd = synth.bert_state_dict(13, n_layers=6, n_labels=1)
    base = _seqs([512, 511, 385, 300, 257, 129, 64, 17], 9)
    reps = 1_460_000 // sum(len(s[0]) for s in base)
    big = CrossEncoder(sd)
    big.model.max_tokens_per_call = reps * sum(len(s[0]) for s in base)      # (one rr_ce_forward_dev call)
    got = big.predict_ids(base * reps)
    alone = CrossEncoder(sd).predict_ids(base)
    want = OC.predict_oracle(sd, base, n_layers=6)
    print("1.46 M tokens: copies differing from the lone call:", int((got.reshape(reps, 8) != alone).any(1).sum()),
          " lone call vs the oracle:", np.abs(alone - want).max())
    assert np.array_equal(got.reshape(reps, 8), np.broadcast_to(alone, (reps, 8)))
    assert np.abs(alone - want).max() < 2e-5


@pytest.mark.parametrize("lens,max_len", [([70], 64), ([100, 5, 12, 30, 3], 64), ([97, 40], 96)],
                         ids=["70 tokens, max_len 64", "100 tokens among short ones, max_len 64", "97 tokens, max_len 96"])
def test_fp32_forward_refuses_a_max_len_below_a_sequence_length(lens, max_len):
    """forward_packed_dev with a max_len below a sequence's length (the per-wave kernel for max_len <= 64, ce_attention_h2
    above): the logits are NaN and `out_of_range` raises ValueError naming max_len -- no wide-range rerun.  The same
    handle with the true max_len then matches the oracle."""
    import torch
    sd = synth.bert_state_dict(5, n_layers=2, n_labels=1, vocab=2000)
    seqs = _seqs(lens, 4, vocab=2000)
    ce = CrossEncoder(sd)
    dev = torch.device("cuda", 0)
    n = np.array(lens)
    cu = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    ids, typ = t(np.concatenate([s[0] for s in seqs])), t(np.concatenate([s[1] for s in seqs]))
    pos, dcu = t(np.arange(cu[-1]) - np.repeat(cu[:-1], n)), t(cu)
    raw = ce.model.forward_packed_dev(ids, typ, pos, dcu, len(seqs), max_len)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="max_len"):
        ce.model.out_of_range()
    assert bool(torch.isnan(raw).all())
    good = ce.model.forward_packed_dev(ids, typ, pos, dcu, len(seqs), int(n.max()))
    torch.cuda.synchronize()
    assert not ce.model.out_of_range()
    want = OC.predict_oracle(sd, seqs, n_layers=2)
    assert np.abs(good.cpu().numpy()[:, 0] - want).max() < 2e-5
