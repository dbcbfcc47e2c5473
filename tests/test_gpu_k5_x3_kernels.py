"""The fp32 mode's WIDE-RANGE kernels (csrc/rr_ce.hip: ce_gemm_x3, ce_attention_x3, ce_add_ln_f32 -- what a handle runs after a
value left fp16's range) one launch at a time against float64, at O(1) magnitudes and far beyond fp16's, and the path end to end
on models whose activations really are that large.

Kernel-level checks run in one child process on the harness library (librr_hip_dbg.so: rr_debug_ce_x3_gemm,
rr_debug_ce_x3_attention, rr_debug_ce_x3_add_ln), as tests/test_gpu_k5_h2_kernels.py does.  The reference is always numpy
float64 on the same fp32 inputs.  An accuracy case prints the kernel's error, numpy float32's on the same data (the yardstick
the mode promises to match) and a defect's (the float64 computation on operands rounded to fp16, or cut to two bf16 terms); a
bar sits within 4x the float32 error -- the rule of test_gpu_k5_h2_kernels.py -- and, for the attention and the LayerNorm, 10x
below the fp16-operand error.  On random data a lost third bf16 term is only ~5x the float32 error of a K = 384 product
(1.6e-6 against 2.7e-7 of sum |x w| on the QKV shape): that class is caught by the cases in which every output is ONE product
(test_x3_gemm_one_product_per_output, test_x3_attention_exact_gather), whose bars are derived, not measured."""
import pathlib
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import cross_encoder as OC
from review_recommender_amd import synth
from review_recommender_amd.cross_encoder import OUT_HIDDEN, CrossEncoder, QueryEncoder

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)
F32_LOGIT_TOL, F32_EMB_TOL = 1e-5, 1e-5         # tests/test_gpu_k5.py's bars of the fp32 mode
F32_HIDDEN_REL = 2e-5                            # its 5e-5 on hidden states of magnitude ~3, relative to max |hidden|

# GEMM: max |out - float64| / (sum_k |x_k w_k| + |b|) per data set (see test_x3_gemm_against_float64)
# -- twice numpy float32's own worst error on these data (3.2e-7 normal and tails, 3.7e-7 wide)
GEMM_BARS = {"normal": 6e-7, "wide": 6e-7, "tails": 6e-7}
# attention: max |ctx - float64| / sum_k p_k |v_k| per score / value pattern (see test_x3_attention_against_float64): the bars
# of test_gpu_k5_h2_kernels.py for its seven patterns; huge_v / mixed_v: numpy float32 itself is at 1.4e-6 / 1.3e-6 (one
# element of V carries the whole sum: the weights' own rounding shows undamped).  huge_scores has no constant bar, see the test.
ATT_BARS = {"normal": 1e-6, "dominant": 1e-6, "identical": 5e-7, "rising": 2.5e-6, "large": 1e-4, "tiny_v": 1e-6, "big_v": 1e-6,
            "huge_v": 2e-6, "mixed_v": 2e-6}
ATT_PATTERNS = list(ATT_BARS) + ["huge_scores"]
# add-LN: max |out - float64| / max_c (|g_c xhat_c| + |b_c|) per row; "offset" = rows of 1e4 +- 1e-2 (fp32 itself carries only
# ~10 steps of that spread), as in test_gpu_k5_h2_kernels.py
LN_BARS = {"rows": 5e-7, "offset": 0.09}
ONE_PRODUCT_BAR = 2.0 ** -21                     # derived: test_x3_gemm_one_product_per_output
GATHER_BAR = 2.0 ** -22                          # derived: test_x3_attention_exact_gather


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
from scipy.special import erf
from review_recommender_amd import _lib
lib = _lib.load()
dev = torch.device("cuda", 0)
ptr = lambda t: C.c_void_p(t.data_ptr())
D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
GUARD = 3                                        # rows behind every output that no kernel may touch
def nan_rows(rows, cols):
    return torch.full((rows + GUARD, cols), float("nan"), dtype=torch.float32, device=dev)
def untouched(t, rows):
    return int(bool(torch.isnan(t[rows:]).all()))

def run_gemm(gelu, x, w, b):
    (M, K), N = x.shape, len(w)
    out = nan_rows(M, N)
    dx, dw, db = D(x), D(w), D(b)
    _lib.check(lib.rr_debug_ce_x3_gemm(int(gelu), M, N, K, ptr(dx), ptr(dw), ptr(db), ptr(out)), "rr_debug_ce_x3_gemm")
    return out[:M].cpu().numpy(), untouched(out, M)

def run_att(x, cu):
    out = nan_rows(len(x), 384)
    dx, dcu = D(x), D(np.asarray(cu, dtype=np.int32))
    _lib.check(lib.rr_debug_ce_x3_attention(ptr(dx), len(x), ptr(dcu), len(cu) - 1, ptr(out)), "rr_debug_ce_x3_attention")
    return out[:len(x)].cpu().numpy(), untouched(out, len(x))

def run_ln(y, h, g, b, eps):
    T = len(y)
    dh = nan_rows(T, 384)
    dh[:T] = D(h)
    dy, dg, db = D(y), D(g), D(b)
    _lib.check(lib.rr_debug_ce_x3_add_ln(ptr(dy), ptr(dh), T, ptr(dg), ptr(db), C.c_float(eps)), "rr_debug_ce_x3_add_ln")
    return dh[:T].cpu().numpy(), untouched(dh, T)

# ------------------------------------------------------------------ GEMM
F32, F64 = np.float32, np.float64
def bf16(a):
    # fp32 -> the nearest bf16 (ties to even), as fp32
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)
def two_terms(a):
    # an fp32 operand cut to its first two bf16 terms (hi + mid), float64: what a split that lost its third term multiplies
    hi = bf16(a)
    return hi.astype(F64) + bf16(np.asarray(a, dtype=F32) - hi)
def m24(rng, shape):
    # random 24-bit mantissas in [1, 2)
    return rng.integers(2 ** 23, 2 ** 24, shape).astype(F64) * 2.0 ** -23
def log_uniform_m24(rng, shape, lo, hi):
    # random 24-bit mantissas, random signs, magnitudes log-uniform inside [1e<lo>, 1e<hi>]: exact in fp32
    t = 10.0 ** rng.uniform(lo + 0.31, hi - 0.31, shape)
    return np.ldexp(m24(rng, shape), np.floor(np.log2(t)).astype(np.int64)) * rng.choice([-1.0, 1.0], shape)
gelu64 = lambda z: 0.5 * z * (1.0 + erf(z / np.sqrt(2.0)))
gelu32 = lambda z: (z * F32(0.5) * (F32(1.0) + erf(z / F32(np.sqrt(2.0))))).astype(F32)
TAILS = np.array([1e5, -1e5, 40.0, -40.0], F32)

SHAPES = [(1, 128, 16), (127, 128, 16), (128, 128, 16), (129, 128, 16), (300, 1152, 384), (517, 384, 1536), (300, 1536, 384)]
for si, (M, N, K) in enumerate(SHAPES):
    gelu = (N, K) == (1536, 384)                 # the FFN-1 shape
    for data in ["normal", "wide"] + (["tails"] if gelu else []):
        rng = np.random.default_rng((31, si))    # (the same x, w, b for every data set of a shape)
        x = rng.standard_normal((M, K)).astype(F32)
        w = (rng.standard_normal((N, K)) * 0.05).astype(F32)
        tiny = rng.random((M, K)) < 0.1
        x[tiny] = (10.0 ** rng.uniform(-9, -4, tiny.sum()) * rng.choice([-1, 1], tiny.sum())).astype(F32)
        x[rng.random((M, K)) < 0.01] = 0.0
        b = rng.standard_normal(N).astype(F32)
        tail_cols = np.zeros(N, bool)
        if data == "wide":                       # 1e6 x, every eighth column back at x: outputs far beyond fp16
            x *= F32(1e6)
            x[:, ::8] *= F32(1e-6)
        elif data == "tails":                    # a quarter of the pre-activations at +-1e5 and +-40 (through the bias)
            tail_cols[rng.choice(N, N // 4, replace=False)] = True
            b[tail_cols] = np.resize(TAILS, tail_cols.sum())
        x64, w64 = x.astype(F64), w.astype(F64)
        pre = x64 @ w64.T + b
        mag = np.abs(x64) @ np.abs(w64).T + np.abs(b)
        ref = gelu64(pre) if gelu else pre
        f32 = x @ w.T + b
        f32 = (gelu32(f32) if gelu else f32).astype(F64)
        two = two_terms(x) @ two_terms(w).T + b
        two = gelu64(two) if gelu else two
        got, guard = run_gemm(gelu, x, w, b)
        finite = int(np.isfinite(got).all())
        got = got.astype(F64)
        e = lambda a: float((np.abs(a - ref) / mag).max())
        # the GELU's tails: gelu(z) is z (z >= 35) or 0 (z <= -35) to far below an fp32 ulp
        tail_err, neg_rel = 0.0, 0.0
        if tail_cols.any():
            tail_err = float((np.abs(got - np.where(pre > 0, pre, 0.0)) / mag)[:, tail_cols].max())
            neg_rel = float((np.abs(got) / np.abs(pre))[:, tail_cols & (b < 0)].max())
        print("GEMM|%s|%d|%d|%d|%d|%.3e|%.3e|%.3e|%d|%d|%.3e|%.3e" % (data, int(gelu), M, N, K, e(got), e(f32), e(two), finite, guard, tail_err, neg_rel))

# one product per output: row i of x holds one non-zero element, x[i][i]; out[i][n] = x[i][i] w[n][i]
for K in (16, 384):
    rng = np.random.default_rng((32, K))
    d = log_uniform_m24(rng, K, -15, 15)
    x = np.zeros((K, K), F32)
    x[np.arange(K), np.arange(K)] = d
    w = (m24(rng, (128, K)) * rng.choice([-1.0, 1.0], (128, K))).astype(F32)
    assert np.array_equal(x[np.arange(K), np.arange(K)].astype(F64), d) and np.abs(d).min() >= 1e-15 and np.abs(d).max() <= 1e15
    ref = d[:, None] * w.astype(F64).T           # exact: 24 x 24 bits
    two = two_terms(d.astype(F32))[:, None] * two_terms(w).T
    got, guard = run_gemm(False, x, w, np.zeros(128, F32))
    finite = int(np.isfinite(got).all())
    rel = lambda a: float((np.abs(a - ref) / np.abs(ref)).max())
    exact = int((got == ref.astype(F32)).sum())
    print("ONE|%d|%.3e|%.3e|%d|%d|%d|%d" % (K, rel(got.astype(F64)), rel(two), finite, guard, exact, got.size))

# ------------------------------------------------------------------ attention
QS = np.log2(np.e) / np.sqrt(32.0)               # the kernel's own scale: scores in base 2
PATTERNS = ["normal", "dominant", "identical", "rising", "large", "tiny_v", "big_v", "huge_v", "mixed_v", "huge_scores"]
def make(pattern, S):
    # one sequence's qkv rows [S][1152] (Q UNSCALED), a function of (pattern, S) only: the same sequence in every batch
    rng = np.random.default_rng((PATTERNS.index(pattern), S))
    q, k, v = (rng.standard_normal((S, 12, 32)) for _ in range(3))
    if pattern == "dominant":                    # one key per head 36.7 log2 units above the rest, for every query
        q[:, :, 0] = 12.0
        k[:, :, 0] = 0.0
        k[rng.integers(0, S, 12), np.arange(12), 0] = 12.0
    elif pattern == "identical":                 # every key the same: the output is the mean of V
        k[:] = k[rng.integers(0, S)]
    elif pattern == "rising":                    # scores rise 0.05 per key: a new maximum in every tile, the last key's the largest
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
    elif pattern == "huge_v":                    # V far beyond it: 25 decades
        v = 10.0 ** rng.uniform(5, 30, v.shape) * rng.choice([-1, 1], v.shape)
    elif pattern == "mixed_v":                   # twelve decades inside every head
        v = 10.0 ** rng.uniform(-6, 6, v.shape) * rng.choice([-1, 1], v.shape)
    elif pattern == "huge_scores":               # scores of magnitude ~1e5: the softmax is one key, or a near-tie of two
        q *= 300.0
        k *= 300.0
    return np.concatenate([q.reshape(S, 384), k.reshape(S, 384), v.reshape(S, 384)], axis=1).astype(F32)

def attend(x, dt):
    # softmax_2(Q K^T log2 e / sqrt 32) V in dtype dt -> ([S][384] context, sum_k p_k |v_k|)
    S = len(x)
    q, k, v = (x[:, 384 * i:384 * (i + 1)].reshape(S, 12, 32).transpose(1, 0, 2).astype(dt) for i in range(3))
    s = (q @ k.transpose(0, 2, 1)) * dt(QS)
    p = np.exp2(s - s.max(-1, keepdims=True))
    l = p.sum(-1, keepdims=True)
    o, mag = (p @ v) / l, (p @ np.abs(v)) / l
    return o.transpose(1, 0, 2).reshape(-1, 384), mag.transpose(1, 0, 2).reshape(-1, 384)

def rel_err(a, ref, mag):
    # max |a - ref| / mag; where mag = 0 (a lone key whose V element is an exact zero) the answer is 0 and nothing else will do
    d = np.abs(a - ref)
    with np.errstate(all="ignore"):
        r = np.where(mag > 0, d / mag, np.where(d == 0, 0.0, np.inf))
    return float(np.nan_to_num(r, nan=np.inf).max())

REF = {}
def errors(pattern, S, got):
    key = (pattern, S)
    if key not in REF:
        x = make(pattern, S)
        ref, mag = attend(x, F64)
        f32 = attend(x, F32)[0].astype(F64)
        with np.errstate(all="ignore"):          # (beyond fp16's range the fp16 operands are infinite: an infinite error)
            f16 = attend(x.astype(np.float16).astype(F64), F64)[0]
        REF[key] = (ref, mag, rel_err(f32, ref, mag), rel_err(f16, ref, mag))
    ref, mag, e32, e16 = REF[key]
    return rel_err(got, ref, mag), e32, e16

SEEN = {}                                        # (pattern, S) -> bits of that sequence's context in the first run
def att_batch(name, pattern, lens):
    x = np.concatenate([make(pattern, S) for S in lens])
    cu = np.concatenate([[0], np.cumsum(lens)])
    got, guard = run_att(x, cu)
    same_seen, err, e32, e16 = True, 0.0, 0.0, 0.0
    for i, S in enumerate(lens):
        rows = got[cu[i]:cu[i + 1]]
        bits = rows.view(np.uint32).copy()
        same_seen &= np.array_equal(SEEN.setdefault((pattern, S), bits), bits)
        e, a, b = errors(pattern, S, rows.astype(F64))
        err, e32, e16 = max(err, e), max(e32, a), max(e16, b)
    print("ATT|%s|%s|%d|%.3e|%.3e|%.3e|%d|%d|%d" % (name, pattern, len(lens), err, e32, e16, int(same_seen), int(np.isfinite(got).all()), guard))

EDGES = [95, 96, 97, 127, 128, 129]
LONG = [255, 256, 257, 383, 384, 385, 511, 512]
P_SMALL = [1, 2, 16, 17, 31, 32, 33, 47, 48, 63, 64]
P_LARGE = [65, 97, 129, 200, 257, 385, 512]
att_batch("lengths 1-70", "normal", list(range(1, 71)))
att_batch("lengths 70-65, tile edges", "normal", list(range(70, 64, -1)) + EDGES + [3])
att_batch("chunk edges, 511, 512", "normal", LONG)
for S in (1, 33, 70, 257, 512):
    att_batch("alone", "normal", [S])
for pattern in PATTERNS:
    att_batch("short", pattern, P_SMALL)
    att_batch("long", pattern, P_LARGE)
    att_batch("alone", pattern, [257])

# exact gather: q_i = k_pi(i) with |k| = 400 -- the softmax is exactly one key, the context is that key's V row
for S in (1, 2, 33, 257, 512):
    rng = np.random.default_rng((33, S))
    k = rng.standard_normal((S, 12, 32))
    k = (k * (400.0 / np.linalg.norm(k, axis=2, keepdims=True))).astype(F32)
    perm = np.stack([rng.permutation(S) for _ in range(12)], axis=1)                 # [S][12]: pi of every head
    q = k[perm, np.arange(12)[None, :]]
    v = log_uniform_m24(rng, (S, 12, 32), -20, 30).astype(F32)
    want = v[perm, np.arange(12)[None, :]].reshape(S, 384)
    s = np.einsum("ihd,jhd->hij", q.astype(F64), k.astype(F64)) * QS
    top = np.sort(s, axis=2)
    gap = float((top[:, :, -1] - top[:, :, -2]).min()) if S > 1 else np.inf            # log2 units between the key and the rest
    hit = bool((s.argmax(2).T == perm).all())
    got, guard = run_att(np.concatenate([q.reshape(S, 384), k.reshape(S, 384), v.reshape(S, 384)], axis=1), [0, S])
    rel = float((np.abs(got.astype(F64) - want) / np.abs(want)).max())
    print("GATHER|%d|%.3e|%d|%d|%.1f|%d|%d|%d" % (S, rel, int((got.view(np.uint32) == want.view(np.uint32)).sum()), want.size, gap, int(hit),
          int(np.isfinite(got).all()), guard))

# ------------------------------------------------------------------ add + LayerNorm
def ln(x, g, b, eps, dt):
    x = x.astype(dt)
    mu = x.mean(1, keepdims=True, dtype=dt)
    xc = x - mu
    xh = xc / np.sqrt((xc * xc).mean(1, keepdims=True, dtype=dt) + dt(eps))
    return xh * g.astype(dt) + b.astype(dt), xh

rng = np.random.default_rng(7)
def ln_case(name, T, kind, eps=1e-12, gscale=None, scale=None):
    y = rng.standard_normal((T, 384)).astype(F32)
    h = rng.standard_normal((T, 384)).astype(F32)
    g = (1.0 + 0.1 * rng.standard_normal(384)).astype(F32)
    b = (0.1 * rng.standard_normal(384)).astype(F32)
    const = np.zeros(T, bool)
    if kind == "offset":                         # a common offset of 1e4, a spread of 1e-2: a one-pass variance loses it all
        y *= F32(1e-2)
        h[:] = F32(1e4)
    elif kind == "constant":                     # rows of one value: (x - mean) = 0, the output must be b exactly
        const[::3] = True
        c = np.resize(np.array([3.0, -0.8125, 1234.5, 0.0, 1.0, -7.25], F32), const.sum())
        y[const] = (c - 0.5)[:, None]
        h[const] = 0.5
    if scale is not None:
        y *= F32(scale)
        h *= F32(scale)
    if gscale is not None:
        g = (gscale * (1.0 + 0.1 * rng.standard_normal(384))).astype(F32)
    eps = float(F32(eps))                        # (what the kernel is handed)
    got, guard = run_ln(y, h, g, b, eps)
    x = y + h                                    # (fp32: the kernel's first operation, and the model's residual add)
    ref, xh = ln(x, g, b, eps, F64)
    den = (np.abs(g * xh) + np.abs(b)).max(1, keepdims=True)
    f32 = ln(x, g, b, eps, F32)[0].astype(F64)
    with np.errstate(all="ignore"):
        e16 = float(np.nan_to_num(np.abs(ln(x.astype(np.float16), g, b, eps, F64)[0] - ref) / den, nan=np.inf).max())
    e = lambda a: float((np.abs(a - ref) / den).max())
    exact_b = bool((got[const] == b[None, :]).all()) if const.any() else True
    print("LN|%s|%d|%.3e|%.3e|%.3e|%d|%d|%d" % (name, T, e(got.astype(F64)), e(f32), e16, int(exact_b), int(np.isfinite(got).all()), guard))

for T in (1, 3, 4, 5, 1000, 4097):
    ln_case("N(0,1) rows", T, "normal")
for T in (5, 1000):
    ln_case("offset 1e4, spread 1e-2", T, "offset")
ln_case("constant rows", 5, "constant")
ln_case("constant rows", 4097, "constant")
ln_case("N(0,1) rows, eps 1e-5", 1000, "normal", eps=1e-5)
ln_case("rows of 1e6 N(0,1)", 1000, "normal", scale=1e6)
ln_case("rows of 1e-6 N(0,1), eps 1e-12", 1000, "normal", scale=1e-6)
ln_case("g ~ 1e5", 1000, "normal", gscale=1e5)

# ------------------------------------------------------------------ argument errors: a status, nothing launched
buf = nan_rows(600, 1152)
p = ptr(buf)
def cu_of(lens):
    return D(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
for name, rc in [("gemm, N = 100", lib.rr_debug_ce_x3_gemm(0, 4, 100, 16, p, p, p, p)),
                 ("gemm, K = 8", lib.rr_debug_ce_x3_gemm(0, 4, 128, 8, p, p, p, p)),
                 ("gemm, M = 0", lib.rr_debug_ce_x3_gemm(1, 0, 128, 16, p, p, p, p)),
                 ("gemm, NULL bias", lib.rr_debug_ce_x3_gemm(0, 4, 128, 16, p, p, None, p)),
                 ("attention, 513 tokens", lib.rr_debug_ce_x3_attention(p, 518, ptr(cu_of([5, 513])), 2, p)),
                 ("attention, an empty sequence", lib.rr_debug_ce_x3_attention(p, 10, ptr(cu_of([5, 0, 5])), 3, p)),
                 ("attention, cu ends before T", lib.rr_debug_ce_x3_attention(p, 12, ptr(cu_of([5, 5])), 2, p)),
                 ("attention, NULL cu", lib.rr_debug_ce_x3_attention(p, 10, None, 2, p)),
                 ("add_ln, T = 0", lib.rr_debug_ce_x3_add_ln(p, p, 0, p, p, C.c_float(1e-12))),
                 ("add_ln, NULL g", lib.rr_debug_ce_x3_add_ln(p, p, 4, None, p, C.c_float(1e-12)))]:
    print("ARG|%s|%d|%d" % (name, rc, int(bool(torch.isnan(buf).all()))))
"""


@pytest.fixture(scope="module")
def kernels_out():
    return _child(KERNELS_CHILD)


def test_x3_gemm_against_float64(kernels_out):
    """ce_gemm_x3 by itself on (M, N, K) = (1 | 127 | 128 | 129, 128, 16) and the model's QKV (300), FFN-2 (517) and FFN-1
    (300, GELU on) shapes, three data sets: `normal` (x ~ N(0,1) with a tenth of the entries at 1e-9 .. 1e-4 and 1 % zeros,
    w ~ 0.05 N(0,1)), `wide` (the same x times 1e6 with every eighth column back at x: one row spans twelve decades and the
    output is far beyond fp16) and, for the GELU, `tails` (a quarter of the pre-activations at +-1e5 and +-40: the result
    is z or 0 to fp32 rounding, never NaN).  Error against sum |x w| + |b| of the float64 product (GELU: the float64 erf
    form); the bar within 4x numpy float32's error on the same data.  No output is NaN, rows past M stay untouched.
    First MI355X run -- kernel / numpy float32 / operands cut to two bf16 terms:
      K = 16 shapes: normal <= 9.5e-8 / <= 1.7e-7 / >= 3.9e-6;  wide <= 1.2e-7 / <= 2.6e-7 / >= 3.6e-6;
      QKV 2.4e-7 / 2.7e-7 / 1.6e-6 (wide 2.8e-7 / 3.7e-7 / 1.6e-6);  FFN-2 (K = 1536) 2.3e-7 / 1.0e-7 / 6.4e-7 (wide 2.5e-7 /
      1.1e-7 / 7.2e-7);  FFN-1 + GELU 2.6e-7 / 3.2e-7 / 1.7e-6 (wide 2.8e-7 / 3.2e-7 / 1.6e-6; tails the same, against z or 0
      themselves 7.2e-8, every negative tail exactly 0).
    The two-term figure is printed, not asserted: on the K = 1536 product it is 2.8x the kernel's error, below any bar that
    float32 itself could meet.  With the a[0] b[2] MFMA taken out by hand `normal` read 3.0e-6 and failed."""
    rows = _lines(kernels_out, "GEMM")
    assert len(rows) == 15, kernels_out
    by = {}
    for data, gelu, M, N, K, err, e32, e2t, finite, guard, tail_err, neg_rel in rows:
        print("%-6s gelu %s  %4s x %4s x %4s  kernel %s  float32 %s  two bf16 terms %s  tails %s / %s" %
              (data, gelu, M, N, K, err, e32, e2t, tail_err, neg_rel))
        assert finite == "1" and guard == "1", (data, M, N, K)
        assert gelu == ("1" if (N, K) == ("1536", "384") else "0")
        # the tails against z or 0 themselves, at the data set's bar; a negative tail is 0 up to an ulp of (1 + erf) = 2^-24,
        # times z / 2, twice over
        assert float(tail_err) < GEMM_BARS[data] and float(neg_rel) <= 2.0 ** -24, (data, tail_err, neg_rel)
        by.setdefault(data, []).append((float(err), float(e32)))
    assert sorted(by) == sorted(GEMM_BARS) and len(by["tails"]) == 1
    for data, bar in GEMM_BARS.items():
        errs = np.array(by[data])
        assert errs[:, 0].max() < bar, (data, errs[:, 0].max(), bar)
        assert bar <= 4 * errs[:, 1].max(), (data, bar, errs[:, 1].max())


def test_x3_gemm_one_product_per_output(kernels_out):
    """K = 16 and 384, M = K, N = 128: row i of x is zero except x[i][i] (a random 24-bit mantissa, random sign, magnitude
    log-uniform in 1e-15 .. 1e15), w dense with random 24-bit mantissas in [1, 2), no bias -- every output is ONE fp32 x fp32
    product and every k-slot of the staging is used once.  |out - x w| <= 2^-21 |x w|, derived: the three dropped term pairs
    are below 2^-23 of the product, and the six partial products enter the accumulator with at most five roundings of
    2^-24 of a value that is at most |x w| (the first lands on zero).  The same product of operands cut to two bf16 terms
    is off by >= 10x that bar, so the bar cannot pass a lost third term.  Magnitudes stay where no term is subnormal.
    First MI355X run -- kernel / bar / two terms: K = 16 9.6e-8 / 4.8e-7 / 1.2e-5, K = 384 1.3e-7 / 4.8e-7 / 1.4e-5; 80 % of the
    outputs are the correctly rounded product.  With the a[0] b[2] MFMA taken out by hand: 7.4e-6."""
    rows = _lines(kernels_out, "ONE")
    assert [r[0] for r in rows] == ["16", "384"], kernels_out
    for K, rel, two, finite, guard, exact, total in rows:
        print("K %3s: max |out - x w| / |x w| %s (bar %.3e), two bf16 terms %s, %s of %s outputs the correctly rounded product" %
              (K, rel, ONE_PRODUCT_BAR, two, exact, total))
        assert finite == "1" and guard == "1", K
        assert float(rel) <= ONE_PRODUCT_BAR, (K, rel)
        assert float(two) >= 10 * ONE_PRODUCT_BAR, (K, two)


def test_x3_attention_against_float64(kernels_out):
    """ce_attention_x3 by itself (Q unscaled: the kernel applies log2 e / sqrt 32) on every length 1..70, the 32-query tile
    edges (95-97, 127-129: wave w owns tiles w and w + 8), the 256-key chunk edges (255-257, 383-385, 511, 512; odd lengths
    end in a lone key of a V^T pair), on the seven score / value patterns of test_gpu_k5_h2_kernels.py and three beyond
    fp16's range: |V| log-uniform in 1e5 .. 1e30, V of 1e-6 .. 1e6 inside every head, q and k times 300 (scores ~1e5: one
    key, or a near-tie of two whose weights hang on the scores' last fp32 bits).  Error of each output element against
    sum_k p_k |v_k| of the float64 softmax; a bar within 4x numpy float32's error and 10x below that of float64 on
    fp16-rounded operands (infinite where fp16 overflows).  No output NaN, the rows behind the last token untouched.
    First MI355X run -- kernel / float32 / fp16 operands (worst batch, worst batch, best batch):
      normal 8.1e-7 / 6.4e-7 / 7.2e-4;  dominant key 5.5e-7 / 6.5e-7 / 4.6e-4;  identical keys 8.6e-8 / 1.8e-7 / 4.7e-5;
      rising scores 1.2e-6 / 1.7e-6 / 4.6e-4;  scores ~100 5.8e-5 / 8.1e-5 / 6.4e-2;  tiny V 5.3e-7 / 6.6e-7 / 5.1e-4;
      V near 6e4 3.6e-7 / 5.2e-7 / 2.8e-4;  huge V 1.0e-6 / 1.4e-6 / inf;  mixed V 1.1e-6 / 1.3e-6 / inf;
      scores ~1e5: short sequences 5.6e-12 / 5.6e-12 / 1.7e-3, long ones 1.9e-2 / 4.5e-2 / 4.1e2, 257 tokens 1.5e-6 / 1.5e-6 / 4.1e2.
    With the lo term of V^T stored at the unpermuted slot by hand `normal` read 1.9e-5 and failed."""
    rows = _lines(kernels_out, "ATT")
    assert len(rows) == 3 + 5 + 3 * len(ATT_PATTERNS), kernels_out
    by = {}
    for name, pattern, n, err, e32, e16, same_seen, finite, guard in rows:
        print("%-26s %-11s %2s sequences  kernel %s  float32 %s  fp16 operands %s" % (name, pattern, n, err, e32, e16))
        assert finite == "1" and guard == "1", (name, pattern)
        by.setdefault(pattern, []).append((float(err), float(e32), float(e16)))
    assert sorted(by) == sorted(ATT_PATTERNS)
    for pattern, bar in ATT_BARS.items():
        errs = np.array(by[pattern])
        assert errs[:, 0].max() < bar, (pattern, errs[:, 0].max(), bar)
        assert bar <= 4 * errs[:, 1].max(), (pattern, bar, errs[:, 1].max())
        assert 10 * bar <= errs[:, 2].min(), (pattern, bar, errs[:, 2].min())
    # huge_scores is as ill-conditioned as its closest pair of scores: where one key wins every query (the short sequences)
    # float32 is off by 1e-11, where two scores of ~1e5 come within a few units (some query among the long ones) by
    # percents -- no constant sits within 4x of both.  Per batch: 4x numpy float32's error on that batch, at least the
    # `normal` bar, and still 10x below the fp16-operand error of the batch.
    for err, e32, e16 in by["huge_scores"]:
        bar = max(4 * e32, ATT_BARS["normal"])
        assert err < bar, ("huge_scores", err, bar)
        assert 10 * bar <= e16, ("huge_scores", bar, e16)


def test_x3_attention_same_bits_alone_and_in_any_batch(kernels_out):
    """A sequence's context is the same bits alone, among 70 others, in ascending or descending order of lengths, and for
    every pattern (the workgroup of a (sequence, head) reads nothing of its neighbours)."""
    rows = _lines(kernels_out, "ATT")
    assert sum(r[0] == "alone" for r in rows) == 5 + len(ATT_PATTERNS)
    for name, pattern, n, err, e32, e16, same_seen, finite, guard in rows:
        assert same_seen == "1", (name, pattern)


def test_x3_attention_exact_gather(kernels_out):
    """K rows of norm 400, q_i = k_pi(i) for a permutation pi per head: every query has one key thousands of log2 units above
    the rest, every other probability is exactly 0 and the context is V's row pi(i) -- V with random 24-bit mantissas,
    random signs, magnitudes log-uniform in 1e-20 .. 1e30.  Lengths 1, 2, 33, 257, 512: the key falls into every slot of
    the permuted V^T tile, into the lone last key of a pair and into the second chunk.  |ctx - V| <= 2^-22 |V| per element
    (derived: p = 1 has one non-zero term, V's three terms enter the accumulator with two roundings at most, 1 / l = 1);
    on paper the three terms add up exactly -- lo + mid fits 16 bits, + hi is V --, so every element should be
    bit-identical.  First MI355X run: all elements bit-identical at every length.  With the lo term of V^T stored at the
    unpermuted slot by hand a neighbour's lo term lands on the key: 5.6e42 at S = 33."""
    rows = _lines(kernels_out, "GATHER")
    assert [r[0] for r in rows] == ["1", "2", "33", "257", "512"], kernels_out
    for S, rel, same, total, gap, hit, finite, guard in rows:
        print("S %3s: max |ctx - V| / |V| %s, %s of %s elements bit-identical, the key leads by >= %s log2 units" % (S, rel, same, total, gap))
        assert hit == "1" and float(gap) >= 1000.0, (S, gap)          # (the data: the argmax of every query is pi)
        assert finite == "1" and guard == "1", S
        assert float(rel) <= GATHER_BAR, (S, rel)


def test_x3_add_ln_against_float64(kernels_out):
    """ce_add_ln_f32 by itself (four tokens per workgroup: T = 1, 3, 4, 5, 1000, 4097) against the float64 LayerNorm of the
    same fp32 sums: N(0,1) rows; a 1e4 offset with a 1e-2 spread (two-pass statistics keep its shape); constant rows give b
    exactly; eps = 1e-5; and, where the h2 kernel would raise its flag or lose the input, rows of 1e6 N(0,1), rows of
    1e-6 N(0,1) with eps = 1e-12 (eps is as large as the variance: its place under the square root matters) and g ~ 1e5.
    This path has no flag: finite and accurate is all.  The rows behind T stay untouched.  Bars within 4x numpy float32's
    error and 10x below the error of an fp16 input, "rows" and "offset" apart.  First MI355X run -- kernel / float32 / fp16
    input: rows 2.2e-7 / 2.1e-7 / >= 2.3e-4 (1e6 rows 2.1e-7, 1e-6 rows 1.9e-7, g ~ 1e5 2.1e-7); offset rows 6.9e-2 / 4.9e-2 /
    1.0.  With eps moved outside the square root by hand: 0.28 on the 1e-6 rows, 4.9e-6 with eps = 1e-5."""
    rows = _lines(kernels_out, "LN")
    assert len(rows) == 14, kernels_out
    by = {}
    for name, T, err, e32, e16, exact_b, finite, guard in rows:
        print("%-32s T %5s  kernel %s  float32 %s  fp16 input %s" % (name, T, err, e32, e16))
        assert finite == "1" and guard == "1" and exact_b == "1", (name, T)
        by.setdefault("offset" if name.startswith("offset") else "rows", []).append((float(err), float(e32), float(e16)))
    for kind, bar in LN_BARS.items():
        errs = np.array(by[kind])
        assert errs[:, 0].max() < bar, (kind, errs[:, 0].max(), bar)
        assert bar <= 4 * errs[:, 1].max(), (kind, bar, errs[:, 1].max())
        assert 10 * bar <= errs[:, 2].min(), (kind, bar, errs[:, 2].min())


def test_x3_harness_entries_refuse_bad_arguments(kernels_out):
    """N not a multiple of 128, K not a multiple of 16, no rows, NULL pointers, a sequence of 0 or 513 tokens, cu_seqlens that
    do not end at T: RR_E_INVALID (-1) from each entry, and nothing was launched (the buffer handed in stays NaN)."""
    rows = _lines(kernels_out, "ARG")
    assert len(rows) == 10, kernels_out
    for name, rc, untouched in rows:
        assert rc == "-1" and untouched == "1", (name, rc)


# ------------------------------------------------------------------ end to end, where the path is used
E2E_LENS = [1, 2, 17, 33, 64, 65, 100, 257]
# (name, [(key below the prefix, factor)], logits asserted)
VARIANTS = [
    ("embedding LayerNorm x 1e5", [("embeddings.LayerNorm.weight", 1e5)], True),
    ("layer 0 attention LayerNorm x 1e5", [("encoder.layer.0.attention.output.LayerNorm.weight", 1e5)], True),
    ("layer 0 FFN-1 x 4e4", [("encoder.layer.0.intermediate.dense.weight", 4e4)], True),
    ("layer 1 V x 1e6", [("encoder.layer.1.attention.self.value.weight", 1e6), ("encoder.layer.1.attention.self.value.bias", 1e6)], True),
    ("layer 1 output LayerNorm x 1e5", [("encoder.layer.1.output.LayerNorm.weight", 1e5)], False),      # saturates the pooler's tanh
]


def _seqs(lens, seed, vocab=2000):
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        ids = rng.integers(0, vocab, n).astype(np.int32)
        ids[0] = 101
        out.append((ids, (np.arange(n) > n // 3).astype(np.int32)))
    return out


def _blown_up(sd, changes):
    prefix = "bert." if "bert.embeddings.word_embeddings.weight" in sd else ""
    big = dict(sd)
    for key, factor in changes:
        big[prefix + key] = np.asarray(sd[prefix + key], dtype=np.float32) * np.float32(factor)
    return big


def _wide(handle):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        handle.model.set_wide_range(True)
    return handle


@pytest.mark.parametrize("name,changes,logits_asserted", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_wide_range_forward_on_a_model_that_needs_it(name, changes, logits_asserted):
    """A two-layer model with one weight blown up, so that ONE producer of the fp16-pair path meets a value beyond fp16's
    range -- the embedding LayerNorm, an add-LayerNorm, the GELU epilogue of FFN-1, the QKV epilogue, the last
    add-LayerNorm -- on eight sequences of 1 .. 257 tokens.  (a) A raw forward on a fresh handle leaves `out_of_range()`
    true and every logit NaN.  (b) `predict_ids` on it warns once and returns the bits of a handle that was put in wide
    range up front.  (c) Those logits are within 1e-5 of the FLOAT64 oracle and the hidden states within 2e-5 max |hidden|
    of it; the float32 oracle's own distance from the float64 one is asserted below a fifth of each bar, so that no bar
    hides an ill-conditioned case.  The last variant saturates the pooler's tanh (float32 oracle: 2.2e-5 on logits):
    hidden states only there, the logit error is printed.  First MI355X run -- kernel / float32 oracle, logits and hidden
    states (relative): 1.1e-6 / 1.1e-6 and 9.6e-7 / 7.2e-7;  1.3e-6 / 3.8e-7 and 1.1e-6 / 7.3e-7;  1.6e-6 / 8.6e-7 and 1.2e-6 /
    8.2e-7;  1.1e-6 / 5.7e-7 and 1.3e-6 / 9.9e-7;  last variant (8.0e-6 / 2.1e-5) and 1.2e-6 / 6.9e-7 of max |hidden| = 4.6e5."""
    import torch
    sd = _blown_up(synth.bert_state_dict(5, n_layers=2, n_labels=1, vocab=2000), changes)
    seqs = _seqs(E2E_LENS, 4)
    want = _wide(CrossEncoder(sd)).predict_ids(seqs)
    # (a)
    auto = CrossEncoder(sd)
    dev = torch.device("cuda", 0)
    lens = np.array(E2E_LENS)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    ids, typ = t(np.concatenate([s[0] for s in seqs])), t(np.concatenate([s[1] for s in seqs]))
    pos = t(np.arange(cu[-1]) - np.repeat(cu[:-1], lens))
    raw = auto.model.forward_packed_dev(ids, typ, pos, t(cu), len(seqs), int(lens.max()))
    torch.cuda.synchronize()
    assert auto.model.out_of_range()
    assert bool(torch.isnan(raw).all())
    # (b)
    with pytest.warns(UserWarning, match="fp16 range") as rec:
        got = auto.predict_ids(seqs)
        again = auto.predict_ids(seqs)
    assert len([w for w in rec if "fp16 range" in str(w.message)]) == 1
    assert auto.model.wide_range and not auto.model.out_of_range()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(again.view(np.uint32), want.view(np.uint32))
    # (c)
    o64 = OC.predict_oracle(sd, seqs, n_layers=2, dtype=np.float64)
    o32 = OC.predict_oracle(sd, seqs, n_layers=2)
    h64 = np.concatenate([OC.bert_hidden(sd, *s, n_layers=2, dtype=np.float64) for s in seqs])
    h32 = np.concatenate([OC.bert_hidden(sd, *s, n_layers=2) for s in seqs])
    hid = auto.model.forward_ids(seqs, OUT_HIDDEN)
    scale = np.abs(h64).max()
    print("%s: logits  kernel %.3e  float32 oracle %.3e (of the float64 oracle);  hidden / max |hidden| = %.3g:  kernel %.3e  float32 oracle %.3e"
          % (name, np.abs(got - o64).max(), np.abs(o32 - o64).max(), scale, np.abs(hid - h64).max() / scale, np.abs(h32 - h64).max() / scale))
    assert np.isfinite(got).all() and np.isfinite(hid).all()
    assert np.abs(h32 - h64).max() < F32_HIDDEN_REL / 5 * scale
    assert np.abs(hid - h64).max() < F32_HIDDEN_REL * scale
    if logits_asserted:
        assert np.abs(o32 - o64).max() < F32_LOGIT_TOL / 5
        assert np.abs(got - o64).max() < F32_LOGIT_TOL


def test_wide_range_logits_do_not_depend_on_batch_composition_or_chunking():
    """A wide-range handle on a model that needs it (embedding LayerNorm x 1e5: every activation of the first layer is
    ~1e5) and on the plain one: logits bitwise the same alone, reversed, and across max_tokens_per_call = 700 chunks;
    OUT_CLS rows likewise."""
    base = synth.bert_state_dict(5, n_layers=2, n_labels=1, vocab=2000)
    seqs = _seqs(E2E_LENS + [300, 512, 129, 31], 6)
    for sd in (base, _blown_up(base, VARIANTS[0][1])):
        ce = _wide(CrossEncoder(sd))
        got = ce.predict_ids(seqs)
        assert np.isfinite(got).all() and not ce.model.out_of_range()
        alone = np.concatenate([ce.predict_ids([s]) for s in seqs])
        assert np.array_equal(got.view(np.uint32), alone.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), ce.predict_ids(seqs[::-1])[::-1].view(np.uint32))
        cls = ce.model.forward_ids(seqs, 1)
        chunked = _wide(CrossEncoder(sd))
        chunked.model.max_tokens_per_call = 700
        assert np.array_equal(got.view(np.uint32), chunked.predict_ids(seqs).view(np.uint32))
        assert np.array_equal(cls.view(np.uint32), chunked.model.forward_ids(seqs, 1).view(np.uint32))
        assert np.array_equal(cls[:3].view(np.uint32), np.concatenate([ce.model.forward_ids([s], 1) for s in seqs[:3]]).view(np.uint32))


def test_wide_range_query_encoder_matches_the_transformers_fixture():
    """The 12-layer query encoder on the wide-range kernels: embeddings within the fp32 mode's 1e-5 of `transformers`."""
    fx = np.load(GOLDEN / "k5_query_encoder.npz")
    sd = synth.bert_state_dict(int(fx["seed"]), n_layers=12, n_labels=0, prefix="")
    enc = _wide(QueryEncoder(sd))
    cu = fx["cu_seqlens"]
    seqs = [(fx["token_ids"][cu[i]:cu[i + 1]], fx["type_ids"][cu[i]:cu[i + 1]]) for i in range(len(cu) - 1)]
    emb = enc.encode_ids(seqs, normalize_embeddings=True)
    assert enc.model.wide_range and not enc.model.out_of_range()
    print("wide-range query encoder: max |embedding error|", np.abs(emb - fx["embeddings"]).max())
    assert np.abs(emb - fx["embeddings"]).max() < F32_EMB_TOL
    assert (emb * fx["embeddings"]).sum(axis=1).min() > 1 - 1e-6
