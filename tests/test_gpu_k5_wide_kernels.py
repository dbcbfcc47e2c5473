"""The encoder's runtime-shape kernels (csrc/rr_ce_w.hip: ce_attention_x3w<32 | 64>, ce_add_ln_w, ce_embed_ln_w -- what a handle
of any block shape other than 384 / 12 / 1536 runs) one launch at a time against float64.

Everything runs in one child process on the harness library (librr_hip_dbg.so: rr_debug_ce_w_attention, rr_debug_ce_w_add_ln,
rr_debug_ce_w_embed_ln), as tests/test_gpu_k5_x3_kernels.py does, and follows its rule for every tolerance: the reference is numpy
float64 on the same fp32 inputs; a case prints the kernel's error, numpy float32's on the same data and -- for the attention --
that of the float64 computation on operands cut to two bf16 terms; a bar is a constant within 4x the float32 error (asserted).
Every bar below is TWICE numpy float32's worst error on these data (that file's GEMM rule), set from numpy's figures alone --
they need no GPU -- before the kernels first ran.  On random data a lost third bf16 term is only 3x .. 13x the float32 error
(test_wide_attention_against_float64 lists both), so no constant can be above float32's error and 10x below the two-term one:
the two-term figure is printed there, not asserted (that file asserts its 10x margin for the attention against an
fp16-operand model, which is 500x float32's error; for its GEMM it prints the two-term figure as this file does).  What
that leaves: a lost third term of V is caught by the exact gather, whose derived bar sits 10x below the two-term error
(asserted); a lost third term of Q, K or P on random data is guarded only by the bars of twice float32's error -- a term
lost altogether moves `normal` to 3.2e-6 or more against a bar of 2.2e-6, but with little room."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)

ATT_SHAPES = [(128, 2), (768, 12), (1024, 16), (256, 8)]          # (hidden, heads): head dim 64, 64, 64, 32
ATT_PATTERNS = ["normal", "dominant", "identical", "rising", "large", "huge_v", "mixed_v"]
# attention: max |ctx - float64| / sum_k p_k |v_k| per pattern, over the four shapes (see test_wide_attention_against_float64)
# -- twice numpy float32's own worst error over the shapes: 1.10e-6, 2.11e-6, 1.57e-7, 1.81e-6, 1.07e-4, 1.97e-6, 1.48e-6
ATT_BARS = {"normal": 2.2e-6, "dominant": 4.2e-6, "identical": 3.1e-7, "rising": 3.6e-6, "large": 2.1e-4, "huge_v": 3.9e-6, "mixed_v": 3.0e-6}
# LayerNorm kernels: max |out - float64| / max_c (|g_c xhat_c| + |b_c|) per row
# -- twice numpy float32's worst on the add-LayerNorm data (2.21e-7)
LN_BAR = 4.4e-7
GATHER_BAR = 2.0 ** -22                          # derived: tests/test_gpu_k5_x3_kernels.py, test_x3_attention_exact_gather


def _child(src: str, timeout: int = 900) -> str:
    from review_recommender_amd.build import DEBUG_LIB_PATH
    assert DEBUG_LIB_PATH.exists(), "librr_hip_dbg.so is missing: __graft_entry__.build() builds it"
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
from review_recommender_amd import _lib, synth
from review_recommender_amd.cross_encoder import BertEncoderGPU
lib = _lib.load()
dev = torch.device("cuda", 0)
ptr = lambda t: C.c_void_p(t.data_ptr())
D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
GUARD = 3                                        # rows behind every output that no kernel may touch
def nan_rows(rows, cols):
    return torch.full((rows + GUARD, cols), float("nan"), dtype=torch.float32, device=dev)
def untouched(t, rows):
    return int(bool(torch.isnan(t[rows:]).all()))

def run_att(x, cu, hidden, heads, entry="w"):
    out = nan_rows(len(x), hidden)
    dx, dcu = D(x), D(np.asarray(cu, dtype=np.int32))
    if entry == "w":
        _lib.check(lib.rr_debug_ce_w_attention(ptr(dx), len(x), ptr(dcu), len(cu) - 1, hidden, heads, ptr(out)), "rr_debug_ce_w_attention")
    else:
        _lib.check(lib.rr_debug_ce_x3_attention(ptr(dx), len(x), ptr(dcu), len(cu) - 1, ptr(out)), "rr_debug_ce_x3_attention")
    return out[:len(x)].cpu().numpy(), untouched(out, len(x))

def run_ln(y, h, g, b, eps, entry="w"):
    T, H = y.shape
    dh = nan_rows(T, H)
    dh[:T] = D(h)
    dy, dg, db = D(y), D(g), D(b)
    if entry == "w":
        _lib.check(lib.rr_debug_ce_w_add_ln(ptr(dy), ptr(dh), T, H, ptr(dg), ptr(db), C.c_float(eps)), "rr_debug_ce_w_add_ln")
    else:
        _lib.check(lib.rr_debug_ce_x3_add_ln(ptr(dy), ptr(dh), T, ptr(dg), ptr(db), C.c_float(eps)), "rr_debug_ce_x3_add_ln")
    return dh[:T].cpu().numpy(), untouched(dh, T)

def run_embed(model, tok, typ, pos, entry="w"):
    T, H = len(tok), model.hidden
    out = nan_rows(T, H)
    dt, dy, dp = (D(np.asarray(a, dtype=np.int32)) for a in (tok, typ, pos))
    if entry == "w":
        _lib.check(lib.rr_debug_ce_w_embed_ln(model.handle, ptr(dt), ptr(dy), ptr(dp), T, ptr(out)), "rr_debug_ce_w_embed_ln")
    else:
        hb = torch.zeros((T, H), dtype=torch.int16, device=dev)
        _lib.check(lib.rr_debug_ce_embed_ln(model.handle, ptr(dt), ptr(dy), ptr(dp), T, ptr(out), ptr(hb)), "rr_debug_ce_embed_ln")
    return out[:T].cpu().numpy(), untouched(out, T)

# ---- data and references
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
    return rng.integers(2 ** 23, 2 ** 24, shape).astype(F64) * 2.0 ** -23
def log_uniform_m24(rng, shape, lo, hi):
    t = 10.0 ** rng.uniform(lo + 0.31, hi - 0.31, shape)
    return np.ldexp(m24(rng, shape), np.floor(np.log2(t)).astype(np.int64)) * rng.choice([-1.0, 1.0], shape)

# ------------------------------------------------------------------ attention
PATTERNS = ["normal", "dominant", "identical", "rising", "large", "huge_v", "mixed_v"]
def make(pattern, S, NH, HD):
    # one sequence's qkv rows [S][3 NH HD] (Q UNSCALED), a function of (pattern, S, NH, HD) only: the same sequence in every batch
    QS = np.log2(np.e) / np.sqrt(float(HD))
    rng = np.random.default_rng((PATTERNS.index(pattern), S, NH, HD))
    q, k, v = (rng.standard_normal((S, NH, HD)) for _ in range(3))
    if pattern == "dominant":                    # one key per head far above the rest, for every query
        q[:, :, 0] = 12.0
        k[:, :, 0] = 0.0
        k[rng.integers(0, S, NH), np.arange(NH), 0] = 12.0
    elif pattern == "identical":                 # every key the same: the output is the mean of V
        k[:] = k[rng.integers(0, S)]
    elif pattern == "rising":                    # scores rise 0.05 per key: a new maximum in every tile, the last key's the largest
        q[:, :, 1:] *= 0.1
        k[:, :, 1:] *= 0.1
        q[:, :, 0] = 4.0
        k[:, :, 0] = np.arange(S)[:, None] * (0.05 / (4.0 * QS))
    elif pattern == "large":                     # scores of magnitude ~100 at any head dim (8.4^2 log2 e): most 2^(s - m) underflow
        q *= 8.4
        k *= 8.4
    elif pattern == "huge_v":                    # V far beyond fp16's range: 25 decades
        v = 10.0 ** rng.uniform(5, 30, v.shape) * rng.choice([-1, 1], v.shape)
    elif pattern == "mixed_v":                   # twelve decades inside every head
        v = 10.0 ** rng.uniform(-6, 6, v.shape) * rng.choice([-1, 1], v.shape)
    H = NH * HD
    return np.concatenate([q.reshape(S, H), k.reshape(S, H), v.reshape(S, H)], axis=1).astype(F32)

def attend(x, NH, HD, dt):
    # softmax_2(Q K^T log2 e / sqrt HD) V in dtype dt -> ([S][H] context, sum_k p_k |v_k|)
    S, H = len(x), NH * HD
    q, k, v = (x[:, H * i:H * (i + 1)].reshape(S, NH, HD).transpose(1, 0, 2).astype(dt) for i in range(3))
    s = (q @ k.transpose(0, 2, 1)) * dt(np.log2(np.e) / np.sqrt(float(HD)))
    p = np.exp2(s - s.max(-1, keepdims=True))
    l = p.sum(-1, keepdims=True)
    o, mag = (p @ v) / l, (p @ np.abs(v)) / l
    return o.transpose(1, 0, 2).reshape(-1, H), mag.transpose(1, 0, 2).reshape(-1, H)

def rel_err(a, ref, mag):
    d = np.abs(a - ref)
    with np.errstate(all="ignore"):
        r = np.where(mag > 0, d / mag, np.where(d == 0, 0.0, np.inf))
    return float(np.nan_to_num(r, nan=np.inf).max())

REF = {}
def errors(pattern, S, NH, HD, got):
    key = (pattern, S, NH, HD)
    if key not in REF:
        x = make(pattern, S, NH, HD)
        ref, mag = attend(x, NH, HD, F64)
        f32 = attend(x, NH, HD, F32)[0].astype(F64)
        two = attend(two_terms(x), NH, HD, F64)[0]
        REF[key] = (ref, mag, rel_err(f32, ref, mag), rel_err(two, ref, mag))
    ref, mag, e32, e2t = REF[key]
    return rel_err(got, ref, mag), e32, e2t

SEEN = {}                                        # (pattern, S, NH, HD) -> bits of that sequence's context in the first run
def att_batch(name, pattern, lens, hidden, NH):
    HD = hidden // NH
    x = np.concatenate([make(pattern, S, NH, HD) for S in lens])
    cu = np.concatenate([[0], np.cumsum(lens)])
    got, guard = run_att(x, cu, hidden, NH)
    same_seen, err, e32, e2t = True, 0.0, 0.0, 0.0
    for i, S in enumerate(lens):
        rows = got[cu[i]:cu[i + 1]]
        bits = rows.view(np.uint32).copy()
        same_seen &= np.array_equal(SEEN.setdefault((pattern, S, NH, HD), bits), bits)
        e, a, b = errors(pattern, S, NH, HD, rows.astype(F64))
        err, e32, e2t = max(err, e), max(e32, a), max(e2t, b)
    print("ATT|%d|%d|%s|%s|%d|%.3e|%.3e|%.3e|%d|%d|%d" % (hidden, NH, name, pattern, len(lens), err, e32, e2t, int(same_seen),
          int(np.isfinite(got).all()), guard))

EDGES = [95, 96, 97, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512]
P_LENS = [1, 2, 33, 64, 129, 257]
for hidden, NH in [(128, 2), (768, 12), (1024, 16), (256, 8)]:
    att_batch("lengths 1-70", "normal", list(range(1, 71)), hidden, NH)
    att_batch("tile and chunk edges", "normal", EDGES[::-1], hidden, NH)
    for S in (1, 33, 70, 129, 512):
        att_batch("alone", "normal", [S], hidden, NH)
    for pattern in PATTERNS[1:]:
        att_batch("patterns", pattern, P_LENS, hidden, NH)
        att_batch("alone", pattern, [129], hidden, NH)

# exact gather at head dim 64: q_i = k_pi(i) with |k| = 400 -- the softmax is exactly one key, the context is that key's V row
NH, HD = 2, 64
for S in (1, 2, 33, 129, 257, 512):
    rng = np.random.default_rng((33, S))
    k = rng.standard_normal((S, NH, HD))
    k = (k * (400.0 / np.linalg.norm(k, axis=2, keepdims=True))).astype(F32)
    perm = np.stack([rng.permutation(S) for _ in range(NH)], axis=1)                 # [S][NH]: pi of every head
    q = k[perm, np.arange(NH)[None, :]]
    v = log_uniform_m24(rng, (S, NH, HD), -20, 30).astype(F32)
    want = v[perm, np.arange(NH)[None, :]].reshape(S, NH * HD)
    s = np.einsum("ihd,jhd->hij", q.astype(F64), k.astype(F64)) * (np.log2(np.e) / 8.0)
    top = np.sort(s, axis=2)
    gap = float((top[:, :, -1] - top[:, :, -2]).min()) if S > 1 else np.inf            # log2 units between the key and the rest
    hit = bool((s.argmax(2).T == perm).all())
    got, guard = run_att(np.concatenate([q.reshape(S, -1), k.reshape(S, -1), v.reshape(S, -1)], axis=1), [0, S], NH * HD, NH)
    rel = float((np.abs(got.astype(F64) - want) / np.abs(want)).max())
    two = float((np.abs(two_terms(want) - want) / np.abs(want)).max())               # the same gather of a V cut to two bf16 terms
    print("GATHER|%d|%.3e|%d|%d|%.1f|%d|%d|%d|%.3e" % (S, rel, int((got.view(np.uint32) == want.view(np.uint32)).sum()), want.size, gap, int(hit),
          int(np.isfinite(got).all()), guard, two))

# ------------------------------------------------------------------ add + LayerNorm, embedding + LayerNorm
def ln(x, g, b, eps, dt):
    x = x.astype(dt)
    mu = x.mean(1, keepdims=True, dtype=dt)
    xc = x - mu
    xh = xc / np.sqrt((xc * xc).mean(1, keepdims=True, dtype=dt) + dt(eps))
    return xh * g.astype(dt) + b.astype(dt), xh

def ln_report(tag, name, H, T, got, guard, x, g, b, eps, const):
    ref, xh = ln(x, g, b, eps, F64)
    den = (np.abs(g * xh) + np.abs(b)).max(1, keepdims=True)
    f32 = ln(x, g, b, eps, F32)[0].astype(F64)
    e = lambda a: float((np.abs(a - ref) / den).max())
    exact_b = bool((got[const] == b[None, :]).all()) if const.any() else True
    print("%s|%s|%d|%d|%.3e|%.3e|%d|%d|%d" % (tag, name, H, T, e(got.astype(F64)), e(f32), int(exact_b), int(np.isfinite(got).all()), guard))

CONSTS = np.array([3.0, -0.8125, 1234.5, 0.0, 1.0, -7.25], F32)
EPS = float(F32(1e-12))
for H in (128, 768, 1024):
    rng = np.random.default_rng((7, H))
    for name, Ts, kind, scale in [("N(0,1) rows", (1, 3, 4, 5, 1000), "normal", None), ("constant rows", (5, 1000), "constant", None),
                                  ("rows of 1e6 N(0,1)", (1000,), "normal", 1e6), ("rows of 1e-6 N(0,1), eps 1e-12", (1000,), "normal", 1e-6)]:
        for T in Ts:
            y = rng.standard_normal((T, H)).astype(F32)
            h = rng.standard_normal((T, H)).astype(F32)
            g = (1.0 + 0.1 * rng.standard_normal(H)).astype(F32)
            b = (0.1 * rng.standard_normal(H)).astype(F32)
            const = np.zeros(T, bool)
            if kind == "constant":               # rows of one value: (x - mean) = 0, the output must be b exactly
                const[::3] = True
                c = np.resize(CONSTS, const.sum())
                y[const] = (c - 0.5)[:, None]
                h[const] = 0.5
            if scale is not None:
                y *= F32(scale)
                h *= F32(scale)
            got, guard = run_ln(y, h, g, b, EPS)
            ln_report("LN", name, H, T, got, guard, y + h, g, b, EPS, const)      # (y + h in fp32: the kernel's first operation)

def tiny_model(H, seed, scale=None, constant=False, precision="fp32"):
    ffn = 1536 if H == 384 else 128
    sd = synth.bert_state_dict(seed, n_layers=1, hidden=H, ffn=ffn, vocab=64, max_pos=512, n_labels=0, prefix="")
    rng = np.random.default_rng((9, H, seed))
    for key in ("word_embeddings", "position_embeddings", "token_type_embeddings"):
        w = rng.standard_normal(sd["embeddings." + key + ".weight"].shape).astype(F32)
        if constant:                             # every table row one value: the sum is constant along the row
            w[:] = np.resize(CONSTS, len(w))[:, None]
        if scale is not None:
            w *= F32(scale)
        sd["embeddings." + key + ".weight"] = w
    sd["embeddings.LayerNorm.weight"] = (1.0 + 0.1 * rng.standard_normal(H)).astype(F32)
    sd["embeddings.LayerNorm.bias"] = (0.1 * rng.standard_normal(H)).astype(F32)
    return BertEncoderGPU(sd, with_head=False, precision=precision, n_heads=12 if H == 384 else H // 64), sd

def embed_ids(T, seed):
    rng = np.random.default_rng((11, T, seed))
    return rng.integers(0, 64, T), rng.integers(0, 2, T), rng.integers(0, 512, T)

for H in (128, 768, 1024):
    for name, Ts, kw in [("N(0,1) rows", (1, 3, 4, 5, 1000), {}), ("constant rows", (5, 1000), {"constant": True}),
                         ("rows of 1e6 N(0,1)", (1000,), {"scale": 1e6}), ("rows of 1e-6 N(0,1), eps 1e-12", (1000,), {"scale": 1e-6})]:
        model, sd = tiny_model(H, 1, **kw)
        for T in Ts:
            tok, typ, pos = embed_ids(T, H)
            got, guard = run_embed(model, tok, typ, pos)
            x = (sd["embeddings.word_embeddings.weight"][tok] + sd["embeddings.token_type_embeddings.weight"][typ]) \
                + sd["embeddings.position_embeddings.weight"][pos]             # (fp32, in the kernel's order)
            ln_report("ELN", name, H, T, got, guard, x, sd["embeddings.LayerNorm.weight"], sd["embeddings.LayerNorm.bias"], EPS,
                      np.full(T, bool(kw.get("constant"))))
        model.close()

# ------------------------------------------------------------------ the bits of the 384 kernels on (384, 12) inputs
for pattern, lens in [("normal", list(range(1, 71))), ("normal", EDGES), ("large", P_LENS), ("mixed_v", P_LENS)]:
    x = np.concatenate([make(pattern, S, 12, 32) for S in lens])
    cu = np.concatenate([[0], np.cumsum(lens)])
    a, b = run_att(x, cu, 384, 12)[0], run_att(x, cu, 384, 12, entry="x3")[0]
    print("SAME|attention %s, %d sequences|%d|%d" % (pattern, len(lens), int(np.array_equal(a.view(np.uint32), b.view(np.uint32))), int(np.isfinite(a).all())))
rng = np.random.default_rng(13)
for T, scale in [(1, 1.0), (5, 1.0), (1000, 1.0), (1000, 1e6), (1000, 1e-6)]:
    y, h = (rng.standard_normal((T, 384)).astype(F32) * F32(scale) for _ in range(2))
    g, b = (1.0 + 0.1 * rng.standard_normal(384)).astype(F32), (0.1 * rng.standard_normal(384)).astype(F32)
    a, c = run_ln(y, h, g, b, EPS)[0], run_ln(y, h, g, b, EPS, entry="x3")[0]
    print("SAME|add_ln T %d scale %g|%d|%d" % (T, scale, int(np.array_equal(a.view(np.uint32), c.view(np.uint32))), int(np.isfinite(a).all())))
for scale in (None, 1e6, 1e-6):
    model, sd = tiny_model(384, 2, scale=scale, precision="bf16")
    for T in (1, 5, 1000):
        tok, typ, pos = embed_ids(T, 384)
        a, c = run_embed(model, tok, typ, pos)[0], run_embed(model, tok, typ, pos, entry="bf16")[0]
        print("SAME|embed_ln T %d scale %s|%d|%d" % (T, scale, int(np.array_equal(a.view(np.uint32), c.view(np.uint32))), int(np.isfinite(a).all())))
    model.close()

# ------------------------------------------------------------------ argument errors: a status, nothing launched
buf = nan_rows(600, 3072)
p = ptr(buf)
def cu_of(lens):
    return D(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
f = C.c_float(1e-12)
arg_model, _ = tiny_model(128, 3)                # a real handle: the checks behind the handle's own are reached
for name, rc in [("attention, hidden 200", lib.rr_debug_ce_w_attention(p, 10, ptr(cu_of([5, 5])), 2, 200, 4, p)),
                 ("attention, hidden / heads = 48", lib.rr_debug_ce_w_attention(p, 10, ptr(cu_of([5, 5])), 2, 768, 16, p)),
                 ("attention, an empty sequence", lib.rr_debug_ce_w_attention(p, 10, ptr(cu_of([5, 0, 5])), 3, 768, 12, p)),
                 ("attention, 513 tokens", lib.rr_debug_ce_w_attention(p, 518, ptr(cu_of([5, 513])), 2, 768, 12, p)),
                 ("attention, cu ends before T", lib.rr_debug_ce_w_attention(p, 12, ptr(cu_of([5, 5])), 2, 768, 12, p)),
                 ("attention, NULL cu", lib.rr_debug_ce_w_attention(p, 10, None, 2, 768, 12, p)),
                 ("attention, NULL ctx", lib.rr_debug_ce_w_attention(p, 10, ptr(cu_of([5, 5])), 2, 768, 12, None)),
                 ("add_ln, hidden 200", lib.rr_debug_ce_w_add_ln(p, p, 4, 200, p, p, f)),
                 ("add_ln, T = 0", lib.rr_debug_ce_w_add_ln(p, p, 0, 768, p, p, f)),
                 ("add_ln, NULL g", lib.rr_debug_ce_w_add_ln(p, p, 4, 768, None, p, f)),
                 ("embed_ln, NULL handle", lib.rr_debug_ce_w_embed_ln(None, p, p, p, 4, p)),
                 ("embed_ln, NULL ids", lib.rr_debug_ce_w_embed_ln(arg_model.handle, None, p, p, 4, p)),
                 ("embed_ln, NULL output", lib.rr_debug_ce_w_embed_ln(arg_model.handle, p, p, p, 4, None)),
                 ("embed_ln, T = 0", lib.rr_debug_ce_w_embed_ln(arg_model.handle, p, p, p, 0, p))]:
    print("ARG|%s|%d|%d" % (name, rc, int(bool(torch.isnan(buf).all()))))
arg_model.close()
"""


@pytest.fixture(scope="module")
def kernels_out():
    return _child(KERNELS_CHILD)


def test_wide_attention_against_float64(kernels_out):
    """ce_attention_x3w by itself (Q unscaled: the kernel applies log2 e / sqrt HD) at (hidden, heads) = (128, 2), (768, 12),
    (1024, 16) -- head dim 64, a 128-key chunk -- and (256, 8) -- head dim 32, a 256-key chunk: one sequence of every length
    1..70, the 32-query tile edges 95-97, the chunk edges 127-129, 255-257, 383-385, 511, 512 (odd lengths end in a lone key
    of a V^T pair), and the patterns `normal`, `dominant`, `identical`, `rising`, `large`, `huge_v`, `mixed_v` of
    tests/test_gpu_k5_x3_kernels.py generalised to (heads, HD).
    Error of each output element against sum_k p_k |v_k| of the float64 softmax; per pattern a bar of twice numpy float32's
    worst error (asserted within 4x of it).  No output NaN, the rows behind the last token untouched.
    numpy's figures, which set the bars (float32, worst batch over the four shapes / two bf16 terms, best batch -- printed, not
    asserted: it is 3x .. 13x the float32 error, see the module docstring):
      normal 1.10e-6 / 3.20e-6;  dominant 2.11e-6 / 6.84e-6;  identical 1.57e-7 / 6.92e-7;  rising 1.81e-6 / 4.66e-6;
      large 1.07e-4 / 7.62e-4;  huge_v 1.97e-6 / 1.32e-5;  mixed_v 1.48e-6 / 1.20e-5.
    First MI355X run -- kernel (worst batch):
      normal 8.7e-7;  dominant 3.1e-6;  identical 1.4e-7;  rising 1.1e-6;  large 9.0e-5;  huge_v 1.2e-6;  mixed_v 1.0e-6."""
    rows = _lines(kernels_out, "ATT")
    assert len(rows) == len(ATT_SHAPES) * (2 + 5 + 2 * (len(ATT_PATTERNS) - 1)), kernels_out
    by = {}
    for hidden, heads, name, pattern, n, err, e32, e2t, same_seen, finite, guard in rows:
        print("%4s / %2s  %-22s %-10s %2s sequences  kernel %s  float32 %s  two bf16 terms %s" % (hidden, heads, name, pattern, n, err, e32, e2t))
        assert finite == "1" and guard == "1", (hidden, heads, name, pattern)
        by.setdefault(pattern, []).append((float(err), float(e32), float(e2t)))
    assert sorted(by) == sorted(ATT_PATTERNS)
    assert sorted({(int(r[0]), int(r[1])) for r in rows}) == sorted(ATT_SHAPES)
    for pattern, bar in ATT_BARS.items():
        errs = np.array(by[pattern])
        print("%-10s kernel %.3e  float32 %.3e  two bf16 terms >= %.3e  bar %.1e" % (pattern, errs[:, 0].max(), errs[:, 1].max(), errs[:, 2].min(), bar))
    for pattern, bar in ATT_BARS.items():
        errs = np.array(by[pattern])
        assert errs[:, 0].max() < bar, (pattern, errs[:, 0].max(), bar)
        assert bar <= 4 * errs[:, 1].max(), (pattern, bar, errs[:, 1].max())


def test_wide_attention_same_bits_alone_and_in_any_batch(kernels_out):
    """A sequence's context is the same bits alone, among 70 others and behind longer ones, at every shape and for every
    pattern (the workgroup of a (sequence, head) reads nothing of its neighbours)."""
    rows = _lines(kernels_out, "ATT")
    assert sum(r[2] == "alone" for r in rows) == len(ATT_SHAPES) * (5 + len(ATT_PATTERNS) - 1)
    for hidden, heads, name, pattern, n, err, e32, e2t, same_seen, finite, guard in rows:
        assert same_seen == "1", (hidden, heads, name, pattern)


def test_wide_attention_exact_gather_at_head_dim_64(kernels_out):
    """(128, 2): K rows of norm 400, q_i = k_pi(i) for a permutation pi per head -- every query has one key thousands of log2
    units above the rest, every other probability is exactly 0 and the context is V's row pi(i); V with random 24-bit
    mantissas, random signs, magnitudes log-uniform in 1e-20 .. 1e30.  Lengths 1, 2, 33, 129, 257, 512: the key falls into
    every slot of the permuted V^T tile, into both 32-row blocks of O^T, into the lone last key of a pair and into the
    second, third and fourth 128-key chunk.  |ctx - V| <= 2^-22 |V| per element: the bound derived in
    tests/test_gpu_k5_x3_kernels.py (test_x3_attention_exact_gather) does not depend on the head dim.  The same gather of a V
    cut to two bf16 terms is off by >= 10x that bar (asserted), so the bar cannot pass a lost third term.
    First MI355X run: every element bit-identical at every length; V cut to two bf16 terms 7.2e-6 .. 7.6e-6 (bar 2.4e-7)."""
    rows = _lines(kernels_out, "GATHER")
    assert [r[0] for r in rows] == ["1", "2", "33", "129", "257", "512"], kernels_out
    for S, rel, same, total, gap, hit, finite, guard, two in rows:
        print("S %3s: max |ctx - V| / |V| %s (two bf16 terms %s), %s of %s elements bit-identical, the key leads by >= %s log2 units" %
              (S, rel, two, same, total, gap))
        assert float(two) >= 10 * GATHER_BAR, (S, two)
        assert hit == "1" and float(gap) >= 1000.0, (S, gap)          # (the data: the argmax of every query is pi)
        assert finite == "1" and guard == "1", S
        assert float(rel) <= GATHER_BAR, (S, rel)


def test_wide_kernels_return_the_bits_of_the_384_kernels(kernels_out):
    """On (384, 12) inputs rr_debug_ce_w_attention == rr_debug_ce_x3_attention (lengths 1..70, the edges, scores ~100, twelve
    decades of V), rr_debug_ce_w_add_ln == rr_debug_ce_x3_add_ln (T = 1, 5, 1000; rows of 1, 1e6, 1e-6) and
    rr_debug_ce_w_embed_ln == the h32 of rr_debug_ce_embed_ln on a bf16 handle (the same): bit for bit."""
    rows = _lines(kernels_out, "SAME")
    assert len(rows) == 4 + 5 + 9, kernels_out
    for name, same, finite in rows:
        assert same == "1" and finite == "1", name


def test_wide_layernorm_kernels_against_float64(kernels_out):
    """ce_add_ln_w and ce_embed_ln_w by themselves at widths 128, 768 and 1024 (2, 12 and 16 values per lane), four tokens per
    workgroup: T = 1, 3, 4, 5, 1000 of N(0,1) rows; constant rows (the result is b exactly); rows of 1e6 N(0,1); rows of
    1e-6 N(0,1) with eps = 1e-12 (eps is as large as the variance: its place under the square root matters).  Against the
    float64 LayerNorm of the same fp32 sums; finite, the rows behind T untouched; one bar within 4x numpy float32's error.
    numpy float32 on the add-LayerNorm data, which set the bar: 6.6e-8 .. 2.21e-7.
    First MI355X run -- kernel / float32, worst case: add-LayerNorm 2.2e-7 / 2.2e-7, embedding LayerNorm 2.0e-7 / 2.4e-7;
    constant rows give b exactly at every width."""
    for tag in ("LN", "ELN"):
        rows = _lines(kernels_out, tag)
        assert len(rows) == 3 * 9, kernels_out
        errs = []
        for name, H, T, err, e32, exact_b, finite, guard in rows:
            print("%-3s %-32s H %4s T %5s  kernel %s  float32 %s" % (tag, name, H, T, err, e32))
            assert finite == "1" and guard == "1" and exact_b == "1", (tag, name, H, T)
            errs.append((float(err), float(e32)))
        errs = np.array(errs)
        assert sorted({r[1] for r in rows}) == ["1024", "128", "768"]
        assert errs[:, 0].max() < LN_BAR, (tag, errs[:, 0].max())
        assert LN_BAR <= 4 * errs[:, 1].max(), (tag, errs[:, 1].max())


def test_wide_harness_entries_refuse_bad_arguments(kernels_out):
    """hidden 200, hidden / heads = 48, an empty sequence, 513 tokens, a cu_seqlens that ends before T, NULL pointers (on a real
    handle where the entry takes one), no rows:
    RR_E_INVALID (-1) from each entry, and nothing was launched (the buffer handed in stays NaN)."""
    rows = _lines(kernels_out, "ARG")
    assert len(rows) == 14, kernels_out
    for name, rc, untouched in rows:
        assert rc == "-1" and untouched == "1", (name, rc)
