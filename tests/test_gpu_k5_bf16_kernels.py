"""K5's bf16 fast path (csrc/rr_ce.hip: ce_embed_ln, ce_proj_ts, ce_attention, ce_ffn_fused) one launch at a time against
float64 -- what tests/test_gpu_k5_h2_kernels.py and tests/test_gpu_k5_x3_kernels.py do for the fp32 mode's two paths.

The launches run in one child process on the harness library (librr_hip_dbg.so: rr_debug_ce_embed_ln, rr_debug_ce_bf16_proj,
rr_debug_ce_bf16_attention, rr_debug_ce_bf16_ffn -- thin wrappers around the launch helpers ce_forward_bf16 itself calls) with
the weights of bf16 handles made by CrossEncoder from synth.bert_state_dict(11, n_layers=2, n_labels=1): the test knows every
weight, and the two layers differ.  Inputs are bf16 bit patterns made in numpy, so kernel and reference read the same
values; every output buffer ends in guard rows of a sentinel (0x7FC1 in bf16 buffers, NaN in fp32 ones).

The reference is numpy float64 on the natural, unpermuted weights rounded to bf16 (tests/test_k5_bf16_emulation_cpu.py, whose
functions the child imports).  Beside it sit that file's emulation -- float64 with bf16 rounding at the sites the kernel's
comments name -- and a named defect.  An accuracy case prints the kernel's, the emulation's and the defect's error against
float64 on the same data; its bar (the constants below) is within 4x the emulation's error -- both round at the same sites
and differ by fp32 accumulation order and an occasional flipped rounding -- and at least 10x below the defect's.  Checks that
follow from the arithmetic (same bits wherever a row sits, a lone key returns its V row, hb = bf16(h32), [CLS] row = row 0,
guards) are exact.
"""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = str(pathlib.Path(__file__).resolve().parent.parent)

# ce_proj_ts: max |out - float64| / (sum |x w| + |b|) over T in PROJ_T and both layers.
# First MI355X run -- kernel / emulation / one chunk from its neighbour's weights: 1.25e-3 / 1.25e-3 / >= 0.25
PROJ_BAR = 2.5e-3
# ce_attention: max |ctx - float64| / sum_k p_k |v_k| per pattern, over the sixteen lengths of ATT_LENS.  First MI355X run --
# kernel / emulation (worst length each): normal 4.34e-3 / 4.34e-3, dominant 1.17e-5 / 1.17e-5, identical 3.86e-3 / 3.86e-3,
# rising 4.75e-3 / 4.75e-3, large 6.44e-3 / 6.44e-3; the defect (first padding key of the 17-token `identical` sequence
# unmasked): 0.323 against 2.65e-3 / 2.65e-3 on that sequence
ATT_BARS = {"normal": 8e-3, "dominant": 4e-5, "identical": 8e-3, "rising": 8e-3, "large": 1.2e-2}
# ce_ffn_fused: per row max |out - float64| / max_c (|g_c xhat_c| + |b_c|), over M in FFN_M and both layers.  First MI355X run --
# kernel / emulation / quads 1 and 2 of one 16-column group of W2 unswapped (M >= 31): normal 2.94e-3 / 2.94e-3 / >= 0.144,
# tails 2.82e-3 / 2.82e-3 / >= 0.080
FFN_BARS = {"normal": 4e-3, "tails": 4e-3}
# ce_embed_ln: the same LayerNorm metric; the yardstick is numpy float32 on the same rows.  First MI355X run -- kernel /
# float32: 2.1e-7 / 1.7e-7
EMBED_BAR = 5e-7

PROJ_T = [1, 31, 32, 33, 255, 256, 257, 300]
ATT_LENS = [1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512]
ATT_PATTERNS = ["normal", "dominant", "identical", "rising", "large"]
FFN_M = [1, 31, 32, 33, 127, 128, 129, 300]
EMBED_T = [1, 3, 4, 5, 130]


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
sys.path.insert(0, os.path.join(@ROOT@, "tests"))
import ctypes as C
import numpy as np, torch
import test_k5_bf16_emulation_cpu as E
from review_recommender_amd import _lib, synth
from review_recommender_amd.cross_encoder import CrossEncoder
lib = _lib.load()
dev = torch.device("cuda", 0)
F32, F64 = np.float32, np.float64
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
DB = lambda bits: D(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16))      # bf16 bits -> an int16 device tensor
GUARD, SENT = 3, 0x7FC1                          # rows behind every output that no kernel may touch; the bf16 sentinel
def bbuf(rows, cols):
    return torch.full((rows + GUARD, cols), SENT, dtype=torch.int16, device=dev)
def fbuf(rows, cols):
    return torch.full((rows + GUARD, cols), float("nan"), dtype=torch.float32, device=dev)
def b_clean(t, rows=0):
    return int(bool((t[rows:] == SENT).all()))
def f_clean(t, rows=0):
    return int(bool(torch.isnan(t[rows:]).all()))
def bits_of(t, rows):
    return t[:rows].cpu().numpy().view(np.uint16)
def same_rows(a, rows):
    # the rows of `a` listed in `rows` (those it has) are the same bytes
    rows = [r for r in rows if r < len(a)]
    return int(all(np.array_equal(a[rows[0]], a[r]) for r in rows))

SD = synth.bert_state_dict(11, n_layers=2, n_labels=1)
SD_TAILS = E.with_tails(SD)
ce = CrossEncoder(SD, precision="bf16")
ce_tails = CrossEncoder(SD_TAILS, precision="bf16")
ce_f32 = CrossEncoder(SD)                        # (the refusals: not a bf16 handle)
H, H_TAILS, H_F32 = ce.model.handle, ce_tails.model.handle, ce_f32.model.handle

# ------------------------------------------------------------------ ce_proj_ts
PROJ_SAME = [0, 31, 32, 255, 256, 299]
X300 = E.rand_bf16(np.random.default_rng(21), (300, 384))
X300[PROJ_SAME] = X300[0]
for layer in (0, 1):
    W = E.layer_weights(SD, layer)
    x = E.bits_f64(X300)
    ref, mag = E.proj_ref(x, W["wqkv"], W["bqkv"])
    delta, r32 = E.proj_delta(x, W["wqkv"], W["bqkv"], ref, mag)
    emu, bad = E.proj_emulation(x, W["wqkv"], W["bqkv"]), E.proj_defect(x, W["wqkv"], W["bqkv"])
    for T in (1, 31, 32, 33, 255, 256, 257, 300):
        out = bbuf(T, 1152)
        dx = DB(X300[:T])
        _lib.check(lib.rr_debug_ce_bf16_proj(H, layer, ptr(dx), T, ptr(out)), "rr_debug_ce_bf16_proj")
        bits = bits_of(out, T)
        got = E.bits_f64(bits)
        e = lambda a: float((np.abs(a[:T] - ref[:T]) / mag[:T]).max())
        outside = int((~E.proj_in_interval(got, ref[:T], delta[:T])).sum())
        print("PROJ|%d|%d|%.3e|%.3e|%.3e|%d|%d|%d|%d|%.3e" % (layer, T, e(got), e(emu), e(bad), outside, same_rows(bits, PROJ_SAME),
              b_clean(out, T), int(np.isfinite(got).all()), float((delta / mag).max())))

# ------------------------------------------------------------------ ce_attention
def run_att(bits, cu, max_len, cls):
    T, n = len(bits), len(cu) - 1
    ctx = bbuf(T, 384)
    ctx_cls = bbuf(n, 384) if cls else None
    dx, dcu = DB(bits), D(np.asarray(cu, dtype=np.int32))
    _lib.check(lib.rr_debug_ce_bf16_attention(ptr(dx), T, ptr(dcu), n, int(max_len), ptr(ctx), ptr(ctx_cls)), "rr_debug_ce_bf16_attention")
    if cls:
        return bits_of(ctx_cls, n), b_clean(ctx_cls, n) & b_clean(ctx)      # (the [CLS] form leaves ALL of ctx alone)
    return bits_of(ctx, T), b_clean(ctx, T)

LENS = [1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512]
for pi, pattern in enumerate(E.ATT_PATTERNS):
    order = [LENS[i] for i in np.random.default_rng((22, pi)).permutation(len(LENS))]
    seqs = {S: E.att_sequence(pattern, S) for S in LENS}
    cu = np.concatenate([[0], np.cumsum(order)])
    packed, guard = run_att(np.concatenate([seqs[S] for S in order]), cu, 512, False)
    rows = {S: packed[cu[i]:cu[i + 1]] for i, S in enumerate(order)}
    cls, cls_guard = run_att(np.concatenate([seqs[S] for S in order]), cu, 512, True)
    cls_same = int(all(np.array_equal(cls[i], rows[S][0]) for i, S in enumerate(order)))
    # the sequences of at most 257 tokens packed again, in another order, with max_len = 257
    short = [S for S in order[::-1] if S <= 257]
    cus = np.concatenate([[0], np.cumsum(short)])
    p2, g2 = run_att(np.concatenate([seqs[S] for S in short]), cus, 257, False)
    same_short = int(all(np.array_equal(p2[cus[i]:cus[i + 1]], rows[S]) for i, S in enumerate(short)))
    guard &= g2
    same_tight = same_512 = 1
    err = emu = 0.0
    for S in LENS:
        for max_len in (S, 512):
            alone, g = run_att(seqs[S], [0, S], max_len, False)
            guard &= g
            if max_len == S: same_tight &= int(np.array_equal(alone, rows[S]))
            else: same_512 &= int(np.array_equal(alone, rows[S]))
        ref, mag = E.att_ref(seqs[S])
        k_err, e_err = E.att_err(E.bits_f64(rows[S]), ref, mag), E.att_err(E.att_emulation(seqs[S]), ref, mag)
        err, emu = max(err, k_err), max(emu, e_err)
        print("ATTLEN|%s|%d|%.3e|%.3e" % (pattern, S, k_err, e_err))
        if (pattern, S) == E.ATT_DEFECT_CASE:
            print("ATTDEF|%s|%d|%.3e|%.3e|%.3e" % (pattern, S, k_err, e_err, E.att_err(E.att_emulation(seqs[S], unmasked_pad=True), ref, mag)))
        if S == 17:
            print("ATTDEF17|%s|%.3e" % (pattern, E.att_err(E.att_emulation(seqs[S], unmasked_pad=True), ref, mag)))
    lone = int(np.array_equal(rows[1], seqs[1][:, 768:]))                        # S = 1: the context IS the V row
    finite = int(np.isfinite(E.bits_f64(packed)).all())
    print("ATT|%s|%.3e|%.3e|%d|%d|%d|%d|%d|%d|%d|%d" % (pattern, err, emu, same_tight, same_512, same_short, lone, cls_same, cls_guard, guard, finite))

# ------------------------------------------------------------------ ce_ffn_fused
FFN_SAME = [0, 31, 32, 127, 128, 299]
rng = np.random.default_rng(23)
CTX300 = E.rand_bf16(rng, (300, 384))
H300 = rng.standard_normal((300, 384)).astype(F32)
CTX300[FFN_SAME] = CTX300[0]
H300[FFN_SAME] = H300[0]
for data, handle, sd in (("normal", H, SD), ("tails", H_TAILS, SD_TAILS)):
    for layer in (0, 1):
        W = E.layer_weights(sd, layer)
        ctx, h = E.bits_f64(CTX300), H300.astype(F64)
        ref, den = E.ffn_ref(ctx, h, W)
        emu, bad, emu_erf = E.ffn_emulation(ctx, h, W), E.ffn_defect(ctx, h, W), E.ffn_emulation(ctx, h, W, phi=E.phi_erf)
        for M in (1, 31, 32, 33, 127, 128, 129, 300):
            dctx = DB(CTX300[:M])
            dh, hb = fbuf(M, 384), bbuf(M, 384)
            dh[:M] = D(H300[:M])
            _lib.check(lib.rr_debug_ce_bf16_ffn(handle, layer, ptr(dctx), ptr(dh), ptr(hb), M), "rr_debug_ce_bf16_ffn")
            out32, hbits = dh[:M].cpu().numpy(), bits_of(hb, M)
            e = lambda a: E.ffn_err(a[:M], ref[:M], den[:M])
            hb_exact = int(np.array_equal(hbits, E.bf16_bits(out32)))
            same = same_rows(out32.view(np.uint32), FFN_SAME) & same_rows(hbits, FFN_SAME)
            print("FFN|%s|%d|%d|%.3e|%.3e|%.3e|%.3e|%.3e|%d|%d|%d|%d" % (data, layer, M, e(out32.astype(F64)), e(emu), e(bad), e(emu_erf),
                  float((np.abs(emu[:M] - emu_erf[:M]) / den[:M]).max()), hb_exact, same, f_clean(dh, M) & b_clean(hb, M), int(np.isfinite(out32).all())))

# ------------------------------------------------------------------ ce_embed_ln
VOCAB, MAX_POS = ce.model.vocab, ce.model.max_pos
rng = np.random.default_rng(24)
TOK = rng.integers(0, VOCAB, 130).astype(np.int32)
POS = rng.integers(0, MAX_POS, 130).astype(np.int32)
TYP = rng.integers(0, 2, 130).astype(np.int32)
TOK[:3], POS[:3], TYP[:3] = [VOCAB - 1, 0, 7], [MAX_POS - 1, 0, 1], [1, 0, 1]
for T in (1, 3, 4, 5, 130):
    h32, hb = fbuf(T, 384), bbuf(T, 384)
    dt, dy, dp = D(TOK[:T]), D(TYP[:T]), D(POS[:T])
    _lib.check(lib.rr_debug_ce_embed_ln(H, ptr(dt), ptr(dy), ptr(dp), T, ptr(h32), ptr(hb)), "rr_debug_ce_embed_ln")
    out32, hbits = h32[:T].cpu().numpy(), bits_of(hb, T)
    ref, den = E.embed_ln(SD, TOK[:T], TYP[:T], POS[:T], F64)
    f32 = E.embed_ln(SD, TOK[:T], TYP[:T], POS[:T], F32)[0].astype(F64)
    e = lambda a: float((np.abs(a - ref) / den).max())
    print("EMB|%d|%.3e|%.3e|%d|%d|%d" % (T, e(out32.astype(F64)), e(f32), int(np.array_equal(hbits, E.bf16_bits(out32))),
          f_clean(h32, T) & b_clean(hb, T), int(np.isfinite(out32).all())))

# ------------------------------------------------------------------ argument errors: a status, nothing launched
bb, ff = bbuf(600, 1152), fbuf(600, 384)
ii = torch.zeros(4096, dtype=torch.int32, device=dev)
b, f, i = ptr(bb), ptr(ff), ptr(ii)
keep = []                                        # (the cu tensors stay alive until their call has returned)
def cu_of(lens, first=0):
    keep.append(D((first + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)))
    return ptr(keep[-1])
proj, att, ffn, emb = lib.rr_debug_ce_bf16_proj, lib.rr_debug_ce_bf16_attention, lib.rr_debug_ce_bf16_ffn, lib.rr_debug_ce_embed_ln
CASES = [
    ("rr_debug_ce_bf16_proj", "NULL handle", lambda: proj(None, 0, b, 4, b)),
    ("rr_debug_ce_bf16_proj", "NULL hb", lambda: proj(H, 0, None, 4, b)),
    ("rr_debug_ce_bf16_proj", "NULL qkv", lambda: proj(H, 0, b, 4, None)),
    ("rr_debug_ce_bf16_proj", "layer -1", lambda: proj(H, -1, b, 4, b)),
    ("rr_debug_ce_bf16_proj", "layer 2 of 2", lambda: proj(H, 2, b, 4, b)),
    ("rr_debug_ce_bf16_proj", "an fp32 handle", lambda: proj(H_F32, 0, b, 4, b)),
    ("rr_debug_ce_bf16_proj", "T = 0", lambda: proj(H, 0, b, 0, b)),
    ("rr_debug_ce_bf16_proj", "T = -3", lambda: proj(H, 0, b, -3, b)),
    ("rr_debug_ce_bf16_attention", "NULL qkv", lambda: att(None, 10, cu_of([5, 5]), 2, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "NULL cu", lambda: att(b, 10, None, 2, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "NULL ctx", lambda: att(b, 10, cu_of([5, 5]), 2, 16, None, b)),
    ("rr_debug_ce_bf16_attention", "T = 0", lambda: att(b, 0, cu_of([0]), 1, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "no sequences", lambda: att(b, 10, cu_of([10]), 0, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "cu ends before T", lambda: att(b, 12, cu_of([5, 5]), 2, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "cu starts at 1", lambda: att(b, 11, cu_of([5, 5], 1), 2, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "an empty sequence", lambda: att(b, 10, cu_of([5, 0, 5]), 3, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "an empty sequence, [CLS] form", lambda: att(b, 10, cu_of([5, 0, 5]), 3, 16, b, b)),
    ("rr_debug_ce_bf16_attention", "a sequence longer than max_len", lambda: att(b, 25, cu_of([5, 20]), 2, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "a negative length", lambda: att(b, 10, cu_of([12, -2]), 2, 16, b, None)),
    ("rr_debug_ce_bf16_attention", "max_len = 513", lambda: att(b, 10, cu_of([5, 5]), 2, 513, b, None)),
    ("rr_debug_ce_bf16_attention", "max_len = 0", lambda: att(b, 10, cu_of([5, 5]), 2, 0, b, None)),
    ("rr_debug_ce_bf16_ffn", "NULL handle", lambda: ffn(None, 0, b, f, b, 4)),
    ("rr_debug_ce_bf16_ffn", "NULL ctx", lambda: ffn(H, 0, None, f, b, 4)),
    ("rr_debug_ce_bf16_ffn", "NULL h32", lambda: ffn(H, 0, b, None, b, 4)),
    ("rr_debug_ce_bf16_ffn", "NULL hb", lambda: ffn(H, 0, b, f, None, 4)),
    ("rr_debug_ce_bf16_ffn", "layer -1", lambda: ffn(H, -1, b, f, b, 4)),
    ("rr_debug_ce_bf16_ffn", "layer 2 of 2", lambda: ffn(H, 2, b, f, b, 4)),
    ("rr_debug_ce_bf16_ffn", "an fp32 handle", lambda: ffn(H_F32, 0, b, f, b, 4)),
    ("rr_debug_ce_bf16_ffn", "M = 0", lambda: ffn(H, 0, b, f, b, 0)),
    ("rr_debug_ce_embed_ln", "NULL handle", lambda: emb(None, i, i, i, 4, f, b)),
    ("rr_debug_ce_embed_ln", "NULL token ids", lambda: emb(H, None, i, i, 4, f, b)),
    ("rr_debug_ce_embed_ln", "NULL type ids", lambda: emb(H, i, None, i, 4, f, b)),
    ("rr_debug_ce_embed_ln", "NULL positions", lambda: emb(H, i, i, None, 4, f, b)),
    ("rr_debug_ce_embed_ln", "NULL h32", lambda: emb(H, i, i, i, 4, None, b)),
    ("rr_debug_ce_embed_ln", "NULL hb", lambda: emb(H, i, i, i, 4, f, None)),
    ("rr_debug_ce_embed_ln", "an fp32 handle", lambda: emb(H_F32, i, i, i, 4, f, b)),
    ("rr_debug_ce_embed_ln", "T = 0", lambda: emb(H, i, i, i, 0, f, b)),
]
for entry, what, call in CASES:
    rc = call()
    msg = lib.rr_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    print("ARG|%s|%s|%d|%d|%d" % (entry, what, rc, int(msg.startswith(entry + ":")), b_clean(bb) & f_clean(ff)))
"""


@pytest.fixture(scope="module")
def kernels_out():
    return _child(KERNELS_CHILD)


def test_bf16_proj_against_float64(kernels_out):
    """ce_proj_ts by itself on T = 1, 31, 32, 33 (a wave's 32 tokens), 255, 256, 257 (a workgroup's 256), 300, with the QKV
    weights of layer 0 and of layer 1; x ~ N(0, 1) as bf16.  (a) Error against sum |x w| + |b| of the float64 product: the
    bar within 4x the emulation's (float64, the output rounded to bf16) and 10x below that of one 32-feature chunk computed
    from its neighbour's weight rows.  (b) Every element inside [rne_bf16(ref - d), rne_bf16(ref + d)] with d = 4 x numpy
    float32's own worst |r32 - r64| / (sum |x w| + |b|) on this data x (sum |x w| + |b|): the output is bf16 of an fp32 sum.
    No bf16 ulps are counted: fp32 accumulation alone moves elements by up to two where the sum cancels.  (c) Rows >= T
    stay untouched.
    First MI355X run -- kernel / emulation / wrong chunk: layer 0 1.206e-3 / 1.206e-3 / 0.418 at T >= 255 (6.75e-4 / 6.75e-4 / 0.257 on
    the single row of T = 1), layer 1 1.251e-3 / 1.251e-3 / 0.414 (6.78e-4 / 6.78e-4 / 0.251); the kernel's figure equals the
    emulation's to every printed digit at all sixteen cases; no element outside its interval, d <= 6.8e-7 (layer 1: 5.8e-7)
    of sum |x w| + |b|."""
    rows = _lines(kernels_out, "PROJ")
    assert [(r[0], r[1]) for r in rows] == [(str(l), str(T)) for l in (0, 1) for T in PROJ_T], kernels_out
    errs = []
    for layer, T, err, emu, bad, outside, same, guard, finite, dmax in rows:
        print("layer %s T %3s  kernel %s  emulation %s  wrong chunk %s  outside the interval %s  (d <= %s of sum |x w| + |b|)"
              % (layer, T, err, emu, bad, outside, dmax))
        assert finite == "1" and guard == "1", (layer, T)
        assert outside == "0", (layer, T, outside)
        errs.append((float(err), float(emu), float(bad)))
    errs = np.array(errs)
    assert errs[:, 0].max() < PROJ_BAR, (errs[:, 0].max(), PROJ_BAR)
    assert PROJ_BAR <= 4 * errs[:, 1].max(), (PROJ_BAR, errs[:, 1].max())
    assert 10 * PROJ_BAR <= errs[:, 2].min(), (PROJ_BAR, errs[:, 2].min())


def test_bf16_proj_same_row_same_bits_anywhere(kernels_out):
    """One input row placed at rows 0, 31, 32, 255, 256 and 299 gives the same 1152 bf16 values bit for bit: the rotated chunk
    order of the second workgroup, every wave and both lane halves change no bit."""
    rows = _lines(kernels_out, "PROJ")
    assert len(rows) == 16
    for layer, T, err, emu, bad, outside, same, guard, finite, dmax in rows:
        assert same == "1", (layer, T)


def test_bf16_attention_against_float64(kernels_out):
    """ce_attention by itself on sequences of 1, 2, 15-17 (a 16-row query block), 31-33 (the 32-key padding), 127-129 (a 128-key
    chunk; eight waves x 16 rows), 255-257, 511, 512 tokens, five score / value patterns for 12 heads each: N(0, 1); one
    key per head 36.7 log2 units above the rest; every key the same; scores rising 0.05 log2 units per key, so the running
    maximum moves in every chunk and the last one rescales the accumulators; scaled scores up to about +-80.  Error of each
    output element against sum_k p_k |v_k| of the float64 softmax.  The emulation: exact scores, numerator from bf16(p),
    denominator from p, output rounded to bf16 (ceiling 2^-7, tests/test_k5_bf16_emulation_cpu.py).  The defect: the first
    padding key of the 17-token `identical` sequence left unmasked.  Every pattern's bar is within 4x its emulation's
    worst error and 10x below the defect's.
    First MI355X run -- kernel / emulation, worst of the sixteen lengths: normal 4.344e-3 / 4.344e-3 (2 tokens; 1.6e-3 at 512),
    dominant 1.169e-5 / 1.169e-5, identical 3.861e-3 / 3.861e-3, rising 4.747e-3 / 4.747e-3, large 6.436e-3 / 6.436e-3; the
    two agree to every printed digit at 75 of the 80 (pattern, length) cases and differ by at most 10 % at the others (256,
    129, 257, 511 tokens: a flipped rounding).  Defect case: 2.651e-3 / 2.651e-3 / 0.3228; the same unmasked key on the
    other patterns' 17-token sequences: normal 4.98e-2, rising 3.79e-2, dominant and large invisible (a zero score weighs
    nothing beside a key tens of log2 units above it).  With key 17 of a 17-token sequence unmasked in the kernel by hand
    the defect case read 0.3228 (normal 4.98e-2, rising 3.79e-2) and this test failed."""
    rows = _lines(kernels_out, "ATT")
    assert [r[0] for r in rows] == ATT_PATTERNS, kernels_out
    per_len = _lines(kernels_out, "ATTLEN")
    assert [(r[0], r[1]) for r in per_len] == [(p, str(S)) for p in ATT_PATTERNS for S in ATT_LENS]
    for pattern, S, err, emu in per_len:
        print("%-10s %3s tokens  kernel %s  emulation %s" % (pattern, S, err, emu))
    for pattern, err17 in _lines(kernels_out, "ATTDEF17"):
        print("%-10s 17 tokens, first padding key unmasked: %s" % (pattern, err17))
    (dp, dS, d_err, d_emu, d_bad), = _lines(kernels_out, "ATTDEF")
    assert (dp, dS) == ("identical", "17")
    print("defect case (%s, %s tokens): kernel %s  emulation %s  unmasked padding key %s" % (dp, dS, d_err, d_emu, d_bad))
    assert float(d_err) <= 4 * float(d_emu) and 10 * 4 * float(d_emu) <= float(d_bad)
    for pattern, err, emu, same_tight, same_512, same_short, lone, cls_same, cls_guard, guard, finite in rows:
        print("%-10s worst of 16 lengths: kernel %s  emulation %s" % (pattern, err, emu))
        assert finite == "1" and guard == "1", pattern
        bar = ATT_BARS[pattern]
        assert float(err) < bar, (pattern, err, bar)
        assert bar <= 4 * float(emu), (pattern, bar, emu)
        assert 10 * bar <= float(d_bad), (pattern, bar, d_bad)


def test_bf16_attention_same_bits_packed_alone_and_at_any_max_len(kernels_out):
    """Each sequence's context rows are the same bits (a) packed with the fifteen others in shuffled order, max_len = 512,
    (b) alone with max_len = its own length, (c) alone with max_len = 512, (d) packed among the sequences of at most 257
    tokens in another order with max_len = 257: the LDS layout follows max_len, the result does not."""
    rows = _lines(kernels_out, "ATT")
    assert len(rows) == 5
    for pattern, err, emu, same_tight, same_512, same_short, lone, cls_same, cls_guard, guard, finite in rows:
        assert (same_tight, same_512, same_short) == ("1", "1", "1"), (pattern, same_tight, same_512, same_short)


def test_bf16_attention_lone_key_returns_its_v_row(kernels_out):
    """S = 1: the 31 padding keys are masked, p = 1 survives bf16, the sum is 1 and v x 1 rounds back to v -- the context is
    the V row bit for bit, in every pattern."""
    rows = _lines(kernels_out, "ATT")
    assert len(rows) == 5
    for row in rows:
        assert row[6] == "1", row[0]


def test_bf16_attention_cls_only_form_is_row_0_of_the_full_one(kernels_out):
    """With ctx_cls given, ctx_cls[sequence] is bitwise row 0 of that sequence in the full run, for all sixteen lengths and
    five patterns, and neither ctx (sentinels throughout) nor the guard rows of ctx_cls are written."""
    rows = _lines(kernels_out, "ATT")
    assert len(rows) == 5
    for row in rows:
        assert row[7] == "1" and row[8] == "1", row[0]


def test_bf16_ffn_against_float64(kernels_out):
    """ce_ffn_fused by itself (output projection, LayerNorm, FFN, LayerNorm) on M = 1, 31, 32, 33 (a wave's 32 tokens), 127, 128,
    129 (a workgroup's 128), 300, on both layers: ctx ~ N(0, 1) as bf16, residual ~ N(0, 1) fp32.  `tails`: handles whose b1
    holds -40, -8, -5, -4.6, 4.6, 5, 8, 40 at eight features, so pre-activations cross the Phi table's +-4.5 clamp.  The
    float64 reference multiplies by the NATURAL W2 and uses the exact erf GELU; the kernel reads W2 with permuted columns
    and Phi from its table.  Per row max |out - float64| / max_c (|g_c xhat_c| + |b_c|); the bar within 4x the emulation's
    error (bf16 at the first LayerNorm's output as operand and at the GELU's output, table Phi) and 10x below that of quads 1
    and 2 of one 16-column group of W2 left unswapped.  Also printed for `tails`: the emulation with the exact erf, and the
    two emulations' distance -- what the table's clamp costs (below -4.5 the fast path returns x 3.4e-6, not 0).
    First MI355X run -- kernel / emulation / unswapped group, at M = 300: normal 2.942e-3 / 2.942e-3 / 0.2055 (layer 1: 2.908e-3 /
    2.908e-3 / 0.1605), tails 2.818e-3 / 2.818e-3 / 0.1356 (layer 1: 2.472e-3 / 2.471e-3 / 0.1067); over the cases of M >= 31 the
    unswapped group reads >= 0.144 (normal) and >= 0.080 (tails).  The emulation with the exact erf: 2.91e-3 / 2.80e-3, and
    6.2e-4 from the table emulation at most -- the table and its clamp cost a fifth of the bf16 roundings.  With the
    permutation of W2's group 37 dropped at load by hand the kernel read 0.2055 / 0.1605 / 0.1356 / 0.1067 and this test failed."""
    rows = _lines(kernels_out, "FFN")
    assert [(r[0], r[1], r[2]) for r in rows] == [(d, str(l), str(M)) for d in ("normal", "tails") for l in (0, 1) for M in FFN_M], kernels_out
    by = {}
    for data, layer, M, err, emu, bad, emu_erf, tab_erf, hb_exact, same, guard, finite in rows:
        print("%-6s layer %s M %3s  kernel %s  emulation %s  unswapped group %s  (emulation with erf %s, table against erf %s)"
              % (data, layer, M, err, emu, bad, emu_erf, tab_erf))
        assert finite == "1", (data, layer, M)
        by.setdefault(data, []).append((float(err), float(emu), float(bad), int(M)))
    assert sorted(by) == sorted(FFN_BARS)
    for data, bar in FFN_BARS.items():
        errs = np.array(by[data])
        assert errs[:, 0].max() < bar, (data, errs[:, 0].max(), bar)
        assert bar <= 4 * errs[:, 1].max(), (data, bar, errs[:, 1].max())
        # (the defect sits in ONE group of 16 of the 1536 features and a row shows it as far as its own activations there go:
        #  1e-2 .. 6e-2 on the single row of M = 1.  Its measure is every case of at least 31 rows.)
        assert 10 * bar <= errs[errs[:, 3] > 1, 2].min(), (data, bar, errs[errs[:, 3] > 1, 2].min())


def test_bf16_ffn_exact_checks(kernels_out):
    """On the kernel's own outputs: hb = rne_bf16(h32) bit for bit; identical (ctx, h32) rows at rows 0, 31, 32, 127, 128 and 299
    give bitwise identical output rows (every wave, both lane halves, the last workgroup's clamped lanes); the rows behind
    M, of h32 and of hb, keep their sentinels."""
    rows = _lines(kernels_out, "FFN")
    assert len(rows) == 32
    for data, layer, M, err, emu, bad, emu_erf, tab_erf, hb_exact, same, guard, finite in rows:
        assert hb_exact == "1" and same == "1" and guard == "1", (data, layer, M, hb_exact, same, guard)


def test_embed_ln_against_float64(kernels_out):
    """ce_embed_ln by itself (four tokens per workgroup: T = 1, 3, 4, 5, 130) with token ids 0 and vocab - 1, position
    max_pos - 1 and type 1 among the inputs: within 4x numpy float32's error against the float64 LayerNorm of the same
    embedding rows; hb = rne_bf16(h32) bit for bit; the rows behind T untouched.
    First MI355X run -- kernel / float32: 1.15e-7 / 1.16e-7 (T = 1), 1.51e-7 / 1.19e-7 (T = 5), 2.12e-7 / 1.73e-7 (T = 130)."""
    rows = _lines(kernels_out, "EMB")
    assert [r[0] for r in rows] == [str(T) for T in EMBED_T], kernels_out
    errs = []
    for T, err, e32, hb_exact, guard, finite in rows:
        print("T %3s  kernel %s  float32 %s" % (T, err, e32))
        assert finite == "1" and guard == "1" and hb_exact == "1", T
        errs.append((float(err), float(e32)))
    errs = np.array(errs)
    assert errs[:, 0].max() < EMBED_BAR, (errs[:, 0].max(), EMBED_BAR)
    assert EMBED_BAR <= 4 * errs[:, 1].max(), (EMBED_BAR, errs[:, 1].max())


def test_bf16_harness_entries_refuse_bad_arguments(kernels_out):
    """NULL pointers (the handle included), a layer outside [0, 2), a handle of the fp32 precision, no rows, cu_seqlens that do
    not run from 0 to T, a sequence of no tokens (both attention forms), of a negative length or longer than max_len,
    max_len outside [1, 512]: RR_E_INVALID (-1) from each entry, rr_last_error names the entry, and nothing was launched
    (the bf16 and fp32 buffers handed in keep their sentinels)."""
    rows = _lines(kernels_out, "ARG")
    assert len(rows) == 37, kernels_out
    for entry, what, rc, named, clean in rows:
        assert rc == "-1" and named == "1" and clean == "1", (entry, what, rc, named, clean)
