"""The arithmetic of K5's bf16 fast path (csrc/rr_ce.hip: ce_embed_ln, ce_proj_ts, ce_attention, ce_ffn_fused) restated in numpy,
without a GPU: for every kernel a float64 REFERENCE of the operation (natural, unpermuted weights rounded once to bf16, exact
erf GELU), an EMULATION (float64 with bf16 round-to-nearest-even at exactly the sites the kernel's comments name) and a DEFECT
emulation (the same, with one named mistake).  tests/test_gpu_k5_bf16_kernels.py imports these functions in its child process
and holds each kernel to the rule of tests/test_gpu_k5_h2_kernels.py: within 4x the emulation's error, 10x below the
defect's.  Nothing here was fitted to kernel output; the tests below check, on small shapes, that the rule's two conditions
can hold at once (defect >= 40x emulation), that each emulation stays under a ceiling derived from its rounding sites, that
the numpy Phi table is ce_gelu_table's, and that the projection's interval check accepts numpy float32's own result.

Rounding sites (from the comments of rr_ce.hip):
  ce_proj_ts    out = bf16(fp32 sum of x w + b)                                    -- one site: the output
  ce_attention  scores exact (bf16 x bf16 products, fp32 sums); numerator sum_k bf16(p_k) v_k, denominator sum_k p_k from the
                unrounded p; output bf16(numerator / denominator)                  -- two sites: p, the output
  ce_ffn_fused  y = LayerNorm1(h + Wo ctx + bo) stays fp32 as the residual, bf16(y) is the FFN's operand; Phi from the 513-knot
                table (linear interpolation, clamped outside +-4.5), bf16(x Phi(x)) is the second product's operand; the second
                LayerNorm's output is fp32 (hb = bf16 of it)                        -- two sites: y, the GELU output
  ce_embed_ln   fp32 throughout: its yardstick is numpy float32, not an emulation
"""
import math

import numpy as np
from scipy.special import erf

F32, F64 = np.float32, np.float64
U = 2.0 ** -8                                    # largest relative error of one rounding to bf16 (8 significand bits)
LN_EPS = float(F32(1e-12))                       # what a handle made by CrossEncoder(sd) is given
C1 = float(F32(0.17677669529663687) * F32(1.4426950408889634))      # log2 e / sqrt 32, as ce_attention forms it

PROJ_CEILING = U                                 # |bf16(r) - r| <= 2^-8 |r| <= 2^-8 (sum |x w| + |b|)
ATT_CEILING = 2 * U                              # 2^-8 of sum p |v| for p, 2^-8 of |out| <= sum p |v| for the output


# ------------------------------------------------------------------ bf16
def bf16_bits(a):
    """fp32 -> the bits of the nearest bf16 (ties to even), uint16"""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_f64(b):
    """bf16 bits -> their values, float64"""
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F32).astype(F64)


def rne_bf16(x):
    """float64 -> fp32 -> the nearest bf16, as float64 (both steps monotonic: so is this)"""
    return bits_f64(bf16_bits(np.asarray(x, dtype=F64).astype(F32)))


def rand_bf16(rng, shape, scale=1.0):
    """N(0, scale) rounded to bf16, as bits"""
    return bf16_bits((rng.standard_normal(shape) * scale).astype(F32))


# ------------------------------------------------------------------ weights
def layer_weights(sd, layer):
    """Layer `layer` of a Hugging Face BERT state dict as the bf16 path holds it: Linear weights rounded once to bf16, in
    their NATURAL order (W2 unpermuted); biases and LayerNorm parameters fp32.  All float64."""
    p = "bert.encoder.layer.%d." % layer
    w = lambda k: rne_bf16(sd[p + k])
    f = lambda k: np.asarray(sd[p + k], dtype=F32).astype(F64)
    qkv = ("query", "key", "value")
    return {"wqkv": np.concatenate([w("attention.self.%s.weight" % n) for n in qkv]),
            "bqkv": np.concatenate([f("attention.self.%s.bias" % n) for n in qkv]),
            "wo": w("attention.output.dense.weight"), "bo": f("attention.output.dense.bias"),
            "ln1_g": f("attention.output.LayerNorm.weight"), "ln1_b": f("attention.output.LayerNorm.bias"),
            "w1": w("intermediate.dense.weight"), "b1": f("intermediate.dense.bias"),
            "w2": w("output.dense.weight"), "b2": f("output.dense.bias"),
            "ln2_g": f("output.LayerNorm.weight"), "ln2_b": f("output.LayerNorm.bias")}


TAIL_FEATURES = np.array([3, 200, 401, 777, 778, 1000, 1300, 1535])     # eight FFN features, in several 32-feature chunks
TAIL_B1 = np.array([-40.0, -8.0, -5.0, -4.6, 4.6, 5.0, 8.0, 40.0], F32)   # pre-activations across the table's +-4.5 clamp


def with_tails(sd):
    """The state dict with b1 of eight features of BOTH layers set to TAIL_B1"""
    out = dict(sd)
    for l in (0, 1):
        k = "bert.encoder.layer.%d.intermediate.dense.bias" % l
        b = np.array(sd[k], dtype=F32)
        b[TAIL_FEATURES] = TAIL_B1
        out[k] = b
    return out


# ------------------------------------------------------------------ ce_proj_ts
def proj_ref(x, w, b):
    """x [T][384], w [N][384], b [N] float64 -> (x w^T + b, sum |x w| + |b|)"""
    return x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)


def proj_emulation(x, w, b):
    return rne_bf16(x @ w.T + b)


def proj_defect(x, w, b, chunk=5):
    """one 32-feature chunk computed from the neighbouring chunk's weight rows (its own bias)"""
    wd = w.copy()
    wd[32 * chunk:32 * chunk + 32] = w[32 * chunk + 32:32 * chunk + 64]
    return rne_bf16(x @ wd.T + b)


def proj_delta(x, w, b, ref, mag):
    """-> (delta, r32): numpy float32's own product r32 on the same data, and delta = 4 x (its worst |r32 - ref| / mag) x mag"""
    r32 = (x.astype(F32) @ w.astype(F32).T + b.astype(F32)).astype(F64)
    return 4.0 * float((np.abs(r32 - ref) / mag).max()) * mag, r32


def proj_in_interval(out, ref, delta):
    """The output is bf16(fp32 sum): with the sum inside [ref - delta, ref + delta] it lies in [rne_bf16(ref - delta),
    rne_bf16(ref + delta)] (rounding is monotonic).  No ulp count: where the sum cancels, one fp32 ulp of the sum is many
    bf16 ulps of the output."""
    return (out >= rne_bf16(ref - delta)) & (out <= rne_bf16(ref + delta))


# ------------------------------------------------------------------ ce_attention
ATT_PATTERNS = ["normal", "dominant", "identical", "rising", "large"]
ATT_DEFECT_CASE = ("identical", 17)              # the sequence on which the unmasked padding key is measured (see its test below)


def att_sequence(pattern, S):
    """One sequence's qkv rows [S][1152] as bf16 BITS (Q unscaled), a function of (pattern, S) only"""
    rng = np.random.default_rng((5, ATT_PATTERNS.index(pattern), S))
    q, k, v = (rng.standard_normal((S, 12, 32)) for _ in range(3))
    if pattern == "dominant":                    # one key per head 36.7 log2 units above the rest, for every query
        q[:, :, 0] = 12.0
        k[:, :, 0] = 0.0
        k[rng.integers(0, S, 12), np.arange(12), 0] = 12.0
    elif pattern == "identical":                 # every key the same: the output is the mean of V
        k[:] = k[rng.integers(0, S)]
    elif pattern == "rising":                    # scores rise ~0.05 log2 units per key: the maximum sits in the LAST 128-key chunk
        q[:, :, 1:] *= 0.1
        k[:, :, 1:] *= 0.1
        q[:, :, 0] = 4.0
        k[:, :, 0] = np.arange(S)[:, None] * (0.05 / (4.0 * C1))
    elif pattern == "large":                     # scaled scores up to about +-80: most 2^(s - m) underflow
        q *= 4.2
        k *= 4.2
    return bf16_bits(np.concatenate([q.reshape(S, 384), k.reshape(S, 384), v.reshape(S, 384)], axis=1).astype(F32))


def _att_split(bits):
    x = bits_f64(bits)
    S = len(x)
    return [x[:, 384 * i:384 * (i + 1)].reshape(S, 12, 32).transpose(1, 0, 2) for i in range(3)]


def _att_merge(o):
    return o.transpose(1, 0, 2).reshape(o.shape[1], 384)


def att_ref(bits):
    """softmax_2(Q K^T log2 e / sqrt 32) V in float64 -> (ctx [S][384], sum_k p_k |v_k| [S][384])"""
    q, k, v = _att_split(bits)
    s = (q @ k.transpose(0, 2, 1)) * C1
    p = np.exp2(s - s.max(-1, keepdims=True))
    l = p.sum(-1, keepdims=True)
    return _att_merge((p @ v) / l), _att_merge((p @ np.abs(v)) / l)


def att_emulation(bits, unmasked_pad=False):
    """Exact scores; numerator from bf16(p), denominator from p itself; bf16(output).  unmasked_pad: the DEFECT -- the first
    padding key (a zero K row and a zero V row: score 0) takes part in the maximum and in the denominator."""
    q, k, v = _att_split(bits)
    s = (q @ k.transpose(0, 2, 1)) * C1
    m = s.max(-1, keepdims=True)
    if unmasked_pad:
        m = np.maximum(m, 0.0)
    p = np.exp2(s - m)
    l = p.sum(-1, keepdims=True)
    if unmasked_pad:
        l = l + np.exp2(-m)
    return _att_merge(rne_bf16((rne_bf16(p) @ v) / l))


def att_err(a, ref, mag):
    """max |a - ref| / mag; where mag = 0 the answer is 0 and nothing else will do"""
    d = np.abs(a - ref)
    with np.errstate(all="ignore"):
        r = np.where(mag > 0, d / mag, np.where(d == 0, 0.0, np.inf))
    return float(np.nan_to_num(r, nan=np.inf).max())


# ------------------------------------------------------------------ ce_ffn_fused
GELU_N, GELU_R = 512, 4.5


def gelu_table():
    """ce_gelu_table: Phi at the 513 knots of [-4.5, 4.5] as fp32 (value, step to the next knot) pairs"""
    h = 2.0 * GELU_R / GELU_N
    phi = np.array([0.5 * (1.0 + math.erf((-GELU_R + i * h) * 0.70710678118654752440)) for i in range(GELU_N + 1)])
    return phi[:-1].astype(F32), (phi[1:] - phi[:-1]).astype(F32)


def phi_table(x, tab=None):
    """Phi(x) as ce_ffn_fused reads it: interval and fraction of t = clamp(x 512 / 9 + 256, 0, 511.99997), value + fraction x step"""
    val, step = tab if tab is not None else gelu_table()
    t = np.clip(np.asarray(x, dtype=F64) * (GELU_N / (2.0 * GELU_R)) + GELU_N / 2.0, 0.0, float(F32(511.99997)))
    i = np.floor(t).astype(np.int64)
    return val[i].astype(F64) + (t - i) * step[i].astype(F64)


def phi_erf(x):
    return 0.5 * (1.0 + erf(np.asarray(x, dtype=F64) / np.sqrt(2.0)))


def layer_norm(x, g, b, eps):
    xc = x - x.mean(1, keepdims=True)
    xh = xc / np.sqrt((xc * xc).mean(1, keepdims=True) + eps)
    return xh * g + b, xh


def ffn_ref(ctx, h, W, eps=LN_EPS):
    """LayerNorm2(y + W2 gelu(W1 y + b1) + b2), y = LayerNorm1(h + Wo ctx + bo), float64, exact erf GELU
    -> (out [M][384], max_c (|g_c xhat_c| + |b_c|) [M][1])"""
    y = layer_norm(h + ctx @ W["wo"].T + W["bo"], W["ln1_g"], W["ln1_b"], eps)[0]
    pre = y @ W["w1"].T + W["b1"]
    out, xh = layer_norm(y + (pre * phi_erf(pre)) @ W["w2"].T + W["b2"], W["ln2_g"], W["ln2_b"], eps)
    return out, (np.abs(W["ln2_g"] * xh) + np.abs(W["ln2_b"])).max(1, keepdims=True)


def ffn_emulation(ctx, h, W, eps=LN_EPS, phi=phi_table, w2=None):
    """bf16(y) is the FFN's operand while y itself stays the residual; bf16(x Phi(x)) with Phi from the table; the rest float64"""
    y = layer_norm(h + ctx @ W["wo"].T + W["bo"], W["ln1_g"], W["ln1_b"], eps)[0]
    pre = rne_bf16(y) @ W["w1"].T + W["b1"]
    g = rne_bf16(pre * phi(pre))
    return layer_norm(y + g @ (W["w2"] if w2 is None else w2).T + W["b2"], W["ln2_g"], W["ln2_b"], eps)[0]


def ffn_defect(ctx, h, W, eps=LN_EPS, group=37):
    """quads 1 and 2 of ONE 16-column group of W2 left unswapped: the kernel's operand order is quads (0, 2, 1, 3)"""
    w2 = W["w2"].copy()
    c = 16 * group
    w2[:, c + 4:c + 8], w2[:, c + 8:c + 12] = W["w2"][:, c + 8:c + 12], W["w2"][:, c + 4:c + 8]
    return ffn_emulation(ctx, h, W, eps, w2=w2)


def ffn_err(a, ref, den):
    return float((np.abs(a - ref) / den).max())


def ffn_ceiling(ctx, h, W, eps=LN_EPS):
    """Where the emulation may sit, from its two rounding sites alone.  A rounding to bf16 moves a value v by at most 2^-8 |v|;
    taken as independent and uniform that is an rms of 2^-8 |v| / sqrt 3.  First order: the FFN's output n moves by
    sum_c J_nc dy_c + sum_j W2_nj dg_j with J = W2 diag(gelu'(pre)) W1; the second LayerNorm scales a change of its input by
    at most |g_n| / sigma(row) (it only removes components).  Six rms of the largest element of a row, over the row's
    max (|g xhat| + |b|): at most a few thousand outputs are looked at, whose largest sits near 3.5 rms."""
    y = layer_norm(h + ctx @ W["wo"].T + W["bo"], W["ln1_g"], W["ln1_b"], eps)[0]
    pre = y @ W["w1"].T + W["b1"]
    phi = phi_erf(pre)
    dgelu = phi + pre * np.exp(-0.5 * pre * pre) / np.sqrt(2.0 * np.pi)
    g = pre * phi
    o = y + g @ W["w2"].T + W["b2"]
    _, xh = layer_norm(o, W["ln2_g"], W["ln2_b"], eps)
    den = (np.abs(W["ln2_g"] * xh) + np.abs(W["ln2_b"])).max(1)
    u2 = U * U / 3.0
    out = np.zeros(len(y))
    for r in range(len(y)):
        J = (W["w2"] * dgelu[r]) @ W["w1"]
        var = (((J * y[r]) ** 2).sum(1) + ((W["w2"] * g[r]) ** 2).sum(1)) * u2
        out[r] = 6.0 * (np.abs(W["ln2_g"]) * np.sqrt(var)).max() / o[r].std() / den[r]
    return float(out.max())


# ------------------------------------------------------------------ ce_embed_ln
def embed_ln(sd, tok, typ, pos, dt, eps=LN_EPS):
    """LayerNorm((word[tok] + type[typ]) + pos[pos]) in dtype dt -> (rows, max_c (|g_c xhat_c| + |b_c|))"""
    e = "bert.embeddings."
    t = lambda k: np.asarray(sd[e + k], dtype=F32).astype(dt)
    x = (t("word_embeddings.weight")[tok] + t("token_type_embeddings.weight")[typ]) + t("position_embeddings.weight")[pos]
    g, b = t("LayerNorm.weight"), t("LayerNorm.bias")
    mu = x.mean(1, keepdims=True, dtype=dt)
    xc = x - mu
    xh = xc / np.sqrt((xc * xc).mean(1, keepdims=True, dtype=dt) + dt(eps))
    return xh * g + b, (np.abs(g * xh) + np.abs(b)).max(1, keepdims=True)


# ------------------------------------------------------------------ the tests
def _sd():
    from review_recommender_amd import synth
    return synth.bert_state_dict(11, n_layers=2, n_labels=1, vocab=600)


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0e38, 1e-40], F64)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0e38, 1e-40], F64)
    got = rne_bf16(x)
    assert np.array_equal(got[:4], want[:4])                     # a tie goes to the even neighbour, just above it goes up
    assert np.all(np.abs(got[4:] - want[4:]) <= U * np.abs(want[4:]) + 2.0 ** -134)
    bits = np.arange(0x0080, 0x7F80, 7, dtype=np.uint16)           # every seventh positive normal bf16 survives a round trip
    assert np.array_equal(bf16_bits(bits_f64(bits).astype(F32)), bits)


def test_phi_table_is_ce_gelu_table():
    """513 knots over [-4.5, 4.5]: value = fp32(Phi(knot)), value + step = the next knot's Phi to fp32 rounding; at a knot the
    interpolation returns the value; outside the range it clamps; linear interpolation stays within h^2 / 8 max |Phi''| =
    9.4e-6 of Phi."""
    val, step = gelu_table()
    assert val.shape == step.shape == (512,) and val.dtype == step.dtype == F32
    knots = -4.5 + np.arange(513) * (9.0 / 512)
    phi = phi_erf(knots)
    assert np.abs(val.astype(F64) - phi[:-1]).max() <= 2.0 ** -24            # (fp32 rounding of a value <= 1)
    assert np.array_equal(val, np.array([0.5 * (1.0 + math.erf(k * 0.70710678118654752440)) for k in knots[:-1]]).astype(F32))
    assert np.abs(val.astype(F64) + step.astype(F64) - phi[1:]).max() <= 2.0 ** -23
    assert np.abs(phi_table(knots[:-1]) - val.astype(F64)).max() <= 2.0 ** -23      # (a knot may fall an ulp short of its interval)
    assert abs(float(phi_table(-40.0)) - 3.4e-6) < 5e-8 and float(phi_table(-40.0)) == float(val[0])
    assert abs(float(phi_table(40.0)) - (1.0 - 3.4e-6)) < 1e-7
    x = np.linspace(-4.5, 4.5, 20001)
    assert np.abs(phi_table(x) - phi_erf(x)).max() <= 9.4e-6 + 2.0 ** -23


def test_projection_emulation_defect_and_interval():
    sd = _sd()
    for layer in (0, 1):
        W = layer_weights(sd, layer)
        x = bits_f64(rand_bf16(np.random.default_rng((1, layer)), (33, 384)))
        ref, mag = proj_ref(x, W["wqkv"], W["bqkv"])
        e = lambda a: float((np.abs(a - ref) / mag).max())
        emu, bad = e(proj_emulation(x, W["wqkv"], W["bqkv"])), e(proj_defect(x, W["wqkv"], W["bqkv"]))
        print("projection, layer %d: emulation %.3e (ceiling %.3e)  wrong chunk %.3e" % (layer, emu, PROJ_CEILING, bad))
        assert emu <= PROJ_CEILING
        assert bad >= 10 * 4 * emu
        delta, r32 = proj_delta(x, W["wqkv"], W["bqkv"], ref, mag)
        assert proj_in_interval(rne_bf16(r32), ref, delta).all()
        # ... and the interval is no formality: the wrong chunk leaves it, so does a result two bf16 steps off
        assert not proj_in_interval(proj_defect(x, W["wqkv"], W["bqkv"]), ref, delta).all()
        off = bits_f64(bf16_bits(ref.astype(F32)) + np.uint16(2))
        assert not proj_in_interval(off, ref, delta)[np.abs(ref) >= 0.1].any()


def test_attention_emulation_under_its_ceiling_and_the_unmasked_key_far_above():
    """Every pattern at lengths over the 16-row, 32-key and 128-key edges: the emulation stays under 2^-7 of sum p |v|.  The
    defect -- the first padding key of a 17-token sequence left unmasked, a zero K row whose score is 0 -- is taken on the
    `identical` pattern (ATT_DEFECT_CASE): all 17 real keys of a (query, head) share ONE score there, and where that score
    is negative the padding key outweighs every one of them (0.32 of sum p |v|).  On `normal` and `rising` it is one key
    among 18 of similar weight (5e-2, 4e-2: printed); where one real key leads by tens of log2 units (`dominant`, `large`)
    a zero score weighs nothing and the defect cannot show in any metric."""
    worst = 0.0
    for pattern in ATT_PATTERNS:
        for S in (1, 2, 16, 17, 33, 129, 257):
            bits = att_sequence(pattern, S)
            ref, mag = att_ref(bits)
            worst = max(worst, att_err(att_emulation(bits), ref, mag))
    print("attention emulation, worst: %.3e (ceiling %.3e)" % (worst, ATT_CEILING))
    assert worst <= ATT_CEILING
    for pattern in ATT_PATTERNS:
        bits = att_sequence(pattern, ATT_DEFECT_CASE[1])
        ref, mag = att_ref(bits)
        emu, bad = att_err(att_emulation(bits), ref, mag), att_err(att_emulation(bits, unmasked_pad=True), ref, mag)
        print("attention, %s, 17 tokens: emulation %.3e  unmasked padding key %.3e" % (pattern, emu, bad))
        if pattern == ATT_DEFECT_CASE[0]:
            assert bad >= 10 * 4 * emu, (pattern, emu, bad)
    # a lone key: p = 1, the context is its V row, bit for bit
    bits = att_sequence("normal", 1)
    assert np.array_equal(bf16_bits(att_emulation(bits).astype(F32)), bits[:, 768:])


def test_ffn_emulation_under_its_ceiling_and_the_unswapped_group_far_above():
    sd = _sd()
    for layer, sdl in ((0, sd), (1, with_tails(sd))):
        W = layer_weights(sdl, layer)
        rng = np.random.default_rng((2, layer))
        ctx = bits_f64(rand_bf16(rng, (6, 384)))
        h = rng.standard_normal((6, 384)).astype(F32).astype(F64)
        ref, den = ffn_ref(ctx, h, W)
        emu, bad = ffn_err(ffn_emulation(ctx, h, W), ref, den), ffn_err(ffn_defect(ctx, h, W), ref, den)
        ceiling = ffn_ceiling(ctx, h, W)
        exact = ffn_err(ffn_emulation(ctx, h, W, phi=phi_erf), ref, den)
        print("fused FFN, layer %d%s: emulation %.3e (ceiling %.3e; with the exact erf %.3e)  unswapped group %.3e"
              % (layer, " (tails)" if layer else "", emu, ceiling, exact, bad))
        assert emu <= ceiling
        assert bad >= 10 * 4 * emu
    # what the table does beyond +-4.5: below -4.5 gelu is x Phi(-4.5) = x 3.4e-6, not 0; above, x (1 - 3.4e-6)
    assert abs(float(-40.0 * phi_table(-40.0)) + 40.0 * 3.4e-6) < 1e-5 and float(-40.0 * phi_erf(-40.0)) == 0.0


def test_embed_ln_float32_is_close_to_float64():
    sd = _sd()
    tok, typ, pos = np.array([0, 599, 7, 101]), np.array([0, 1, 1, 0]), np.array([0, 511, 3, 200])
    ref, den = embed_ln(sd, tok, typ, pos, F64)
    e32 = float((np.abs(embed_ln(sd, tok, typ, pos, F32)[0].astype(F64) - ref) / den).max())
    assert 0.0 < e32 < 1e-6
