"""The encoder forward at block shapes other than 384 / 12 / 1536 (csrc/rr_ce.hip: ce_forward_w over ce_gemm_x3 and the kernels of
csrc/rr_ce_w.hip) end to end against the float64 oracle, oracle.cross_encoder.bert_hidden(..., n_heads=, dtype=np.float64).

The rule for every tolerance is that of tests/test_gpu_k5_x3_kernels.py: a bar is a constant within 4x the error of the float32
oracle (the reference's arithmetic) on the same model and sequences against the float64 one, asserted as bar <= 4 * e32.  Every
bar below is twice the float32 oracle's error, set from numpy alone before the kernels first ran."""
import functools
import warnings

import numpy as np
import pytest

from oracle import cross_encoder as OC
from review_recommender_amd import synth
from review_recommender_amd.cross_encoder import OUT_CLS, OUT_HIDDEN, OUT_LOGITS, BertEncoderGPU, CrossEncoder, QueryEncoder

pytestmark = pytest.mark.gpu
F64 = np.float64
SHAPES = [(128, 2, 512), (768, 12, 3072), (1024, 16, 4096)]
LENS = list(range(1, 41)) + [127, 128, 129, 512]
# per shape: (hidden states, max |error| / max |hidden|; logits, max |error|) -- twice the float32 oracle's own figures
# (128: 2.83e-7 and 2.14e-7;  768: 1.10e-6 and 2.66e-6;  1024: 1.15e-6 and 3.80e-6); CLS rows are hidden states: their bar
HIDDEN_BARS = {128: 5.7e-7, 768: 2.2e-6, 1024: 2.3e-6}
LOGIT_BARS = {128: 4.3e-7, 768: 5.3e-6, 1024: 7.6e-6}
# the 12-layer 768 query encoder, unit vectors: twice the float32 oracle's 2.55e-7
QUERY_BAR = 5.1e-7


def _seqs(lens, seed, vocab=2000):
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        ids = rng.integers(0, vocab, n).astype(np.int32)
        ids[0] = 101
        out.append((ids, (np.arange(n) > n // 3).astype(np.int32)))
    return out


def _logits(sd, h_cls, dt):
    pooled = np.tanh(h_cls.astype(dt) @ sd["bert.pooler.dense.weight"].astype(dt).T + sd["bert.pooler.dense.bias"].astype(dt))
    return (pooled @ sd["classifier.weight"].astype(dt).T + sd["classifier.bias"].astype(dt)).astype(dt)


@functools.lru_cache(maxsize=None)
def reference(hidden, heads, ffn):
    """(state dict, sequences, float64 hidden states of every token, float32 ones, float64 logits, float32 logits), computed
    once per shape and left unchanged."""
    sd = synth.bert_state_dict(5, n_layers=2, hidden=hidden, ffn=ffn, vocab=2000, n_labels=1)
    seqs = _seqs(LENS, 4)
    h64 = [OC.bert_hidden(sd, *s, n_layers=2, n_heads=heads, dtype=F64) for s in seqs]
    h32 = [OC.bert_hidden(sd, *s, n_layers=2, n_heads=heads) for s in seqs]
    l64 = _logits(sd, np.stack([h[0] for h in h64]), F64)
    l32 = _logits(sd, np.stack([h[0] for h in h32]), np.float32)
    return sd, seqs, np.concatenate(h64), np.concatenate(h32), l64, l32


@pytest.mark.parametrize("hidden,heads,ffn", SHAPES, ids=["128-2-512", "768-12-3072", "1024-16-4096"])
def test_wide_forward_against_float64(hidden, heads, ffn):
    """Two-layer models at 128 / 2 / 512, 768 / 12 / 3072 and 1024 / 16 / 4096 on sequences of 1 .. 40, 127, 128, 129 and 512 tokens:
    OUT_HIDDEN (relative to max |hidden|), OUT_CLS (likewise) and OUT_LOGITS against the float64 oracle, each under a bar of
    twice the float32 oracle's error (asserted within 4x of it).
    float32 oracle, hidden / logits: 128: 2.83e-7 / 2.14e-7;  768: 1.10e-6 / 2.66e-6;  1024: 1.15e-6 / 3.80e-6.
    First MI355X run -- kernel, hidden / CLS / logits: 128: 3.01e-7 / 2.09e-7 / 1.92e-7;  768: 2.19e-6 / 1.70e-6 / 3.85e-6;
    1024: 2.37e-6 / 2.37e-6 / 7.31e-6 -- the 1024 case missed its bar (2.3e-6): FFN-2 then was ONE ce_gemm_x3 launch, a sum
    over K = 4096 in one fp32 accumulator (6 K / 16 additions in a row), 2.1x the float32 oracle's blocked sums.  ce_forward_w
    now sums FFN-2 over K in chunks of 2048, one launch each, and the LayerNorm adds the parts -- 768: 1.57e-6 / 1.54e-6 /
    3.79e-6;  1024: 2.00e-6 / 1.86e-6 / 6.80e-6 (chunks of 1024: 1.27e-6 and 1.81e-6 on hidden states, at twice the launches).
    The bars are the ones chosen before the first run."""
    sd, seqs, h64, h32, l64, l32 = reference(hidden, heads, ffn)
    model = BertEncoderGPU(sd, n_heads=heads)
    assert (model.hidden, model.n_heads, model.ffn) == (hidden, heads, ffn)
    hid = model.forward_ids(seqs, OUT_HIDDEN)
    cls = model.forward_ids(seqs, OUT_CLS)
    logits = model.forward_ids(seqs, OUT_LOGITS)
    assert hid.shape == h64.shape and cls.shape == (len(seqs), hidden) and logits.shape == (len(seqs), 1)
    scale = np.abs(h64).max()
    first = np.concatenate([[0], np.cumsum([len(s[0]) for s in seqs])])[:-1]
    e_hid, e32_hid = np.abs(hid - h64).max() / scale, np.abs(h32 - h64).max() / scale
    e_cls = np.abs(cls - h64[first]).max() / scale
    e_log, e32_log = np.abs(logits - l64).max(), np.abs(l32 - l64).max()
    print("%d / %d / %d: hidden / max |hidden| = %.3g: kernel %.3e  float32 oracle %.3e;  CLS kernel %.3e;  logits kernel %.3e  float32 oracle %.3e"
          % (hidden, heads, ffn, scale, e_hid, e32_hid, e_cls, e_log, e32_log))
    assert np.isfinite(hid).all() and np.isfinite(cls).all() and np.isfinite(logits).all()
    assert HIDDEN_BARS[hidden] <= 4 * e32_hid and LOGIT_BARS[hidden] <= 4 * e32_log
    model.close()
    missed = [name for name, e, bar in [("hidden", e_hid, HIDDEN_BARS[hidden]), ("CLS", e_cls, HIDDEN_BARS[hidden]),
                                        ("logits", e_log, LOGIT_BARS[hidden])] if not e < bar]
    assert not missed, (missed, e_hid, e_cls, HIDDEN_BARS[hidden], e_log, LOGIT_BARS[hidden])


@pytest.mark.parametrize("hidden,heads,ffn", SHAPES, ids=["128-2-512", "768-12-3072", "1024-16-4096"])
def test_wide_forward_does_not_depend_on_batch_composition_or_chunking(hidden, heads, ffn):
    """Logits and CLS rows are the same bits for every sequence alone, all in one call, and chunked with
    max_tokens_per_call = 600; after a forward `out_of_range` is False and `set_wide_range(True)` changes no bit."""
    sd, seqs, *_ = reference(hidden, heads, ffn)
    seqs = seqs[:12] + seqs[36:]                 # 1 .. 12, 37 .. 40, 127, 128, 129, 512
    ce = CrossEncoder(sd, n_heads=heads)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    logits, cls = ce.predict_ids(seqs), ce.model.forward_ids(seqs, OUT_CLS)
    assert np.isfinite(logits).all() and not ce.model.out_of_range()
    assert np.array_equal(bits(logits), bits(np.concatenate([ce.predict_ids([s]) for s in seqs])))
    assert np.array_equal(bits(cls), bits(np.concatenate([ce.model.forward_ids([s], OUT_CLS) for s in seqs])))
    chunked = CrossEncoder(sd, n_heads=heads)
    chunked.model.max_tokens_per_call = 600
    assert np.array_equal(bits(logits), bits(chunked.predict_ids(seqs)))
    assert np.array_equal(bits(cls), bits(chunked.model.forward_ids(seqs, OUT_CLS)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ce.model.set_wide_range(True)
    assert np.array_equal(bits(logits), bits(ce.predict_ids(seqs))) and not ce.model.out_of_range()
    assert np.array_equal(bits(cls), bits(ce.model.forward_ids(seqs, OUT_CLS)))
    assert ce.model.last_forward_ms() > 0.0


def test_wide_query_encoder_against_float64():
    """A 12-layer 768 / 12 / 3072 encoder without a head: `encode_ids(..., normalize_embeddings=True)` against
    `encode_oracle(dtype=float64)` under twice the float32 oracle's error; norms within 1e-6 of 1 (one fp32 normalisation:
    768 squares summed and one division, each rounded to 6e-8).
    float32 oracle 2.55e-7.  First MI355X run -- kernel 3.7e-7; with FFN-2 summed in chunks of 2048 (see above) 4.0e-7."""
    sd = synth.bert_state_dict(8, n_layers=12, hidden=768, ffn=3072, vocab=2000, n_labels=0, prefix="")
    seqs = _seqs([3, 5, 8, 9, 12, 17, 33, 64], 9)
    o64 = OC.encode_oracle(sd, seqs, n_layers=12, dtype=F64)
    o32 = OC.encode_oracle(sd, seqs, n_layers=12)
    enc = QueryEncoder(sd)
    assert enc.hidden == 768 and enc.model.n_heads == 12
    emb = enc.encode_ids(seqs, normalize_embeddings=True)
    e, e32 = np.abs(emb - o64).max(), np.abs(o32 - o64).max()
    print("768 / 12 / 3072 x 12 layers: unit vectors  kernel %.3e  float32 oracle %.3e" % (e, e32))
    assert emb.shape == (len(seqs), 768) and emb.dtype == np.float32
    assert QUERY_BAR <= 4 * e32
    assert e < QUERY_BAR
    assert np.abs(np.linalg.norm(emb.astype(F64), axis=1) - 1.0).max() < 1e-6


def test_wide_shapes_refuse_bf16_and_shapes_outside_the_family():
    """precision="bf16" at 768 is refused before any device call (ValueError naming the precision); rr_ce_create itself
    answers RR_E_INVALID with a NULL handle to bf16 at 768, to hidden 200, to a head dim of 48 and to ffn 1000, and names
    the precision or the number."""
    import ctypes as C
    from review_recommender_amd import _lib
    sd = synth.bert_state_dict(5, n_layers=1, hidden=768, ffn=3072, vocab=64, n_labels=1)
    with pytest.raises(ValueError, match="precision bf16"):
        CrossEncoder(sd, precision="bf16")
    lib = _lib.load()
    z = np.zeros(8, np.float32)
    ptrs = (C.c_void_p * 25)(*[z.ctypes.data] * 25)             # never read: the shape is refused first
    for (hidden, heads, ffn, precision), word in [((768, 12, 3072, 0), "precision bf16"), ((200, 2, 512, 1), "hidden 200"),
                                                  ((768, 16, 3072, 1), "head dim 48"), ((768, 12, 1000, 1), "ffn 1000"),
                                                  ((2048, 32, 4096, 1), "hidden 2048")]:
        cfg = _lib.CEConfig(hidden, 1, heads, ffn, 64, 512, 2, 1, 1e-12, precision)
        h = C.c_void_p(0xdead)
        rc = lib.rr_ce_create(0, C.byref(cfg), ptrs, 25, C.byref(h))
        assert rc == -1 and not h.value, (hidden, heads, ffn, precision, rc)
        with pytest.raises(ValueError, match=word):
            _lib.check(rc, "rr_ce_create")
