"""RR_CE_OUT_MEAN through rr_ce_forward_dev on its four forward paths -- bf16 at 384 (ce_forward_bf16), fp32 at 384 on the fp16-pair
kernels (ce_forward_h2), the same after set_wide_range(True) (ce_forward_x3), fp32 at 128 / 2 / 512 (ce_forward_w) -- on the ids
of tests/golden/k5_mean_pooling.npz (sequences of 1, 2, 3, 9, 17, 64, 65 and 128 tokens).

  * the pooled rows are `model_pool_mean` of the SAME handle's OUT_HIDDEN rows, bit for bit: every layer ran over all tokens
    and the kernel summed them in the contract's order;
  * on the three fp32 paths the normalised rows are within 1e-5 of `transformers`' (the project's embedding bar);
  * a sequence alone and among the others gives the same bits;
  * OUT_CLS and OUT_LOGITS give the same bits before and after an OUT_MEAN call on the handle (the [CLS]-only tail is theirs);
  * a model that leaves fp16's range: NaN rows for the whole call, `out_of_range()`, and `forward_ids` reruns by itself."""
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from pool_model import bits
from review_recommender_amd import synth
from review_recommender_amd.cross_encoder import OUT_CLS, OUT_HIDDEN, OUT_LOGITS, OUT_MEAN, BertEncoderGPU, model_pool_mean

pytestmark = pytest.mark.gpu
F32_EMB_TOL = 1e-5                               # tests/test_gpu_k5.py's bar of the fp32 query encoder
BF16_EMB_TOL = 8e-3                              # ... and of the bf16 one (printed and held too: the same model family)
PATHS = ["bf16-384", "fp32-384", "fp32-384-wide", "fp32-128"]


def state_dict(fx, name, changes=()):
    """The golden model `name` WITH a pooler / classifier: bert_state_dict draws the head last, so the encoder's weights are
    the ones the fixture was made with."""
    hidden, heads, ffn = (int(v) for v in fx[name + "_shape"])
    sd = synth.bert_state_dict(int(fx[name + "_seed"]), n_layers=int(fx["n_layers"]), hidden=hidden, ffn=ffn, vocab=int(fx["vocab"]),
                               n_labels=1, prefix="")
    for key, factor in changes:
        sd[key] = sd[key] * np.float32(factor)
    return sd, heads


def wide(model):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.set_wide_range(True)
    return model


@pytest.fixture(scope="module")
def world():
    fx = np.load(GOLDEN / "k5_mean_pooling.npz")
    cu = fx["cu_seqlens"]
    seqs = [(fx["token_ids"][cu[i]:cu[i + 1]], np.zeros(cu[i + 1] - cu[i], dtype=np.int32)) for i in range(len(cu) - 1)]
    sd384, h384 = state_dict(fx, "h384")
    sd128, h128 = state_dict(fx, "h128")
    models = {"bf16-384": BertEncoderGPU(sd384, precision="bf16", n_heads=h384), "fp32-384": BertEncoderGPU(sd384, n_heads=h384),
              "fp32-384-wide": wide(BertEncoderGPU(sd384, n_heads=h384)), "fp32-128": BertEncoderGPU(sd128, n_heads=h128)}
    assert all(m.n_labels == 1 for m in models.values())
    return dict(fx=fx, cu=cu, seqs=seqs, models=models)


@pytest.mark.parametrize("path", PATHS)
def test_mean_rows_are_the_model_of_the_hidden_rows_and_match_transformers(world, path):
    m, fx, seqs, cu = world["models"][path], world["fx"], world["seqs"], world["cu"]
    cls0, logits0 = m.forward_ids(seqs, OUT_CLS), m.forward_ids(seqs, OUT_LOGITS)
    mean = m.forward_ids(seqs, OUT_MEAN)
    hidden = m.forward_ids(seqs, OUT_HIDDEN)
    assert not m.out_of_range() and m.wide_range == (path == "fp32-384-wide")
    assert mean.shape == (len(seqs), m.hidden) and mean.dtype == np.float32 and np.isfinite(mean).all()
    assert np.array_equal(bits(mean), bits(model_pool_mean(hidden, cu)))
    assert np.array_equal(bits(mean[0]), bits(hidden[0]))                       # one token: the mean is the token
    # the [CLS] modes before and after: the same bits (and CLS is the first hidden row of every sequence, not a mean)
    assert np.array_equal(bits(m.forward_ids(seqs, OUT_CLS)), bits(cls0)) and np.array_equal(bits(m.forward_ids(seqs, OUT_LOGITS)), bits(logits0))
    assert np.abs(cls0[3:] - mean[3:]).max() > 0.1
    emb = (mean / np.maximum(np.linalg.norm(mean, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    want = fx[("h128" if path == "fp32-128" else "h384") + "_embeddings"]
    err = np.abs(emb - want).max()
    print(f"{path}: max |normalised mean - transformers| {err:.3e}")
    assert err < (BF16_EMB_TOL if path == "bf16-384" else F32_EMB_TOL)


@pytest.mark.parametrize("path", PATHS)
def test_a_sequence_alone_and_among_the_others_gives_the_same_bits(world, path):
    m, seqs = world["models"][path], world["seqs"]
    batch = m.forward_ids(seqs, OUT_MEAN)
    for i in (0, 2, 4, 6):
        assert np.array_equal(bits(m.forward_ids([seqs[i]], OUT_MEAN)[0]), bits(batch[i])), len(seqs[i][0])
    rev = m.forward_ids(seqs[::-1], OUT_MEAN)
    assert np.array_equal(bits(rev[::-1]), bits(batch))
    chunked_cap, m.max_tokens_per_call = m.max_tokens_per_call, 130                  # several calls: 1 + 2 + ... split at 130 tokens
    try:
        assert np.array_equal(bits(m.forward_ids(seqs, OUT_MEAN)), bits(batch))
    finally:
        m.max_tokens_per_call = chunked_cap


def test_a_pass_beyond_the_fp16_range_poisons_every_pooled_row(world):
    """Layer 0's FFN-1 x 4e4 (tests/test_gpu_k5_x3_kernels.py's variant): the GELU epilogue meets |x| > 65504 on the fp16-pair
    path.  The raw OUT_MEAN call returns NaN in every row -- never a finite mean of garbage --, `out_of_range()` says why, and
    `forward_ids` switches the handle and returns what a handle in wide range from the start returns."""
    import torch
    fx, seqs, cu = world["fx"], world["seqs"], world["cu"]
    sd, heads = state_dict(fx, "h384", [("encoder.layer.0.intermediate.dense.weight", 4e4)])
    want = wide(BertEncoderGPU(sd, n_heads=heads)).forward_ids(seqs, OUT_MEAN)
    assert np.isfinite(want).all()
    auto = BertEncoderGPU(sd, n_heads=heads)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    lens = np.diff(cu)
    ids = np.concatenate([s[0] for s in seqs])
    pos = np.arange(cu[-1]) - np.repeat(cu[:-1], lens)
    raw = auto.forward_packed_dev(t(ids), t(np.zeros_like(ids)), t(pos), t(cu), len(seqs), int(lens.max()), OUT_MEAN)
    torch.cuda.synchronize()
    assert auto.out_of_range()
    assert raw.shape == (len(seqs), 384) and bool(torch.isnan(raw).all())
    with pytest.warns(UserWarning, match="fp16 range"):
        got = auto.forward_ids(seqs, OUT_MEAN)
    assert auto.wide_range and not auto.out_of_range()
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want))


def test_an_unknown_mode_is_still_refused(world):
    m, seqs = world["models"]["fp32-384"], world["seqs"]
    with pytest.raises(ValueError, match="unknown mode 4"):
        m.forward_ids(seqs[:2], 4)
