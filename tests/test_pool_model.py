"""Mean pooling on the host (CPU): `cross_encoder.model_pool_mean` -- the statement of csrc/rr_ce_pool.hip's summation order --
against float64, `pooling_of_dir` on model directories, and tests/golden/k5_mean_pooling.npz pinned to the numpy oracle.

The accuracy bar is the rule of tests/test_gpu_k5_x3_kernels.py: twice numpy float32's own worst error against float64 on
the same rows, computed here (tests/pool_model.py: pool_errors)."""
import json

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import cross_encoder as OC
from pool_model import F32, F64, bits, pool_errors, rows_of
from review_recommender_amd import synth
from review_recommender_amd.cross_encoder import model_pool_mean, pooling_of_dir

LENGTHS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 511, 512]


@pytest.mark.parametrize("data", ["normal", "offset"])
@pytest.mark.parametrize("hidden", [128, 384, 1024])
def test_model_pool_mean_against_float64(hidden, data):
    rows, cu = rows_of(hidden, data, LENGTHS)
    got = model_pool_mean(rows, cu)
    assert got.dtype == F32 and got.shape == (len(LENGTHS), hidden)
    err, err_np = pool_errors(got, rows, cu)
    print(f"hidden {hidden} {data}: model_pool_mean {err:.3e}, numpy float32 {err_np:.3e}")
    assert err <= 2 * err_np
    # a sequence of one token is that token; of two, (a + b) / 2 in one rounding each
    assert np.array_equal(bits(got[0]), bits(rows[0]))
    assert np.array_equal(bits(got[1]), bits((rows[1] + rows[2]) / F32(2)))


def test_the_order_is_the_documented_one():
    """Eight interleaved partial sums in increasing t, the tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), one division:
    spelled out with scalar float32 operations on one column of 21 tokens."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((21, 128)) * 10.0 ** rng.integers(-3, 4, (21, 128))).astype(F32)
    p = [F32(0)] * 8
    for t in range(21):
        p[t % 8] = F32(p[t % 8] + x[t, 5])
    want = F32(F32(F32(F32(p[0] + p[1]) + F32(p[2] + p[3])) + F32(F32(p[4] + p[5]) + F32(p[6] + p[7]))) / F32(21))
    got = model_pool_mean(x, [0, 21])
    assert bits(got[0, 5:6])[0] == bits(np.array([want]))[0]


def test_a_sequence_alone_and_inside_a_batch_gives_the_same_bits():
    rows, cu = rows_of(384, "offset", LENGTHS, seed=1)
    batch = model_pool_mean(rows, cu)
    for s in range(len(LENGTHS)):
        alone = model_pool_mean(rows[cu[s]:cu[s + 1]], [0, LENGTHS[s]])
        assert np.array_equal(bits(alone[0]), bits(batch[s])), LENGTHS[s]
    order = np.argsort(LENGTHS)[::-1]                  # the same sequences in another order
    rev = np.concatenate([rows[cu[s]:cu[s + 1]] for s in order])
    cu_rev = np.concatenate([[0], np.cumsum([LENGTHS[s] for s in order])])
    assert np.array_equal(bits(model_pool_mean(rev, cu_rev)), bits(batch[order]))
    for bad in ([0, 5, 5, int(cu[-1])], [1, int(cu[-1])], [0, 7]):
        with pytest.raises(ValueError):
            model_pool_mean(rows, bad)


REFUSED = ["pooling_mode_max_tokens", "pooling_mode_mean_sqrt_len_tokens", "pooling_mode_weightedmean_tokens", "pooling_mode_lasttoken"]


def pooling_cfg(*on):
    keys = ["pooling_mode_cls_token", "pooling_mode_mean_tokens"] + REFUSED
    return dict({"word_embedding_dimension": 384, "include_prompt": True}, **{k: k in on for k in keys})


def test_pooling_of_dir(tmp_path):
    bare = tmp_path / "bare"
    bare.mkdir()
    assert pooling_of_dir(bare) == "cls"                                  # no 1_Pooling: a plain Hugging Face directory

    def model_dir(name, cfg, nested=False):
        d = tmp_path / name
        (d / "1_Pooling").mkdir(parents=True)
        (d / "1_Pooling" / "config.json").write_text(json.dumps(cfg))
        if nested:
            (d / "0_Transformer").mkdir()
        return d

    assert pooling_of_dir(model_dir("cls", pooling_cfg("pooling_mode_cls_token"))) == "cls"
    assert pooling_of_dir(model_dir("mean", pooling_cfg("pooling_mode_mean_tokens"))) == "mean"
    nested = model_dir("nested", pooling_cfg("pooling_mode_mean_tokens"), nested=True)
    assert pooling_of_dir(nested) == "mean" and pooling_of_dir(nested / "0_Transformer") == "mean"
    assert pooling_of_dir(str(nested)) == "mean"
    for mode in REFUSED:
        with pytest.raises(ValueError, match=mode):
            pooling_of_dir(model_dir("no_" + mode, pooling_cfg(mode)))
    with pytest.raises(ValueError, match="pooling_mode_cls_token.*pooling_mode_mean_tokens"):   # two modes: concatenated vectors
        pooling_of_dir(model_dir("both", pooling_cfg("pooling_mode_cls_token", "pooling_mode_mean_tokens")))
    with pytest.raises(ValueError, match="no pooling_mode"):
        pooling_of_dir(model_dir("none", pooling_cfg()))


def golden_seqs(fx):
    cu = fx["cu_seqlens"]
    return [(fx["token_ids"][cu[i]:cu[i + 1]], np.zeros(cu[i + 1] - cu[i], dtype=np.int32)) for i in range(len(cu) - 1)]


@pytest.mark.parametrize("name", ["h384", "h128"])
def test_the_golden_file_is_the_oracles_float64_mean(name):
    """tests/golden/k5_mean_pooling.npz (`transformers` on a padded batch with its mask) against the float64 mean of
    oracle.cross_encoder.bert_hidden over the unpadded tokens, l2-normalised: the bar of the CLS fixture's oracle test
    (tests/test_oracle_k5.py: 2e-5)."""
    fx = np.load(GOLDEN / "k5_mean_pooling.npz")
    hidden, heads, ffn = (int(v) for v in fx[name + "_shape"])
    sd = synth.bert_state_dict(int(fx[name + "_seed"]), n_layers=int(fx["n_layers"]), hidden=hidden, ffn=ffn, vocab=int(fx["vocab"]),
                               n_labels=0, prefix="")
    seqs = golden_seqs(fx)
    assert [len(s[0]) for s in seqs] == [1, 2, 3, 9, 17, 64, 65, 128]
    mean = np.stack([OC.bert_hidden(sd, *s, n_layers=int(fx["n_layers"]), n_heads=heads, prefix="", dtype=F64).mean(axis=0) for s in seqs])
    emb = mean / np.maximum(np.linalg.norm(mean, axis=1, keepdims=True), 1e-12)
    print(name, "max |oracle - golden|", np.abs(emb - fx[name + "_embeddings"]).max())
    np.testing.assert_allclose(emb, fx[name + "_embeddings"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(mean, fx[name + "_mean_raw"], atol=2e-5 * np.abs(mean).max(), rtol=0)
    np.testing.assert_allclose(np.linalg.norm(fx[name + "_embeddings"], axis=1), 1.0, atol=1e-6)
