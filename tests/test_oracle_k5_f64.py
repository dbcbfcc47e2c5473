"""The K5 oracle in double precision (CPU): oracle/cross_encoder.py with dtype=np.float64 -- the reference of the wide-range
kernel tests (tests/test_gpu_k5_x3_kernels.py) -- against its float32 self on the fixture model, and the default untouched."""
import numpy as np

from conftest import GOLDEN
from oracle import cross_encoder as OC
from review_recommender_amd import synth


def split(fx):
    cu = fx["cu_seqlens"]
    return [(fx["token_ids"][cu[i]:cu[i + 1]], fx["type_ids"][cu[i]:cu[i + 1]]) for i in range(len(cu) - 1)]


def test_float64_oracle_agrees_with_the_float32_oracle_on_the_fixture_model():
    """Same fp32 weights, every step in float64: on the fixture model (6 layers, O(1) activations) the two oracles agree
    within 2e-6 on logits -- the float32 oracle's own rounding --, the float64 one returns float64, and the default is the
    float32 oracle bit for bit (dtype=np.float32 spelled out gives the same bits as no dtype at all)."""
    fx = np.load(GOLDEN / "k5_cross_encoder.npz")
    sd = synth.bert_state_dict(int(fx["seed"]), n_layers=int(fx["n_layers"]), n_labels=1)
    seqs = split(fx)
    pick = [i for i, (ids, _) in enumerate(seqs) if len(ids) <= 140][:10] + [i for i, (ids, _) in enumerate(seqs) if len(ids) in (257, 512)][:2]
    some = [seqs[i] for i in pick]
    f32 = OC.predict_oracle(sd, some, n_layers=6)
    f64 = OC.predict_oracle(sd, some, n_layers=6, dtype=np.float64)
    assert f32.dtype == np.float32 and f64.dtype == np.float64
    print("float32 vs float64 oracle: max |logit difference|", np.abs(f32 - f64).max())
    assert np.abs(f32 - f64).max() < 2e-6
    assert np.array_equal(f32, OC.predict_oracle(sd, some, n_layers=6, dtype=np.float32))
    h32 = OC.bert_hidden(sd, *some[0], n_layers=6)
    h64 = OC.bert_hidden(sd, *some[0], n_layers=6, dtype=np.float64)
    assert h32.dtype == np.float32 and h64.dtype == np.float64
    assert np.abs(h32 - h64).max() < 2e-5                     # (hidden states of magnitude ~3)


def test_float64_query_encoder_oracle():
    fx = np.load(GOLDEN / "k5_query_encoder.npz")
    sd = synth.bert_state_dict(int(fx["seed"]), n_layers=12, n_labels=0, prefix="")
    seqs = split(fx)[:4]
    e32 = OC.encode_oracle(sd, seqs, n_layers=12)
    e64 = OC.encode_oracle(sd, seqs, n_layers=12, dtype=np.float64)
    assert e32.dtype == np.float32 and e64.dtype == np.float64
    assert np.abs(e32 - e64).max() < 2e-6
    np.testing.assert_allclose(np.linalg.norm(e64, axis=1), 1.0, atol=1e-12)
