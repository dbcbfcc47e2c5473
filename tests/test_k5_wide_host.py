"""cross_encoder.model_shape: the encoder's block shape read off a state dict and checked against what rr_ce_create accepts
(include/rr_hip.h), without a GPU or the library."""
import numpy as np
import pytest

from review_recommender_amd import synth
from review_recommender_amd.cross_encoder import model_shape


def _sd(hidden, ffn, prefix="bert."):
    return synth.bert_state_dict(1, n_layers=1, hidden=hidden, ffn=ffn, vocab=16, max_pos=8, n_labels=1, prefix=prefix)


@pytest.mark.parametrize("hidden,heads,ffn", [(128, 2, 512), (256, 8, 1024), (768, 12, 3072), (1024, 16, 4096), (384, 12, 1536)])
def test_model_shape_of_the_supported_shapes(hidden, heads, ffn):
    """TinyBERT-L-2, a 32-wide-head model, BERT-base, bge-large and the shape with kernels of its own: (hidden, heads, ffn)
    comes back as given, with either prefix of the state dict."""
    assert model_shape(_sd(hidden, ffn), n_heads=heads) == (hidden, heads, ffn)
    assert model_shape(_sd(hidden, ffn, prefix=""), n_heads=heads) == (hidden, heads, ffn)


def test_model_shape_default_heads_and_the_config_override():
    """Without n_heads: 12 at hidden 384, hidden // 64 elsewhere.  `num_attention_heads` of a config.json wins over the
    default, the keyword over both."""
    assert model_shape(_sd(384, 1536))[1] == 12
    assert model_shape(_sd(128, 512))[1] == 2
    assert model_shape(_sd(768, 3072))[1] == 12
    assert model_shape(_sd(1024, 4096))[1] == 16
    assert model_shape(_sd(256, 1024))[1] == 4
    assert model_shape(_sd(256, 1024), cfg={"num_attention_heads": 8}) == (256, 8, 1024)
    assert model_shape(_sd(256, 1024), n_heads=4, cfg={"num_attention_heads": 8}) == (256, 4, 1024)
    assert model_shape(_sd(384, 1536), cfg={"num_attention_heads": 6}) == (384, 6, 1536)      # head dim 64: the runtime-shape kernels
    assert model_shape(_sd(768, 3072), cfg={}) == (768, 12, 3072)


@pytest.mark.parametrize("hidden,heads,ffn,number", [(200, None, 512, "200"), (2048, None, 4096, "2048"), (768, 16, 3072, "48"),
                                                     (768, 12, 1000, "1000")])
def test_model_shape_refuses_a_shape_outside_the_family(hidden, heads, ffn, number):
    """hidden 200 (no multiple of 128), hidden 2048 (beyond 1024), head dim 48 (768 / 16), ffn 1000: a ValueError that names
    the offending number, in rr_ce_create's words."""
    with pytest.raises(ValueError, match=r"rr_ce_create: .*\b%s\b" % number):
        model_shape(_sd(hidden, ffn), n_heads=heads)


def test_model_shape_refuses_bf16_at_another_shape():
    """precision bf16 at 768 / 12 / 3072: a ValueError that names the precision; at 384 / 12 / 1536 it passes."""
    with pytest.raises(ValueError, match="precision bf16"):
        model_shape(_sd(768, 3072), precision="bf16")
    assert model_shape(_sd(384, 1536), precision="bf16") == (384, 12, 1536)
    assert model_shape(_sd(768, 3072), precision="fp32") == (768, 12, 3072)


def test_model_shape_needs_a_bert_state_dict():
    with pytest.raises(ValueError):
        model_shape({"x": np.zeros(3)})
    sd = _sd(128, 512)
    del sd["bert.encoder.layer.0.intermediate.dense.weight"]
    with pytest.raises(ValueError, match="no encoder layers"):
        model_shape(sd)
