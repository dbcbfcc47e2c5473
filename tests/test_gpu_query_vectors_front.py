"""The query vectors of the query front (`QueryText(..., encoder=)`: device WordPiece of the encoder's vocabulary, the forward,
rr_query_vectors_dev) against `QueryEncoder.encode(queries, normalize_embeddings=True)`, bit for bit on every query the front
answers; bit 32 of ``needs_host`` exactly where the tokenizer's CPU model hands the query back; zeros in every flagged row."""
import json

import numpy as np
import pytest

from conftest import GOLDEN
from query_cases import CRAFTED, corpus_vocab
from query_vector_cases import assert_bitwise

pytestmark = pytest.mark.gpu

MAX_LENGTH = 32
# an ordinary query, a hard code point (U+03A3: wp_unicode.model_tokenize flags it), the empty string, non-ASCII the table
# maps (accents stripped, CJK split), more than MAX_LENGTH pieces (one per letter)
FIRST = ["wireless cat socks", "Σigma cat", "", "Çat naïve café 中文 socks",
         " ".join("abcdefghijklmnopqrstuvwxyz"[i % 26] for i in range(2 * MAX_LENGTH))]
ALL = FIRST + CRAFTED


@pytest.fixture(scope="module")
def world():
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.querytext import QueryText
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    tok = WordPieceTokenizer({w: i for i, w in enumerate(json.loads((GOLDEN / "k5_tokenizer.json").read_text())["vocab"])})
    enc = QueryEncoder(synth.bert_state_dict(53, n_layers=2, n_labels=0, prefix="", vocab=len(tok.vocab)), tok,
                       max_length=MAX_LENGTH)
    qt = QueryText(corpus_vocab(), rerank_tokenizer=tok, max_length=512, encoder=enc)
    yield {"tok": tok, "enc": enc, "qt": qt}
    qt.close()


def model_flags(queries, tok):
    from review_recommender_amd.wp_unicode import model_tokenize
    return np.array([model_tokenize(q.encode("utf-8"), tok, MAX_LENGTH)[1] != 0 for q in queries])


def test_the_queries_cover_what_they_are_named_for(world):
    from review_recommender_amd.wp_unicode import model_tokenize
    tok = world["tok"]
    assert model_flags(FIRST, tok).tolist() == [False, True, False, False, False]
    assert len(model_tokenize(FIRST[4].encode(), tok, None)[0]) > MAX_LENGTH == len(model_tokenize(FIRST[4].encode(), tok, MAX_LENGTH)[0])
    assert model_tokenize(FIRST[3].encode(), tok, MAX_LENGTH)[0] == tok.encode_pair(FIRST[3], None, MAX_LENGTH)[0].tolist()
    assert tok.unk_id not in tok.encode_pair("café 中文", None, MAX_LENGTH)[0].tolist()


@pytest.mark.parametrize("B", [1, 3, 65, len(ALL)])
def test_front_vectors_equal_the_host_encoder_bitwise(world, B):
    from review_recommender_amd.querytext import FLAG_ENCODER
    qt, enc, tok = world["qt"], world["enc"], world["tok"]
    queries = ALL[:B]
    front = qt.front(queries, 0.5)
    assert front.qvecs.shape == (B, 384) and front.qvecs.is_cuda
    got = front.qvecs.cpu().numpy()
    flags = front.needs_host.cpu().numpy()
    qt.check()
    assert qt.redo_vectors(front) is False                               # (O(1) activations: the fp16-pair kernels hold)
    want = enc.encode(queries, normalize_embeddings=True)
    assert want.dtype == np.float32 and np.isfinite(want).all() and not enc.model.wide_range
    assert ((flags & FLAG_ENCODER) != 0).tolist() == model_flags(queries, tok).tolist()
    answered = flags == 0
    if B >= 3:
        assert answered.any() and not answered.all()
    assert_bitwise(got[answered], want[answered])
    assert not got[~answered].view(np.uint32).any()                      # zeros, every bit
    if B == len(ALL):
        assert (flags & FLAG_ENCODER).any() and (flags & ~FLAG_ENCODER).any()     # both kinds of flag were met


def test_front_without_vectors_and_without_an_encoder(world):
    from review_recommender_amd.querytext import QueryText
    front = world["qt"].front(ALL[:3], 0.5, vectors=False)
    assert front.qvecs is None and not (front.needs_host.cpu().numpy() & 32).any()
    with pytest.raises(ValueError, match="QueryEncoder with a tokenizer"):
        QueryText(corpus_vocab(), encoder=object())
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import QueryEncoder
    with pytest.raises(ValueError, match="QueryEncoder with a tokenizer"):
        QueryText(corpus_vocab(), encoder=QueryEncoder(synth.bert_state_dict(53, n_layers=2, n_labels=0, prefix="", vocab=200)))
