"""CPU side of the GPU index builder (bm25.build_bm25_index): the vocabulary ids it hands the device are
BM25Corpus.from_corpus's, and the document offsets of the flattened token stream are right."""
import math

import numpy as np

from review_recommender_amd.bm25 import BM25Corpus, doc_offsets, factorize_corpus


def _ids_of(c: BM25Corpus, corpus):
    return np.array([c.vocab[w] for doc in corpus for w in doc], dtype=np.int32)


def test_factorized_ids_are_from_corpus_dict_ids():
    rng = np.random.default_rng(3)
    corpus = [[f"w{int(t)}" for t in rng.zipf(1.3, rng.integers(0, 40)) % 500] for _ in range(300)]
    corpus[5] = []
    tok, off, vocab = factorize_corpus(corpus)
    c = BM25Corpus.from_corpus(corpus)
    assert vocab == c.vocab and list(vocab) == list(c.vocab)          # same ids, same first-appearance order
    assert tok.dtype == np.int32 and np.array_equal(tok, _ids_of(c, corpus))
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(d) for d in corpus])]))


def test_non_str_tokens_take_the_dict_loop():
    nan = math.nan
    corpus = [["a", None, "b"], [None, 3, "a"], [nan, "c", 3.0], [], [True, 1, "b"]]
    tok, off, vocab = factorize_corpus(corpus)
    c = BM25Corpus.from_corpus(corpus)
    assert list(vocab.items()) == list(c.vocab.items())
    assert np.array_equal(tok, _ids_of(c, corpus))
    assert tok[1] == vocab[None] and tok[3] == vocab[None]             # None is a token, not a missing value


def test_doc_offsets():
    corpus = [["x"] * n for n in (0, 3, 0, 0, 1, 7, 0)]
    off = doc_offsets(corpus)
    assert off.dtype == np.int64
    assert off.tolist() == [0, 0, 3, 3, 3, 4, 11, 11]
    assert doc_offsets([]).tolist() == [0]
    assert doc_offsets([[], []]).tolist() == [0, 0, 0]


def test_from_ids_equals_from_corpus():
    rng = np.random.default_rng(8)
    corpus = [[f"w{int(t)}" for t in rng.integers(0, 90, rng.integers(0, 30))] for _ in range(400)]
    corpus[0], corpus[-1] = [], ["w1"] * 5
    for case in (corpus, [[], []], [["a"]]):
        want = BM25Corpus.from_corpus(case)
        tok, off, vocab = factorize_corpus(case)
        got = BM25Corpus.from_ids(tok, off, len(vocab), vocab=vocab)
        for k in ("doc_indptr", "doc_terms", "doc_tf", "doc_len"):
            a, b = getattr(got, k), getattr(want, k)
            assert a.dtype == b.dtype and np.array_equal(a, b), k
        assert got.idf.tobytes() == want.idf.tobytes() and got.avgdl == want.avgdl and got.vocab == want.vocab
