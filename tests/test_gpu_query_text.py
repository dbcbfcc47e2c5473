"""The query front on the device (querytext.QueryText, csrc/rr_query.hip) against querytext.model_front, bit for bit: BM25
ids, packed gate groups, reranker ids and the needs_host flags, over batch sizes that cross a workgroup, empty and flagged
batches; and the three consumers (K2, the gate match, the pair kernels) fed with the device-made buffers against the same
kernels fed with the host-packed ones."""
import json

import numpy as np
import pytest

from conftest import GOLDEN
from query_cases import CRAFTED, corpus_vocab, random_ascii_queries

pytestmark = pytest.mark.gpu

N, POOL = 2000, 150


@pytest.fixture(scope="module")
def tok():
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    return WordPieceTokenizer({w: i for i, w in enumerate(json.loads((GOLDEN / "k5_tokenizer.json").read_text())["vocab"])})


@pytest.fixture(scope="module")
def fronts(tok):
    """QueryText per max_length, made on first use."""
    from review_recommender_amd.querytext import QueryText
    made = {}

    def get(L, vocab=None):
        key = (L, id(vocab))
        if key not in made:
            made[key] = QueryText(corpus_vocab() if vocab is None else vocab, rerank_tokenizer=tok if L else None,
                                  max_length=L or 512)
        return made[key]
    yield get
    for qt in made.values():
        qt.close()


def expected(queries, vocab, tok=None, L=512):
    """The arrays the kernels must write, from the model: dict like QueryFront.host_arrays()."""
    from review_recommender_amd.querytext import model_front
    ms = [model_front(q, vocab, rerank_tokenizer=tok, max_length=L) for q in queries]
    cum = lambda xs: np.cumsum([0] + list(xs)).astype(np.int32)
    terms = [t for m in ms for t in m.terms]
    out = {"needs_host": np.array([m.flag for m in ms], dtype=np.int32),
           "ids": np.array([i for m in ms for i in m.ids], dtype=np.int32), "ids_off": cum(len(m.ids) for m in ms),
           "q_term": cum(len(m.terms) for m in ms), "q_groups": np.array([len(m.groups) for m in ms], dtype=np.int32),
           "term_off": cum(len(w) for _, w in terms), "term_group": np.array([g for g, _ in terms], dtype=np.int32),
           "term_bytes": np.frombuffer(b"".join(w for _, w in terms), dtype=np.uint8)}
    if tok is not None:
        out["rr_ids"] = np.array([i for m in ms for i in m.rerank_ids], dtype=np.int32)
        out["rr_off"] = cum(len(m.rerank_ids) for m in ms)
    return out, ms


def assert_front(qt, queries, vocab, tok=None, L=512):
    front = qt.front(queries, 0.5)
    got = front.host_arrays()
    qt.check()
    want, ms = expected(queries, vocab, tok, L)
    assert set(got) == set(want)
    assert set(np.flatnonzero(got["needs_host"]).tolist()) == {i for i, m in enumerate(ms) if m.flag}      # the sets, exactly
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    return front, ms


def test_crafted_queries_equal_the_model_bitwise(fronts, tok):
    _, ms = assert_front(fronts(512), CRAFTED, corpus_vocab(), tok, 512)
    assert sum(1 for m in ms if m.flag) >= 5 and sum(1 for m in ms if m.groups) >= 40


@pytest.mark.parametrize("B", [1, 5, 257])
def test_batch_sizes_across_a_workgroup(fronts, tok, B):
    queries = [CRAFTED[(7 * i + 3) % len(CRAFTED)] for i in range(B)]
    assert_front(fronts(512), queries, corpus_vocab(), tok, 512)


def test_without_a_reranker_and_with_an_empty_vocabulary(fronts):
    front, _ = assert_front(fronts(0), CRAFTED[:40], corpus_vocab())
    assert front.rerank_staged is None
    empty = {}
    _, ms = assert_front(fronts(0, empty), ["cat dog", "red"], empty)
    assert [m.ids for m in ms] == [[-1, -1], [-1]]


def test_empty_flagged_and_mixed_batches(fronts, tok):
    qt, vocab = fronts(512), corpus_vocab()
    _, ms = assert_front(qt, ["", "", ""], vocab, tok, 512)
    assert not any(m.flag for m in ms)
    _, ms = assert_front(qt, ["the of and", "?!", " "], vocab, tok, 512)
    flagged = ["z" * 1025, "cat " + "t" * 65, "y" * 2000]
    _, ms = assert_front(qt, flagged, vocab, tok, 512)
    assert all(m.flag for m in ms)
    _, ms = assert_front(qt, ["red cat", flagged[0], "blue dog socks", flagged[1], "wireless"], vocab, tok, 512)
    assert [bool(m.flag) for m in ms] == [False, True, False, True, False]


@pytest.mark.parametrize("L", [8, 9, 512])
def test_reranker_ids_equal_pack_queries(fronts, tok, L):
    from review_recommender_amd.rerank import pack_queries
    letters = "abcdefghijklmnopqrstuvwxyz"
    queries = [" ".join(letters[i % 26] for i in range(n)) for n in (L - 4, L - 3, L - 2, 0, 2)]    # one id per letter
    id_lists = [tok.text_ids(q) for q in queries]
    assert [len(i) for i in id_lists] == [L - 4, L - 3, L - 2, 0, 2] and max(len(q) for q in queries) <= 1024
    front, ms = assert_front(fronts(L), queries, corpus_vocab(), tok, L)
    packed = pack_queries(id_lists, L)
    got = front.host_arrays()
    assert packed.host_queries == [2] == np.flatnonzero(got["needs_host"]).tolist() and got["needs_host"][2] == 4
    assert got["rr_ids"].tobytes() == packed.ids.tobytes() and got["rr_off"].tobytes() == packed.off.tobytes()
    buf, at = front.rerank_staged                               # as RerankText.pairs(staged=) reads it
    want_buf, want_at = packed.buffer()
    assert buf[:len(packed.off)].cpu().numpy().tolist() == want_buf[:want_at].tolist()
    assert buf[at:at + len(packed.ids)].cpu().numpy().tolist() == packed.ids.tolist()


def test_bad_offsets_are_refused(fronts, hip):
    qt = fronts(0)
    raw = np.frombuffer(b"red catblue dog", dtype=np.uint8)
    for off in ([0, 7, 3, 15], [0, 7, 16], [-1, 7, 15]):
        front = qt.front_bytes(raw, np.array(off, dtype=np.int64), [0.5] * (len(off) - 1))
        flags = front.needs_host.cpu().numpy()
        with pytest.raises(ValueError, match="offsets"):
            qt.check()
        assert (flags & 16).any()
    qt.check()                                                  # (the count was cleared)
    import ctypes as C
    assert hip.rr_query_front_dev(qt._h, None, 0, None, 0, None, None, 512, *([None] * 4), 0, *([None] * 5), 0, 0, None) == -1
    assert hip.rr_query_strip_dev(qt._h, None, None, 0, 1, None, None, None, 0, None) == -1
    assert hip.rr_query_status(None, C.byref(C.c_int32())) == -1


# ---------------------------------------------------------------------------------- the consumers
@pytest.fixture(scope="module")
def world(tok):
    import torch
    from review_recommender_amd import synth
    from review_recommender_amd.bm25 import BM25Corpus
    from review_recommender_amd.engine import HybridSearcher
    from review_recommender_amd.gate import GateText
    from review_recommender_amd.index import ProductIndex
    from review_recommender_amd.rerank import RerankText
    words = [w for w in tok.vocab if w.isascii() and w.isalpha()]
    rng = np.random.default_rng(5)
    texts = [t + " " + " ".join(rng.choice(words, size=6)) for t in synth.text_corpus(N, 3, mean_len=20)]
    corpus = BM25Corpus.from_corpus([t.split() for t in texts])
    index = ProductIndex.from_rows(synth.unit_rows(N, 384, 1), normalize=False)
    index.set_meta(*synth.metadata(N, 2))
    searcher = HybridSearcher(index, corpus.to_device(0), GateText.from_texts(texts), RerankText.from_texts(texts, tok, 512))
    rows = torch.from_numpy(np.stack([rng.permutation(N)[:POOL] for _ in range(64)]).astype(np.int64)).cuda()
    pick = lambda: " ".join(rng.choice(texts[int(rng.integers(N))].split(), size=int(rng.integers(2, 6))))
    queries = [pick() for _ in range(24)] + random_ascii_queries(20, seed=3) + \
        ["red cat socks", "black", "wireless noise cancelling headphones", "", "the of", "pinK kitten", "golden design print"]
    return {"searcher": searcher, "corpus": corpus, "rows": rows, "queries": queries[:64] + [""] * (64 - len(queries))}


def test_consumers_read_the_device_buffers_as_the_host_packed_ones(world, tok):
    import torch
    from review_recommender_amd import text
    from review_recommender_amd.gate import pack_groups
    from review_recommender_amd.querytext import QueryText, model_front
    from review_recommender_amd.rerank import pack_queries
    s, corpus, rows, queries = world["searcher"], world["corpus"], world["rows"], world["queries"]
    assert rows.shape == (len(queries), POOL)
    assert not any(model_front(q, corpus.vocab, rerank_tokenizer=tok, max_length=512).flag for q in queries)
    qt = QueryText(corpus.vocab, rerank_tokenizer=tok, max_length=512)
    try:
        front = qt.front(queries, 0.5)
        # K2
        id_lists = [corpus.term_ids(text.tokenize_query(q)) for q in queries]
        want = s.bm25_at(id_lists, rows)
        got = s.bm25_at(front.terms, rows)
        assert float(want.abs().max()) > 0 and torch.equal(got, want)
        # the gate match
        packed = pack_groups([text.build_gate_groups(q) for q in queries], 0.5)
        want_g, want_h = s.gate_text.factors(rows, packed, want_hits=True)
        got_g, got_h = s.gate_text.factors(rows, front, staged=front.gate_staged, want_hits=True)
        assert len(set(want_g.flatten().tolist())) > 2 and torch.equal(got_g, want_g) and torch.equal(got_h, want_h)
        # the pair kernels
        pq = pack_queries([tok.text_ids(q) for q in queries], 512)
        want_p = s.rerank_text.pairs(rows, 20, pq)
        got_p = s.rerank_text.pairs(rows, 20, front, staged=front.rerank_staged)
        assert int(want_p[3][-1]) > 20 * len(queries) * 3
        assert all(torch.equal(g, w) for g, w in zip(got_p, want_p))
        qt.check()
        s.gate_text.check()
        s.rerank_text.check()
    finally:
        qt.close()
