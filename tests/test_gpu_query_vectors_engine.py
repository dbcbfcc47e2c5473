"""`SearchEngine(query_vectors="device")` against the same engine with `query_vectors="host"`, over one index built from text
with one encoder: frames, snips and dbg of `run_search_batch(queries, ...)` WITHOUT qvecs, bit for bit, with queries the front
hands back; a device tensor as `search_batch`'s qvecs; what the constructor refuses."""
import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

N = 300
WEIGHTS = dict(w_dense=0.45, w_bm25=0.15, w_rerank=0.3, w_prior=0.1, w_best=0.1, prior_C=20.0)
# handed back: a hard code point (the encoder's tokenizer: bit 32, the reranker's: bit 8), more than 1024 bytes (bit 1)
FLAGGED = ["Σigma cat socks", "yellow cat socks soft " * 50]


@pytest.fixture(scope="module")
def world():
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import CrossEncoder, QueryEncoder
    from review_recommender_amd.engine import SearchEngine
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(synth.WORDS) + ["##s", "##ing", "caf", "##e", "中", "文"]
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    enc = QueryEncoder(synth.bert_state_dict(31, n_layers=2, n_labels=0, prefix="", vocab=len(words)), tok)
    ce = CrossEncoder(synth.bert_state_dict(41, n_layers=2, vocab=len(words)), tok)
    texts = synth.text_corpus(N, 3, mean_len=25)
    n_rev, stars = synth.metadata(N, 2)
    products = pd.DataFrame({"sku": synth.skus(N), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})
    rev = pd.DataFrame({"sku": [products["sku"][i % N] for i in range(2 * N)], "text": [f"review {i} of it" for i in range(2 * N)],
                        "stars": [float(1 + i % 5) for i in range(2 * N)]})
    reviews = (rev, synth.unit_rows(2 * N, 384, 77))
    host = SearchEngine.from_products(products, enc, cross_encoder=ce, reviews=reviews, query_vectors="host")
    dev = SearchEngine.from_products(products, enc, cross_encoder=ce, reviews=reviews, query_vectors="device", query_text="device",
                                     gate="device", rerank="device")
    assert len(host.meta) == len(dev.meta) == N
    rng = np.random.default_rng(8)
    corpus_queries = [" ".join(rng.choice(texts[int(rng.integers(N))].split(), size=int(rng.integers(2, 6)))) for _ in range(10)]
    queries = corpus_queries[:5] + [FLAGGED[0], "red cat socks", "", "café 中文 mug"] + corpus_queries[5:] + [FLAGGED[1], "black dog toys"]
    return {"host": host, "dev": dev, "enc": enc, "ce": ce, "products": products, "queries": queries}


def same_answers(got, want):
    assert len(got) == len(want)
    for (gf, gs, gd), (wf, ws, wd) in zip(got, want):
        pd.testing.assert_frame_equal(gf, wf, check_exact=True)
        for c in gf.columns:                                   # (check_exact compares values; the bits as well)
            if gf[c].values.dtype.kind == "f":
                assert gf[c].values.tobytes() == wf[c].values.tobytes(), c
        assert gs == ws and gd == wd


@pytest.mark.parametrize("rerank_k", [0, 20])
def test_device_query_vectors_equal_host_bitwise(world, monkeypatch, rerank_k):
    host, dev, enc, queries = world["host"], world["dev"], world["enc"], world["queries"]
    assert dev.query_vectors == "device" and host.query_vectors == "host" and dev._query_text.encoder is enc
    args = (10, rerank_k, *WEIGHTS.values(), True, 50000, 8, 0.5)
    want = host.run_search_batch(queries, *args)
    assert any(s for _, s, _ in want) and any(f["_bm25"].abs().max() > 0 for f, _, _ in want)
    assert any((f["_gate"] < 1).any() for f, _, _ in want) and all(len(f) == 10 for f, _, _ in want)
    encoded = []
    inner = enc.encode
    monkeypatch.setattr(enc, "encode", lambda s, **k: (encoded.append(list(s)), inner(s, **k))[1])
    got = dev.run_search_batch(queries, *args)
    assert encoded == [FLAGGED]                                # nothing but the queries handed back went through the host
    same_answers(got, want)
    # explicit qvecs keep their meaning: no vectors are made, none are encoded
    del encoded[:]
    qv = inner(queries, normalize_embeddings=True)
    same_answers(dev.run_search_batch(queries, *args, qvecs=qv), want)
    assert encoded == []
    same_answers([dev.run_search(queries[0], *args)], want[:1])           # run_search is unchanged: the host encoder, one query


def test_a_device_tensor_as_qvecs(world):
    import torch
    from review_recommender_amd import synth
    s = world["dev"].searcher
    qv = synth.unit_rows(5, 384, 99)
    ids = [[1, 2], [], [3], [4, 5, 6], [7]]
    want = s.search_batch(qv, ids, 10)
    got = s.search_batch(torch.from_numpy(qv).cuda(), ids, 10)
    strided = torch.from_numpy(np.concatenate([qv, qv], axis=1)).cuda()[:, :384]              # made contiguous by the call
    for res in (got, s.search_batch(strided, ids, 10)):
        for name in ("pool_rows", "columns", "order", "dense_raw", "bm25_raw"):
            assert getattr(res, name).tobytes() == getattr(want, name).tobytes(), name
    with pytest.raises(ValueError, match="float32 on"):
        s.search_batch(torch.from_numpy(qv).cuda().double(), ids, 10)
    with pytest.raises(ValueError, match="float32 on"):
        s.search_batch(torch.from_numpy(qv), ids, 10)
    with pytest.raises(ValueError, match=r"qvecs must be \(B, 384\)"):
        s.search_batch(torch.from_numpy(qv).cuda()[:, :100], ids, 10)
    with pytest.raises(ValueError, match="carries the query vectors"):
        s.search_batch(None, ids, 10)
    front = world["dev"]._query_text.front(["red cat"], 0.5, vectors=False)
    with pytest.raises(ValueError, match="carries the query vectors"):
        s.search_batch(None, None, 10, query_front=front)


def test_what_the_constructor_refuses(world):
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.engine import SearchEngine
    host, enc = world["host"], world["enc"]
    make = lambda **kw: SearchEngine(host.meta, None, None, index=host.index, **kw)
    with pytest.raises(ValueError, match="query_vectors must be"):
        make(encoder=enc, query_vectors="gpu")
    with pytest.raises(ValueError, match="needs query_text=\"device\""):
        make(encoder=enc, query_vectors="device")
    with pytest.raises(ValueError, match="this package's QueryEncoder with a tokenizer"):
        make(query_text="device", query_vectors="device")

    class Other:
        def encode(self, sentences, **kw):
            return np.zeros((len(sentences), 384), dtype=np.float32)
    with pytest.raises(ValueError, match="this package's QueryEncoder with a tokenizer"):
        make(encoder=Other(), query_text="device", query_vectors="device")
    bare = QueryEncoder(synth.bert_state_dict(31, n_layers=2, n_labels=0, prefix="", vocab=len(enc.tokenizer.vocab)))
    with pytest.raises(ValueError, match="this package's QueryEncoder with a tokenizer"):
        make(encoder=bare, query_text="device", query_vectors="device")
    with pytest.raises(ValueError, match="query_vectors must be"):
        SearchEngine.from_products(world["products"], enc, query_vectors="nowhere")
