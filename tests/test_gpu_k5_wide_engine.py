"""A 768-wide query encoder and a 128-wide cross-encoder through `SearchEngine`: the index `from_products` builds has the encoder's
width and the oracle's rows, query vectors made on the device equal the host's bit for bit, `search` returns the oracle's skus,
the device rerank equals the host rerank bit for bit, and an encoder of another width than the index is refused."""
import numpy as np
import pandas as pd
import pytest

from oracle import cross_encoder as OC
from oracle.bm25 import BM25OkapiOracle
from oracle.pipeline import run_search_oracle
from parity import assert_ranking_matches

pytestmark = pytest.mark.gpu

N = 3000
VOCAB = 2000
WEIGHTS = dict(w_dense=0.45, w_bm25=0.15, w_rerank=0.3, w_prior=0.1, w_best=0.1, prior_C=20.0)
# index rows against the float64 oracle's unit vectors on every 47th product (64 of them: the float64 oracle takes 80 ms per
# product), max |error|: twice the float32 oracle's own 1.36e-7 (numpy alone, before the kernels first ran)
ROW_BAR = 2.7e-7
ROW_STEP = 47


@pytest.fixture(scope="module")
def world():
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import CrossEncoder, QueryEncoder
    from review_recommender_amd.embed import filter_products
    from review_recommender_amd.engine import SearchEngine
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(synth.WORDS) + ["##s", "##ing"]
    words += ["w%04d" % i for i in range(VOCAB - len(words))]
    assert len(words) == VOCAB
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    sd_q = synth.bert_state_dict(31, n_layers=2, hidden=768, ffn=3072, n_labels=0, prefix="", vocab=VOCAB)
    enc = QueryEncoder(sd_q, tok)
    ce = CrossEncoder(synth.bert_state_dict(41, n_layers=2, hidden=128, ffn=512, vocab=VOCAB), tok, n_heads=2)
    texts = synth.text_corpus(N, 3, mean_len=25)
    n_rev, stars = synth.metadata(N, 2)
    products = pd.DataFrame({"sku": synth.skus(N), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})
    host = SearchEngine.from_products(products, enc, cross_encoder=ce)
    qv = SearchEngine.from_products(products, enc, cross_encoder=ce, query_vectors="device", query_text="device")
    rr = SearchEngine.from_products(products, enc, cross_encoder=ce, rerank="device")
    _, model_texts = filter_products(products)
    assert len(host.meta) == len(model_texts) == N
    rng = np.random.default_rng(8)
    queries = [" ".join(rng.choice(texts[int(rng.integers(N))].split(), size=int(rng.integers(2, 6)))) for _ in range(8)]
    return {"host": host, "qv": qv, "rr": rr, "enc": enc, "ce": ce, "tok": tok, "sd_q": sd_q, "texts": model_texts, "queries": queries}


@pytest.fixture(scope="module")
def oracle_rows(world):
    """The float64 oracle's unit vectors of every 47th product (float64), computed once."""
    tok, enc = world["tok"], world["enc"]
    seqs = [tok.encode_pair(t, None, enc.max_length) for t in world["texts"][::ROW_STEP]]
    return seqs, OC.encode_oracle(world["sd_q"], seqs, n_layers=2, dtype=np.float64)


def same_answers(got, want):
    assert len(got) == len(want)
    for (gf, gs, gd), (wf, ws, wd) in zip(got, want):
        pd.testing.assert_frame_equal(gf, wf, check_exact=True)
        for c in gf.columns:                                   # (check_exact compares values; the bits as well)
            if gf[c].values.dtype.kind == "f":
                assert gf[c].values.tobytes() == wf[c].values.tobytes(), c
        assert gs == ws and gd == wd


def test_from_products_builds_an_index_of_the_encoders_width(world, oracle_rows):
    """`from_products` with a 768 / 12 / 3072 encoder gives an index of dim 768 whose rows are the float64 oracle's unit vectors
    within twice the float32 oracle's error (asserted within 4x of it) on every 47th product; every row is finite and of
    norm 1 to 1e-6.  float32 oracle 1.36e-7.  First MI355X run -- index rows 2.98e-7, a tenth above the bar: FFN-2
    then summed K = 3072 in one fp32 accumulator.  With the sum in chunks of 2048 (tests/test_gpu_k5_wide.py,
    test_wide_forward_against_float64) 2.05e-7.  The bar is the one chosen before the first run."""
    host, enc = world["host"], world["enc"]
    seqs, want = oracle_rows
    assert enc.hidden == 768 and host.index.dim == 768 and host.index.n_rows == N
    rows = host.index.download_rows()
    assert rows.shape == (N, 768) and np.isfinite(rows).all()
    o32 = OC.encode_oracle(world["sd_q"], seqs, n_layers=2)
    e, e32 = np.abs(rows[::ROW_STEP] - want).max(), np.abs(o32 - want).max()
    print("768-wide index of %d products: rows  kernel %.3e  float32 oracle %.3e" % (N, e, e32))
    assert ROW_BAR <= 4 * e32
    assert e < ROW_BAR
    assert np.abs(np.linalg.norm(rows.astype(np.float64), axis=1) - 1.0).max() < 1e-6


@pytest.mark.parametrize("rerank_k", [0, 20])
def test_device_query_vectors_equal_host_bitwise_at_768(world, rerank_k):
    """`run_search_batch` of 8 queries with query_vectors="device" and "host": bitwise equal frames, snips and dbg."""
    host, qv = world["host"], world["qv"]
    assert qv.query_vectors == "device" and host.query_vectors == "host"
    args = (10, rerank_k, *WEIGHTS.values(), False, 0, 8, 0.5)
    want = host.run_search_batch(world["queries"], *args)
    assert all(len(f) == 10 for f, _, _ in want) and any(f["_bm25"].abs().max() > 0 for f, _, _ in want)
    front = qv._query_text.front(world["queries"], 0.5)
    assert tuple(front.qvecs.shape) == (8, 768)
    same_answers(qv.run_search_batch(world["queries"], *args), want)


def test_search_returns_the_oracles_skus(world):
    """`search(query, k=10, alpha=0.5)` against `run_search_oracle` on the oracle's float64 query vector (and the index's rows,
    which the test above holds to the oracle's), through parity.assert_ranking_matches with the tie band of
    tests/test_gpu_k5.py (2e-5)."""
    from review_recommender_amd.artifacts import build_bm25_blob
    host, tok, enc = world["host"], world["tok"], world["enc"]
    V = host.index.download_rows()
    blob = build_bm25_blob(host.meta)
    bm25 = BM25OkapiOracle(blob["corpus"])
    for query in world["queries"][:4]:
        got, _, _ = host.search(query, k=10, alpha=0.5)
        q64 = OC.encode_oracle(world["sd_q"], [tok.encode_pair(query, None, enc.max_length)], n_layers=2, dtype=np.float64)[0]
        want, _, _, cand = run_search_oracle(query=query, qvec=q64.astype(np.float32), meta=host.meta, V=V, bm25=bm25, bm25_skus=blob["skus"],
                                             k=10, rerank_k=0, w_dense=0.5, w_bm25=0.5, w_rerank=0.0, w_prior=0.0, w_best=0.0,
                                             prior_C=20.0, min_reviews=8, gate_penalty=1.0)
        assert_ranking_matches(got["sku"].tolist(), want["sku"].tolist(), want["_final"].values, 2e-5,
                               cand["sku"].tolist(), cand["_final"].values)


def test_device_rerank_with_a_128_wide_cross_encoder_equals_host_bitwise(world):
    """rerank="device" with the 128 / 2 / 512 cross-encoder against rerank="host": the frames of `run_search_batch`, bit for bit."""
    host, rr = world["host"], world["rr"]
    assert rr.searcher.rerank_text is not None and host.searcher.rerank_text is None
    assert world["ce"].model.hidden == 128 and world["ce"].model.n_heads == 2
    args = (10, 20, *WEIGHTS.values(), False, 0, 8, 0.5)
    want = host.run_search_batch(world["queries"], *args)
    assert any(f["_rerank"].abs().max() > 0 for f, _, _ in want)
    same_answers(rr.run_search_batch(world["queries"], *args), want)


def test_an_encoder_of_another_width_is_refused(world):
    """A 384-wide QueryEncoder on the 768-wide index: a ValueError that names both numbers."""
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.engine import SearchEngine
    host = world["host"]
    small = QueryEncoder(synth.bert_state_dict(31, n_layers=1, n_labels=0, prefix="", vocab=VOCAB), world["tok"])
    assert small.hidden == 384
    with pytest.raises(ValueError, match=r"384.*768"):
        SearchEngine(host.meta, None, None, encoder=small, index=host.index)
