"""`SearchEngine(rerank="device")` (rerank.py, csrc/rr_pairs.hip) against `rerank="host"`: the frames of `run_search` and
`run_search_batch`, bit for bit -- the packed forward does not depend on how the pairs are batched, so the same ids give the
same logits -- with the hand-back of long queries, chunking, the wide-range rerun and the refusals."""
import warnings

import numpy as np
import pandas as pd
import pytest

import cli_worlds as W

pytestmark = pytest.mark.gpu

N = 300
LONG_QUERY = "yellow cat socks soft " * 150                     # 600 tokens: more than 512 - 3
QUERIES = ["wireless headphones for running", "yellow cat socks", "blue insulated coffee mug"]
ARGS = dict(k=10, w_dense=0.45, w_bm25=0.15, w_rerank=0.3, w_prior=0.1, w_best=0.0, prior_C=20.0, use_snips=False, max_scan=0,
            min_reviews=8)


@pytest.fixture(scope="module")
def world():
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import CrossEncoder
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(synth.WORDS) + ["for", "the", "of", "and"]
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    texts = synth.text_corpus(N, 3, mean_len=25)
    texts[5] = (texts[5] + " ") * 40                            # cut at 2000 characters, inside a word or not
    texts[9] = ""
    n_rev, stars = synth.metadata(N, 2)
    meta = pd.DataFrame({"sku": synth.skus(N), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})
    blob = {"skus": meta["sku"].tolist(), "corpus": [t.split() for t in texts]}
    emb = synth.unit_rows(N, W.DIM, 1234)
    sd = synth.bert_state_dict(41, n_layers=2, vocab=len(words))
    return {"meta": meta, "emb": emb, "blob": blob, "tok": tok, "sd": sd, "ce": CrossEncoder(sd, tok), "engines": {},
            "qvecs": synth.unit_rows(len(QUERIES) + 1, W.DIM, 99), "words": words}


def engine_of(world, flavour, gate, rerank, ce=None):
    from review_recommender_amd.engine import SearchEngine
    key = (flavour, gate, rerank, id(ce))
    if key not in world["engines"]:
        world["engines"][key] = SearchEngine(world["meta"], world["emb"], world["blob"], cross_encoder=ce or world["ce"],
                                             flavour=flavour, gate=gate, rerank=rerank)
    return world["engines"][key]


def bits_equal(got: pd.DataFrame, want: pd.DataFrame):
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for c in got.columns:
        g, w = got[c].values, want[c].values
        assert g.dtype == w.dtype, c
        if g.dtype.kind == "f":
            assert g.tobytes() == w.tobytes(), (c, g[:5], w[:5])
        else:
            assert g.tolist() == w.tolist(), c


def same_answers(got, want):
    assert len(got) == len(want)
    for (gf, gs, gd), (wf, ws, wd) in zip(got, want):
        bits_equal(gf, wf)
        assert gs == ws and gd == wd


def no_host_predict(monkeypatch, ce):
    def boom(*a, **k):
        raise AssertionError("the host predict ran although the engine has a token plane")
    monkeypatch.setattr(ce, "predict", boom)


@pytest.mark.parametrize("gate", ["host", "device"])
@pytest.mark.parametrize("flavour", ["app", "cli"])
def test_device_rerank_equals_host_rerank_bitwise(world, flavour, gate, monkeypatch):
    host = engine_of(world, flavour, gate, "host")
    dev = engine_of(world, flavour, gate, "device")
    assert dev.searcher.rerank_text is not None and host.searcher.rerank_text is None
    assert world["ce"].activation is None
    floor = 150 if flavour == "app" else 100
    for rerank_k, pen in ((20, 0.5), (20, 1.0), (floor, 0.5), (400, 0.5)):    # < pool, = pool, > n_rows (pool = rr_k = 300)
        args = dict(ARGS, rerank_k=rerank_k, gate_penalty=pen)
        want = [host.run_search(q, qvec=v, **args) for q, v in zip(QUERIES, world["qvecs"])]
        want_b = host.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
        assert all(f["_rerank"].dtype == np.float32 and f["_rerank"].nunique() > 1 for f, _, _ in want)
        with monkeypatch.context() as m:
            no_host_predict(m, world["ce"])
            got = [dev.run_search(q, qvec=v, **args) for q, v in zip(QUERIES, world["qvecs"])]
            got_b = dev.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
        same_answers(got, want)
        same_answers(got_b, want_b)
    dev.searcher.rerank_text.check()


def test_sigmoid_differs_by_at_most_one_ulp(world, monkeypatch):
    host, dev = engine_of(world, "app", "host", "host"), engine_of(world, "app", "host", "device")
    args = dict(ARGS, rerank_k=40, gate_penalty=0.5)
    monkeypatch.setattr(world["ce"], "activation", "sigmoid")
    want = host.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
    got = dev.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
    for (gf, _, _), (wf, _, _) in zip(got, want):
        assert gf["sku"].tolist() == wf["sku"].tolist()
        g, w = gf["_rerank"].values, wf["_rerank"].values
        assert g.dtype == w.dtype == np.float32
        ulps = np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64))
        print("sigmoid: largest difference of _rerank in float32 ulps:", int(ulps.max()))
        assert ulps.max() <= 1
        for c in ("_dense", "_bm25", "_prior", "_best", "_gate", "_trust", "_final"):
            assert np.abs(gf[c].values.astype(np.float64) - wf[c].values.astype(np.float64)).max() <= 1e-6, c


def test_a_query_longer_than_the_model_goes_through_the_host(world):
    host, dev = engine_of(world, "app", "host", "host"), engine_of(world, "app", "host", "device")
    assert len(world["tok"].text_ids(LONG_QUERY)) > 512 - 3
    queries = [QUERIES[0], LONG_QUERY, QUERIES[1], QUERIES[2]]
    args = dict(ARGS, rerank_k=30, gate_penalty=0.5)
    calls = []
    predict = world["ce"].predict
    want = host.run_search_batch(queries, qvecs=world["qvecs"], **args)
    world["ce"].predict = lambda pairs, **kw: (calls.append(len(pairs)), predict(pairs, **kw))[1]
    try:
        got = dev.run_search_batch(queries, qvecs=world["qvecs"], **args)
        alone = dev.run_search(LONG_QUERY, qvec=world["qvecs"][1], **args)
    finally:
        del world["ce"].predict
    assert calls == [30, 30]                                     # only the long query's rows, once per call
    same_answers(got, want)
    same_answers([alone], [want[1]])


def test_three_chunks_equal_one(world, monkeypatch):
    host, dev = engine_of(world, "cli", "host", "host"), engine_of(world, "cli", "host", "device")
    args = dict(ARGS, rerank_k=20, gate_penalty=1.0)
    one = dev.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
    want = host.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
    monkeypatch.setattr(world["ce"].model, "max_tokens_per_call", 512 * 25)       # 60 pairs: 25 + 25 + 10, cut inside queries
    calls = []
    pairs = dev.searcher.rerank_text.pairs
    monkeypatch.setattr(dev.searcher.rerank_text, "pairs", lambda *a, **k: (calls.append(a[3:5]), pairs(*a, **k))[1])
    three = dev.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
    assert calls == [(0, 25), (25, 25), (50, 10)]
    same_answers(three, one)
    same_answers(three, want)


def test_what_the_device_path_refuses(world):
    from review_recommender_amd.engine import SearchEngine
    from review_recommender_amd.rerank import pack_queries
    with pytest.raises(ValueError, match="CrossEncoder with a tokenizer"):
        SearchEngine(world["meta"], world["emb"], world["blob"], cross_encoder=W.FakeCrossEncoder(), rerank="device")
    with pytest.raises(MemoryError, match="rerank_max_bytes"):
        SearchEngine(world["meta"], world["emb"], world["blob"], cross_encoder=world["ce"], rerank="device", rerank_max_bytes=1)
    dev = engine_of(world, "app", "host", "device")
    packed = pack_queries([[5, 6]], 512)
    with pytest.raises(ValueError, match="either rerank_fn or rerank_pairs"):
        dev.searcher.search_batch(world["qvecs"][:1], None, 5, 5, rerank_fn=lambda r: r, rerank_pairs=(world["ce"], packed, None))
    host = engine_of(world, "app", "host", "host")
    with pytest.raises(ValueError, match="token plane"):
        host.searcher.search_batch(world["qvecs"][:1], None, 5, 5, rerank_pairs=(world["ce"], packed, None))


def test_a_model_beyond_the_fp16_range_is_rerun_on_the_wide_kernels(world):
    """The recipe of tests/test_gpu_embed_build.py (one FFN blown up, |intermediate| ~ 1e5) on a model with a head: the
    first pass poisons its logits with NaN, the device path switches the handle once, with the warning, and answers finite
    scores -- the ones the host path gives on the same handle state."""
    from review_recommender_amd.cross_encoder import CrossEncoder
    sd = dict(world["sd"])
    key = [k for k in sd if k.endswith("encoder.layer.1.intermediate.dense.weight")][0]
    sd[key] = np.asarray(sd[key], dtype=np.float32) * np.float32(4.0e4)
    ce = CrossEncoder(sd, world["tok"])
    dev, host = engine_of(world, "app", "host", "device", ce), engine_of(world, "app", "host", "host", ce)
    args = dict(ARGS, rerank_k=20, gate_penalty=0.5)
    assert not ce.model.wide_range
    with pytest.warns(UserWarning, match="fp16 range"):
        got = dev.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
    assert ce.model.wide_range and all(np.isfinite(f["_rerank"].values).all() for f, _, _ in got)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # (the handle has switched: no second warning)
        again = dev.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
        want = host.run_search_batch(QUERIES, qvecs=world["qvecs"][:3], **args)
    same_answers(again, got)
    same_answers(got, want)
