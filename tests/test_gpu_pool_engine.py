"""`QueryEncoder(pooling="mean")` from text to search results: `encode` against `transformers`' mean-pooled rows
(tests/golden/k5_mean_pooling.npz, whose ids are words of the test vocabulary), the device product-embedding builder, the
query vectors made on the device, and `search` over the mean-pooled index against the numpy oracle fed with float64 mean
vectors of the float64 encoder oracle.  A CLS encoder on the same weights shows that the test sees the mode."""
import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN
from oracle import cross_encoder as OC
from oracle.bm25 import BM25OkapiOracle
from oracle.pipeline import run_search_oracle
from parity import assert_ranking_matches
from pool_model import bits
from review_recommender_amd import synth

pytestmark = pytest.mark.gpu
N = 2000                                         # products (the float64 oracle below costs ~2 ms each on the host)
F32_EMB_TOL = 1e-5                               # the project's embedding bar (tests/test_gpu_k5.py)
WEIGHTS = dict(w_dense=0.55, w_bm25=0.25, w_rerank=0.0, w_prior=0.1, w_best=0.1, prior_C=20.0)
QUERIES = ["yellow cat socks", "wireless noise cancelling headphones", "insulated travel mug coffee", "", "fast usb charger cable",
           "mechanical gaming keyboard rgb backlight", "dog", "soft cotton shirt graphic print design pattern blue"]


@pytest.fixture(scope="module")
def world():
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    fx = np.load(GOLDEN / "k5_mean_pooling.npz")
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(synth.WORDS)           # make_k5_pooling_golden.py's vocabulary
    assert len(words) == int(fx["vocab"])
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    sd = synth.bert_state_dict(int(fx["h384_seed"]), n_layers=int(fx["n_layers"]), n_labels=0, prefix="", vocab=len(words))
    enc = QueryEncoder(sd, tok, pooling="mean")
    texts = synth.text_corpus(N, 3, mean_len=20)
    n_rev, stars = synth.metadata(N, 2)
    products = pd.DataFrame({"sku": synth.skus(N), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})
    return dict(fx=fx, words=words, tok=tok, sd=sd, enc=enc, products=products, texts=texts)


def oracle_mean64(sd, tok, texts, n_layers):
    """float64 mean over the tokens of the float64 encoder oracle, l2-normalised (float64)."""
    sd = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}      # (the same values: numpy would promote them per call)
    rows = []
    for t in texts:
        ids, typ = tok.encode_pair(t, None, 512)
        rows.append(OC.bert_hidden(sd, np.asarray(ids), np.asarray(typ), n_layers, prefix="", dtype=np.float64).mean(axis=0))
    m = np.stack(rows)
    return m / np.maximum(np.linalg.norm(m, axis=1, keepdims=True), 1e-12)


def test_encode_matches_the_transformers_fixture_and_cls_does_not(world):
    from review_recommender_amd.cross_encoder import OUT_CLS, OUT_MEAN, QueryEncoder
    fx, enc, words, tok = world["fx"], world["enc"], world["words"], world["tok"]
    assert enc.pooling == "mean" and enc.out_mode == OUT_MEAN
    cu = fx["cu_seqlens"]
    seqs = [fx["token_ids"][cu[i]:cu[i + 1]] for i in range(len(cu) - 1)]
    text_rows = [i for i, s in enumerate(seqs) if len(s) >= 2]                  # ([CLS] alone is no text's tokenisation)
    texts = [" ".join(words[t] for t in seqs[i][1:-1]) for i in text_rows]
    for i, t in zip(text_rows, texts):
        assert tok.encode_pair(t, None, 512)[0].tolist() == seqs[i].tolist()
    emb = enc.encode(texts, normalize_embeddings=True)
    err = np.abs(emb - fx["h384_embeddings"][text_rows]).max()
    print("encode(texts, normalize_embeddings=True) vs transformers' mean pooling: max |error|", err)
    assert emb.dtype == np.float32 and emb.shape == (len(texts), 384) and err < F32_EMB_TOL
    ids = enc.encode_ids([(s, np.zeros(len(s), dtype=np.int32)) for s in seqs], normalize_embeddings=True)
    assert np.abs(ids - fx["h384_embeddings"]).max() < F32_EMB_TOL
    assert np.array_equal(bits(enc.encode(texts[3], normalize_embeddings=True)), bits(emb[3]))       # a str: one row
    # the same weights with CLS pooling: other vectors (the default, as before)
    cls = QueryEncoder(world["sd"], tok)
    assert cls.pooling == "cls" and cls.out_mode == OUT_CLS
    other = cls.encode(texts, normalize_embeddings=True)
    print("CLS rows of the same weights: max |difference|", np.abs(other - emb).max(axis=1).min())
    assert np.abs(other[1:] - emb[1:]).max(axis=1).min() > 1e-2                # (every text of more than [CLS] [SEP])
    with pytest.raises(ValueError, match="pooling must be one of"):
        QueryEncoder(world["sd"], tok, pooling="max")


def test_the_device_builder_stores_the_rows_encode_returns(world):
    """tests/test_gpu_embed_build.py's comparison: QueryEncoder.encode (host tokenizer, rows through the host) +
    from_rows(normalize=True) against the rows the device builder left in its index, bit for bit."""
    from review_recommender_amd.embed import build_product_embeddings, filter_products
    from review_recommender_amd.index import ProductIndex
    enc, products = world["enc"], world["products"]
    index, meta, _ = build_product_embeddings(products, enc, chunk_tokens=16_384)          # several chunks
    _, texts = filter_products(products)
    assert index.n_rows == len(texts) == len(meta) == N
    want = ProductIndex.from_rows(enc.encode(texts), normalize=True).download_rows()
    got = index.download_rows()
    diff = np.flatnonzero((bits(want) != bits(got)).any(axis=1))
    print("rows that differ from the host path:", len(diff), "max |diff|", np.abs(want - got).max())
    assert len(diff) == 0, diff[:10]
    sample = np.arange(0, N, 97)
    v64 = oracle_mean64(world["sd"], world["tok"], [texts[i] for i in sample], 2)
    assert np.abs(got[sample] - v64).max() < F32_EMB_TOL


@pytest.fixture(scope="module")
def engines(world):
    from review_recommender_amd.engine import SearchEngine
    host = SearchEngine.from_products(world["products"], world["enc"], query_vectors="host")
    dev = SearchEngine.from_products(world["products"], world["enc"], query_text="device", query_vectors="device")
    assert len(host.meta) == len(dev.meta) == N
    return host, dev


def test_device_query_vectors_equal_host_bitwise(world, engines, monkeypatch):
    host, dev = engines
    enc = world["enc"]
    assert dev.query_vectors == "device" and host.query_vectors == "host" and dev._query_text.encoder is enc
    args = (10, 0, *WEIGHTS.values(), False, 0, 8, 0.5)
    want = host.run_search_batch(QUERIES, *args)
    encoded = []
    inner = enc.encode
    monkeypatch.setattr(enc, "encode", lambda s, **k: (encoded.append(list(s)), inner(s, **k))[1])
    got = dev.run_search_batch(QUERIES, *args)
    assert encoded == []                                       # every query vector was made on the device
    assert len(got) == len(want) == len(QUERIES)
    for (gf, gs, gd), (wf, ws, wd) in zip(got, want):
        pd.testing.assert_frame_equal(gf, wf, check_exact=True)
        for c in gf.columns:
            if gf[c].values.dtype.kind == "f":
                assert gf[c].values.tobytes() == wf[c].values.tobytes(), c
        assert gs == ws and gd == wd
    assert all(len(f) == 10 for f, _, _ in want) and any(f["_bm25"].abs().max() > 0 for f, _, _ in want)


def test_search_returns_the_skus_of_the_oracle_on_float64_mean_vectors(world, engines):
    host, _ = engines
    meta, sd, tok = host.meta, world["sd"], world["tok"]
    texts = meta["agg_text"].tolist()
    V = oracle_mean64(sd, tok, texts, 2).astype(np.float32)
    corpus = [t.split() for t in texts]
    bm25 = BM25OkapiOracle(corpus)
    for query in QUERIES[:3]:
        got, _, _ = host.search(query, k=10, alpha=0.5)
        qvec = oracle_mean64(sd, tok, [query], 2)[0].astype(np.float32)
        want, _, _, cand = run_search_oracle(query=query, qvec=qvec, meta=meta, V=V, bm25=bm25, bm25_skus=meta["sku"].tolist(), k=10,
                                             rerank_k=0, w_dense=0.5, w_bm25=0.5, w_rerank=0.0, w_prior=0.0, w_best=0.0, prior_C=20.0,
                                             min_reviews=8, gate_penalty=1.0)
        print(query, "max |_final - oracle|", np.abs(got["_final"].values - want["_final"].values).max())
        # (two scores each within the 1e-5 bar may swap: per tie band, as tests/test_gpu_k5.py compares its end-to-end search)
        assert_ranking_matches(got["sku"].tolist(), want["sku"].tolist(), want["_final"].values, 2 * F32_EMB_TOL,
                               pool_ids=cand["sku"].tolist(), pool_final=cand["_final"].values)
        assert np.allclose(got["_final"].values, want["_final"].values, atol=F32_EMB_TOL, rtol=0)


def test_a_model_directory_that_says_mean_builds_mean_pooled_vectors_from_the_command_line(world, tmp_path):
    """`python -m review_recommender_amd.embed --target product --model DIR` on a directory whose 1_Pooling/config.json says
    pooling_mode_mean_tokens: the vectors written are the mean encoder's (the device builder's bits), `--pooling cls` over the
    same directory writes the CLS encoder's, and a directory that says max is refused by name before anything is built --
    unless the caller names a pooling."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    from review_recommender_amd import artifacts, embed
    from review_recommender_amd.cross_encoder import QueryEncoder
    from test_gpu_k5 import write_model_dir

    def pooling_file(d, mode):
        (d / "1_Pooling").mkdir(exist_ok=True)
        cfg = {"word_embedding_dimension": 384, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": False,
               "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}
        cfg[mode] = True
        (d / "1_Pooling" / "config.json").write_text(json.dumps(cfg))

    model = tmp_path / "enc"
    write_model_dir(model, world["sd"], world["words"])
    pooling_file(model, "pooling_mode_mean_tokens")
    loaded = QueryEncoder.from_pretrained_dir(model)
    assert loaded.pooling == "mean" and QueryEncoder.from_pretrained_dir(model, pooling="cls").pooling == "cls"
    small = world["products"].iloc[:200]
    small.to_parquet(tmp_path / "products.parquet", index=False)
    argv = ["--target", "product", "--input", str(tmp_path / "products.parquet"), "--batch", "16", "--device", "0"]
    # one real process for the default (--pooling auto = the directory's); the override and the refusal through main() here
    proc = subprocess.run([sys.executable, "-m", "review_recommender_amd.embed"] + argv + ["--model", str(model), "--out-dir", str(tmp_path / "out")],
                          cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "[ok] wrote" in proc.stdout, proc.stdout + proc.stderr
    assert embed.main(argv + ["--model", str(model), "--out-dir", str(tmp_path / "out_cls"), "--pooling", "cls"]) == 0
    for out, enc in (("out", world["enc"]), ("out_cls", QueryEncoder(world["sd"], world["tok"]))):
        index, _, _ = embed.build_product_embeddings(small, enc)
        assert np.array_equal(bits(np.load(tmp_path / out / artifacts.EMB_FILE)), bits(index.download_rows())), out
    assert not np.array_equal(np.load(tmp_path / "out" / artifacts.EMB_FILE), np.load(tmp_path / "out_cls" / artifacts.EMB_FILE))
    bad = tmp_path / "enc_max"
    write_model_dir(bad, world["sd"], world["words"])
    pooling_file(bad, "pooling_mode_max_tokens")
    with pytest.raises(ValueError, match="pooling_mode_max_tokens"):
        embed.main(argv + ["--model", str(bad), "--out-dir", str(tmp_path / "never")])
    assert not (tmp_path / "never").exists()
    assert embed.main(argv + ["--model", str(bad), "--out-dir", str(tmp_path / "forced"), "--pooling", "mean"]) == 0       # named: served
    assert np.array_equal(bits(np.load(tmp_path / "forced" / artifacts.EMB_FILE)), bits(np.load(tmp_path / "out" / artifacts.EMB_FILE)))
