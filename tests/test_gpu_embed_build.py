"""Product embeddings built on the GPU (review-recommender_amd/embed.py): device rows into an index
(rr_index_store_rows_dev), text -> device tokenizer -> encoder -> index against `transformers`' fixture and against the
existing host path, row shards, the written files, the engine without files, the command line."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, ROOT
from review_recommender_amd import _lib, synth
from review_recommender_amd.index import ProductIndex
from review_recommender_amd.wordpiece import WordPieceTokenizer

pytestmark = pytest.mark.gpu
F32_EMB_TOL = 1e-5          # the bar tests/test_gpu_k5.py holds the fp32 query encoder to


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_store_rows_dev_equals_the_host_upload(dtype):
    import torch
    n, dim = 20_000, 384
    rng = np.random.default_rng(1)
    rows = (rng.standard_normal((n, dim)) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)
    rows[17] = 0.0                                                   # ||x|| < eps: x / eps
    Q = synth.unit_rows(16, dim, 2)
    host = ProductIndex.from_rows(rows, normalize=True, dtype=dtype)
    want = host.dense_topk(Q, 10)
    d_rows = torch.from_numpy(rows).cuda()

    ix = ProductIndex(None, n_rows=n, dim=dim, dtype=dtype)         # contiguous, in three calls
    for a, b in ((0, 7000), (7000, 7001), (7001, n)):
        ix.store_rows_dev(d_rows[a:b], first_row=a)
    torch.cuda.synchronize()
    got = ix.dense_topk(Q, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))

    sc = ProductIndex(None, n_rows=n, dim=dim, dtype=dtype)         # scattered: source row i is row order[i] of the index
    order = rng.permutation(n)
    sc.store_rows_dev(torch.from_numpy(rows[order]).cuda(), row_ids=torch.from_numpy(order.astype(np.int64)).cuda())
    got = sc.dense_topk(Q, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    if dtype == "f32":
        a = host.download_rows()
        assert np.array_equal(bits(a), bits(ix.download_rows())) and np.array_equal(bits(a), bits(sc.download_rows()))
        assert np.array_equal(bits(a[100:300]), bits(ix.download_rows(100, 200)))
        np.testing.assert_allclose(np.linalg.norm(a[:17], axis=1), 1.0, atol=1e-6)
    else:
        with pytest.raises(ValueError, match="bf16"):
            ix.download_rows()

    # an index that has been searched with the filter scan (its bf16 plane and row-norm bounds exist): rows stored over
    # it must be the ones the next search sees
    assert ix.last_scan_info()[0] == 5
    new = (rng.standard_normal((64, dim))).astype(np.float32)
    new[:16] = Q * 5.0                                               # row 300 + i becomes query i itself
    ix.store_rows_dev(torch.from_numpy(new).cuda(), first_row=300)
    torch.cuda.synchronize()
    rows2 = rows.copy()
    rows2[300:364] = new
    want2 = ProductIndex.from_rows(rows2, normalize=True, dtype=dtype).dense_topk(Q, 10)
    got2 = ix.dense_topk(Q, 10)
    assert ix.last_scan_info()[0] == 5
    assert np.array_equal(got2[0][:, 0], 300 + np.arange(16))
    assert np.array_equal(got2[0], want2[0]) and np.array_equal(bits(got2[1]), bits(want2[1]))

    # refused: an adopted matrix, rows outside the index, ids outside the index
    mat = torch.zeros((256, 384), dtype=torch.float32, device="cuda")
    adopted = ProductIndex(None, n_rows=256, dim=384, device_ptr=mat.data_ptr(), keepalive=mat)
    with pytest.raises(ValueError, match="caller-owned"):
        adopted.store_rows_dev(d_rows[:4])
    with pytest.raises(ValueError, match="outside"):
        ix.store_rows_dev(d_rows[:4], first_row=n - 3)
    with pytest.raises(ValueError, match="row id"):
        ix.store_rows_dev(d_rows[:2], row_ids=torch.tensor([5, n], dtype=torch.int64, device="cuda"))


def fixture_world():
    """tests/golden/k5_query_encoder.npz as TEXT: piece i is "t<i>", so the text "t1017 t2003" tokenises to the fixture's
    ids (101 ... 102) on any correct WordPiece implementation."""
    fx = np.load(GOLDEN / "k5_query_encoder.npz")
    vocab = {f"t{i}": i for i in range(30_522)}
    del vocab["t0"], vocab["t100"], vocab["t101"], vocab["t102"]
    vocab.update({"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102})
    cu = fx["cu_seqlens"]
    seqs = [fx["token_ids"][cu[i]:cu[i + 1]] for i in range(len(cu) - 1)]
    assert all(s[0] == 101 and s[-1] == 102 and (s[1:-1] >= 999).all() for s in seqs)
    texts = [" ".join(f"t{t}" for t in s[1:-1]) for s in seqs]
    return fx, WordPieceTokenizer(vocab), texts


def test_text_to_index_matches_the_transformers_fixture():
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.embed import embed_texts_into
    fx, tok, texts = fixture_world()
    enc = QueryEncoder(synth.bert_state_dict(int(fx["seed"]), n_layers=12, n_labels=0, prefix=""), tok)
    ix = ProductIndex(None, n_rows=len(texts), dim=384)
    embed_texts_into(ix, texts, enc, chunk_tokens=1024)              # several chunks
    got = ix.download_rows()
    err = np.abs(got - fx["embeddings"]).max()
    print("text -> device tokenizer -> encoder -> index: max |embedding error| vs transformers", err)
    assert got.shape == fx["embeddings"].shape and err < F32_EMB_TOL


def product_world(n=3000, seed=9):
    rng = np.random.default_rng(seed)
    texts = synth.text_corpus(n, seed, mean_len=25)
    for i in 10 + rng.choice(n - 10, 12, replace=False):
        texts[i] = texts[i] + " café naïve 中文 mug"                   # the device leaves these to the host
    short = 10 + rng.choice(n - 10, 9, replace=False)
    for i in short:
        texts[i] = "tiny"                                            # dropped by the filter
    texts[5] = "  " + texts[5].replace(" ", " \r\n ", 3) + "\t"       # normalize_text has work to do
    texts[6] = (texts[6] + " ") * 40                                 # cut at 4 000 characters, 512 tokens
    n_rev, stars = synth.metadata(n, seed + 1)
    return pd.DataFrame({"sku": synth.skus(n), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})


@pytest.fixture(scope="module")
def built():
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.embed import build_product_embeddings, filter_products
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(synth.WORDS) + ["##s", "##ing", "caf", "##e", "naive", "中", "文"]
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    enc = QueryEncoder(synth.bert_state_dict(77, n_layers=12, n_labels=0, prefix="", vocab=len(words)), tok)
    products = product_world()
    index, meta, emb = build_product_embeddings(products, enc, chunk_tokens=16_384)
    _, texts = filter_products(products)
    return dict(enc=enc, products=products, index=index, meta=meta, texts=texts, rows=index.download_rows())


def test_build_equals_the_host_path_bit_for_bit(built):
    """QueryEncoder.encode (host tokenizer, host packing, rows through the host) + from_rows(normalize=True) is the only way
    the parent commit can make these rows: the packed forward does not depend on batch composition and the normalisation is
    the same kernel, so the device build must give the same bits."""
    assert len(built["texts"]) == len(built["products"]) - 9 == built["index"].n_rows
    assert sum(not t.isascii() for t in built["texts"]) >= 10
    want = ProductIndex.from_rows(built["enc"].encode(built["texts"]), normalize=True).download_rows()
    diff = np.flatnonzero((bits(want) != bits(built["rows"])).any(axis=1))
    print("rows that differ from the host path:", len(diff), "max |diff|", np.abs(want - built["rows"]).max())
    assert len(diff) == 0, diff[:10]
    assert built["meta"]["agg_text"].tolist() == [t for t in built["products"]["agg_text"] if t != "tiny"]


def test_a_model_beyond_the_fp16_range_is_redone_chunk_by_chunk(built):
    """The fp32 mode's out-of-range flag inside the pipelined builder.  With one FFN blown up (|intermediate| ~ 1e5, as
    tests/test_gpu_k5.py does for forward_ids) EVERY chunk leaves fp16's range, and when the first chunk's flag is read the
    second is already queued on the fp16-pair kernels: each chunk must be redone on its own flag, whatever the handle has
    switched to meanwhile.  No NaN may reach the index, and the rows are the ones QueryEncoder.encode gives (which runs the
    wide-range kernels from its first flag on), bit for bit."""
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.embed import embed_texts_into
    tok = built["enc"].tokenizer
    sd = synth.bert_state_dict(78, n_layers=12, n_labels=0, prefix="", vocab=len(tok.vocab))
    key = [k for k in sd if k.endswith("encoder.layer.2.intermediate.dense.weight")][0]
    sd[key] = np.asarray(sd[key], dtype=np.float32) * np.float32(4.0e4)
    texts = built["texts"][:700]
    assert sum(not t.isascii() for t in texts) >= 1
    probe = QueryEncoder(sd, tok)                                     # the condition is real: a plain pass flags
    seq = [tok.encode_pair(texts[0], None, 512)]
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()
    n0 = len(seq[0][0])
    raw = probe.model.forward_packed_dev(t(seq[0][0]), t(seq[0][1]), t(np.arange(n0)), t([0, n0]), 1, n0, 1)
    torch.cuda.synchronize()
    assert probe.model.out_of_range() and bool(torch.isnan(raw).all())

    ref = QueryEncoder(sd, tok)
    with pytest.warns(UserWarning, match="fp16 range"):
        want = ProductIndex.from_rows(ref.encode(texts), normalize=True).download_rows()
    assert np.isfinite(want).all()
    for chunk_tokens in (2048, 8192):                                # ~10 and ~3 chunks
        enc = QueryEncoder(sd, tok)
        ix = ProductIndex(None, n_rows=len(texts), dim=384)
        from review_recommender_amd.embed import _plan_chunks
        assert len(_plan_chunks([len(x.encode()) for x in texts], 512, chunk_tokens)) >= 3
        with pytest.warns(UserWarning, match="fp16 range"):
            kept = embed_texts_into(ix, texts, enc, chunk_tokens=chunk_tokens, keep_rows=True)
        got = ix.download_rows()
        bad = np.flatnonzero(~np.isfinite(got).all(axis=1))
        assert len(bad) == 0, ("rows left NaN", bad[:10], len(bad))
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(kept), bits(want))
        assert enc.model.wide_range


def test_row_shards_equal_the_halves_of_the_whole_build(built):
    from review_recommender_amd.embed import build_product_embeddings
    n = built["index"].n_rows
    cutp = n // 2 + 7
    for lo, hi in ((0, cutp), (cutp, n)):
        ix, meta, _ = build_product_embeddings(built["products"], built["enc"], rows=(lo, hi), chunk_tokens=32_768)
        assert ix.row_offset == lo and ix.n_rows == hi - lo
        assert np.array_equal(bits(ix.download_rows()), bits(built["rows"][lo:hi]))
        assert meta["sku"].tolist() == built["meta"]["sku"].tolist()[lo:hi]
    with pytest.raises(ValueError):
        build_product_embeddings(built["products"], built["enc"], rows=(5, n + 1))


def test_files_round_trip_and_the_engine_without_files(built, tmp_path):
    from review_recommender_amd import artifacts
    from review_recommender_amd.embed import build_product_embeddings
    from review_recommender_amd.engine import SearchEngine
    index, meta, emb = build_product_embeddings(built["products"], built["enc"], data_dir=tmp_path)
    on_disk = np.load(tmp_path / artifacts.EMB_FILE)
    assert on_disk.dtype == np.float32 and on_disk.shape == (len(meta), 384)
    assert np.array_equal(bits(on_disk), bits(built["rows"])) and np.array_equal(bits(emb), bits(on_disk))
    np.testing.assert_allclose(np.linalg.norm(on_disk, axis=1), 1.0, atol=1e-6)
    pq = pd.read_parquet(tmp_path / artifacts.META_FILE)
    assert list(pq.columns) == ["sku", "n_reviews", "avg_stars", "last_ts", "agg_text"] and len(pq) == len(meta)
    with open(tmp_path / artifacts.BM25_FILE, "wb") as f:
        import pickle
        pickle.dump(artifacts.build_bm25_blob(pq), f, protocol=4)          # nlp/12_product_prep.py's file, from the same table
    a = SearchEngine.from_artifacts(tmp_path, encoder=built["enc"])
    b = SearchEngine.from_products(built["products"], built["enc"])
    assert np.array_equal(bits(a.index.download_rows()), bits(b.index.download_rows()))
    for query in ("wireless cat socks", "blue insulated coffee mug", "usb cable fast charger"):
        fa, sa, da = a.run_search(query, 10, 0, 0.5, 0.3, 0.0, 0.2, 0.0, 20.0)
        fb, sb, db = b.run_search(query, 10, 0, 0.5, 0.3, 0.0, 0.2, 0.0, 20.0)
        pd.testing.assert_frame_equal(fa, fb, check_exact=True)
        assert sa == sb and da == db and len(fa) == 10
    # bf16 storage: the same rows as from_artifacts(dtype="bf16") (normalise again, then round)
    qv = a.encode("wireless cat socks")[None, :]
    a16 = SearchEngine.from_artifacts(tmp_path, encoder=built["enc"], dtype="bf16")
    b16 = SearchEngine.from_products(built["products"], built["enc"], dtype="bf16")
    ra, rb = a16.index.dense_topk(qv, 50), b16.index.dense_topk(qv, 50)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(bits(ra[1]), bits(rb[1]))


def test_bf16_index_keeps_the_fp32_rows_for_the_file(built, tmp_path):
    from review_recommender_amd.embed import build_product_embeddings
    index, meta, emb = build_product_embeddings(built["products"], built["enc"], dtype="bf16", data_dir=tmp_path, rows=(0, 400))
    assert index.dtype == "bf16" and np.array_equal(bits(emb), bits(built["rows"][:400]))
    want = ProductIndex.from_rows(built["enc"].encode(built["texts"][:400]), normalize=True, dtype="bf16")
    q = synth.unit_rows(3, 384, 4)
    ra, rb = index.dense_topk(q, 20), want.dense_topk(q, 20)
    assert np.array_equal(ra[0] - 0, rb[0]) and np.array_equal(bits(ra[1]), bits(rb[1]))


def test_command_line_writes_the_two_files(built, tmp_path):
    from test_gpu_k5 import write_model_dir
    from review_recommender_amd import artifacts
    tok = built["enc"].tokenizer
    words = sorted(tok.vocab, key=tok.vocab.get)
    write_model_dir(tmp_path / "enc", synth.bert_state_dict(77, n_layers=12, n_labels=0, prefix="", vocab=len(words)), words)
    small = built["products"].iloc[:300].rename(columns={"agg_text": "body"})
    small.to_parquet(tmp_path / "products.parquet", index=False)
    cmd = [sys.executable, "-m", "review_recommender_amd.embed", "--target", "product", "--input", str(tmp_path / "products.parquet"),
           "--text-col", "body", "--model", str(tmp_path / "enc"), "--batch", "16", "--shard-rows", "100", "--device", "0",
           "--out-dir", str(tmp_path / "out")]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "[ok] wrote" in proc.stdout
    from review_recommender_amd.embed import build_product_embeddings
    index, meta, _ = build_product_embeddings(small, built["enc"], text_col="body")
    got = np.load(tmp_path / "out" / artifacts.EMB_FILE)
    assert np.array_equal(bits(got), bits(index.download_rows()))
    pq = pd.read_parquet(tmp_path / "out" / artifacts.META_FILE)
    assert list(pq.columns) == ["sku", "n_reviews", "avg_stars", "last_ts", "agg_text"]
    assert pq["sku"].tolist() == meta["sku"].tolist() and pq["agg_text"].tolist() == meta["agg_text"].tolist()
    review = subprocess.run(cmd[:4] + ["review"] + cmd[5:], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert review.returncode != 0 and "review embeddings are not built here" in review.stderr
