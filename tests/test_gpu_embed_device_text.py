"""Product embeddings and the reranker's token plane built from agg_text that never leaves the device
(embed.build_product_embeddings_device, RerankText.from_device over the head kernels of csrc/rr_textprep.hip) against the
builders that take a column of Python strings (build_product_embeddings, RerankText.from_texts): the same rows bit for bit,
the same tables, the same files, the same planes."""
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from review_recommender_amd import synth
from review_recommender_amd import textprep as T
from review_recommender_amd.wordpiece import WordPieceTokenizer
from test_gpu_embed_build import bits

pytestmark = pytest.mark.gpu
CHUNK_TOKENS = 16_384
WORDS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(synth.WORDS) + ["##s", "##ing", "caf", "##e", "naive", "中", "文"]
# hand-made products: (row they are inserted at, sku, bytes).  The builder of products.parquet never makes a product of fewer
# than 10 characters, Unicode spaces (it collapses them) or malformed bytes, so these are given as device text directly.
BAD_SKU = "ZZ-MALFORMED"
HAND_MADE = [
    (0, "ZZ-TINY", b"tiny"),
    (3, "ZZ-SPACES", "wireless\u2003headphones\u00a0bluetooth\u3000 caf\u00e9 \u4e2d\u6587 mug \u2028 noise\u0085cancelling \u205f".encode()),
    (60, BAD_SKU, b"ab \xed\xa0\x80 c"),                                       # a lone surrogate: cleaned on the host, then too short
    (61, "ZZ-BLANK", " \u2003 \n\u3000".encode()),
    (150, "ZZ-LONG-SPACES", ("blue\u2003\u2003mug \u3000caf\u00e9 \n" * 1500).encode()),
    (10 ** 6, "ZZ-NINE", "\u4e2d\u6587 na\u00efv \u00e9".encode()),                # 9 code points: dropped
    (10 ** 6, "ZZ-TEN", "\u4e2d\u6587 na\u00efve \u00e9".encode()),                # 10: kept, the last row
]


def make_reviews(n_skus: int, seed: int):
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(n_skus):
        long = s % 40 == 7
        k = 80 if long else int(rng.integers(1, 5))
        texts = synth.text_corpus(k, 1000 * seed + s, mean_len=70 if long else 25)
        if s % 9 == 0:
            texts[0] += " café naïve 中文 mug"
        for j, t in enumerate(texts):
            rows.append({"id": f"r{s}-{j}", "sku": synth.skus(1, s)[0], "ts": pd.Timestamp("2021-03-01", tz="UTC") + pd.Timedelta(days=int(rng.integers(0, 900))),
                         "stars": float(rng.integers(1, 6)), "text": t})
    return pd.DataFrame(rows)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """About 200 products through build_products(keep_device=True), the hand-made ones spliced into the device text; the
    host build of the same table, once."""
    import torch
    from review_recommender_amd import products as P
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.embed import build_product_embeddings
    tok = WordPieceTokenizer({w: i for i, w in enumerate(WORDS)})
    enc = QueryEncoder(synth.bert_state_dict(77, n_layers=12, n_labels=0, prefix="", vocab=len(WORDS)), tok)
    base, _, text = P.build_products(make_reviews(200, 5), 80, keep_device=True)
    off = text.d_off.cpu().numpy()
    blob = text.d_text[:text.text_bytes].cpu().numpy().tobytes()
    docs = [blob[off[i]:off[i + 1]] for i in range(text.n)]
    rows = base.to_dict("records")
    for at, sku, raw in HAND_MADE:
        at = min(at, len(docs))
        docs.insert(at, raw)
        rows.insert(at, {"sku": sku, "n_reviews": 1, "avg_stars": np.nan, "last_ts": pd.NaT})
    products = pd.DataFrame(rows)[["sku", "n_reviews", "avg_stars", "last_ts"]]
    products["last_ts"] = pd.to_datetime(products["last_ts"], utc=True)
    new_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=new_off[1:])
    d_text = torch.from_numpy(np.frombuffer(b"".join(docs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    dtext = P.DeviceProductText(products["sku"].tolist(), d_text, torch.from_numpy(new_off).cuda(), len(docs), int(new_off[-1]), 0)
    full = dtext.with_text(products)
    host_dir = tmp_path_factory.mktemp("host")
    index, meta, emb = build_product_embeddings(full, enc, chunk_tokens=CHUNK_TOKENS, data_dir=host_dir)
    return dict(enc=enc, tok=tok, products=products, text=dtext, full=full, docs=docs, host_dir=host_dir, meta=meta, emb=emb,
                rows=index.download_rows())


def test_the_world_holds_what_the_kernels_must_meet(world):
    docs, window = world["docs"], T.WINDOW_BYTES
    assert 190 <= len(docs) <= 230
    assert sum(len(d) > window for d in docs) >= 5                       # rr_tp_clean would hand these to the host
    assert sum(any(b >= 0x80 for b in d) for d in docs) >= 20
    assert sum(any(ord(c) in T.WHITESPACE and ord(c) > 0x80 for c in d.decode("utf-8", "surrogatepass")) for d in docs) >= 3
    statuses = [T.model_head(d, 4000, True, 10)[1] for d in docs]
    assert statuses.count(T.SHORT) == 3 and statuses.count(T.NEEDS_HOST) == 1
    assert sum(len(d.decode("utf-8", "surrogatepass")) > 4000 for d in docs) >= 5    # the cut at 4000 has work to do


def test_device_text_build_equals_the_host_build(world, tmp_path):
    from review_recommender_amd import artifacts
    from review_recommender_amd.embed import MIN_TEXT_LEN, build_product_embeddings_device, normalize_text
    stats = {}
    index, meta, emb, kept = build_product_embeddings_device(world["products"], world["text"], world["enc"], chunk_tokens=CHUNK_TOKENS,
                                                             data_dir=tmp_path, stats=stats)
    want_kept = [i for i, t in enumerate(world["full"]["agg_text"]) if len(normalize_text(t)) >= MIN_TEXT_LEN]
    assert kept.tolist() == want_kept and len(kept) == len(world["docs"]) - 4
    got = index.download_rows()
    diff = np.flatnonzero((bits(got) != bits(world["rows"])).any(axis=1))
    assert got.shape == world["rows"].shape and len(diff) == 0, diff[:10]
    pd.testing.assert_frame_equal(meta, world["meta"], check_exact=True)
    # no quiet fall-back: only the crafted malformed document was cleaned on the host, none was handed back for its length
    assert stats["host_clean_docs"] == [world["products"]["sku"].tolist().index(BAD_SKU)]
    assert np.array_equal(bits(emb), bits(world["emb"]))
    a, b = np.load(tmp_path / artifacts.EMB_FILE), np.load(world["host_dir"] / artifacts.EMB_FILE)
    assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    assert (tmp_path / artifacts.EMB_FILE).read_bytes() == (world["host_dir"] / artifacts.EMB_FILE).read_bytes()
    pd.testing.assert_frame_equal(pd.read_parquet(tmp_path / artifacts.META_FILE), pd.read_parquet(world["host_dir"] / artifacts.META_FILE),
                                  check_exact=True)

    # without files: no agg_text is fetched; small head blocks give the same rows
    stats = {}
    index2, meta2, emb2, kept2 = build_product_embeddings_device(world["products"], world["text"], world["enc"],
                                                                 chunk_tokens=CHUNK_TOKENS, stats=stats, head_bytes=20_000)
    assert emb2 is None and kept2.tolist() == want_kept and "agg_text" not in meta2.columns
    pd.testing.assert_frame_equal(meta2, world["meta"].drop(columns=["agg_text"]), check_exact=True)
    assert np.array_equal(bits(index2.download_rows()), bits(world["rows"]))
    assert stats["seconds"]["write_heads"] > 0 and stats["host_clean_docs"] == [world["products"]["sku"].tolist().index(BAD_SKU)]


def test_row_shards_equal_the_halves_of_the_whole(world):
    from review_recommender_amd.embed import build_product_embeddings_device
    n = len(world["rows"])
    cut = n // 2 + 3
    for lo, hi in ((0, cut), (cut, n)):
        ix, meta, _, kept = build_product_embeddings_device(world["products"], world["text"], world["enc"], rows=(lo, hi),
                                                            chunk_tokens=CHUNK_TOKENS)
        assert ix.row_offset == lo and ix.n_rows == hi - lo == len(kept)
        assert np.array_equal(bits(ix.download_rows()), bits(world["rows"][lo:hi]))
        assert meta["sku"].tolist() == world["meta"]["sku"].tolist()[lo:hi]
    with pytest.raises(ValueError):
        build_product_embeddings_device(world["products"], world["text"], world["enc"], rows=(5, n + 1))
    with pytest.raises(ValueError, match="products for the text"):
        build_product_embeddings_device(world["products"].iloc[:-1], world["text"], world["enc"])


def test_when_no_product_survives(world):
    import torch
    from review_recommender_amd import products as P
    from review_recommender_amd.embed import build_product_embeddings_device
    raw = b"tiny" + " \u3000 ".encode()
    text = P.DeviceProductText(["a", "b"], torch.from_numpy(np.frombuffer(raw + b"\0" * 16, dtype=np.uint8).copy()).cuda(),
                               torch.tensor([0, 4, len(raw)], dtype=torch.int64).cuda(), 2, len(raw), 0)
    with pytest.raises(RuntimeError, match="No products left after filtering."):
        build_product_embeddings_device(pd.DataFrame({"sku": ["a", "b"]}), text, world["enc"])


def test_a_kept_document_cleaned_on_the_host_lands_in_its_slot(world):
    """The host builder cannot take a lone surrogate at all (str.encode refuses it), so this row is held to the encoder's own
    answer for the cleaned string."""
    import torch
    from review_recommender_amd import products as P
    from review_recommender_amd.embed import build_product_embeddings_device, normalize_text
    from review_recommender_amd.index import ProductIndex
    docs = [b"blue mug coffee insulated", b"  wireless cat \n socks \xed\xa0\x80 blue\tmug ", "café 中文 travel mug".encode()]
    off = np.zeros(4, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    text = P.DeviceProductText(["a", "b", "c"], torch.from_numpy(np.frombuffer(b"".join(docs) + b"\0" * 16, dtype=np.uint8).copy()).cuda(),
                               torch.from_numpy(off).cuda(), 3, int(off[-1]), 0)
    stats = {}
    index, meta, _, kept = build_product_embeddings_device(pd.DataFrame({"sku": ["a", "b", "c"]}), text, world["enc"], stats=stats)
    assert kept.tolist() == [0, 1, 2] and stats["host_clean_docs"] == [1] and meta["sku"].tolist() == ["a", "b", "c"]
    cleaned = [normalize_text(d.decode("utf-8", "surrogatepass")) for d in docs]
    want = ProductIndex.from_rows(world["enc"].encode(cleaned), normalize=True).download_rows()
    assert np.array_equal(bits(index.download_rows()), bits(want))


@pytest.mark.parametrize("with_rows", [False, True])
def test_token_plane_from_device_equals_from_texts(world, with_rows):
    from review_recommender_amd.rerank import RerankText
    agg = world["full"]["agg_text"].tolist()
    rows = None
    if with_rows:
        rows = np.r_[np.arange(len(agg) - 1, 40, -3), [60, 61, 60]].astype(np.int64)         # permuted, repeated, the malformed one
    texts = agg if rows is None else [agg[int(i)] for i in rows]
    want = RerankText.from_texts(texts, world["tok"], 128, chunk_docs=64)
    got = RerankText.from_device(world["text"], world["tok"], 128, rows=rows, chunk_docs=64)
    assert got.n == want.n == len(texts) and got.n_tokens == want.n_tokens and got.max_length == want.max_length
    assert np.array_equal(got.d_off.cpu().numpy(), want.d_off.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(got.tokens(), want.tokens()))
    assert got.host_docs == want.host_docs and len(want.host_docs) >= 1
    assert (got.cls_id, got.sep_id, got.vocab_size, got.row_offset) == (want.cls_id, want.sep_id, want.vocab_size, want.row_offset)
    small = RerankText.from_device(world["text"], world["tok"], 128, rows=rows, chunk_docs=64, max_chars=50)
    cut = RerankText.from_texts(texts, world["tok"], 128, chunk_docs=64, max_chars=50)
    assert all(np.array_equal(a, b) for a, b in zip(small.tokens(), cut.tokens())) and small.host_docs == cut.host_docs
    for p in (want, got, small, cut):
        p.close()


def test_command_line_from_reviews_equals_the_two_step_route(world, tmp_path):
    from test_gpu_k5 import write_model_dir
    from review_recommender_amd import artifacts, embed, products as P
    from review_recommender_amd.cross_encoder import QueryEncoder
    write_model_dir(tmp_path / "enc", synth.bert_state_dict(77, n_layers=12, n_labels=0, prefix="", vocab=len(WORDS)), WORDS)
    make_reviews(60, 6).to_parquet(tmp_path / "reviews.parquet", index=False)
    cmd = [sys.executable, "-m", "review_recommender_amd.embed", "--target", "product", "--reviews", str(tmp_path / "reviews.parquet"),
           "--model", str(tmp_path / "enc"), "--batch", "16", "--device", "0", "--out-dir", str(tmp_path / "out")]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "[ok] wrote" in proc.stdout
    # the two-step route: products.parquet on the way, then the builder that reads it
    table, _ = P.build_products(P.load_reviews(tmp_path / "reviews.parquet"), 80)
    table.to_parquet(tmp_path / "products.parquet", index=False)
    enc = QueryEncoder.from_pretrained_dir(str(tmp_path / "enc"), device=0, precision="fp32")
    embed.build_product_embeddings(pd.read_parquet(tmp_path / "products.parquet"), enc, chunk_tokens=16 * 512, data_dir=tmp_path / "two")
    a, b = np.load(tmp_path / "out" / artifacts.EMB_FILE), np.load(tmp_path / "two" / artifacts.EMB_FILE)
    assert a.shape == b.shape == (60, 384) and np.array_equal(bits(a), bits(b))
    pd.testing.assert_frame_equal(pd.read_parquet(tmp_path / "out" / artifacts.META_FILE), pd.read_parquet(tmp_path / "two" / artifacts.META_FILE),
                                  check_exact=True)
    for argv in (cmd[3:] + ["--input", "x.parquet"], ["--target", "review", "--reviews", "r.parquet", "--model", "m"]):
        with pytest.raises(SystemExit) as e:
            embed.parse_args(argv)
        assert e.value.code == 2
