"""Review embeddings built on the GPU (review-recommender_amd/embed.py: build_review_embeddings): raw review text -> device
cleaning, spam filter and dedup -> device tokenizer -> encoder -> rows, against the reference's few lines of pandas and `re`
(restated in textprep_texts.py: nlp/11_build_product_embeddings.py:99-118) and against the existing host-text path; the
written file, the ReviewIndex made without the file, the command line."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from review_recommender_amd import _lib, synth
from review_recommender_amd import textprep as T
from review_recommender_amd.index import ProductIndex
from review_recommender_amd.wordpiece import WordPieceTokenizer

import textprep_texts as X

pytestmark = pytest.mark.gpu
F32_EMB_TOL = 1e-5          # the bar tests/test_gpu_k5.py and tests/test_gpu_embed_build.py hold the fp32 encoder to
WORDS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(synth.WORDS) + ["##s", "##ing", "caf", "##e", "naive", "中", "文"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def review_world(n=1500, n_skus=40, seed=12):
    rng = np.random.default_rng(seed)
    texts = synth.text_corpus(n, seed, mean_len=25)
    sku = [f"B{int(s):09d}" for s in rng.integers(0, n_skus, n)]
    spot = iter((20 + rng.permutation(n - 20)[:400]).tolist())
    planted = {}

    def plant(kind, text, same_sku_as=None):
        i = next(spot)
        texts[i] = text
        if same_sku_as is not None:
            sku[i] = sku[same_sku_as]
        planted.setdefault(kind, []).append(i)
        return i

    for t in ("tiny", "", "   \r\n\t ", None, "中文中文中文中文中", "a b c d e"):                     # short
        plant("short", t)
    for t in ("great mug see http://a.b/c and www.d.e for more", "USE CODE mug20 at the till today", "this review is Sponsored content",
              "nice discount  code inside the box", "I received this mug for FREE and love it", "sooooooooooo good it hurts",
              "中" * 12 + " is all it says", "visit WWW.x.y or Https://z now"):                       # spam
        plant("spam", t)
    for t in ("one link http://a.b/c is fine here", "free mug, then i received this", "aAaAaAaAaAaA alternating case is fine",
              "http:// www. are not links at all"):                                                   # looks like spam, is not
        plant("clean", t)
    for _ in range(12):                                                                              # duplicates in one sku
        a = next(spot)
        b = plant("dup", texts[a], a)
        c = plant("dup", "  " + texts[a].replace(" ", " \r\n ", 2) + " ", a)                     # equal only once normalised
        assert len({a, b, c}) == 3
    for _ in range(8):                                                                               # the same text under another sku
        a = next(spot)
        i = plant("twin", texts[a])
        sku[i] = "B%09d" % ((int(sku[a][1:]) + 1) % n_skus)
    a = plant("spam", "buy now discount code inside")                                                # duplicates of a dropped row
    plant("spam", "buy now discount code inside", a)
    for t in ("café naïve 中文 mug that keeps coffee warm", "中文 文中 blue insulated mug café", "naïve café　mug socks wireless cable"):
        plant("unicode", t)
    for t in ("ΣΑΣ ΟΔΟΣ mug with a final sigma inside", "wireless ΟΔΟΣ charger cable fast"):          # the tokenizer leaves these to the host
        plant("tok_host", t)
    far = texts[next(spot)]
    for t in ("ılık çay mug keeps warm all day", "İstanbul coffee mug blue insulated", "clasſic ſponsored mug review",      # the clean stage
              far + " " * (T.WINDOW_BYTES + 10), ("wireless socks " * 300 + "\n") * 5):                                                # leaves these to the host
        plant("clean_host", t)
    plant("dup", far, planted["clean_host"][3])                                                       # a duplicate of a host-cleaned row
    plant("cut", (texts[6] + " ") * 40)                                                               # cut at 4000 characters
    stars = rng.integers(1, 6, n).astype(object)
    stars[5], stars[9] = "five", None
    ts = pd.Series(pd.Timestamp("2020-01-01", tz="UTC") + pd.to_timedelta(rng.integers(0, 10**8, n), unit="s")).astype(str)
    frame = pd.DataFrame({"sku": sku, "id": np.arange(1000, 1000 + n), "stars": stars, "ts": ts, "text": texts, "extra": 0})
    return frame, planted


def expected(frame, no_spam, no_dedup):
    """nlp/11_build_product_embeddings.py:103-118, restated: the rows that stay, in file order."""
    df = frame[["id", "sku", "ts", "stars", "text"]].copy()                                           # :103-108
    df["id"], df["sku"], df["text"] = df["id"].astype(str), df["sku"].astype(str), df["text"].fillna("").astype(str)
    df["stars"] = pd.to_numeric(df["stars"], errors="coerce")
    df["ts"] = pd.to_datetime(df["ts"], utc=True, errors="coerce")
    keep, dropped = X.ref_keep(df, no_spam, no_dedup)                                                 # :111-118
    return df.loc[keep].reset_index(drop=True), [X.ref_normalize(t) for t in df.loc[keep, "text"]], dropped


@pytest.fixture(scope="module")
def world():
    from review_recommender_amd.cross_encoder import QueryEncoder
    tok = WordPieceTokenizer({w: i for i, w in enumerate(WORDS)})
    enc = QueryEncoder(synth.bert_state_dict(77, n_layers=12, n_labels=0, prefix="", vocab=len(WORDS)), tok)
    frame, planted = review_world()
    return dict(enc=enc, frame=frame, planted=planted, built={})


def build(world, no_spam=False, no_dedup=False):
    from review_recommender_amd.embed import build_review_embeddings
    key = (no_spam, no_dedup)
    if key not in world["built"]:
        stats = {}
        table, emb, _ = build_review_embeddings(world["frame"], world["enc"], no_spam=no_spam, no_dedup=no_dedup,
                                                chunk_tokens=16_384, stats=stats)
        world["built"][key] = (table, emb, stats)
    return world["built"][key]


@pytest.mark.parametrize("no_spam,no_dedup", [(False, False), (True, False), (False, True), (True, True)])
def test_rows_are_the_ones_the_reference_keeps(world, no_spam, no_dedup):
    table, emb, stats = build(world, no_spam, no_dedup)
    want, _, (n_short, n_spam, n_dup) = expected(world["frame"], no_spam, no_dedup)
    assert list(table.columns) == ["id", "sku", "ts", "stars", "text"]
    pd.testing.assert_frame_equal(table, want, check_exact=True)
    assert emb.shape == (len(want), 384) and emb.dtype == np.float32
    assert (stats["short"], stats["spam"], stats["duplicate"]) == (n_short, n_spam, n_dup)
    assert n_short >= 6 and (n_spam >= 9) == (not no_spam) and (n_dup >= 25) == (not no_dedup)
    p, ids = world["planted"], world["frame"]["id"].astype(str)
    # both host stages had work, and exactly the planted rows: with the spam rules off no code point is left to the host
    folded = p["clean_host"][:3]
    assert sorted(stats["host_clean_docs"]) == sorted(p["clean_host"][3:] + ([] if no_spam else folded))
    kept_ids = table["id"].tolist()
    assert sorted(kept_ids[i] for i in stats["host_docs"]) == sorted(ids[i] for i in p["tok_host"])
    assert all(ids[i] in kept_ids for i in p["unicode"] + p["clean"] + p["twin"] + p["cut"])
    assert not any(ids[i] in kept_ids for i in p["short"])


def test_embeddings_equal_the_host_text_path(world):
    """The same normalised strings through embed_texts_into (host text -> the same tokenizer, encoder and store kernels).
    The bar is F32_EMB_TOL; the rows come out BITWISE equal (measured: max |diff| 0.0 on 1 458 rows; the packed forward does
    not depend on how documents are chunked), so that is what is asserted."""
    from review_recommender_amd.embed import embed_texts_into
    table, emb, _ = build(world)
    _, texts, _ = expected(world["frame"], False, False)
    ix = ProductIndex(None, n_rows=len(texts), dim=384)
    embed_texts_into(ix, texts, world["enc"], chunk_tokens=16_384)
    want = ix.download_rows()
    err = np.abs(emb - want).max()
    same = np.array_equal(bits(emb), bits(want))
    print("review rows vs embed_texts_into on the host-normalised strings: max |diff|", err, "bitwise equal:", same)
    assert err < F32_EMB_TOL and same
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-6)
    assert sum(not t.isascii() for t in texts) >= 5 and max(len(t) for t in texts) == 4000


def test_file_round_trip_and_the_index_without_the_file(world, tmp_path, hip):
    import torch
    from review_recommender_amd import artifacts
    from review_recommender_amd.embed import build_review_embeddings
    from review_recommender_amd.reviews import ReviewIndex
    skus = sorted(set(world["frame"]["sku"]))[3:] + ["B999999999"]             # a few reviews belong to unknown skus
    table, emb, ri = build_review_embeddings(world["frame"], world["enc"], chunk_tokens=16_384, data_dir=tmp_path, product_skus=skus)
    first = build(world)
    pd.testing.assert_frame_equal(table, first[0], check_exact=True)
    assert np.array_equal(bits(emb), bits(first[1]))
    raw = pd.read_parquet(tmp_path / artifacts.REVIEWS_FILE)
    assert list(raw.columns) == ["id", "sku", "ts", "stars", "text", "embedding"]
    got_table, got_emb = artifacts.load_reviews(tmp_path)
    pd.testing.assert_frame_equal(got_table, table, check_exact=True)
    assert got_emb.dtype == np.float32 and np.array_equal(bits(got_emb), bits(emb))

    other = ReviewIndex(got_table, got_emb, skus)                              # the existing constructor, from the file
    assert np.array_equal(ri.indptr, other.indptr) and np.array_equal(ri.ids, other.ids) and ri.texts == other.texts
    assert np.array_equal(ri.stars, other.stars, equal_nan=True)
    B, pool = 7, len(skus)
    q = torch.from_numpy(synth.unit_rows(B, 384, 5)).cuda()
    rows = torch.from_numpy(np.tile(np.arange(pool, dtype=np.int64), (B, 1))).cuda()

    def best(index, max_rows):
        score = torch.empty((B, pool), dtype=torch.float32, device="cuda")
        rid = torch.empty((B, pool), dtype=torch.int32, device="cuda")
        _lib.check(hip.rr_reviews_best_cut_dev(index.handle, C.c_void_p(q.data_ptr()), B, C.c_void_p(rows.data_ptr()), pool, 0, max_rows,
                                               C.c_void_p(score.data_ptr()), C.c_void_p(rid.data_ptr()), None), "rr_reviews_best_cut_dev")
        torch.cuda.synchronize()
        return score.cpu().numpy(), rid.cpu().numpy()

    for max_rows in (300000, 200):
        a, b = best(ri, max_rows), best(other, max_rows)
        assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
        assert (a[1][:, :-1] >= 0).sum() > B * (pool - 1) // 2 and (a[1][:, -1] == -1).all()
    ri.close()
    other.close()


def test_refusals(world):
    from review_recommender_amd.embed import build_review_embeddings
    frame = world["frame"]
    with pytest.raises(ValueError, match=r"missing \['id', 'text'\]"):
        build_review_embeddings(frame.drop(columns=["id", "text"]), world["enc"])
    with pytest.raises(ValueError, match=r"missing \['stars', 'ts'\]"):
        build_review_embeddings(frame.drop(columns=["ts", "stars"]), world["enc"])
    with pytest.raises(ValueError, match="(?i)split.*by sku"):
        build_review_embeddings(frame, world["enc"], max_text_bytes=10_000)
    only_short = frame.iloc[world["planted"]["short"]]
    with pytest.raises(RuntimeError, match="No reviews left after filtering."):
        build_review_embeddings(only_short, world["enc"])
    with pytest.raises(RuntimeError, match="No reviews left after filtering."):
        build_review_embeddings(frame.iloc[:0], world["enc"])


def test_command_line(world, tmp_path):
    from test_gpu_k5 import write_model_dir
    from review_recommender_amd import artifacts
    from review_recommender_amd.embed import build_review_embeddings
    write_model_dir(tmp_path / "enc", synth.bert_state_dict(77, n_layers=12, n_labels=0, prefix="", vocab=len(WORDS)), WORDS)
    small = world["frame"].iloc[:400].assign(stars=lambda d: d["stars"].astype(str))      # one type per column for the file
    small.to_parquet(tmp_path / "reviews.parquet", index=False)
    base = [sys.executable, "-m", "review_recommender_amd.embed", "--target", "review", "--input", str(tmp_path / "reviews.parquet"),
            "--model", str(tmp_path / "enc"), "--batch", "16", "--shard-rows", "100", "--device", "0"]
    for flags in ([], ["--no-spam", "--no-dedup"]):
        out = tmp_path / ("out" + str(len(flags)))
        proc = subprocess.run(base + ["--out-dir", str(out)] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert proc.returncode == 0, proc.stdout + proc.stderr
        table, emb, _ = build_review_embeddings(small, world["enc"], no_spam=bool(flags), no_dedup=bool(flags))
        assert f"[ok] wrote {out}/{artifacts.REVIEWS_FILE} total rows={len(table):,}" in proc.stdout
        assert ("[review] spam filtered" in proc.stdout) == (not flags) and ("[review] dedup removed" in proc.stdout) == (not flags)
        got_table, got_emb = artifacts.load_reviews(out)
        pd.testing.assert_frame_equal(got_table, table, check_exact=True)
        assert np.array_equal(bits(got_emb), bits(emb))
    resume = subprocess.run(base + ["--out-dir", str(tmp_path / "r"), "--resume"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert resume.returncode == 2 and "--resume is not supported" in resume.stderr and "truncates" in resume.stderr
    assert not (tmp_path / "r").exists()
    small.drop(columns=["id", "text"]).to_parquet(tmp_path / "products.parquet", index=False)
    wrong = subprocess.run(base[:6] + [str(tmp_path / "products.parquet")] + base[7:], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert wrong.returncode != 0 and "Traceback" not in wrong.stderr
    assert "missing ['id', 'text']" in wrong.stderr and "review embeddings are not built here" in wrong.stderr
