"""products.model_build_products (the specification of the products builder) against a run of the reference's
nlp/10_product_prep.py (tests/golden/products_prep.json), its ordering against pandas' own sort at the edges, the clean
model without the cut against nlp/10's whitespace rule, and the command lines' argument handling.  No GPU."""
import numpy as np
import pytest

from products_cases import NAT, frame_values, load_golden


def test_model_equals_the_reference_run():
    from review_recommender_amd import products as P
    reviews, gold = load_golden()
    got, deduped = P.model_build_products(reviews, gold["max_reviews_per_sku"])
    assert deduped == gold["deduped"]
    assert list(got.columns) == list(P.COLUMNS)
    assert {c: str(got[c].dtype) for c in got.columns} == gold["dtypes"]
    assert frame_values(got) == gold["products"]
    assert max(gold["products"]["n_reviews"]) > 80                 # the cut at 80 texts is exercised
    big = gold["products"]["n_reviews"].index(max(gold["products"]["n_reviews"]))
    assert got["agg_text"][big].count(P.SEPARATOR) == 79


def test_model_keeps_fewer_texts_when_asked():
    from review_recommender_amd import products as P
    reviews, gold = load_golden()
    full, _ = P.model_build_products(reviews, 10 ** 6)
    one, _ = P.model_build_products(reviews, 1)
    for col in ("sku", "n_reviews", "last_ts"):
        assert full[col].equals(one[col])
    assert [t.split(P.SEPARATOR)[0] for t in full["agg_text"]] == one["agg_text"].tolist()
    assert [t.count(P.SEPARATOR) + 1 for t in full["agg_text"]] == gold["products"]["n_reviews"]


def test_model_order_is_pandas_sort_at_the_edges():
    """NaN strictly behind -inf, NaT strictly behind the earliest time, -0.0 == 0.0, ties by row: sort_values itself."""
    import pandas as pd
    from review_recommender_amd.products import model_order
    rng = np.random.default_rng(3)
    stars = np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, 5.0, 4.5, -1.0])[rng.integers(0, 8, 400)]
    ts = np.array([NAT, NAT + 1, -1, 0, np.iinfo(np.int64).max, 7], dtype=np.int64)[rng.integers(0, 6, 400)]
    code = rng.integers(0, 3, 400)
    df = pd.DataFrame({"sku": code, "stars": stars, "ts": pd.DatetimeIndex(ts.view("datetime64[ns]")).tz_localize("UTC")})
    assert df["ts"].isna().sum() == np.count_nonzero(ts == NAT)
    want = df.sort_values(["sku", "stars", "ts"], ascending=[True, False, False]).index.to_numpy()
    got = model_order(code, stars, ts, np.arange(400))
    assert got.tolist() == want.tolist()


def test_clean_model_without_the_cut_is_nlp10s_rule_for_every_code_point():
    from review_recommender_amd import products as P, textprep as T
    for c in range(0x110000):
        s = "ab" + chr(c) + "cd"
        got, status = T.model_clean(s, spam=False, max_chars=0)
        if 0xD800 <= c < 0xE000:                                   # no UTF-8 form: the host cleans the row
            assert status == T.NEEDS_HOST, hex(c)
        elif got != P.normalize_text(s) or status != T.SHORT:
            raise AssertionError(hex(c))
    long = " ".join(["word  x"] * 1500)                  # 10 499 code points after cleaning: no cut at 4000
    got, status = T.model_clean(long, spam=False, max_chars=0)
    assert (got, status) == (P.normalize_text(long), 0) and len(got) == 10499
    assert len(T.model_clean(long, spam=False)[0]) == T.MAX_CHARS  # nlp/11's cut is still the default


def test_prepare_columns_without_stars_and_ts():
    import pandas as pd
    from review_recommender_amd import products as P
    df = pd.DataFrame({"id": [1, 2, 3], "sku": ["b", "a", "b"], "text": ["a text of enough length", None, "another long enough text"]})
    sku, texts, stars, ts = P.prepare_columns(df)
    assert texts[1] == "" and np.isnan(stars).all() and (ts == NAT).all()
    got, deduped = P.model_build_products(df)
    assert deduped == 1 and got["sku"].tolist() == ["b"]           # sku "a" has no surviving row: no product
    assert got["n_reviews"].tolist() == [2] and np.isnan(got["avg_stars"][0]) and pd.isna(got["last_ts"][0])
    assert got["agg_text"][0] == "a text of enough length \nanother long enough text"
    with pytest.raises(ValueError, match="missing columns"):
        P.prepare_columns(df.drop(columns=["sku"]))


def test_command_line_arguments(tmp_path):
    import pandas as pd
    from review_recommender_amd import prep, products as P
    a = P.parse_args([])
    assert (a.inp, a.out, a.max_reviews_per_sku, a.device) == (P.DEF_IN, P.DEF_OUT, 80, 0)
    a = P.parse_args(["--in", "x.parquet", "--out", "y.parquet", "--max-reviews-per-sku", "7", "--device", "1"])
    assert (a.inp, a.out, a.max_reviews_per_sku, a.device) == ("x.parquet", "y.parquet", 7, 1)
    for bad in (["--max-reviews-per-sku", "0"], ["--max-reviews-per-sku", "many"], ["--frobnicate"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)
    with pytest.raises(FileNotFoundError, match="Missing input"):
        P.load_reviews(tmp_path / "absent.parquet")
    pd.DataFrame({"id": [1], "text": ["long enough text"]}).to_parquet(tmp_path / "nosku.parquet")
    with pytest.raises(ValueError, match="missing columns.*sku"):
        P.load_reviews(tmp_path / "nosku.parquet")
    pd.DataFrame({"id": [1, 2, 3], "sku": ["a", "a", "b"], "text": ["long enough text", "short", None], "extra": 0}).to_parquet(
        tmp_path / "r.parquet")
    df = P.load_reviews(tmp_path / "r.parquet")                  # the raw-length filter, and only the columns nlp/10 reads
    assert df["id"].tolist() == [1] and list(df.columns) == ["id", "sku", "text"]
    a = prep.parse_args(["--reviews", "r.parquet", "--max-reviews-per-sku", "5"])
    assert (a.reviews, a.max_reviews_per_sku, a.data_dir) == ("r.parquet", 5, "data/processed")
    assert prep.parse_args([]).reviews == ""
    with pytest.raises(SystemExit):
        prep.parse_args(["--reviews", "r.parquet", "--max-reviews-per-sku", "0"])
