#!/usr/bin/env python
"""Generates tests/golden/products_prep.json by RUNNING THE REFERENCE'S OWN nlp/10_product_prep.py (load_reviews, then
build_products) on a seeded synthetic review table.

    python tests/golden/make_products_golden.py     # needs the reference checkout; only these vectors travel

The file holds data only: "input" = the rows build_products received (after load_reviews: id / sku / text as str, stars a
float or null = NaN, ts int64 ns UTC or null = NaT), "products" = the frame it returned (avg_stars null = NaN, last_ts
null = NaT), "deduped" = its second result.  The table is small, and this script ASSERTS that it contains what the tests rely
on: a sku with more than 80 survivors, ties on (stars, ts), NaN stars and NaT, a sku whose stars are all NaN, a sku with every
row dropped, duplicates inside and across skus, texts with \\r\\n, NBSP, U+0085, U+001F, a 3-byte and a 4-byte character,
and a text of 9 and one of 10 code points after cleaning.
"""
import importlib.util
import json
import os
import pathlib
import tempfile

import numpy as np
import pandas as pd

REF = pathlib.Path(os.environ.get("RR_REFERENCE", "/root/reference"))
OUT = pathlib.Path(__file__).resolve().parent / "products_prep.json"
WORDS = ("great sturdy cheap broke mug lamp cable quiet loud soft battery screen arrived late early works "
         "fine poor love hate return again never café 中文 naïve \U0001f600 größe").split()
SPACES = ["\r\n", "\u00a0", "\u0085", "\u001f", "  ", "\t", " \n ", "\u2003", "\u3000"]


def load_reference_module(rel, name):
    spec = importlib.util.spec_from_file_location(name, REF / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_table(seed=10):
    rng = np.random.default_rng(seed)
    rows = []                                             # (sku, text, stars, ts)
    star_pool = [1.0, 2.0, 3.0, 4.0, 5.0, 4.5, np.nan]
    day = 86400 * 10 ** 9
    ts_pool = [None] + [1_600_000_000 * 10 ** 9 + int(d) * day for d in range(6)]

    def sentence(k):
        words = [WORDS[int(j)] for j in rng.integers(0, len(WORDS), k)]
        out = words[0]
        for w in words[1:]:
            out += (SPACES[int(rng.integers(0, len(SPACES)))] if rng.random() < 0.3 else " ") + w
        return out

    def add(sku, text, stars=None, ts=None):
        s = star_pool[int(rng.integers(0, len(star_pool)))] if stars is None else stars
        t = ts_pool[int(rng.integers(0, len(ts_pool)))] if ts is None else ts
        rows.append((sku, text, s, None if t == "nat" else t))

    skus = ["a10", "a9", "B1", "Z", "z", "é1", "sku-0", "sku 0", "10", "9"]
    for i in range(100):                                  # more than 80 survivors, few distinct (stars, ts): ties
        add("BIG", f"{sentence(6)} #{i}", stars=[5.0, 4.0, np.nan][i % 3], ts=[ts_pool[1], ts_pool[2], "nat"][(i // 3) % 3])
    for i in range(150):
        add(skus[int(rng.integers(0, len(skus)))], f"{sentence(int(rng.integers(3, 14)))} {i}")
    for i in range(6):                                    # a sku whose stars are all NaN (and one whose ts are all NaT)
        add("NANSTARS", f"no stars were given here {i}", stars=np.nan)
        add("NATS", f"no time was given here {i}", ts="nat")
    for t in ["  \r\n abc  \t ", "\u0085\u0085\u0085\u0085 short \u001f\u001f\u001f", "a b c d e\n\n\n"]:
        add("DROPPED", t)                                 # every row cleans to fewer than 10 code points
    add("EDGE", " abcdefghi \r\n")                        # 9 code points after cleaning: dropped
    add("EDGE", "\u00a0abcdefghij\u0085")                 # 10: kept
    add("EDGE", "中文中文 \U0001f600\U0001f600\U0001f600\U0001f600\U0001f600")      # 10 code points, 31 bytes
    add("EDGE", "ends in a wide one \U0001f600", stars=5.0)
    add("EDGE", "line one\r\nline two nbsp\u0085nel\u001fus 中 \U0001f600", stars=5.0)
    for sku in ("a9", "a10"):                             # duplicates across skus stay, inside a sku they go
        add(sku, "the very same   review text")
        add(sku, "the very same review text")
    order = rng.permutation(len(rows))                    # skus interleaved in row order
    rows = [rows[int(j)] for j in order]
    return pd.DataFrame({"id": np.arange(len(rows)), "sku": [r[0] for r in rows],
                         "ts": pd.to_datetime(pd.Series([pd.NaT if r[3] is None else pd.Timestamp(r[3], tz="UTC") for r in rows]),
                                              utc=True),
                         "stars": [r[2] for r in rows], "text": [r[1] for r in rows]})


def check_table(ref, df):
    clean = df["text"].map(ref.normalize_text)
    alive = clean.str.len() >= 10
    first = ~pd.DataFrame({"sku": df["sku"], "c": clean})[alive].duplicated()
    kept = df[alive][first]
    per = kept.groupby("sku").size()
    assert per.max() > 80, "no sku with more than 80 survivors"
    assert kept.duplicated(subset=["sku", "stars", "ts"]).any(), "no ties on (stars, ts)"
    assert kept["stars"].isna().any() and kept["ts"].isna().any(), "no NaN stars / NaT"
    assert (kept.groupby("sku")["stars"].count() == 0).any(), "no sku whose stars are all NaN"
    assert set(df["sku"]) - set(kept["sku"]), "no sku with every row dropped"
    dup = pd.DataFrame({"sku": df["sku"], "c": clean})[alive]
    assert dup.duplicated().any(), "no duplicates inside a sku"
    assert (dup.drop_duplicates().groupby("c")["sku"].nunique() > 1).any(), "no duplicates across skus"
    for piece in ("\r\n", "\u00a0", "\u0085", "\u001f"):
        assert df["text"].str.contains(piece, regex=False).any(), repr(piece)
    assert any(any(0x800 <= ord(c) < 0x10000 for c in t) for t in df["text"]), "no 3-byte character"
    assert any(any(ord(c) >= 0x10000 for c in t) for t in df["text"]), "no 4-byte character"
    assert (clean.str.len() == 9).any() and (clean.str.len() == 10).any(), "no text of 9 / 10 code points"
    assert 200 <= len(df) <= 400


def main():
    ref = load_reference_module("nlp/10_product_prep.py", "ref_product_prep_10")
    table = make_table()
    with tempfile.TemporaryDirectory() as d:
        path = pathlib.Path(d) / "reviews_merged.parquet"
        table.to_parquet(path, index=False)
        df = ref.load_reviews(path)
    assert len(df) == len(table)                          # (every crafted row passes the reference's raw-length filter)
    check_table(ref, df)
    nat = df["ts"].isna().to_numpy()
    ts_ns = df["ts"].dt.tz_localize(None).to_numpy(dtype="datetime64[ns]").view(np.int64)
    inp = {"id": df["id"].tolist(), "sku": df["sku"].tolist(), "text": df["text"].tolist(),
           "stars": [None if np.isnan(v) else float(v) for v in df["stars"]],
           "ts": [None if m else int(v) for v, m in zip(ts_ns, nat)]}
    products, deduped = ref.build_products(df.copy(), max_reviews_per_sku=80)
    assert list(products.columns) == ["sku", "n_reviews", "avg_stars", "last_ts", "agg_text"]
    lnat = products["last_ts"].isna().to_numpy()
    l_ns = products["last_ts"].dt.tz_localize(None).to_numpy(dtype="datetime64[ns]").view(np.int64)
    out = {"generator": "tests/golden/make_products_golden.py",
           "source": "reference nlp/10_product_prep.py load_reviews + build_products(max_reviews_per_sku=80)",
           "pandas": pd.__version__, "max_reviews_per_sku": 80, "input": inp, "deduped": int(deduped),
           "dtypes": {c: str(products[c].dtype) for c in products.columns},
           "products": {"sku": products["sku"].tolist(), "n_reviews": [int(v) for v in products["n_reviews"]],
                        "avg_stars": [None if np.isnan(v) else float(v) for v in products["avg_stars"]],
                        "last_ts": [None if m else int(v) for v, m in zip(l_ns, lnat)],
                        "agg_text": products["agg_text"].tolist()}}
    OUT.write_text(json.dumps(out, ensure_ascii=True, indent=0, sort_keys=True) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size:,} bytes): {len(df)} rows -> {len(products)} products, deduped {deduped}")


if __name__ == "__main__":
    main()
