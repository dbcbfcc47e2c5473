"""What the products tests share: the fixture of tests/golden/products_prep.json as frames, and the crafted order cases."""
import json
import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "products_prep.json"
NAT = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
SPECIAL_STARS = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, 1.0, 2.0, 3.0, 4.0, 5.0, 4.5])
FINITE_STARS = np.array([-0.0, 0.0, np.nan, 1.0, 2.0, 3.0, 4.0, 5.0, 4.5])
SPECIAL_TS = np.array([NAT, NAT + 1, -1, 0, I64_MAX] + [1_600_000_000_000_000_000 + s * 10 ** 9 for s in range(50)], dtype=np.int64)
TILE_SEGMENTS = (0, 1, 79, 80, 81, 255, 256, 257, 4095, 4096, 4097)      # 4096 = the sort's tile


def load_golden():
    """(reviews frame as nlp/10's load_reviews returns it, the fixture's dict)."""
    import pandas as pd
    d = json.loads(GOLDEN.read_text())
    i = d["input"]
    ts = pd.to_datetime(pd.Series([pd.NaT if v is None else pd.Timestamp(v, tz="UTC") for v in i["ts"]]), utc=True)
    reviews = pd.DataFrame({"id": i["id"], "sku": i["sku"], "ts": ts, "stars": [np.nan if v is None else v for v in i["stars"]],
                            "text": i["text"]})
    return reviews, d


def frame_values(products):
    """A products frame as plain lists, NaN -> None, last_ts -> int64 ns with NaT -> None: what the fixture stores."""
    ts = products["last_ts"].dt.tz_localize(None).to_numpy(dtype="datetime64[ns]").view(np.int64)
    out = {"sku": products["sku"].tolist(), "n_reviews": [int(v) for v in products["n_reviews"]],
           "avg_stars": [None if np.isnan(v) else float(v) for v in products["avg_stars"]],
           "last_ts": [None if v == NAT else int(v) for v in ts]}
    if "agg_text" in products.columns:
        out["agg_text"] = products["agg_text"].tolist()
    return out


def order_case(seg_lens, seed, stars_pool=SPECIAL_STARS, dropped=0.1):
    """Rows of len(seg_lens) skus, sku k with seg_lens[k] survivors, interleaved in row order, plus `dropped` (a share) rows
    that did not survive -> (status int32, group int32, stars float64, ts int64).  stars_pool=None: arbitrary POSITIVE
    doubles over many binades (a sum of one sign has condition number 1, so n roundings bound its relative error)."""
    rng = np.random.default_rng(seed)
    code = np.repeat(np.arange(len(seg_lens), dtype=np.int32), seg_lens)
    m = len(code)
    n_drop = int(m * dropped) + (3 if dropped else 0)
    group = np.concatenate([code, rng.integers(-1, max(len(seg_lens), 1), n_drop).astype(np.int32)])
    status = np.concatenate([np.zeros(m, np.int32), rng.choice(np.array([1, 8, 9], np.int32), n_drop)])
    p = rng.permutation(m + n_drop)
    group, status = group[p], status[p]
    stars = stars_pool[rng.integers(0, len(stars_pool), m + n_drop)] if stars_pool is not None else np.exp(rng.normal(0.0, 3.0, m + n_drop))
    ts = SPECIAL_TS[rng.integers(0, len(SPECIAL_TS), m + n_drop)]
    return status, group, np.ascontiguousarray(stars, dtype=np.float64), np.ascontiguousarray(ts)


def model_order_case(status, group, stars, ts, n_skus):
    """What rr_products_order_dev must answer for the case, by products.model_order: (perm, seg_off, n_reviews, star sum in
    row order, star count, last_ts)."""
    from review_recommender_amd.products import model_order
    rows = np.flatnonzero(status == 0)
    code, s, t = group[rows], stars[rows], ts[rows]
    perm = rows[model_order(code, s, t, rows)].astype(np.int32)
    n_reviews = np.bincount(code, minlength=n_skus).astype(np.int64)
    seg = np.zeros(n_skus + 1, np.int64)
    np.cumsum(n_reviews, out=seg[1:])
    ok = ~np.isnan(s)
    with np.errstate(invalid="ignore"):
        star_sum = np.bincount(code[ok], weights=s[ok], minlength=n_skus).astype(np.float64)
    star_cnt = np.bincount(code[ok], minlength=n_skus).astype(np.int64)
    last = np.full(n_skus, NAT, np.int64)
    np.maximum.at(last, code, t)
    return perm, seg, n_reviews, star_sum, star_cnt, last
