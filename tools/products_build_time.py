"""Times the GPU products build (review-recommender_amd/products.py: build_products) on a synthetic review table.

    python tools/products_build_time.py 1000000 --out profiles/products_build_1M.json

Prints one JSON line: (a) the clean, dedup, order + KPIs and concatenate stages alone, the text resident on the device, HIP
events around each call, median of 5 after a warm-up call; (b) the wall clock of build_products and of its phases
(stats["seconds"]), best of 2 builds after a warm-up build; (c) the wall clock of products.model_build_products (numpy and
Python on one core) on the same table as the host baseline, and whether the two frames are equal.  The table is
tools/review_build_time.py's, with a time stamp per row."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def make_reviews(n, n_skus):
    import pandas as pd
    from tools.review_build_time import make_reviews as base
    df = base(n)
    rng = np.random.default_rng(11)
    if n_skus:
        df["sku"] = [f"B{s:09d}" for s in rng.integers(0, n_skus, n)]
    df["ts"] = pd.to_datetime(1_500_000_000 + rng.integers(0, 2000, n) * 86400, unit="s", utc=True)      # ties are common
    df["stars"] = df["stars"].astype(np.float64)
    df.loc[rng.random(n) < 0.02, "stars"] = np.nan
    return df


def stage_times(df, max_per_sku, repeats=5):
    import torch
    from review_recommender_amd import embed, products as P, textprep as T
    sku, texts, stars, ts = P.prepare_columns(df)
    raw, off = embed._utf8_column(texts)
    n, total = len(texts), int(off[-1])
    tp, pb = T.TextPrep(0), P.ProductsPrep(0)
    d_raw = torch.from_numpy(raw[:total].copy()).cuda()
    d_text = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(off)).cuda()
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3

    clean = lambda: tp.clean(d_raw.data_ptr(), total, d_off.data_ptr(), n, False, d_text.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), st,
                             max_chars=0)
    res = {"text_bytes": total, "clean_s": [timed(clean) for _ in range(repeats + 1)][1:]}
    status = d_st.clone()
    left = int(np.count_nonzero(status.cpu().numpy() & T.NEEDS_HOST))
    skus, group = P.sku_ranks(sku, status.cpu().numpy() == 0)
    n_skus = len(skus)
    d_grp = torch.from_numpy(group).cuda()
    dd = []
    for _ in range(repeats + 1):
        d_st.copy_(status)
        dd.append(timed(lambda: tp.dedup(d_text.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr(), d_st.data_ptr(), n, 64, st)))
    res["dedup_s"] = dd[1:]
    tp.check()
    keep = d_st.cpu().numpy() == 0
    d_stars, d_ts = torch.from_numpy(stars).cuda(), torch.from_numpy(ts).cuda()
    d_perm = torch.empty(n, dtype=torch.int32, device="cuda")
    d_seg = torch.empty(n_skus + 1, dtype=torch.int64, device="cuda")
    d_kpi = torch.empty((4, max(n_skus, 1)), dtype=torch.int64, device="cuda")
    order = lambda: pb.order(d_st.data_ptr(), d_grp.data_ptr(), d_stars.data_ptr(), d_ts.data_ptr(), n, n_skus, d_perm.data_ptr(),
                             d_seg.data_ptr(), *[d_kpi[j].data_ptr() for j in range(4)], st)
    res["order_kpis_s"] = [timed(order) for _ in range(repeats + 1)][1:]
    cap = int(d_len.cpu().numpy()[keep].astype(np.int64).sum()) + 2 * int(np.count_nonzero(keep))
    d_out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    d_out_off = torch.empty(n_skus + 1, dtype=torch.int64, device="cuda")
    d_count = torch.empty(1, dtype=torch.int64, device="cuda")
    concat = lambda: pb.concat(d_text.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), n, d_perm.data_ptr(), d_seg.data_ptr(), n_skus,
                               max_per_sku, d_out.data_ptr(), cap, d_out_off.data_ptr(), d_count.data_ptr(), st)
    res["concat_s"] = [timed(concat) for _ in range(repeats + 1)][1:]
    pb.check()
    res.update(rows=n, left_to_host=left, kept=int(np.count_nonzero(keep)), n_skus=n_skus, agg_text_bytes=int(d_count.cpu()[0]),
               longest_sku=int(np.diff(d_seg.cpu().numpy()).max()) if n_skus else 0)
    for k in ("clean_s", "dedup_s", "order_kpis_s", "concat_s"):
        res[k.replace("_s", "_median_s")] = float(np.median(res[k]))
    res["device_stages_median_s"] = sum(res[k] for k in ("clean_median_s", "dedup_median_s", "order_kpis_median_s", "concat_median_s"))
    tp.close()
    pb.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reviews", type=int)
    ap.add_argument("--skus", type=int, default=0, help="distinct skus (default: reviews / 25)")
    ap.add_argument("--max-reviews-per-sku", type=int, default=80)
    ap.add_argument("--builds", type=int, default=2)
    ap.add_argument("--no-model", action="store_true", help="skip the host baseline")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from review_recommender_amd import products as P
    t0 = time.perf_counter()
    df = make_reviews(a.reviews, a.skus)
    res = {"reviews": a.reviews, "skus": int(df["sku"].nunique()), "max_reviews_per_sku": a.max_reviews_per_sku,
           "make_table_s": time.perf_counter() - t0, "mean_chars": float(df["text"].iloc[:5000].str.len().mean())}
    print("table made", res, flush=True)
    P.build_products(df.iloc[:4096], a.max_reviews_per_sku)                  # warm-up: scratch, allocator, clocks
    res["stages"] = stage_times(df, a.max_reviews_per_sku)
    print("stages", res["stages"], flush=True)
    runs, products = [], None
    for _ in range(a.builds):
        stats = {}
        t0 = time.perf_counter()
        products, deduped = P.build_products(df, a.max_reviews_per_sku, stats=stats)
        runs.append({"build_s": time.perf_counter() - t0, "seconds": stats["seconds"], "products": len(products), "deduped": deduped,
                     "host_clean_docs": len(stats["host_clean_docs"]), "dropped": [stats["short"], stats["duplicate"]]})
        print("build", runs[-1], flush=True)
    res["builds"] = runs
    res["build_s"] = min(r["build_s"] for r in runs)
    best = min(runs, key=lambda r: r["build_s"])["seconds"]
    res["slowest_phase"] = max(best, key=best.get)
    if not a.no_model:
        t0 = time.perf_counter()
        want, want_deduped = P.model_build_products(df, a.max_reviews_per_sku)
        res["model_build_products_s"] = time.perf_counter() - t0
        res["equals_model"] = bool(want_deduped == runs[-1]["deduped"] and want.equals(products))
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
