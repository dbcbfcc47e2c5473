"""Times the GPU review-embedding build (review-recommender_amd/embed.py: build_review_embeddings) on a synthetic review table.

    python tools/review_build_time.py 1000000 --precision fp32 --out profiles/review_build_1M_fp32.json

Prints one JSON line: (a) the clean, dedup and compact stages alone, text resident on the device, HIP events around each call,
median of 5; (b) the wall clock of the whole build and of its phases (stats["seconds"]), best of 2 builds, of which
"tokenize_encode_store" is the tokenizer + encoder + row store over the surviving rows; (c) the pandas path for the same
steps on one core: normalize_text, the length filter, looks_spammy and drop_duplicates as nlp/11_build_product_embeddings.py:
111-118 runs them."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def make_reviews(n, seed=5, n_base=20000):
    """n reviews of ~40 words over n / 25 skus: 20 % with line breaks and doubled blanks, 3 % with non-ASCII words, 5 %
    duplicates of an earlier review of the same sku, 2 % spam (two links or a promo phrase), 1 % too short."""
    import pandas as pd
    from review_recommender_amd import synth
    rng = np.random.default_rng(seed)
    base = synth.text_corpus(n_base, seed, mean_len=40)
    pick = rng.integers(0, n_base, n)
    kind = rng.random(n)
    sku = rng.integers(0, max(1, n // 25), n)
    texts = []
    for i in range(n):
        t = f"{base[pick[i]]} {i}"
        k = kind[i]
        if k < 0.20:
            t = "  " + t.replace(" ", "  ", 3).replace(" ", "\r\n", 1) + " \n"
        elif k < 0.23:
            t = t + " café 中文 \U0001f600 naïve"
        elif k < 0.25:
            t = t + (" see http://a.b/c and www.d.e" if i % 2 else " use code MUG20 today")
        elif k < 0.26:
            t = "ok"
        elif k < 0.31 and i > 100:
            j = int(rng.integers(0, i))
            t, sku[i] = texts[j], sku[j]
        texts.append(t)
    return pd.DataFrame({"id": np.arange(n), "sku": [f"B{s:09d}" for s in sku], "ts": pd.Timestamp("2021-01-01", tz="UTC"),
                         "stars": rng.integers(1, 6, n), "text": texts})


def pandas_path(df):
    """nlp/11_build_product_embeddings.py:111-118 with embed.normalize_text / looks_spammy (the reference's own functions)."""
    from review_recommender_amd import embed
    t = {}
    t0 = time.perf_counter()
    d = df[["sku", "text"]].copy()
    d["__txt"] = d["text"].map(embed.normalize_text)
    d = d[d["__txt"].str.len() >= embed.MIN_TEXT_LEN]
    t["normalize_and_length_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    d = d[~d["__txt"].apply(embed.looks_spammy)]
    t["looks_spammy_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    d = d.drop_duplicates(subset=["sku", "__txt"])
    t["drop_duplicates_s"] = time.perf_counter() - t0
    t["total_s"] = sum(t.values())
    t["rows_kept"] = len(d)
    return t


def stage_times(df, repeats=5):
    import pandas as pd
    import torch
    from review_recommender_amd import embed, textprep as T
    raw, off = embed._utf8_column(df["text"].tolist())
    n, total = len(df), int(off[-1])
    tp = T.TextPrep(0)
    d_raw = torch.from_numpy(raw[:total].copy()).cuda()
    d_text = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(off)).cuda()
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    d_grp = torch.from_numpy(pd.factorize(df["sku"])[0].astype(np.int32)).cuda()
    o_text = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
    o_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    o_src = torch.empty(n, dtype=torch.int32, device="cuda")
    o_cnt = torch.empty(2, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3

    clean = lambda: tp.clean(d_raw.data_ptr(), total, d_off.data_ptr(), n, True, d_text.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), st)
    res = {"text_bytes": total, "clean_s": [timed(clean) for _ in range(repeats + 1)][1:]}
    status = d_st.clone()
    dd = []
    for _ in range(repeats + 1):
        d_st.copy_(status)
        dd.append(timed(lambda: tp.dedup(d_text.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr(), d_st.data_ptr(), n, 64, st)))
    res["dedup_s"] = dd[1:]
    compact = lambda: tp.compact(d_text.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), n, o_text.data_ptr(), total,
                                 o_off.data_ptr(), o_src.data_ptr(), o_cnt.data_ptr(), st)
    res["compact_s"] = [timed(compact) for _ in range(repeats + 1)][1:]
    tp.check()
    s = d_st.cpu().numpy()
    res.update(left_to_host=int(np.count_nonzero(s & T.NEEDS_HOST)), short=int(np.count_nonzero(s & T.SHORT)),
               spam=int(np.count_nonzero(s & T.SPAM)), duplicate=int(np.count_nonzero(s & T.DUP)), kept=int(o_cnt.cpu()[0]),
               kept_bytes=int(o_cnt.cpu()[1]))
    for k in ("clean_s", "dedup_s", "compact_s"):
        res[k.replace("_s", "_median_s")] = float(np.median(res[k]))
    res["clean_GB_per_s"] = total / res["clean_median_s"] / 1e9
    tp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reviews", type=int)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--builds", type=int, default=2)
    ap.add_argument("--no-pandas", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from tools.embed_build_time import make_world
    from review_recommender_amd import embed, synth
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    t0 = time.perf_counter()
    df = make_reviews(a.reviews)
    res = {"reviews": a.reviews, "precision": a.precision, "make_table_s": time.perf_counter() - t0,
           "mean_chars": float(df["text"].iloc[:5000].str.len().mean())}
    print("table made", res, flush=True)
    words, _ = make_world(1)
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    enc = QueryEncoder(synth.bert_state_dict(7, n_layers=12, n_labels=0, prefix="", vocab=len(words)), tok, precision=a.precision)
    embed.build_review_embeddings(df.iloc[:4096], enc)                       # warm-up: scratch, allocator, clocks
    res["stages"] = stage_times(df)
    print("stages", res["stages"], flush=True)
    runs = []
    for _ in range(a.builds):
        stats = {}
        t0 = time.perf_counter()
        table, emb, _ = embed.build_review_embeddings(df, enc, stats=stats)
        runs.append({"build_s": time.perf_counter() - t0, "seconds": stats["seconds"], "rows": len(table),
                     "host_clean_docs": len(stats["host_clean_docs"]), "host_docs": len(stats["host_docs"]),
                     "dropped": [stats["short"], stats["spam"], stats["duplicate"]]})
        print("build", runs[-1], flush=True)
        del table, emb
    res["builds"] = runs
    res["build_s"] = min(r["build_s"] for r in runs)
    if not a.no_pandas:
        res["pandas"] = pandas_path(df)
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
