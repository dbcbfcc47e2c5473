"""Times the hand-over of agg_text from the products build to the product-embedding build, both ways.

    python tools/product_embed_time.py 1000000 --skus 40000 --out profiles/product_embed_device_text.json

The table is tools/products_build_time.py's (synthetic reviews over a fixed number of skus); build_products(keep_device=True)
leaves agg_text on the device.  Prints one JSON line:
(a) the host hand-over, wall clock: DeviceProductText.agg_text() (the copy back and the Python strings), filter_products
    (normalize_text per product), and what embed_texts_into then does to the strings before the tokenizer sees them (UTF-8 for
    the lengths, UTF-8 again per chunk, the join, the pinned staging buffer and its copy up), best of 2;
(b) the device hand-over: rr_textprep_head_measure_dev and rr_textprep_head_write_dev between HIP events, the text resident,
    median of 5 after a warm-up call (the read-back of the lengths between the two is timed apart, wall clock);
(c) the whole build both ways on the same encoder (seeded weights, the vocabulary of tools/embed_build_time.py), best of 2,
    and whether the two indexes hold the same bits.
Recorded, not gated."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def host_hand_over(products, text, chunk_tokens, max_length):
    import torch
    from review_recommender_amd import embed
    t = {}
    text._texts = None
    t0 = time.perf_counter()
    full = text.with_text(products)
    t["agg_text_copy_back_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    meta, texts = embed.filter_products(full)
    t["filter_products_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lens = [len(s.encode("utf-8")) for s in texts]
    for a, b in embed._plan_chunks(lens, max_length, chunk_tokens):
        docs = [s.encode("utf-8") for s in texts[a:b]]
        off = np.zeros(len(docs) + 1, dtype=np.int64)
        np.cumsum([len(d) for d in docs], out=off[1:])
        stage = torch.empty(8 * len(off) + int(off[-1]) + 8, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        host[:8 * len(off)] = off.view(np.uint8)
        host[8 * len(off):8 * len(off) + int(off[-1])] = np.frombuffer(b"".join(docs), dtype=np.uint8)
        stage.to("cuda", non_blocking=True)
    torch.cuda.synchronize()
    t["utf8_and_staging_s"] = time.perf_counter() - t0
    t["total_s"] = sum(t.values())
    t["kept"] = len(texts)
    return t


def device_hand_over(text, repeats=5):
    import torch
    from review_recommender_amd import embed, textprep as T
    n = text.n
    tp = T.TextPrep(0)
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = (text.d_text.data_ptr(), text.text_bytes, text.d_off.data_ptr(), n, None, n, embed.MAX_TEXT_LEN, True, embed.MIN_TEXT_LEN,
            d_len.data_ptr(), d_st.data_ptr())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3

    res = {"measure_s": [timed(lambda: tp.head_measure(*args, st)) for _ in range(repeats + 1)][1:]}
    t0 = time.perf_counter()
    lens, status = d_len.cpu().numpy(), d_st.cpu().numpy()
    res["read_back_lengths_s"] = time.perf_counter() - t0
    tp.head_offsets(d_len.data_ptr(), d_st.data_ptr(), n, d_off.data_ptr(), st)
    total = int(d_off[n].item())
    d_heads = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
    write = lambda: tp.head_write(*args, d_heads.data_ptr(), total, d_off.data_ptr(), st)
    res["write_s"] = [timed(write) for _ in range(repeats + 1)][1:]
    tp.check()
    res.update(docs=n, text_bytes=int(text.text_bytes), head_bytes=total, kept=int(np.count_nonzero(status == 0)),
               left_to_host=int(np.count_nonzero(status & T.NEEDS_HOST)), longest_doc_bytes=int(np.diff(text.d_off.cpu().numpy()).max()),
               docs_over_the_clean_window=int(np.count_nonzero(np.diff(text.d_off.cpu().numpy()) > T.WINDOW_BYTES)))
    res["measure_median_s"] = float(np.median(res["measure_s"]))
    res["write_median_s"] = float(np.median(res["write_s"]))
    res["measure_plus_write_median_s"] = res["measure_median_s"] + res["write_median_s"]
    res["measure_gb_per_s_of_text"] = text.text_bytes / res["measure_median_s"] / 1e9
    tp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reviews", type=int)
    ap.add_argument("--skus", type=int, default=40000)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--builds", type=int, default=2)
    ap.add_argument("--no-builds", action="store_true", help="the hand-over only, no encoder")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from tools.embed_build_time import make_world
    from tools.products_build_time import make_reviews
    from review_recommender_amd import embed, products as P, synth
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    df = make_reviews(a.reviews, a.skus)
    P.build_products(df.iloc[:4096], 80)                                      # warm-up: scratch, allocator, clocks
    t0 = time.perf_counter()
    products, _, text = P.build_products(df, 80, keep_device=True)
    res = {"reviews": a.reviews, "skus": int(text.n), "precision": a.precision, "build_products_keep_device_s": time.perf_counter() - t0}
    chunk_tokens, L = 131072, 512
    runs = [host_hand_over(products, text, chunk_tokens, L) for _ in range(2)]
    res["host_hand_over"] = min(runs, key=lambda r: r["total_s"])
    print("host hand-over", res["host_hand_over"], flush=True)
    res["device_hand_over"] = device_hand_over(text)
    print("device hand-over", res["device_hand_over"], flush=True)
    if not a.no_builds:
        words, _ = make_world(0)
        tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
        enc = QueryEncoder(synth.bert_state_dict(7, n_layers=12, n_labels=0, prefix="", vocab=len(words)), tok, precision=a.precision)
        small = P.build_products(df.iloc[:8192], 80, keep_device=True)
        embed.build_product_embeddings_device(small[0], small[2], enc)[0].close()         # warm-up
        host_runs, dev_runs, rows = [], [], {}
        for _ in range(a.builds):
            text._texts = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix = embed.build_product_embeddings(text.with_text(products), enc)[0]
            host_runs.append(time.perf_counter() - t0)
            rows["host"] = ix.download_rows() if a.precision == "fp32" else None
            ix.close()
            stats = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix = embed.build_product_embeddings_device(products, text, enc, stats=stats)[0]
            dev_runs.append({"build_s": time.perf_counter() - t0, "seconds": stats["seconds"], "host_clean_docs": len(stats["host_clean_docs"]),
                             "host_docs": len(stats["host_docs"])})
            rows["device"] = ix.download_rows() if a.precision == "fp32" else None
            ix.close()
            print("builds", host_runs[-1], dev_runs[-1], flush=True)
        res["host_text_build_s"] = host_runs
        res["device_text_builds"] = dev_runs
        res["device_text_build_s"] = [r["build_s"] for r in dev_runs]
        if a.precision == "fp32":
            res["same_bits"] = bool(np.array_equal(rows["host"].view(np.uint32), rows["device"].view(np.uint32)))
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
