"""Times the GPU product-embedding build (review-recommender_amd/embed.py) on synthetic product texts near 4 000 characters.

    python tools/embed_build_time.py 100000 --precision fp32 --out profiles/embed_build_100k_fp32.json
    python tools/embed_build_time.py 100000 --precision bf16 --out profiles/embed_build_100k_bf16.json
    python tools/embed_build_time.py 100000 --precision bf16 --nonascii 0.3 --no-host-path        (30 % of the texts carry
        accents, curly quotes, emoji or CJK; profiles/embed_build_100k_bf16_utf8.json)

Prints one JSON line: (a) documents/s of the device tokenizer alone (HIP events around rr_wp_encode_dev, texts resident) beside
the host tokenizer on a sample of the same texts on one core; (b) documents/s of the whole build_product_embeddings beside
the host path the library had before it (QueryEncoder.encode + ProductIndex.from_rows) on a sample small enough to finish.
(c) The tokenizer's share of the GPU time comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python3 tools/embed_build_time.py 20000 --build-only --out FILE`, which also
writes the wall clock of that build split into filter_products and embed_texts_into."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


NONASCII = ["caf\u00e9", "na\u00efve", "\u201cgreat\u201d", "it\u2019s", "\U0001f600", "\u2764\ufe0f", "\u4e2d\u6587", "\u00dcber", "5\u20ac", "\u2122",
            "\u043c\u0438\u0440"]        # accents, curly quotes, emoji, CJK, currency, TM, Cyrillic


def make_world(n_docs, seed=3, n_pieces=30_522, nonascii=0.0):
    """A 30 522-piece vocabulary (the synthetic words, ## forms, single characters, filler) and texts of ~4 000 characters.
    nonascii: the fraction of the texts that carry one to four non-ASCII words (NONASCII) at random places."""
    from review_recommender_amd import synth
    rng = np.random.default_rng(seed)
    words = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    words += list(synth.WORDS) + ["##s", "##ing", "##ed", "##er", "##ly"] + list("abcdefghijklmnopqrstuvwxyz0123456789.,!?-'")
    seen = set(words)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    while len(words) < n_pieces:
        w = "".join(rng.choice(letters, size=int(rng.integers(3, 10))))
        w = w if rng.random() < 0.7 else "##" + w
        if w not in seen:
            seen.add(w)
            words.append(w)
    base = np.array(list(synth.WORDS) + [w + s for w in synth.WORDS[:20] for s in ("s", "ing", "ed")] + [".", ",", "Great", "USB-C"])
    texts = [" ".join(rng.choice(base, size=int(rng.integers(480, 530)))) for _ in range(min(n_docs, 2000))]
    texts = [texts[i % len(texts)] + f" {i}" for i in range(n_docs)]              # all different, same statistics
    if nonascii > 0:
        for i in np.flatnonzero(rng.random(n_docs) < nonascii):
            parts = texts[i].split(" ")
            for _ in range(int(rng.integers(1, 5))):
                parts.insert(int(rng.integers(0, len(parts) + 1)), NONASCII[rng.integers(len(NONASCII))])
            texts[i] = " ".join(parts)
    return words, texts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("docs", type=int)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--host-sample", type=int, default=512, help="documents of the host-path comparison")
    ap.add_argument("--build-only", action="store_true", help="one build and nothing else (for a profiler run)")
    ap.add_argument("--nonascii", type=float, default=0.0, metavar="FRACTION",
                    help="fraction of the texts that carry non-ASCII words (accents, curly quotes, emoji, CJK)")
    ap.add_argument("--no-host-path", action="store_true", help="skip the host-path comparison (b)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import pandas as pd
    import torch
    from review_recommender_amd import embed, synth
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.index import ProductIndex
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    words, texts = make_world(a.docs, nonascii=a.nonascii)
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    enc = QueryEncoder(synth.bert_state_dict(7, n_layers=12, n_labels=0, prefix="", vocab=len(words)), tok, precision=a.precision)
    products = pd.DataFrame({"sku": synth.skus(a.docs), "agg_text": texts})
    res = {"docs": a.docs, "precision": a.precision, "mean_chars": float(np.mean([len(t) for t in texts[:2000]])), "pieces": len(words),
           "nonascii": a.nonascii, "nonascii_docs": sum(not t.isascii() for t in texts)}
    embed.build_product_embeddings(products.iloc[:2048], enc)[0].close()             # warm-up: scratch, allocator, clocks
    if a.build_only:
        t0 = time.perf_counter()
        meta, texts_f = embed.filter_products(products)
        t1 = time.perf_counter()
        ix = ProductIndex(None, n_rows=len(texts_f), dim=384)
        embed.embed_texts_into(ix, texts_f, enc)                      # what build_product_embeddings does behind its filter
        t2 = time.perf_counter()
        ix.close()
        line = json.dumps({"docs": a.docs, "precision": a.precision, "build_s": t2 - t0, "filter_products_s": t1 - t0,
                           "embed_texts_into_s": t2 - t1})
        print(line)
        if a.out:
            pathlib.Path(a.out).write_text(line + "\n")
        return
    # (a) tokenizer alone: 8 192 documents per call, texts already on the device side of the copy
    wp = enc._device_wp
    norm = [embed.normalize_text(t) for t in texts[:8192]]
    docs = [t.encode() for t in norm]
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        q = wp.queue(docs, 512)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    res["device_tokenizer_docs"] = len(docs)
    res["device_tokenizer_s"] = times                       # includes the H2D copy of the text
    res["device_tokenizer_docs_per_s"] = len(docs) / float(np.median(times))
    res["tokens_per_doc"] = int(q[1].numpy()[0]) / len(docs)
    t0 = time.perf_counter()
    n_host = min(300, len(norm))
    for t in norm[:n_host]:
        tok.encode_pair(t, None, 512)
    res["host_tokenizer_docs_per_s"] = n_host / (time.perf_counter() - t0)
    res["host_tokenizer_sample"] = n_host
    # (b) the whole build, beside the host path on a sample
    runs = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = {}
        try:
            ix = embed.build_product_embeddings(products, enc, stats=stats)[0]
        except TypeError:                    # (a build without the host-pass statistics)
            ix = embed.build_product_embeddings(products, enc)[0]
        runs.append(time.perf_counter() - t0)
        ix.close()
    res["build_s"] = runs
    res["build_docs_per_s"] = a.docs / min(runs)
    if "host_docs" in stats:
        res["host_pass_docs"] = len(stats["host_docs"])
        res["host_pass_share"] = len(stats["host_docs"]) / a.docs
    if a.no_host_path:
        line = json.dumps(res)
        print(line)
        if a.out:
            pathlib.Path(a.out).write_text(line + "\n")
        return
    t0 = time.perf_counter()
    _, texts_f = embed.filter_products(products)
    res["host_filter_normalize_s"] = time.perf_counter() - t0
    n = min(a.host_sample, a.docs)
    tok._cache.clear()
    t0 = time.perf_counter()
    rows = enc.encode(texts_f[:n])
    ProductIndex.from_rows(rows, normalize=True).close()
    dt = time.perf_counter() - t0
    res["host_path_sample"] = n
    res["host_path_docs_per_s"] = n / dt
    res["speedup_over_host_path"] = res["build_docs_per_s"] / res["host_path_docs_per_s"]
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
