"""Times the BM25 index built from RAW TEXT: the device tokenizer and vocabulary (csrc/rr_doctok.hip) against the host path.

    python tools/bm25_text_build_time.py 1000000 --out profiles/bm25_text_build_1M.json
    python tools/bm25_text_build_time.py 1000000 --skip-host --reps 1      # under rocprofv3 --kernel-trace --stats

Synthetic documents of about 120 Zipf tokens (200 k vocabulary, as tools/bm25_build_time.py) rendered as text: mixed case,
punctuation between the words, stop words and one-letter words among them, apostrophes, and a share of documents with
non-ASCII text (accents, CJK, the Kelvin sign, the dotted capital I).  Prints one JSON line with, in seconds:
  device path   pack (embed._utf8_column), upload (H2D of the text), tokenize (both passes), vocabulary (table, scan, ids),
                vocabulary_download (bytes to the host and the dict), index_build (build_bm25_index_ids), and their sum
  host path     host_tokenize (artifacts.build_bm25_blob), host_factorize (bm25.factorize_corpus), host_index_build
                (build_bm25_index_ids from the host ids: upload + the same device build), and their sum
and speedup = host sum / device sum, for the FIRST device run (cold: it pays for the allocations, as the single host run
does) and for the best of --reps.  The two indexes are compared (df, CSR arrays) before anything is reported.
long_token: one document that is a single alphanumeric run of LONG_TOKEN bytes, tokenised alone (one lane walks it)."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

VOCAB, LEN = 200_000, 120
LONG_TOKEN = 1 << 20
STOPS = ["the", "and", "of", "a", "to", "in", "is", "it", "for", "with", "I", "x"]
EXTRA = [" caf\u00e9 na\u00efve \u6f22\u5b57 mug", " 25 \u212a rated, \u0130stanbul-made", " \u2014 it's the kid's o'clock\u2026"]


def render(n_docs, seed=5):
    """n_docs texts; every 8th word is a stop word or a single letter, about one document in five holds non-ASCII text."""
    rng = np.random.default_rng(seed)
    lower = np.array([f"w{i}" for i in range(VOCAB)], dtype=object)
    forms = [lower, np.array([w.upper() for w in lower], dtype=object), np.array([w + "," for w in lower], dtype=object),
             np.array([w + "." for w in lower], dtype=object), np.array(["(" + w + ")" for w in lower], dtype=object),
             np.array([w + "'s" for w in lower], dtype=object)]
    stops = np.array(STOPS + [s.title() for s in STOPS], dtype=object)
    texts = []
    step = 100_000
    for s in range(0, n_docs, step):
        m = min(step, n_docs - s)
        ids = (rng.zipf(1.1, m * LEN) - 1) % VOCAB
        form = rng.choice(len(forms), m * LEN, p=[0.6, 0.08, 0.1, 0.1, 0.04, 0.08])
        words = np.empty(m * LEN, dtype=object)
        for f, table in enumerate(forms):
            sel = form == f
            words[sel] = table[ids[sel]]
        words[::8] = stops[rng.integers(0, len(stops), len(words[::8]))]
        words = words.reshape(m, LEN)
        extra = rng.integers(0, 5 * len(EXTRA), m)
        texts += [" ".join(row) + (EXTRA[e] if e < len(EXTRA) else "") for row, e in zip(words.tolist(), extra.tolist())]
    return texts


def note(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("docs", type=int)
    ap.add_argument("--reps", type=int, default=2, help="device-path repetitions (the first pays for the allocations)")
    ap.add_argument("--skip-host", action="store_true", help="leave the host path (and the comparison) out")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import pandas as pd
    import torch
    from review_recommender_amd import bm25 as B
    from review_recommender_amd.artifacts import build_bm25_blob
    from review_recommender_amd.doctok import DeviceDocTokenizer
    note("rendering the texts")
    texts = render(a.docs)
    note("device path")
    res = {"docs": a.docs, "non_ascii_docs": sum(not t.isascii() for t in texts)}
    torch.zeros(1, device="cuda:0")
    dt = DeviceDocTokenizer(0)
    runs = []
    index = None
    for _ in range(a.reps):
        if index is not None:
            index.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tok, off, vocab = dt.tokenize(texts)
        t1 = time.perf_counter()
        index = B.build_bm25_index_ids(tok, off, len(vocab), vocab=vocab, host_copy=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        r = dict(dt.seconds, index_build=t2 - t1, strings_to_index=t2 - t0)
        runs.append({k: round(v, 6) for k, v in r.items()})
    res.update(text_bytes=dt.sizes()[1], tokens=int(tok.numel()), n_terms=len(vocab), device_runs=runs)
    best = min(runs, key=lambda r: r["strings_to_index"])
    res["device_path_first_run"] = runs[0]
    res["device_path_best_run"] = best
    note("one long token")
    lt = DeviceDocTokenizer(0)
    for _ in range(2):
        t0 = time.perf_counter()
        ltok, loff, lvocab = lt.tokenize(["ab1" * (LONG_TOKEN // 3)])
        res["long_token"] = {"bytes": LONG_TOKEN // 3 * 3, "tokens": int(ltok.numel()), "tokenize": round(lt.seconds["tokenize"], 6),
                             "vocabulary": round(lt.seconds["vocabulary"], 6), "total": round(time.perf_counter() - t0, 6)}
    lt.close()
    if not a.skip_host:
        meta = pd.DataFrame({"sku": np.arange(a.docs), "agg_text": texts})
        note("host path: build_bm25_blob")
        t0 = time.perf_counter()
        corpus = build_bm25_blob(meta)["corpus"]
        t1 = time.perf_counter()
        note("host path: factorize_corpus")
        h_tok, h_off, h_vocab = B.factorize_corpus(corpus)
        t2 = time.perf_counter()
        del corpus
        host_index = B.build_bm25_index_ids(h_tok, h_off, len(h_vocab), vocab=h_vocab, host_copy=False)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        note("comparing the two indexes")
        res["host_path"] = {"host_tokenize": round(t1 - t0, 6), "host_factorize": round(t2 - t1, 6),
                            "host_index_build": round(t3 - t2, 6), "strings_to_index": round(t3 - t0, 6)}
        same = (np.array_equal(tok.cpu().numpy(), h_tok) and np.array_equal(off.cpu().numpy(), h_off) and vocab == h_vocab
                and list(vocab) == list(h_vocab) and np.array_equal(index.df, host_index.df))
        ca, cb = index.copy_csr(), host_index.copy_csr()
        same = same and all(np.array_equal(ca[k], cb[k]) for k in ca)
        res["identical_to_host_path"] = bool(same)
        res["speedup_first_run"] = round(res["host_path"]["strings_to_index"] / runs[0]["strings_to_index"], 2)
        res["speedup_best_run"] = round(res["host_path"]["strings_to_index"] / best["strings_to_index"], 2)
        host_index.close()
    index.close()
    dt.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")
    if not a.skip_host and not res["identical_to_host_path"]:
        raise SystemExit("the device path and the host path disagree")


if __name__ == "__main__":
    main()
