"""Times the BM25 index builders on synthetic Zipf corpora (120 tokens per document, 200 k vocabulary).

    python tools/bm25_build_time.py 1000000 strings   # host from_corpus + upload, factorize, H2D, device build
    python tools/bm25_build_time.py 10000000 ids      # device build from ids (build_bm25_index_ids)

Prints one JSON line (and writes it to the path of --out).  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python3 tools/bm25_build_time.py ...`."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

VOCAB, LEN = 200_000, 120


def zipf_ids(n_docs, seed=5):
    rng = np.random.default_rng(seed)
    tok = np.empty(n_docs * LEN, dtype=np.int32)
    step = 1_000_000
    for s in range(0, n_docs, step):
        e = min(n_docs, s + step)
        tok[s * LEN:e * LEN] = ((rng.zipf(1.1, (e - s) * LEN) - 1) % VOCAB).astype(np.int32)
    return tok, np.arange(0, n_docs * LEN + 1, LEN, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("docs", type=int)
    ap.add_argument("mode", choices=["strings", "ids"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true", help="strings mode: leave out from_corpus + to_device")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from review_recommender_amd import bm25 as B
    dev = torch.device("cuda:0")
    tok, off = zipf_ids(a.docs)
    T = int(off[-1])
    res = {"docs": a.docs, "tokens": T, "vocab_cap": VOCAB, "mode": a.mode}
    if a.mode == "strings":
        names = np.array([f"w{i}" for i in range(VOCAB)], dtype=object)
        corpus = [names[tok[i * LEN:(i + 1) * LEN]].tolist() for i in range(a.docs)]
        t0 = time.perf_counter()
        ids, off2, vocab = B.factorize_corpus(corpus)
        res["host_factorize_s"] = time.perf_counter() - t0
        if not a.skip_host:
            t0 = time.perf_counter()
            c = B.BM25Corpus.from_corpus(corpus)
            res["host_from_corpus_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            ix = c.to_device()
            res["host_to_device_s"] = time.perf_counter() - t0
            ix.close()
            del c
        t0 = time.perf_counter()
        B.build_bm25_index(corpus).close()
        res["device_path_from_strings_s"] = time.perf_counter() - t0
        tok, off, n_terms = ids, off2, len(vocab)
        del corpus
    else:
        n_terms = int(tok.max()) + 1
    res["n_terms"] = n_terms
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d_tok, d_off = torch.from_numpy(tok).to(dev), torch.from_numpy(off).to(dev)
    torch.cuda.synchronize()
    res["h2d_s"] = time.perf_counter() - t0
    res["h2d_bytes"] = tok.nbytes + off.nbytes
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ix = B.build_bm25_index_ids(d_tok, d_off, n_terms, host_copy=False)
        times.append(time.perf_counter() - t0)
        res["nnz"] = ix.nnz
        ix.close()
    res["device_build_s"] = times
    # the sort moves: per pass read key (+ payload) twice (histogram, scatter), write key + payload
    nnz = res["nnz"]
    passes_term = max(1, (int(n_terms - 1).bit_length() + 7) // 8)
    passes_doc = max(1, (int(a.docs - 1).bit_length() + 7) // 8)
    post_bytes = passes_term * T * (4 + 8 + 8)
    fwd_bytes = passes_doc * nnz * (4 + 12 + 12)
    res["radix_passes"] = {"postings": passes_term, "forward": passes_doc}
    res["radix_bytes"] = post_bytes + fwd_bytes
    res["radix_s_at_8TBps"] = (post_bytes + fwd_bytes) / 8e12
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
