"""Times the query text of one batch on the host and on the GPU (review-recommender_amd/querytext.py, csrc/rr_query.hip).

    python tools/query_text_time.py --out profiles/query_text_b256.json

One GPU, the corpus of tools/gate_time.py (100 k products, synth.text_corpus), B = 256 queries of 2-5 corpus words, pool 150,
gate_penalty 0.5, the gate on the device.  Prints one JSON line:
  (a) host_front_s        the host front end alone, as run_search_batch runs it per query: tokenize_query, term_ids,
                          build_gate_groups, pack_groups, and text_ids with pack_queries;
  (b) device_front_s      the device front end between HIP events (the upload, the WordPiece kernels, rr_query_front_dev,
                          rr_query_strip_dev), with and without the reranker's ids; device_front_wall_s: the host's share of
                          queueing it (encode, pinned staging, launches), which runs ahead of the kernels;
  (c) search_batch_*_s    a gated HybridSearcher.search_batch FROM STRINGS, both ways, alternating in one loop: the host way
                          tokenises, looks up and builds groups in Python and hands lists over, the device way calls
                          QueryText.front and hands the QueryFront over;
  (d) run_search_batch_*_s  SearchEngine.run_search_batch (frames included), query_text="host" and "device", alternating;
each as median / p10 / p90 over the timed repetitions after warm-up calls.  The yardstick is the host path of the same run.
The two paths' results are compared bitwise.  Nothing is asserted about which is faster: the JSON says it."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from gate_time import make_queries, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--mean-words", type=int, default=1200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import pandas as pd
    import torch
    from review_recommender_amd import synth, text as T
    from review_recommender_amd.engine import FusionWeights, SearchEngine
    from review_recommender_amd.gate import pack_groups
    from review_recommender_amd.querytext import QueryText
    from review_recommender_amd.rerank import pack_queries
    from review_recommender_amd.wordpiece import WordPieceTokenizer

    t0 = time.perf_counter()
    texts = synth.text_corpus(a.docs, 3, mean_len=a.mean_words)
    res = {"docs": a.docs, "batch": a.batch, "pool": 150, "gate_penalty": 0.5, "make_corpus_s": time.perf_counter() - t0}
    n_rev, stars = synth.metadata(a.docs, 2)
    meta = pd.DataFrame({"sku": synth.skus(a.docs), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})
    blob = {"skus": meta["sku"].tolist(), "corpus": [t[:240].split() for t in texts]}      # K2 over short documents
    emb = synth.unit_rows(a.docs, 384, 1)
    engines = {qt: SearchEngine(meta, emb, blob, normalize=False, gate="device", query_text=qt) for qt in ("host", "device")}
    searcher, bm25 = engines["device"].searcher, engines["device"].searcher.bm25
    tok = WordPieceTokenizer({w: i for i, w in enumerate(["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(synth.WORDS))})
    queries = make_queries(a.batch, 7)
    qvecs = synth.unit_rows(a.batch, 384, 9)
    w = FusionWeights(0.55, 0.20, 0.0, 0.20, 0.0, 20.0, 8, 0.5)
    res["query_bytes"] = int(sum(len(q.encode()) for q in queries))

    # (a) the host front end
    def host_front(with_rerank=True):
        toks = [T.tokenize_query(q) for q in queries]
        ids = [bm25.term_ids(t) for t in toks]
        groups = [T.build_gate_groups(q) for q in queries]
        packed = pack_groups(groups, 0.5)
        pq = pack_queries([tok.text_ids(q) for q in queries], 512) if with_rerank else None
        return ids, groups, packed, pq

    for name, flag in (("host_front_s", True), ("host_front_no_rerank_s", False)):
        ts = []
        for _ in range(a.reps + 2):
            t0 = time.perf_counter()
            host_front(flag)
            ts.append(time.perf_counter() - t0)
        res[name] = spread(ts[2:])

    # (b) the device front end, HIP events around everything it queues
    for name, qt in (("device_front", QueryText(bm25.corpus.vocab, rerank_tokenizer=tok, max_length=512)),
                     ("device_front_no_rerank", engines["device"]._query_text)):
        ev, wall = [], []
        for _ in range(a.reps + 3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            front = qt.front(queries, 0.5)
            e1.record()
            wall.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1) / 1e3)
        qt.check()
        res[name + "_s"], res[name + "_wall_s"] = spread(ev[3:]), spread(wall[3:])
        res[name + "_flagged"] = int((front.needs_host.cpu().numpy() != 0).sum())

    # (c) a gated search_batch from strings
    def batch_host():
        toks = [T.tokenize_query(q) for q in queries]
        ids = [bm25.term_ids(t) for t in toks]
        groups = [T.build_gate_groups(q) for q in queries]
        return searcher.search_batch(qvecs, ids, 10, 0, w, gate_groups=groups)

    def batch_device():
        return searcher.search_batch(qvecs, None, 10, 0, w, query_front=engines["device"]._query_text.front(queries, 0.5))

    for _ in range(3):
        rd, rh = batch_device(), batch_host()
    assert not rd.needs_host.any()
    assert np.array_equal(rd.pool_rows, rh.pool_rows) and rd.columns.tobytes() == rh.columns.tobytes(), "the two fronts differ"
    res["batches_equal_bitwise"] = True
    e2e = {"device": [], "host": []}
    for _ in range(a.reps):
        for name, fn in (("device", batch_device), ("host", batch_host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                           # (returns numpy: the device has finished)
            e2e[name].append(time.perf_counter() - t0)
    res["search_batch_device_text_s"], res["search_batch_host_text_s"] = spread(e2e["device"]), spread(e2e["host"])

    # (d) run_search_batch, frames included
    run = lambda qt: engines[qt].run_search_batch(queries, 10, 0, 0.55, 0.20, 0.0, 0.20, 0.0, 20.0, False, 0, 8, 0.5, qvecs=qvecs)
    for _ in range(2):
        got, want = run("device"), run("host")
    for (gf, gs, gd), (wf, ws, wd) in zip(got, want):
        assert gs == ws and gd == wd and list(gf.columns) == list(wf.columns)
        assert all(gf[c].values.tobytes() == wf[c].values.tobytes() if gf[c].dtype.kind == "f" else gf[c].tolist() == wf[c].tolist()
                   for c in gf.columns), "the two engines differ"
    res["engines_equal_bitwise"] = True
    e2e = {"device": [], "host": []}
    for _ in range(max(a.reps // 2, 3)):
        for name in ("device", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name)
            e2e[name].append(time.perf_counter() - t0)
    res["run_search_batch_device_text_s"], res["run_search_batch_host_text_s"] = spread(e2e["device"]), spread(e2e["host"])
    res["device_text_batch_faster"] = res["search_batch_device_text_s"]["median"] < res["search_batch_host_text_s"]["median"]
    res["device_text_engine_faster"] = res["run_search_batch_device_text_s"]["median"] < res["run_search_batch_host_text_s"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
