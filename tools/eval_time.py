"""Times a sweep of ranking configurations over a labelled dev set by three routes (review-recommender_amd/evals.py,
csrc/rr_evals.hip).

    python tools/eval_time.py --out profiles/eval_sweep.json

One GPU, an index of --docs products (synth.text_corpus, unit rows), --queries labelled queries (2-5 words of one product's
text, the vector that product's row plus noise, labels from the index's own dense answer), --configs configurations: the four
BENCHMARK_CONFIGS and weight variants of "Hybrid" (three gate penalties in all; "Hybrid + Rerank" is the one reranking
configuration, scored by a seeded --layers-layer cross-encoder).  Gate, reranker pairs and query text on the device in every
route; the query vectors are given (no encoder is timed).  Prints one JSON line:
  (a) per_query_route     the reference's own loop: `evaluate_ranking_methods(engine.run_search, ...)`, one search and one frame
                          per query and configuration -- timed on the FIRST --slice QUERIES ONLY (stated in the JSON), wall
                          clock; per_query_route_full_s_extrapolated = that time * queries / slice;
  (b) batch_route         `run_search_batch` in batches of 256 (what its frames allow) per configuration plus
                          `model_ir_metrics` over the sku lists, all queries, wall clock; its search and model parts apart;
  (c) evaluate            `SearchEngine.evaluate`, all queries, wall clock (median of --reps), and once more with HIP events
                          around every stage: the query fronts, K1, K2, the gate match, the reranker, K3 per configuration,
                          rr_ir_metrics_dev per configuration (sums over the batches; per launch = sum / launches).
The tables of (b) and (c) are compared bitwise.  Nothing is asserted about which is faster: the JSON says it."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--mean-words", type=int, default=60)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--configs", type=int, default=16)
    ap.add_argument("--slice", type=int, default=256)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import pandas as pd
    import torch
    from review_recommender_amd import evals, synth
    from review_recommender_amd.cross_encoder import CrossEncoder
    from review_recommender_amd.engine import SearchEngine
    from review_recommender_amd.wordpiece import WordPieceTokenizer

    say = lambda *s: print("[eval_time]", *s, file=sys.stderr, flush=True)
    texts = synth.text_corpus(a.docs, 3, mean_len=a.mean_words)
    n_rev, stars = synth.metadata(a.docs, 2)
    meta = pd.DataFrame({"sku": synth.skus(a.docs), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})
    blob = {"skus": meta["sku"].tolist(), "corpus": [t.split() for t in texts]}
    emb = synth.unit_rows(a.docs, 384, 1)
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(synth.WORDS) + ["##s", "##ing", "for", "the", "with"]
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    ce = CrossEncoder(synth.bert_state_dict(41, n_layers=a.layers, vocab=len(words)), tok)
    engine = SearchEngine(meta, emb, blob, normalize=False, cross_encoder=ce, gate="device", rerank="device", query_text="device")
    say("engine ready")

    rng = np.random.default_rng(11)
    source = rng.choice(a.docs, size=a.queries, replace=False)
    queries = [" ".join(rng.choice(texts[p].split(), size=int(rng.integers(2, 6)))) for p in source]
    qv = emb[source] + 0.6 * synth.unit_rows(a.queries, 384, 5)
    qv = (qv / np.linalg.norm(qv, axis=1, keepdims=True)).astype(np.float32)
    configs = dict(evals.BENCHMARK_CONFIGS)
    hybrid = evals.BENCHMARK_CONFIGS["Hybrid"]
    for i in range(a.configs - len(configs)):
        wd = 0.2 + 0.05 * i
        configs[f"Hybrid v{i}"] = dict(hybrid, w_dense=wd, w_bm25=0.8 - wd - 0.1, w_prior=0.1, min_reviews=(1, 5, 8)[i % 3],
                                       gate_penalty=(0.3, 0.5)[i % 2])
    configs = dict(list(configs.items())[:a.configs])
    # labels: the index's own dense top-30 at ranks 1, 4, 12, 19, 30 and one sku no index holds; every fifth query none
    rows = np.concatenate([engine.index.dense_topk(qv[i:i + 1024], 30)[0] for i in range(0, a.queries, 1024)])
    skus = meta["sku"].tolist()
    test_queries = [{"id": f"q{i}", "query": q,
                     "relevant_items": set() if i % 5 == 4 else {skus[rows[i][r - 1]] for r in (1, 4, 12, 19, 30)} | {"NOT-IN-INDEX"}}
                    for i, q in enumerate(queries)]
    labels = evals.LabelSet.from_queries(test_queries, skus)
    res = {"docs": a.docs, "queries": a.queries, "configs": len(configs), "rerank_configs": sum(c["rerank_k"] > 0 for c in configs.values()),
           "gate_penalties": sorted({c["gate_penalty"] for c in configs.values()}), "cross_encoder_layers": a.layers,
           "labels": int(len(labels.lab_row)), "coverage_rate": labels.coverage()["coverage_rate"]}

    # (c) evaluate: wall clock, then stage by stage
    report = engine.evaluate(labels, configs, qvecs=qv)                       # warm-up
    wall = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        report = engine.evaluate(labels, configs, qvecs=qv)
        summary = report.summary
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    res["evaluate_wall_s"] = {"median": float(np.median(wall)), "min": float(min(wall)), "max": float(max(wall))}
    say("evaluate", res["evaluate_wall_s"])
    pairs = {}

    def timed(owner, attr, stage):
        inner = getattr(owner, attr)

        def wrapper(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = inner(*args, **kw)
            e1.record()
            pairs.setdefault(stage, []).append((e0, e1))
            return out
        setattr(owner, attr, wrapper)
        return lambda: setattr(owner, attr, inner) if owner is evals.DeviceLabels else delattr(owner, attr)

    s = engine.searcher
    undo = [timed(engine._query_text, "front", "front"), timed(s, "dense_pool", "k1"), timed(s, "bm25_at", "k2"),
            timed(s.gate_text, "gate", "gate"), timed(s.rerank_text, "scores", "rerank"), timed(s, "fuse", "k3"),
            timed(evals.DeviceLabels, "metrics", "metrics")]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    engine.evaluate(labels, configs, qvecs=qv)
    torch.cuda.synchronize()
    res["evaluate_wall_with_events_s"] = time.perf_counter() - t0
    for u in undo:
        u()
    stages = {}
    for stage, evs in pairs.items():
        ms = [e0.elapsed_time(e1) for e0, e1 in evs]
        stages[stage] = {"launches": len(ms), "sum_s": float(sum(ms)) / 1e3, "per_launch_ms": float(np.median(ms))}
    res["evaluate_stages"] = stages
    res["shared_stages_s"] = sum(stages[n]["sum_s"] for n in ("front", "k1", "k2", "gate", "rerank") if n in stages)
    res["metrics_kernel_cheaper_than_k3"] = stages["metrics"]["per_launch_ms"] < stages["k3"]["per_launch_ms"]
    say("stages", stages)

    # (b) run_search_batch in batches of 256 + the model
    t_search = t_model = 0.0
    tables = {}
    for name, c in configs.items():
        got = []
        for first in range(0, a.queries, 256):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            answers = engine.run_search_batch(queries[first:first + 256], qvecs=qv[first:first + 256], **c)
            t1 = time.perf_counter()
            for q, (frame, _, _) in zip(test_queries[first:first + 256], answers):
                got.append(list(evals.model_ir_metrics(frame["sku"].tolist(), q["relevant_items"]).values()))
            t_search, t_model = t_search + (t1 - t0), t_model + (time.perf_counter() - t1)
        tables[name] = np.array(got)
        say("batch route", name, round(t_search, 2), round(t_model, 2))
    res["batch_route_s"] = {"total": t_search + t_model, "run_search_batch": t_search, "model": t_model}
    res["tables_equal_bitwise"] = all(report.metrics_dev[n].cpu().numpy().tobytes() == tables[n].tobytes() for n in configs)
    assert res["tables_equal_bitwise"], "evaluate and run_search_batch + model disagree"

    # (a) the reference's loop over run_search, on a slice
    n = min(a.slice, a.queries)
    vec = {q: v for q, v in zip(queries[:n], qv[:n])}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = evals.evaluate_ranking_methods(lambda q, **c: engine.run_search(q, qvec=vec[q], **c), test_queries[:n], configs)
    res["per_query_route"] = {"queries_timed": n, "stated": f"timed on the first {n} of {a.queries} queries only", "s": time.perf_counter() - t0}
    res["per_query_route_full_s_extrapolated"] = res["per_query_route"]["s"] * a.queries / n
    assert list(table.index) == list(configs)
    res["speedup_evaluate_over_batch_route"] = res["batch_route_s"]["total"] / res["evaluate_wall_s"]["median"]
    res["speedup_evaluate_over_per_query_route_extrapolated"] = res["per_query_route_full_s_extrapolated"] / res["evaluate_wall_s"]["median"]
    res["summary_ndcg10"] = {m: float(summary.loc[m, "ndcg@10"]) for m in list(configs)[:4]}
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
