#!/usr/bin/env python3
"""Generates tests/golden/ir_metrics.json and benchmark_configs.json by RUNNING THE REFERENCE'S OWN evals modules
(/root/reference/evals/performance_metrics.py and test_queries.py) in the build container.

    python tests/golden/make_ir_metrics_golden.py     # needs /root/reference; the reference never travels: only these vectors do

Both modules import with numpy + pandas only.  Nothing of them is touched but one module global: validate_ground_truth
reads the module's own TEST_QUERIES, which is set to the fixture's dev set for that one call.

  ir_metrics.json  (stored compactly, skus as integers: tests/ir_metrics_cases.py expands it)
    universe    the skus of a synthetic index: "P00000" .. in row order (n_index of them); "Z...." skus are in no index
    cases       IRMetrics.evaluate_query(id, retrieved, relevant_items, relevance_scores) on seeded cases: every k of K_VALUES
                x the scenarios below (no labels; every labelled sku absent; a hit at rank 1, at rank k, only beyond rank 64,
                none; integer and fractional grades 0-4; relevance_scores with keys outside relevant_items; a label segment
                of one entry, of 30 and of 300 entries; random mixes).  Floats are stored by repr.
    ranking     evaluate_ranking_methods(stub, test_queries, configs) on a stub search function that replays the recorded
                sku lists (and raises for one query, which the reference logs and leaves out), its aggregate table, and
                validate_ground_truth of the same dev set against the universe
  benchmark_configs.json   BENCHMARK_CONFIGS as settings data
"""
import importlib.util
import json
import logging
import pathlib
import sys

import numpy as np
import pandas as pd

HERE = pathlib.Path(__file__).resolve().parent
REF = pathlib.Path("/root/reference")
sys.path.insert(0, str(HERE.parent))

import ir_metrics_cases as cases_file  # noqa: E402

K_VALUES = (1, 4, 5, 7, 8, 9, 10, 19, 20, 50, 65, 130)
N_INDEX = 4000


def load_reference_module(rel, name):
    spec = importlib.util.spec_from_file_location(name, REF / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sku(row):
    return f"P{int(row):05d}"


def absent(rng, n):
    return [f"Z{int(x):04d}" for x in rng.choice(10000, size=n, replace=False)]


def scenarios(rng, k, retrieved_rows):
    """(name, relevant_items, relevance_scores or None) for one retrieved list."""
    others = np.setdiff1d(np.arange(N_INDEX), retrieved_rows)
    pick_other = lambda n: [sku(r) for r in rng.choice(others, size=n, replace=False)]
    ret = [sku(r) for r in retrieved_rows]
    out = [("no_labels", [], None),
           ("all_absent", absent(rng, 3), None),
           ("hit_rank_1", [ret[0]] + pick_other(2), None),
           ("hit_rank_k", [ret[-1]] + pick_other(2) + absent(rng, 1), None),
           ("hit_beyond_64" if k > 64 else "hit_last_only", [ret[int(rng.integers(64, k))] if k > 64 else ret[-1]], None),
           ("no_hit", pick_other(5), None),
           ("one_entry", [ret[int(rng.integers(k))]], None)]
    # integer grades 0-4 on some retrieved skus, some other skus and an absent one
    some = [ret[i] for i in rng.choice(k, size=min(k, 6), replace=False)]
    keys = some + pick_other(3) + absent(rng, 1)
    grades = {s: float(rng.integers(0, 5)) for s in keys}
    out.append(("graded_int", [s for s in keys if grades[s] >= 1.0], grades))
    # fractional grades
    grades = {s: float(rng.uniform(0.0, 4.0)) for s in keys}
    out.append(("graded_fraction", [s for s in keys if grades[s] >= 2.0], grades))
    grades = {s: float(np.round(rng.uniform(0.0, 4.0), 2)) for s in keys}
    out.append(("graded_fraction_2dp", list(keys), grades))
    # relevance_scores with keys outside relevant_items, and a relevant sku the scores leave out
    grades = {s: float(rng.integers(1, 5)) + 0.5 for s in keys}
    out.append(("scores_outside_relevant", keys[::2] + ([s for s in ret if s not in grades][:1] or pick_other(1)), grades))
    # a label segment of 300 entries
    # a label segment of 300 entries (at three list lengths; 30 entries at the others)
    n_big = 300 if k in (10, 20, 130) else 30
    big = list(dict.fromkeys([ret[i] for i in rng.choice(k, size=min(k, 12), replace=False)] + pick_other(n_big)))[:n_big]
    out.append((f"segment_{n_big}", big, None))
    out.append(("segment_30_graded", big[:30:3], {s: float(np.round(rng.uniform(0.0, 4.0), 1)) for s in big[:30]}))
    # random mixes
    for i in range(4):
        n_hit = int(rng.integers(0, min(k, 15) + 1))
        keys = [ret[j] for j in rng.choice(k, size=n_hit, replace=False)] + pick_other(int(rng.integers(0, 8))) + \
            absent(rng, int(rng.integers(0, 3)))
        if i % 3 == 0:
            out.append((f"mix_{i}", keys, None))
        else:
            grades = {s: float(rng.uniform(0.0, 4.0)) if i % 3 == 1 else float(rng.integers(0, 5)) for s in keys}
            out.append((f"mix_{i}", [s for s in keys if rng.random() < 0.7], grades))
    return ret, out


def floats(d):
    return {name: repr(float(v)) for name, v in d.items()}


def main():
    logging.disable(logging.CRITICAL)          # (the reference logs the stub's one failing query)
    pm = load_reference_module("evals/performance_metrics.py", "ref_performance_metrics")
    tq = load_reference_module("evals/test_queries.py", "ref_test_queries")
    rng = np.random.default_rng(20260)
    cases = []
    for k in K_VALUES:
        rows = rng.choice(N_INDEX, size=k, replace=False)
        ret, scen = scenarios(rng, k, rows)
        for name, relevant, scores in scen:
            ev = pm.IRMetrics()
            got = ev.evaluate_query(f"{name}@{k}", ret, set(relevant), None if scores is None else dict(scores))
            cases.append({"id": f"{name}@{k}", "k": k, "retrieved": ret, "relevant_items": sorted(set(relevant)),
                          "relevance_scores": None if scores is None else {s: repr(v) for s, v in scores.items()},
                          "metrics": floats(got)})

    # evaluate_ranking_methods on a stub that replays recorded lists
    configs = {name: dict(c) for name, c in tq.BENCHMARK_CONFIGS.items()}
    queries, tops, replies = [], [], {name: {} for name in configs}
    for i in range(12):
        top = rng.choice(N_INDEX, size=60, replace=False)
        relevant = [sku(top[j]) for j in (0, 3, 11, 18, 29) if rng.random() < 0.8] + absent(rng, 1)
        qd = {"id": f"q{i}", "query": f"query number {i}", "relevant_items": sorted(relevant)} if i % 5 else \
            {"query": f"query number {i}", "relevant_items": sorted(relevant)}            # (no id: the query is the id)
        if i == 7:
            qd["relevant_items"] = []
        queries.append(qd)
        tops.append([int(r) for r in top])
        for name, c in configs.items():
            perm = rng.permutation(60)[:c["k"]] if name != "Dense Only" else np.arange(c["k"])
            replies[name][qd["query"]] = None if (i == 9 and name == "Hybrid") else [sku(top[j]) for j in perm]

    def stub(query, **config):
        name = next(n for n, c in configs.items() if c == config)
        skus = replies[name][query]
        if skus is None:
            raise RuntimeError("stub failure")
        return pd.DataFrame({"sku": skus}), {}, {}

    table = pm.evaluate_ranking_methods(stub, [dict(q, relevant_items=set(q["relevant_items"])) for q in queries], configs)
    tq.TEST_QUERIES = [dict(q, id=q.get("id", q["query"]), relevant_items=set(q["relevant_items"])) for q in queries]
    cov = tq.validate_ground_truth(pd.DataFrame({"sku": [sku(r) for r in range(N_INDEX)]}))
    cov["missing_by_query"] = {q: sorted(v) for q, v in cov["missing_by_query"].items()}
    cov["coverage_rate"] = repr(float(cov["coverage_rate"]))
    ranking = {"test_queries": queries, "top": tops, "configs": configs, "replies": replies,
               "table": {m: floats(table.loc[m].to_dict()) for m in table.index}, "columns": list(table.columns),
               "coverage": cov}
    out = {"n_index": N_INDEX, "numpy": np.__version__, "cases": cases, "ranking": ranking}
    small = cases_file.compact(out)
    (HERE / "ir_metrics.json").write_text(cases_file.dumps(small))
    (HERE / "benchmark_configs.json").write_text(
        "{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(c)}" for n, c in configs.items()) + "\n}\n")
    assert cases_file.load() == out, "the compact file does not expand to what the reference was called with"
    print(f"wrote {len(cases)} cases, {len(queries)} ranking queries x {len(configs)} methods")


if __name__ == "__main__":
    main()
