"""evals.py on the CPU: `model_ir_metrics`, `IRMetrics` and `evaluate_ranking_methods` against a run of the reference's own
evals modules (tests/golden/ir_metrics.json, made by make_ir_metrics_golden.py), bit for bit; `LabelSet`'s CSR, n_rel, ideal
DCG and coverage; the two dev-set forms."""
import json
import pathlib

import numpy as np
import pandas as pd
import pytest

import ir_metrics_cases
from review_recommender_amd import evals

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def golden():
    return ir_metrics_cases.load()


def scores_of(case):
    return None if case["relevance_scores"] is None else {s: float(v) for s, v in case["relevance_scores"].items()}


def universe(golden):
    return [f"P{r:05d}" for r in range(golden["n_index"])]


def test_the_fixture_covers_the_cases(golden):
    ids = {c["id"] for c in golden["cases"]}
    assert len(golden["cases"]) == len(ids) >= 200
    assert {c["k"] for c in golden["cases"]} == {1, 4, 5, 7, 8, 9, 10, 19, 20, 50, 65, 130}
    for name in ("no_labels", "all_absent", "hit_rank_1", "hit_rank_k", "no_hit", "graded_int", "graded_fraction",
                 "scores_outside_relevant", "one_entry", "segment_300"):
        assert f"{name}@10" in ids and f"{name}@130" in ids
    assert "hit_beyond_64@65" in ids and "hit_beyond_64@130" in ids
    by_id = {c["id"]: c for c in golden["cases"]}
    assert len(by_id["segment_300@20"]["relevant_items"]) == 300
    c = by_id["hit_beyond_64@130"]
    assert c["retrieved"].index(c["relevant_items"][0]) >= 64 and float(c["metrics"]["mrr"]) > 0
    c = by_id["scores_outside_relevant@10"]
    assert set(c["relevance_scores"]) - set(c["relevant_items"]) and set(c["relevant_items"]) - set(c["relevance_scores"])


def test_model_equals_the_reference_bitwise(golden):
    for case in golden["cases"]:
        got = evals.model_ir_metrics(case["retrieved"], case["relevant_items"], scores_of(case))
        assert tuple(got) == evals.COLUMNS
        for name, want in case["metrics"].items():
            assert repr(got[name]) == want, (case["id"], name, got[name], want)
        first = next((i + 1 for i, s in enumerate(case["retrieved"]) if s in set(case["relevant_items"])), 0)
        assert got["first_hit"] == float(first) and got["mrr"] == (1.0 / first if first else 0.0)


def test_irmetrics_class_equals_the_reference_bitwise(golden):
    ev = evals.IRMetrics()
    for case in golden["cases"][::7]:
        got = ev.evaluate_query(case["id"], case["retrieved"], set(case["relevant_items"]), scores_of(case))
        assert list(got) == list(case["metrics"])                      # the reference's seven, in its order
        assert {n: repr(v) for n, v in got.items()} == case["metrics"]
    report = ev.detailed_report()
    assert list(report.index) == [c["id"] for c in golden["cases"][::7]] and list(report.columns) == list(evals.METRIC_NAMES)
    agg = ev.aggregate_metrics()
    for name in evals.METRIC_NAMES:
        assert agg[name] == np.mean([float(c["metrics"][name]) for c in golden["cases"][::7]])
    assert evals.IRMetrics().aggregate_metrics() == {} and evals.IRMetrics().detailed_report().empty


def test_evaluate_ranking_methods_equals_the_reference_bitwise(golden):
    r = golden["ranking"]
    configs = r["configs"]
    assert configs == evals.BENCHMARK_CONFIGS == json.loads((GOLDEN / "benchmark_configs.json").read_text())
    calls = []

    def stub(query, **config):
        name = next(n for n, c in configs.items() if c == config)
        calls.append((name, query))
        skus = r["replies"][name][query]
        if skus is None:
            raise RuntimeError("stub failure")
        return pd.DataFrame({"sku": skus}), {}, {}

    queries = [dict(q, relevant_items=set(q["relevant_items"])) for q in r["test_queries"]]
    table = evals.evaluate_ranking_methods(stub, queries, configs)
    assert len(calls) == len(queries) * len(configs)                   # one search per query and method
    assert list(table.index) == list(r["table"]) and list(table.columns) == r["columns"]
    for method, row in r["table"].items():
        assert {n: repr(float(table.loc[method, n])) for n in row} == row, method
    assert any(v is None for v in r["replies"]["Hybrid"].values())     # the failing query was left out, as in the reference


def test_label_set_csr(golden):
    skus = universe(golden)
    row_of = {s: i for i, s in enumerate(skus)}
    cases = golden["cases"]
    queries = [{"id": c["id"], "query": c["id"], "relevant_items": c["relevant_items"], "relevance_scores": scores_of(c)}
               for c in cases]
    labels = evals.LabelSet.from_queries(queries, skus)
    assert len(labels) == len(cases) and labels.lab_off[0] == 0 and labels.lab_off[-1] == len(labels.lab_row)
    assert labels.lab_off.dtype == np.int64 and labels.lab_row.dtype == np.int64 and labels.lab_grade.dtype == np.float64
    assert labels.lab_rel.dtype == np.uint8 and labels.n_rel.dtype == np.int32 and labels.idcg.shape == (len(cases), 2)
    for b, c in enumerate(cases):
        lo, hi = labels.lab_off[b], labels.lab_off[b + 1]
        rows = labels.lab_row[lo:hi]
        assert (np.diff(rows) > 0).all()                               # ascending, no row twice
        relevant, scores = set(c["relevant_items"]), scores_of(c)
        grades = scores if scores is not None else {s: 1.0 for s in relevant}
        want = sorted(row_of[s] for s in set(grades) | relevant if s in row_of)
        assert rows.tolist() == want
        for row, grade, rel in zip(rows, labels.lab_grade[lo:hi], labels.lab_rel[lo:hi]):
            assert grade == grades.get(skus[row], 0.0) and rel == (skus[row] in relevant)
        assert labels.n_rel[b] == len(relevant)                        # absent skus count
        ideal = sorted(grades.values(), reverse=True)
        assert labels.idcg[b, 0] == evals.model_dcg(ideal, 5) and labels.idcg[b, 1] == evals.model_dcg(ideal, 10)
    by_id = {c["id"]: b for b, c in enumerate(cases)}
    b = by_id["all_absent@10"]
    assert labels.lab_off[b] == labels.lab_off[b + 1] and labels.n_rel[b] == 3 and labels.idcg[b, 1] > 0
    b = by_id["no_labels@10"]
    assert labels.lab_off[b] == labels.lab_off[b + 1] and labels.n_rel[b] == 0 and labels.idcg[b, 1] == 0
    assert labels.lab_off[by_id["segment_300@20"] + 1] - labels.lab_off[by_id["segment_300@20"]] == 300
    assert labels.lab_off[by_id["one_entry@20"] + 1] - labels.lab_off[by_id["one_entry@20"]] == 1


def test_coverage_equals_validate_ground_truth(golden):
    r = golden["ranking"]
    labels = evals.LabelSet.from_queries(r["test_queries"], universe(golden))
    got = labels.coverage()
    want = dict(r["coverage"], coverage_rate=float(r["coverage"]["coverage_rate"]))
    assert got == want and 0 < got["coverage_rate"] < 1 and got["missing_by_query"]


def test_both_devset_forms_parse_to_the_same_labels(golden, tmp_path):
    r = golden["ranking"]
    skus = universe(golden)
    dicts = [dict(q, id=q.get("id", q["query"])) for q in r["test_queries"]]
    lines = [{"query": q["query"], "relevant": q["relevant_items"]} for q in r["test_queries"]]
    a = evals.LabelSet.from_queries([dict(q, id=q["query"]) for q in dicts], skus)
    b = evals.LabelSet.from_queries(lines, skus)
    path = tmp_path / "dev.jsonl"
    path.write_text("\n".join(json.dumps(line) for line in lines) + "\n")
    c = evals.LabelSet.from_queries(evals.load_devset(path), skus)
    (tmp_path / "dev.json").write_text(json.dumps(dicts))
    d = evals.LabelSet.from_queries(evals.load_devset(tmp_path / "dev.json"), skus)
    assert a.ids == b.ids == c.ids == [q["query"] for q in lines] and d.ids == [q["id"] for q in dicts]
    for other in (b, c, d):
        for name in ("lab_off", "lab_row", "lab_grade", "lab_rel", "n_rel", "idcg"):
            assert getattr(a, name).tobytes() == getattr(other, name).tobytes(), name
        assert other.texts == a.texts


def test_what_the_label_set_refuses(golden):
    skus = universe(golden)
    q = [{"id": "a", "query": "x", "relevant_items": ["P00001"]}]
    with pytest.raises(ValueError, match="duplicate skus"):
        evals.LabelSet.from_queries(q, skus + ["P00007"])
    with pytest.raises(ValueError, match="duplicate query ids"):
        evals.LabelSet.from_queries(q + q, skus)
    with pytest.raises(ValueError, match="relevant_items"):
        evals.LabelSet.from_queries([{"query": "x"}], skus)
    with pytest.raises(ValueError, match="'query'"):
        evals.LabelSet.from_queries([{"relevant": []}], skus)


def test_saved_files_have_the_references_layout(golden, tmp_path):
    r = golden["ranking"]
    summary = pd.DataFrame({m: {n: float(v) for n, v in row.items()} for m, row in r["table"].items()}).T
    results = evals.benchmark_results_of(summary, 23)
    assert list(results) == list(r["table"]) + ["_metadata"] and results["_metadata"]["num_queries"] == 23
    assert all(list(results[m]) == ["ndcg@10", "mrr", "recall@20"] for m in r["table"])
    evals.save_benchmark_results(results, summary, tmp_path / "out")
    assert json.loads((tmp_path / "out" / "benchmark_results.json").read_text()) == results
    back = pd.read_csv(tmp_path / "out" / "detailed_results.csv", index_col=0)
    assert list(back.index) == list(summary.index) and list(back.columns) == list(summary.columns)
    table = (tmp_path / "out" / "readme_table.md").read_text()
    assert table.startswith("# Performance Metrics\n\n| Metric | Dense Only | BM25 Only | Hybrid | Hybrid + Rerank |\n")
    assert f"| nDCG@10 | {summary.loc['Dense Only', 'ndcg@10']:.3f} |" in table and "| MRR@10 |" in table and "| Recall@20 |" in table
