"""tests/golden/ir_metrics.json in its compact form and back (the file is written by golden/make_ir_metrics_golden.py).

A sku is stored as an integer: row r of the synthetic index "P%05d" % r as r, a sku no index holds "Z%04d" % x as -(x + 1).
The retrieved list is stored once per k; a case is [name, k, relevant codes, null | [[code, repr(grade)], ...], the seven
metrics by repr]; the ranking part stores per query its 60 candidate rows and per method the positions the stub replies with
(null = the stub raises).  `expand` gives the dictionaries the reference was called with, `compact` is its inverse."""
import json
import pathlib

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
METRICS = ("ndcg@5", "ndcg@10", "mrr", "recall@10", "recall@20", "precision@5", "precision@10")


def sku(code):
    return f"P{code:05d}" if code >= 0 else f"Z{-code - 1:04d}"


def code(s):
    return int(s[1:]) if s[0] == "P" else -int(s[1:]) - 1


def compact(full):
    retrieved, cases = {}, []
    for c in full["cases"]:
        rows = [code(s) for s in c["retrieved"]]
        assert retrieved.setdefault(str(c["k"]), rows) == rows and c["id"].endswith(f"@{c['k']}")
        scores = None if c["relevance_scores"] is None else [[code(s), v] for s, v in c["relevance_scores"].items()]
        cases.append([c["id"].rsplit("@", 1)[0], c["k"], [code(s) for s in c["relevant_items"]], scores,
                      [c["metrics"][m] for m in METRICS]])
    r = full["ranking"]
    queries, perms = [], {m: [] for m in r["replies"]}
    for q, top in zip(r["test_queries"], r["top"]):
        queries.append([q.get("id"), [code(s) for s in q["relevant_items"]], top])
        at = {sku(row): j for j, row in enumerate(top)}
        for m, replies in r["replies"].items():
            perms[m].append(None if replies[q["query"]] is None else [at[s] for s in replies[q["query"]]])
    cov = dict(r["coverage"], missing_by_query={q: [code(s) for s in v] for q, v in r["coverage"]["missing_by_query"].items()})
    return {"n_index": full["n_index"], "numpy": full["numpy"], "retrieved": retrieved, "cases": cases,
            "ranking": {"queries": queries, "perms": perms, "table": {m: [row[c] for c in METRICS] for m, row in r["table"].items()},
                        "coverage": cov}}


def expand(small):
    cases = []
    for name, k, relevant, scores, metrics in small["cases"]:
        cases.append({"id": f"{name}@{k}", "k": k, "retrieved": [sku(r) for r in small["retrieved"][str(k)]],
                      "relevant_items": [sku(c) for c in relevant],
                      "relevance_scores": None if scores is None else {sku(c): v for c, v in scores},
                      "metrics": dict(zip(METRICS, metrics))})
    r = small["ranking"]
    queries, replies = [], {m: {} for m in r["perms"]}
    for i, (qid, relevant, top) in enumerate(r["queries"]):
        q = {"query": f"query number {i}", "relevant_items": [sku(c) for c in relevant]}
        queries.append(q if qid is None else dict(id=qid, **q))
        for m, perms in r["perms"].items():
            replies[m][q["query"]] = None if perms[i] is None else [sku(top[j]) for j in perms[i]]
    cov = dict(r["coverage"], missing_by_query={q: [sku(c) for c in v] for q, v in r["coverage"]["missing_by_query"].items()})
    return {"n_index": small["n_index"], "numpy": small["numpy"], "cases": cases,
            "ranking": {"test_queries": queries, "top": [q[2] for q in r["queries"]], "replies": replies,
                        "configs": json.loads((GOLDEN / "benchmark_configs.json").read_text()),
                        "table": {m: dict(zip(METRICS, row)) for m, row in r["table"].items()}, "columns": list(METRICS),
                        "coverage": cov}}


def dumps(small):
    """One case, one query, one list per line."""
    line = lambda x: json.dumps(x, separators=(",", ":"))
    r = small["ranking"]
    parts = [f'"n_index":{small["n_index"]},"numpy":{line(small["numpy"])}',
             '"retrieved":{\n' + ",\n".join(f'"{k}":{line(v)}' for k, v in small["retrieved"].items()) + "}",
             '"cases":[\n' + ",\n".join(line(c) for c in small["cases"]) + "]",
             '"ranking":{"queries":[\n' + ",\n".join(line(q) for q in r["queries"]) + '],\n"perms":{\n'
             + ",\n".join(f"{line(m)}:{line(v)}" for m, v in r["perms"].items()) + '},\n"table":' + line(r["table"])
             + ',\n"coverage":' + line(r["coverage"]) + "}"]
    return "{" + ",\n".join(parts) + "}\n"


def load():
    return expand(json.loads((GOLDEN / "ir_metrics.json").read_text()))
