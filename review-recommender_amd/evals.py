"""Evaluation of ranking configurations: the reference's ``evals/`` interface and its batched form on the GPU.

Boundary kept:
  IRMetrics.evaluate_query / aggregate_metrics / detailed_report      evals/performance_metrics.py:156-235
  evaluate_ranking_methods(search_function, test_queries, configs)    evals/performance_metrics.py:238-281
  BENCHMARK_CONFIGS, validate_ground_truth                            evals/test_queries.py:147-188, 255-312
  save_benchmark_results' three files                                 evals/run_benchmark.py:158-230

`model_ir_metrics` is the numpy statement of `evaluate_query` -- the CPU model of csrc/rr_evals.hip and what the host uses
for the ideal DCG; `IRMetrics` and `evaluate_ranking_methods` are computed by it (pinned to a run of the reference's own
module: tests/golden/ir_metrics.json).  `LabelSet` turns a dev set into the CSR the kernel reads; `SearchEngine.evaluate`
(`evaluate_engine` here) searches the labelled queries in batches, shares every stage the fusion weights do not touch among
the configurations, and leaves only the (Q, 8) metric tables on the device to be read.

    python -m review_recommender_amd.evals --data-dir D --devset FILE [--configs FILE.json] --out DIR
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import pathlib
import sys
from datetime import datetime
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import pandas as pd

logger = logging.getLogger(__name__)

METRIC_NAMES = ("ndcg@5", "ndcg@10", "mrr", "recall@10", "recall@20", "precision@5", "precision@10")
COLUMNS = METRIC_NAMES + ("first_hit",)                 # rr_ir_metrics_dev's d_metrics, in this order
LOG2_TABLE = np.log2(np.arange(1, 11) + 1)              # the discounts of ranks 1 .. 10 (uploaded: d_log2)
KEY_METRICS = ("ndcg@10", "mrr", "recall@20")           # evals/run_benchmark.py:130
MAX_BATCH = 1024                                        # include/rr_hip.h: RR_MAX_BATCH

# evals/test_queries.py:255-312, as settings data (tests/golden/benchmark_configs.json is the same table)
BENCHMARK_CONFIGS = {
    name: dict(k=k, rerank_k=rr, w_dense=wd, w_bm25=wb, w_rerank=wr, w_prior=wp, w_best=0.0, prior_C=20.0, use_snips=False,
               max_scan=50000, min_reviews=mr, gate_penalty=gp)
    for name, k, rr, wd, wb, wr, wp, mr, gp in (("Dense Only", 20, 0, 1.0, 0.0, 0.0, 0.0, 1, 0.0),
                                                ("BM25 Only", 20, 0, 0.0, 1.0, 0.0, 0.0, 1, 0.0),
                                                ("Hybrid", 20, 0, 0.5, 0.3, 0.0, 0.2, 5, 0.3),
                                                ("Hybrid + Rerank", 50, 20, 0.4, 0.2, 0.3, 0.1, 5, 0.5))}


# ------------------------------------------------------------------------------------------------- the model
def model_dcg(grades: Sequence[float], c: int) -> float:
    """DCG at cut-off ``c`` <= 10 as numpy computes ``np.sum(rel / np.log2(ranks + 1))`` on a contiguous float64 array: one
    division per term, the terms added left to right from 0.0 below eight of them, else
    ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)) and the tail one by one."""
    if c > len(LOG2_TABLE):
        raise ValueError(f"the discount table holds {len(LOG2_TABLE)} ranks")
    t = [float(np.float64(g) / LOG2_TABLE[i]) for i, g in enumerate(list(grades)[:max(c, 0)])]
    if len(t) < 8:
        res = 0.0
        for x in t:
            res += x
    else:
        res = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))
        for x in t[8:]:
            res += x
    return 0.0 + res


def model_ir_metrics(retrieved_skus: Sequence, relevant_items: Iterable, relevance_scores: Optional[Dict] = None) -> Dict[str, float]:
    """IRMetrics.evaluate_query in plain Python floats: the seven metrics of the reference plus ``first_hit`` (the 1-based
    rank of the first retrieved item that is in ``relevant_items``, 0.0 when there is none; mrr is its reciprocal)."""
    retrieved = list(retrieved_skus)
    relevant = set(relevant_items)
    scores = {s: 1.0 for s in relevant} if relevance_scores is None else relevance_scores
    grades = [float(scores.get(s, 0.0)) for s in retrieved]
    ideal = sorted((float(v) for v in scores.values()), reverse=True)
    out = {}
    for c in (5, 10):
        idcg = model_dcg(ideal, c)
        out[f"ndcg@{c}"] = 0.0 if idcg == 0.0 else model_dcg(grades, c) / idcg
    first = next((i + 1 for i, s in enumerate(retrieved) if s in relevant), 0)
    out["mrr"] = 1.0 / first if first else 0.0
    hits = lambda c: len(set(retrieved[:c]) & relevant)
    for c in (10, 20):
        out[f"recall@{c}"] = hits(c) / len(relevant) if relevant else 0.0
    for c in (5, 10):
        top = retrieved[:c]
        out[f"precision@{c}"] = hits(c) / len(top) if top else 0.0
    out["first_hit"] = float(first)
    return {name: float(out[name]) for name in COLUMNS}


class IRMetrics:
    """The reference's per-query evaluator (evals/performance_metrics.py:156-235), computed by `model_ir_metrics`."""

    def __init__(self):
        self.results: Dict[str, Dict[str, float]] = {}

    def evaluate_query(self, query_id, retrieved_items, relevant_items, relevance_scores=None) -> Dict[str, float]:
        full = model_ir_metrics(retrieved_items, relevant_items, relevance_scores)
        metrics = {name: full[name] for name in METRIC_NAMES}
        self.results[query_id] = metrics
        return metrics

    def aggregate_metrics(self) -> Dict[str, float]:
        if not self.results:
            return {}
        rows = list(self.results.values())
        return {name: np.mean([r[name] for r in rows]) for name in rows[0]}

    def detailed_report(self) -> pd.DataFrame:
        if not self.results:
            return pd.DataFrame()
        return pd.DataFrame.from_dict(self.results, orient="index")


def evaluate_ranking_methods(search_function, test_queries: List[Dict], method_configs: Dict[str, Dict], *,
                             graded: bool = False) -> pd.DataFrame:
    """Methods x metrics: per configuration ``search_function(query, **config)`` for every test query, one query at a time,
    the means of `IRMetrics`.  As in the reference a query whose search raises is logged and left out, and the labels are
    BINARY: a query's ``relevance_scores`` are not read unless ``graded`` (this build's addition; `SearchEngine.evaluate`
    grades with them, so it equals this function with ``graded=True`` -- and with the default on a dev set without
    relevance_scores)."""
    results = {}
    for name, config in method_configs.items():
        logger.info("Evaluating method: %s", name)
        evaluator = IRMetrics()
        for qd in test_queries:
            query = qd["query"]
            try:
                frame, _, _ = search_function(query, **config)
                evaluator.evaluate_query(qd.get("id", query), frame["sku"].tolist(), set(qd["relevant_items"]),
                                         qd.get("relevance_scores") if graded else None)
            except Exception as e:
                logger.error("Error evaluating query '%s' with method '%s': %s", query, name, e)
        results[name] = evaluator.aggregate_metrics()
    return pd.DataFrame(results).T


# ------------------------------------------------------------------------------------------------- the labels
def _normalise_query(qd: Dict) -> Dict:
    """One dev-set entry in the evals form.  The app tab's JSONL line ``{"query", "relevant"}`` becomes
    ``{"id": query, "query", "relevant_items"}``."""
    if "query" not in qd:
        raise ValueError(f"a dev-set entry needs a 'query': {qd!r}")
    if "relevant_items" in qd:
        relevant = qd["relevant_items"]
    elif "relevant" in qd:
        relevant = qd["relevant"]
    else:
        raise ValueError(f"a dev-set entry needs 'relevant_items' (or the JSONL form's 'relevant'): {qd!r}")
    out = {"id": qd.get("id", qd["query"]), "query": qd["query"], "relevant_items": {str(s) for s in relevant}}
    if qd.get("relevance_scores") is not None:
        out["relevance_scores"] = {str(s): float(v) for s, v in qd["relevance_scores"].items()}
    return out


def load_devset(path) -> List[Dict]:
    """A dev set from a file: JSON lines (one entry per line, either form) or one JSON list of entries."""
    text = pathlib.Path(path).read_text(encoding="utf-8")
    try:
        data = json.loads(text)
        entries = data if isinstance(data, list) else [data]
    except json.JSONDecodeError:
        entries = [json.loads(line) for line in text.splitlines() if line.strip()]
    return [_normalise_query(e) for e in entries]


class LabelSet:
    """A dev set against one index: per query its labelled rows as a CSR (rows ascending inside a query), ``n_rel`` and the
    ideal DCG -- what rr_ir_metrics_dev reads (include/rr_hip.h).  An entry stands for every sku of ``relevant_items`` or of
    the keys of ``relevance_scores`` that the index holds: its grade is the relevance_scores value (1.0 with binary labels,
    0.0 for a relevant sku the scores leave out), its flag says whether it is in ``relevant_items``.  Skus the index lacks
    have no entry but count in ``n_rel`` and in the ideal DCG, as in the reference."""

    def __init__(self, queries: List[Dict], meta_skus: Sequence):
        skus = [str(s) for s in meta_skus]
        row_of = {s: i for i, s in enumerate(skus)}
        if len(row_of) != len(skus):
            raise ValueError("the metadata holds duplicate skus: a label would be ambiguous")
        self.queries = queries
        self.ids = [q["id"] for q in queries]
        if len(set(self.ids)) != len(self.ids):
            raise ValueError("the dev set holds duplicate query ids: the reference's report keeps one row per id")
        self.texts = [q["query"] for q in queries]
        self._available = set(row_of)
        Q = len(queries)
        self.lab_off = np.zeros(Q + 1, dtype=np.int64)
        self.n_rel = np.zeros(Q, dtype=np.int32)
        self.idcg = np.zeros((Q, 2), dtype=np.float64)
        rows, grades, rels = [], [], []
        for b, q in enumerate(queries):
            relevant = q["relevant_items"]
            scores = q.get("relevance_scores")
            if scores is None:
                scores = {s: 1.0 for s in relevant}
            entries = sorted((row_of[s], float(scores.get(s, 0.0)), s in relevant)
                             for s in set(scores) | relevant if s in row_of)
            rows += [e[0] for e in entries]
            grades += [e[1] for e in entries]
            rels += [e[2] for e in entries]
            self.lab_off[b + 1] = len(rows)
            self.n_rel[b] = len(relevant)
            ideal = sorted((float(v) for v in scores.values()), reverse=True)
            self.idcg[b] = model_dcg(ideal, 5), model_dcg(ideal, 10)
        self.lab_row = np.asarray(rows, dtype=np.int64)
        self.lab_grade = np.asarray(grades, dtype=np.float64)
        self.lab_rel = np.asarray(rels, dtype=np.uint8)

    @classmethod
    def from_queries(cls, test_queries: Iterable[Dict], meta_skus: Sequence) -> "LabelSet":
        """``test_queries``: the evals dicts (``id``, ``query``, ``relevant_items``, optional ``relevance_scores``) or the app
        tab's JSONL lines (``query``, ``relevant``), in any mix."""
        return cls([_normalise_query(q) for q in test_queries], meta_skus)

    def __len__(self) -> int:
        return len(self.queries)

    def coverage(self) -> Dict:
        """What validate_ground_truth returns for this dev set (evals/test_queries.py:147-188); the missing skus sorted."""
        total = found = 0
        missing = {}
        for q in self.queries:
            relevant = q["relevant_items"]
            total += len(relevant)
            found += len(relevant & self._available)
            if relevant - self._available:
                missing[q["id"]] = sorted(relevant - self._available)
        return {"total_queries": len(self.queries), "total_relevant_items": total, "found_relevant_items": found,
                "coverage_rate": found / total if total > 0 else 0.0, "missing_by_query": missing}

    def upload(self, device) -> "DeviceLabels":
        return DeviceLabels(self, device)


class DeviceLabels:
    """A LabelSet's arrays on one device, and the metrics kernel over them."""

    def __init__(self, labels: LabelSet, device):
        import torch
        from . import _lib
        self.lib = _lib.load()
        self.labels = labels
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.lab_off, self.lab_row, self.lab_grade = up(labels.lab_off), up(labels.lab_row), up(labels.lab_grade)
        self.lab_rel, self.n_rel, self.idcg, self.log2 = up(labels.lab_rel), up(labels.n_rel), up(labels.idcg), up(LOG2_TABLE)

    def metrics(self, out_rows, order, first: int = 0, out=None, mean=None):
        """rr_ir_metrics_dev over K3's (B, pool) rows and (B, k) order for the queries [first, first + B) of the label set,
        queued on the current stream: the (B, 8) float64 table (written into ``out`` if given), and the column means into
        ``mean`` (8,) if given."""
        import torch
        from . import _lib
        B, pool = out_rows.shape
        k = order.shape[1]
        if order.shape[0] != B or first < 0 or first + B > len(self.labels):
            raise ValueError(f"{B} x {pool} rows and {tuple(order.shape)} order for queries [{first}, {first + B}) of "
                             f"{len(self.labels)}")
        if out_rows.dtype != torch.int64 or order.dtype != torch.int32 or not out_rows.is_contiguous() or not order.is_contiguous():
            raise ValueError("out_rows must be contiguous int64 and order contiguous int32, as K3 writes them")
        if out is None:
            out = torch.empty((B, len(COLUMNS)), dtype=torch.float64, device=self.device)
        lo, hi = int(self.labels.lab_off[first]), int(self.labels.lab_off[first + B])
        with torch.cuda.device(self.device):
            off = self.lab_off[first:first + B + 1]
            if lo:
                off = off - lo
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
            _lib.check(self.lib.rr_ir_metrics_dev(
                p(out_rows), p(order), B, pool, k, p(off), p(self.lab_row[lo:hi]), p(self.lab_grade[lo:hi]), p(self.lab_rel[lo:hi]),
                hi - lo, p(self.n_rel[first:first + B]), p(self.idcg[first:first + B]), p(self.log2), p(out), p(mean),
                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "rr_ir_metrics_dev")
        return out

    def mean(self, table):
        """The column means of a (Q, 8) metrics table (rr_ir_mean_dev), an (8,) float64 device tensor."""
        import torch
        from . import _lib
        out = torch.empty((len(COLUMNS),), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rr_ir_mean_dev(C.c_void_p(table.data_ptr()), table.shape[0], C.c_void_p(out.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "rr_ir_mean_dev")
        return out


# ------------------------------------------------------------------------------------------------- the engine
class EvalReport:
    """`SearchEngine.evaluate`'s answer.  ``metrics_dev[method]``: the (Q, 8) float64 table on the device (`COLUMNS`);
    ``summary``: methods x the reference's seven metrics, what `evaluate_ranking_methods` returns; ``detailed(method)``: the
    per-query frame (index = the query ids, the eight columns), downloaded when asked for."""

    def __init__(self, labels: LabelSet, metrics_dev: Dict, means: Dict):
        self.labels, self.metrics_dev = labels, metrics_dev
        self.summary = pd.DataFrame({m: dict(zip(COLUMNS, v.cpu().numpy().tolist())) for m, v in means.items()}).T
        self.summary = self.summary[list(METRIC_NAMES)] if len(self.summary) else self.summary

    def detailed(self, method: str) -> pd.DataFrame:
        return pd.DataFrame(self.metrics_dev[method].cpu().numpy(), index=self.labels.ids, columns=list(COLUMNS))


_CONFIG_KEYS = ("k", "rerank_k", "w_dense", "w_bm25", "w_rerank", "w_prior", "w_best", "prior_C")
_CONFIG_DEFAULTS = {"use_snips": False, "max_scan": 0, "min_reviews": 8, "gate_penalty": 0.5}     # run_search's own


def _config(name: str, config: Dict) -> Dict:
    """A method's configuration as run_search reads its keyword arguments."""
    unknown = set(config) - set(_CONFIG_KEYS) - set(_CONFIG_DEFAULTS)
    missing = [key for key in _CONFIG_KEYS if key not in config]
    if unknown or missing:
        raise ValueError(f"method {name!r}: " + (f"unknown run_search arguments {sorted(unknown)}" if unknown else
                                                  f"run_search arguments {missing} are missing"))
    return dict(_CONFIG_DEFAULTS, **config)


def evaluate_engine(engine, test_queries, method_configs: Dict[str, Dict], *, qvecs=None, batch: int = MAX_BATCH) -> EvalReport:
    """`SearchEngine.evaluate` (see there)."""
    import torch
    from .engine import APP_POOL_FLOOR, APP_TRUST_SAT, CLI_POOL_FLOOR, FusionWeights
    from . import text

    labels = test_queries if isinstance(test_queries, LabelSet) else \
        LabelSet.from_queries(test_queries, engine.meta["sku"].astype(str).tolist())
    configs = {name: _config(name, c) for name, c in method_configs.items()}
    Q = len(labels)
    if Q == 0 or not configs:
        raise ValueError("evaluate needs at least one labelled query and one configuration")
    if not 1 <= batch <= MAX_BATCH:
        raise ValueError(f"batch must be 1 .. {MAX_BATCH}")
    if qvecs is None and engine.encoder is None:
        raise ValueError("no query encoder was given; pass qvecs")
    if qvecs is not None:
        qvecs = np.asarray(qvecs, dtype=np.float32)
        if qvecs.shape[0] != Q:
            raise ValueError(f"{qvecs.shape[0]} query vectors for {Q} queries")
    searcher = engine.searcher
    dev_labels = labels.upload(searcher.device)
    app = engine.flavour == "app"
    floor = APP_POOL_FLOOR if app else CLI_POOL_FLOOR
    weights = {name: FusionWeights(c["w_dense"], c["w_bm25"], c["w_rerank"], c["w_prior"], c["w_best"], c["prior_C"],
                                   c["min_reviews"], c["gate_penalty"], APP_TRUST_SAT, app) for name, c in configs.items()}
    tables = {name: torch.empty((Q, len(COLUMNS)), dtype=torch.float64, device=searcher.device) for name in configs}
    device_gate, device_rerank = searcher.gate_text is not None, searcher.rerank_text is not None

    def host_text(qs):
        return {"toks": [text.tokenize_query(q) for q in qs], "groups": [text.build_gate_groups(q) for q in qs]}

    def search_configs(qs, qv, fronts, made):
        """Every configuration over one batch of queries: per method the DeviceBatch K3 left.  ``fronts``: gate penalty ->
        the batch's QueryFront (query_text="device"), or None: the host's tokens and groups in ``made`` are used, as
        run_search_batch's host path uses them.  What does not depend on the weights is made once: the arguments here, the
        kernels' outputs in ``shared`` (HybridSearcher.search_batch_dev)."""
        shared, rerank_args, gate_args = {}, {}, {}
        term_ids = None
        if fronts is None and searcher.bm25 is not None:
            term_ids = [searcher.bm25.term_ids(t) for t in made["toks"]]
        out = {}
        for name, c in configs.items():
            rerank_k, pen = c["rerank_k"], c["gate_penalty"]
            args = {}
            if fronts is None or not device_gate:                  # (the host gate, or the device gate over host-packed groups)
                if pen not in gate_args:
                    gate_args[pen] = engine._gate_args(made["groups"], pen)
                args.update(gate_args[pen])
            if rerank_k > 0:
                if rerank_k not in rerank_args:
                    if fronts is not None and device_rerank:
                        rerank_args[rerank_k] = {"rerank_pairs": (
                            engine.cross_encoder, None, lambda b, rows: engine._rerank_fn(qs[b:b + 1])(rows[None, :])[0])}
                    else:
                        rerank_args[rerank_k] = engine._rerank_args(qs, rerank_k)
                args.update(rerank_args[rerank_k])
            front = q_in = None
            if fronts is not None:
                front = fronts[pen if device_gate else None]
                q_in = fronts["vectors"].qvecs
            if qv is not None:
                q_in = qv
            out[name] = searcher.search_batch_dev(
                q_in, term_ids, c["k"], rerank_k, weights[name], pool_floor=floor, reviews=engine.reviews if c["use_snips"] else None,
                max_scan=c["max_scan"], bm25_f64=not app, query_front=front, shared=shared, **args)
        return out

    for first in range(0, Q, batch):
        qs = [str(q) for q in labels.texts[first:first + batch]]
        B = len(qs)
        qv = None
        if qvecs is not None:
            qv = qvecs[first:first + B]
        elif engine.query_vectors != "device":
            qv = np.asarray(engine.encoder.encode(qs, normalize_embeddings=True), dtype=np.float32)
        flagged = np.zeros(0, dtype=np.int64)
        if engine._query_text is None:
            answers = search_configs(qs, qv, None, host_text(qs))
        else:
            # one front per gate penalty the device gate reads (its factor table is staged with the bytes); the query vectors
            # are made once, by the first
            pens = list(dict.fromkeys(c["gate_penalty"] for c in configs.values())) if device_gate else [None]
            fronts = {}
            with torch.cuda.device(searcher.device):
                for i, pen in enumerate(pens):
                    fronts[pen] = engine._query_text.front(qs, 0.5 if pen is None else pen, vectors=qv is None and i == 0)
            fronts["vectors"] = fronts[pens[0]]
            made = None if device_gate else host_text(qs)
            answers = search_configs(qs, qv, fronts, made)
            engine._query_text.check()
            if qv is None and engine._query_text.redo_vectors(fronts["vectors"]):
                answers = search_configs(qs, qv, fronts, made)      # (the vectors were made again on the wide-range kernels)
            flagged = np.flatnonzero(fronts["vectors"].needs_host.cpu().numpy())       # (B flags: all that is read back)
        if len(flagged):
            # the queries the front handed back: searched again through the host functions, in one batch of their own, and put
            # in place on the device (as _search_device_text puts them in place on the host)
            sub_qs = [qs[i] for i in flagged]
            sub_qv = qv[flagged] if qv is not None else \
                np.asarray(engine.encoder.encode(sub_qs, normalize_embeddings=True), dtype=np.float32)
            sub = search_configs(sub_qs, sub_qv, None, host_text(sub_qs))
            at = torch.from_numpy(flagged).to(searcher.device)
            for name in configs:
                answers[name].pool_rows.index_copy_(0, at, sub[name].pool_rows)
                answers[name].order.index_copy_(0, at, sub[name].order)
        for name in configs:
            dev_labels.metrics(answers[name].pool_rows, answers[name].order, first, out=tables[name][first:first + B])
    means = {name: dev_labels.mean(tables[name]) for name in configs}
    return EvalReport(labels, tables, means)


# ------------------------------------------------------------------------------------------------- the command line
def format_results_for_readme(benchmark_results: Dict) -> str:
    """evals/run_benchmark.py:158-198: the README's table, one column per method of the results."""
    methods = [m for m in benchmark_results if m != "_metadata"]
    if not methods or "_metadata" not in benchmark_results:
        return "No benchmark results available"
    table = "| Metric | " + " | ".join(methods) + " |\n"
    table += "|--------|" + "|".join("-" * (len(m) + 2) for m in methods) + "|\n"
    for key, shown in (("ndcg@10", "nDCG@10"), ("mrr", "MRR@10"), ("recall@20", "Recall@20")):
        table += f"| {shown} |" + "".join(f" {benchmark_results[m].get(key, 0.0):.3f} |" for m in methods) + "\n"
    return table


def save_benchmark_results(benchmark_results: Dict, results_df: pd.DataFrame, output_dir) -> None:
    """benchmark_results.json, detailed_results.csv and readme_table.md in the layout of evals/run_benchmark.py:201-230."""
    out = pathlib.Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / "benchmark_results.json", "w") as f:
        json.dump(benchmark_results, f, indent=2)
    results_df.to_csv(out / "detailed_results.csv")
    with open(out / "readme_table.md", "w") as f:
        f.write("# Performance Metrics\n\n")
        f.write(format_results_for_readme(benchmark_results))
        f.write(f"\n\n*Generated on {datetime.now().strftime('%Y-%m-%d %H:%M:%S')}*\n")


def benchmark_results_of(summary: pd.DataFrame, n_queries: int, config_file: str = "default") -> Dict:
    """The summary dictionary run_performance_benchmark builds (evals/run_benchmark.py:129-148)."""
    results = {m: {key: float(summary.loc[m, key]) if key in summary.columns else 0.0 for key in KEY_METRICS}
               for m in summary.index}
    results["_metadata"] = {"timestamp": datetime.now().isoformat(), "num_queries": int(n_queries), "config_file": config_file,
                            "data_files_checked": True}
    return results


def main(argv=None) -> int:
    import argparse
    from .cli import _load_encoders
    ap = argparse.ArgumentParser(prog="python -m review_recommender_amd.evals",
                                 description="Evaluate ranking configurations on a labelled dev set, on the GPU")
    ap.add_argument("--data-dir", required=True, help="directory with the three artefacts")
    ap.add_argument("--devset", required=True, help="JSON lines {query, relevant} or the evals dicts (a JSON list)")
    ap.add_argument("--configs", default="", help="JSON file {method: run_search keyword arguments}; default: BENCHMARK_CONFIGS")
    ap.add_argument("--out", required=True, help="directory for benchmark_results.json, detailed_results.csv, readme_table.md")
    ap.add_argument("--qvecs-npy", default="", help=".npy with one query embedding per dev-set entry (offline use)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emb-model-dir", default="")
    ap.add_argument("--rerank-model-dir", default="")
    ap.add_argument("--ce-precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--gate", choices=["host", "device"], default="device")
    ap.add_argument("--query-text", choices=["host", "device"], default="device")
    ap.add_argument("--flavour", choices=["app", "cli"], default="app")
    ap.add_argument("--allow-hub", action="store_true")
    args = ap.parse_args(argv)
    from .artifacts import ArtifactError
    from .engine import SearchEngine
    devset = load_devset(args.devset)
    configs = json.loads(pathlib.Path(args.configs).read_text()) if args.configs else BENCHMARK_CONFIGS
    qvecs = np.load(args.qvecs_npy).astype(np.float32) if args.qvecs_npy else None
    enc, ce = _load_encoders(args) if (qvecs is None or args.rerank_model_dir) else (None, None)
    if qvecs is None and enc is None:
        raise SystemExit("[ERR] no query encoder; pass --emb-model-dir or --qvecs-npy (or opt in to the hub loader with --allow-hub)")
    try:
        engine = SearchEngine.from_artifacts(args.data_dir, encoder=enc, cross_encoder=ce, flavour=args.flavour, device=args.device,
                                             gate=args.gate, query_text=args.query_text)
    except ArtifactError as e:
        raise SystemExit(f"[ERR] {e}")
    labels = LabelSet.from_queries(devset, engine.meta["sku"].astype(str).tolist())
    cov = labels.coverage()
    print(f"Ground truth validation: {cov['coverage_rate']:.2%} coverage "
          f"({cov['found_relevant_items']} of {cov['total_relevant_items']} labelled skus are in the index)")
    report = engine.evaluate(labels, configs, qvecs=qvecs)
    results = benchmark_results_of(report.summary, len(labels), args.configs or "default")
    print(format_results_for_readme(results))
    save_benchmark_results(results, report.summary, args.out)
    print(f"[ok] wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
