"""`SearchEngine.evaluate` (evals.py, csrc/rr_evals.hip) against `run_search_batch` + the CPU model: per configuration the
per-query table equals `model_ir_metrics` over the sku lists `run_search_batch` returns with the same arguments, bit for
bit, and the summary equals the model's `evaluate_ranking_methods` within the mean's bound (nq * 2^-52 relative) -- for the
gate, the reranker and the query text on the device and on the host, for the CLI flavour, with flagged queries, with
review snippets and with the query vectors made on the device.  Nothing but the metrics comes back to the host, and a sweep
runs every stage the weights do not touch once."""
import numpy as np
import pandas as pd
import pytest

import cli_worlds as W

pytestmark = pytest.mark.gpu

N = 3000
NQ = 70            # more than 64 queries, and no multiple of the metrics kernel's four queries per workgroup
ABSENT = "NOT-IN-THE-INDEX"
LABEL_RANKS = (1, 4, 12, 19, 30)
GRADES = (3.0, 2.5, 1.0, 0.5, 2.0)
# more than 1024 bytes, a token of 65 bytes
FLAGGED = ["z" * 1025, "red cat " + "t" * 65]


@pytest.fixture(scope="module")
def world():
    from review_recommender_amd import evals, synth
    from review_recommender_amd.cross_encoder import CrossEncoder
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(synth.WORDS) + ["for", "the", "of", "and", "red", "cat", "##s", "sock"]
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    texts = synth.text_corpus(N, 3, mean_len=25)
    n_rev, stars = synth.metadata(N, 2)
    meta = pd.DataFrame({"sku": synth.skus(N), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})
    blob = {"skus": meta["sku"].tolist(), "corpus": [t.split() for t in texts]}
    emb = synth.unit_rows(N, W.DIM, 1234)
    rng = np.random.default_rng(81)
    # a query is a few words of one product's text, its vector that product's row plus noise: the dense and the BM25 legs
    # agree on one relevant product, so no configuration's table is all zeros
    source = rng.choice(N, size=NQ - 2, replace=False)
    queries = [" ".join(rng.choice(texts[p].split(), size=int(rng.integers(2, 6)))) for p in source] + ["", "the of"]
    noise = synth.unit_rows(NQ, W.DIM, 99)
    qv = noise.copy()
    qv[:NQ - 2] = emb[source] + 0.6 * noise[:NQ - 2]
    qv /= np.linalg.norm(qv, axis=1, keepdims=True)
    rev = pd.DataFrame({"sku": [meta["sku"][i % N] for i in range(2 * N)], "text": [f"review {i} of it" for i in range(2 * N)],
                        "stars": [float(1 + i % 5) for i in range(2 * N)]})
    sd = synth.bert_state_dict(41, n_layers=2, vocab=len(words))
    w = {"meta": meta, "emb": emb, "blob": blob, "ce": CrossEncoder(sd, tok), "engines": {}, "want": {},
         "reviews": (rev, synth.unit_rows(2 * N, W.DIM, 77)), "queries": queries, "qvecs": qv.astype(np.float32), "evals": evals}
    # the labels: the host engine's own dense-only answer at ranks 1, 4, 12, 19 and 30 and one sku no index holds; every
    # fifth query has none, every third labelled one is graded
    host = engine_of(w, "host", "host", "host")
    dense = host.run_search_batch(queries, qvecs=w["qvecs"], **dict(evals.BENCHMARK_CONFIGS["Dense Only"], k=30))
    test_queries = []
    for i, (q, (frame, _, _)) in enumerate(zip(queries, dense)):
        skus = frame["sku"].tolist()
        picked = [] if i % 5 == 4 else [skus[r - 1] for r in LABEL_RANKS] + [ABSENT]
        qd = {"id": f"q{i:02d}", "query": q, "relevant_items": set(picked)}
        if picked and i % 3 == 0:
            qd["relevance_scores"] = dict(zip(picked, GRADES + (4.0,)))
        test_queries.append(qd)
    w["test_queries"] = test_queries
    return w


def engine_of(world, query_text, gate, rerank, flavour="app"):
    from review_recommender_amd.engine import SearchEngine
    key = (query_text, gate, rerank, flavour)
    if key not in world["engines"]:
        world["engines"][key] = SearchEngine(world["meta"], world["emb"], world["blob"], cross_encoder=world["ce"], flavour=flavour,
                                             gate=gate, rerank=rerank, query_text=query_text, reviews=world["reviews"])
    return world["engines"][key]


def model_tables(evals, engine, test_queries, qvecs, configs):
    """Per method the (Q, 8) table of the model over run_search_batch's sku lists, and the model's summary."""
    queries = [q["query"] for q in test_queries]
    lists, tables = {}, {}
    for name, config in configs.items():
        answers = engine.run_search_batch(queries, qvecs=qvecs, **config)
        lists[name] = {q["query"]: frame["sku"].tolist() for q, (frame, _, _) in zip(test_queries, answers)}
        tables[name] = np.array([[evals.model_ir_metrics(lists[name][q["query"]], q["relevant_items"], q.get("relevance_scores"))[c]
                                  for c in evals.COLUMNS] for q in test_queries])

    def replay(query, **config):
        name = next(n for n, c in configs.items() if c == config)
        return pd.DataFrame({"sku": lists[name][query]}), {}, {}
    return tables, evals.evaluate_ranking_methods(replay, test_queries, configs, graded=True)


def check_report(evals, report, tables, summary, test_queries):
    nq = len(test_queries)
    assert list(report.summary.index) == list(summary.index) and list(report.summary.columns) == list(summary.columns)
    for name, want in tables.items():
        frame = report.detailed(name)
        assert list(frame.index) == [q["id"] for q in test_queries] and list(frame.columns) == list(evals.COLUMNS)
        got = frame.values
        bad = np.flatnonzero((np.ascontiguousarray(got).view(np.uint64) != want.view(np.uint64)).any(axis=1))
        assert len(bad) == 0, (name, [(test_queries[b]["id"], got[b].tolist(), want[b].tolist()) for b in bad[:3]])
        dev = report.metrics_dev[name]
        assert dev.is_cuda and tuple(dev.shape) == (nq, 8) and dev.cpu().numpy().tobytes() == want.tobytes()
        ref = summary.loc[name].values.astype(np.float64)
        assert (np.abs(report.summary.loc[name].values - ref) <= nq * 2.0 ** -52 * np.abs(ref)).all(), (name, report.summary.loc[name], ref)


def reference(world, flavour):
    """The model's tables for the four BENCHMARK_CONFIGS, once per flavour (from the all-host engine)."""
    evals = world["evals"]
    if flavour not in world["want"]:
        host = engine_of(world, "host", "host", "host", flavour)
        world["want"][flavour] = model_tables(evals, host, world["test_queries"], world["qvecs"], evals.BENCHMARK_CONFIGS)
        for name, table in world["want"][flavour][0].items():          # a table of zeros would prove nothing
            mid = (table[:, 1] > 0) & (table[:, 1] < 1)
            assert mid.sum() * 3 >= NQ, (flavour, name, int(mid.sum()))
    return world["want"][flavour]


@pytest.mark.parametrize("variant", [("device", "device", "device", "app"), ("host", "host", "host", "app"),
                                     ("device", "host", "host", "app"), ("host", "device", "device", "app"),
                                     ("device", "device", "device", "cli")], ids="-".join)
def test_evaluate_equals_run_search_batch_and_the_model(world, variant):
    evals = world["evals"]
    tables, summary = reference(world, variant[3])
    report = engine_of(world, *variant).evaluate(world["test_queries"], evals.BENCHMARK_CONFIGS, qvecs=world["qvecs"])
    check_report(evals, report, tables, summary, world["test_queries"])
    assert isinstance(report, evals.EvalReport)


def test_batches_smaller_than_the_query_set(world):
    """The same tables when the queries go through in batches of 32 (three batches, the last of 6)."""
    evals = world["evals"]
    tables, summary = reference(world, "app")
    report = engine_of(world, "device", "device", "device").evaluate(world["test_queries"], evals.BENCHMARK_CONFIGS,
                                                                    qvecs=world["qvecs"], batch=32)
    check_report(evals, report, tables, summary, world["test_queries"])


def test_nothing_is_downloaded_but_the_metrics(world, monkeypatch):
    from review_recommender_amd import engine as E
    evals = world["evals"]
    dev = engine_of(world, "device", "device", "device")

    def boom(*a, **k):
        raise AssertionError("evaluate built a frame or a host BatchResult")
    monkeypatch.setattr(E.SearchEngine, "_frame", boom)
    monkeypatch.setattr(E.BatchResult, "__init__", boom)
    monkeypatch.setattr(E.DeviceBatch, "download", boom)
    report = dev.evaluate(world["test_queries"], evals.BENCHMARK_CONFIGS, qvecs=world["qvecs"])
    tables, _ = reference(world, "app")
    for name, want in tables.items():
        assert report.metrics_dev[name].cpu().numpy().tobytes() == want.tobytes()


def test_a_sweep_shares_what_the_weights_do_not_touch(world, monkeypatch):
    evals = world["evals"]
    dev = engine_of(world, "device", "device", "device")
    hybrid = evals.BENCHMARK_CONFIGS["Hybrid"]
    sweep = dict(evals.BENCHMARK_CONFIGS)
    for i, (wd, wb, wp, mr) in enumerate([(0.6, 0.2, 0.2, 5), (0.4, 0.4, 0.2, 5), (0.5, 0.5, 0.0, 1), (0.3, 0.3, 0.4, 8),
                                          (0.7, 0.3, 0.0, 5), (0.2, 0.6, 0.2, 20)]):
        sweep[f"Hybrid v{i}"] = dict(hybrid, w_dense=wd, w_bm25=wb, w_prior=wp, min_reviews=mr, gate_penalty=(0.3, 0.5)[i % 2])
    alone = {name: dev.evaluate(world["test_queries"], {name: c}, qvecs=world["qvecs"]) for name, c in sweep.items()}
    counts = {"k1": [], "k2": 0, "gate": 0, "rerank": 0, "k3": 0, "metrics": 0}
    s = dev.searcher
    k1, k2, gate, scores, fuse = s.dense_pool, s.bm25_at, s.gate_text.gate, s.rerank_text.scores, s.fuse
    metrics = evals.DeviceLabels.metrics
    monkeypatch.setattr(s, "dense_pool", lambda q, pool, *a, **k: (counts["k1"].append(pool), k1(q, pool, *a, **k))[1])
    monkeypatch.setattr(s, "bm25_at", lambda *a, **k: (counts.__setitem__("k2", counts["k2"] + 1), k2(*a, **k))[1])
    monkeypatch.setattr(s.gate_text, "gate", lambda *a, **k: (counts.__setitem__("gate", counts["gate"] + 1), gate(*a, **k))[1])
    monkeypatch.setattr(s.rerank_text, "scores", lambda *a, **k: (counts.__setitem__("rerank", counts["rerank"] + 1), scores(*a, **k))[1])
    monkeypatch.setattr(s, "fuse", lambda *a, **k: (counts.__setitem__("k3", counts["k3"] + 1), fuse(*a, **k))[1])
    monkeypatch.setattr(evals.DeviceLabels, "metrics",
                        lambda self, *a, **k: (counts.__setitem__("metrics", counts["metrics"] + 1), metrics(self, *a, **k))[1])
    report = dev.evaluate(world["test_queries"], sweep, qvecs=world["qvecs"])
    # one batch; every configuration has pool 150 (the app's floor); penalties 0.0, 0.3 and 0.5; one rerank_k
    assert counts == {"k1": [150], "k2": 1, "gate": 3, "rerank": 1, "k3": len(sweep), "metrics": len(sweep)}
    for name in sweep:
        assert report.metrics_dev[name].cpu().numpy().tobytes() == alone[name].metrics_dev[name].cpu().numpy().tobytes(), name
        assert report.summary.loc[name].values.tobytes() == alone[name].summary.loc[name].values.tobytes(), name
    # the variants are not copies of one another
    assert len({report.metrics_dev[name].cpu().numpy().tobytes() for name in sweep}) >= 6


def test_flagged_queries_and_snippets(world):
    """A batch with queries the front hands back, and a configuration with use_snips (the best-review column in K3)."""
    evals = world["evals"]
    host, dev = engine_of(world, "host", "host", "host"), engine_of(world, "device", "device", "device")
    queries = world["queries"][:6] + [FLAGGED[0]] + world["queries"][6:20] + [FLAGGED[1]] + world["queries"][20:30]
    at = [i for i, q in enumerate(queries) if q not in FLAGGED]
    qv = np.empty((len(queries), W.DIM), dtype=np.float32)
    qv[at] = world["qvecs"][:30]
    qv[[6, 21]] = world["qvecs"][40:42]
    configs = {"snips": dict(evals.BENCHMARK_CONFIGS["Hybrid + Rerank"], use_snips=True, w_best=0.2, w_dense=0.3),
               "snips, smaller scan": dict(evals.BENCHMARK_CONFIGS["Hybrid"], use_snips=True, w_best=0.3, max_scan=2000),
               "Hybrid": evals.BENCHMARK_CONFIGS["Hybrid"]}
    first = host.run_search_batch(queries, qvecs=qv, **configs["snips"])
    test_queries = []
    for i, (q, (frame, snips, _)) in enumerate(zip(queries, first)):
        skus = frame["sku"].tolist()
        test_queries.append({"id": i, "query": q, "relevant_items": {skus[0], skus[3], skus[11], ABSENT},
                             "relevance_scores": {skus[0]: 1.5, skus[3]: 4.0, skus[30]: 2.0}})
    assert any(s for _, s, _ in first)
    tables, summary = model_tables(evals, host, test_queries, qv, configs)
    assert tables["snips"].tobytes() != tables["Hybrid"][:, :].tobytes()
    report = dev.evaluate(test_queries, configs, qvecs=qv)
    check_report(evals, report, tables, summary, test_queries)
    flagged_rows = tables["snips"][[6, 21]]
    assert (flagged_rows[:, 7] == 1.0).all()                  # the handed-back queries' own answers were put in place


def test_query_vectors_made_on_the_device(world):
    """No qvecs: the front makes the vectors once per batch (query_vectors="device"); the handed-back queries are encoded on
    the host, those only."""
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import QueryEncoder
    from review_recommender_amd.engine import SearchEngine
    evals = world["evals"]
    ce = world["ce"]
    vocab = max(ce.tokenizer.vocab.values()) + 1
    enc = QueryEncoder(synth.bert_state_dict(31, n_layers=2, n_labels=0, prefix="", vocab=vocab), ce.tokenizer)
    products = world["meta"].iloc[:300].reset_index(drop=True)
    host = SearchEngine.from_products(products, enc, cross_encoder=ce, query_vectors="host")
    dev = SearchEngine.from_products(products, enc, cross_encoder=ce, query_vectors="device", query_text="device", gate="device",
                                     rerank="device")
    rng = np.random.default_rng(4)
    texts = products["agg_text"].tolist()
    queries = [" ".join(rng.choice(texts[int(rng.integers(300))].split(), size=3)) for _ in range(9)] + [FLAGGED[1], "red cat socks"]
    configs = {n: evals.BENCHMARK_CONFIGS[n] for n in ("Dense Only", "Hybrid + Rerank")}
    first = host.run_search_batch(queries, **configs["Dense Only"])
    test_queries = [{"query": q, "relevant": [f["sku"][0], f["sku"][3], f["sku"][12]]} for q, (f, _, _) in zip(queries, first)]
    labels = evals.LabelSet.from_queries(test_queries, products["sku"].tolist())
    tables, summary = model_tables(evals, host, labels.queries, None, configs)
    encoded = []
    inner = enc.encode
    enc.encode = lambda s, **k: (encoded.append(list(s)), inner(s, **k))[1]
    try:
        report = dev.evaluate(test_queries, configs)
    finally:
        del enc.encode
    assert encoded == [[FLAGGED[1]]]
    check_report(evals, report, tables, summary, labels.queries)
