"""rr_ir_metrics_dev / rr_ir_mean_dev (csrc/rr_evals.hip) through the C ABI alone: the cases of tests/golden/ir_metrics.json
(a run of the reference's own IRMetrics.evaluate_query) as hand-made out_rows / order / labels, bit for bit; the column
means within nq * 2^-52 relative of numpy's (the worst case of any summation order of nq non-negative float64 values) and
bitwise the same on two calls; what the entry points refuse."""
import ctypes as C

import numpy as np
import pytest

import ir_metrics_cases

pytestmark = pytest.mark.gpu

K_VALUES = (1, 4, 5, 7, 8, 9, 10, 19, 20, 50, 65, 130)
RR_E_INVALID = -1


@pytest.fixture(scope="module")
def world():
    import torch
    from review_recommender_amd import _lib, evals
    golden = ir_metrics_cases.load()
    cases = golden["cases"]
    for c in cases:                                   # the eighth column, from its definition
        rel = set(c["relevant_items"])
        first = next((i + 1 for i, s in enumerate(c["retrieved"]) if s in rel), 0)
        c["want"] = [float(c["metrics"][n]) for n in evals.METRIC_NAMES] + [float(first)]
    return {"lib": _lib.load(), "torch": torch, "evals": evals, "cases": cases, "n_index": golden["n_index"],
            "skus": [f"P{r:05d}" for r in range(golden["n_index"])], "log2": evals.LOG2_TABLE}


def stage(world, cases, rng, pool_extra=7):
    """Device arguments of one call for ``cases`` (all of one k): the retrieved rows scattered over a pool of k + pool_extra
    distinct rows (the fillers may be labelled: they are not retrieved), order = where they went; the labels as a CSR."""
    torch, evals = world["torch"], world["evals"]
    k = cases[0]["k"]
    pool = k + pool_extra
    nq = len(cases)
    out_rows = np.empty((nq, pool), dtype=np.int64)
    order = np.empty((nq, k), dtype=np.int32)
    queries = []
    for b, c in enumerate(cases):
        ret = np.array([int(s[1:]) for s in c["retrieved"]], dtype=np.int64)
        labelled = [int(s[1:]) for s in list(c["relevant_items"]) + list(c["relevance_scores"] or {}) if s.startswith("P")]
        fill = rng.permutation(np.setdiff1d(np.array(labelled, dtype=np.int64), ret))[:pool_extra // 2]    # labelled, not retrieved
        fill = np.concatenate([fill, np.setdiff1d(np.arange(pool + k), np.concatenate([ret, fill]))])
        where = rng.permutation(pool)
        out_rows[b, where[:k]] = ret
        out_rows[b, where[k:]] = fill[:pool - k]
        order[b] = where[:k]
        scores = None if c["relevance_scores"] is None else {s: float(v) for s, v in c["relevance_scores"].items()}
        queries.append({"id": b, "query": str(b), "relevant_items": c["relevant_items"], "relevance_scores": scores})
    lab = evals.LabelSet.from_queries(queries, world["skus"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = {"out_rows": up(out_rows), "order": up(order), "lab_off": up(lab.lab_off), "lab_row": up(lab.lab_row),
         "lab_grade": up(lab.lab_grade), "lab_rel": up(lab.lab_rel), "n_rel": up(lab.n_rel), "idcg": up(lab.idcg),
         "log2": up(world["log2"]), "metrics": torch.full((nq, 8), -7.0, dtype=torch.float64, device="cuda"),
         "mean": torch.full((8,), -7.0, dtype=torch.float64, device="cuda")}
    return t, dict(nq=nq, pool=pool, k=k, n_labels=len(lab.lab_row))


def call(world, t, nq, pool, k, n_labels, mean=True, **override):
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None and x.numel() else None
    a = dict(out_rows=p(t["out_rows"]), order=p(t["order"]), nq=nq, pool=pool, k=k, lab_off=p(t["lab_off"]),
             lab_row=p(t["lab_row"]), lab_grade=p(t["lab_grade"]), lab_rel=p(t["lab_rel"]), n_labels=n_labels,
             n_rel=p(t["n_rel"]), idcg=p(t["idcg"]), log2=p(t["log2"]), metrics=p(t["metrics"]),
             mean=p(t["mean"]) if mean else None)
    a.update(override)
    stream = C.c_void_p(world["torch"].cuda.current_stream().cuda_stream)
    return world["lib"].rr_ir_metrics_dev(a["out_rows"], a["order"], a["nq"], a["pool"], a["k"], a["lab_off"], a["lab_row"],
                                          a["lab_grade"], a["lab_rel"], a["n_labels"], a["n_rel"], a["idcg"], a["log2"],
                                          a["metrics"], a["mean"], stream)


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257])
def test_metrics_equal_the_reference_bitwise(world, nq):
    torch = world["torch"]
    rng = np.random.default_rng(1000 + nq)
    seen = set()
    for k in K_VALUES:
        of_k = [c for c in world["cases"] if c["k"] == k]
        # nq cases of this k in shuffled order (17 per k: with repeats beyond that, each at another place in the pool)
        pick = rng.permutation(len(of_k))[:nq] if nq <= len(of_k) else \
            np.concatenate([rng.permutation(len(of_k)), rng.integers(0, len(of_k), size=nq - len(of_k))])
        cases = [of_k[i] for i in pick]
        seen |= {c["id"] for c in cases}
        t, dims = stage(world, cases, rng)
        assert call(world, t, **dims) == 0
        torch.cuda.synchronize()
        got = t["metrics"].cpu().numpy()
        want = np.array([c["want"] for c in cases], dtype=np.float64)
        bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
        assert len(bad) == 0, (k, [(cases[b]["id"], got[b].tolist(), want[b].tolist()) for b in bad[:3]])
        # the column means: within nq * 2^-52 relative of numpy's, and the same bits on a second call
        mean = t["mean"].cpu().numpy()
        ref = np.mean(want, axis=0)
        assert (np.abs(mean - ref) <= nq * 2.0 ** -52 * np.abs(ref)).all(), (k, mean, ref)
        assert call(world, t, **dims) == 0
        torch.cuda.synchronize()
        assert t["mean"].cpu().numpy().tobytes() == mean.tobytes() and t["metrics"].cpu().numpy().tobytes() == got.tobytes()
        # NULL d_mean is legal and leaves the table the same
        t["mean"].fill_(-3.0)
        t["metrics"].fill_(-7.0)
        assert call(world, t, mean=False, **dims) == 0
        torch.cuda.synchronize()
        assert t["metrics"].cpu().numpy().tobytes() == got.tobytes() and (t["mean"].cpu().numpy() == -3.0).all()
        # rr_ir_mean_dev alone is the same launch
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert world["lib"].rr_ir_mean_dev(C.c_void_p(t["metrics"].data_ptr()), nq, C.c_void_p(t["mean"].data_ptr()), stream) == 0
        torch.cuda.synchronize()
        assert t["mean"].cpu().numpy().tobytes() == mean.tobytes()
    if nq >= 257:
        assert len(seen) == len(world["cases"])       # every case of the fixture went through


def test_k_up_to_the_pool_limit(world):
    """k = pool = RR_MAX_POOL: the walk beyond rank 64 reaches a first hit at the last rank, and ends without one."""
    torch, evals = world["torch"], world["evals"]
    k = pool = 2048
    rng = np.random.default_rng(5)
    rows = rng.permutation(world["n_index"])[:k]
    skus = [world["skus"][r] for r in rows]
    outside = sorted(set(world["skus"]) - set(skus))
    labels = [[skus[-1]], [outside[0], outside[1]], [skus[64]], [skus[63], skus[2047]], [skus[1000], skus[1900]]]
    cases = [{"k": k, "retrieved": skus, "relevant_items": rel, "relevance_scores": None} for rel in labels]
    t, dims = stage(world, cases, rng, pool_extra=0)
    assert dims["pool"] == pool and call(world, t, **dims) == 0
    torch.cuda.synchronize()
    got = t["metrics"].cpu().numpy()
    want = np.array([[evals.model_ir_metrics(skus, rel)[n] for n in evals.COLUMNS] for rel in labels])
    assert got.tobytes() == want.tobytes(), (got, want)
    assert want[:, 7].tolist() == [2048.0, 0.0, 65.0, 64.0, 1001.0]


def test_labels_may_be_absent_altogether(world):
    """n_labels = 0 with NULL label arrays: every query's segment is empty."""
    torch = world["torch"]
    cases = [c for c in world["cases"] if c["id"] in ("no_labels@10", "all_absent@10")] * 3
    t, dims = stage(world, cases, np.random.default_rng(2))
    assert dims["n_labels"] == 0 and t["lab_row"].numel() == 0
    assert call(world, t, **dims) == 0
    torch.cuda.synchronize()
    assert t["metrics"].cpu().numpy().tobytes() == np.array([c["want"] for c in cases]).tobytes()
    assert (t["metrics"].cpu().numpy() == 0).all()


def test_invalid_arguments_are_refused(world):
    torch = world["torch"]
    cases = [c for c in world["cases"] if c["k"] == 10][:5]
    t, dims = stage(world, cases, np.random.default_rng(3))
    bad = [dict(nq=0), dict(nq=-1), dict(pool=0), dict(pool=2049, k=10), dict(k=0), dict(k=dims["pool"] + 1), dict(n_labels=-1),
           dict(out_rows=None), dict(order=None), dict(lab_off=None), dict(n_rel=None), dict(idcg=None), dict(log2=None),
           dict(metrics=None), dict(lab_row=None), dict(lab_grade=None), dict(lab_rel=None)]
    for override in bad:
        assert call(world, t, **dict(dims, **{k: v for k, v in override.items() if k in dims}),
                    **{k: v for k, v in override.items() if k not in dims}) == RR_E_INVALID, override
        assert world["lib"].rr_last_error()
    torch.cuda.synchronize()
    assert (t["metrics"].cpu().numpy() == -7.0).all() and (t["mean"].cpu().numpy() == -7.0).all()    # nothing was launched
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, mean = C.c_void_p(t["metrics"].data_ptr()), C.c_void_p(t["mean"].data_ptr())
    assert world["lib"].rr_ir_mean_dev(m, 0, mean, stream) == RR_E_INVALID
    assert world["lib"].rr_ir_mean_dev(None, 5, mean, stream) == RR_E_INVALID
    assert world["lib"].rr_ir_mean_dev(m, 5, None, stream) == RR_E_INVALID
    assert call(world, t, **dims) == 0                                                              # (and the good call goes through)
    torch.cuda.synchronize()
