"""The gate kernels (csrc/rr_gate.hip) on the GPU: the plane bitwise against gate.model_gate_plane, the match against
text.calculate_gate_factor on the ORIGINAL strings (float32 bits of the factor, the hit masks), and the engine with
gate="device" against gate="host" frame for frame, one query at a time and in batches."""
import json

import numpy as np
import pandas as pd
import pytest

import cli_worlds as W
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ZEBRA = "zebra"


def gate_mod():
    from review_recommender_amd import gate
    return gate


def want_gate(doc, groups, penalty):
    """(float32 factor, hit mask) of the reference's function on the original string."""
    from review_recommender_amd import text as T
    body = doc[:6000].lower()
    hits = sum(1 << g for g, grp in enumerate(groups) if any(s in body for s in grp))
    return np.float32(T.calculate_gate_factor(doc[:6000], groups, penalty)[0]), hits


def run_match(gt, docs, rows, groups, pens, row_offset=0):
    """The kernel (and the host function for the queries it cannot hold) on `rows` -> asserts both outputs against
    `want_gate`; returns the packed groups."""
    import torch
    G = gate_mod()
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    packed = G.pack_groups(groups, pens)
    pens = [pens] * len(groups) if np.isscalar(pens) else pens
    d_rows = torch.from_numpy(rows).to(gt.d_plane.device)
    host = lambda b, r: np.array([want_gate(docs[i - row_offset], groups[b], pens[b])[0] for i in r], dtype=np.float32)
    gate = gt.gate(d_rows, packed, host).cpu().numpy()
    _, hits = gt.factors(d_rows, packed, want_hits=True)
    hits = hits.cpu().numpy()
    gt.check()
    assert gate.dtype == np.float32 and gate.shape == rows.shape == hits.shape
    for b in range(rows.shape[0]):
        for j, r in enumerate(rows[b]):
            f, h = want_gate(docs[r - row_offset], groups[b], pens[b])
            assert gate[b, j].tobytes() == f.tobytes(), (b, j, int(r), gate[b, j], f, sorted(map(sorted, groups[b])))
            if b not in packed.host_queries:
                assert hits[b, j] == h, (b, j, int(r), bin(hits[b, j]), bin(h))
    return packed


# ------------------------------------------------------------------------------------------------ the plane
def plane_docs():
    G = gate_mod()
    pat = "Ab C-dE f0G'h "
    ascii_of = lambda n: (pat * (n // len(pat) + 1))[:n]
    docs = ["", "a"]
    for unit in (G.PER_THREAD, G.MATCH_STEP, G.PLANE_STEP, 2 * G.PLANE_STEP):
        docs += [ascii_of(unit + d) for d in (-1, 0, 1)]
    for ch in ("x", "é", "€", "\U0001f600"):
        docs += [ch * 5990 + "Tail-Ends-H" [:10 + d] for d in (0, 1)]                   # 6000 / 6001 code points
    docs.append(ascii_of(100_000))
    for ch in ("\u212a", "\u0130"):
        docs += [ch, ch + "Rest", "x" * 5999 + ch + "z", "é" * 5999 + ch + "z", "x" * 6000 + ch, "€" * 5998 + ch + ch + ch]
        docs += ["X" * (G.PLANE_STEP - d) + ch + "yZ" for d in (0, 1, 2, 3)]                 # across a step boundary
        docs += ["X" * (G.PER_THREAD - d) + ch + ch + "y" for d in (0, 1, 2, 3)]             # ... and a thread's
    docs += ["ab\ud800cd", "\udfff\u212a", "A\u212a\u0130\u212aB"]
    docs += ["Q" * n for n in range(1, 17)] + ["Wx" * 9]                                     # every start alignment 0..15
    return docs


def split_plane(gt):
    blob = gt.d_plane[:gt.plane_bytes].cpu().numpy().tobytes()
    off = gt.d_off.cpu().numpy()
    return [blob[off[i]:off[i + 1]] for i in range(gt.n)], off


def test_plane_equals_the_model_bitwise():
    import torch
    from review_recommender_amd.embed import _utf8_column
    from review_recommender_amd.products import DeviceProductText
    G = gate_mod()
    docs = plane_docs()
    want = [G.model_gate_plane(d) for d in docs]
    gt = G.GateText.from_texts(docs, 0, stage_bytes=4096)
    got, off = split_plane(gt)
    assert gt.n == len(docs) and off[0] == 0 and off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, docs[i][:40], len(g), len(w))
    starts = {int(o) % 16 for o in off[:-1]}
    assert starts == set(range(16))
    assert gt.nbytes == gt.plane_bytes + G.SLACK + 8 * (len(docs) + 1)
    # from the device layout, the WHOLE texts (the 100 KB one included: only its head may be read)
    raw, roff = _utf8_column(docs)
    dev = gt.d_plane.device
    d_text = torch.from_numpy(np.array(raw)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(roff, dtype=np.int64)).to(dev)
    gd = G.GateText.from_device(DeviceProductText(["s"] * len(docs), d_text, d_off, len(docs), int(roff[-1]), 0))
    got_d, off_d = split_plane(gd)
    assert got_d == got and off_d.tolist() == off.tolist()
    with pytest.raises(MemoryError, match='gate="host"'):
        G.GateText.from_texts(docs, 0, max_bytes=1000)
    empty = G.GateText.from_texts([], 0)
    assert empty.n == 0 and empty.plane_bytes == 0 and empty.d_off.cpu().tolist() == [0]
    for h in (gt, gd, empty):
        h.close()


# ------------------------------------------------------------------------------------------------ the match
@pytest.fixture(scope="module")
def slide():
    """Documents with ZEBRA (or a near miss) at every position around the first boundaries of every step size."""
    G = gate_mod()
    docs = []
    for unit in (G.PER_THREAD, G.MATCH_STEP, G.PLANE_STEP):
        for p in range(unit - 16 - len(ZEBRA), unit + 2):
            word = ZEBRA if p % 3 else "zebrb"
            docs.append("." * p + word + "," * (p % 5))
    long64 = "abcdefgh" * 8
    for p in range(G.MATCH_STEP - 80, G.MATCH_STEP + 2, 7):       # the longest term across a step's end
        docs.append("-" * p + (long64 if p % 2 else long64[:-1] + "X") + "=")
    gt = G.GateText.from_texts(docs, 0)
    yield docs, gt
    gt.close()


def test_match_slides_a_term_across_every_boundary(slide):
    docs, gt = slide
    n = len(docs)
    long64 = "abcdefgh" * 8
    groups = [[{ZEBRA}], [{"zebrb"}, {ZEBRA}], [{long64}, {ZEBRA, "zebrb"}], [{long64 + "i"}, {long64}]]
    rows = np.tile(np.arange(n, dtype=np.int64), (len(groups), 1))
    packed = run_match(gt, docs, rows, groups, [0.5, 0.3, 0.7, 0.5])
    assert packed.host_queries == [3]                  # the term above the limit: the host function, the same answer


@pytest.fixture(scope="module")
def edge():
    from review_recommender_amd import text as T
    docs = ["prefix " + ZEBRA,              # 0: ends on the document's last byte
            "one zeb", "ra two",            # 1, 2: completed by the next / the previous document only
            "ze", "bra",                    # 3, 4
            "é" * 5995 + ZEBRA + " after", "é" * 5996 + ZEBRA,       # 5: ends at character 6000, 6: at 6001
            "\U0001f600" * 5996 + ZEBRA, "ZEBRA Red HEADSET", "i am bored", "zebu zeb z", "zebr", "z", "",
            "only a headset here", "earbud earphones", "x" * 6100, "\u212aelvin blac\u212a \u0130nk", "noise-canceling anc",
            "yellow cat socks wireless", "Noise Cancelling HEADPHONES for the red dog", "a" * 15 + ZEBRA, "a" * 16 + ZEBRA]
    G = gate_mod()
    gt = G.GateText.from_texts(docs, 0)
    head = T.SYNONYMS["headphone"]
    assert sorted(head)[-1] == "headset" and len(head) == 7
    queries = [
        [{ZEBRA}],
        [],                                                                           # 0 groups
        [{"red"}, {"zebu"}, {"zeb"}, {"z"}, {"zebras"}, head],                        # 6 groups; a shared first byte and prefix
        [head],                                                                       # seven terms, only the last one hits doc 14
        [{"kelvin"}, {"black"}, {"ink"}, {"i"}],
        [set(T.SYNONYMS["noise"]), {"dog", "dogs", "puppy", "puppies"}],
        T.build_gate_groups("wireless yellow cat socks"),
        [{"x" * 64}, {"x" * 63 + "y"}],
        [{"a" + ZEBRA}, {"aa" + ZEBRA}],
    ]
    yield docs, gt, queries
    gt.close()


@pytest.mark.parametrize("pool", [1, 150, 257])
def test_match_edges_and_pools(edge, pool):
    docs, gt, queries = edge
    n, B = len(docs), len(queries)
    assert B == 9 and [len(q) for q in queries[:3]] == [1, 0, 6]
    rng = np.random.default_rng(pool)
    if pool == 1:
        rows = rng.integers(0, n, (B, 1))
    else:                       # every document for every query, then repeats
        rows = np.concatenate([np.tile(np.arange(n), (B, 1)), rng.integers(0, n, (B, pool - n))], axis=1)
    run_match(gt, docs, rows, queries, [0.5, 0.5, 0.3, 0.0, 0.7, 1.0, 0.5, 0.5, 0.5])


def test_match_with_a_row_offset_and_rows_outside(edge):
    G = gate_mod()
    docs = edge[0]
    gt = G.GateText.from_texts(docs, 0, row_offset=1000)
    n = len(docs)
    rows = np.tile(np.arange(1000, 1000 + n, dtype=np.int64), (2, 1))
    run_match(gt, docs, rows, [[{ZEBRA}], [{"red"}, {"headset"}]], 0.5, row_offset=1000)
    # a row outside [row_offset, row_offset + n): no text is read, every group misses, and the status says so
    import torch
    packed = G.pack_groups([[{ZEBRA}], [{"red"}, {"headset"}]], 0.5)
    bad = torch.tensor([[0, 999, 1000 + n, -5], [1000, 1000 + n - 1, 2 ** 40, 1008]], dtype=torch.int64, device=gt.d_plane.device)
    gate, hits = gt.factors(bad, packed, want_hits=True)
    assert gate.cpu().numpy().tolist() == [[0.5] * 4, [0.25, 0.25, 0.25, 1.0]] and hits.cpu().numpy().tolist() == [[0] * 4, [0, 0, 0, 3]]
    with pytest.raises(ValueError, match="outside the plane"):
        gt.check()
    gt.check()                                          # (the counter was cleared)
    gt.close()


def test_reference_run_gate_factors_through_the_kernel():
    from review_recommender_amd import text as T
    G = gate_mod()
    cases = json.loads((GOLDEN / "cli_helpers.json").read_text())["gate_factor"]
    docs = sorted({c["text"] for c in cases})
    row_of = {t: i for i, t in enumerate(docs)}
    gt = G.GateText.from_texts(docs, 0)
    keys = sorted({(c["q"], c["penalty"]) for c in cases})
    import torch
    for a in range(0, len(keys), 9):
        part = keys[a:a + 9]
        groups = [T.build_gate_groups(q) for q, _ in part]
        packed = G.pack_groups(groups, [p for _, p in part])
        assert not packed.host_queries
        rows = torch.from_numpy(np.tile(np.arange(len(docs), dtype=np.int64), (len(part), 1))).to(gt.d_plane.device)
        gate = gt.factors(rows, packed).cpu().numpy()
        for b, (q, pen) in enumerate(part):
            for c in cases:
                if (c["q"], c["penalty"]) == (q, pen):
                    assert gate[b, row_of[c["text"]]].tobytes() == np.float32(c["y"]).tobytes(), c
    gt.check()
    gt.close()


# ------------------------------------------------------------------------------------------------ the engine
ENGINE_WORLDS = ("plain", "nan1", "reviews")
_worlds, _engines = {}, {}


def world_of(name, tmp_path_factory):
    from review_recommender_amd import artifacts
    if name not in _worlds:
        world = W.make_world(name)
        path = tmp_path_factory.mktemp("gate_" + name)
        artifacts.save_artifacts(path, world["meta"], world["emb"], world["blob"])
        if world["reviews"] is not None:
            artifacts.save_reviews(path, *world["reviews"])
        _worlds[name] = (world, path)
    return _worlds[name]


def engine_of(name, flavour, gate, tmp_path_factory):
    from review_recommender_amd.engine import SearchEngine
    key = (name, flavour, gate)
    if key not in _engines:
        _, path = world_of(name, tmp_path_factory)
        _engines[key] = SearchEngine.from_artifacts(path, flavour=flavour, cross_encoder=W.FakeCrossEncoder(), gate=gate)
    return _engines[key]


@pytest.fixture(scope="module")
def search_cases():
    return json.loads((GOLDEN / "cli_search.json").read_text())["cases"]


def search_args(case):
    a = case["args"]
    return (a["k"], a["rerank_k"], a["w_dense"], a["w_bm25"], a["w_rerank"], a["w_prior"], a["w_best"], a["prior_C"],
            not a["no_snippets"], a["max_reviews_scan"], 8, a["gate_penalty"])


def assert_same_answer(got, want):
    (gf, gs, gd), (wf, ws, wd) = got, want
    pd.testing.assert_frame_equal(gf, wf, check_exact=True)
    assert gs == ws and gd == wd


@pytest.mark.parametrize("flavour", ["cli", "app"])
@pytest.mark.parametrize("world_name", ENGINE_WORLDS)
def test_engine_device_gate_equals_host_gate(world_name, flavour, search_cases, tmp_path_factory, monkeypatch):
    from review_recommender_amd import text as T
    from review_recommender_amd.engine import SearchEngine
    world, _ = world_of(world_name, tmp_path_factory)
    mine = [c for c in search_cases if c["world"] == world_name]
    assert mine
    if world_name == "plain":
        assert {c["args"]["gate_penalty"] for c in mine} >= {0.0, 0.3, 0.5, 1.0}
    host = engine_of(world_name, flavour, "host", tmp_path_factory)
    want = [host.run_search(c["query"], *search_args(c), qvec=W.qvec_of(c, world["emb"])) for c in mine]
    assert any((f["_gate"] != 1).any() for f, _, _ in want)
    dev = engine_of(world_name, flavour, "device", tmp_path_factory)
    assert dev.searcher.gate_text is not None and host.searcher.gate_text is None

    def boom(*a, **k):
        raise AssertionError("the host gate ran although the engine has a gate plane")
    monkeypatch.setattr(T, "calculate_gate_factor", boom)
    monkeypatch.setattr(SearchEngine, "_gate_rows", boom)
    for c, w in zip(mine, want):
        assert_same_answer(dev.run_search(c["query"], *search_args(c), qvec=W.qvec_of(c, world["emb"])), w)
    dev.searcher.gate_text.check()


@pytest.mark.parametrize("gate", ["host", "device"])
@pytest.mark.parametrize("world_name,flavour", [("plain", "cli"), ("reviews", "app")])
def test_run_search_batch_equals_run_search_query_by_query(world_name, flavour, gate, search_cases, tmp_path_factory):
    world, _ = world_of(world_name, tmp_path_factory)
    engine = engine_of(world_name, flavour, gate, tmp_path_factory)
    # nine (query, query vector) pairs of the plain world's cases: all five queries, several vectors
    by = {(c["config"], c["query"]): c for c in search_cases if c["world"] == "plain"}
    picked = ([by["hybrid", q] for q in W.QUERIES] + [by["cli_defaults", q] for q in W.QUERIES[:3]]
              + [by["wide_pool", W.QUERIES[0]]])
    assert len(picked) == 9 and len({c["query"] for c in picked}) == 5
    queries = [c["query"] for c in picked]
    qvecs = np.stack([W.qvec_of(c, world["emb"]) for c in picked])
    args = list(search_args(next(c for c in search_cases if c["config"] == "cli_defaults")))
    args[8] = world_name == "reviews"                   # use_snips
    args[6] = 0.25 if world_name == "reviews" else args[6]
    alone = [engine.run_search(q, *args, qvec=v) for q, v in zip(queries, qvecs)]
    assert any((f["_gate"] != 1).any() for f, _, _ in alone)
    for n in (1, 5, 9):
        got = engine.run_search_batch(queries[:n], *args, qvecs=qvecs[:n])
        assert len(got) == n
        for g, w in zip(got, alone):
            assert_same_answer(g, w)
    assert engine.run_search_batch([], *args) == []


def test_run_search_batch_with_an_encoder(tmp_path_factory):
    """One encode call for the whole batch; the encoder's batch invariance is not claimed anywhere, so only shapes and
    skus are compared (this stand-in happens to be invariant)."""
    from review_recommender_amd import synth
    engine = engine_of("plain", "cli", "device", tmp_path_factory)

    class Encoder:
        calls = 0

        def encode(self, texts, normalize_embeddings=True):
            Encoder.calls += 1
            return np.stack([synth.unit_rows(1, W.DIM, sum(map(ord, t)))[0] for t in texts])
    engine.encoder = Encoder()
    try:
        got = engine.run_search_batch(W.QUERIES, 10, 0, 0.5, 0.3, 0.0, 0.2, 0.0, 20.0, False, 0, 8, 0.5)
        assert Encoder.calls == 1 and len(got) == len(W.QUERIES)
        for q, (frame, snips, dbg) in zip(W.QUERIES, got):
            alone = engine.run_search(q, 10, 0, 0.5, 0.3, 0.0, 0.2, 0.0, 20.0, False, 0, 8, 0.5)[0]
            assert frame.shape == alone.shape and frame["sku"].tolist() == alone["sku"].tolist()
    finally:
        engine.encoder = None
