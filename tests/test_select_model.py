"""tests/select_model.py on the CPU: the model of rr_kth_largest_reg against np.partition, the model of rr_select against a
brute-force sort, and -- a condition, not a measurement -- every named input of tests/test_gpu_select_kernels.py reaches
the door, the sub-branch or the branch it is named after.  An input that misses its door is a wrong input."""
import numpy as np
import pytest

import select_model as M


@pytest.fixture(scope="module")
def cases():
    return M.select_cases()


def test_caps_are_the_ones_the_cases_were_built_for():
    assert (M.RR_SEL_LCAP, M.RR_SEL_GCAP, M.RR_SEL_CCAP, M.RR_SEL_SORTCAP, M.RR_SEL_RK, M.RR_SEL_THREADS) == (4096, 4096, 12288, 8192, 8, 1024)
    assert (M.RR_X3_MCAP, M.RR_MAX_SCAN_WAVES, M.RR_FLT_MAXQ, M.RR_SEL_LISTED) == (16384, 8192, 128, 8)


@pytest.mark.parametrize("name", list(M.kth_key_sets()))
def test_kth_largest_reg_is_a_lower_bound_that_k_keys_reach(name):
    keys, k = M.kth_key_sets()[name]
    true = M.kth_largest_exact(keys, k)
    got = M.kth_largest_reg(keys, k)
    assert got <= true, (hex(got), hex(true))
    assert int((keys.astype(np.int64) >= got).sum()) >= k
    assert M.kth_largest_reg(keys, k, max_steps=16) == true            # 16 two-bit steps resolve all 32 bits
    nz = keys[keys != 0]
    if len(nz) >= k and len(nz) > 1:
        # the 14 bits resolved start at the highest bit the NON-ZERO keys differ in: tau is within 2^-14 of their spread
        spread_bit = (int(keys.max()) ^ int(nz.min())).bit_length() - 1
        assert true - got < (1 << max(spread_bit + 1 - 2 * M.STEPS, 0)), (hex(got), hex(true), spread_bit)


def test_kth_largest_reg_resolution_per_step():
    keys = M.f2key(np.random.default_rng(5).standard_normal(3000).astype(np.float32))
    true = M.kth_largest_exact(keys, 150)
    last = 0
    for steps in range(0, 17):
        got = M.kth_largest_reg(keys, 150, max_steps=steps)
        assert last <= got <= true
        last = got
    assert last == true


def test_every_select_case_reaches_its_door(cases):
    seen = set()
    for name, c in cases.items():
        L = M.levels(c["scores"][None], c["n_rows"], c["tiles_per_wave"])
        r = M.select(L, 0, c["pool"], keys=c["keys"])
        for what, want in c["want"].items():
            assert r[what] == want, (name, what, r[what], want)
        seen.add((r["door"], r["sort"], r["sub"], r["step3b"]))
        assert r["rows"].max() < c["n_rows"] and len(set(r["rows"].tolist())) == c["pool"]
    # every door, both sorts, every slow sub-branch
    for combo in [(None, "rank", None, None), (None, "bitonic", None, None), ("groups", None, "all", False), ("tiles", None, "all", False),
                  ("rows", None, "listed", False), ("rows", None, "listed", True), ("rows", None, "all", True), ("rows", None, "all", False),
                  ("few", None, "listed", False)]:
        assert combo in seen, combo
    # each RK instance of the bisection
    ngs = [M.levels(cases[f"fast rank, {ng} groups"]["scores"][None], cases[f"fast rank, {ng} groups"]["n_rows"], 1)["n_waves"]
           for ng in (1000, 2000, 4000, 8000)]
    assert [(ng + M.RR_SEL_THREADS - 1) // M.RR_SEL_THREADS for ng in ngs] == [1, 2, 4, 8]


def test_the_cases_sit_on_both_sides_of_every_cap(cases):
    def trace(name):
        c = cases[name]
        return M.select(M.levels(c["scores"][None], c["n_rows"], c["tiles_per_wave"]), 0, c["pool"], keys=c["keys"])
    assert trace("n_cand 1024: the last rank sort")["trace"][3] == M.RR_SEL_THREADS and trace("fast bitonic, n_cand 1025")["sort"] == "bitonic"
    assert trace("fast bitonic, n_cand 6144")["trace"][3] == M.RR_SEL_CCAP // 2 and trace("door 3: n_cand 6145")["door"] == "rows"
    assert trace("4096 groups stay fast")["trace"][1] == M.RR_SEL_LCAP and trace("door 1: 4097 groups")["trace"][1] == M.RR_SEL_LCAP + 1
    assert trace("4096 tiles stay fast")["trace"][2] == M.RR_SEL_GCAP and trace("door 2: 4097 tiles")["trace"][2] == M.RR_SEL_GCAP + 1
    assert trace("door 2: 4097 tiles")["trace"][1] <= M.RR_SEL_LCAP
    assert trace("slow, listed tiles, n_cand 8192")["slow"][1] == M.RR_SEL_SORTCAP and trace("slow, step 3b, n_cand 8193")["step3b"]
    r = trace("slow, step 3b, 20000 tied at the cut")
    tie = np.flatnonzero(cases["slow, step 3b, 20000 tied at the cut"]["scores"] == M.TOP)
    assert len(tie) == 20000 - 50 and r["rows"][50:].tolist() == sorted(tie.tolist())[:100]      # the smallest rows of the tie
    c = cases["ragged last tile, tie across the end"]
    assert c["n_rows"] % 64 and (c["scores"][-17:] == M.TOP).all()
    c = cases["short last run, tie across the end"]
    L = M.levels(c["scores"][None], c["n_rows"], 3)
    assert L["n_tiles"] % 3 == 1 and c["n_rows"] % 64 and (c["scores"][-59:] == M.TOP).all()


def test_select_against_a_brute_force_sort():
    rng = np.random.default_rng(9)
    for n_rows, tpw, pool in [(1, 1, 1), (63, 1, 63), (65, 1, 10), (700, 2, 150), (5000, 3, 150), (20000, 1, 257), (20000, 5, 2048)]:
        s = rng.integers(-6, 7, n_rows).astype(np.float32) / np.float32(4)             # many ties, +0.0 only
        s[s == 0] = 0.0
        s[rng.permutation(n_rows)[:n_rows // 10]] = -np.inf
        if n_rows > 100:
            s[rng.permutation(n_rows)[:3]] = np.inf
        L = M.levels(s[None], n_rows, tpw)
        r = M.select(L, 0, pool, row_offset=1000)
        brute = sorted(range(n_rows), key=lambda i: (-float(s[i]), i))[:pool]
        assert r["rows"].tolist() == [i + 1000 for i in brute]
        assert r["bits"].tolist() == s[brute].view(np.uint32).tolist()
        if r["door"] is None:
            # the fast path's lists hold the answer: every row of the top-pool reaches tau, in a tile and a group that reach it
            assert r["trace"][3] >= pool and (M.f2key(s[brute]).astype(np.int64) >= r["tau"]).all()


def test_levels_and_device_layouts():
    s = np.arange(2 * 200, dtype=np.float32).reshape(2, 200)
    L = M.levels(s, 200, 3, 16)
    assert (L["n_tiles"], L["n_pad"], L["n_waves"]) == (4, 256, 2)
    assert L["sims"][1, 199] == 399 and np.isneginf(L["sims"][:, 200:]).all()
    assert L["gmax"][0].tolist() == [63, 127, 191, 199] and M.key2f(L["keys"][0]).tolist() == [191, 199]       # the short last run
    sims, gmax, keys = M.device(L)
    assert sims.shape == (16, 16, 16) and gmax.shape == (4, 16) and keys.shape == (2, 16)
    assert sims[(77 >> 4), 1, 77 & 15] == 277 and gmax[2, 0] == 191 and keys[1, 1] == M.f2key(np.float32([399]))[0]
    assert np.isposinf(sims[:, 2:]).all()
    sims, gmax, keys = M.device(M.levels(s, 200, 3, 0), slots=8)
    assert sims.shape == (8, 256) and sims[1, 77] == 277 and gmax.shape == (8, 4) and keys.shape == (8, 2)


def test_select_launches_share_a_geometry(cases):
    for name, (qs, names) in M.select_launches().items():
        L, pool = M.launch_levels(names, qs, cases)
        assert L["nq"] == len(names) and L["n_waves"] <= M.RR_MAX_SCAN_WAVES, name
    doors = [M.select(M.launch_levels(M.select_launches()["doors, qs 0"][1], 0, cases)[0], q, M.POOL) for q in range(5)]
    # rank sort | bitonic sort | slow on listed tiles (twice: at the door and near the sort cap) | slow with step 3b
    assert len({(d["door"], d["sort"], d["step3b"]) for d in doors}) == 4 and len({d["trace"][3] for d in doors}) == 5


def test_group_kth_cases_reach_their_branches():
    rk = set()
    for name, c in M.group_kth_cases().items():
        ng = c["n_waves"] * c["gpw"]
        for (s, i), want in zip(c["per"], c["want"]):
            keys, eps = c["keys"][s, :, i], c["eps"][M.RR_FLT_MAXQ * s + i]
            tau, value = M.group_kth(keys, c["kth"], eps)
            assert (value == -np.inf) == (want == "-inf"), (name, s, i)
            if want == "value":
                # the property the shards rely on
                assert int((keys.astype(np.int64) >= tau).sum()) >= c["kth"] and value <= float(M.key2f(np.uint32([tau]))[0]) - float(eps)
                rk.add((ng + M.RR_SEL_THREADS - 1) // M.RR_SEL_THREADS)
    assert {1, 2, 3, 8} <= rk                  # ng 300, 1500, 3000, 8192: the instances <1>, <2>, <4>, <8>
    c = M.group_kth_cases()["RK 2, padding keys"]
    zeros = [(c["keys"][0, :, i] == 0).sum() for i in range(3)]
    assert zeros[0] < c["kth"] < zeros[1] and len(c["keys"][0]) - zeros[2] < c["kth"]
    c = M.group_kth_cases()["RK 1, eps edges"]
    assert M.group_kth(c["keys"][0, :, 1], 38, 0.01)[0] <= M.KEY_NEG_INF and M.group_kth(c["keys"][0, :, 8], 38, 0.01)[0] <= M.KEY_NEG_INF


def test_mtile_cases_reach_their_branches():
    seen = set()
    for name, c in M.mtile_cases().items():
        L = c["L"]
        for q in range(L["nq"]):
            eps = None if c["eps"] is None else c["eps"][q]
            floor = None if c["floor"] is None else c["floor"][q]
            r = M.select_mtiles(L, q, c["pool"], eps, floor)
            want = dict(c["want"][q])
            tau_is = want.pop("tau_is", None)
            for what, v in want.items():
                assert r[what] == v, (name, q, what, r[what], v)
            if tau_is == "own":
                assert r["tau"] > M.f2key(np.float32([floor]))[0]
            if eps is not None and r["branch"] not in ("small", "no eps"):
                assert M.gap_ok(L, q, r["open"]), (name, q)
            if r["fb"] == 0:
                assert r["count"] == len(r["listed"]) > 0 and max(r["listed"]) < (L["n_rows"] + 15) // 16
            seen.add((r["branch"], r["fb"]))
    assert {("own", 0), ("own", 1), ("small", 1), ("no eps", 1), ("floor", 0), ("hot", 0)} <= seen
    c = M.mtile_cases()["hot shard"]
    r = M.select_mtiles(c["L"], 1, c["pool"], c["eps"][1], c["floor"][1])
    assert r["tau"] == M.f2key(c["floor"][1:2])[0] and r["c0"] == 160           # the floor's cut, the shard's own `open`


def test_mtile_device_layouts():
    mt = np.arange(2 * 13, dtype=np.float32).reshape(2, 13)                      # 200 rows: 13 M-tiles, 4 tiles
    L = M.mtile_levels(mt, 200, 3, 2, 2, 16)
    assert L["keys"].shape == (2, 4) and L["keys"][0, 3] == 0                    # wave 1 holds one tile: its second group is padding
    assert [t.tolist() for t in L["group_tiles"]] == [[0, 1], [2], [3], []]
    m0, k = M.mtile_device(L, 0)
    m1, _ = M.mtile_device(L, 1)
    assert m0.shape == (4, 16, 4) and m1.shape == (8, 16, 2) and k.shape == (4, 16)
    assert m0[2, 1, 3] == 13 + 11 and m1[5, 1, 1] == 13 + 11 and np.isneginf(m0[3, 0, 1:]).all()
