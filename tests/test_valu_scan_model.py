"""tests/valu_scan_model.py on the CPU: the chain models agree where they overlap, the level model equals brute force, the list
models equal a literal transcription of the kernels' ballot loops, and every named input reaches the door it is named after."""
import itertools

import numpy as np
import pytest

import fltw_bf16_model as FB
import fltw_model as FW
import rescore_model as RM
import valu_scan_model as M


def test_the_runtime_width_chains_are_the_384_chains_at_384():
    V = M.ragged(200, 384, 5)
    V[3, 9] = np.nan
    V[5, 100] = np.inf
    V[7] = 0.0
    Vb = RM.round_to_bf16(V)
    for q in M.queries(3, 384, 6):
        assert M.bits(FW.chain_w(V, q)).tolist() == M.bits(RM.chain_f32(V, q)).tolist()
        assert M.bits(FB.chain_wb(Vb, q)).tolist() == M.bits(RM.chain_bf16(Vb, q)).tolist()


def test_f64_bound_is_gamma_28_at_384():
    S = M.stored_rows(M.ragged(10, 384, 1), "f32")
    q = M.queries(1, 384)[0]
    mag = np.abs(S.astype(np.float64) * q.astype(np.float64)).sum(axis=1)
    assert np.allclose(M.f64_bound(S, q, 384), RM.GAMMA_28 * mag, rtol=1e-12, atol=384 * 2.0 ** -150)
    assert M.gamma(28) == RM.GAMMA_28


def _brute_levels(stored, QP, n_rows, C):
    # float64 scores, maxima by plain loops
    T = (n_rows + 63) // 64
    W = (T + C - 1) // C
    NB = len(QP)
    sims = np.full((NB, 64 * T), -np.inf)
    sims[:, :n_rows] = QP.astype(np.float64) @ stored.astype(np.float64).T
    gmax = np.array([[sims[b, 64 * t:64 * t + 64].max() for t in range(T)] for b in range(NB)])
    smax = np.array([[gmax[b, w * C:min((w + 1) * C, T)].max() for w in range(W)] for b in range(NB)])
    return sims, gmax, smax


@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("n_rows,dim,C", [(1, 64, 1), (65, 100, 1), (130, 384, 2), (300, 192, 3)])
def test_level_model_equals_brute_force_within_the_bound(dtype, n_rows, dim, C):
    stored = M.stored_rows(M.ragged(n_rows, dim, n_rows), dtype)
    D = stored.shape[1]
    QP = M.pad_queries(M.queries(3, dim, n_rows), D, 4)              # slot 3: the zero query
    g = M.geom_of(n_rows, C)
    assert not M.geom_problems(g, n_rows)
    sims, gmax, smax = M.expected_levels(stored, QP, g, dtype)
    assert sims.shape == (4, g["n_pad"]) and gmax.shape == (4, g["n_tiles"]) and smax.shape == (4, g["n_waves"])
    ref_s, ref_g, ref_w = _brute_levels(stored, QP, n_rows, C)
    S = M.from_bits(sims).astype(np.float64)
    bound = np.stack([M.f64_bound(stored, q, D) for q in QP])
    assert (np.abs(S[:, :n_rows] - ref_s[:, :n_rows]) <= bound).all()
    assert np.isneginf(S[:, n_rows:]).all() and (sims[3, :n_rows] == 0).all()
    # a maximum of scores within `bound` of the references is within the largest bound of the reference maximum
    assert (np.abs(M.from_bits(gmax) - ref_g) <= bound.max()).all()
    assert (np.abs(RM.key2f(smax).astype(np.float64) - ref_w) <= bound.max()).all()
    # and the model's maxima are exactly the maxima of ITS scores
    Sf = M.from_bits(sims).reshape(4, g["n_tiles"], 64)
    assert (M.from_bits(gmax) == Sf.max(axis=2)).all()
    for w in range(g["n_waves"]):
        assert (RM.key2f(smax[:, w]) == Sf[:, w * C:(w + 1) * C].max(axis=(1, 2))).all()
    n, bad, worst = M.f64_excess(sims[0], stored, QP[0])
    assert n == n_rows and bad == 0 and worst <= 1.0


# ------------------------------------------------------------------ the lists
def _ballot_words(flags):
    nq = len(flags)
    for i in range((nq + 63) // 64):
        m = 0
        for lane in range(64):
            q = 64 * i + lane
            if q < nq and flags[q] != 0:
                m |= 1 << lane
        yield i, m


def _loop_list(flags, NB):
    # rr_flagged_list, line by line
    lst, n, total = [0] * NB, 0, 0
    for i, m in _ballot_words(flags):
        total += bin(m).count("1")
        while m and n < NB:
            b = (m & -m).bit_length() - 1
            m &= m - 1
            lst[n] = 64 * i + b
            n += 1
    if total > NB:
        return 0, lst
    for j in range(1, NB):
        if j >= n and n > 0:
            lst[j] = lst[j - 1]
    return n, lst


def _loop_slice(flags, skip, NB):
    # rr_flagged_slice, line by line
    lst, n, seen = [0] * NB, 0, 0
    for i, m in _ballot_words(flags):
        while m and n < NB:
            b = (m & -m).bit_length() - 1
            m &= m - 1
            seen += 1
            if seen - 1 < skip:
                continue
            lst[n] = 64 * i + b
            n += 1
    for j in range(1, NB):
        if j >= n and n > 0:
            lst[j] = lst[j - 1]
    return n, lst


def _same(model, loop):
    return model[0] == loop[0] and model[1].tolist() == loop[1]


def test_list_models_equal_the_loops_on_all_patterns_of_nine_queries():
    for pat in itertools.product((0, 1), repeat=9):
        f = np.array(pat, dtype=np.int32)
        for NB in (1, 2, 4, 8):
            assert _same(M.flagged_list(f, NB), _loop_list(f, NB)), (pat, NB)
        for skip in (0, 1, 3, 8, 9):
            assert _same(M.flagged_slice(f, skip, 8), _loop_slice(f, skip, 8)), (pat, skip)
    assert M.flagged_list(np.ones(9, dtype=np.int32), 8)[0] == 0


def test_list_models_equal_the_loops_across_ballot_words():
    at = (63, 64, 65, 255)
    for nq in (64, 65, 66, 256):
        for r in range(len(at) + 1):
            for qs in itertools.combinations(at, r):
                f = np.zeros(nq, dtype=np.int32)
                f[[q for q in qs if q < nq]] = 1
                assert _same(M.flagged_list(f, 8), _loop_list(f, 8)), (nq, qs)
                for skip in (0, 1, 2, 4):
                    assert _same(M.flagged_slice(f, skip, 8), _loop_slice(f, skip, 8)), (nq, qs, skip)
    for nq in (9, 64, 65, 256):
        for name, f in M.flag_patterns(nq).items():
            assert _same(M.flagged_list(f, 8), _loop_list(f, 8)), (nq, name)
            for skip in (0, 8, 16, 24):
                assert _same(M.flagged_slice(f, skip, 8), _loop_slice(f, skip, 8)), (nq, name, skip)
    f = M.flag_patterns(256)["twenty"]
    assert int(f.sum()) == 20
    assert [M.flagged_slice(f, s)[0] for s in (0, 8, 16, 24)] == [8, 8, 4, 0]
    n, lst = M.flagged_slice(f, 16)
    assert lst[3:].tolist() == [lst[3]] * 5                      # slice of 4, the last repeated
    f = M.flag_patterns(256)["eight"]
    assert M.flagged_list(f)[0] == 8 and len({q // 64 for q in M.flagged_list(f)[1]}) == 4      # four ballot words


# ------------------------------------------------------------------ the named inputs
@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("dim,runs", [(384, (1,)), (100, (1,)), (128, (3, 6)), (64, (4,))])
def test_special_rows_reach_their_doors(dtype, dim, runs):
    n_rows = 64 * (M.special_layout(10 ** 6, runs)["nan_tile"] + 2) + 37
    V, Q, plants = M.special_rows(n_rows, dim, runs)
    stored = M.stored_rows(V, dtype)
    D = stored.shape[1]
    QP = M.pad_queries(Q, D, 4)
    full, zero, tiny = (M.chain(stored, q, dtype) for q in QP[:3])
    ref_full, ref_zero = M.f64_scores(stored, QP[0]), M.f64_scores(stored, QP[1])
    r = plants["nan"][0]
    assert np.isnan(ref_full[r]) and np.isnan(full[r]) and np.isneginf(M.stored_scores(stored, QP[0], dtype)[r])
    assert np.isinf(full[plants["pinf"][0]]) and np.isinf(full[plants["ninf"][0]])
    assert full[plants["pinf"][0]] == -full[plants["ninf"][0]] == np.sign(QP[0][M.C_INF]) * np.inf
    r = plants["inf_zero"][0]
    assert QP[1][M.C_ZERO] == 0 and np.isnan(ref_zero[r]) and np.isnan(zero[r]) and np.isinf(full[r])
    r = plants["overflow"][0]
    assert full[r] == np.inf and np.isfinite(ref_full[r]) and ref_full[r] > float(np.finfo(np.float32).max)
    assert M.bits(full[plants["zero"]])[0] == 0 and M.bits(tiny[plants["zero"]])[0] == 0
    r = plants["negzero"][0]
    assert (stored[r, :dim] != 0).all() and (np.abs(stored[r].astype(np.float64) * QP[2]) < 2.0 ** -150).all()
    assert M.bits(tiny[r:r + 1])[0] == (M.NEG_ZERO_BITS if M.negzero_reaches(dim, dtype) else 0)
    assert full[r] != 0 and abs(float(full[r])) < 2.0 ** -126        # against a normal query: a denormal score
    assert np.isnan(full[plants["nan_tile"]]).all() and np.isnan(tiny[plants["nan_tile"]]).all()
    a, b = plants["ties"]
    assert a // 64 + 1 == b // 64 and M.bits(full[a:a + 1])[0] == M.bits(full[b:b + 1])[0] and full[a] == np.nanmax(full[np.isfinite(full)])
    for C in runs:
        g = M.geom_of(n_rows, C)
        sims, gmax, smax = M.expected_levels(stored, QP, g, dtype)
        tiles, wruns = M.mixed_zero(sims, g)
        L = M.special_layout(g["n_tiles"], runs)
        assert gmax[0, a // 64] == gmax[0, b // 64]
        if max(runs) % C == 0:                                       # the tie seam is a run seam of the longest run and of its divisors
            assert (b // 64) % C == 0 and a // 64 // C + 1 == b // 64 // C and smax[0, a // 64 // C] == smax[0, b // 64 // C]
        assert gmax[0, L["nan_tile"]] == M.NEG_INF_BITS and gmax[2, L["nan_tile"]] == M.NEG_INF_BITS
        if C == 1:
            assert smax[0, L["nan_tile"]] == M.KEY_NEG_INF
        if M.negzero_reaches(dim, dtype):
            assert np.argwhere(tiles).tolist() == [[2, L["zero_tile"]]] and np.argwhere(wruns).tolist() == [[2, L["zero_tile"] // C]]
            assert gmax[2, L["zero_tile"]] == 0 and smax[2, L["zero_tile"] // C] == RM.f2key(np.float32(0.0))
        else:
            assert not tiles.any() and not wruns.any()
            assert gmax[2, L["zero_tile"]] == 0


@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("C,n_tiles,nq", [(3, 47, 1), (6, 47, 8), (4, 95, 5), (1, 16, 3)])
def test_maxima_plants_reach_their_places(dtype, C, n_tiles, nq):
    n_rows = 64 * (n_tiles - 1) + 37
    dim = 64
    g = M.geom_of(n_rows, C)
    V = M.ragged(n_rows, dim, 9)
    Q = M.queries(nq, dim, 9)
    planted = M.maxima_plants(V, Q, g, avoid=(5,))
    assert len(planted) == 3 * nq and len({p[2] for p in planted.values()}) == 3 * nq
    assert {planted[(0, "first")][2] % 64, planted[(0, "last")][2] % 64} == {0, 63}
    stored = M.stored_rows(V, dtype)
    sims, gmax, smax = M.expected_levels(stored, M.pad_queries(Q, 64, M.nb_of(nq)), g, dtype)
    S = M.from_bits(sims)
    for (b, where), (w, tile, row) in planted.items():
        assert not w * C <= 5 < (w + 1) * C and w < g["n_waves"] - 1
        assert tile == w * C + {"first": 0, "last": C - 1, "middle": C // 2}[where]
        run = S[b, 64 * C * w:64 * C * (w + 1)]
        assert int(np.argmax(run)) + 64 * C * w == row and abs(float(S[b, row]) - (4 + b)) < 0.1
        assert gmax[b, tile] == sims[b, row] and smax[b, w] == RM.f2key(S[b, row:row + 1])[0]


def test_pick_tiles_serves_every_grid_the_probe_allows():
    for waves in ((8,), (16,), (32,), (8, 16), (12, 24), (4,), (20, 28)):
        probes = [(97 + w - 1) // w for w in waves]
        t = M.pick_tiles(97, probes, at_least=12)
        assert t >= 12
        for w in waves:
            assert M.multi_tile_ok(t, w), (waves, t, w)
            c = (t + w - 1) // w
            n_w = (t + c - 1) // c
            assert c >= 3 and t - (n_w - 1) * c < c


def test_routing_tables():
    assert [M.nb_of(n) for n in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    assert M.kernel_id("f32", 384) == 1 and M.kernel_id("bf16", 384) == 2 and M.kernel_id("f32", 768, True) == 111
    assert M.dim_pad_of(100) == 128 and M.dim_pad_of(1000) == 1024 and M.dim_pad_of(64) == 64
    w = M.bf16_words(M.stored_rows(np.array([[1.0, -2.0, np.nan, 2.0 ** -133]], dtype=np.float32), "bf16"))
    assert w[0, :4].tolist() == [0x3F80, 0xC000, 0x7FC0, 0x0001]
