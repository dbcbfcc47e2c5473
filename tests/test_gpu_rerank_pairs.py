"""The reranker's token plane and pair kernels (rerank.RerankText, csrc/rr_pairs.hip) on the GPU: the plane bitwise against
rerank.model_plane, measure + write bitwise against rerank.model_pairs on tok / typ / pos / cu, ranges of the pair list,
the scan across workgroups, rows outside the plane and the limits the host refuses."""
import ctypes as C
import itertools

import numpy as np
import pytest

import wp_utf8_texts as U

pytestmark = pytest.mark.gpu

RR_E_INVALID = -1


def R():
    from review_recommender_amd import rerank
    return rerank


def two_letter_tokenizer():
    """676 single-piece words of two letters: n words give n tokens, and 509 of them fit 2000 characters."""
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + ["".join(p) for p in itertools.product("abcdefghijklmnopqrstuvwxyz", repeat=2)]
    return WordPieceTokenizer({w: i for i, w in enumerate(words)}), words[4:]


def words_of(words, n, start):
    return " ".join(words[(start + 7 * i) % len(words)] for i in range(n))


# ------------------------------------------------------------------------------------------------ the plane
def plane_docs(L):
    absent = U.SCRIPTS["kana"][1]                       # (not in the vocabulary: a word of it is one [UNK])
    big = (absent * 50 + " ") * 39                      # 1989 characters, 5889 bytes, 39 pieces: more than the window holds
    assert len(big) <= 2000 and len(big.encode()) > 4096
    rng = np.random.default_rng(5)
    docs = ["soft warm mug", "Café naïve Zoë Über “great” mug 5€", "", "a " * (L - 3), "a " * (L - 2), "   ",
            U.random_text(rng, 300, 0.3), big, "中文mug一丁 привет МИР", U.random_text(rng, 2500, 0.2),
            "lamp " * 500, "good mug Σ lamp", U.random_text(rng, 900, 0.6), "x" * 120 + " mug", "great"]
    return docs, {7, 11}


@pytest.mark.parametrize("L,chunk_docs,row_offset", [(512, 4, 0), (16, 3, 7), (512, 1000, 3)])
def test_plane_equals_the_model_bitwise(L, chunk_docs, row_offset):
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    tok = WordPieceTokenizer({w: i for i, w in enumerate(U.vocabulary())})
    docs, handed_back = plane_docs(L)
    want = R().model_plane(docs, tok, L)
    assert len(want[3]) == L - 3 == len(want[4]) and max(len(w) for w in want) == L - 3
    rt = R().RerankText.from_texts(docs, tok, L, 0, chunk_docs=chunk_docs, row_offset=row_offset)
    try:
        got = rt.tokens()
        off = rt.d_off.cpu().numpy()
        assert rt.n == len(docs) and rt.row_offset == row_offset and rt.max_length == L
        assert off.dtype == np.int64 and off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert rt.n_tokens == off[-1] and rt.nbytes == 2 * max(rt.n_tokens, 1) + 8 * (len(docs) + 1)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.uint16 and g.tolist() == w.tolist(), (i, docs[i][:40], len(g), len(w))
        from review_recommender_amd.wp_unicode import model_tokenize
        flagged = {i: model_tokenize(d[:2000], tok, L - 1)[2] for i, d in enumerate(docs)}
        assert set(rt.host_docs) == {i for i, why in flagged.items() if why}
        assert flagged[11] == "hard"
        if L == 512:                                    # (at L = 16 the window holds the 13 pieces of the long document)
            assert flagged[7] == "window" and set(rt.host_docs) >= handed_back
            if chunk_docs == 4:                         # the two hand-backs, and a chunk boundary, in different chunks
                assert len({i // chunk_docs for i in handed_back}) == 2
    finally:
        rt.close()


def test_plane_limits():
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    tok = WordPieceTokenizer({w: i for i, w in enumerate(U.vocabulary())})
    with pytest.raises(MemoryError, match='rerank="host"'):
        R().RerankText.from_texts(["soft mug"] * 10, tok, 512, 0, max_bytes=90)
    with pytest.raises(ValueError, match="max_length"):
        R().RerankText.from_texts(["soft mug"], tok, 2, 0)
    empty = R().RerankText.from_texts([], tok, 512, 0)
    assert empty.n == 0 and empty.n_tokens == 0 and empty.d_off.cpu().tolist() == [0]
    empty.close()


# ------------------------------------------------------------------------------------------------ measure + write
def pair_world(L, row_offset=0):
    """(handle, model plane, queries' ids, tokenizer): texts of 0, 1, avail // 2, avail // 2 + 1 and avail tokens, queries of
    0, 1 and avail."""
    tok, words = two_letter_tokenizer()
    avail = L - 3
    texts = [words_of(words, n, 11 * n) for n in (0, 1, avail // 2, avail // 2 + 1, avail)]
    queries = [words_of(words, n, 300 + n) for n in (0, 1, avail)]
    assert all(len(t) <= 2000 for t in texts)
    q_ids = [tok.text_ids(q) for q in queries]
    plane = R().model_plane(texts, tok, L)
    assert [len(p) for p in plane] == [0, 1, avail // 2, avail // 2 + 1, avail] and [len(q) for q in q_ids] == [0, 1, avail]
    rt = R().RerankText.from_texts(texts, tok, L, 0, row_offset=row_offset, chunk_docs=2)
    return rt, plane, q_ids, tok


def run_pairs(rt, rows, rr_k, q_ids, first_pair=0, n_pairs=None):
    import torch
    packed = R().pack_queries(q_ids, rt.max_length)
    assert not packed.host_queries
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).cuda()
    out = rt.pairs(d_rows, rr_k, packed, first_pair, n_pairs)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def assert_pairs_equal(got, want):
    for name, g, w in zip(("tok", "typ", "pos", "cu"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (name, g[:40], w[:40])


@pytest.mark.parametrize("L", [16, 17, 512])
def test_measure_and_write_equal_the_model_bitwise(L):
    rt, plane, q_ids, tok = pair_world(L)
    avail = L - 3
    try:
        seen = set()
        for shift in range(5):                          # every text in front of every query within the first rr_k = 4 columns
            rows = np.array([[(shift + b + j) % 5 for j in range(5)] for b in range(3)], dtype=np.int64)
            got = run_pairs(rt, rows, 4, q_ids)
            want = R().model_pairs(plane, rows, 5, 4, q_ids, L, tok.cls_id, tok.sep_id, 0, 12)
            assert_pairs_equal(got, want)
            rt.check()
            for b in range(3):
                for j in range(4):
                    n_a, n_b = len(q_ids[b]), len(plane[rows[b, j]])
                    ka, kb = R().keep_lengths(n_a, n_b, L)
                    seen.add(("no cut" if (ka, kb) == (n_a, n_b) else "text cut" if ka == n_a else "query cut" if kb == n_b
                              else "both cut") + (" tie" if n_a == n_b else ""))
        assert seen >= {"no cut", "no cut tie", "text cut", "query cut", "both cut tie"}, seen
        assert avail % 2 == (0 if L == 17 else 1)
    finally:
        rt.close()


def test_a_range_inside_the_pair_list_equals_the_slice():
    L = 16
    rt, plane, q_ids, tok = pair_world(L)
    try:
        rows = np.array([[4, 3, 2, 1, 0], [0, 4, 1, 3, 2], [2, 4, 4, 0, 1]], dtype=np.int64)
        tok_f, typ_f, pos_f, cu_f = run_pairs(rt, rows, 4, q_ids)
        for first, n in ((2, 7), (5, 1), (0, 12), (11, 1), (3, 0)):          # (2, 7): starts in query 0, ends in query 2
            got = run_pairs(rt, rows, 4, q_ids, first, n)
            a, b = cu_f[first], cu_f[first + n]
            assert_pairs_equal(got, (tok_f[a:b], typ_f[a:b], pos_f[a:b], cu_f[first:first + n + 1] - a))
            assert_pairs_equal(got, R().model_pairs(plane, rows, 5, 4, q_ids, L, tok.cls_id, tok.sep_id, first, n))
        rt.check()
    finally:
        rt.close()


@pytest.mark.parametrize("rr_k", [300, 900])             # 1 500 pairs; 4 500: more than one chunk of the device-wide scan
def test_cu_is_right_across_the_workgroups_of_the_scan(rr_k):
    L = 16
    rt, plane, q_ids, tok = pair_world(L)
    try:
        rng = np.random.default_rng(rr_k)
        q5 = [q_ids[i] for i in (2, 0, 1, 2, 1)]
        rows = rng.integers(0, 5, size=(5, rr_k + 3)).astype(np.int64)
        got = run_pairs(rt, rows, rr_k, q5)
        assert_pairs_equal(got, R().model_pairs(plane, rows, rr_k + 3, rr_k, q5, L, tok.cls_id, tok.sep_id, 0, 5 * rr_k))
        rt.check()
    finally:
        rt.close()


# ------------------------------------------------------------------------------------------------ faults
def status(rt):
    from review_recommender_amd import _lib
    bad = C.c_int32(-1)
    rc = _lib.load().rr_pairs_status(rt._h, C.byref(bad))
    return rc, bad.value


def test_rows_outside_the_plane_read_no_text_and_are_counted():
    L = 16
    rt, plane, q_ids, tok = pair_world(L, row_offset=7)
    try:
        rows = np.array([[7, 8, 9, 10, 11], [11, 6, 9, 8, 7], [10, 9, 12, 7, 8]], dtype=np.int64)     # 6: below, 12: above
        got = run_pairs(rt, rows, 4, q_ids)
        want = R().model_pairs(plane, rows, 5, 4, q_ids, L, tok.cls_id, tok.sep_id, 0, 12, row_offset=7)
        assert_pairs_equal(got, want)
        for p, b in ((5, 1), (10, 2)):
            a, e = got[3][p], got[3][p + 1]
            assert got[0][a:e].tolist() == [tok.cls_id] + q_ids[b] + [tok.sep_id, tok.sep_id]
            assert got[1][a:e].tolist() == [0] * (len(q_ids[b]) + 2) + [1]
        assert status(rt) == (RR_E_INVALID, 2)
        assert status(rt) == (0, 0)
        run_pairs(rt, rows, 4, q_ids, 0, 5)                               # pairs 0..4: none of the two
        assert status(rt) == (0, 0)
        run_pairs(rt, rows, 4, q_ids, 5, 1)
        with pytest.raises(ValueError, match="outside the plane"):
            rt.check()
    finally:
        rt.close()


def test_limits_the_host_checks_are_refused_and_nothing_is_written():
    import torch
    from review_recommender_amd import _lib
    L = 16
    rt, plane, q_ids, tok = pair_world(L)
    try:
        lib = _lib.load()
        packed = R().pack_queries(q_ids, L)
        d_q, at = rt.upload(packed)
        rows = torch.arange(15, dtype=torch.int64, device="cuda").reshape(3, 5) % 5
        keep = torch.full((12, 2), -7, dtype=torch.int32, device="cuda")
        cu = torch.full((13,), -7, dtype=torch.int32, device="cuda")
        ids = torch.full((3 * 12 * L,), -7, dtype=torch.int32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())

        def measure(pool=5, rr_k=4, max_length=L, first=0, n=12):
            return lib.rr_pairs_measure_dev(rt._h, p(rt.d_off), rt.n, 0, p(rows), pool, rr_k, p(d_q), 3, max_length, first, n,
                                            p(keep), p(cu), None)

        def write(pool=5, rr_k=4, first=0, n=12, n_tokens=12 * L):
            return lib.rr_pairs_write_dev(rt._h, p(rt.d_tok), p(rt.d_off), rt.n, 0, p(rows), pool, rr_k,
                                          C.c_void_p(d_q.data_ptr() + 4 * at), p(d_q), 3, tok.cls_id, tok.sep_id, first, n, p(keep),
                                          p(cu), n_tokens, p(ids), C.c_void_p(ids.data_ptr() + 4 * 12 * L),
                                          C.c_void_p(ids.data_ptr() + 8 * 12 * L), None)

        for bad in (dict(rr_k=6), dict(first=6, n=7), dict(first=-1, n=1), dict(max_length=2), dict(rr_k=0)):
            assert measure(**bad) == RR_E_INVALID, bad
            assert lib.rr_last_error()
        for bad in (dict(rr_k=6), dict(first=6, n=7), dict(n_tokens=(1 << 27) + 1), dict(n_tokens=-1)):
            assert write(**bad) == RR_E_INVALID, bad
        torch.cuda.synchronize()
        assert bool((keep == -7).all()) and bool((cu == -7).all()) and bool((ids == -7).all())
        assert status(rt) == (0, 0)
        # the same buffers through the calls as they are meant: written, and equal to the model
        assert measure() == 0 and write() == 0
        torch.cuda.synchronize()
        want = R().model_pairs(plane, rows.cpu().numpy(), 5, 4, q_ids, L, tok.cls_id, tok.sep_id, 0, 12)
        n_tok = int(cu[12])
        assert np.array_equal(cu.cpu().numpy(), want[3]) and np.array_equal(ids[:n_tok].cpu().numpy(), want[0])
        assert np.array_equal(ids[12 * L:12 * L + n_tok].cpu().numpy(), want[1])
        assert np.array_equal(ids[24 * L:24 * L + n_tok].cpu().numpy(), want[2])
        # lengths that do not fit the offsets: the pair is not written, and counted
        keep[3, 1] = 1000
        ids.fill_(-7)
        assert write() == 0
        torch.cuda.synchronize()
        a, e = int(cu[3]), int(cu[4])
        assert bool((ids[a:e] == -7).all()) and np.array_equal(ids[:a].cpu().numpy(), want[0][:a])
        assert status(rt) == (RR_E_INVALID, 1)
    finally:
        rt.close()
