"""The review-cleaning stages on the GPU (csrc/rr_textprep.hip through review-recommender_amd/textprep.py): the clean kernel
against its CPU model (textprep.model_clean_bytes, itself held to the reference in test_textprep_model.py), dedup against
pandas' drop_duplicates, compaction against numpy, and a ReviewIndex made from device rows against one made from host rows."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from review_recommender_amd import _lib, synth
from review_recommender_amd import textprep as T

import textprep_texts as X

pytestmark = pytest.mark.gpu

MALFORMED = [b"abc\xff" + b"d" * 10, b"\xc3", b"ab\xe4\xb8", b"\x80abc", b"\xc0\xaf" + b"a" * 10, b"\xed\xa0\x80" + b"a" * 10,
             b"\xf4\x90\x80\x80" + b"a" * 10, b"a\xe4\xb8\xadb\x80" + b"a" * 10, b"\xf0\x9f\x98" + b"a" * 10,
             b"ab " * 5 + b"\xe4\xb8", b"x" * (T.SLICE_BYTES - 1) + b"\xf0\x9f\x98", b"x" * (T.TILE_BYTES - 2) + b"\xf0\x9f\x98\x80\x80" + b"y" * 9]


@pytest.fixture(scope="module")
def tp():
    t = T.TextPrep(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def documents():
    texts = X.crafted(T.WINDOW_BYTES) + X.random_texts(3000, 11) + X.boundary_variants(T.TILE_BYTES, T.SLICE_BYTES)
    docs = [s.encode("utf-8") for s in texts] + MALFORMED
    return docs, {spam: [T.model_clean_bytes(d, spam) for d in docs] for spam in (True, False)}


def compare(docs, want, out, lens, st, off=None):
    if off is None:
        off = np.zeros(len(docs) + 1, dtype=np.int64)
        np.cumsum([len(d) for d in docs], out=off[1:])
    assert len(lens) == len(st) == len(docs)
    for i, (text, status) in enumerate(want):
        assert st[i] == status and lens[i] == len(text), (i, docs[i][:60], st[i], status, lens[i], len(text))
        slot = out[off[i]:off[i + 1]]
        assert slot[:len(text)].tobytes() == text, (i, docs[i][:60])
        assert (slot[len(text):] == 0xEE).all(), (i, "bytes written behind the text")


@pytest.mark.parametrize("spam", [True, False])
def test_clean_equals_the_model(tp, documents, spam):
    docs, want = documents
    out, lens, st = tp.clean_docs(docs, spam)
    tp.check()
    compare(docs, want[spam], out, lens, st)
    n_host = int(np.count_nonzero(st == T.NEEDS_HOST))
    print(f"spam={spam}: {len(docs)} documents, {n_host} left to the host, {int(np.count_nonzero(st & T.SPAM))} spam, "
          f"{int(np.count_nonzero(st & T.SHORT))} short")
    assert n_host >= len(MALFORMED) and (st[st != T.NEEDS_HOST] & T.NEEDS_HOST == 0).all()
    assert out[-1] == 0xEE                                          # nothing behind the last document


def test_clean_in_place_and_small_batches(tp, documents):
    import torch
    docs, want = documents
    docs, want = docs[:600], want[True][:600]
    blob = b"".join(docs)
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    d_text = torch.from_numpy(np.frombuffer(blob + b"\xee", dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off).cuda()
    d_len = torch.zeros(len(docs), dtype=torch.int32, device="cuda")
    d_st = torch.zeros(len(docs), dtype=torch.int32, device="cuda")
    tp.clean(d_text.data_ptr(), len(blob), d_off.data_ptr(), len(docs), True, d_text.data_ptr(), d_len.data_ptr(), d_st.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tp.check()
    out, lens, st = d_text.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy()
    for i, (text, status) in enumerate(want):
        assert st[i] == status and lens[i] == len(text) and out[off[i]:off[i] + len(text)].tobytes() == text, i
    assert out[-1] == 0xEE
    # one document, and none
    one = [b"  one  review\r\nabout http://a and www.b  "]
    compare(one, [T.model_clean_bytes(one[0], True)], *tp.clean_docs(one, True))
    out, lens, st = tp.clean_docs([], True)
    assert len(lens) == 0 and len(st) == 0 and (out == 0xEE).all()
    tp.check()


def test_broken_offsets_are_reported_and_nothing_is_written_for_them(tp):
    docs = [b"first review, fine  ", b"second review", b"third review, also fine"]      # 20, 13 and 23 bytes
    good = np.array([0, 20, 33, 56], dtype=np.int64)
    for bad_off, bad_doc in ((np.array([0, 20, 18, 56]), 1), (np.array([0, 20, 33, 57]), 2), (np.array([-1, 20, 33, 56]), 0),
                             (np.array([0, 20, 33 + (1 << 40), 56]), None)):
        out, lens, st = tp.clean_docs(docs, True, offsets=bad_off)
        with pytest.raises(ValueError, match="offsets that decrease or leave the text"):
            tp.check()
        broken = [i for i in range(3) if bad_off[i] < 0 or bad_off[i + 1] < bad_off[i] or bad_off[i + 1] > 56]
        assert (bad_doc in broken) if bad_doc is not None else broken == [1, 2]
        for i in range(3):
            if i in broken:
                assert st[i] == T.NEEDS_HOST and lens[i] == 0
            else:
                a, b = int(bad_off[i]), int(bad_off[i + 1])
                text, status = T.model_clean_bytes(b"".join(docs)[a:b], True)
                assert st[i] == status and lens[i] == len(text) and out[a:a + len(text)].tobytes() == text
        written = np.zeros(len(out), dtype=bool)
        for i in range(3):
            if i not in broken:
                written[int(bad_off[i]):int(bad_off[i]) + int(lens[i])] = True
        assert (out[~written] == 0xEE).all()
    tp.check()                                                       # the counter was reset
    out, lens, st = tp.clean_docs(docs, True, offsets=good)
    tp.check()
    assert (st == 0).all()


# ---------------------------------------------------------------------------------------------- dedup, compact
def dedup_world(seed=4, n=2000, n_groups=50):
    rng = np.random.default_rng(seed)
    words = synth.text_corpus(n, seed, mean_len=12)
    group = rng.integers(0, n_groups, n).astype(np.int32)
    status = np.zeros(n, dtype=np.int32)
    status[rng.choice(n, 150, replace=False)] = rng.choice([T.SHORT, T.SPAM, T.SHORT | T.SPAM, T.NEEDS_HOST], 150)
    texts = [w.encode() for w in words]
    r = iter(rng.permutation(n)[:400].tolist())
    for _ in range(30):                                   # the same text in one group, three times
        a, b, c = next(r), next(r), next(r)
        texts[b] = texts[c] = texts[a]
        group[b] = group[c] = group[a]
        status[[a, b, c]] = 0
    for _ in range(30):                                   # the same text in two groups: both stay
        a, b = next(r), next(r)
        texts[b] = texts[a]
        group[b] = (group[a] + 1) % n_groups
    for _ in range(30):                                   # a prefix of another text, and a difference in the last byte only
        a, b, c = next(r), next(r), next(r)
        texts[b] = texts[a][:-3]
        texts[c] = texts[a][:-1] + (b"#" if texts[a][-1:] != b"#" else b"!")
        group[b] = group[c] = group[a]
        status[[a, b, c]] = 0
    for _ in range(30):                                   # duplicates of a document that is already dropped: the later ones count
        a, b, c = sorted([next(r), next(r), next(r)])
        texts[b] = texts[c] = texts[a]
        group[b] = group[c] = group[a]
        status[a], status[b], status[c] = T.SPAM, 0, 0
    texts[next(r)] = b""                                  # empty survivors are equal to each other too
    e1, e2 = next(r), next(r)
    texts[e1] = texts[e2] = b""
    group[e2] = group[e1]
    status[[e1, e2]] = 0
    long = ("review " * 1500).encode()                    # longer than one pass of a wave's compare loop
    l1, l2, l3 = next(r), next(r), next(r)
    texts[l1], texts[l2], texts[l3] = long, long, long[:-1] + b"?"
    group[l2] = group[l3] = group[l1]
    status[[l1, l2, l3]] = 0
    return texts, group, status


def slots_of(texts, slack_seed=1):
    """Offsets that leave unused bytes behind every text, as the clean stage does."""
    rng = np.random.default_rng(slack_seed)
    size = np.array([len(t) for t in texts]) + rng.integers(0, 9, len(texts))
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum(size, out=off[1:])
    blob = np.full(int(off[-1]) + 1, 0x2A, dtype=np.uint8)
    for t, a in zip(texts, off[:-1]):
        blob[a:a + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return blob, off


def test_dedup_equals_drop_duplicates(tp):
    import torch
    texts, group, status = dedup_world()
    n = len(texts)
    blob, off = slots_of(texts)
    frame = pd.DataFrame({"sku": group, "__txt": texts})
    alive = frame[status == 0]
    kept = alive.drop_duplicates(subset=["sku", "__txt"]).index.to_numpy()      # nlp/11...:117
    want = status.copy()
    want[np.setdiff1d(alive.index.to_numpy(), kept)] |= T.DUP
    assert 80 < np.count_nonzero(want & T.DUP) < 200
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_text, d_off, d_len, d_grp = dev(blob), dev(off), dev(np.array([len(t) for t in texts], dtype=np.int32)), dev(group)
    st = torch.cuda.current_stream().cuda_stream
    for bits in (64, 3, 64, 3, 4):
        d_st = dev(status)
        tp.dedup(d_text.data_ptr(), len(blob) - 1, d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr(), d_st.data_ptr(), n, bits, st)
        got = d_st.cpu().numpy()
        tp.check()
        assert np.array_equal(got, want), (bits, np.flatnonzero(got != want)[:10])
    tp.dedup(d_text.data_ptr(), len(blob) - 1, d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr(), d_st.data_ptr(), 0, 64, st)
    with pytest.raises(ValueError, match="hash_bits"):
        tp.dedup(d_text.data_ptr(), len(blob) - 1, d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr(), d_st.data_ptr(), n, 0, st)


def check_compact(tp, texts, status):
    """rr_textprep_compact_dev against numpy: counts, offsets (a cumsum of the kept lengths), src_row and the gathered text
    (every survivor at its rank)."""
    import torch
    n = len(texts)
    blob, off = slots_of(texts, 2)
    lens = np.array([len(t) for t in texts], dtype=np.int32)
    keep = np.flatnonzero(status == 0)
    want_text = b"".join(texts[i] for i in keep)
    want_off = np.concatenate([[0], np.cumsum(lens[keep], dtype=np.int64)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1, a.dtype))).cuda()   # (no NULL for n = 0)
    d_text, d_off, d_len, d_st = dev(blob), dev(off), dev(lens), dev(status.astype(np.int32))
    o_text = torch.full((len(want_text) + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    o_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    o_src = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    o_cnt = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    tp.compact(d_text.data_ptr(), len(blob) - 1, d_off.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), n, o_text.data_ptr(),
               len(want_text), o_off.data_ptr(), o_src.data_ptr(), o_cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tp.check()
    m = len(keep)
    assert o_cnt.cpu().tolist() == [m, len(want_text)]
    assert np.array_equal(o_off.cpu().numpy()[:m + 1], want_off) and (o_off.cpu().numpy()[m + 1:] == -1).all()
    assert np.array_equal(o_src.cpu().numpy()[:m], keep) and (o_src.cpu().numpy()[m:] == -1).all()
    got = o_text.cpu().numpy()
    assert got[:len(want_text)].tobytes() == want_text and (got[len(want_text):] == 0xEE).all()


@pytest.mark.parametrize("case", ["mixed", "all dropped", "none dropped", "only the last kept"])
def test_compact_equals_the_host(tp, case):
    texts, _, status = dedup_world(seed=6, n=1500)
    if case == "all dropped":
        status[:] = T.SHORT
    elif case == "none dropped":
        status[:] = 0
    elif case == "only the last kept":
        status[:] = T.DUP
        status[-1] = 0
    check_compact(tp, texts, status)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2049])
def test_compact_at_the_edges_of_the_scan_chunks(tp, n):
    """The ranking kernel scans the documents in chunks of 1024 and carries (count, bytes) from chunk to chunk: no document,
    one, a chunk less one, a full chunk, one more, and two chunks and one.  Every third document is dropped."""
    rng = np.random.default_rng(100 + n)
    texts = [rng.integers(97, 123, int(rng.integers(0, 12)), dtype=np.uint8).tobytes() for _ in range(n)]
    status = np.zeros(n, dtype=np.int32)
    status[2::3] = [T.SHORT, T.SPAM, T.DUP, T.NEEDS_HOST][n % 4]
    check_compact(tp, texts, status)


def test_review_index_from_device_rows_equals_the_host_one(hip):
    """rr_reviews_create_dev against rr_reviews_create on the shapes of test_gpu_reviews.py's batched case: the same rows
    from device memory give the same review ids and the same score BITS (the normalisation is the same kernel)."""
    import torch
    from test_gpu_reviews import make
    from review_recommender_amd.reviews import ReviewIndex
    meta, V, reviews, E = make(2500, 15000, seed=9)
    skus = meta["sku"].tolist()
    host = ReviewIndex(reviews, E, skus)
    devi = ReviewIndex.from_device_rows(reviews, torch.from_numpy(E).cuda(), skus)
    assert np.array_equal(host.indptr, devi.indptr) and np.array_equal(host.ids, devi.ids) and host.texts == devi.texts
    B, pool = 9, 150
    rng = np.random.default_rng(3)
    q = torch.from_numpy(synth.unit_rows(B, 384, 77)).cuda()
    rows = torch.from_numpy(np.stack([rng.permutation(2500)[:pool] for _ in range(B)]).astype(np.int64)).cuda()

    def best(ri, max_rows):
        score = torch.empty((B, pool), dtype=torch.float32, device="cuda")
        rid = torch.empty((B, pool), dtype=torch.int32, device="cuda")
        _lib.check(hip.rr_reviews_best_cut_dev(ri.handle, C.c_void_p(q.data_ptr()), B, C.c_void_p(rows.data_ptr()), pool, 0, max_rows,
                                               C.c_void_p(score.data_ptr()), C.c_void_p(rid.data_ptr()), None), "rr_reviews_best_cut_dev")
        torch.cuda.synchronize()
        return score.cpu().numpy().view(np.uint32), rid.cpu().numpy()

    for max_rows in (300000, 150, 37):
        a, b = best(host, max_rows), best(devi, max_rows)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]) and (a[1] >= 0).sum() > 30
    with pytest.raises(ValueError):
        ReviewIndex.from_device_rows(reviews, torch.from_numpy(E[:-1]).cuda(), skus)
    host.close()
    devi.close()
