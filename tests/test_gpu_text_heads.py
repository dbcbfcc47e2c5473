"""The head kernels (csrc/rr_textprep.hip: rr_textprep_head_measure_dev / rr_textprep_head_write_dev) against their CPU
model, textprep.model_head (itself held to normalize_text and str[:k] in test_head_model.py): byte for byte, with the lengths
and the status words, over one crafted batch of the smallest shapes at which a streamed, tiled walk can go wrong."""
import ctypes as C

import numpy as np
import pytest

from review_recommender_amd import _lib
from review_recommender_amd import textprep as T

pytestmark = pytest.mark.gpu

WS3 = b"\xe2\x80\x80"         # U+2000
WIDE = "\U0001F600".encode()         # F0 9F 98 80


@pytest.fixture(scope="module")
def tp():
    t = T.TextPrep(0)
    yield t
    t.close()


def tile_bytes():
    window, tile, per = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.load().rr_textprep_limits(C.byref(window), C.byref(tile), C.byref(per)), "rr_textprep_limits")
    return window.value, tile.value, per.value


def crafted(k: int):
    window, tile, per = tile_bytes()
    cjk = "中".encode()

    def upto(n):                      # n bytes of well-formed text with few code points: a head of 4000 reaches past a tile
        return cjk * ((n - 16) // 3) + b"a" * (n - 3 * ((n - 16) // 3))

    docs = [b"", b"abcdefghi", cjk * 10, b"   \t ", b" lead", b"x" * k, b"y" * (k + 1), cjk * k, cjk * (k + 1),
            ("é " * k).encode(), b" \n" + b"ab  " * k]
    docs.append(upto(tile - 5) + b" \t\n " * 3 + b"after the edge " * 3)                       # a whitespace run over a tile edge
    docs.append(upto(2 * tile - 1) + WS3 * 4 + b"second edge")
    for s in (1, 2):                                                                              # a 3-byte whitespace, split
        docs.append(upto(tile - s) + WS3 + b"b after")
        docs.append(upto(tile - s) + WS3)
        docs.append(b"q" * (tile - s) + WS3 + b"r")
    for s in (1, 2, 3):                                                                           # a 4-byte letter, split
        docs.append(upto(tile - s) + WIDE + b"b after")
        docs.append(upto(tile - s - 1) + b" " + WIDE)
        docs.append(b"q" * (tile - s) + WIDE)
    for s in (0, 1, 2, 3):                                                                        # a slice edge inside a tile
        docs.append(b"ab" + b"c" * (per - 2 - s) + WIDE + WS3 + b"zz" + WS3 + WS3 + cjk)
    docs.append(b"head" + b" " * (window + 700) + b"tail words")                                 # a run longer than the window
    docs.append(b"head" + WS3 * (window // 3 + 100) + b"tail")
    long = b"x" * 200_000                                                                         # the head ends in the first tile
    docs.append(long)
    docs.append(b"word " * 40_000)
    docs.append(long[:k] + b"\xff" + long[k + 1:])                                               # one byte behind the stop point
    docs.append(long[:k - 1] + b"\xff" + long[k:])                                               # the last code point of the walk
    docs.append(long[:k // 2] + b"\x80" + long[k // 2 + 1:])                                     # inside the walk
    docs.append(b"x" * (k - 1) + b"  y" + b"z" * 50)                                             # the pending space is the last emission
    docs.append(b"x" * (k - 1) + b"  \xff" + b"z" * 50)                                          # ... and what made it due is malformed
    docs.append(b"x" * (k - 1) + b" \t \n")                                                      # all whitespace after k - 1 emissions
    docs.append(b"x" * k + b"\xe2\x80")                                                          # truncated, behind the stop
    docs.append(upto(tile - 1) + b"\xe2\x80")                                                    # truncated at the document's end, over an edge
    docs.append(upto(tile - 2) + b"\xf0\x9f\x98" + b"a")                                         # wrong continuation over an edge
    docs.append(upto(tile) + b"\x80" + b"a")                                                     # a stray continuation byte first in a tile
    docs.append(upto(tile - 1) + b"\xed\xa0\x80")                                                # a surrogate over an edge
    return docs


def compare(docs, rows, k, norm, min_chars, got):
    out, out_off, lens, st = got
    src = range(len(docs)) if rows is None else rows
    assert len(lens) == len(st) == len(src) == len(out_off) - 1
    at = 0
    for j, i in enumerate(src):
        text, status = T.model_head(docs[i], k, norm, min_chars)
        assert (int(st[j]), int(lens[j])) == (status, len(text)), (j, i, docs[i][:40], k, norm, int(st[j]), status, int(lens[j]), len(text))
        assert int(out_off[j]) == at, (j, i)
        if status == 0:
            assert out[at:at + len(text)].tobytes() == text, (j, i, docs[i][:40], k, norm)
            at += len(text)
    assert int(out_off[-1]) == at
    assert (out[at:] == 0xEE).all(), "bytes written behind the last head"


def test_heads_equal_the_model_byte_for_byte(tp):
    rng = np.random.default_rng(7)
    seen = set()
    for k in (7, 4000):
        docs = crafted(k)
        perm = rng.permutation(len(docs)).tolist()
        rows = perm + perm[:9] + [perm[3]] * 3                     # permutes and repeats
        for norm in (True, False):
            for r in (None, rows):
                got = tp.head_docs(docs, k, norm, T.MIN_CHARS, doc_rows=r)
                tp.check()
                compare(docs, r, k, norm, T.MIN_CHARS, got)
                seen |= set(int(s) for s in got[3])
    assert seen == {0, T.SHORT, T.NEEDS_HOST}
    # no filter, no documents, and one document
    docs = crafted(7)
    compare(docs, None, 7, True, 0, tp.head_docs(docs, 7, True, 0))
    compare([], None, 7, True, 0, tp.head_docs([], 7, True, 0))
    one = [b"word " * 40_000]
    compare(one, None, 4000, True, 10, tp.head_docs(one, 4000, True, 10))
    tp.check()


def test_a_refused_call_writes_nothing_and_is_reported(tp):
    import torch
    docs = [b"first document here", b"   the second   one  ", b"and a third document"]
    blob = b"".join(docs)
    good_off = np.zeros(4, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=good_off[1:])
    k, norm, minc = 12, True, 0
    want = [T.model_head(d, k, norm, minc)[0] for d in docs]
    total = sum(len(w) for w in want)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    d_text = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    def measure(off, rows, n):
        d_off, d_rows = up(off, np.int64), (None if rows is None else up(rows, np.int32))
        d_len, d_st = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
        tp.head_measure(d_text.data_ptr(), len(blob), d_off.data_ptr(), len(off) - 1, None if rows is None else d_rows.data_ptr(), n,
                        k, norm, minc, d_len.data_ptr(), d_st.data_ptr(), st.cuda_stream)
        st.synchronize()
        return d_len, d_st

    def write(off, rows, n, d_len, d_st, cap):
        d_off, d_rows = up(off, np.int64), (None if rows is None else up(rows, np.int32))
        d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        tp.head_offsets(d_len.data_ptr(), d_st.data_ptr(), n, d_out_off.data_ptr(), st.cuda_stream)
        d_out = torch.full((total + 16,), 0xEE, dtype=torch.uint8, device=dev)
        tp.head_write(d_text.data_ptr(), len(blob), d_off.data_ptr(), len(off) - 1, None if rows is None else d_rows.data_ptr(), n,
                      k, norm, minc, d_len.data_ptr(), d_st.data_ptr(), d_out.data_ptr(), cap, d_out_off.data_ptr(), st.cuda_stream)
        st.synchronize()
        return d_out.cpu().numpy()

    def refused():
        with pytest.raises(ValueError, match="rr_textprep_status"):
            tp.check()
        tp.check()                                                  # the count was taken: the next check is clean

    d_len, d_st = measure(good_off, None, 3)
    tp.check()
    assert d_len.cpu().tolist() == [len(w) for w in want] and d_st.cpu().tolist() == [0, 0, 0]
    assert write(good_off, None, 3, d_len, d_st, total)[:total].tobytes() == b"".join(want)
    tp.check()

    for off, rows in ((np.array([0, 30, 19, len(blob)]), None),                # offsets that decrease
                      (np.array([0, 19, 40, len(blob) + 1]), None),            # ... that leave the text
                      (good_off, [0, 3, 1]), (good_off, [-1, 1, 2])):          # a source row outside the documents
        bad_len, bad_st = measure(off, rows, 3)
        assert bad_len.cpu().tolist() == [0, 0, 0] and bad_st.cpu().tolist() == [T.NEEDS_HOST] * 3
        refused()
        assert (write(off, rows, 3, d_len, d_st, total) == 0xEE).all()        # (lengths and status words of the good call)
        refused()
    assert (write(good_off, None, 3, d_len, d_st, total - 1) == 0xEE).all()   # a capacity one byte too small
    refused()
    assert write(good_off, None, 3, d_len, d_st, total)[:total].tobytes() == b"".join(want)
    tp.check()
    with pytest.raises(ValueError, match="max_chars"):
        tp.head_measure(d_text.data_ptr(), len(blob), up(good_off, np.int64).data_ptr(), 3, None, 3, -1, True, 0, d_len.data_ptr(),
                        d_st.data_ptr(), st.cuda_stream)
