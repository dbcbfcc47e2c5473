"""The CPU model of the review-cleaning kernel (review-recommender_amd/textprep.py: model_clean) against the reference's
normalize_text and looks_spammy, restated in textprep_texts.py (nlp/11_build_product_embeddings.py:22-39).  No GPU: the kernel
itself is held to this model in test_gpu_textprep.py."""
import re

import pytest

from review_recommender_amd import textprep as T

import textprep_texts as X


def check_against_reference(texts, spam=True):
    """Wherever the model does not say needs_host, (normalised, short, spam) equals the reference's.  Returns the number of
    texts the model leaves to the host."""
    left = 0
    for s in texts:
        got, st = T.model_clean(s, spam)
        if st & T.NEEDS_HOST:
            assert st == T.NEEDS_HOST and got == ""
            left += 1
            continue
        want, short, spammy = X.ref_clean(s)
        assert got == want, (s[:80], got[:80], want[:80])
        assert bool(st & T.SHORT) == short, (s[:80], st)
        if spam:
            assert bool(st & T.SPAM) == spammy, (s[:120], st)
        else:
            assert not st & T.SPAM
    return left


def test_constants_equal_the_library(hip):
    import ctypes as C
    w, t, p = C.c_int32(), C.c_int32(), C.c_int32()
    assert hip.rr_textprep_limits(C.byref(w), C.byref(t), C.byref(p)) == 0
    assert (w.value, t.value, p.value) == (T.WINDOW_BYTES, T.TILE_BYTES, T.SLICE_BYTES)
    assert T.WINDOW_BYTES >= 16384 and T.WINDOW_BYTES % T.TILE_BYTES == 0 and T.TILE_BYTES % T.SLICE_BYTES == 0
    assert (T.MIN_CHARS, T.MAX_CHARS) == (X.MIN_TEXT_LEN, X.MAX_TEXT_LEN)


def test_whitespace_set_is_str_isspace_and_re_s():
    ws = re.compile(r"\s")
    for c in range(0x110000):
        if 0xD800 <= c <= 0xDFFF:
            continue
        ch = chr(c)
        assert (c in T.WHITESPACE) == ch.isspace() == bool(ws.fullmatch(ch)), hex(c)
        got, st = T.model_clean("ab" + ch + "cd", spam=False)             # between two letters
        assert st == T.SHORT and got == ("ab cd" if ch.isspace() else "ab" + ch + "cd"), hex(c)
    assert len(T.WHITESPACE) == 29
    # each is at least as long in UTF-8 as the space that replaces it: the normalised text fits the raw text's place
    assert all(len(chr(c).encode()) >= 1 for c in T.WHITESPACE)


def test_ignorecase_set_is_what_re_folds_onto_the_patterns_letters():
    letters = [re.compile(re.escape(l), re.I) for l in X.PATTERN_LETTERS]
    others = [re.compile(re.escape(l), re.I) for l in ":/. "]
    for c in range(0x80, 0x110000):
        if 0xD800 <= c <= 0xDFFF:
            continue
        ch = chr(c)
        folded = any(p.fullmatch(ch) for p in letters)
        assert not any(p.fullmatch(ch) for p in others), hex(c)
        assert folded == (c in T.FOLDED), hex(c)
        if folded or c < 0x3000 and c % 7 == 0:                            # the model's answer, for all of them and a sample of the rest
            pad = "" if ch.isspace() else ch
            assert (T.model_clean("abcdefghij" + ch, True)[1] == T.NEEDS_HOST) == folded, hex(c)
            assert T.model_clean("abcdefghij" + ch, False) == ("abcdefghij" + pad, 0), hex(c)
    assert sorted(T.FOLDED) == [0x130, 0x131, 0x17F]


def test_crafted_texts():
    texts = X.crafted(T.WINDOW_BYTES)
    assert len(texts) >= 300
    left = check_against_reference(texts, True)
    assert 7 <= left <= 20                      # the three folded code points and the texts beyond the window, nothing else
    assert check_against_reference(texts, False) < left
    # what the list is there for happens in it
    res = [T.model_clean(s, True) for s in texts]
    assert sum(st == T.SPAM for _, st in res) > 80 and sum(st == 0 for _, st in res) > 80 and sum(st & T.SHORT > 0 for _, st in res) > 20
    assert any(len(g) == T.MAX_CHARS and g.endswith(" ") for g, _ in res)            # the cut right behind a collapsed space
    assert any(len(g) == T.MAX_CHARS and g.endswith(X.E4) for g, _ in res)           # ... and on a 4-byte character
    for s, want in (("http:// www. " + X.fill(10), 0), ("http://ahttp://b " + X.fill(10), 0), ("wwww.x www.y " + X.fill(10), T.SPAM),
                    ("i received thisfree", T.SPAM), ("free and i received this", 0), ("aAaAaAaAaAaA bcd", 0),
                    ("", T.SHORT), (" \t\n ", T.SHORT), (X.E3 * 9, T.SHORT), (X.E3 + X.E2 * 9, 0)):
        assert T.model_clean(s, True)[1] == want, s
    wide = (X.E4 + "\U0001F601") * 2000
    pad = T.WINDOW_BYTES - len(wide.encode())
    assert T.model_clean(" " * pad + wide, True) == (wide, 0) and T.model_clean(" " * (pad + 1) + wide, True) == ("", T.NEEDS_HOST)
    for c in sorted(T.FOLDED):
        assert T.model_clean(X.fill(12) + chr(c), True)[1] == T.NEEDS_HOST
        assert T.model_clean(X.fill(12) + chr(c), False) == (X.fill(12) + chr(c), 0)


def test_random_texts():
    texts = X.random_texts(4000, 5)
    left = check_against_reference(texts, True)
    assert left <= 0.05 * len(texts) and left == 0      # the generator's alphabet holds nothing the kernel leaves to the host
    assert check_against_reference(texts, False) == 0
    st = [T.model_clean(s, True)[1] for s in texts]
    assert sum(x & T.SPAM > 0 for x in st) > 400 and sum(x == 0 for x in st) > 400 and sum(x & T.SHORT > 0 for x in st) > 100


def test_boundary_variants_agree_too():
    assert check_against_reference(X.boundary_variants(T.TILE_BYTES, T.SLICE_BYTES), True) == 0


def test_malformed_bytes_are_left_to_the_host():
    for raw in (b"abc\xff" + b"d" * 10, b"\xc3", b"ab\xe4\xb8", b"\x80abc", b"\xc0\xaf" + b"a" * 10, b"\xed\xa0\x80" + b"a" * 10,
                b"\xf4\x90\x80\x80" + b"a" * 10, b"a\xe4\xb8\xadb\x80" + b"a" * 10, b"\xf0\x9f\x98" + b"a" * 10):
        assert T.model_clean_bytes(raw, False) == (b"", T.NEEDS_HOST), raw
    assert T.model_clean("ab\ud800cdefghijk", False) == ("", T.NEEDS_HOST)


def test_host_spam_rule_is_the_reference():
    from review_recommender_amd import embed
    for s in X.crafted(T.WINDOW_BYTES)[::3]:
        t = X.ref_normalize(s)
        assert embed.normalize_text(s) == t and embed.looks_spammy(t) == X.ref_spammy(t)
