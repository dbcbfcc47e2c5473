"""textprep.model_head -- the statement the head kernels (csrc/rr_textprep.hip: rr_tp_head) are tested against -- checked
against the reference's own words: embed.normalize_text (strip, \\s+ -> " ", [:4000]) and str[:k]."""
import random
import re

import pytest

from review_recommender_amd import embed, textprep as T

CUTS = (1, 9, 10, 11, 4000)
SPACES = sorted(T.WHITESPACE)
LETTERS = ["a", "Z", "7", ".", "é", "Ж", "中", "€", "\U0001F600", "\U00010348"]    # 1, 2, 3 and 4 bytes


def normalize(s: str, k: int) -> str:
    """embed.normalize_text with the cut at k instead of 4000."""
    return re.sub(r"\s+", " ", s.replace("\r", " ").replace("\n", " ").strip())[:k]


def head(s: str, k: int, norm: bool, min_chars: int = 0):
    out, st = T.model_head(s.encode("utf-8"), k, norm, min_chars)
    return out.decode("utf-8"), st


def test_the_cut_of_normalize_text_is_the_models_default_use():
    s = "  x y " * 3000
    assert head(s, embed.MAX_TEXT_LEN, True)[0] == embed.normalize_text(s)
    assert T.MAX_CHARS == embed.MAX_TEXT_LEN and T.MIN_CHARS == embed.MIN_TEXT_LEN


@pytest.mark.parametrize("k", CUTS)
def test_every_whitespace_code_point_leading_trailing_doubled_and_between(k):
    assert len(SPACES) == 29 and all(chr(c).isspace() and re.fullmatch(r"\s", chr(c)) for c in SPACES)
    for c in SPACES:
        w = chr(c)
        for s in (w + "ab", "ab" + w, "ab" + w + w + "cd", "ab" + w + "cd", w + w + "ab" + w + "c" + w + w, w, w + w,
                  "abcdefgh" + w + "ij", "abcdefghi" + w + "jk", "abcdefghij" + w + "k"):
            assert head(s, k, True) == (normalize(s, k), 0), (hex(c), s, k)
            assert head(s, k, False) == (s[:k], 0), (hex(c), s, k)


def test_random_strings_against_normalize_text_and_the_slice():
    rng = random.Random(20240611)
    n = 0
    for _ in range(2400):
        parts = []
        for _ in range(rng.randrange(0, 40)):
            r = rng.random()
            parts.append(chr(rng.choice(SPACES)) if r < 0.35 else rng.choice(LETTERS) if r < 0.75 else chr(rng.randrange(0x21, 0x7F)))
        s = "".join(parts)
        for k in (rng.choice(CUTS), rng.randrange(1, 45)):
            want = normalize(s, k)
            assert head(s, k, True, 10) == (want, T.SHORT if len(want) < 10 else 0), (s, k)
            assert head(s, k, False, 10) == (s[:k], T.SHORT if len(s[:k]) < 10 else 0), (s, k)
        n += 1
    assert n >= 2000


def test_the_space_as_the_kth_emission_and_no_trailing_space():
    assert head("abc  d", 4, True) == ("abc ", 0) == (normalize("abc  d", 4), 0)       # the space is the 4th emission
    assert head("abc  d", 5, True) == ("abc d", 0)
    assert head("abc  \n", 4, True) == ("abc", 0)                                 # all whitespace after k - 1 emissions
    assert head("abc  \n", 4000, True) == ("abc", 0)
    assert head("  ", 5, True) == ("", 0) and head("", 5, False) == ("", 0)
    assert head("abc", 0, True) == ("", 0)


def test_status_short_counts_code_points_of_the_head():
    assert head("123456789", 4000, True, 10)[1] == T.SHORT and head("1234567890", 4000, True, 10)[1] == 0
    assert head("1234 6789", 4000, True, 10)[1] == T.SHORT and head("1234  67890", 4000, True, 10) == ("1234 67890", 0)
    assert head("中" * 10, 4000, False, 10)[1] == 0 and head("中" * 9, 4000, False, 10)[1] == T.SHORT
    assert head("1234567890", 9, True, 10)[1] == T.SHORT        # the cut comes first
    assert head("x", 4000, True, 0)[1] == 0                     # min_chars 0: no filter


BAD = [b"\x80", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xe2\x80",
       b"\xf0\x9f\x98", b"\xff", b"\xe2\x28\xa1"]


@pytest.mark.parametrize("norm", [True, False])
def test_malformed_bytes_before_and_behind_the_stop_point(norm):
    for bad in BAD:
        assert T.model_head(b"abc" + bad, 3, norm) == (b"abc", 0), bad                  # just behind: never examined
        assert T.model_head(b"ab" + bad + b"c", 3, norm) == (b"", T.NEEDS_HOST), bad   # just before
        assert T.model_head(bad, 1, norm) == (b"", T.NEEDS_HOST)
        assert T.model_head(b"abc" + bad, 4, norm) == (b"", T.NEEDS_HOST), bad
        assert T.model_head(b"abc" + bad, 0, norm) == (b"", 0)
    # the non-space behind a pending space is decoded to know that the space is due
    assert T.model_head(b"abc \xff", 4, True) == (b"", T.NEEDS_HOST)
    assert T.model_head(b"abc x\xff", 4, True) == (b"abc ", 0)
    assert T.model_head(b"abc \xff", 4, False) == (b"abc ", 0)
    # the same notion of malformed as model_clean_bytes
    for bad in BAD:
        assert T.model_clean_bytes(b"abc" + bad, spam=False)[1] == T.NEEDS_HOST
    # length is never a reason
    long = ("word " * 40000).encode()
    assert len(long) > T.WINDOW_BYTES and T.model_head(long, 4000, True, 10) == (embed.normalize_text(long.decode()).encode(), 0)
