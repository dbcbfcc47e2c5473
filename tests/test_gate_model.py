"""The CPU statement of the gate kernels (gate.model_gate_plane, gate.model_gate_hits, gate.pack_groups) against Python's
own `s in text[:6000].lower()` and `text.calculate_gate_factor`: for every code point, at the cut, on the reference-run
fixtures and on seeded random texts.  tests/test_gpu_gate.py then holds the kernels to the model bitwise."""
import json
import pathlib
import re

import numpy as np
import pytest

from conftest import GOLDEN
from review_recommender_amd import gate as G
from review_recommender_amd import text as T

_ASCII_RUNS_B = re.compile(rb"[\x00-\x7f]+")
_ASCII_RUNS_S = re.compile("[\x00-\x7f]+")


def runs_of_image(image: bytes):
    return _ASCII_RUNS_B.findall(image)


def runs_of_lower(s: str):
    return [r.encode("ascii") for r in _ASCII_RUNS_S.findall(s.lower())]


def factor_of(text, groups, penalty):
    """The gate factor through the model and the factor table: (Python float, float32)."""
    hits = G.model_gate_hits(G.model_gate_plane(text), [sorted(g) for g in groups])
    missed = len(groups) - bin(hits).count("1")
    return G.factor_table(penalty, np.float64)[missed], G.factor_table(penalty)[missed], hits


# ------------------------------------------------------------------------------------------------ all of Unicode
def test_every_code_point_keeps_the_ascii_runs_of_lower():
    """An ASCII string occurs in s.lower() exactly when it occurs in one of its maximal ASCII runs, so equal runs are the
    "every ASCII pattern" property.  Every code point alone, between lower-case and between upper-case neighbours."""
    folds = {}
    for c in range(0x110000):
        ch = chr(c)
        for s in (ch, "ab" + ch + "cd", "AB" + ch + "CD"):
            if runs_of_image(G.model_gate_plane(s)) != runs_of_lower(s):
                pytest.fail(f"U+{c:04X} in {s!r}: image {G.model_gate_plane(s)!r}, lower() {s.lower()!r}")
        if c >= 0x80 and any(ord(x) < 0x80 for x in ch.lower()):
            folds[c] = ch.lower()
    # the list csrc/rr_gate.hip, include/rr_hip.h and gate.py name; a later Python that disagrees fails here
    assert folds == {0x130: "i\u0307", 0x212A: "k"} == G.FOLDS_TO_ASCII
    src = (pathlib.Path(G.__file__).parent / "csrc" / "rr_gate.hip").read_text()
    assert "C4 B0    (U+0130)   -> 69 B0" in src and "E2 84 AA (U+212A)   -> 6B" in src
    assert G.model_gate_plane("\u0130") == b"i\xb0" and G.model_gate_plane("a\u212ab") == b"akb"


# ------------------------------------------------------------------------------------------------ the cut
@pytest.mark.parametrize("wide", ["x", "é", "€", "\U0001f600"], ids=["1-byte", "2-byte", "3-byte", "4-byte"])
@pytest.mark.parametrize("n", [5999, 6000, 6001])
def test_the_cut_counts_code_points(wide, n):
    assert len(wide.encode()) == {"x": 1, "é": 2, "€": 3, "\U0001f600": 4}[wide]
    # a term that ends exactly at character n, behind n - 4 wide characters
    s = wide * (n - 4) + "RED!" + wide * 50
    image = G.model_gate_plane(s)
    assert image == s[:6000].lower().encode("utf-8")
    assert (b"red!" in image) == ("red!" in s[:6000].lower()) == (n <= 6000)
    assert runs_of_image(image) == runs_of_lower(s[:6000])
    # the two folding code points as the last character kept and as the first one dropped
    for ch, low in (("\u212a", b"k"), ("\u0130", b"i\xb0")):
        s = wide * (n - 1) + ch + "z"
        image = G.model_gate_plane(s)
        assert runs_of_image(image) == runs_of_lower(s[:6000])
        assert image.endswith(low + b"z") == (n < 6000) and image.endswith(low) == (n == 6000)
    assert G.model_gate_plane(wide * 7, max_chars=0) == b"" and G.model_gate_plane("", max_chars=5) == b""
    assert G.model_gate_plane("\ud800A".encode("utf-8", "surrogatepass")) == b"\xed\xa0\x80a"      # a lone surrogate


# ------------------------------------------------------------------------------------------------ reference-run cases
def test_reference_run_gate_factors_through_the_model():
    cases = json.loads((GOLDEN / "cli_helpers.json").read_text())["gate_factor"]
    assert len(cases) >= 60
    for c in cases:
        groups = T.build_gate_groups(c["q"])
        f64, f32, _ = factor_of(c["text"], groups, c["penalty"])
        assert f64 == c["y"] and f32 == np.float32(c["y"]), c
        assert f32.tobytes() == np.float32(T.calculate_gate_factor(c["text"][:6000], groups, c["penalty"])[0]).tobytes()


def test_model_equals_calculate_gate_factor_on_random_texts():
    rng = np.random.default_rng(20251019)
    words = ["black", "ink", "kit", "red", "bored", "noise cancelling", "noise-canceling", "anc", "k", "i", "socks", "sock"]
    pieces = words + ["BLAC\u212a", "\u0130NK", "\u212aIT", "\u212a", "\u0130", " ", "  ", "-", "é", "€", "RED", "Bored",
                      "blac", "in", "\U0001f600", "NOISE", "Cancelling", "x" * 40]
    n_hit = n_miss = 0
    for _ in range(400):
        text = "".join(rng.choice(pieces, size=int(rng.integers(0, 40))))
        if rng.random() < 0.1:
            text = "é" * int(rng.integers(5900, 6001)) + text
        groups = [set(rng.choice(words, size=int(rng.integers(1, 4)))) for _ in range(int(rng.integers(0, 7)))]
        penalty = float(rng.choice([0.0, 0.3, 0.5, 0.7, 1.0]))
        want, matched, total = T.calculate_gate_factor(text[:6000], groups, penalty)
        f64, f32, hits = factor_of(text, groups, penalty)
        assert f64 == want and f32 == np.float32(want) and bin(hits).count("1") == matched, (text, groups)
        n_hit += matched
        n_miss += total - matched
    assert n_hit > 100 and n_miss > 100
    # U+0130 and U+212A inside and next to terms, spelled out
    for text, term, want in [("BLAC\u212a", "black", True), ("blac\u212a ink", "k i", True), ("\u0130nk", "ink", False),
                             ("\u0130nk", "i", True), ("\u0130nk", "nk", True), ("x\u0130", "xi", True), ("a\u212a\u212ab", "akkb", True),
                             ("\u212a", "k", True), ("K", "k", True), ("\u0131", "i", False), ("\u017f", "s", False)]:
        assert (term in text.lower()) == want == bool(G.model_gate_hits(G.model_gate_plane(text), [[term]])), (text, term)


# ------------------------------------------------------------------------------------------------ pack_groups
def test_pack_groups_layout_factors_and_limits():
    six = T.build_gate_groups("yellow red blue green black white pink")           # the cap of six groups
    assert len(six) == 6
    seven_terms = [T.SYNONYMS["headphone"]]
    assert len(seven_terms[0]) == 7
    multi = [T.SYNONYMS["noise"]]
    assert {"noise cancelling", "noise-canceling"} <= multi[0]
    batch = [six, seven_terms, multi, [], [{"a" * G.MAX_TERM_BYTES}], [{"a" * (G.MAX_TERM_BYTES + 1)}], [{"café"}],
             [{"t"}] * 7]
    pens = [0.0, 0.3, 0.5, 1.0, 0.5, 0.5, 0.5, 0.5]
    p = G.pack_groups(batch, pens)
    assert p.host_queries == [5, 6, 7] and p.n_queries == 8 and p.any_groups
    assert p.q_groups.tolist() == [6, 1, 1, 0, 1, 0, 0, 0]
    assert p.term_off.dtype == p.term_group.dtype == p.q_term.dtype == p.q_groups.dtype == np.int32
    assert p.factor.dtype == np.float32 and p.factor.shape == (8, 7)
    blob = p.term_bytes.tobytes()
    for q, groups in enumerate(batch):
        a, b = int(p.q_term[q]), int(p.q_term[q + 1])
        got = [(int(p.term_group[t]), blob[p.term_off[t]:p.term_off[t + 1]].decode()) for t in range(a, b)]
        want = [] if q in p.host_queries else [(g, t) for g, grp in enumerate(groups) for t in sorted(grp)]
        assert got == want
        f = 1.0
        for m in range(7):                          # the reference's loop: a Python float, cast once
            assert p.factor[q, m].tobytes() == np.float32(f).tobytes()
            f *= pens[q]
    assert p.factor[0].tolist() == [1.0, 0, 0, 0, 0, 0, 0] and p.factor[3].tolist() == [1.0] * 7
    one = G.pack_groups([six], 0.5)                 # a scalar penalty
    assert one.factor[0].tolist() == [0.5 ** m for m in range(7)] and one.host_queries == []
    none = G.pack_groups([[], []], 0.5)
    assert not none.any_groups and none.term_bytes.size == 0 and none.term_off.tolist() == [0]
    buf, where = p.buffer()
    assert all(o % 16 == 0 for o in where.values()) and buf.dtype == np.uint8
    assert buf[where["factor"]:where["factor"] + p.factor.nbytes].view(np.float32).reshape(8, 7).tobytes() == p.factor.tobytes()
    with pytest.raises(ValueError, match="length zero"):
        G.pack_groups([[{"red", ""}]], 0.5)
    with pytest.raises(ValueError):
        G.pack_groups([six], [0.5, 0.5])
    too_many = [{"t%d" % i for i in range(G.MAX_TERMS + 1)}]
    too_long = [{chr(97 + i % 26) * 60 + str(i) for i in range(17)}]
    assert sum(len(t) for t in too_long[0]) > G.QUERY_TERM_BYTES
    assert G.pack_groups([too_many, too_long], 0.5).host_queries == [0, 1]
    with pytest.raises(ValueError, match="not ASCII"):
        G.model_gate_hits(b"cafe", [["café"]])
