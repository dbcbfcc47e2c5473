"""doctok.model_tokenize -- the specification of the device tokenizer of the BM25 corpus (csrc/rr_doctok.hip), written
over bytes without `re` -- against text.tokenize_document (nlp/12_product_prep.py:75-78 with `re` and str.lower()), and
the fact its byte rules rest on: exactly two code points outside ASCII lower-case onto ASCII."""
import json
import pathlib
import random

from review_recommender_amd import doctok, text

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
ALPHABET = list("ab1AZ' .-\n") + ["\u0130", "\u212a", "\u0307", "\u00e9", "\u6f22", "\U0001F600"]


def model(t: str):
    return [b.decode("ascii") for b in doctok.model_tokenize(t.encode("utf-8", "surrogatepass"))]


def test_the_reference_run_cases():
    cases = json.loads((GOLDEN / "index_tokenizer.json").read_text())["cases"]
    assert len(cases) == 27
    for c in cases:
        assert model(c["text"]) == c["tokens"] == text.tokenize_document(c["text"]), c["text"]


def test_the_greedy_apostrophe_rule():
    for s, want in (("a'b'c", ["a'b"]), ("aa'bb'cc", ["aa'bb", "cc"]), ("rock'n'roll", ["rock'n", "roll"]), ("ab''cd", ["ab", "cd"]),
                    ("x'", []), ("'ab", ["ab"]), ("it's", ["it's"]), ("won't", []), ("Won't WON'T wont", ["wont"]),
                    ("a\u212ab", ["akb"]), ("\u212a\u212a", ["kk"]), ("a\u0130b", ["ai"]), ("\u0130'x", []), ("q\u0130'xx", ["qi", "xx"]),
                    ("aa\0bb", ["aa", "bb"]), ("aa'\u212a", ["aa'k"]), ("aa'\u0130b", ["aa'i"])):
        assert text.tokenize_document(s) == want, s
        assert model(s) == want, s


def test_exactly_two_code_points_outside_ascii_lower_case_onto_ascii():
    onto = {c: chr(c).lower() for c in range(0x80, 0x110000) if any(ord(x) < 0x80 for x in chr(c).lower())}
    assert onto == doctok.LOWERS_TO_ASCII == {0x212A: "k", 0x0130: "i\u0307"}
    assert "\u212a".encode() == doctok.KELVIN == b"\xe2\x84\xaa" and "\u0130".encode() == doctok.DOTTED_I == b"\xc4\xb0"
    assert not "\u0307".isalnum() and text.tokenize_document("a\u0307b") == []          # U+0307 separates


def test_every_code_point_in_a_few_contexts():
    """U+0000 .. U+10FFFF, surrogates included, 2048 at a time (joined by spaces: under the 5000-token cap)."""
    contexts = (lambda c: "a" + c + "b", lambda c: c + "'" + c, lambda c: "xx" + c + "'" + c + "yy", lambda c: c,
                lambda c: "zz'" + c + c)
    for lo in range(0, 0x110000, 2048):
        cps = [chr(c) for c in range(lo, lo + 2048)]
        for f in contexts:
            s = " ".join(f(c) for c in cps)
            want = text.tokenize_document(s)
            assert len(want) < text.INDEX_TOKEN_CAP
            assert model(s) == want, (hex(lo), f("?"))


def test_random_strings_over_the_hard_alphabet():
    rng = random.Random(20240607)
    for _ in range(100_000):
        s = "".join(rng.choices(ALPHABET, k=rng.randint(0, 24)))
        assert model(s) == text.tokenize_document(s), repr(s)


def test_the_cap_counts_kept_tokens():
    s = " ".join(["the", "x", "tok%d" % 1] * 6000)
    assert model(s) == text.tokenize_document(s) == ["tok1"] * 5000
    s = " ".join("w%d" % i for i in range(4999)) + " the a last"
    assert model(s)[-1] == "last" and len(model(s)) == 5000 and model(s) == text.tokenize_document(s)


def test_the_stop_words_fit_the_kernel_table():
    """rr_doctok_create packs a stop word into one 64-bit word and holds at most 64 of them."""
    assert len(text.INDEX_STOP_WORDS) == 56
    assert all(1 <= len(w.encode("ascii")) <= 8 for w in text.INDEX_STOP_WORDS)
