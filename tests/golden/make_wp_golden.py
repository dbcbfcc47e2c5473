"""Regenerates tests/golden/wp_ascii.json: `transformers.BertTokenizer` (the slow, pure-Python one, lower-casing) on a
synthetic vocabulary of a few thousand pieces over ASCII texts chosen for the edges of csrc/rr_wordpiece.hip.

    python tests/golden/make_wp_golden.py

Stored: the vocabulary (id = position), and per case the text, its max_length and the ids transformers returned.  The file
holds data only; tests/test_gpu_wordpiece.py compares the device tokenizer with it id for id.
"""
import json
import pathlib
import random
import string
import sys
import tempfile

OUT = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent.parent))

from review_recommender_amd import synth  # noqa: E402

PUNCT = [chr(c) for c in range(33, 127) if not chr(c).isalnum()]
DELETED = [0x00, 0x01, 0x08, 0x0B, 0x0C, 0x0E, 0x1F, 0x7F]


def make_vocab(rng):
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    singles = list(string.ascii_lowercase + string.digits)
    words += singles + ["##" + c for c in singles if c not in "qz"]        # (no ##q / ##z: some tails cannot match)
    words += [p for p in PUNCT if p not in "~`"]                               # two punctuation bytes are not pieces
    seen = set(words)
    syll = ["".join(rng.choice("bcdfghklmnprstvw") + rng.choice("aeiou") for _ in range(rng.randint(1, 3))) for _ in range(4000)]
    for s in list(synth.WORDS) + syll:
        for form in (s, "##" + s):
            if form not in seen and rng.random() < 0.75:
                seen.add(form)
                words.append(form)
    words += ["Upper", "##Case", "café", "中", "x" * 100, "##" + "y" * 99, "w" * 101]    # never matchable / at the length limit
    return words


def main():
    from transformers import BertTokenizer
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    rng = random.Random(20260)
    vocab = make_vocab(rng)
    plain = [w for w in vocab[5:] if not w.startswith("##") and w.isascii() and w.isalnum() and w.islower() and len(w) > 1]
    cont = [w[2:] for w in vocab if w.startswith("##") and w.isascii() and w[2:].isalnum() and w[2:].islower()]

    def word():
        w = rng.choice(plain) + "".join(rng.choice(cont) for _ in range(rng.choice([0, 0, 1, 2])))
        r = rng.random()
        if r < 0.15:
            w = w.upper() if r < 0.05 else w.capitalize()
        elif r < 0.22:
            i = rng.randrange(len(w) + 1)
            w = w[:i] + chr(rng.choice(DELETED)) + w[i:]                  # a deleted byte inside the word: the halves join
        elif r < 0.27:
            w += rng.choice("qz") * rng.randint(1, 2)                     # a tail without a match: one [UNK]
        return w

    def sentence(n_words):
        out = []
        for _ in range(n_words):
            out.append(word())
            r = rng.random()
            out.append(rng.choice(PUNCT) if r < 0.12 else rng.choice([" ", " ", " ", "  ", "\t", "\n", "\r\n"]) if r < 0.9 else
                       rng.choice(PUNCT) + " ")
        return "".join(out)

    cases = []
    add = lambda text, L=512: cases.append((text, L))
    add("".join(PUNCT))
    add(" ".join(PUNCT))
    add("a" + "".join(PUNCT) + "b")
    for p in PUNCT:
        add(f"ba{p}ko {p}{p} x{p}")
    for d in DELETED:
        add("so" + chr(d) + "ft co" + chr(d) + chr(d) + "tton" + chr(d) + " " + chr(d) + " end")
    add("".join(chr(c) for c in range(128) if c not in (91, 93)))                 # every byte once (brackets below)
    add("[ ] [x] ]a[")
    add("x" * 100); add("x" * 101); add("y" + "y" * 99); add("yy" + "y" * 99); add("w" * 101); add("w" * 100 + " ok")
    add("ab" + "x" * 98); add("ab" + "x" * 99)
    add("Upper Case upper case UPPERCASE")
    add("sofq"); add("qsoft"); add("soft" + "z"); add("zq qz q z")
    add(""); add(" "); add("   \t\n\r  "); add("\x00\x01\x7f"); add(" \x00 ")
    add("a"); add("A"); add("0"); add("a.b,c")
    for L in (8, 32, 512):
        for k in (L - 3, L - 2, L - 1, L):
            add(" ".join(rng.choice(plain[:200]) for _ in range(k)), L)          # k whole-piece words = k pieces
    for _ in range(6):
        t = sentence(900)
        add(t[:4000])
    add(("soft" * 1000)[:4000]); add(". " * 2000); add("a " * 2000)
    for L in (8, 32, 512):
        for _ in range(40 if L < 512 else 60):
            add(sentence(rng.randint(1, 60)), L)

    with tempfile.TemporaryDirectory() as d:
        vf = pathlib.Path(d) / "vocab.txt"
        vf.write_text("\n".join(vocab) + "\n", encoding="utf-8")
        tok = BertTokenizer(str(vf), do_lower_case=True)
        host = WordPieceTokenizer.from_vocab_file(vf)
        # (the L-3 .. L candidates above are made of whole vocabulary pieces, one piece per word: the assert below checks
        # that documents of exactly L-3, L-2 and L-1 pieces are there)
        fixed = list(cases)
        counts = {}
        for i, (text, L) in enumerate(fixed):
            assert text.isascii(), (i, text[:60])
            ids = tok(text, truncation=True, max_length=L)["input_ids"]
            assert ids == host.encode_pair(text, None, L)[0].tolist(), (i, text[:60])
            counts[i] = len(tok.tokenize(text))
            fixed[i] = {"text": text, "max_length": L, "ids": ids}
        for L in (8, 32, 512):
            have = {counts[i] for i, c in enumerate(fixed) if c["max_length"] == L}
            assert {L - 3, L - 2, L - 1} <= have, (L, sorted(have)[:10])
    (OUT / "wp_ascii.json").write_text(json.dumps({"vocab": vocab, "cases": fixed}, ensure_ascii=True, separators=(",", ":")))
    print(len(vocab), "pieces,", len(fixed), "cases,", (OUT / "wp_ascii.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
