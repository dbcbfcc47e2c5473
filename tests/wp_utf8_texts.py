"""Mixed-script vocabulary and random text for the UTF-8 tokenizer tests (test_wp_unicode_model.py, test_gpu_wordpiece_utf8.py,
golden/make_wp_utf8_golden.py).  No test lives here."""
import unicodedata

import numpy as np


def _assigned(lo, hi):
    return [chr(c) for c in range(lo, hi + 1) if unicodedata.category(chr(c)) not in ("Cn", "Co", "Cs")]


SCRIPTS = {
    "accents": list("àáâãäåæçèéêëìíîïñòóôõöøùúûüýÿÀÉÎÕÜŠšŽžŁłĐđßİıŒœǅǆ"),
    "marks": _assigned(0x0300, 0x036F),
    "greek": [c for c in _assigned(0x0370, 0x03FF) if c != "Σ"],
    "cyrillic": _assigned(0x0400, 0x04FF),
    "hebrew": _assigned(0x0591, 0x05F4),
    "arabic": _assigned(0x0600, 0x06FF),
    "devanagari": _assigned(0x0900, 0x097F),
    "hangul": [chr(c) for c in range(0xAC00, 0xD7A4, 37)],
    "jamo": _assigned(0x1100, 0x11FF),
    "kana": _assigned(0x3040, 0x30FF),
    "cjk": ([chr(c) for c in range(0x4E00, 0xA000, 97)] + [chr(c) for c in range(0x3400, 0x4DC0, 211)]
            + [chr(c) for c in range(0x20000, 0x2A6E0, 1999)]),
    "compat": _assigned(0xF900, 0xFAFF)[::7] + _assigned(0x2F800, 0x2FA1D)[::17],
    "emoji": _assigned(0x1F300, 0x1F6FF)[::5] + _assigned(0x2600, 0x27BF)[::5] + _assigned(0x1F900, 0x1F9FF)[::5]
             + ["\u200d", "\ufe0f"],
    "math": _assigned(0x1D400, 0x1D7FF)[::9],
    "controls": [chr(c) for c in list(range(0, 0x20)) + list(range(0x7F, 0xA0))] + ["\u200b", "\ufeff", "\ufffd", "\u00ad"],
    "spaces": [chr(c) for c in range(0x110000) if unicodedata.category(chr(c)) == "Zs"] + ["\u2028", "\u2029", "\t", "\n", "\r"],
    "punct": list("’‘“”«»—–…·¿¡、。「」！？™©®°€£") + list("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"),
}
HARD_SAMPLES = ["Σ", "〮", "᭄", "\U0001d165"]
ASCII_WORDS = ("soft warm mug lamp cable great good bad fits well battery charger the a and is was for with this very small "
               "large usb screen cover phone case love hate return price cheap quality works broke day week").split()


def vocabulary():
    """[PAD] [UNK] [CLS] [SEP] [MASK], ASCII words, letters and ## letters, and pieces in every script of SCRIPTS in their
    MAPPED form (what the tokenizer matches: lower-cased, NFD, Mn stripped)."""
    from review_recommender_amd.wp_unicode import mapped_form
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list(ASCII_WORDS)
    words += ["cafe", "naive", "zoe", "uber", "##fe", "##ive", "##s", "##ing", "##ed", "##er"]
    for c in "abcdefghijklmnopqrstuvwxyz0123456789":
        words += [c, "##" + c]
    words += list("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~")
    for name in ("accents", "greek", "cyrillic", "hebrew", "arabic", "devanagari", "hangul", "jamo", "kana", "math"):
        for ch in SCRIPTS[name][::2]:
            m = mapped_form(ch)
            for x in m:
                words += [x, "##" + x]
            if len(m) > 1:
                words += [m, "##" + m]
    words += ["αβγ", "##δε", "λογος", "привет", "##ет", "мир", "שלום", "سلام", "नम", "##सत", "かな", "##かな", "カタ",
              "ᄒ" + "ᅡ" + "ᆫ", "##" + "ᄀ" + "ᅮ" + "ᆨ"]
    for name in ("cjk", "compat", "emoji", "punct"):
        for ch in SCRIPTS[name][::2]:
            words += list(mapped_form(ch))
    seen, out = set(), []
    for w in words:
        if w and w not in seen:
            seen.add(w)
            out.append(w)
    return out


def random_text(rng, n_chars, density, hard=0.0):
    """About n_chars characters: ASCII words with, at rate `density`, a run from one script, an accented word or a word damaged
    with a mark, a control or punctuation; `hard`: the rate of hard code points (0 = none)."""
    names = [n for n in SCRIPTS if n not in ("spaces", "controls")]
    seps = [" ", " ", " ", "  ", "\n", ", ", ". ", "\u00a0", "\u3000", "\u2009"]
    parts, size = [], 0
    while size < n_chars:
        r = rng.random()
        if r >= density:
            w = ASCII_WORDS[rng.integers(len(ASCII_WORDS))]
            if rng.random() < 0.1:
                w = w.capitalize()
        else:
            kind = rng.random()
            if kind < 0.55:
                pool = SCRIPTS[names[rng.integers(len(names))]]
                w = "".join(pool[i] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 9))))
            elif kind < 0.8:
                w = ASCII_WORDS[rng.integers(len(ASCII_WORDS))]
                k = int(rng.integers(0, len(w) + 1))
                pool = SCRIPTS[("accents", "marks", "controls", "punct", "spaces")[rng.integers(5)]]
                w = w[:k] + pool[rng.integers(len(pool))] + w[k:]
            else:
                w = "".join(SCRIPTS[names[rng.integers(len(names))]][0:1] + [ASCII_WORDS[rng.integers(len(ASCII_WORDS))]]
                            + [SCRIPTS["marks"][rng.integers(len(SCRIPTS["marks"]))]])
            if hard and rng.random() < hard:
                w += HARD_SAMPLES[rng.integers(len(HARD_SAMPLES))]
        s = seps[rng.integers(len(seps))]
        parts += [w, s]
        size += len(w) + len(s)
    return "".join(parts)[:n_chars]


def fixture_texts():
    """The texts of tests/golden/wp_utf8.json (make_wp_utf8_golden.py): every script of the vocabulary, the per-code-point
    rules at their edges, and random mixed text."""
    texts = [
        "Café naïve Zoë Über",                                  # accents stripped
        "café naïve",                                                    # the same, decomposed
        "“great” mug ’s — 5€ ™",                        # curly quotes, dash, currency, TM
        "αβγδε ΑΒΓ λογος άέή",       # Greek, accents
        "привет МИР йё",      # Cyrillic: short i, io lose their marks
        "שׁלום سلام نمست",
        "नमस्ते नम",                          # Devanagari: virama and vowel signs
        "中文mug一丁 㐀 \U00020000x",                           # CJK isolates, also inside a word
        "豈更 﨎 \U0002f800",                                           # compatibility ideographs (mapped)
        "かなかな カタカナ がぱ",            # kana; voiced marks are Mn
        "한국어 한 한",                              # Hangul syllables -> jamo; jamo
        "\U0001f600 \U0001f44d\U0001f3fd mug❤️ \U0001f468‍\U0001f469",   # emoji, VS16, ZWJ
        "\U0001d400\U0001d401 \U0001d7ce ① ½ ﬁ Ⅷ",               # math alphanumerics, no NFKC
        "so­ft co​tton ﻿mug � x\u0085y",                        # deleted inside words
        "a b c　d e f g",                               # every kind of blank
        "İstanbul İ ı ǅ ẞ ß",                         # special lower-casing
        "¿qué? ¡sí! 、。「」！",             # Unicode punctuation
        "x" * 100 + " " + "é" * 100 + " " + "é" * 101 + " " + "中" * 3,
        "", "   ", "́", "́̂ a", "​",
    ]
    rng = np.random.default_rng(77)
    for d in (0.1, 0.3, 0.6, 1.0):
        for n in (40, 200, 900):
            texts.append(random_text(rng, n, d))
    return texts


def mixed_product_texts(n, seed, fraction=0.3):
    """synth.text_corpus with `fraction` of the texts carrying accents, curly quotes, emoji or CJK; a few more hold a hard code
    point (the only documents of this table the UTF-8 kernel leaves to the host)."""
    from review_recommender_amd import synth
    rng = np.random.default_rng(seed)
    texts = synth.text_corpus(n, seed, mean_len=25)
    extras = ["café", "naïve", "“great”", "it’s", "\U0001f600", "❤️", "中文", "Über",
              "5€", "™", "мир"]
    for i in np.flatnonzero(rng.random(n) < fraction):
        words = texts[i].split(" ")
        for _ in range(int(rng.integers(1, 5))):
            words.insert(int(rng.integers(0, len(words) + 1)), extras[rng.integers(len(extras))])
        texts[i] = " ".join(words)
    hard = 20 + rng.choice(n - 20, 5, replace=False)
    for i in hard:
        texts[i] = texts[i] + " ΚΣ " + HARD_SAMPLES[1]
    texts[7] = (texts[7] + " café ") * 40                          # cut at 4 000 characters
    return texts
