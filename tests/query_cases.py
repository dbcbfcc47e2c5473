"""Queries shared by the query front's tests (test_query_model.py on the CPU, test_gpu_query_text.py and
test_gpu_query_engine.py on the GPU)."""
import random

from review_recommender_amd import text

KELVIN, DOTTED_I = "K", "İ"

# every colour word inside a longer word: a substring raises the group, a token would not
COLOR_INSIDE = ["x" + w + "y" for g in text.COLORS.values() for w in sorted(g)]

CRAFTED = COLOR_INSIDE + [
    "credit card", "standard", "prose poem",                 # red through "red", brown through "tan", pink through "rose"
    "black",                                                 # the colour group {black} and the keyword {black}: one group
    "black BLACK Black",
    "sock", "socks", "sock socks",                           # only the key raises the synonym group
    "noise", "noise cancelling headphones", "anc",           # the multi-word terms; "anc" is a term, not a key
    "wireless cat dog keyboard design headphone sock noise",             # 8 synonym groups, cut at 6
    "golden red navy emerald wireless kitten puppy",                     # 4 colours + more, cut at 6
    "yellow red blue green black white pink purple orange brown gray",   # 11 colours, cut at 6
    "cat cat cat kitten kitten", "wireless wireless mouse mouse",        # repeated tokens
    "the and of", "a an the and or of for to in on with is are it this that", "",     # stop words only, empty
    "   ", "?!", "the",
    "a'b'c", "''", "'lead", "trail'", "a''b", "a'b'c'd'e", "don't won't it's", "'", "x'", "'x", "rock'n'roll",
    "x", "a b c 7", "q",                                     # one-byte tokens stay
    "pin" + KELVIN + " sock", "pin" + KELVIN, KELVIN + "itty cat", "blac" + KELVIN,      # U+212A lower-cases to k
    "soc" + DOTTED_I + "x", DOTTED_I + "t", "p" + DOTTED_I + "nk",                      # U+0130: i, then a separator
    "猫 wireless 犬", "café réd", "红red色",                   # CJK, Latin-1
    "cat\0dog", "\0", "red\0\0blue",                         # NUL separates
    "t" * 64, "t" * 65, "a " + "u" * 64 + " cat", "red " + "v" * 65 + " cat", "w" * 40 + "'" + "w" * 23, "w" * 40 + "'" + "w" * 24,
    ("cat dog " * 128)[:1024], ("cat dog " * 129)[:1025], "z" * 1024, " " * 1025,
    "Wireless Bluetooth HEADPHONES for my kitten", "mustard-yellow socks, size 9!", "USB-C cable 2m",
    "pinky promise", "tanned leather", "maroon5", "grey/gray", "prints and patterns",
]
assert len(("cat dog " * 128)[:1024].encode()) == 1024


def random_ascii_queries(n: int = 2000, seed: int = 11, max_bytes: int = 200, max_word: int = 20):
    """Seeded ASCII queries of at most ``max_bytes`` bytes whose runs of letters have at most ``max_word`` bytes: words from
    text.py's lists, random words, punctuation, apostrophes, upper case."""
    rng = random.Random(seed)
    words = sorted({w for g in list(text.COLORS.values()) + list(text.SYNONYMS.values()) for w in g}
                   | set(text.SYNONYMS) | set(text.QUERY_STOP_WORDS))
    seps = [" ", " ", " ", "  ", ", ", "-", "'", "''", ".", "/", " '", "' ", "\t"]
    out = []
    for _ in range(n):
        parts = []
        for _ in range(rng.randint(0, 12)):
            r = rng.random()
            if r < 0.5:
                w = rng.choice(words)
            else:
                w = "".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(rng.randint(1, max_word)))
            if rng.random() < 0.2:
                w = w.upper() if rng.random() < 0.5 else w.capitalize()
            parts.append(w[:max_word])
            parts.append(rng.choice(seps))
        out.append("".join(parts)[:max_bytes])
    return out


def corpus_vocab(extra=()):
    """A small BM25 vocabulary: text.py's words, some of the crafted queries' tokens, and entries no query token can equal."""
    words = sorted({w for g in list(text.COLORS.values()) + list(text.SYNONYMS.values()) for w in g if " " not in w and "-" not in w})
    words += ["don't", "a'b", "c", "x", "7", "pink", "socki", "t" * 64, "t" * 65, "café", "Upper", "two words", "mouse",
              "card", "usb", "2m", "rock'n", "roll"]
    words += list(extra)
    vocab = {}
    for w in words:
        vocab.setdefault(w, len(vocab))
    return vocab
