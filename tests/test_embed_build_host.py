"""Host side of the GPU embedding builder (review-recommender_amd/embed.py): the reference's text normalisation and product
filter (nlp/11_build_product_embeddings.py:22-36, 58-62, 86-89) on literal cases, and the piece table the device tokenizer
matches against, walked in numpy."""
import numpy as np
import pandas as pd
import pytest

from review_recommender_amd import embed
from review_recommender_amd.vocabtable import table_lookup


def test_normalize_text_literal_cases():
    n = embed.normalize_text
    assert embed.MIN_TEXT_LEN == 10 and embed.MAX_TEXT_LEN == 4000
    assert n("a\r\nb\tc") == "a b c"                       # \r and \n become blanks, the run (and the tab) collapses
    assert n("a   b \t\t c") == "a b c"
    assert n("  lead and trail \n") == "lead and trail"
    assert len(n("x" * 4001)) == 4000 and n("x" * 4001) == "x" * 4000
    assert n("ab " * 2000) == ("ab " * 2000)[:4000]         # cut AFTER collapsing, so a trailing blank may stay
    assert n(None) == ""
    assert n(12.5) == "12.5" and n(7) == "7"
    assert n("a\u00a0\u00a0b") == "a b"                 # U+00A0: Python's \s matches it on str
    assert n("\u00a0a b\u00a0") == "a b"                # ... and strip() takes it off the ends as well
    assert n("") == ""


def test_product_filter_keeps_order_raw_text_and_nan_columns():
    df = pd.DataFrame({"sku": ["a", "b", "c", "d", "e"],
                       "agg_text": ["  long enough text\r\nhere ", "short", None, "123456789", "exactly 10"],
                       "n_reviews": [3, 4, 5, 6, 7]}, index=[10, 11, 12, 13, 14])
    meta, texts = embed.filter_products(df)
    assert list(meta.columns) == ["sku", "n_reviews", "avg_stars", "last_ts", "agg_text"]
    assert meta["sku"].tolist() == ["a", "e"] and meta["n_reviews"].tolist() == [3, 7]
    assert meta["agg_text"].tolist() == ["  long enough text\r\nhere ", "exactly 10"]       # the RAW column
    assert texts == ["long enough text here", "exactly 10"]
    assert meta["avg_stars"].isna().all() and meta["last_ts"].isna().all()
    assert list(meta.index) == [0, 1]
    other = df.rename(columns={"agg_text": "body"})
    meta2, texts2 = embed.filter_products(other, "body")
    assert texts2 == texts and meta2["agg_text"].tolist() == meta["agg_text"].tolist()
    with pytest.raises(RuntimeError, match="No products left"):
        embed.filter_products(pd.DataFrame({"sku": ["a", "b"], "agg_text": ["tiny", None]}))
    with pytest.raises(ValueError):
        embed.filter_products(pd.DataFrame({"agg_text": ["no sku column here"]}))


def walk(slots: np.ndarray, blob: np.ndarray, piece: str):
    """The id the table holds for `piece` (its ## form included), or None: the probe sequence the kernel follows."""
    form = 1 if piece.startswith("##") and len(piece) > 2 else 0
    body = piece[2:].encode() if form else piece.encode()
    pid = table_lookup(slots, blob, body, len(body) | (form << 16))
    return None if pid < 0 else pid


def test_piece_table_finds_every_piece_and_no_absent_string(hip):
    rng = np.random.default_rng(5)
    letters = "abcdefghijklmnopqrstuvwxyz0123456789"
    pieces = {"[PAD]": 0, "[UNK]": 1, "[CLS]": 2, "[SEP]": 3}
    while len(pieces) < 6000:
        w = "".join(rng.choice(list(letters), size=rng.integers(1, 9)))
        pieces.setdefault(w if rng.random() < 0.6 else "##" + w, len(pieces))
    pieces["café"] = len(pieces)                           # non-ASCII: found under its id
    pieces["x" * 101] = len(pieces)                        # longer than max_chars_per_word: left out
    pieces["##" + "y" * 100] = len(pieces)                 # 100 characters after the ##: kept
    pieces["!"] = len(pieces) + 3                          # a gap in the ids: the missing ones are empty pieces
    slots, blob, kept = embed.build_piece_table(pieces)
    assert len(slots) & (len(slots) - 1) == 0 and len(slots) >= 2 * kept
    assert kept == len(pieces) - 1
    assert int((slots[:, 3] >= 0).sum()) == kept
    for p, i in pieces.items():
        want = None if p == "x" * 101 else i
        assert walk(slots, blob, p) == want, p
    absent = 0
    for _ in range(3000):
        w = "".join(rng.choice(list(letters), size=rng.integers(1, 9)))
        for cand in (w, "##" + w):
            if cand not in pieces:
                absent += 1
                assert walk(slots, blob, cand) is None, cand
    assert absent > 3000
    # the ## form and the plain form of the same letters are different pieces
    two = {"[UNK]": 0, "[CLS]": 1, "[SEP]": 2, "ab": 3, "##ab": 4}
    slots, blob, kept = embed.build_piece_table(two)
    assert walk(slots, blob, "ab") == 3 and walk(slots, blob, "##ab") == 4 and walk(slots, blob, "##a") is None


def test_chunks_never_exceed_the_token_budget():
    lens = [0, 5, 4000, 4000, 10, 300, 2, 2, 4000]
    chunks = embed._plan_chunks(lens, 512, 1024)
    assert chunks[0][0] == 0 and chunks[-1][1] == len(lens)
    assert all(a < b for a, b in chunks) and all(chunks[i][1] == chunks[i + 1][0] for i in range(len(chunks) - 1))
    for a, b in chunks:
        assert b - a == 1 or sum(min(512, l + 2) for l in lens[a:b]) <= 1024
    assert embed._plan_chunks([], 512, 1024) == []
