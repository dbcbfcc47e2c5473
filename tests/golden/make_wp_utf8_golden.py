"""Regenerates tests/golden/wp_utf8.json: `transformers.BertTokenizer` (the slow, pure-Python one, lower-casing) on a small
mixed-script vocabulary (tests/wp_utf8_texts.py: accent-stripped Latin, Greek, Cyrillic, Hebrew, Arabic, Devanagari, CJK,
kana, Hangul jamo, emoji, mathematical alphanumerics) over texts chosen for the per-code-point rules of
review-recommender_amd/wp_unicode.py.

    python tests/golden/make_wp_utf8_golden.py

Stored: the vocabulary (id = position), the texts, the ids at max_length 32 and 512, and "ids_from": "transformers" when
BertTokenizer wrote them (it is then also compared with the host tokenizer, id for id) or "host" when `transformers` is
not installed and review-recommender_amd/wordpiece.py did.  The file holds data only.
"""
import json
import pathlib
import sys
import tempfile

OUT = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent.parent))
sys.path.insert(0, str(OUT.parent))

import wp_utf8_texts as X  # noqa: E402


def main():
    from review_recommender_amd.wordpiece import WordPieceTokenizer
    vocab, texts = X.vocabulary(), X.fixture_texts()
    host = WordPieceTokenizer({w: i for i, w in enumerate(vocab)})
    try:
        from transformers import BertTokenizer
    except ImportError:
        BertTokenizer = None
    out = {"ids_from": "transformers" if BertTokenizer else "host", "vocab": vocab, "texts": texts}
    with tempfile.TemporaryDirectory() as d:
        vf = pathlib.Path(d) / "vocab.txt"
        vf.write_text("\n".join(vocab) + "\n", encoding="utf-8")
        tok = BertTokenizer(str(vf), do_lower_case=True) if BertTokenizer else None
        for L in (32, 512):
            rows = []
            for i, t in enumerate(texts):
                ids = host.encode_pair(t, None, L)[0].tolist()
                if tok is not None:
                    theirs = tok(t, truncation=True, max_length=L)["input_ids"]
                    assert theirs == ids, (i, t.encode("unicode_escape")[:80], theirs[:16], ids[:16])
                    ids = theirs
                rows.append(ids)
            out[f"ids_max{L}"] = rows
    unk = sum(r.count(host.unk_id) for r in out["ids_max512"])
    (OUT / "wp_utf8.json").write_text(json.dumps(out, ensure_ascii=True, separators=(",", ":")))
    print(out["ids_from"], len(vocab), "pieces,", len(texts), "texts,", unk, "[UNK],", (OUT / "wp_utf8.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
