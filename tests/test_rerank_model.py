"""The CPU statement of the reranker's token plane and pair assembly (rerank.model_plane / model_pairs / pack_queries)
against `WordPieceTokenizer.encode_pair`, which is what the host path runs; and the new ABI calls, header against ctypes."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

from review_recommender_amd import rerank as R
from review_recommender_amd.wordpiece import WordPieceTokenizer

ROOT = pathlib.Path(__file__).resolve().parent.parent
LENGTHS = (3, 4, 8, 9, 16, 17)


def word_tokenizer(n_words=64):
    """Single-piece words: n words give n tokens.  qN are query words, tN text words (so a swapped side shows)."""
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + [f"q{i}" for i in range(n_words)] + [f"t{i}" for i in range(n_words)]
    words += ["ab", "abcd", "ee", "eeee", "eb", "ea", "eabc"]
    return WordPieceTokenizer({w: i for i, w in enumerate(words)})


def side(prefix, n):
    return " ".join(f"{prefix}{i % 64}" for i in range(n))


@pytest.mark.parametrize("L", LENGTHS)
def test_model_pairs_over_model_plane_equals_encode_pair(L):
    tok = word_tokenizer()
    avail = L - 3
    texts = [side("t", n_b) for n_b in range(3 * avail + 3)]
    plane = R.model_plane(texts, tok, L)
    assert [len(p) for p in plane] == [min(n_b, avail) for n_b in range(len(texts))]
    n = len(texts)
    rows = np.arange(n, dtype=np.int64)[None, :]
    differ = 0
    for n_a in range(2 * avail + 3):
        q = side("q", n_a)
        q_ids = tok.text_ids(q)
        assert len(q_ids) == n_a
        got_tok, got_typ, got_pos, cu = R.model_pairs(plane, rows, n, n, [q_ids], L, tok.cls_id, tok.sep_id, 0, n)
        assert cu[0] == 0 and len(cu) == n + 1
        for j, text in enumerate(texts):
            want_ids, want_typ = tok.encode_pair(q, text, L)
            a, b = cu[j], cu[j + 1]
            same = (np.array_equal(got_tok[a:b], want_ids) and np.array_equal(got_typ[a:b], want_typ))
            if n_a <= avail:
                assert same, (L, n_a, j, got_tok[a:b], want_ids)
                assert np.array_equal(got_pos[a:b], np.arange(b - a)) and b - a <= max(L, 3)
            else:
                differ += not same
    if avail % 2:             # why a query of more than avail tokens is the host's: the plane's cap shows there (both sides
        assert differ > 0     # cut to halves, and the odd token goes to whichever side is longer AFTER the cap)


def test_keep_lengths_is_encode_pairs_rule():
    tok = word_tokenizer()
    for L in LENGTHS:
        for n_a in range(0, 2 * L):
            for n_b in range(0, 2 * L):
                ids, typ = tok.encode_pair(side("q", n_a), side("t", n_b), L)
                ka, kb = R.keep_lengths(n_a, n_b, L)
                assert (ka + 2, kb + 1) == (int((typ == 0).sum()), int((typ == 1).sum())), (L, n_a, n_b)


def test_pack_queries_lists_exactly_the_long_queries():
    for L in LENGTHS:
        avail = L - 3
        lists = [list(range(5, 5 + n)) for n in (0, 1, avail, avail + 1, 2 * avail + 2, max(avail - 1, 0))]
        p = R.pack_queries(lists, L)
        assert p.host_queries == [q for q, ids in enumerate(lists) if len(ids) > avail] and p.n_queries == len(lists)
        assert p.off.dtype == np.int32 and p.ids.dtype == np.int32 and p.off[0] == 0 and p.off[-1] == len(p.ids)
        for q, ids in enumerate(lists):
            got = p.ids[p.off[q]:p.off[q + 1]].tolist()
            assert got == ([] if q in p.host_queries else ids)
        buf, at = p.buffer()
        assert buf.dtype == np.int32 and at == len(lists) + 1 and len(buf) >= at + 1
        assert buf[:at].tolist() == p.off.tolist() and buf[at:at + len(p.ids)].tolist() == p.ids.tolist()


def test_model_plane_cuts_at_2000_code_points_before_tokenising():
    tok = word_tokenizer()
    v = tok.vocab
    L = 4096
    head = "ab " * 666                                              # 1998 characters
    cases = {
        head + "abcd": [v["ab"]] * 666 + [v["ab"]],                 # the 2000th character splits a word: the half is tokenised
        head + "éééé": [v["ab"]] * 666 + [v["ee"]],                 # ... splits a run of two-byte characters: code points, not bytes
        "éb " * 666 + "éabc": [v["eb"]] * 666 + [v["ea"]],         # NFD lengthens every word: the cut counts the ORIGINAL characters
        "éb " * 500 + "eabc": [v["eb"]] * 500,                # decomposed: 4 characters a word, the cut falls on the blank
        "": [], "   \n\t ": [],
    }
    plane = R.model_plane(list(cases), tok, L)
    for (text, want), got in zip(cases.items(), plane):
        assert got.dtype == np.uint16 and got.tolist() == want, (text[:20], len(got), len(want))
    assert [p.tolist() for p in R.model_plane(list(cases), tok, 10)] == [w[:7] for w in cases.values()]
    assert R.model_plane(["ab abcd"], tok, 512, max_chars=4)[0].tolist() == [v["ab"], v["[UNK]"]]    # "ab a"


def test_header_and_ctypes_agree_on_the_pair_calls():
    from review_recommender_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rr_hip.h").read_text(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(rr_pairs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header))
    assert set(decls) == {"rr_pairs_create", "rr_pairs_destroy", "rr_pairs_measure_dev", "rr_pairs_write_dev", "rr_pairs_status"}
    assert set(decls) == {n for n in _lib.PROTOTYPES if n.startswith("rr_pairs_")}

    def kind(arg):
        arg = " ".join(arg.split())
        if "*" in arg:
            return "ptr"
        return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}[arg.split()[0]]

    for name, args in decls.items():
        res, argtypes = _lib.PROTOTYPES[name]
        want = [kind(a) for a in args.split(",")]
        got = ["ptr" if t is ctypes.c_void_p or hasattr(t, "contents") else t for t in argtypes]
        assert res is ctypes.c_int and got == want, name
    assert "rr_pairs.hip" in __import__("review_recommender_amd.build", fromlist=["SOURCES"]).SOURCES


def test_rerank_device_refuses_what_it_cannot_serve():
    """The engine's keyword, as far as it goes without a GPU: anything but this package's CrossEncoder keeps the host path."""
    import pandas as pd
    from review_recommender_amd.engine import SearchEngine
    meta = pd.DataFrame({"sku": ["a", "b"], "agg_text": ["x", "y"]})
    emb = np.eye(2, 8, dtype=np.float32)

    class Fake:
        def predict(self, pairs, **kw):
            return np.zeros(len(pairs), dtype=np.float32)

    with pytest.raises(ValueError, match="CrossEncoder with a tokenizer"):
        SearchEngine(meta, emb, cross_encoder=Fake(), rerank="device")
    with pytest.raises(ValueError, match="CrossEncoder with a tokenizer"):
        SearchEngine(meta, emb, cross_encoder=None, rerank="device")
    with pytest.raises(ValueError, match="rerank must be"):
        SearchEngine(meta, emb, rerank="gpu")
    big = WordPieceTokenizer({**{f"w{i}": i for i in range(1 << 16)}, "[UNK]": 1 << 16, "[CLS]": 0, "[SEP]": 1})
    with pytest.raises(ValueError, match="uint16"):
        R.RerankText.from_texts(["x"], big, 512)
