"""querytext.model_front -- the CPU statement of what csrc/rr_query.hip computes -- against the host functions it stands in
for (text.tokenize_query, BM25Corpus.term_ids, text.build_gate_groups, gate.pack_groups, rerank.pack_queries), and the
vocabulary table, built by the library on the host, walked on the host.  No GPU."""
import json
import sys

import numpy as np
import pytest

from review_recommender_amd import querytext as Q
from review_recommender_amd import text
from review_recommender_amd.bm25 import BM25Corpus
from review_recommender_amd.gate import pack_groups
from review_recommender_amd.rerank import pack_queries
from review_recommender_amd.wordpiece import WordPieceTokenizer

from conftest import GOLDEN
from query_cases import CRAFTED, COLOR_INSIDE, corpus_vocab, random_ascii_queries


@pytest.fixture(scope="module")
def corpus():
    """A BM25 corpus whose vocabulary is query_cases.corpus_vocab(), in that id order."""
    c = BM25Corpus.from_corpus([list(corpus_vocab())])
    assert c.vocab == corpus_vocab()
    return c


def assert_front_equals_host(q, m, corpus, penalty=0.5):
    """One unflagged query: tokens, ids, groups and the packed arrays against the host functions."""
    assert m.flag == 0
    toks = text.tokenize_query(q)
    assert m.tokens == toks, q
    assert m.ids == corpus.term_ids(toks).tolist(), q
    groups = text.build_gate_groups(q)
    assert [set(g) for g in m.groups] == groups and [sorted(g) for g in groups] == m.groups, q
    packed = pack_groups([groups], penalty)
    assert packed.host_queries == []
    assert b"".join(w for _, w in m.terms) == packed.term_bytes.tobytes()
    assert [g for g, _ in m.terms] == packed.term_group.tolist()
    assert np.cumsum([0] + [len(w) for _, w in m.terms]).tolist() == packed.term_off.tolist()
    assert packed.q_term.tolist() == [0, len(m.terms)] and packed.q_groups.tolist() == [len(m.groups)]


def test_crafted_queries_equal_the_host_functions(corpus):
    flagged = {}
    for q in CRAFTED:
        m = Q.model_front(q, corpus.vocab)
        if m.flag:
            flagged[q] = m.flag
            assert (m.tokens, m.ids, m.groups, m.terms) == ([], [], [], [])
        else:
            assert_front_equals_host(q, m, corpus)
    # exactly the queries over a limit are handed back: 1025 bytes, a token of 65 bytes
    want = {q: (Q.FLAG_QUERY if len(q.encode()) > 1024 else Q.FLAG_TOKEN) for q in CRAFTED
            if len(q.encode()) > 1024 or any(len(t) > 64 for t in text._TOKEN.findall(q.lower()))}
    assert flagged == want and len(want) >= 5
    assert Q.model_front("t" * 64, corpus.vocab).ids == [corpus.vocab["t" * 64]]


def test_crafted_queries_say_what_the_issue_says(corpus):
    groups = lambda q: Q.model_front(q, corpus.vocab).groups
    for q in COLOR_INSIDE:
        assert len(groups(q)) == 2 and groups(q)[1] == [q], q                 # the colour by substring + the keyword
    assert groups("credit card")[0] == sorted(text.COLORS["red"])
    assert groups("standard")[0] == sorted(text.COLORS["brown"])
    assert groups("prose poem")[0] == sorted(text.COLORS["pink"])
    assert groups("black") == [["black"]]
    assert groups("sock") == [sorted(text.SYNONYMS["sock"])] and groups("socks") == [["socks"]]
    assert groups("noise") == [sorted(text.SYNONYMS["noise"])]
    assert len(groups("wireless cat dog keyboard design headphone sock noise")) == text.MAX_GATE_GROUPS
    assert groups("cat cat cat kitten kitten") == [sorted(text.SYNONYMS["cat"]), ["kitten"]]
    assert Q.model_front("a'b'c", corpus.vocab).tokens == ["a'b", "c"]
    assert Q.model_front("pinK", corpus.vocab).tokens == ["pink"] and groups("pinK")[0] == sorted(text.COLORS["pink"])
    assert Q.model_front("socİx", corpus.vocab).tokens == ["soci", "x"]


def test_every_code_point_inside_a_query(corpus):
    """Every code point c in 'xx' + c + 'yy' (and inside and behind a colour word: 're' + c + 'd', 'pin' + c): the tokens and
    the groups are the host functions' -- the token rule and the substring rule over all of Unicode."""
    vocab = corpus.vocab
    for cp in range(sys.maxunicode + 1):
        ch = chr(cp)
        q = "xx" + ch + "yy re" + ch + "d pin" + ch
        m = Q.model_front(q, vocab)
        assert m.flag == 0
        if m.tokens != text.tokenize_query(q) or [set(g) for g in m.groups] != text.build_gate_groups(q):
            raise AssertionError(f"U+{cp:04X}: {m.tokens} / {text.tokenize_query(q)}; {m.groups} / {text.build_gate_groups(q)}")


def test_random_ascii_queries_are_never_flagged(corpus):
    qs = random_ascii_queries()
    assert len(qs) == 2000 and max(len(q) for q in qs) <= 200 and len(set(qs)) > 1500
    for q in qs:
        assert_front_equals_host(q, Q.model_front(q, corpus.vocab), corpus)


def test_reranker_ids_equal_pack_queries():
    tok = WordPieceTokenizer({w: i for i, w in enumerate(json.loads((GOLDEN / "k5_tokenizer.json").read_text())["vocab"])})
    letters = "abcdefghijklmnopqrstuvwxyz"                       # one id per letter: 510 of them stay inside 1024 bytes
    for L in (8, 9, 512):
        for n in (0, 1, L - 4, L - 3, L - 2):
            q = " ".join(letters[i % 26] for i in range(n))
            ids = tok.text_ids(q)
            assert len(ids) == n and len(q) <= 1024
            m = Q.model_front(q, {}, rerank_tokenizer=tok, max_length=L)
            packed = pack_queries([ids], L)
            assert m.flag == (Q.FLAG_RERANK if n > L - 3 else 0) and (packed.host_queries == [0]) == (n > L - 3)
            assert m.rerank_ids == packed.ids.tolist()


# ---------------------------------------------------------------------------------- the vocabulary table
def colliding_tokens(n_slots: int):
    """Two tokens of [a-z] whose walks start at the same slot, found by searching the model hash."""
    seen = {}
    for a in "abcdefghijklmnopqrstuvwxyz":
        for b in "abcdefghijklmnopqrstuvwxyz":
            t = (a + b).encode()
            s = Q.model_slot(t, n_slots)
            if s in seen:
                return seen[s], t
            seen[s] = t
    raise AssertionError("no collision among 676 tokens")


def test_vocabulary_table_is_found_entry_by_entry(corpus):
    vocab = corpus.vocab
    slots, blob, kept = Q.build_vocab_table(vocab)
    n_slots = len(slots)
    assert n_slots & (n_slots - 1) == 0 and n_slots >= 2 * len(vocab)
    eligible = {w: i for w, i in vocab.items() if 1 <= len(w.encode()) <= 64 and set(w) <= set("abcdefghijklmnopqrstuvwxyz0123456789'")}
    assert kept == len(eligible) == int((slots[:, 3] >= 0).sum())
    assert set(vocab) - set(eligible) == {"t" * 65, "café", "Upper", "two words"}
    for w, i in vocab.items():
        assert Q.table_lookup(slots, blob, w.encode()) == (i if w in eligible else -1), w
    for w in ("mous", "mousey", "kitte", "kittenss", "zzz", "t" * 63):       # a proper prefix, a proper extension, a stranger
        assert w not in vocab and Q.table_lookup(slots, blob, w.encode()) == -1
    for s in range(n_slots):                                                   # a slot's hash and length are its bytes'
        h, first, length, i = (int(v) for v in slots[s])
        if i >= 0:
            assert (h & 0xFFFFFFFF) == Q.model_hash(blob[first:first + length].tobytes())


def test_two_entries_in_one_slot_chain():
    a, b = colliding_tokens(64)
    vocab = {a.decode(): 0, b.decode(): 1, "filler": 2}
    slots, blob, kept = Q.build_vocab_table(vocab)
    assert len(slots) == 64 and kept == 3 and Q.model_slot(a, 64) == Q.model_slot(b, 64)
    s = Q.model_slot(a, 64)
    assert slots[s][3] == 0 and slots[(s + 1) & 63][3] == 1                   # the second sits behind the first
    assert Q.table_lookup(slots, blob, a) == 0 and Q.table_lookup(slots, blob, b) == 1
    assert Q.model_front(a.decode() + " " + b.decode() + " x", vocab).ids == [0, 1, -1]


def test_small_vocabularies():
    slots, blob, kept = Q.build_vocab_table({"cat": 0})
    assert len(slots) == 64 and kept == 1
    assert [Q.table_lookup(slots, blob, t) for t in (b"cat", b"ca", b"cats", b"c")] == [0, -1, -1, -1]
    slots, blob, kept = Q.build_vocab_table({})
    assert len(slots) == 64 and kept == 0 and (slots[:, 3] == -1).all()
    assert Q.table_lookup(slots, blob, b"cat") == -1
    assert Q.model_front("cat", {}).ids == [-1]
    slots, blob, kept = Q.build_vocab_table({"gap": 3})                        # ids 0..2 have no string: empty entries
    assert kept == 1 and Q.table_lookup(slots, blob, b"gap") == 3


def test_a_corpus_without_vocabulary_is_refused():
    c = BM25Corpus.from_ids(np.array([0, 1], dtype=np.int32), np.array([0, 2], dtype=np.int64), 2)
    with pytest.raises(ValueError) as e:
        c.term_ids(["x"])
    with pytest.raises(ValueError, match=str(e.value)):
        Q.QueryText(c.vocab)
