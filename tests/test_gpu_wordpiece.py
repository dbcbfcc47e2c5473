"""The device WordPiece tokenizer (csrc/rr_wordpiece.hip, embed.DeviceWordPiece) against `transformers` fixtures and the
host tokenizer: ids, cu_seqlens, positions, types and the longest sequence, exactly."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import GOLDEN
from review_recommender_amd import _lib
from review_recommender_amd.wordpiece import WordPieceTokenizer

pytestmark = pytest.mark.gpu


def device_tokenizer(tok):
    from review_recommender_amd.embed import DeviceWordPiece
    return DeviceWordPiece(tok, 0)


def run(wp, texts, L):
    tok, typ, pos, cu, max_len, needs = wp.encode_dev(texts, L)
    return tok.cpu().numpy(), typ.cpu().numpy(), pos.cpu().numpy(), cu.cpu().numpy(), max_len, needs


def assert_equals_host(got, want_ids, what=""):
    """want_ids: one id list per document.  Everything rr_ce_forward_dev is handed must be exactly the host's."""
    tok, typ, pos, cu, max_len, _ = got
    lens = np.array([len(w) for w in want_ids], dtype=np.int64)
    want_cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    assert np.array_equal(cu, want_cu), what
    flat = np.concatenate([np.asarray(w, dtype=np.int32) for w in want_ids])
    if not np.array_equal(tok, flat):
        bad = int(np.flatnonzero(tok != flat)[0])
        doc = int(np.searchsorted(want_cu, bad, side="right") - 1)
        raise AssertionError(f"{what}: document {doc} differs at token {bad - want_cu[doc]}: "
                             f"{tok[want_cu[doc]:want_cu[doc + 1]][:24]} != {flat[want_cu[doc]:want_cu[doc + 1]][:24]}")
    assert not typ.any(), what
    assert np.array_equal(pos, np.arange(len(flat), dtype=np.int32) - np.repeat(want_cu[:-1], lens).astype(np.int32)), what
    assert max_len == int(lens.max()), what


def test_wp_ascii_fixture_exactly():
    fx = json.loads((GOLDEN / "wp_ascii.json").read_text())
    tok = WordPieceTokenizer({w: i for i, w in enumerate(fx["vocab"])})
    wp = device_tokenizer(tok)
    for L in sorted({c["max_length"] for c in fx["cases"]}):
        cases = [c for c in fx["cases"] if c["max_length"] == L]
        got = run(wp, [c["text"] for c in cases], L)
        assert got[5] == [], (L, got[5])
        assert_equals_host(got, [c["ids"] for c in cases], f"wp_ascii.json max_length {L}")


def random_documents(vocab, n, seed, max_len=4000):
    """Lengths 0 .. max_len, every one of the 128 byte values drawn; words are vocabulary pieces glued together with
    random damage (case, deleted bytes inside, unmatched tails, over-long runs)."""
    rng = np.random.default_rng(seed)
    plain = [w for w in vocab if w.isascii() and w.isalnum() and not w.startswith("[")]
    cont = [w[2:] for w in vocab if w.startswith("##") and w.isascii() and w[2:].isalnum()]
    every = [chr(c) for c in range(128)]
    seps = [" ", " ", " ", " ", "  ", "\t", "\n", "\r", ".", ",", "-", "'"]
    docs = []
    for d in range(n):
        target = int(rng.integers(0, 301)) if rng.random() < 0.5 else int(rng.integers(0, max_len + 1))
        parts, size = [], 0
        while size < target:
            r = rng.random()
            if r < 0.70:
                w = plain[rng.integers(len(plain))]
                for _ in range(int(rng.integers(0, 3))):
                    w += cont[rng.integers(len(cont))]
            elif r < 0.80:
                w = "".join(every[c] for c in rng.integers(0, 128, size=int(rng.integers(1, 12))))
            elif r < 0.86:
                w = plain[rng.integers(len(plain))].upper()
            elif r < 0.92:
                w = plain[rng.integers(len(plain))]
                k = int(rng.integers(0, len(w) + 1))
                w = w[:k] + every[int(rng.choice([0, 1, 8, 11, 12, 14, 31, 127]))] + w[k:]
            elif r < 0.97:
                w = plain[rng.integers(len(plain))] + "qzqz"[:int(rng.integers(1, 4))]
            else:
                w = plain[rng.integers(len(plain))] * int(rng.integers(10, 40))      # around and beyond 100 characters
            s = seps[rng.integers(len(seps))]
            parts += [w, s]
            size += len(w) + len(s)
        docs.append("".join(parts)[:target])
    return docs


def host_ids(tok, texts):
    out = []
    for t in texts:
        tok._cache.clear() if len(tok._cache) > 500_000 else None
        out.append(tok.text_ids(t))
    return out


def cut(tok, ids, L):
    return [[tok.cls_id] + i[:L - 2] + [tok.sep_id] for i in ids]


def test_random_ascii_documents_equal_the_host_tokenizer():
    fx = json.loads((GOLDEN / "wp_ascii.json").read_text())
    tok = WordPieceTokenizer({w: i for i, w in enumerate(fx["vocab"])})
    wp = device_tokenizer(tok)
    texts = random_documents(fx["vocab"], 20_000, 7)
    assert all(t.isascii() and len(t) <= 4000 for t in texts)
    seen = np.zeros(128, dtype=bool)
    for t in texts[:2000]:
        seen[np.frombuffer(t.encode(), dtype=np.uint8)] = True
    assert seen.all()
    full = host_ids(tok, texts)
    for L in (8, 32, 512):
        got = run(wp, texts, L)
        print("max_length", L, "documents flagged:", len(got[5]))
        assert len(got[5]) == 0                     # no all-ASCII document of at most 4 000 bytes may be left to the host
        assert_equals_host(got, cut(tok, full, L), f"random documents, max_length {L}")


@pytest.mark.parametrize("n_docs", [1, 1023, 1024, 1025, 2049])
def test_cu_seqlens_at_the_edges_of_the_scan_chunks(n_docs):
    """rr_wp_scan sums the lengths in chunks of 1024 documents and keeps the longest: documents of one to three short
    words on either side of a chunk's edge, the longest one last."""
    fx = json.loads((GOLDEN / "wp_ascii.json").read_text())
    tok = WordPieceTokenizer({w: i for i, w in enumerate(fx["vocab"])})
    plain = [w for w in fx["vocab"] if w.isascii() and w.isalnum() and len(w) <= 6 and len(tok.text_ids(w)) == 1]   # one piece each
    rng = np.random.default_rng(n_docs)
    texts = [" ".join(plain[i] for i in rng.integers(0, len(plain), int(rng.integers(1, 4)))) for _ in range(n_docs)]
    texts[-1] = " ".join(plain[i] for i in rng.integers(0, len(plain), 5))
    want = cut(tok, host_ids(tok, texts), 32)
    lens = np.array([len(w) for w in want])
    assert lens[-1] == 7 and (lens[:-1] <= 5).all()                   # the maximum is the last document's alone
    got = run(device_tokenizer(tok), texts, 32)
    assert got[5] == []
    assert np.array_equal(got[3], np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)) and got[4] == 7
    assert_equals_host(got, want, f"{n_docs} short documents")


def test_documents_beyond_the_window_are_right_or_flagged():
    """20 000-byte ASCII documents: only the first max_length - 2 pieces matter, so the first 4 096 bytes answer them unless
    they hold too few pieces (then, and only then, the document may be left to the host)."""
    fx = json.loads((GOLDEN / "wp_ascii.json").read_text())
    tok = WordPieceTokenizer({w: i for i, w in enumerate(fx["vocab"])})
    wp = device_tokenizer(tok)
    base = random_documents(fx["vocab"], 40, 11, max_len=20_000)
    texts = [(t * (20_000 // max(len(t), 1) + 1))[:20_000] if t else "x" * 20_000 for t in base]
    texts += ["a" * 20_000, " " * 20_000, "soft " * 4000, "\x01" * 20_000, ("x" * 4095 + " ") * 4 + "soft"]
    full = host_ids(tok, texts)
    for L in (8, 32, 512):
        tokd, typ, pos, cu, max_len, needs = run(wp, texts, L)
        want = cut(tok, full, L)
        for i in range(len(texts)):
            ids = tokd[cu[i]:cu[i + 1]].tolist()
            if i in needs:
                assert ids == [tok.cls_id, tok.sep_id]
            else:
                assert ids == want[i], (L, i)
        # a flag is allowed only when the window was not enough: the words that end inside the first 3 000 bytes end inside
        # the window too, except one that runs on past it -- so max_length - 1 pieces there leave no excuse
        early = host_ids(tok, [t[:3000] for t in texts])
        for i in needs:
            assert len(early[i]) < L - 1, (L, i, len(early[i]))


def test_a_vocabulary_of_the_real_size():
    rng = np.random.default_rng(3)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    words = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    seen = set(words)
    for c in "abcdefghijklmnopqrstuvwxyz0123456789.,!?-'":
        for w in (c, "##" + c) if c.isalnum() else (c,):
            seen.add(w)
            words.append(w)
    while len(words) < 30_522:
        w = "".join(rng.choice(letters, size=int(rng.integers(2, 9))))
        w = w if rng.random() < 0.7 else "##" + w
        if w not in seen:
            seen.add(w)
            words.append(w)
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    wp = device_tokenizer(tok)
    texts = random_documents(words, 1500, 5)
    full = host_ids(tok, texts)
    for L in (32, 512):
        got = run(wp, texts, L)
        assert got[5] == []
        assert_equals_host(got, cut(tok, full, L), f"30 522 pieces, max_length {L}")
    assert int(np.concatenate([np.asarray(f) for f in full if f]).max()) > 20_000      # ids from all over the table


def test_input_checks_return_invalid_and_leave_the_outputs_alone(hip):
    import torch
    fx = json.loads((GOLDEN / "k5_tokenizer.json").read_text())
    tok = WordPieceTokenizer({w: i for i, w in enumerate(fx["vocab"])})
    wp = device_tokenizer(tok)
    dev = torch.device("cuda", 0)
    text = torch.from_numpy(np.frombuffer(b"soft mug", dtype=np.uint8).copy()).to(dev)
    off = torch.tensor([0, 4, 8], dtype=torch.int64, device=dev)
    out = torch.full((6, 64), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(text_bytes=8, n_docs=2, L=8, cap=16, handle=None, d_off=off):
        return hip.rr_wp_encode_dev(handle or wp.handle, p(text), text_bytes, p(d_off), n_docs, L, cap, p(out[0]), p(out[1]),
                                    p(out[2]), p(out[3]), p(out[4]), p(out[5]), None)
    for kw, word in ((dict(L=1), "max_length"), (dict(L=0), "max_length"), (dict(n_docs=0), "documents"),
                     (dict(text_bytes=1 << 31), "2^31"), (dict(text_bytes=-1), "text bytes"), (dict(cap=3), "token_capacity")):
        assert call(**kw) == -1, kw
        assert word in hip.rr_last_error().decode(), (kw, hip.rr_last_error())
    assert hip.rr_wp_encode_dev(wp.handle, p(text), 8, None, 2, 8, 16, p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(out[4]),
                                p(out[5]), None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    # special ids out of range, decreasing piece offsets: refused at creation
    from review_recommender_amd.wp_unicode import unicode_tables
    t = unicode_tables()
    uni = tuple(x for a in (t["stage1"], t["stage2"], t["pool"]) for x in (_lib.ptr(a), len(a)))
    blob = np.frombuffer(b"abc", dtype=np.uint8).copy()
    h = C.c_void_p()
    good = np.array([0, 1, 2, 3], dtype=np.int64)
    assert hip.rr_wp_create_utf8(0, _lib.ptr(blob), _lib.ptr(good), 3, 3, 0, 1, 100, *uni, C.byref(h)) == -1
    assert "special ids" in hip.rr_last_error().decode()
    assert hip.rr_wp_create_utf8(0, _lib.ptr(blob), _lib.ptr(np.array([0, 2, 1, 3], dtype=np.int64)), 3, 0, 1, 2, 100, *uni,
                                 C.byref(h)) == -1
    assert "decrease" in hip.rr_last_error().decode()
    assert hip.rr_wp_create_utf8(0, _lib.ptr(blob), _lib.ptr(good), 3, 0, 1, 2, 256, *uni, C.byref(h)) == -1
    # a valid call; then text offsets that decrease (they live on the device: the kernel refuses the document, reads
    # nothing, and rr_wp_status reports it)
    assert call() == 0
    torch.cuda.synchronize()
    wp.check()
    assert out[3, :3].tolist() == [0, 3, 6] and out[4, :2].tolist() == [0, 0] and int(out[5, 0]) == 3
    bad_off = torch.tensor([0, 4, 2], dtype=torch.int64, device=dev)
    assert call(d_off=bad_off) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="offsets"):
        wp.check()
    assert out[4, :2].tolist() == [0, 1] and out[3, :3].tolist() == [0, 3, 5]
    wp.check()                                                    # reported once
