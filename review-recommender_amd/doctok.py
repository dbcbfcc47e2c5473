"""The BM25 corpus tokenised on the GPU (csrc/rr_doctok.hip): from raw product text to token ids, and the kernel's model.

Stands in for nlp/12_product_prep.py:42-49,75-83 (``text.tokenize_document`` restates it with ``re``) followed by
``bm25.factorize_corpus``: ``DeviceDocTokenizer.tokenize(texts)`` gives the ``(tok, doc_off, vocab)`` of
``factorize_corpus([tokenize_document(t) for t in texts])`` with ``tok`` and ``doc_off`` left on the device, where
``bm25.build_bm25_index_ids`` reads them.  ``model_tokenize`` states over bytes, without ``re``, exactly what the kernel
computes -- what wp_unicode.model_tokenize is for the WordPiece kernel.

The rules (tests/test_doctok_model.py checks them against ``str.lower()`` and ``re`` over every code point):
  * exactly two code points outside ASCII lower-case onto ASCII: U+212A KELVIN SIGN -> ``k`` and U+0130 -> ``i`` + U+0307 (a
    separator); every other byte >= 0x80 is a separator, as is NUL, so no document needs the host;
  * ``[a-z0-9]+(?:'[a-z0-9]+)?`` is greedy, left to right: in a chain of runs joined by single apostrophes the joiners
    alternate (``a'b'c`` -> ``a'b``, ``c``);
  * a token's bytes are the mapped bytes; stop words and one-byte tokens go, then the first 5000 tokens stay.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .text import INDEX_STOP_WORDS, INDEX_TOKEN_CAP

TILE_BYTES = 4096           # bytes per step of the kernel's walk (rr_doctok_limits; tests read the library's value)
KELVIN = "\u212a".encode("utf-8")          # E2 84 AA -> k
DOTTED_I = "\u0130".encode("utf-8")        # C4 B0    -> i, then a separator (U+0307)
LOWERS_TO_ASCII = {0x212A: "k", 0x0130: "i\u0307"}      # every code point >= 0x80 whose str.lower() holds an ASCII character

# alnums to their lower case, the apostrophe to itself, everything else (NUL and every byte >= 0x80 included) to a space
_MAP = bytes((c + 32 if 65 <= c <= 90 else c) if (48 <= c <= 57 or 65 <= c <= 90 or 97 <= c <= 122 or c == 39) else 32
             for c in range(256))
_STOP = frozenset(w.encode("ascii") for w in INDEX_STOP_WORDS)


def model_tokenize(data: bytes) -> List[bytes]:
    """The tokens rr_doctok_count_dev / rr_doctok_emit_dev give for one document of raw bytes."""
    mapped = bytes(data).replace(KELVIN, b"k").replace(DOTTED_I, b"i ").translate(_MAP)
    out: List[bytes] = []
    for chunk in mapped.split():                   # maximal pieces of alnums and apostrophes
        runs = chunk.split(b"'")                   # an empty run = two apostrophes in a row, or one at either end
        i = 0
        while i < len(runs):
            if not runs[i]:
                i += 1
                continue
            if i + 1 < len(runs) and runs[i + 1]:  # one apostrophe, then a run: the token takes both
                tok = runs[i] + b"'" + runs[i + 1]
                i += 2
            else:
                tok = runs[i]
                i += 1
            if len(tok) > 1 and tok not in _STOP:
                out.append(tok)
                if len(out) == INDEX_TOKEN_CAP:
                    return out
    return out


def encode_text(t) -> bytes:
    """A text's bytes as the device reads them; a lone surrogate becomes its three (separator) bytes."""
    return t if isinstance(t, (bytes, bytearray)) else str(t).encode("utf-8", "surrogatepass")


def _pack(texts) -> Tuple[np.ndarray, np.ndarray]:
    if len(texts) and not isinstance(texts[0], (bytes, bytearray)):
        from .embed import _utf8_column
        return _utf8_column(texts)
    docs = [encode_text(t) for t in texts]
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), off


def _upload(a: np.ndarray, dev):
    """A host array (possibly a read-only view of an Arrow buffer) as a tensor on `dev`."""
    import warnings
    import torch
    if a.size == 0:
        return torch.zeros(1, dtype=torch.from_numpy(np.zeros(1, a.dtype)).dtype, device=dev)[:0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # (from_numpy on a read-only array: it is only read)
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class DeviceDocTokenizer:
    """The index-time tokenizer and the vocabulary on one GPU.  Work is queued on torch's current stream of `device`."""

    def __init__(self, device: int = 0, stop_words: Optional[Sequence[str]] = None):
        import torch
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the document tokenizer runs on the device only")
        lib = _lib.load()
        tile, per, cap = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(lib.rr_doctok_limits(C.byref(tile), C.byref(per), C.byref(cap)), "rr_doctok_limits")
        if (tile.value, cap.value) != (TILE_BYTES, INDEX_TOKEN_CAP):
            raise _lib.HipLibraryError("doctok.py and csrc/rr_doctok.hip disagree on the tile or the token cap")
        self.tile = tile.value
        self.device = int(device)
        words = sorted(w.encode("ascii") for w in (INDEX_STOP_WORDS if stop_words is None else stop_words))
        off = np.zeros(len(words) + 1, dtype=np.int64)
        np.cumsum([len(w) for w in words], out=off[1:])
        blob = np.frombuffer(b"".join(words) + b"\0", dtype=np.uint8).copy()
        h = C.c_void_p()
        _lib.check(lib.rr_doctok_create(self.device, _lib.ptr(blob), _lib.ptr(off), len(words), C.byref(h)), "rr_doctok_create")
        self._h = h
        self.seconds: Dict[str, float] = {}

    # -- the C calls
    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def sizes(self) -> Tuple[int, int, int, int]:
        """(T, arena bytes, n_terms, vocabulary bytes); waits for the device.  ValueError for offsets that decrease or leave
        the text (the handle keeps what the calls before established)."""
        out = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.load().rr_doctok_sizes(self._h, _lib.ptr(out)), "rr_doctok_sizes")
        return tuple(int(x) for x in out)

    def tokenize_stream_dev(self, d_text, text_bytes: int, d_off, n_docs: int):
        """The two passes: -> (doc_off int64[n + 1] on the device, T).  The token stream stays in the handle."""
        import torch
        lib = _lib.load()
        dev = torch.device("cuda", self.device)
        doc_off = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        p_text = C.c_void_p(d_text.data_ptr() if d_text is not None and d_text.numel() else 0)
        p_off = C.c_void_p(d_off.data_ptr())
        _lib.check(lib.rr_doctok_count_dev(self._h, p_text, int(text_bytes), p_off, int(n_docs), C.c_void_p(doc_off.data_ptr()),
                                           self._stream()), "rr_doctok_count_dev")
        T = self.sizes()[0]
        _lib.check(lib.rr_doctok_emit_dev(self._h, p_text, int(text_bytes), p_off, int(n_docs), C.c_void_p(doc_off.data_ptr()),
                                          self._stream()), "rr_doctok_emit_dev")
        return doc_off, T

    def vocab_dev(self, T: int, hash_bits: int = 64):
        """Ids in first-appearance order -> (tok int32[T] on the device, n_terms, vocabulary bytes).  Waits."""
        import torch
        tok = torch.empty(max(T, 1), dtype=torch.int32, device=torch.device("cuda", self.device))[:T]
        _lib.check(_lib.load().rr_doctok_vocab_dev(self._h, int(hash_bits), C.c_void_p(tok.data_ptr() if T else 0), self._stream()),
                   "rr_doctok_vocab_dev")
        _, _, n_terms, vbytes = self.sizes()
        return tok, n_terms, vbytes

    def vocab_terms(self, tok, n_terms: int, vbytes: int) -> List[str]:
        """The vocabulary in id order, copied from the device."""
        blob = np.empty(max(vbytes, 1), dtype=np.uint8)
        off = np.zeros(n_terms + 1, dtype=np.int64)
        _lib.check(_lib.load().rr_doctok_copy_vocab(self._h, C.c_void_p(tok.data_ptr() if tok.numel() else 0), _lib.ptr(blob),
                                                    _lib.ptr(off)), "rr_doctok_copy_vocab")
        return _split_ascii(blob[:vbytes], off)

    def token_stream(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(arena offsets int64[T], lengths int32[T], arena bytes) of the stream before the vocabulary (tests)."""
        T, arena_bytes, _, _ = self.sizes()
        pos, ln = np.empty(T, dtype=np.int64), np.empty(T, dtype=np.int32)
        arena = np.zeros(max(arena_bytes, 1), dtype=np.uint8)
        _lib.check(_lib.load().rr_doctok_copy_tokens(self._h, _lib.ptr(pos) if T else None, _lib.ptr(ln) if T else None,
                                                     _lib.ptr(arena)), "rr_doctok_copy_tokens")
        return pos, ln, arena

    # -- whole columns
    def tokenize_dev(self, d_text, text_bytes: int, d_off, n_docs: int, hash_bits: int = 64):
        """``d_text`` uint8 and ``d_off`` int64[n + 1] tensors on the device (the layout embed._utf8_column makes) ->
        (tok int32[T], doc_off int64[n + 1]) on the device and vocab: Dict[str, int]."""
        import time
        import torch
        with torch.cuda.device(self.device):
            t0 = time.perf_counter()
            doc_off, T = self.tokenize_stream_dev(d_text, text_bytes, d_off, n_docs)
            torch.cuda.current_stream(self.device).synchronize()
            t1 = time.perf_counter()
            tok, n_terms, vbytes = self.vocab_dev(T, hash_bits)
            t2 = time.perf_counter()
            terms = self.vocab_terms(tok, n_terms, vbytes)
            vocab = dict(zip(terms, range(n_terms)))
            t3 = time.perf_counter()
        self.seconds.update(tokenize=t1 - t0, vocabulary=t2 - t1, vocabulary_download=t3 - t2)
        return tok, doc_off, vocab

    def tokenize(self, texts, hash_bits: int = 64, offsets: Optional[np.ndarray] = None):
        """The same for a column of str (or bytes); ``offsets`` replaces the running sum of their lengths (tests)."""
        import time
        import torch
        texts = texts.tolist() if hasattr(texts, "tolist") else list(texts)
        t0 = time.perf_counter()
        raw, off = _pack(texts)
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.int64)
        t1 = time.perf_counter()
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_text = _upload(raw, dev)
            d_off = _upload(off, dev)
            torch.cuda.current_stream(dev).synchronize()
            t2 = time.perf_counter()
            self.seconds.update(pack=t1 - t0, upload=t2 - t1)
            return self.tokenize_dev(d_text, len(raw), d_off, len(texts), hash_bits)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_doctok_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _split_ascii(blob: np.ndarray, off: np.ndarray) -> List[str]:
    """Term i = blob[off[i] : off[i + 1]] as str (the vocabulary is ASCII)."""
    n = len(off) - 1
    if n == 0:
        return []
    try:
        import pyarrow as pa
        arr = pa.LargeStringArray.from_buffers(n, pa.py_buffer(np.ascontiguousarray(off, dtype=np.int64)),
                                               pa.py_buffer(np.ascontiguousarray(blob)))
        return arr.to_pylist()
    except ImportError:
        s = blob.tobytes().decode("ascii")
        o = off.tolist()
        return [s[o[i]:o[i + 1]] for i in range(n)]


def ids_to_corpus(tok: np.ndarray, doc_off: np.ndarray, vocab: Dict[str, int]) -> List[List[str]]:
    """The token lists the ids stand for (``blob["corpus"]``): one object-array take and one split."""
    if len(doc_off) <= 1:                          # no documents (np.split would give one empty piece)
        return []
    terms = np.empty(len(vocab), dtype=object)
    terms[:] = list(vocab)                         # (dicts keep insertion order = id order)
    flat = terms[np.asarray(tok, dtype=np.int64)] if len(vocab) else np.empty(0, dtype=object)
    return [a.tolist() for a in np.split(flat, np.asarray(doc_off[1:-1], dtype=np.int64))]
