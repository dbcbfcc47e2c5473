"""Review text cleaned, filtered and deduplicated on the GPU (csrc/rr_textprep.hip), and the kernel's model on the CPU.

Stands in for nlp/11_build_product_embeddings.py:110-118: `normalize_text`, the length filter, `looks_spammy` and
`drop_duplicates(subset=["sku", "__txt"])`, in front of the device tokenizer.  `TextPrep` is a thin ctypes wrapper of the three
stages (clean, dedup, compact); `model_clean` states in plain Python, without `re`, exactly what the clean kernel computes,
needs_host included -- what wp_unicode.model_tokenize is for the tokenizer.

The head calls (`head_measure`, `head_offsets`, `head_write`) serve product text that is already on the device
(products.DeviceProductText): the first max_chars code points of a document of ANY length, normalised as nlp/11's
normalize_text does (for embed.build_product_embeddings_device) or verbatim (str[:k], for RerankText.from_device).
`model_head` is their statement in Python.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

SHORT, SPAM, NEEDS_HOST, DUP = 1, 2, 4, 8          # include/rr_hip.h: RR_TP_*
WINDOW_BYTES = 16384        # bytes of a document the kernel holds on chip (rr_textprep_limits; tests/test_textprep_model.py
TILE_BYTES = 4096           # checks the three against the library): bytes per step of its walk,
SLICE_BYTES = 16            # consecutive bytes per thread
MIN_CHARS, MAX_CHARS = 10, 4000                    # nlp/11_build_product_embeddings.py:22-23

# str.isspace() and re's \s (str patterns) agree on these 29 code points
WHITESPACE = frozenset([*range(0x09, 0x0E), *range(0x1C, 0x21), 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029,
                        0x202F, 0x205F, 0x3000])
# the code points >= 0x80 that re.IGNORECASE folds onto a letter of the spam patterns (onto i, i and s)
FOLDED = frozenset([0x130, 0x131, 0x17F])
URL_PREFIXES = ("http://", "https://", "www.")
PROMO_PHRASES = ("discount code", "use code", "sponsored")
_LOWER = {c: c + 32 for c in range(ord("A"), ord("Z") + 1)}


def model_clean_bytes(raw: bytes, spam: bool = True, max_chars: int = MAX_CHARS) -> Tuple[bytes, int]:
    """What rr_textprep_clean_dev answers for one document: (normalised UTF-8 text, status word).  A document left to the
    host has the status NEEDS_HOST alone and no text.  max_chars: the cut of rr_textprep_clean_chars_dev, 0 = none
    (nlp/10_product_prep.py)."""
    if len(raw) > WINDOW_BYTES:
        return b"", NEEDS_HOST
    try:
        s = raw.decode("utf-8")                    # strict: overlong forms, surrogates and > U+10FFFF are malformed
    except UnicodeDecodeError:
        return b"", NEEDS_HOST
    if spam and any(ord(c) in FOLDED for c in s):
        return b"", NEEDS_HOST
    out: List[str] = []                            # one entry per code point of the result
    after_space = False
    for c in s:
        if ord(c) in WHITESPACE:
            after_space = True
            continue
        if after_space and out:                    # strip() and the collapse of \s+ at once
            out.append(" ")
        out.append(c)
        after_space = False
    if max_chars:
        del out[max_chars:]                        # after the collapse: the text may now end in a space
    status = SHORT if len(out) < MIN_CHARS else 0
    txt = "".join(out)
    if spam and _spammy(txt, out):
        status |= SPAM
    return txt.encode("utf-8"), status


def _decode_one(raw: bytes, i: int) -> Tuple[int, int]:
    """The code point that starts at raw[i], strictly: (code point, bytes), or (-1, 0) for a byte that starts nothing, too
    few or wrong continuation bytes, an overlong form, a surrogate or a value above U+10FFFF."""
    b = raw[i]
    if b < 0x80:
        return b, 1
    if 0xC2 <= b <= 0xDF:
        n, c, lowest = 2, b & 0x1F, 0x80
    elif b & 0xF0 == 0xE0:
        n, c, lowest = 3, b & 0x0F, 0x800
    elif 0xF0 <= b <= 0xF4:
        n, c, lowest = 4, b & 0x07, 0x10000
    else:
        return -1, 0
    if i + n > len(raw):
        return -1, 0
    for k in range(1, n):
        t = raw[i + k]
        if t & 0xC0 != 0x80:
            return -1, 0
        c = (c << 6) | (t & 0x3F)
    if c < lowest or c > 0x10FFFF or 0xD800 <= c <= 0xDFFF:
        return -1, 0
    return c, n


def model_head(raw: bytes, max_chars: int, normalize: bool, min_chars: int = 0) -> Tuple[bytes, int]:
    """What rr_textprep_head_measure_dev / rr_textprep_head_write_dev answer for one document of ANY length: (the UTF-8
    bytes of its head, status word).  A walk over code points, decoded strictly one at a time WHILE fewer than max_chars
    have been emitted; a malformed one met during that walk gives (b"", NEEDS_HOST), bytes behind the point where the walk
    stops are never examined.  normalize=True: a whitespace code point (WHITESPACE) sets a pending flag and emits nothing;
    any other first emits one U+0020 if the flag is set and something was emitted before -- the space counts, and when it
    is the max_chars-th emission the walk stops there -- then itself: embed.normalize_text (strip, \\s+ -> " ",
    [:max_chars]) as a prefix computation.  normalize=False: every code point is emitted verbatim: s[:max_chars].
    Status: SHORT when min_chars > 0 and fewer than min_chars code points were emitted, else 0."""
    out = bytearray()
    emitted, pending, i = 0, False, 0
    while emitted < max_chars and i < len(raw):
        c, n = _decode_one(raw, i)
        if n == 0:
            return b"", NEEDS_HOST
        if normalize and c in WHITESPACE:
            pending = True
        else:
            if pending and emitted:
                out.append(0x20)
                emitted += 1
            pending = False
            if emitted < max_chars:
                out += raw[i:i + n]
                emitted += 1
        i += n
    return bytes(out), (SHORT if min_chars > 0 and emitted < min_chars else 0)


def _spammy(txt: str, chars: List[str]) -> bool:
    low = txt.translate(_LOWER)                    # ASCII letters only; FOLDED was left to the host
    # URL_RE: the only whitespace left is U+0020, so a match runs to its token's end: one per token that holds a prefix
    # which ends before the token does
    urls = sum(any(p in tok[:-1] for p in URL_PREFIXES) for tok in low.split(" "))
    if urls >= 2 or any(p in low for p in PROMO_PHRASES):
        return True
    i = low.find("i received this")                # ... .* free: the earliest end, then any later start
    if i >= 0 and low.find("free", i + 15) >= 0:
        return True
    run = 0                                        # REPEAT_RE: ten equal consecutive code points, case-sensitive
    for k, c in enumerate(chars):
        run = run + 1 if k and c == chars[k - 1] else 1
        if run >= 10:
            return True
    return False


def model_clean(text, spam: bool = True, max_chars: int = MAX_CHARS) -> Tuple[str, int]:
    """`model_clean_bytes` for a str (or bytes): (normalised text, status word).  A str with a lone surrogate has no UTF-8
    form: it is encoded as the three bytes the kernel calls malformed."""
    raw = text if isinstance(text, (bytes, bytearray)) else str(text).encode("utf-8", "surrogatepass")
    out, status = model_clean_bytes(bytes(raw), spam, max_chars)
    return out.decode("utf-8"), status


class TextPrep:
    """The three device stages on one GPU.  Every pointer argument is a device address (int); calls are queued on `stream`
    (a hipStream_t as int, None = the NULL stream) and must be stream-ordered per handle."""

    def __init__(self, device: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the text stages run on the device only")
        lib = _lib.load()
        window, tile, per = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(lib.rr_textprep_limits(C.byref(window), C.byref(tile), C.byref(per)), "rr_textprep_limits")
        if (window.value, tile.value, per.value) != (WINDOW_BYTES, TILE_BYTES, SLICE_BYTES):
            raise _lib.HipLibraryError("textprep.py and csrc/rr_textprep.hip disagree on the kernel's window")
        self.device = device
        h = C.c_void_p()
        _lib.check(lib.rr_textprep_create(device, C.byref(h)), "rr_textprep_create")
        self._h = h

    def clean(self, text: int, text_bytes: int, offsets: int, n_docs: int, spam: bool, out: int, out_len: int, status: int,
              stream: Optional[int] = None, max_chars: int = MAX_CHARS) -> None:
        """max_chars: the cut in code points (nlp/11's 4000), 0 = none (nlp/10)."""
        _lib.check(_lib.load().rr_textprep_clean_chars_dev(self._h, C.c_void_p(text), int(text_bytes), C.c_void_p(offsets),
                                                           int(n_docs), 1 if spam else 0, int(max_chars), C.c_void_p(out),
                                                           C.c_void_p(out_len), C.c_void_p(status), C.c_void_p(stream)),
                   "rr_textprep_clean_dev")

    def dedup(self, text: int, text_bytes: int, offsets: int, lens: int, group: int, status: int, n_docs: int,
              hash_bits: int = 64, stream: Optional[int] = None) -> None:
        _lib.check(_lib.load().rr_textprep_dedup_dev(self._h, C.c_void_p(text), int(text_bytes), C.c_void_p(offsets),
                                                     C.c_void_p(lens), C.c_void_p(group), C.c_void_p(status), int(n_docs),
                                                     int(hash_bits), C.c_void_p(stream)), "rr_textprep_dedup_dev")

    def compact(self, text: int, text_bytes: int, offsets: int, lens: int, status: int, n_docs: int, out_text: int,
                out_bytes: int, out_offsets: int, src_row: int, count: int, stream: Optional[int] = None) -> None:
        _lib.check(_lib.load().rr_textprep_compact_dev(self._h, C.c_void_p(text), int(text_bytes), C.c_void_p(offsets),
                                                       C.c_void_p(lens), C.c_void_p(status), int(n_docs), C.c_void_p(out_text),
                                                       int(out_bytes), C.c_void_p(out_offsets), C.c_void_p(src_row),
                                                       C.c_void_p(count), C.c_void_p(stream)), "rr_textprep_compact_dev")

    def head_measure(self, text: int, text_bytes: int, offsets: int, n_src_docs: int, doc_rows: Optional[int], n_docs: int,
                     max_chars: int, normalize: bool, min_chars: int, out_len: int, status: int,
                     stream: Optional[int] = None) -> None:
        """Pass 1 of the heads (`model_head`): lengths and status words of n_docs documents; doc_rows: address of the int32
        source row of every output document, None = identity."""
        _lib.check(_lib.load().rr_textprep_head_measure_dev(self._h, C.c_void_p(text), int(text_bytes), C.c_void_p(offsets),
                                                            int(n_src_docs), C.c_void_p(doc_rows), int(n_docs), int(max_chars),
                                                            1 if normalize else 0, int(min_chars), C.c_void_p(out_len),
                                                            C.c_void_p(status), C.c_void_p(stream)), "rr_textprep_head_measure_dev")

    def head_offsets(self, out_len: int, status: int, n_docs: int, out_off: int, stream: Optional[int] = None) -> None:
        """out_off int64 [n_docs + 1]: where pass 2 writes the surviving heads, back to back."""
        _lib.check(_lib.load().rr_textprep_head_offsets_dev(self._h, C.c_void_p(out_len), C.c_void_p(status), int(n_docs),
                                                            C.c_void_p(out_off), C.c_void_p(stream)), "rr_textprep_head_offsets_dev")

    def head_write(self, text: int, text_bytes: int, offsets: int, n_src_docs: int, doc_rows: Optional[int], n_docs: int,
                   max_chars: int, normalize: bool, min_chars: int, out_len: int, status: int, out_text: int, out_bytes: int,
                   out_off: int, stream: Optional[int] = None) -> None:
        """Pass 2: the heads of the documents whose status word is 0, at out_text + out_off[j]."""
        _lib.check(_lib.load().rr_textprep_head_write_dev(self._h, C.c_void_p(text), int(text_bytes), C.c_void_p(offsets),
                                                          int(n_src_docs), C.c_void_p(doc_rows), int(n_docs), int(max_chars),
                                                          1 if normalize else 0, int(min_chars), C.c_void_p(out_len),
                                                          C.c_void_p(status), C.c_void_p(out_text), int(out_bytes),
                                                          C.c_void_p(out_off), C.c_void_p(stream)), "rr_textprep_head_write_dev")

    def check(self) -> None:
        """Raises ValueError when a call since the last check met offsets that decrease or leave the text (waits for the device)."""
        bad = C.c_int32()
        _lib.check(_lib.load().rr_textprep_status(self._h, C.byref(bad)), "rr_textprep_status")

    # -- whole batches from host data: what the tests and small callers use
    def clean_docs(self, docs: Sequence[bytes], spam: bool = True, offsets: Optional[np.ndarray] = None,
                   max_chars: int = MAX_CHARS):
        """(texts, lengths, status words) of rr_textprep_clean_dev for `docs`, out of place; `offsets` replaces the running
        sum of their lengths (tests: broken offsets).  Does not call check()."""
        import torch
        n = len(docs)
        blob = b"".join(docs)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(d) for d in docs], out=off[1:])
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.int64)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_text = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to(dev)
            d_off = torch.from_numpy(off).to(dev)
            d_out = torch.full((len(blob) + 1,), 0xEE, dtype=torch.uint8, device=dev)
            d_len = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
            d_st = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
            self.clean(d_text.data_ptr(), len(blob), d_off.data_ptr(), n, spam, d_out.data_ptr(), d_len.data_ptr(), d_st.data_ptr(),
                       torch.cuda.current_stream(dev).cuda_stream, max_chars)
            torch.cuda.current_stream(dev).synchronize()
            out, lens, st = d_out.cpu().numpy(), d_len.cpu().numpy()[:n], d_st.cpu().numpy()[:n]
        return out, lens, st

    def head_docs(self, docs: Sequence[bytes], max_chars: int, normalize: bool, min_chars: int = 0,
                  doc_rows: Optional[Sequence[int]] = None, offsets: Optional[np.ndarray] = None, capacity: Optional[int] = None):
        """(output buffer, out_off, lengths, status words) of measure + offsets + write for `docs`; `doc_rows` picks the
        source document of every output document, `offsets` replaces the running sum of the lengths and `capacity` the size
        the write call is told (tests: broken arguments; the buffer itself always has room).  The buffer is filled with 0xEE
        first.  Does not call check()."""
        import torch
        blob = b"".join(docs)
        off = np.zeros(len(docs) + 1, dtype=np.int64)
        np.cumsum([len(d) for d in docs], out=off[1:])
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.int64)
        n_src = len(off) - 1
        rows = None if doc_rows is None else np.ascontiguousarray(doc_rows, dtype=np.int32)
        n = n_src if rows is None else len(rows)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            d_text = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to(dev)
            d_off = torch.from_numpy(off).to(dev)
            d_rows = None if rows is None else torch.from_numpy(rows if n else np.zeros(1, np.int32)).to(dev)
            p_rows = None if d_rows is None else d_rows.data_ptr()
            d_len = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
            d_st = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
            d_out_off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
            args = (d_text.data_ptr(), len(blob), d_off.data_ptr(), n_src, p_rows, n, max_chars, normalize, min_chars,
                    d_len.data_ptr(), d_st.data_ptr())
            self.head_measure(*args, st.cuda_stream)
            self.head_offsets(d_len.data_ptr(), d_st.data_ptr(), n, d_out_off.data_ptr(), st.cuda_stream)
            out_off = d_out_off.cpu().numpy()
            room = max(int(out_off[-1]), 0)
            d_out = torch.full((room + 16,), 0xEE, dtype=torch.uint8, device=dev)
            self.head_write(*args, d_out.data_ptr(), room if capacity is None else capacity, d_out_off.data_ptr(), st.cuda_stream)
            st.synchronize()
            return d_out.cpu().numpy(), out_off, d_len.cpu().numpy()[:n], d_st.cpu().numpy()[:n]

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_textprep_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
