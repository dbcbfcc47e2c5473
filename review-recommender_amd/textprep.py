"""Review text cleaned, filtered and deduplicated on the GPU (csrc/rr_textprep.hip), and the kernel's model on the CPU.

Stands in for nlp/11_build_product_embeddings.py:110-118: `normalize_text`, the length filter, `looks_spammy` and
`drop_duplicates(subset=["sku", "__txt"])`, in front of the device tokenizer.  `TextPrep` is a thin ctypes wrapper of the three
stages (clean, dedup, compact); `model_clean` states in plain Python, without `re`, exactly what the clean kernel computes,
needs_host included -- what wp_unicode.model_tokenize is for the tokenizer.
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

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_textprep_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
