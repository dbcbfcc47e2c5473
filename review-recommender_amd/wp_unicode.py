"""Unicode tables and the CPU model of the device tokenizer (csrc/rr_wordpiece.hip: rr_wp_tokenize_utf8).

Everything `wordpiece.basic_tokenize` does to a text for an uncased vocabulary reduces to a rule per code point, so the device
needs a table lookup per code point and no normaliser:

    class of a raw code point c
        deleted   c == 0, c == 0xFFFD, _is_control(c)              (the neighbours join)
        blank     _is_whitespace(c), U+2028, U+2029                (what str.split() breaks on)
        cjk       _is_cjk(c)                                       (its mapped form is a word of its own)
        other     everything else
    mapped form of a cjk / other c:   f(c) = NFD(c.lower()) without its Mn characters      (0 .. 3 code points)
        a mapped code point with _is_punctuation is a word of its own, the others extend the current word
    hard      c depends on its neighbours: U+03A3 (lower-cased to a final sigma by context) and every code point that has,
              itself or in NFD(c.lower()), a character of non-zero combining class that is not Mn (canonical reordering of
              such marks is not local).  A document with one stays with the host tokenizer.

(NFD(NFC(x)) == NFD(x), so the host's NFC step changes nothing once NFD and the Mn strip have run.)  The tables are made
from the RUNNING interpreter's `unicodedata`, never from a list, so that they agree with the host tokenizer they stand in for.

`unicode_tables()`  two stages over U+0000 .. U+10FFFF in blocks of 128 code points:
    stage1  uint16 [8704]       block -> index of its (shared) block in stage2
    stage2  uint32 [blocks*128] class (bits 0-2) | mapped code points n (3-4) | identity: f(c) = c (5) |
                                punctuation flag of mapped code point j (6 + j) | first mapped code point in pool (9-31)
    pool    uint32 []           the mapped code points of the entries that are not identities
`model_tokenize()`  what the kernel does, in Python: the specification of its ids and of its needs_host flags.
"""
from __future__ import annotations

import functools
import unicodedata
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from .wordpiece import WordPieceTokenizer, _is_cjk, _is_control, _is_punctuation, _is_whitespace

DELETED, BLANK, CJK, OTHER, HARD = 0, 1, 2, 3, 4
BLOCK = 128
N_BLOCKS = 0x110000 // BLOCK
WINDOW = 4096           # RR_WP_WINDOW: raw bytes the kernel reads, and the bound on the mapped bytes it holds

REASONS = ("hard", "malformed", "window", "bound")


def mapped_form(ch: str) -> str:
    return "".join(x for x in unicodedata.normalize("NFD", ch.lower()) if unicodedata.category(x) != "Mn")


def is_hard(cp: int) -> bool:
    if cp == 0x03A3:
        return True
    ch = chr(cp)
    return any(unicodedata.combining(x) != 0 and unicodedata.category(x) != "Mn"
               for x in ch + unicodedata.normalize("NFD", ch.lower()))


def char_class(cp: int) -> int:
    ch = chr(cp)
    if cp == 0 or cp == 0xFFFD or _is_control(ch):
        return DELETED
    if _is_whitespace(ch) or cp in (0x2028, 0x2029):
        return BLANK
    if is_hard(cp):
        return HARD
    return CJK if _is_cjk(cp) else OTHER


@functools.lru_cache(maxsize=1)
def unicode_tables() -> Dict[str, object]:
    """{"stage1", "stage2", "pool": numpy arrays as the module text lays them out; "hard": the hard code points, sorted;
    "unidata_version"}.  About 2 s of Python once per process."""
    stage1 = np.zeros(N_BLOCKS, dtype=np.uint16)
    blocks: Dict[bytes, int] = {}
    rows: List[np.ndarray] = []
    pool: List[int] = []
    pooled: Dict[Tuple[int, ...], int] = {}
    hard: List[int] = []
    category = unicodedata.category
    for b in range(N_BLOCKS):
        row = np.zeros(BLOCK, dtype=np.uint32)
        for j in range(BLOCK):
            cp = b * BLOCK + j
            if category(chr(cp)) in ("Cn", "Co", "Cs"):          # most of the code space: deleted (entry 0)
                continue
            k = char_class(cp)
            if k == HARD:
                hard.append(cp)
            if k not in (CJK, OTHER):
                row[j] = k
                continue
            m = mapped_form(chr(cp))
            if len(m) > 3:
                raise RuntimeError(f"U+{cp:04X} maps to {len(m)} code points: the entry format holds 3")
            e = k | len(m) << 3
            for i, x in enumerate(m):
                e |= int(_is_punctuation(x)) << (6 + i)
            if m == chr(cp):
                e |= 1 << 5
            elif m:
                key = tuple(map(ord, m))
                if key not in pooled:
                    pooled[key] = len(pool)
                    pool.extend(key)
                e |= pooled[key] << 9
            row[j] = e
        key = row.tobytes()
        if key not in blocks:
            blocks[key] = len(rows)
            rows.append(row)
        stage1[b] = blocks[key]
    if len(pool) >= 1 << 23 or len(rows) >= 1 << 16:
        raise RuntimeError("the Unicode table outgrew its entry format")
    return {"stage1": stage1, "stage2": np.concatenate(rows), "pool": np.asarray(pool or [0], dtype=np.uint32),
            "hard": hard, "unidata_version": unicodedata.unidata_version}


def table_bytes(tables=None) -> int:
    t = tables or unicode_tables()
    return int(t["stage1"].nbytes + t["stage2"].nbytes + t["pool"].nbytes)


def lookup(cp: int, tables=None) -> Tuple[int, str, Tuple[bool, ...]]:
    """(class, mapped form, punctuation flag per mapped code point) of one code point, READ FROM THE TABLE."""
    t = tables or unicode_tables()
    e = int(t["stage2"][int(t["stage1"][cp >> 7]) * BLOCK + (cp & 127)])
    k, n = e & 7, (e >> 3) & 3
    if k not in (CJK, OTHER):
        return k, "", ()
    m = chr(cp) if e & 32 else "".join(chr(int(x)) for x in t["pool"][(e >> 9):(e >> 9) + n])
    return k, m, tuple(bool((e >> (6 + i)) & 1) for i in range(n))


def utf8_well_formed(raw: bytes) -> bool:
    """The kernel's rule, byte by byte: lead bytes C2-F4 with their continuation bytes inside the text, no overlong form,
    no surrogate, nothing above U+10FFFF, no continuation byte without its lead.  (= Python's strict decoder.)"""
    i, n = 0, len(raw)
    while i < n:
        b = raw[i]
        if b < 0x80:
            i += 1
            continue
        if b < 0xC2 or b > 0xF4:
            return False
        ln = 4 if b >= 0xF0 else 3 if b >= 0xE0 else 2
        if i + ln > n:
            return False
        cp = b & (0xFF >> (ln + 1))
        for c in raw[i + 1:i + ln]:
            if c & 0xC0 != 0x80:
                return False
            cp = cp << 6 | (c & 0x3F)
        if (ln == 3 and cp < 0x800) or (ln == 4 and cp < 0x10000) or cp > 0x10FFFF or 0xD800 <= cp <= 0xDFFF:
            return False
        i += ln
    return True


_INFO: Dict[str, Tuple[int, str, Tuple[int, ...], int]] = {}


def _info(ch: str):
    """(class, mapped text, kind per mapped character: 1 blank / 2 a word of its own / 3 word character, mapped UTF-8 bytes)."""
    hit = _INFO.get(ch)
    if hit is None:
        k, m, punct = lookup(ord(ch))
        if k == BLANK:
            hit = (k, " ", (1,), 1)
        else:
            hit = (k, m, tuple(2 if (k == CJK or p) else 3 for p in punct), len(m.encode("utf-8")))
        _INFO[ch] = hit
    return hit


def window_of(raw: bytes, window: int = WINDOW) -> Tuple[int, bool]:
    """(bytes the kernel reads, whether the document was cut): the window ends on a character boundary -- at most three
    continuation bytes are given back."""
    if len(raw) <= window:
        return len(raw), False
    wlen = window
    for _ in range(3):
        if wlen > 0 and raw[wlen] & 0xC0 == 0x80:
            wlen -= 1
        else:
            break
    return wlen, True


def model_words(text: str) -> Optional[List[str]]:
    """The words the kernel forms from `text` (what `basic_tokenize` gives), or None when it holds a hard code point."""
    infos = list(map(_info, text))
    if any(i[0] == HARD for i in infos):
        return None
    chars = "".join(i[1] for i in infos)
    kinds = [k for i in infos for k in i[2]]
    words, i, n = [], 0, len(chars)
    while i < n:
        if kinds[i] == 2:
            words.append(chars[i])
            i += 1
        elif kinds[i] == 3:
            e = i + 1
            while e < n and kinds[e] == 3:
                e += 1
            words.append(chars[i:e])
            i = e
        else:
            i += 1
    return words


def model_tokenize(text: Union[str, bytes], tokenizer: WordPieceTokenizer, max_length: Optional[int] = None,
                   window: int = WINDOW, want_ids: bool = True) -> Tuple[Optional[List[int]], int, Optional[str]]:
    """(ids, needs_host, reason) as rr_wp_encode_dev answers one document.  needs_host = 1 comes with the
    placeholder [CLS] [SEP] and one of REASONS, tested in the kernel's order over the bytes it reads (the whole document,
    or its first `window` bytes):
        "malformed"  the bytes read are not well-formed UTF-8
        "hard"       they hold a hard code point
        "bound"      their mapped text is longer than `window` bytes
        "window"     the document is longer than the window and the words that end inside it give fewer than
                     max_length - 2 pieces
    want_ids=False skips the pieces where the flag does not depend on them (ids is then None)."""
    L = max_length or tokenizer.max_length
    raw = text if isinstance(text, (bytes, bytearray)) else text.encode("utf-8")
    flagged = [tokenizer.cls_id, tokenizer.sep_id]
    wlen, cut = window_of(raw, window)
    head = bytes(raw[:wlen])
    if not utf8_well_formed(head):
        return flagged, 1, "malformed"
    infos = list(map(_info, head.decode("utf-8")))
    if any(i[0] == HARD for i in infos):
        return flagged, 1, "hard"
    if sum(i[3] for i in infos) > window:
        return flagged, 1, "bound"
    if not want_ids and not cut:
        return None, 0, None
    chars = "".join(i[1] for i in infos)
    kinds = [k for i in infos for k in i[2]]
    pieces: List[int] = []
    vocab, unk, n = tokenizer.vocab, tokenizer.unk_id, len(chars)
    i = 0
    while i < n:
        k = kinds[i]
        if k == 2:
            pieces.append(vocab.get(chars[i], unk))
            i += 1
        elif k == 3:
            e = i + 1
            while e < n and kinds[e] == 3:
                e += 1
            if not (cut and e == n):                 # the window may have cut this word: it does not count
                pieces.extend(tokenizer._word(chars[i:e]))
            i = e
        else:
            i += 1
    room = L - 2
    if cut and len(pieces) < room:
        return flagged, 1, "window"
    return [tokenizer.cls_id] + pieces[:room] + [tokenizer.sep_id], 0, None
