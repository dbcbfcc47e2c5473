"""The vocabulary table of csrc/rr_prims.h walked in plain Python: what the device probe does, for the CPU models and the
host tests of the tables the library builds (embed.build_piece_table, querytext.build_vocab_table).

A table is `slots` [n_slots][4] int32 = hash, first byte, key, id (-1 = empty) over the bytes `blob`.  The key is what must
match besides the hash: the length in bytes (the query vocabulary), or the length | ## form << 16 (WordPiece); it defaults
to the length."""
from __future__ import annotations

from typing import Optional

import numpy as np

HASH_BASE = 0x01000193


def model_hash(token: bytes) -> int:
    h = 0
    for b in token:
        h = (h * HASH_BASE + b) & 0xFFFFFFFF
    return h


def model_slot(token: bytes, n_slots: int, key: Optional[int] = None) -> int:
    """The slot a token's walk through the table starts at."""
    key = len(token) if key is None else key
    h = model_hash(token) ^ ((key * 0x9E3779B1) & 0xFFFFFFFF)
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h & (n_slots - 1)


def table_lookup(slots: np.ndarray, blob: np.ndarray, token: bytes, key: Optional[int] = None) -> int:
    """The kernel's walk: from the token's slot to the first empty one, hash and key compared first, then the bytes."""
    key = len(token) if key is None else key
    n_slots, h = len(slots), model_hash(token)
    s = model_slot(token, n_slots, key)
    for _ in range(n_slots):
        hash_, first, key_, id_ = (int(v) for v in slots[s])
        if id_ < 0:
            return -1
        if (hash_ & 0xFFFFFFFF) == h and key_ == key and blob[first:first + len(token)].tobytes() == token:
            return id_
        s = (s + 1) & (n_slots - 1)
    return -1
