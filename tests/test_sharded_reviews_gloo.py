"""The collectives of the best-review column on row shards, on CPU: two processes, gloo backend.  `exchange_counts` sums the
(B, 256) int64 counts of a round identically on both ranks; the all-gather of the packed picks followed by select-by-owner
gives every candidate the entry of the rank that owns its row, bit for bit (a -0.0 score keeps its sign)."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from review_recommender_amd.sharded import (exchange_counts, exchange_picks, exchange_review_tops, owner_of, pack_picks,
                                            select_by_owner, shard_bounds, unpack_picks)

N_ROWS, B, POOL = 11, 3, 7          # 11 rows on 2 ranks: [0, 6) and [6, 11)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def batch():
    rng = np.random.default_rng(8)
    rows = np.stack([rng.permutation(N_ROWS)[:POOL] for _ in range(B)]).astype(np.int64)
    counts = [rng.integers(0, 2 ** 40, (B, 256)).astype(np.int64) for _ in range(2)]       # sums beyond int32
    picks = []
    for r in range(2):
        lo, hi = shard_bounds(N_ROWS, 2, r)
        own = (rows >= lo) & (rows < hi)
        raw = np.where(own, rng.standard_normal((B, POOL)), 0.0).astype(np.float32)
        ids = np.where(own, rng.integers(0, 2 ** 31 - 1, (B, POOL)), -1).astype(np.int32)
        picks.append((raw, ids, own))
    r0, c0 = np.argwhere(picks[0][2])[0]
    picks[0][0][r0, c0] = -0.0                                       # an owner's -0.0 beside the other rank's +0.0
    return rows, counts, picks


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rows, counts, picks = batch()
        c = torch.from_numpy(counts[rank].copy())
        out = exchange_counts(c, world)
        assert out is c
        raw, ids = exchange_picks(pack_picks(torch.from_numpy(picks[rank][0]), torch.from_numpy(picks[rank][1])),
                                  torch.from_numpy(rows), N_ROWS, world)
        tops = exchange_review_tops(torch.tensor([5 + rank, 3, 0], dtype=torch.int64), world)
        ret[rank] = (c.numpy().copy(), str(c.dtype), raw.numpy().copy(), ids.numpy().copy(), str(raw.dtype), str(ids.dtype), tops)
    finally:
        dist.destroy_process_group()


def test_two_ranks_sum_the_counts_and_take_every_pick_from_its_owner():
    world = 2
    rows, counts, picks = batch()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, free_port(), ret), nprocs=world, join=True)
    want_raw = np.where(picks[0][2], picks[0][0], picks[1][0])
    want_ids = np.where(picks[0][2], picks[0][1], picks[1][1])
    assert np.signbit(want_raw).sum() > np.signbit(want_raw[want_raw != 0]).sum(), "the batch holds a -0.0"
    for r in range(world):
        c, cdt, raw, ids, rdt, idt, tops = ret[r]
        assert cdt == "torch.int64" and np.array_equal(c, counts[0] + counts[1]), r
        assert (rdt, idt) == ("torch.float32", "torch.int32")
        assert np.array_equal(raw.view(np.int32), want_raw.view(np.int32)), "score BITS of the owner's entry"
        assert np.array_equal(ids, want_ids)
        assert tops.tolist() == [5, 3, 0, 6, 3, 0]


def test_packing_is_a_bijection_on_bits_and_one_rank_is_the_identity():
    raw = torch.tensor([[0.0, -0.0, 1.5, float("-inf"), -3.25e-40]], dtype=torch.float32)
    ids = torch.tensor([[-1, 0, 2 ** 31 - 1, 7, -1]], dtype=torch.int32)
    words = pack_picks(raw, ids)
    assert words.dtype == torch.int64 and words.shape == (1, 5)
    assert words[0, 2].item() == (0x3FC00000 << 32) | (2 ** 31 - 1) and words[0, 0].item() == 0xFFFFFFFF
    r2, i2 = unpack_picks(words)
    assert torch.equal(r2.view(torch.int32), raw.view(torch.int32)) and torch.equal(i2, ids)
    rows = torch.tensor([[3, 0, 10, -1, 99]])
    r1, i1 = exchange_picks(words, rows, N_ROWS, 1)
    assert torch.equal(r1.view(torch.int32), raw.view(torch.int32)) and torch.equal(i1, ids)
    c = torch.arange(512, dtype=torch.int64).view(2, 256)
    assert exchange_counts(c, 1) is c


def test_owner_follows_shard_bounds_for_every_row():
    for n, world in ((11, 2), (3000, 8), (3000, 3), (5, 8), (16, 4)):
        want = np.zeros(n, dtype=np.int64)
        for r in range(world):
            lo, hi = shard_bounds(n, world, r)
            want[lo:hi] = r
        assert np.array_equal(owner_of(torch.arange(n), n, world).numpy(), want), (n, world)
        out = owner_of(torch.tensor([-1, -5, n, n + 100]), n, world)
        assert out.min() >= 0 and out.max() < world
    g = torch.arange(2 * 6, dtype=torch.int64).view(2, 2, 3)
    rows = torch.tensor([[0, 6, 10], [5, 7, 1]])
    assert select_by_owner(g, rows, N_ROWS).tolist() == [[0, 7, 8], [3, 10, 5]]
