"""The collective half of sharded.exchange_plane on CPU: two processes, gloo backend, uneven token planes.  Every rank must
end with the same joined ids and offsets -- the ones rerank.join_planes makes of the two planes side by side -- and the
gated payload layout keeps the ungated one's offsets.  The device half (RerankText.concat) is tests/test_gpu_sharded_rerank.py."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from review_recommender_amd.rerank import join_planes
from review_recommender_amd.sharded import PayloadLayout, exchange_plane_arrays


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def planes():
    """Two uneven planes: 5 documents with 11 ids, then 2 documents (the first one empty) with 3 ids."""
    rng = np.random.default_rng(3)
    lens = [[4, 0, 3, 3, 1], [0, 3]]
    out = []
    for ls in lens:
        off = np.zeros(len(ls) + 1, dtype=np.int64)
        np.cumsum(ls, out=off[1:])
        tok = rng.integers(-32768, 32768, int(off[-1])).astype(np.int16)      # uint16 ids live in an int16 tensor
        out.append((torch.from_numpy(tok), torch.from_numpy(off)))
    return out


def _worker(rank, world, port, parts, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tok, off = exchange_plane_arrays(parts[rank][0], parts[rank][1], world)
        ret[rank] = (tok.numpy().copy(), off.numpy().copy(), str(tok.dtype), str(off.dtype))
    finally:
        dist.destroy_process_group()


def test_two_ranks_end_with_the_same_joined_plane():
    world, parts = 2, planes()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, free_port(), parts, ret), nprocs=world, join=True)
    want_tok = np.concatenate([parts[0][0].numpy(), parts[1][0].numpy()])
    want_off = np.array([0, 4, 4, 7, 10, 11, 11, 14], dtype=np.int64)
    for r in range(world):
        tok, off, tdt, odt = ret[r]
        assert (tdt, odt) == ("torch.int16", "torch.int64")
        assert np.array_equal(tok, want_tok) and np.array_equal(off, want_off), r


def test_join_planes_rebases_offsets_and_one_rank_is_the_identity():
    parts = planes()
    tok, off = join_planes([p[0] for p in parts], [p[1] for p in parts])
    assert off.tolist() == [0, 4, 4, 7, 10, 11, 11, 14] and tok.tolist() == parts[0][0].tolist() + parts[1][0].tolist()
    tok1, off1 = exchange_plane_arrays(parts[0][0], parts[0][1], 1)
    assert torch.equal(tok1, parts[0][0]) and torch.equal(off1, parts[0][1])
    empty = (torch.zeros(0, dtype=torch.int16), torch.zeros(1, dtype=torch.int64))      # a shard without documents
    tok2, off2 = join_planes([parts[0][0], empty[0], parts[1][0]], [parts[0][1], empty[1], parts[1][1]])
    assert torch.equal(tok2, tok) and torch.equal(off2, off)


def test_gated_payload_layout_appends_one_aligned_column():
    for B, pool in ((3, 150), (1, 37), (5, 37), (256, 150)):
        plain, gated = PayloadLayout(B, pool), PayloadLayout(B, pool, gate=True)
        for name in ("off_rows", "off_n", "off_avg", "off_l1p", "off_dense", "off_bm25"):
            assert getattr(plain, name) == getattr(gated, name)
        assert gated.off_gate == plain.nbytes and gated.off_gate % 16 == 0
        assert gated.nbytes == plain.nbytes + (B * pool * 4 + 15) // 16 * 16
        buf = torch.zeros(gated.nbytes, dtype=torch.uint8)
        v = gated.views(buf)
        v["gate"][:] = 0.25
        assert v["gate"].shape == (B, pool) and v["gate"].dtype == torch.float32 and float(v["bm25"].abs().sum()) == 0
        assert "gate" not in plain.views(torch.zeros(plain.nbytes, dtype=torch.uint8))
