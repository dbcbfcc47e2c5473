"""Row-sharded search over the GPUs of one node.

One process per GPU (torch.distributed; backend "nccl" is RCCL over xGMI).  Rank r owns a
contiguous row range of the matrix, of n_reviews / avg_stars, and of the BM25 documents;
idf / avgdl are corpus-wide and replicated.  Per query batch every rank runs K1 and K2 on
its shard, packs the candidate payload

    rows int64 | n_reviews f64 | avg_stars f64 | log1p_n f64 | dense f32 | bm25 f32     (40 B/candidate)

into ONE contiguous device buffer, and a single all-gather moves all ranks' buffers to all
ranks.  K3 then reads the gathered blocks in place ([rank][query][pool] addressing),
merges world x pool candidates to the global top-pool by (dense desc, row asc) and fuses.
Every rank ends with the same result.  The global top-pool is contained in the union of
the local top-pools, and a row's score does not depend on the shard it sits in
(csrc/rr_dense.hip), so the answer equals the single-GPU answer bit for bit.

The attribute gate depends on (query, product text) only: with ``gate_groups`` every rank matches its OWN candidates against
the gate plane of its own rows (gate.GateText, 1/world of the corpus) between K2 and the all-gather, the factor rides in the
payload as one more float32 column (44 B/candidate), and K3 reads it through the merge's slot map (rr_fuse_topk_cand_dev):
one K3 pass, no host wait, no replicated texts.  The reranker scores the MERGED pool, so its token plane (about 1 KB per
product) is replicated once per index (`exchange_plane`); per batch every rank assembles and scores its share of the pairs
on the device (``rerank_pairs``).

The best review per candidate (``reviews=True``) also belongs to the MERGED pool, and its review table is sharded with the
products (reviews.ReviewIndex.shard: 1/world of the embeddings per rank).  The reference's ``iloc[:max_rows]`` cut is an
order statistic over review ids that lie on different ranks: the ranks find it together in at most four rounds of 256-way
narrowing, whose (B, 256) counts are summed by an all-reduce (`exchange_counts`); every rank then picks the best review of
the merged rows it owns, one all-gather of (score bits | id) words combines the picks (`exchange_picks`, `select_by_owner`),
and K3 runs again with the pool-aligned column.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .engine import FusionWeights, HybridSearcher, check_columns
from .index import MAX_CANDIDATES, MAX_POOL


def shard_bounds(n_rows: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous row range of ``rank``: the first n_rows % world ranks get one extra row."""
    if not (0 <= rank < world):
        raise ValueError("rank outside [0, world)")
    base, extra = divmod(n_rows, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


@dataclass(frozen=True)
class PayloadLayout:
    """Byte offsets of the candidate payload one rank contributes (all 16-B aligned)."""
    n_queries: int
    pool: int
    gate: bool = False          # a float32 column of gate factors behind bm25 (44 B/candidate instead of 40)

    @property
    def count(self) -> int:
        return self.n_queries * self.pool

    def _al(self, x: int) -> int:
        return (x + 15) // 16 * 16

    @property
    def off_rows(self) -> int: return 0
    @property
    def off_n(self) -> int: return self._al(self.count * 8)
    @property
    def off_avg(self) -> int: return self.off_n + self._al(self.count * 8)
    @property
    def off_l1p(self) -> int: return self.off_avg + self._al(self.count * 8)
    @property
    def off_dense(self) -> int: return self.off_l1p + self._al(self.count * 8)
    @property
    def off_bm25(self) -> int: return self.off_dense + self._al(self.count * 4)
    @property
    def off_gate(self) -> int: return self.off_bm25 + self._al(self.count * 4)
    @property
    def nbytes(self) -> int: return self.off_gate + (self._al(self.count * 4) if self.gate else 0)

    def views(self, buf):
        """Typed (n_queries, pool) views into one rank's uint8 buffer (torch tensor)."""
        import torch
        c, shape = self.count, (self.n_queries, self.pool)
        v = lambda off, n, dt: buf[off:off + n].view(dt).view(shape)
        out = {"rows": v(self.off_rows, c * 8, torch.int64), "n": v(self.off_n, c * 8, torch.float64),
               "avg": v(self.off_avg, c * 8, torch.float64), "l1p": v(self.off_l1p, c * 8, torch.float64),
               "dense": v(self.off_dense, c * 4, torch.float32), "bm25": v(self.off_bm25, c * 4, torch.float32)}
        if self.gate:
            out["gate"] = v(self.off_gate, c * 4, torch.float32)
        return out


class PendingExchange:
    """An all-gather that has been started (`exchange_start`): `wait()` returns the gathered (world, nbytes) tensor once
    the CURRENT stream may read it (RCCL: the collective runs on the process group's own stream; wait() makes the
    current stream wait for it without blocking the host -- kernels enqueued in between run under the collective)."""

    def __init__(self, out, work=None, finish=None):
        self.out, self.work, self._finish = out, work, finish

    def wait(self):
        if self.work is not None:
            self.work.wait()
            self.work = None
        if self._finish is not None:
            self._finish()
            self._finish = None
        return self.out


def _gather(src, world: int, group=None, out=None, start: bool = False):
    """The one all-gather of this module and its three transports: every rank contributes ``src`` (contiguous, the same shape
    and dtype on all ranks) and ends with the (world,) + src.shape tensor ``out`` (allocated beside ``src`` unless given).
    ``start``: returns the started PendingExchange instead of waiting for it."""
    import torch
    import torch.distributed as dist
    if out is None:
        out = torch.empty((world,) + tuple(src.shape), dtype=src.dtype, device=src.device)
    if world == 1:
        out[0].copy_(src)
        pend = PendingExchange(out)
    elif dist.get_backend(group) == "nccl":                       # RCCL over xGMI
        pend = PendingExchange(out, dist.all_gather_into_tensor(out, src, group=group, async_op=True))
    elif src.is_cuda:                                             # gloo rehearsal on a GPU box: gloo gathers host tensors
        host = torch.empty(out.shape, dtype=src.dtype)
        work = dist.all_gather([host[r] for r in range(world)], src.cpu(), group=group, async_op=True)
        pend = PendingExchange(out, work, lambda: out.copy_(host))
    else:                                                         # gloo (CPU tests)
        pend = PendingExchange(out, dist.all_gather([out[r] for r in range(world)], src, group=group, async_op=True))
    return pend if start else pend.wait()


def exchange_start(buf, world: int, group=None, out=None) -> PendingExchange:
    """Starts the path's one collective (all-gather of every rank's payload buffer) without waiting for it: what lets
    batch i's exchange run under K1 of batch i + 1 (ShardedSearcher.submit / finish).  ``out``: a caller-owned
    (world, nbytes) uint8 buffer to gather into."""
    return _gather(buf, world, group, out, start=True)


def exchange(buf, world: int, group=None):
    """The path's one collective: all-gather of every rank's payload buffer.
    Returns a (world, nbytes) uint8 tensor, identical on every rank."""
    return exchange_start(buf, world, group).wait()


def exchange_floor_start(bound, world: int, group=None):
    """exchange_floor without waiting for it (RCCL): returns the work handle whose wait() orders the CURRENT stream behind
    the all-reduce, or None when it has already happened (one rank, gloo)."""
    import torch.distributed as dist
    if world == 1:
        return None
    if dist.get_backend(group) == "nccl":
        return dist.all_reduce(bound, op=dist.ReduceOp.MIN, group=group, async_op=True)
    host = bound.cpu()                                            # gloo reduces host tensors (a CPU tensor is its own copy)
    dist.all_reduce(host, op=dist.ReduceOp.MIN, group=group)
    if host is not bound:                                         # gloo rehearsal on a GPU box
        bound.copy_(host)
    return None


def exchange_floor(bound, world: int, group=None):
    """The tiny collective in front of the shards' selection: element-wise MINIMUM over the ranks
    of the per-query bounds of HybridSearcher.dense_scan -- a lower bound of the corpus-wide pool-th best score.
    In place; B floats."""
    work = exchange_floor_start(bound, world, group)
    if work is not None:
        work.wait()
    return bound


def floor_kth(pool_local: int, world: int) -> int:
    """The rank of the row whose score a shard reports as its bound for the floor.  The shards' kth best rows together hold
    >= pool rows for any kth >= ceil(pool / world).  A shard is only sure of ~8 kth rescored rows (kth opened 8-row M-tiles):
    with kth >= ceil(pool / 8) + 1 its own list of `pool` rows fills without the exact fallback also at world >= 8
    (ceil(150 / 8) = 19 M-tiles = 152 rows would just do)."""
    return min(max((pool_local + world - 1) // world, (pool_local + 7) // 8 + 1), pool_local)


def split_pairs(n_pairs: int, world: int, rank: int) -> Tuple[int, int]:
    """Even split of the flattened (query, candidate) pair list of the rerank step across ranks
    ("pairs B x 200 are split evenly across ranks after the merge"): the same rule as shard_bounds."""
    return shard_bounds(n_pairs, world, rank)


def exchange_scores(local, n_pairs: int, world: int, group=None):
    """The second, tiny all-gather of the rerank flow (only when rerank_k > 0): every rank contributes the
    reranker scores of its share of the pairs (float32 tensor of split_pairs' length); returns the full
    (n_pairs,) tensor, identical on every rank."""
    import torch
    if world == 1:
        return local
    share = (n_pairs + world - 1) // world                     # shares differ by at most one pair: pad to the longest
    buf = torch.zeros(share, dtype=torch.float32, device=local.device)
    buf[:local.numel()] = local
    out = _gather(buf, world, group)
    bounds = [split_pairs(n_pairs, world, r) for r in range(world)]
    return torch.cat([out[r, :hi - lo] for r, (lo, hi) in enumerate(bounds)])


def exchange_counts(counts, world: int, group=None):
    """The collective of one round of the review cut (reviews.model_cut): element-wise SUM over the ranks of the (B, 256)
    int64 counts, in place.  Integer sums: the same on every rank whatever order the transport adds in."""
    import torch.distributed as dist
    if world == 1:
        return counts
    if dist.get_backend(group) == "nccl":
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group, async_op=True).wait()    # (orders the stream, not the host)
        return counts
    host = counts.cpu()                                           # gloo reduces host tensors (a CPU tensor is its own copy)
    dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
    if host is not counts:
        counts.copy_(host)
    return counts


def owner_of(rows, n_rows: int, world: int):
    """The rank whose shard holds each row of ``rows`` (int64 tensor of global rows) under `shard_bounds`; rows outside the
    corpus are given to the nearest rank (none owns them: its pick for them is "no review")."""
    base, extra = divmod(n_rows, world)
    head = extra * (base + 1)                                     # rows of the ranks that hold one row more
    own = rows.div(base + 1, rounding_mode="floor")
    if base > 0:
        own = own.where(rows < head, (rows - head).div(base, rounding_mode="floor") + extra)
    return own.clamp_(0, world - 1)


def pack_picks(best_raw, best_ids):
    """(score float32, review id int32) per candidate as ONE int64 word: score bits << 32 | id.  Bits, not values: the
    ranks' columns are never added (-0.0 + 0.0 would change a score's bit pattern)."""
    import torch
    return torch.stack([best_ids, best_raw.view(torch.int32)], dim=-1).view(torch.int64).squeeze(-1)


def unpack_picks(words):
    """The inverse of pack_picks: (best_raw float32, best_ids int32), contiguous."""
    import torch
    pair = words.contiguous().view(torch.int32).view(tuple(words.shape) + (2,))
    return pair[..., 1].contiguous().view(torch.float32), pair[..., 0].contiguous()


def select_by_owner(gathered, rows, n_rows: int):
    """``gathered``: (world, B, pool) int64 picks of every rank for the same merged ``rows`` (B, pool); returns (B, pool):
    every candidate's word from the rank that OWNS its row."""
    world = gathered.shape[0]
    own = owner_of(rows, n_rows, world)
    return gathered.view(world, -1).gather(0, own.view(1, -1)).view(rows.shape)


def exchange_picks(words, rows, n_rows: int, world: int, group=None):
    """The all-gather of the best-review step: every rank contributes its (B, pool) int64 picks (pack_picks) of the merged
    rows; returns (best_raw, best_ids) with every candidate's entry taken from its owner rank, identical on every rank."""
    return unpack_picks(select_by_owner(_gather(words, world, group), rows, n_rows))


def exchange_review_tops(top, world: int, group=None):
    """Once per index: every rank contributes the largest per-product review counts of its shard (ReviewIndex.top_counts,
    int64); returns all ranks' counts in one numpy array, replicated -- the numbers the skip rule of the cut's rounds is
    decided from on the host (reviews.pool_reviews_bound)."""
    return _gather(top, world, group).cpu().numpy().reshape(-1)


def exchange_plane_arrays(tok, off, world: int, group=None):
    """The collective half of `exchange_plane`: every rank contributes the ids (int16, its n_tokens) and the offsets (int64
    [n + 1]) of its shard's token plane; all ranks end with the same joined (ids, offsets) of the whole corpus
    (rerank.join_planes).  Three all-gathers: the sizes, then the id and the offset tensors padded to the longest."""
    import torch
    from .rerank import join_planes
    if world == 1:
        return join_planes([tok], [off])
    sizes = _gather(torch.tensor([int(tok.numel()), int(off.numel())], dtype=torch.int64, device=tok.device),
                        world, group).cpu().tolist()
    n_tok, n_off = max(s[0] for s in sizes), max(s[1] for s in sizes)
    tok_pad = torch.zeros(max(n_tok, 1), dtype=tok.dtype, device=tok.device)
    tok_pad[:tok.numel()] = tok
    off_pad = torch.zeros(n_off, dtype=torch.int64, device=off.device)
    off_pad[:off.numel()] = off
    # (the ids travel as bytes: gloo has no 16-bit integers)
    toks, offs = _gather(tok_pad.view(torch.uint8), world, group).view(tok.dtype), _gather(off_pad, world, group)
    return join_planes([toks[r, :sizes[r][0]] for r in range(world)], [offs[r, :sizes[r][1]] for r in range(world)])


def exchange_plane(local, world: int, group=None):
    """Replicates the reranker's token plane: ``local`` is this rank's rerank.RerankText over its own rows; returns the plane
    of the whole corpus (row_offset 0: rank 0's), identical on every rank.  A collective, once per index, not per batch: about
    1 KB per product crosses the wire, where the gate plane (6 KB per product) stays sharded."""
    from .rerank import RerankText
    if world == 1:
        return local
    tok, off = exchange_plane_arrays(local.d_tok[:local.n_tokens], local.d_off, world, group)
    whole = RerankText.from_arrays(tok, off, local)
    whole.row_offset = 0                # (shard_bounds: rank 0's rows begin at 0)
    return whole


@dataclass
class PendingBatch:
    """What ShardedSearcher.submit leaves for finish: the batch's parameters, its payload and the started all-gather."""
    B: int
    k: int
    pool: int
    pool_local: int
    rr_k: int
    w: FusionWeights
    lay: "PayloadLayout"
    buf: object
    pending: "PendingExchange"
    gate_fn: object = None
    rerank_fn: object = None
    packed: object = None         # gate_groups: the batch's gate.PackedGroups (the payload then carries the gate column),
    gate_host: object = None      # the host function of its over-limit queries,
    staged: object = None         # and the packed groups on the device (overlapped form: uploaded at submit, ahead of K1)
    rerank_pairs: object = None   # (cross_encoder, rerank.PackedQueries, rerank_host)
    # the overlapped form (ShardedSearcher.enable_overlap): stage 0 = scanned (K1's scan on the scans' stream, the floor's
    # all-reduce started), 1 = payload built and its all-gather started, 2 = finished
    stage: int = 1
    slot: int = -1
    bound: object = None
    floor_work: object = None
    terms: object = None
    bm25_mode: str = "forward"
    plain_q: object = None        # set when K1 could not be split on this rank: the queries of the whole K1 stage 1 then runs
    two_pass: bool = False        # a host gate, a reranker or reviews: finish merges, forms the pool-aligned columns, runs K3 again
    reviews: object = None        # (queries, max_scan, best_out) of a batch with the best-review column


class _Overlap:
    """Streams and ring buffers of the overlapped shard step: scans on a stream masked to the first ``scan_cus`` CUs, every
    batch's tail (selection against the floor, K2, metadata gather, payload all-gather, merge + K3) on a stream masked to the
    rest, three batches deep (include/rr_hip.h: scan slots)."""
    SLOTS = 3

    def __init__(self, searcher: HybridSearcher, scan_cus: int):
        import torch
        lib, dev = searcher.lib, searcher.device
        total = torch.cuda.get_device_properties(dev).multi_processor_count
        if not (0 < scan_cus < total) or scan_cus % 32 or (total - scan_cus) % 32:
            # the dispatcher deals one-per-CU workgroups to the 32 shader engines in turn: a share that is not a multiple of
            # 32 leaves engines with CUs that get two of them (measured: 240 CUs take twice the time of 224)
            raise ValueError(f"scan_cus {scan_cus} must be a multiple of 32 inside (0, {total})")
        self.scan_cus, self.handles = scan_cus, []
        streams = []
        for first, n in ((0, scan_cus), (scan_cus, total - scan_cus)):
            h = C.c_void_p()
            _lib.check(lib.rr_stream_create_cu_range(dev.index, first, n, C.byref(h)), "rr_stream_create_cu_range")
            self.handles.append(h)
            streams.append(torch.cuda.ExternalStream(h.value, device=dev))
        self.scan_stream, self.tail_stream = streams
        _lib.check(lib.rr_index_set_scan_cus(searcher.index.handle, scan_cus), "rr_index_set_scan_cus")
        self.lib, self.index = lib, searcher.index
        self.seq = 0
        self.pending = None            # the ticket whose payload has not been built yet (stage 0)
        self.unfinished = 0
        self.rings = {}                # (B, pool_local, pool, k, world) -> per-slot buffers

    def buffers(self, key, make):
        if key not in self.rings:
            self.rings[key] = [make() for _ in range(self.SLOTS)]
        return self.rings[key]

    def close(self):
        import torch
        torch.cuda.synchronize()
        if self.index.handle:
            _lib.check(self.lib.rr_index_set_scan_cus(self.index.handle, 0), "rr_index_set_scan_cus")
        for h in self.handles:
            _lib.check(self.lib.rr_stream_destroy(h), "rr_stream_destroy")
        self.handles = []


class ShardedSearcher:
    """K1 + K2 per shard, one all-gather, K3 on the merged pool."""

    def __init__(self, searcher: HybridSearcher, n_total_rows: int, rank: int, world: int, group=None, rerank_text=None,
                 reviews=None):
        """``searcher.gate_text``: the gate plane of THIS shard's rows (``GateText.from_texts(texts[lo:hi], ...,
        row_offset=lo)``), for ``gate_groups``.  ``rerank_text``: the token plane of the WHOLE corpus (`exchange_plane` of
        the shards' planes), for ``rerank_pairs``; one rank takes its searcher's.  ``reviews``: the review index of THIS
        shard's rows (``ReviewIndex.shard(..., lo, hi)``; one rank may pass a whole index), for ``reviews=True``.  With more
        than one rank the constructor then runs one collective (`exchange_review_tops`) when a process group is up; a test
        that plays the shards in one process sets ``review_tops`` itself."""
        lo, hi = shard_bounds(n_total_rows, world, rank)
        ix = searcher.index
        if ix.row_offset != lo or ix.n_rows != hi - lo:
            raise ValueError(f"rank {rank} must hold rows [{lo}, {hi}); its index holds "
                             f"[{ix.row_offset}, {ix.row_offset + ix.n_rows})")
        self.s, self.rank, self.world, self.group, self.n_total = searcher, rank, world, group, n_total_rows
        self.rerank_text = rerank_text if rerank_text is not None else (searcher.rerank_text if world == 1 else None)
        # diagnostic: run the payload + exchange + merge path even with one rank (bench.py --force-payload)
        self.force_payload = False
        # row shards select against a corpus-wide floor (two-phase K1 + exchange_floor); RR_NO_SHARD_FLOOR=1: every shard
        # selects on its own threshold (one collective less, ~8x the rescoring at 8 shards)
        self.use_floor = os.environ.get("RR_NO_SHARD_FLOOR") is None
        self._ov: Optional[_Overlap] = None
        self.reviews = reviews
        self.review_tops = None         # the ranks' largest per-product review counts (numpy, replicated): the skip rule's input
        self.review_rounds_run = 0      # rounds of the cut this searcher has launched (tests, tools)
        if reviews is not None:
            import torch
            import torch.distributed as dist
            if (reviews.row_lo, reviews.row_hi) != (lo, hi):
                raise ValueError(f"rank {rank} holds rows [{lo}, {hi}); its review index is over rows "
                                 f"[{reviews.row_lo}, {reviews.row_hi})")
            top = torch.from_numpy(reviews.top_counts(MAX_POOL))
            if world == 1:
                self.review_tops = top.numpy()
            elif dist.is_available() and dist.is_initialized():
                self.review_tops = exchange_review_tops(top if dist.get_backend(group) != "nccl" else top.to(searcher.device),
                                                        world, group)

    def enable_overlap(self, scan_cus: Optional[int] = None) -> bool:
        """Runs every batch's tail beside the NEXT batch's scan ("keep K1 -> K2-gather -> allgather -> K3 on-stream
        ... pipeline batches"): the scans get a stream masked to ``scan_cus`` CUs (a multiple of 32), the tails one masked to
        the rest (rr_stream_create_cu_range), and submit / finish become a three-stage pipeline -- scan(i + 1) | payload(i) |
        merge(i - 1).  Answers are bit for bit those of the straight path (tests/test_gpu_sharded.py).
        The masked streams are blocking HIP streams: a caller that enqueues its own commands on the NULL stream (torch's
        default stream) makes every one of them a barrier across both -- run the calling loop on a stream of its own
        (``torch.cuda.set_stream(torch.cuda.Stream())``, as bench.py does).
        ``scan_cus`` None: ON for real row shards (world > 1) with the split the full-step proxy measured best on MI355X
        (tools/shard_step_proxy.py, profiles/r04_overlap_ab.md: per rank-step without the collectives' wire) --
            <= 1.5M rows per shard (8 GPUs at 10M): 128 | 128 CUs   0.433 -> 0.350 ms
            <= 3M   rows           (4 GPUs)       : 160 |  96       0.663 -> 0.584 ms
            <= 6M   rows           (2 GPUs)       : 192 |  64       1.131 -> 1.016 ms
        and OFF for one rank / larger shards (10M rows on one GPU lose: the tail needs the CUs there and whatever runs beside
        the scan slows it).  RR_TAIL_OVERLAP_CUS=n forces a split (also with one rank), RR_NO_TAIL_OVERLAP=1 turns it off.
        Returns whether the overlap is on."""
        if self._ov is not None:
            return True
        if os.environ.get("RR_NO_TAIL_OVERLAP") is not None:
            return False
        forced = os.environ.get("RR_TAIL_OVERLAP_CUS")
        if scan_cus is None and forced:
            scan_cus = int(forced)
        if scan_cus is None and self.world > 1:
            n = self.s.index.n_rows
            scan_cus = 128 if n <= 1_500_000 else 160 if n <= 3_000_000 else 192 if n <= 6_000_000 else None
        if scan_cus is None:
            return False
        self._ov = _Overlap(self.s, scan_cus)
        return True

    def disable_overlap(self) -> None:
        if self._ov is not None:
            self._flush_overlap()
            self._ov.close()
            self._ov = None

    def local_scan(self, q_dev, pool_local: int):
        """Phase 1 of K1 on this rank: the scan and this shard's bound per query (None: the call cannot be split)."""
        self._flush_overlap()
        return self.s.dense_scan(q_dev, pool_local, floor_kth(pool_local, self.world))

    def local_payload(self, q_dev, term_id_lists, pool_local: int, bm25_mode: str = "forward", floor=None, buf=None,
                      gate=None, gate_host=None):
        """K1 (+ the floor exchange when there is more than one shard) + K2 + metadata gather into the payload buffer of
        this rank.  ``floor``: tests that play several shards in one process pass the minimum they formed themselves
        (after calling local_scan on every shard); ``False`` = plain K1.
        ``gate``: the batch's gate.PackedGroups -- the layout then has the gate column, and behind K2, on the same stream,
        this rank's candidates are matched against the gate plane of its own rows into it (every candidate of a shard's
        list, fill entries included, is a row of the shard: DESIGN.md section 5).  The packed terms are uploaded ahead of K1.
        ``gate_host(b, rows)``: for the queries of ``gate.host_queries``, on this rank's own rows."""
        import torch
        self._flush_overlap()
        s = self.s
        B = q_dev.shape[0]
        if gate is not None and s.gate_text is None:
            raise ValueError("gate groups need the gate plane of this shard's rows: HybridSearcher(..., gate_text=GateText...)")
        lay = PayloadLayout(B, pool_local, gate=gate is not None)
        if buf is None:                 # (``buf``: a caller-owned uint8 buffer of lay.nbytes to build the payload in)
            buf = torch.empty(lay.nbytes, dtype=torch.uint8, device=s.device)
        v = lay.views(buf)
        staged = s.gate_text.upload(gate) if gate is not None else None
        import torch.distributed as dist
        if floor is None and self.world > 1 and self.use_floor and dist.is_available() and dist.is_initialized():
            bound = self.local_scan(q_dev, pool_local)
            # every rank takes the same branch: whether a call can be split depends on the batch and on the shard sizes
            # only through properties all shards share (n_queries, pool; a shard too small for the filter path reports
            # -inf bounds instead) -- a rank that could not split contributes -inf, i.e. no floor at all
            mine = bound if bound is not None else torch.full((B,), float("-inf"), dtype=torch.float32, device=s.device)
            floor = exchange_floor(mine, self.world, self.group)
            if bound is None:
                floor = False
        if floor is None or floor is False:
            s.dense_pool(q_dev, pool_local, out=(v["rows"], v["dense"]))   # K1 writes the payload in place
        else:
            s.dense_select(q_dev, pool_local, floor, out=(v["rows"], v["dense"]))
        self._payload_tail(v, term_id_lists, bm25_mode, gate, gate_host, staged)
        return lay, buf

    def _payload_tail(self, v, terms, bm25_mode: str, packed, gate_host, staged) -> None:
        """Behind K1, on the current stream, into the payload views ``v``: K2 at the candidate rows, the gate match of this
        rank's own candidates against its own plane when the batch has packed groups, and the metadata gather."""
        s = self.s
        s.bm25_at(terms, v["rows"], bm25_mode, out=v["bm25"])          # K2 writes the payload in place too
        if packed is not None:
            s.gate_text.gate(v["rows"], packed, gate_host, staged, out=v["gate"])
        _lib.check(s.lib.rr_index_gather_meta_dev(
            s.index.handle, C.c_void_p(v["rows"].data_ptr()), v["rows"].numel(),
            C.c_void_p(v["n"].data_ptr()), C.c_void_p(v["avg"].data_ptr()),
            C.c_void_p(v["l1p"].data_ptr()), s._stream()), "rr_index_gather_meta_dev")

    def search_batch_dev(self, q_dev, term_id_lists: Optional[Sequence[Sequence[int]]], k: int,
                         weights: Optional[FusionWeights] = None, pool_floor: int = 150,
                         bm25_mode: str = "forward", rerank_k: int = 0, gate_fn=None, rerank_fn=None,
                         gate_groups=None, gate_host=None, rerank_pairs=None, reviews: bool = False, max_scan: int = 0,
                         best_out: Optional[dict] = None):
        """Device-resident queries in, device tensors out: (pool_rows, columns, order).

        ``reviews`` / ``max_scan`` (names and meaning of HybridSearcher.search_batch, with the searcher's own shard index):
        the `_best` column -- per candidate of the merged pool the best review among the first ``max_scan`` reviews, in file
        order, of all the pool's candidates.  ``best_out``: a dict that receives ``"best_ids"`` (B, pool) int32 GLOBAL review
        ids (-1: none) and ``"best_raw"`` (B, pool) float32, device tensors aligned with pool_rows (what
        ``ReviewIndex.snippets`` takes).  A two-pass batch: the merge, the cut's rounds across the ranks (skipped when no
        pool of this size can hold more than ``max_scan`` reviews), every rank's picks for the rows it owns, one all-gather
        of them, K3 again.

        ``gate_groups`` / ``gate_host`` (instead of gate_fn; names and meaning of HybridSearcher.search_batch): per query
        its gate groups, matched on the device against the gate plane of this rank's OWN rows before the exchange; the
        factor travels in the payload and K3 runs once (rr_fuse_topk_cand_dev).  ``gate_host(b, rows)`` is called for the
        queries over the match kernel's limits only, with this rank's own candidate rows of query b.
        ``rerank_pairs`` = ``(cross_encoder, packed_queries, rerank_host)`` (instead of rerank_fn): after the merge pass every
        rank assembles and scores its share of the B x rr_k pairs on the device against the replicated token plane
        (``self.rerank_text``), the scores are all-gathered and K3 runs again with them.  ``rerank_host(b, rows)`` is called
        for the queries of ``packed_queries.host_queries`` only, with the rows of this rank's share of query b's pairs, and
        returns one score per row.

        ``gate_fn(rows (B, pool) global rows, numpy) -> (B, pool) float32`` and
        ``rerank_fn(query_idx (n,), rows (n,)) -> (n,) float32`` (scores of the (query, product) pairs given) are
        host callables over the MERGED pool (app/app_product_search.py:271-303): the shards' candidates are
        merged first (K3 with k = pool gives the pool order), gate strings are matched on the host, the
        B x rr_k reranker pairs are split evenly across the ranks, their scores gathered with a second tiny
        all-gather, and K3 runs again on the same gathered payload with the pool-aligned columns."""
        s = self.s
        if self.world == 1 and not self.force_payload:
            # nothing to exchange: K1 -> K2 -> gate -> K3 straight through, metadata read from the index
            B, w, pool, _, rr_k, tl, packed, two_pass = self._plan(q_dev, term_id_lists, k, weights, pool_floor, rerank_k,
                                                                   gate_fn, rerank_fn, gate_groups, gate_host, rerank_pairs,
                                                                   reviews)
            self._flush_overlap()
            staged = s.gate_text.upload(packed) if packed is not None else None      # (ahead of the kernels)
            rows, dense = s.dense_pool(q_dev, pool)
            bm = s.bm25_at(tl, rows, bm25_mode)
            gate = rerank = best = None
            if reviews:                     # one GPU sees every list: the cut by bisection and the pick, one call
                best = self._best_whole(q_dev, rows, max_scan, best_out)
            if gate_fn is not None or ((rerank_fn is not None or rerank_pairs is not None) and rr_k > 0):
                gate, rerank = self._pool_columns(rows, B, pool, rr_k, gate_fn, rerank_fn, rerank_pairs)
            if packed is not None:
                gate = s.gate_text.gate(rows, packed, gate_host, staged)      # pool-aligned: the pool order is K1's already
            return s.fuse(HybridSearcher.make_params(w, min(k, pool), pool, pool, rr_k), B, rows, dense, bm,
                          None, rerank, best, gate)
        return self.finish(self.submit(q_dev, term_id_lists, k, weights, pool_floor, bm25_mode, rerank_k, gate_fn, rerank_fn,
                                       gate_groups, gate_host, rerank_pairs, reviews, max_scan, best_out))

    def submit(self, q_dev, term_id_lists, k: int, weights: Optional[FusionWeights] = None, pool_floor: int = 150,
               bm25_mode: str = "forward", rerank_k: int = 0, gate_fn=None, rerank_fn=None,
               gate_groups=None, gate_host=None, rerank_pairs=None, reviews: bool = False, max_scan: int = 0,
               best_out: Optional[dict] = None) -> "PendingBatch":
        """First half of search_batch_dev for row shards: K1 (+ floor exchange) + K2 + metadata gather on this rank, then the
        payload all-gather is STARTED (exchange_start) and the call returns.  `finish(ticket)` waits for the collective on
        the stream and runs the merge (K3).  Calling submit(batch i + 1) before finish(batch i) puts batch i's all-gather
        under batch i + 1's K1 ("pipeline batches so the all-gather of batch i overlaps K1 of batch i+1"):

            t = s.submit(q[0], ...)
            for i in range(1, n):
                t_next = s.submit(q[i], ...)
                res[i - 1] = s.finish(t)
                t = t_next
            res[n - 1] = s.finish(t)

        Every answer is bit for bit the one search_batch_dev gives (same kernels, same order per batch)."""
        B, w, pool, pool_local, rr_k, tl, packed, two_pass = self._plan(
            q_dev, term_id_lists, k, weights, pool_floor, rerank_k, gate_fn, rerank_fn, gate_groups, gate_host, rerank_pairs,
            reviews)
        if self._ov is not None:
            if not two_pass:
                t = self._submit_overlapped(q_dev, tl, B, k, pool, pool_local, w, bm25_mode, packed, gate_host)
                if t is not None:
                    return t
            self._flush_overlap()      # a batch the pipeline does not take (host columns, a call K1 cannot split): in order, behind it
        lay, buf = self.local_payload(q_dev, tl, pool_local, bm25_mode, gate=packed, gate_host=gate_host)
        pending = exchange_start(buf, self.world, self.group)
        return PendingBatch(B, k, pool, pool_local, rr_k, w, lay, buf, pending, gate_fn, rerank_fn, packed=packed,
                            gate_host=gate_host, rerank_pairs=rerank_pairs, two_pass=two_pass,
                            reviews=(q_dev, int(max_scan), best_out) if reviews else None)

    def _plan(self, q_dev, term_id_lists, k: int, weights, pool_floor: int, rerank_k: int, gate_fn, rerank_fn,
              gate_groups, gate_host, rerank_pairs, reviews: bool = False):
        """The batch's plan, with every check that can refuse it, before any launch or collective (every rank computes the
        same tests on the same batch, so no rank is left waiting in a collective the others never join):
        (B, weights, pool, pool_local, rr_k, term lists, the gate's PackedGroups or None, two_pass).  ``two_pass``: a host
        gate, a reranker or the best-review column needs the merged pool first (merge, pool-aligned columns, K3 again); a
        gate matched on the device is a payload column, such a batch is an ordinary one-pass batch."""
        w = weights or FusionWeights()
        B = q_dev.shape[0]
        pool = min(max(k, rerank_k, pool_floor), self.n_total)
        if self.world * pool > MAX_CANDIDATES:      # K3 merges world x pool candidates per query (include/rr_hip.h: RR_MAX_CANDIDATES)
            raise ValueError(f"{self.world} shards x pool {pool} = {self.world * pool} candidates per query exceed "
                             f"the merge limit of {MAX_CANDIDATES}: the pool may be at most "
                             f"{MAX_CANDIDATES // self.world} with {self.world} shards")
        pool_local = min(pool, self.s.index.n_rows)
        rr_k = min(rerank_k, pool)
        if self.world > 1:
            # every rank must contribute the same count for the strided addressing
            assert pool_local == pool, "each shard needs at least `pool` rows"
        tl = term_id_lists if term_id_lists is not None else [[] for _ in range(B)]
        packed = check_columns(B, w, self.s.gate_text, self.rerank_text, gate_fn, gate_groups, gate_host, rerank_fn, rerank_pairs)
        if reviews:
            if self.reviews is None:
                raise ValueError("reviews=True needs the review index of this shard's rows: ShardedSearcher(..., "
                                 "reviews=ReviewIndex.shard(...))")
            lo, hi = shard_bounds(self.n_total, self.world, self.rank)
            if (self.reviews.row_lo, self.reviews.row_hi) != (lo, hi):
                raise ValueError(f"the review index is over rows [{self.reviews.row_lo}, {self.reviews.row_hi}), "
                                 f"not this rank's [{lo}, {hi})")
            if self.review_tops is None:
                raise ValueError("the ranks' review counts have not been exchanged (review_tops): construct the searcher "
                                 "with the process group up")
        two_pass = gate_fn is not None or ((rerank_fn is not None or rerank_pairs is not None) and rr_k > 0) or bool(reviews)
        return B, w, pool, pool_local, rr_k, tl, packed, two_pass

    # ------------------------------------------------------------------ the overlapped form
    def _flush_overlap(self) -> None:
        """Builds the payload of the ticket still at stage 0 (its scan is parked in a slot: a plain K1 call would void it)."""
        ov = self._ov
        if ov is not None and ov.pending is not None:
            t, ov.pending = ov.pending, None
            self._build_payload(t)

    def _submit_overlapped(self, q_dev, tl, B, k, pool, pool_local, w, bm25_mode, packed=None, gate_host=None):
        import torch
        import torch.distributed as dist
        ov, s = self._ov, self.s
        if ov.unfinished > 2:
            raise RuntimeError("the overlapped pipeline is three batches deep: finish() earlier tickets before submitting more")
        slot = ov.seq % ov.SLOTS
        with_floor = self.world > 1 and self.use_floor and dist.is_available() and dist.is_initialized()
        kth = floor_kth(pool_local, self.world) if with_floor else 0
        cur = torch.cuda.current_stream(s.device)
        staged = s.gate_text.upload(packed) if packed is not None else None     # (ahead of K1; the copy has finished on return)
        ready = torch.cuda.Event()
        ready.record(cur)                                   # (the caller's stream produced q_dev)
        with torch.cuda.stream(ov.scan_stream):
            ov.scan_stream.wait_event(ready)
            bound_ring = ov.buffers(("bound", B), lambda: torch.empty((B,), dtype=torch.float32, device=s.device))
            bound = s.dense_scan_slot(slot, q_dev, pool_local, kth, bound_out=bound_ring[slot])
            plain_q = None
            if bound is None:
                if not with_floor:
                    return None                             # (no floor exchange to keep in step: the caller's plain path)
                # Row shards: whether K1 can be split may depend on THIS rank's rows (no finite row-norm bound: NaN / inf rows;
                # a shard a few rows short of the filter path).  The ranks' collectives must stay in the same order, so this
                # rank stays in the pipeline: it contributes "no floor" (-inf) to the all-reduce, and its stage 1 runs the
                # whole K1 in its slot instead of the selection.
                bound = bound_ring[slot]
                bound.fill_(float("-inf"))
                plain_q = q_dev
            work = exchange_floor_start(bound, self.world, self.group) if with_floor else None
        ov.seq += 1
        ov.unfinished += 1
        lay = PayloadLayout(B, pool_local, gate=packed is not None)
        t = PendingBatch(B, k, pool, pool_local, 0, w, lay, None, None, stage=0, slot=slot,
                         bound=bound if with_floor else None, floor_work=work, terms=tl, bm25_mode=bm25_mode, plain_q=plain_q,
                         packed=packed, gate_host=gate_host, staged=staged)
        prev, ov.pending = ov.pending, t
        if prev is not None:
            self._build_payload(prev)                       # batch i - 1's tail goes to its stream beside this scan
        return t

    def _build_payload(self, t: "PendingBatch") -> None:
        """Stage 1 on the tails' stream: selection (against the exchanged floor), K2, metadata gather into the slot's payload
        buffer, and the all-gather is started."""
        import torch
        ov, s = self._ov, self.s
        B, pool_local, lay = t.B, t.pool_local, t.lay
        ring = ov.buffers(("payload", lay.nbytes, self.world), lambda: (
            torch.empty(lay.nbytes, dtype=torch.uint8, device=s.device),
            torch.empty((self.world, lay.nbytes), dtype=torch.uint8, device=s.device)))
        buf, gathered = ring[t.slot]
        v = lay.views(buf)
        with torch.cuda.stream(ov.tail_stream):
            if t.floor_work is not None:
                t.floor_work.wait()                         # (orders this stream behind the all-reduce, not the host)
            if t.plain_q is not None:
                s.dense_pool(t.plain_q, pool_local, out=(v["rows"], v["dense"]), slot=t.slot)
            else:
                s.dense_select_slot(t.slot, B, pool_local, floor=t.bound, out=(v["rows"], v["dense"]))
            self._payload_tail(v, t.terms, t.bm25_mode, t.packed, t.gate_host, t.staged)
            t.pending = exchange_start(buf, self.world, self.group, out=gathered)
        t.buf, t.stage, t.terms, t.plain_q = buf, 1, None, None

    def _finish_overlapped(self, t: "PendingBatch"):
        import torch
        ov, s = self._ov, self.s
        if t.stage == 0:
            if ov.pending is t:
                ov.pending = None
            self._build_payload(t)
        B, k, pool, pool_local, w, lay = t.B, t.k, t.pool, t.pool_local, t.w, t.lay
        k_out = min(k, pool)
        out_rows, cols, order = ov.buffers(("out", B, pool, k_out), lambda: (
            torch.empty((B, pool), dtype=torch.int64, device=s.device),
            torch.empty((B, 8, pool), dtype=torch.float64, device=s.device),
            torch.empty((B, k_out), dtype=torch.int32, device=s.device)))[t.slot]
        cur = torch.cuda.current_stream(s.device)
        with torch.cuda.stream(ov.tail_stream):
            self.merge(lay, t.pending.wait(), B, k_out, pool, pool_local, w, out=(out_rows, cols, order))
            done = torch.cuda.Event()
            done.record(ov.tail_stream)
        cur.wait_event(done)                                # the caller's stream may read the answer
        t.stage, t.staged = 2, None
        ov.unfinished -= 1
        # (the answer lives in the slot's ring buffers: valid until three more batches have been submitted)
        return out_rows, cols, order

    def finish(self, t: "PendingBatch"):
        """Second half: the gathered payload is merged and fused (K3, with the payload's gate column when the batch has one;
        with a host gate or a reranker: merge, pool-aligned columns, K3 again)."""
        if t.slot >= 0:
            return self._finish_overlapped(t)
        B, pool, pool_local, rr_k, w, lay = t.B, t.pool, t.pool_local, t.rr_k, t.w, t.lay
        k_out = min(t.k, pool)
        gathered = t.pending.wait()
        if not t.two_pass:
            res = self.merge(lay, gathered, B, k_out, pool, pool_local, w)
        else:
            # pass A: the merge alone fixes the pool order; pass B: the same payload + the pool-aligned columns
            merged_rows, _, _ = self.merge(lay, gathered, B, pool, pool, pool_local, w)
            gate, rerank = self._pool_columns(merged_rows, B, pool, rr_k, t.gate_fn, t.rerank_fn, t.rerank_pairs)
            best = self.best_column(*t.reviews[:2], merged_rows, t.reviews[2]) if t.reviews is not None else None
            res = self.merge(lay, gathered, B, k_out, pool, pool_local, w, rr_k, rerank, gate, best=best)
        self._keep = (gathered, t.buf)   # alive until the stream has consumed them
        return res

    def merge(self, lay: PayloadLayout, gathered, B: int, k_out: int, pool: int, pool_local: int, w: FusionWeights,
              rr_k: int = 0, rerank=None, gate=None, out=None, best=None):
        """K3 over a gathered payload, on the current stream: ``gathered`` holds ``self.world`` blocks of layout ``lay``
        ([rank][query][pool_local] addressing); they are merged to the top ``pool`` by (dense desc, row asc) and fused ->
        (out_rows (B, pool), cols (B, 8, pool) f64, order (B, k_out)).  The payload's gate column is read through the merge
        when the layout has one; ``rerank`` / ``best`` / ``gate``: pool-aligned (B, pool) float32 columns of a second pass (a
        host gate and the payload's column exclude each other).  ``out``: the three tensors to write into instead of fresh ones."""
        import torch
        s = self.s
        params = HybridSearcher.make_params(w, k_out, pool, self.world * pool_local, rr_k,
                                            cand_per_rank=pool_local, stride_bytes=lay.nbytes)
        if out is None:
            out = (torch.empty((B, pool), dtype=torch.int64, device=s.device),
                   torch.empty((B, 8, pool), dtype=torch.float64, device=s.device),
                   torch.empty((B, k_out), dtype=torch.int32, device=s.device))
        base = gathered.data_ptr()
        ptr = lambda off: C.c_void_p(base + off)
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        _lib.check(s.lib.rr_fuse_topk_cand_dev(
            s.index.handle, C.byref(params), B, ptr(lay.off_rows), ptr(lay.off_dense), ptr(lay.off_bm25),
            ptr(lay.off_n), ptr(lay.off_avg), ptr(lay.off_l1p), p(rerank), p(best), p(gate),
            ptr(lay.off_gate) if lay.gate else None, p(out[0]), p(out[1]), p(out[2]), s._stream()), "rr_fuse_topk_cand_dev")
        return out

    # ------------------------------------------------------------------ the best-review column
    def _best_whole(self, q_dev, rows, max_scan: int, best_out):
        """One rank, no payload: rr_reviews_best_cut_dev as HybridSearcher.search_batch calls it."""
        import torch
        s = self.s
        B, pool = rows.shape
        best = torch.empty((B, pool), dtype=torch.float32, device=s.device)
        ids = torch.empty((B, pool), dtype=torch.int32, device=s.device)
        q = q_dev if q_dev.is_cuda else q_dev.to(s.device)
        _lib.check(s.lib.rr_reviews_best_cut_dev(
            self.reviews.handle, C.c_void_p(q.data_ptr()), B, C.c_void_p(rows.data_ptr()), pool, s.index.row_offset,
            int(max_scan), C.c_void_p(best.data_ptr()), C.c_void_p(ids.data_ptr()), s._stream()), "rr_reviews_best_cut_dev")
        if best_out is not None:
            best_out["best_ids"], best_out["best_raw"] = ids, best
        return best

    def review_plan(self, pool: int, max_scan: int) -> str:
        """What a batch's best-review step runs, decided on the host from replicated numbers (every rank branches alike, no
        device value is read): "none" -- max_scan <= 0, no review is scored; "skip" -- no pool of ``pool`` products can hold
        more than max_scan reviews (reviews.pool_reviews_bound of the ranks' exchanged counts), the cut cannot bite, every
        cut is n_total; "rounds" -- the cut is found across the ranks."""
        from .reviews import pool_reviews_bound
        if max_scan <= 0:
            return "none"
        return "skip" if pool_reviews_bound(self.review_tops, pool) <= max_scan else "rounds"

    def review_cuts(self, rows, max_scan: int, reduce=None):
        """The rounds of the cut on the merged ``rows`` (B, pool): int32 (B,) global review ids, identical on every rank.
        One launch per round (the narrowing with the previous sums rides in front of the counting), one all-reduce of the
        (B, 256) counts behind it (``reduce``: what sums them instead of `exchange_counts`), one launch at the end."""
        from .reviews import cut_rounds
        rv, off = self.reviews, self.s.index.row_offset
        reduce = reduce or (lambda c: exchange_counts(c, self.world, self.group))
        state, sums = rv.cut_begin(rows.shape[0]), None
        R = cut_rounds(rv.n_total)
        for r in range(R):
            sums = reduce(rv.cut_counts(state, rows, max_scan, off, sums=sums, first=r == 1))
            self.review_rounds_run += 1
        return rv.cut_end(state, sums, max_scan, first=R == 1)

    def best_local(self, q_dev, rows, cuts):
        """This rank's picks for the merged ``rows``: (B, pool) int64 words (pack_picks); rows of other shards: (0, -1)."""
        q = q_dev if q_dev.is_cuda else q_dev.to(self.s.device)
        return pack_picks(*self.reviews.best_at(q, rows, cuts, self.s.index.row_offset))

    def best_column(self, q_dev, max_scan: int, rows, best_out=None):
        """The pool-aligned `_best` column of a batch, on the current stream: plan, cuts, this rank's picks, the all-gather,
        every candidate's entry from its owner.  Returns best_raw (B, pool) float32; ``best_out`` gets ids and scores."""
        import torch
        s, (B, pool) = self.s, rows.shape
        with torch.cuda.device(s.device):
            plan = self.review_plan(pool, max_scan)
            if plan == "none":
                raw = torch.zeros((B, pool), dtype=torch.float32, device=s.device)
                ids = torch.full((B, pool), -1, dtype=torch.int32, device=s.device)
            else:
                cuts = (self.review_cuts(rows, max_scan) if plan == "rounds" else
                        torch.full((B,), self.reviews.n_total, dtype=torch.int32, device=s.device))
                raw, ids = exchange_picks(self.best_local(q_dev, rows, cuts), rows, self.n_total, self.world, self.group)
        if best_out is not None:
            best_out["best_ids"], best_out["best_raw"] = ids, raw
        return raw

    def _pool_columns(self, rows_dev, B: int, pool: int, rr_k: int, gate_fn, rerank_fn, rerank_pairs=None):
        """Host gate factors (gate_fn: every rank, all pairs: string work on replicated texts) and reranker scores (this
        rank's share of the B x rr_k pairs + the score all-gather) for the merged pool; device tensors or None.  With
        ``rerank_pairs`` the share is assembled and scored on the device and the rows stay there, unless a query of the
        batch is over the pair kernel's limit."""
        import torch
        s = self.s
        gate = rerank = None
        n_pairs = B * rr_k
        lo, hi = split_pairs(n_pairs, self.world, self.rank)

        def spread(mine):                                        # my share -> all ranks' scores -> (B, pool), zeros beyond rr_k
            full = exchange_scores(mine, n_pairs, self.world, self.group)
            col = torch.zeros((B, pool), dtype=torch.float32, device=s.device)
            col[:, :rr_k] = full.view(B, rr_k)
            return col

        if rerank_pairs is not None and rr_k > 0:
            ce, rr_queries, rerank_host = rerank_pairs
            with torch.cuda.device(s.device):
                mine = self.rerank_text.scores(ce, rows_dev, rr_k, rr_queries, lo, hi - lo)
                if rr_queries.host_queries:                      # (a property of the batch: every rank branches alike)
                    rows_h = rows_dev.cpu().numpy()
                    for b in rr_queries.host_queries:
                        a, e = max(lo, b * rr_k), min(hi, (b + 1) * rr_k)
                        if a < e:                                # this rank's pairs of query b only
                            r = np.ascontiguousarray(rerank_host(b, rows_h[b, a - b * rr_k:e - b * rr_k]), dtype=np.float32)
                            mine[a - lo:e - lo].copy_(torch.from_numpy(r.reshape(e - a)))
                rerank = spread(mine)
        if gate_fn is None and (rerank_fn is None or rr_k <= 0):
            return gate, rerank
        rows_h = rows_dev.cpu().numpy()
        if gate_fn is not None:
            g = np.ascontiguousarray(gate_fn(rows_h), dtype=np.float32)
            gate = torch.from_numpy(g).to(s.device)
        if rerank_fn is not None and rr_k > 0:
            idx = np.arange(lo, hi)
            qi, ci = idx // rr_k, idx % rr_k
            mine = np.asarray(rerank_fn(qi, rows_h[qi, ci]), dtype=np.float32).reshape(-1)
            if mine.shape[0] != hi - lo:
                raise ValueError("rerank_fn must return one score per pair")
            rerank = spread(torch.from_numpy(mine).to(s.device))
        return gate, rerank
