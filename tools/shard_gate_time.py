"""Times a gated query batch on the row-sharded path with the host gate and with the gate before the merge (sharded.py).

    python tools/shard_gate_time.py --out profiles/shard_gate_b256.json

One GPU, ONE process: the corpus of tools/gate_time.py (100 k products whose agg_text fills the gate's 6000 characters) is cut
into eight row shards that all live on this GPU.  Per batch (256 queries, pool 150, gate_penalty 0.5) every shard builds its
payload as a rank would, one after the other; the all-gather is replaced by the in-process copy the tests use
(tests/test_gpu_sharded_gate.py); K3 merges the eight lists.  Nothing here is a multi-GPU number: the shards' work that
eight GPUs do side by side runs back to back, there is no wire, and the floor exchange (a collective) is left out, so every
shard selects on its own threshold.  What the comparison shows is the cost that does NOT shrink with the ranks: the host
gate is the same Python loop over the merged pool on every rank.

A full batch = from the first launch to the finished answer on the host (rows, columns, order), median / p10 / p90:
  gate_fn_s        the parent's path: payloads, K3 with k = pool for the merged order, rows to the host, the host gate
                   (pandas slice + text.calculate_gate_factor per candidate, SearchEngine._gate_rows' loop; run once here,
                   every rank repeats it), upload, K3 again with the pool-aligned column;
  gate_groups_s    the gate before the merge: payloads with the gate column (every shard matches its own candidates against
                   the plane of its own rows), ONE K3 (rr_fuse_topk_cand_dev);
  no_gate_s        payloads, one K3;
and on ONE rank that holds the whole corpus and runs the payload path (force_payload), because the overlapped pipeline's
collectives need a process group for more than one rank:
  one_rank_gate_groups_s           search_batch_dev(gate_groups=...), one batch at a time;
  one_rank_overlap_gate_groups_s   the same batches through enable_overlap()'s pipeline, two tickets in flight: per batch
                                   from its submit to its answer on the host, and `per_batch_s`, the loop's wall clock over
                                   its batches.
Also the bytes of gate plane per shard, and that the three gated forms answer bitwise the same.  The one condition is
device_gate_batch_faster: gate_groups_s < gate_fn_s (medians) on the same corpus in the same run; the ratio and the gate's
added time over the ungated batch are recorded, not gated."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from gate_time import make_queries, spread      # noqa: E402  (the corpus is synth.text_corpus with gate_time's arguments)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--mean-words", type=int, default=1200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--scan-cus", type=int, default=128)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import pandas as pd
    import torch
    from review_recommender_amd import gate as G, synth, text as T
    from review_recommender_amd.bm25 import BM25Corpus
    from review_recommender_amd.engine import FusionWeights, HybridSearcher
    from review_recommender_amd.index import ProductIndex
    from review_recommender_amd.sharded import PayloadLayout, ShardedSearcher, shard_bounds

    n, B, world, pool, k, pen = a.docs, a.batch, a.shards, 150, 10, 0.5
    t0 = time.perf_counter()
    texts = synth.text_corpus(n, 3, mean_len=a.mean_words)
    chars = np.array([len(t) for t in texts])
    res = {"docs": n, "batch": B, "shards": world, "pool": pool, "gate_penalty": pen, "min_chars": int(chars.min()),
           "mean_chars": float(chars.mean()), "make_corpus_s": time.perf_counter() - t0}
    assert chars.min() >= 6000, "every document must fill the gate's 6000 characters"
    print("corpus", res, flush=True)
    series = pd.Series(texts)
    V = synth.unit_rows(n, 384, 1)
    n_rev, stars = synth.metadata(n, 2)
    vocab = 5000
    ip, terms, tf, dl = synth.bm25_forward_csr(n, vocab, 30, 4)
    corpus = BM25Corpus(ip, terms, tf, dl, vocab)

    def build(lo, hi):
        ix = ProductIndex(V[lo:hi], row_offset=lo)
        ix.set_meta(n_rev[lo:hi].astype(np.float64), stars[lo:hi])
        return HybridSearcher(ix, corpus.slice(lo, hi).to_device(row_offset=lo),
                              gate_text=G.GateText.from_texts(texts[lo:hi], 0, row_offset=lo))

    t0 = time.perf_counter()
    shards = [ShardedSearcher(build(*shard_bounds(n, world, r)), n, r, world) for r in range(world)]
    res["shards_build_s"] = time.perf_counter() - t0
    res["plane_bytes_per_shard"] = [int(sh.s.gate_text.plane_bytes) for sh in shards]
    res["plane_device_bytes_per_shard"] = [int(sh.s.gate_text.nbytes) for sh in shards]

    queries = make_queries(B, 7)
    groups = [T.build_gate_groups(q) for q in queries]
    q_dev = torch.from_numpy(synth.unit_rows(B, 384, 9)).cuda()
    tl = synth.query_terms(B, vocab, 5, np.bincount(terms, minlength=vocab))
    w = FusionWeights(0.55, 0.20, 0.0, 0.20, 0.0, 20.0, 8, pen)
    packed = G.pack_groups(groups, pen)
    assert not packed.host_queries
    res.update(groups_per_query=float(np.mean([len(g) for g in groups])), queries_without_groups=int(sum(not g for g in groups)))

    def gate_rows(g, rows):                                  # SearchEngine._gate_rows
        if not g:
            return np.ones(len(rows), dtype=np.float32)
        heads = series.iloc[rows].str.slice(0, 6000).tolist()
        return np.array([T.calculate_gate_factor(t, g, pen)[0] for t in heads], dtype=np.float32)

    gate_fn = lambda rows: np.stack([gate_rows(g, r) for g, r in zip(groups, rows)])
    lays = {False: PayloadLayout(B, pool), True: PayloadLayout(B, pool, gate=True)}
    gathered = {g: torch.empty((world, lay.nbytes), dtype=torch.uint8, device="cuda") for g, lay in lays.items()}

    def fuse(lay, buf, k_out, gate=None):
        return shards[0].merge(lay, buf, B, k_out, pool, pool, w, gate=gate)

    def batch(mode):
        gated = mode == "gate_groups"
        lay, buf = lays[gated], gathered[gated]
        for r, sh in enumerate(shards):
            sh.local_payload(q_dev, tl, pool, buf=buf[r], gate=packed if gated else None)     # (built in place: the "all-gather")
        if mode == "gate_fn":
            rows, _, _ = fuse(lay, buf, pool)
            g = torch.from_numpy(np.ascontiguousarray(gate_fn(rows.cpu().numpy()), dtype=np.float32)).cuda()
            out = fuse(lay, buf, k, g)
        else:
            out = fuse(lay, buf, k)
        return [t.cpu().numpy() for t in out]                # (the device has finished)

    for _ in range(3):                                       # warm-up of every shape the timed loops use
        got_groups, got_none = batch("gate_groups"), batch("no_gate")
    got_fn = batch("gate_fn")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got_groups, got_fn)), "the two gates differ"
    assert got_groups[1][:, 7].tobytes() != got_none[1][:, 7].tobytes()
    res["gates_equal_bitwise"] = True
    res["gated_candidates_fraction"] = float((got_groups[1][:, 5, :] != 1).mean())

    times = {"gate_groups": [], "no_gate": [], "gate_fn": []}
    for i in range(a.reps):
        for mode in ("gate_groups", "no_gate") + (("gate_fn",) if i < a.host_reps else ()):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch(mode)
            times[mode].append(time.perf_counter() - t0)
    for mode, xs in times.items():
        res[mode + "_s"] = spread(xs)
    for sh in shards:
        sh.s.gate_text.check()

    # one rank, the whole corpus, the payload path: straight and through the overlapped pipeline
    del shards, gathered
    torch.cuda.empty_cache()
    one = ShardedSearcher(build(0, n), n, 0, 1)
    one.force_payload = True
    kw = dict(pool_floor=pool, gate_groups=groups)
    cur = torch.cuda.Stream()                                # (the masked streams are blocking: keep off the NULL stream)
    with torch.cuda.stream(cur):
        straight = []
        for i in range(a.reps + 3):
            cur.synchronize()
            t0 = time.perf_counter()
            ans = [t.cpu().numpy() for t in one.search_batch_dev(q_dev, tl, k, w, **kw)]
            straight.append(time.perf_counter() - t0)
        res["one_rank_gate_groups_s"] = spread(straight[3:])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ans, got_groups)), "one rank differs from eight shards"
        res["overlap_scan_cus"] = a.scan_cus
        assert one.enable_overlap(a.scan_cus)
        try:
            lat, inflight, n_batches = [], [], a.reps + 3
            cur.synchronize()
            wall0 = None
            for i in range(n_batches):
                if i == 3:
                    cur.synchronize()
                    wall0 = time.perf_counter()
                inflight.append((time.perf_counter(), one.submit(q_dev, tl, k, w, **kw)))
                assert inflight[-1][1].slot >= 0, "the gated batch left the pipeline"
                while len(inflight) > 2:
                    t0, t = inflight.pop(0)
                    last = [x.cpu().numpy() for x in one.finish(t)]
                    lat.append(time.perf_counter() - t0)
            while inflight:
                t0, t = inflight.pop(0)
                last = [x.cpu().numpy() for x in one.finish(t)]
                lat.append(time.perf_counter() - t0)
            wall = time.perf_counter() - wall0
        finally:
            one.disable_overlap()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(last, got_groups)), "the pipeline's answer differs"
        res["one_rank_overlap_gate_groups_s"] = dict(spread(lat[3:]), per_batch_s=wall / (n_batches - 3), in_flight=2)
    one.s.gate_text.check()

    res["gate_fn_over_gate_groups"] = res["gate_fn_s"]["median"] / res["gate_groups_s"]["median"]
    res["gate_groups_added_over_no_gate_s"] = res["gate_groups_s"]["median"] - res["no_gate_s"]["median"]
    res["device_gate_batch_faster"] = res["gate_groups_s"]["median"] < res["gate_fn_s"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    if not res["device_gate_batch_faster"]:
        raise SystemExit("the gate before the merge is not faster than the host gate")


if __name__ == "__main__":
    main()
