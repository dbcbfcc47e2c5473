"""Times the reranker's pair building of one query batch on the host and on the GPU (review-recommender_amd/rerank.py,
csrc/rr_pairs.hip).

    python tools/rerank_time.py --out profiles/rerank_pairs_b64.json

One GPU, 100 k products whose agg_text has about 2000 characters (synth.text_corpus), a word-list vocabulary, seeded 6-layer
weights (synth.bert_state_dict), B = 64 queries of the corpus' words, rerank_k = 200 (BASELINE config 5: 12 800 pairs per
batch).  Prints one JSON line:
  (a) host_pairs_s        the host's pair building alone, as the engine runs it with rerank="host": the pandas slice of the
                          candidates' texts, CrossEncoder.tokenize_pairs, and the numpy packing of BertEncoderGPU.forward_ids
                          (lengths, concatenation, positions) per chunk -- no upload, no forward;
  (b) device_pairs_s      RerankText.pairs over the same chunks: rr_pairs_measure_dev, the read-back of the token count,
                          rr_pairs_write_dev; the wall clock up to a device synchronise.  write_kernel_s: rr_pairs_write_dev
                          alone between HIP events, and the bytes it moves (2 read + 12 written per token) over that time;
  (c) forward_s           forward_packed_dev over the chunks (b) made, up to a device synchronise;
  (d) run_search_batch_*  SearchEngine.run_search_batch end to end with rerank="host" and rerank="device", alternating;
  (e) plane_build_s       RerankText.from_texts over the column, and that per 100 k products;
each of (a)-(d) as median / p10 / p90 over the timed repetitions after warm-up.  The two engines' frames are compared
bitwise.  Nothing is asserted about the times: the figures are what the run reports."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8e12


def spread(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)), "n": len(xs)}


def host_pairs(engine, ce, queries, rows, cap):
    """The parent's pair building without the device: slice, tokenize_pairs, forward_ids' packing.  Returns the tokens."""
    texts = engine._texts.iloc[rows.reshape(-1)].str.slice(0, 2000).tolist()
    seqs = ce.tokenize_pairs([(queries[i // rows.shape[1]], t) for i, t in enumerate(texts)])
    lens = np.array([len(s[0]) for s in seqs], dtype=np.int64)
    n, start, total = len(seqs), 0, 0
    while start < n:
        end, tot = start, 0
        while end < n and (end == start or tot + lens[end] <= cap):
            tot += int(lens[end])
            end += 1
        part = seqs[start:end]
        cu = np.zeros(len(part) + 1, dtype=np.int32)
        np.cumsum(lens[start:end], out=cu[1:])
        ids = np.concatenate([np.asarray(s[0], dtype=np.int32) for s in part])
        typ = np.concatenate([np.asarray(s[1], dtype=np.int32) for s in part])
        pos = (np.arange(tot, dtype=np.int32) - np.repeat(cu[:-1], lens[start:end])).astype(np.int32)
        packed = np.concatenate([ids, typ, pos, cu]).astype(np.int32)
        total += tot
        start = end
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--mean-words", type=int, default=330)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rerank-k", type=int, default=200)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import ctypes as C
    import pandas as pd
    import torch
    from review_recommender_amd import _lib, rerank as R, synth
    from review_recommender_amd.cross_encoder import FP32_MAX_TOKENS, OUT_LOGITS, CrossEncoder
    from review_recommender_amd.engine import SearchEngine
    from review_recommender_amd.wordpiece import WordPieceTokenizer

    t0 = time.perf_counter()
    texts = synth.text_corpus(a.docs, 3, mean_len=a.mean_words)
    chars = np.array([len(t) for t in texts])
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(synth.WORDS)
    tok = WordPieceTokenizer({w: i for i, w in enumerate(words)})
    ce = CrossEncoder(synth.bert_state_dict(41, n_layers=a.layers, vocab=len(words)), tok)
    L = ce.max_length
    res = {"docs": a.docs, "batch": a.batch, "rerank_k": a.rerank_k, "layers": a.layers, "precision": ce.model.precision,
           "max_length": L, "mean_chars": float(chars.mean()), "make_corpus_s": time.perf_counter() - t0}
    print("corpus", res, flush=True)
    n_rev, stars = synth.metadata(a.docs, 2)
    meta = pd.DataFrame({"sku": synth.skus(a.docs), "n_reviews": n_rev, "avg_stars": stars, "agg_text": texts})
    blob = {"skus": meta["sku"].tolist(), "corpus": [t[:240].split() for t in texts]}      # K2 over short documents
    emb = synth.unit_rows(a.docs, 384, 1)
    host = SearchEngine(meta, emb, blob, normalize=False, cross_encoder=ce, rerank="host")
    t0 = time.perf_counter()
    dev = SearchEngine(meta, emb, blob, normalize=False, cross_encoder=ce, rerank="device")
    res["engine_build_device_s"] = time.perf_counter() - t0
    rt = dev.searcher.rerank_text
    res.update(plane_tokens=rt.n_tokens, plane_device_bytes=rt.nbytes, plane_host_docs=len(rt.host_docs),
               plane_tokens_per_doc=rt.n_tokens / a.docs)

    # (e) the plane alone
    builds = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r2 = R.RerankText.from_texts(texts, tok, L, 0)         # (ends in a stream synchronise)
        builds.append(time.perf_counter() - t0)
        r2.close()
    res["plane_build_s"] = spread(builds[1:])
    res["plane_build_s_per_100k"] = res["plane_build_s"]["median"] * 1e5 / a.docs

    rng = np.random.default_rng(7)
    queries = [" ".join(rng.choice(synth.WORDS, size=int(rng.integers(2, 6)))) for _ in range(a.batch)]
    qvecs = synth.unit_rows(a.batch, 384, 9)
    args = (10, a.rerank_k, 0.45, 0.15, 0.3, 0.1, 0.0, 20.0, False, 0, 8, 1.0)
    run = lambda e: e.run_search_batch(queries, *args, qvecs=qvecs)

    # the candidate rows of the batch, as both paths see them
    pool = min(max(10, a.rerank_k, 150), a.docs)
    rr_k = min(a.rerank_k, pool)
    with torch.cuda.device(0):
        d_rows, _ = dev.searcher.dense_pool(torch.from_numpy(qvecs).cuda(), pool)
        torch.cuda.synchronize()
    rows = d_rows.cpu().numpy()
    cap = min(ce.model.max_tokens_per_call, FP32_MAX_TOKENS)
    step = max(1, cap // L)
    total = a.batch * rr_k
    res.update(pool=pool, pairs=total, pairs_per_chunk=step, chunks=(total + step - 1) // step)

    # (a) the host's pair building
    t_host = []
    for _ in range(a.host_reps + 1):
        t0 = time.perf_counter()
        n_tok_host = host_pairs(host, ce, queries, rows[:, :rr_k], cap)
        t_host.append(time.perf_counter() - t0)
    res["host_pairs_s"] = spread(t_host[1:])

    # (b) measure + read-back + write, (c) the forward over what (b) made
    packed = R.pack_queries([tok.text_ids(q) for q in queries], L)
    staged = rt.upload(packed)
    t_pairs, t_fwd = [], []
    for _ in range(a.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chunks = [rt.pairs(d_rows, rr_k, packed, s, min(step, total - s), staged) for s in range(0, total, step)]
        torch.cuda.synchronize()
        t_pairs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        outs = [ce.model.forward_packed_dev(*c, c[3].numel() - 1, L, OUT_LOGITS) for c in chunks]
        torch.cuda.synchronize()
        t_fwd.append(time.perf_counter() - t0)
    n_tok = int(sum(c[0].numel() for c in chunks))
    assert n_tok == n_tok_host, (n_tok, n_tok_host)
    assert not bool(torch.isnan(torch.cat(outs)).any())
    res.update(tokens=n_tok, tokens_per_pair=n_tok / total, device_pairs_s=spread(t_pairs[2:]), forward_s=spread(t_fwd[2:]))

    # rr_pairs_write_dev alone, all pairs in one launch, between HIP events
    lib, p = _lib.load(), (lambda t: C.c_void_p(t.data_ptr()))
    with torch.cuda.device(0):
        keep = torch.empty((total, 2), dtype=torch.int32, device="cuda")
        cu = torch.empty(total + 1, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.rr_pairs_measure_dev(rt._h, p(rt.d_off), rt.n, 0, p(d_rows), pool, rr_k, p(staged[0]), a.batch, L, 0, total,
                                            p(keep), p(cu), st), "rr_pairs_measure_dev")
        assert int(cu[total]) == n_tok
        ids = torch.empty(3 * n_tok, dtype=torch.int32, device="cuda")
        t_write, t_measure = [], []
        for _ in range(a.reps + 3):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            _lib.check(lib.rr_pairs_measure_dev(rt._h, p(rt.d_off), rt.n, 0, p(d_rows), pool, rr_k, p(staged[0]), a.batch, L, 0,
                                                total, p(keep), p(cu), st), "rr_pairs_measure_dev")
            e1.record()
            _lib.check(lib.rr_pairs_write_dev(rt._h, p(rt.d_tok), p(rt.d_off), rt.n, 0, p(d_rows), pool, rr_k,
                                              C.c_void_p(staged[0].data_ptr() + 4 * staged[1]), p(staged[0]), a.batch, rt.cls_id,
                                              rt.sep_id, 0, total, p(keep), p(cu), n_tok, p(ids), C.c_void_p(ids.data_ptr() + 4 * n_tok),
                                              C.c_void_p(ids.data_ptr() + 8 * n_tok), st), "rr_pairs_write_dev")
            e2.record()
            torch.cuda.synchronize()
            t_measure.append(e0.elapsed_time(e1) / 1e3)
            t_write.append(e1.elapsed_time(e2) / 1e3)
        rt.check()
    moved = 14 * n_tok
    res.update(measure_kernels_s=spread(t_measure[3:]), write_kernel_s=spread(t_write[3:]), write_kernel_bytes=moved,
               write_kernel_bytes_per_s=moved / np.median(t_write[3:]),
               write_kernel_fraction_of_hbm_peak=moved / np.median(t_write[3:]) / HBM_BYTES_PER_S)

    # (d) run_search_batch end to end, the two paths alternating
    want, got = run(host), run(dev)                          # warm-up of both, and the comparison
    for _ in range(2):
        run(dev)
    equal = all(gf.shape == wf.shape and all(gf[c].values.tobytes() == wf[c].values.tobytes() if gf[c].dtype.kind == "f"
                                             else gf[c].tolist() == wf[c].tolist() for c in gf.columns)
                for (gf, _, _), (wf, _, _) in zip(got, want))
    res["frames_equal_bitwise"] = bool(equal)
    e2e = {"device": [], "host": []}
    for i in range(a.reps):
        for name, e in (("device", dev), ("host", host)):
            if name == "host" and i >= a.host_reps:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(e)                                           # (returns frames: the device has finished)
            e2e[name].append(time.perf_counter() - t0)
    res["run_search_batch_device_s"] = spread(e2e["device"])
    res["run_search_batch_host_s"] = spread(e2e["host"])
    res["device_pairs_over_host_pairs"] = res["device_pairs_s"]["median"] / res["host_pairs_s"]["median"]
    res["device_pairs_over_forward"] = res["device_pairs_s"]["median"] / res["forward_s"]["median"]
    res["run_search_batch_host_over_device"] = res["run_search_batch_host_s"]["median"] / res["run_search_batch_device_s"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    if not equal:
        raise SystemExit("the frames of rerank=\"device\" and rerank=\"host\" differ")


if __name__ == "__main__":
    main()
