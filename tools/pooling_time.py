#!/usr/bin/env python3
"""What mean pooling on the device costs (csrc/rr_ce_pool.hip, RR_CE_OUT_MEAN), three measurements in one run:

 (a) `ce_pool_mean` alone on 256 sequences x 512 tokens at hidden 384 / 768 / 1024, beside a device-to-device hipMemcpyAsync of
     the same T x hidden floats -- what RR_CE_OUT_HIDDEN does with them -- alternating in the same loop, one HIP-event pair per
     launch (rr_debug_ce_pool_time of the harness library).  The kernel moves half the copy's bytes (it reads T x hidden
     floats and writes n_seqs x hidden; the copy reads and writes T x hidden).
 (b) the forward of a 6-layer 384 / 12 / 1536 encoder with OUT_MEAN beside OUT_CLS on that workload, in both precisions,
     alternating, between the handle's own HIP events (rr_ce_last_forward_ms): OUT_MEAN gives up the [CLS]-only tail of the
     last layer and adds the pooling kernel.
 (c) the route without the kernel: OUT_HIDDEN, the T x hidden floats down to the host, a float32 numpy mean per sequence --
     host clock around `forward_ids` + the means (it ends on the host by construction), beside `forward_ids(OUT_MEAN)` on the
     same clock.

Every figure is the median of --reps after --warmup untimed repetitions, with its range.  Prints one JSON document; --out
writes it to a file as well (profiles/encoder_pooling.json).  Needs librr_hip_dbg.so (python review-recommender_amd/build.py
--debug)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ["RR_DEBUG_HARNESS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

N_SEQS, LENGTH, VOCAB, LAYERS = 256, 512, 2000, 6


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--forward-reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from review_recommender_amd import _lib, synth
    from review_recommender_amd.cross_encoder import OUT_CLS, OUT_HIDDEN, OUT_MEAN, BertEncoderGPU
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    T = N_SEQS * LENGTH
    cu = torch.arange(0, T + 1, LENGTH, dtype=torch.int32, device=dev)
    result = {"what": "mean pooling on the device: median [min, max] of %d repetitions after %d warm-ups, HIP events unless "
                      "named a host clock" % (a.reps, a.warmup),
              "workload": "%d sequences x %d tokens" % (N_SEQS, LENGTH), "device": torch.cuda.get_device_name(0)}

    # ---- (a) the kernel alone beside the copy of the same rows
    kernel = {}
    for hidden in (384, 768, 1024):
        rows = torch.randn((T, hidden), dtype=torch.float32, device=dev)
        out = torch.empty((N_SEQS, hidden), dtype=torch.float32, device=dev)
        copy = torch.empty_like(rows)
        ms_pool, ms_copy = (C.c_float * a.reps)(), (C.c_float * a.reps)()
        torch.cuda.synchronize()
        _lib.check(lib.rr_debug_ce_pool_time(ptr(rows), T, ptr(cu), N_SEQS, hidden, ptr(out), ptr(copy), a.warmup, a.reps, ms_pool,
                                             ms_copy), "rr_debug_ce_pool_time")
        want = rows.view(N_SEQS, LENGTH, hidden).double().mean(dim=1)
        assert float((out.double() - want).abs().max()) < 1e-6 and bool(torch.equal(copy, rows))       # (both did their work)
        p, c = stats(list(ms_pool)), stats(list(ms_copy))
        read = T * hidden * 4
        p["bytes"], c["bytes"] = read + N_SEQS * hidden * 4, 2 * read
        p["gb_per_s"], c["gb_per_s"] = round(p["bytes"] / p["median_ms"] / 1e6, 1), round(c["bytes"] / c["median_ms"] / 1e6, 1)
        kernel["hidden %d" % hidden] = {"ce_pool_mean": p, "hipMemcpyAsync_d2d": c,
                                        "kernel_over_copy": round(p["median_ms"] / c["median_ms"], 3)}
        del rows, out, copy
    result["a_kernel_alone"] = kernel

    # ---- (b) the forward with OUT_MEAN beside OUT_CLS, (c) OUT_HIDDEN + download + numpy
    rng = np.random.default_rng(3)
    ids = rng.integers(0, VOCAB, (N_SEQS, LENGTH)).astype(np.int32)
    seqs = [(row, np.zeros(LENGTH, np.int32)) for row in ids]
    sd = synth.bert_state_dict(1, n_layers=LAYERS, vocab=VOCAB, n_labels=0, prefix="")
    forward, host_route = {}, {}
    for precision in ("fp32", "bf16"):
        model = BertEncoderGPU(sd, with_head=False, precision=precision, max_tokens_per_call=T)
        ms = {OUT_CLS: [], OUT_MEAN: []}
        for i in range(-1, a.forward_reps):                  # one warm-up of each mode, then alternating
            for mode in (OUT_CLS, OUT_MEAN):
                model.forward_ids(seqs, mode)
                if i >= 0:
                    ms[mode].append(model.last_forward_ms())
        cls, mean = stats(ms[OUT_CLS]), stats(ms[OUT_MEAN])
        forward[precision] = {"layers": LAYERS, "OUT_CLS": cls, "OUT_MEAN": mean,
                              "mean_minus_cls_ms": round(mean["median_ms"] - cls["median_ms"], 4),
                              "one_layers_share_ms": round(cls["median_ms"] / LAYERS, 4)}
        wall = {"hidden": [], "mean": []}
        for i in range(-1, a.forward_reps):
            t0 = time.perf_counter()
            h = model.forward_ids(seqs, OUT_HIDDEN)
            e = h.reshape(N_SEQS, LENGTH, -1).mean(axis=1, dtype=np.float32)
            t1 = time.perf_counter()
            m = model.forward_ids(seqs, OUT_MEAN)
            t2 = time.perf_counter()
            if i >= 0:
                wall["hidden"].append((t1 - t0) * 1e3)
                wall["mean"].append((t2 - t1) * 1e3)
        assert float(np.abs(e - m).max()) < 1e-4
        host_route[precision] = {"clock": "host, around forward_ids (upload of the ids, forward, download) + the numpy means",
                                 "OUT_HIDDEN_download_numpy_mean": stats(wall["hidden"]), "OUT_MEAN": stats(wall["mean"]),
                                 "downloaded_mb": {"OUT_HIDDEN": round(T * 384 * 4 / 1e6, 1), "OUT_MEAN": round(N_SEQS * 384 * 4 / 1e6, 2)}}
        model.close()
    result["b_forward_mean_beside_cls"] = forward
    result["c_route_without_the_kernel"] = host_route
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
