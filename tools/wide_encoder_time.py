#!/usr/bin/env python3
"""K5 timing at encoder shapes other than 384 / 12 / 1536 (csrc/rr_ce_w.hip + ce_gemm_x3): the forward between HIP events for
256 sequences of 512 tokens and for 256 queries of 8 tokens, at 768 / 12 / 3072 x 12 layers (BERT-base, bge-base) and at
1024 / 16 / 4096 x 24 layers (bge-large), each beside the 384 / 12 / 1536 x 6 model on `set_wide_range(True)` -- the same
three-term arithmetic on the kernels built for that shape -- in the same run.  `flop_scaled_ratio` = (time / model FLOPs) of
the shape over (time / model FLOPs) of the 384 model on the same workload: 1.0 means the runtime-shape kernels run at the
384 kernels' rate.  Prints one JSON document; --out writes it to a file as well (profiles/wide_encoder.json)."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = [("384/12/1536 x 6, wide range", 384, 12, 1536, 6), ("768/12/3072 x 12", 768, 12, 3072, 12), ("1024/16/4096 x 24", 1024, 16, 4096, 24)]
WORKLOADS = [("256 x 512 tokens", 256, 512), ("256 queries x 8 tokens", 256, 8)]
VOCAB = 2000


def model_flops(hidden, ffn, layers, lens):
    """What the forward computes: the four GEMMs of every token and Q K^T + P V of every sequence, per layer."""
    lens = np.asarray(lens, dtype=np.float64)
    return layers * (lens.sum() * 2.0 * hidden * (4 * hidden + 2 * ffn) + (4.0 * hidden * lens * lens).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from review_recommender_amd import synth
    from review_recommender_amd.cross_encoder import OUT_CLS, BertEncoderGPU
    rng = np.random.default_rng(3)
    result = {"what": "HIP-event time of rr_ce_forward_dev (RR_CE_OUT_CLS), median of %d after one warm-up" % a.reps, "workloads": {}}
    times = {}
    for name, hidden, heads, ffn, layers in MODELS:
        sd = synth.bert_state_dict(1, n_layers=layers, hidden=hidden, ffn=ffn, vocab=VOCAB, n_labels=0, prefix="")
        model = BertEncoderGPU(sd, with_head=False, n_heads=heads)
        del sd
        if hidden == 384:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                model.set_wide_range(True)
        for wname, n, length in WORKLOADS:
            ids = rng.integers(0, VOCAB, (n, length)).astype(np.int32)
            seqs = [(row, np.zeros(length, np.int32)) for row in ids]
            model.forward_ids(seqs, OUT_CLS)
            ms = []
            for _ in range(a.reps):
                model.forward_ids(seqs, OUT_CLS)
                ms.append(model.last_forward_ms())
            t = float(np.median(ms))
            flops = model_flops(hidden, ffn, layers, [length] * n)
            times[(name, wname)] = (t, flops)
            result["workloads"].setdefault(wname, {})[name] = {
                "forward_ms": round(t, 3), "model_tflop": round(flops / 1e12, 4), "model_tflops_per_s": round(flops / t / 1e9, 2)}
        model.close()
    base = MODELS[0][0]
    for wname, _, _ in WORKLOADS:
        t0, f0 = times[(base, wname)]
        for name, *_ in MODELS[1:]:
            t, f = times[(name, wname)]
            row = result["workloads"][wname][name]
            row["time_ratio_to_384"] = round(t / t0, 3)
            row["flop_ratio_to_384"] = round(f / f0, 3)
            row["flop_scaled_ratio"] = round((t / f) / (t0 / f0), 3)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
