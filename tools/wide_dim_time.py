"""Times K1 on indexes of other embedding widths than 384 (csrc/rr_dense_fltw.hip against the VALU scans).

    python tools/wide_dim_time.py --label head --out profiles/wide_dim_scan.json
    python tools/wide_dim_time.py --dtype bf16 --batches 1,64,256 --label bf16 --out profiles/wide_dim_bf16_scan.json

One GPU, 1M unit rows made on the device, widths 768 and 1024, batches 5, 8, 9, 16, 64, 256, pool 150: rr_dense_topk_dev
between HIP events on the default stream, one warm-up call and `--reps` (>= 20) timed ones per shape.  One JSON line per
(width, batch) goes to stdout and is APPENDED to --out (so the lines of two builds -- `--label parent`, `--label head` --
stand in one file):
  call_ms          median / p10 / p90 of the whole call (padding, scans, selections, flagged-query passes);
  last_scan_info   (family, variant, queries of the launch, MFMA terms, element bytes) of the last scan launch;
  last_scan_ms     rr_index_last_scan_ms: the last timed scan launch by itself;
  scans_per_call, scan_ms_per_call   rr_index_scan_stats over the timed calls: launches and their summed time per call;
  stream_bytes     bytes of matrix one scan launch streams (rows x padded width x element bytes);
  scan_fraction_of_hbm_peak   stream_bytes x scans_per_call / scan_ms_per_call over 8 TB/s;
  queries_per_s    batch / median call;
  device_bytes     hipMemGetInfo's free memory before the matrix was made minus after this shape's calls: the rows, and
                   whatever the index allocated beside them so far (the bf16 plane of an fp32 index from its first batched
                   call on, scratch).  `--dtype bf16`: the same rows rounded once to bf16 in a bf16 index, which has no plane.
`--summary` reads --out back and prints head / parent rate ratios per shape and the smallest batch from which the head
wins at both widths."""
import argparse
import ctypes as C
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8e12
WIDTHS = (768, 1024)
BATCHES = (5, 8, 9, 16, 64, 256)


def spread(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)), "n": len(xs)}


def summary(path):
    lines = [json.loads(l) for l in pathlib.Path(path).read_text().splitlines() if l.strip()]
    by = {(l["label"], l["dim"], l["batch"]): l for l in lines}
    wins = {}
    for dim in WIDTHS:
        for b in BATCHES:
            h, p = by.get(("head", dim, b)), by.get(("parent", dim, b))
            if h and p:
                r = p["call_ms"]["median"] / h["call_ms"]["median"]
                wins[(dim, b)] = r
                print(f"dim {dim} batch {b}: parent {p['call_ms']['median']:.3f} ms, head {h['call_ms']['median']:.3f} ms, head / parent rate {r:.2f}")
    # a bf16 index (--dtype bf16 --label bf16) against the parent's fp32 index of the same rows (--label parent)
    for (label, dim, b), h in sorted(by.items(), key=lambda kv: (kv[0][1], kv[0][2])):
        p = by.get(("parent", dim, b))
        if label == "bf16" and p:
            print(f"dim {dim} batch {b}: parent fp32 {p['call_ms']['median']:.3f} ms / {p['device_bytes'] / 2**30:.2f} GiB, "
                  f"bf16 {h['call_ms']['median']:.3f} ms / {h['device_bytes'] / 2**30:.2f} GiB, "
                  f"bf16 / fp32 time {h['call_ms']['median'] / p['call_ms']['median']:.3f}")
    cross = [b for b in BATCHES if all(wins.get((d, b2), 0) > 1.0 for d in WIDTHS for b2 in BATCHES if b2 >= b)]
    print("smallest batch from which the head wins at both widths:", cross[0] if cross else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--pool", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="head")
    ap.add_argument("--dtype", default="f32", choices=("f32", "bf16"), help="storage of the index (bf16: the rows rounded once)")
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)), help="comma-separated batch sizes (default: the issue's grid)")
    ap.add_argument("--out", default="")
    ap.add_argument("--summary", action="store_true")
    a = ap.parse_args()
    if a.summary:
        return summary(a.out)
    assert a.reps >= 20, "at least 20 timed calls per shape"
    import torch
    from review_recommender_amd import _lib
    from review_recommender_amd.index import ProductIndex
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    for dim in WIDTHS:
        g = torch.Generator(device="cuda")
        g.manual_seed(dim)
        torch.cuda.empty_cache()
        free_before = torch.cuda.mem_get_info(dev)[0]
        mat = torch.randn((a.rows, dim), generator=g, device=dev)
        mat /= mat.norm(dim=1, keepdim=True)
        if a.dtype == "bf16":
            mat = mat.to(torch.bfloat16)
        ix = ProductIndex(None, n_rows=a.rows, dim=dim, device_ptr=mat.data_ptr(), keepalive=mat, dtype=a.dtype)
        for b in [int(x) for x in a.batches.split(",")]:
            q = torch.randn((b, dim), generator=g, device=dev)
            q /= q.norm(dim=1, keepdim=True)
            rows = torch.empty((b, a.pool), dtype=torch.int64, device=dev)
            sc = torch.empty((b, a.pool), dtype=torch.float32, device=dev)
            call = lambda: _lib.check(lib.rr_dense_topk_dev(ix.handle, C.c_void_p(q.data_ptr()), b, a.pool, C.c_void_p(rows.data_ptr()),
                                                            C.c_void_p(sc.data_ptr()), None), "rr_dense_topk_dev")
            call()                                          # warm-up (scratch, the bf16 plane, the row-norm bound)
            torch.cuda.synchronize()
            total, n = C.c_double(), C.c_int64()
            _lib.check(lib.rr_index_scan_stats(ix.handle, C.byref(total), C.byref(n)), "rr_index_scan_stats")     # (drains the warm-up's)
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(torch.cuda.default_stream())
                call()
                e1.record(torch.cuda.default_stream())
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            _lib.check(lib.rr_index_scan_stats(ix.handle, C.byref(total), C.byref(n)), "rr_index_scan_stats")
            info = ix.last_scan_info()
            try:
                last_ms = ix.last_scan_ms()
            except ValueError:                              # (the bf16 VALU scans record no event pair of their own)
                last_ms = None
            torch.cuda.empty_cache()                        # (the fp32 rows a bf16 matrix was rounded from, the queries of earlier shapes)
            device_bytes = free_before - torch.cuda.mem_get_info(dev)[0]
            stream_bytes = a.rows * ix.dim_padded * info[4]
            scan_ms = total.value / a.reps
            line = {"label": a.label, "dtype": a.dtype, "device_bytes": device_bytes, "rows": a.rows, "dim": dim, "batch": b, "pool": a.pool, "call_ms": spread(ms),
                    "last_scan_info": list(info), "last_scan_ms": last_ms, "scans_per_call": n.value / a.reps,
                    "scan_ms_per_call": scan_ms, "stream_bytes": stream_bytes,
                    "scan_fraction_of_hbm_peak": stream_bytes * (n.value / a.reps) / (scan_ms / 1e3) / HBM_BYTES_PER_S if scan_ms > 0 else None,
                    "queries_per_s": b / (float(np.median(ms)) / 1e3)}
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")
        ix.close()
        ix = mat = q = rows = sc = None                     # (the index keeps its adopted matrix alive: the next width's device_bytes starts clean)


if __name__ == "__main__":
    main()
