"""``nlp/10_product_prep.py`` on the GPU: ``reviews_merged.parquet`` -> ``products.parquet`` (sku, n_reviews, avg_stars,
last_ts, agg_text).

    python -m review_recommender_amd.products --in data/processed/reviews_merged.parquet \\
        --out data/processed/products.parquet --max-reviews-per-sku 80

``model_build_products`` states the step in numpy, once (nlp/10_product_prep.py:21-85):

1. clean: runs of ``str.isspace()`` characters become one U+0020, the text is stripped; NO cut at 4000 characters (unlike
   nlp/11); a row survives with at least 10 code points;
2. dedup: a survivor goes when an earlier one has the same sku and the same cleaned text;
3. KPIs per sku over all of its survivors: ``n_reviews``, ``avg_stars`` = the float64 mean of the non-NaN stars rounded to 3
   (NaN without any), ``last_ts`` = the largest non-NaT ts (else NaT); skus in code-point order, none without a survivor;
4. order inside a sku: stars descending with NaN last, then ts descending with NaT last, then the row's position
   (pandas' sort is stable).  ``-0.0 == 0.0``; the infinities order as numbers, so ``-inf`` comes BEFORE NaN and the earliest
   representable time before NaT, as ``sort_values`` has them;
5. ``agg_text`` = the cleaned texts of the first ``max_reviews_per_sku`` rows of that order joined by ``" \\n"``;
6. ``deduped`` = rows in - rows that survive 1 and 2.

``build_products`` computes the same on the device: rr_textprep_clean_chars_dev (no cut, no spam rules) and
rr_textprep_dedup_dev (csrc/rr_textprep.hip), then rr_products_order_dev and rr_products_concat_dev (csrc/rr_products.hip).
The concatenated text stays on the device in the layout ``DeviceDocTokenizer.tokenize_dev`` reads
(``keep_device=True`` -> ``prep.build_bm25_blob_device``), so the BM25 index needs no host copy of it.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import pathlib
import sys
import time
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib

DEF_IN = "data/processed/reviews_merged.parquet"          # nlp/10_product_prep.py:18-19
DEF_OUT = "data/processed/products.parquet"
MIN_CHARS = 10                                             # :43,50
MAX_REVIEWS_PER_SKU = 80                                   # :91
SEPARATOR = " \n"                                          # :76
COLUMNS = ("sku", "n_reviews", "avg_stars", "last_ts", "agg_text")
NAT = np.iinfo(np.int64).min


def normalize_text(s) -> str:
    """nlp/10_product_prep.py:21-24."""
    s = (s or "").replace("\r", " ").replace("\n", " ").strip()
    return " ".join(s.split())


def prepare_columns(reviews) -> Tuple[np.ndarray, List[str], np.ndarray, np.ndarray]:
    """nlp/10_product_prep.py:29-41 -> (sku as an object array of str, texts, stars float64 with NaN, ts int64 ns with NaT =
    INT64_MIN).  ``stars`` / ``ts`` may be absent: all NaN / NaT."""
    import pandas as pd
    miss = {"id", "sku", "text"} - set(reviews.columns)
    if miss:
        raise ValueError(f"review table missing columns: {sorted(miss)} (need at least id, sku, text)")
    n = len(reviews)
    sku = reviews["sku"].astype(str).to_numpy(dtype=object)
    texts = reviews["text"].fillna("").astype(str).tolist()
    if "stars" in reviews.columns:
        stars = pd.to_numeric(reviews["stars"], errors="coerce").to_numpy(dtype=np.float64, na_value=np.nan)
    else:
        stars = np.full(n, np.nan)
    if "ts" in reviews.columns:
        t = pd.to_datetime(reviews["ts"], utc=True, errors="coerce")
        ts = np.ascontiguousarray(t.dt.tz_localize(None).to_numpy(dtype="datetime64[ns]")).view(np.int64)
    else:
        ts = np.full(n, NAT, dtype=np.int64)
    return sku, texts, np.ascontiguousarray(stars, dtype=np.float64), np.ascontiguousarray(ts, dtype=np.int64)


def _frame(skus, n_reviews, star_sum, star_cnt, last_ts, agg_text=None):
    """The reference's frame: sku object, n_reviews int64, avg_stars float64 rounded to 3, last_ts datetime64[ns, UTC]."""
    import pandas as pd
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.where(star_cnt > 0, np.asarray(star_sum, dtype=np.float64) / np.maximum(star_cnt, 1), np.nan)
    cols = {"sku": np.asarray(skus, dtype=object), "n_reviews": np.asarray(n_reviews, dtype=np.int64),
            "avg_stars": np.round(avg.astype(np.float64), 3),
            "last_ts": pd.DatetimeIndex(np.asarray(last_ts, dtype=np.int64).view("datetime64[ns]")).tz_localize("UTC")}
    df = pd.DataFrame(cols)
    if agg_text is not None:
        df["agg_text"] = np.asarray(agg_text, dtype=object) if len(agg_text) else pd.Series([], dtype=object)
    return df


def model_order(code: np.ndarray, stars: np.ndarray, ts: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """The order of step 4 over parallel arrays: positions sorted by (code, stars descending NaN last, ts descending NaT
    last, rows)."""
    nan, nat = np.isnan(stars), ts == NAT
    star_key = np.where(nan, 0.0, -(np.where(nan, 0.0, stars) + 0.0))
    ts_key = np.where(nat, 0, -np.where(nat, 0, ts))
    return np.lexsort((rows, ts_key, nat, star_key, nan, code))


def model_build_products(reviews, max_reviews_per_sku: int = MAX_REVIEWS_PER_SKU):
    """(products, deduped) of nlp/10_product_prep.py:46-85 in numpy: the specification in this module's docstring."""
    sku, texts, stars, ts = prepare_columns(reviews)
    clean = [normalize_text(t) for t in texts]
    seen = set()
    rows = []
    for i, c in enumerate(clean):
        if len(c) >= MIN_CHARS and (sku[i], c) not in seen:
            seen.add((sku[i], c))
            rows.append(i)
    rows = np.asarray(rows, dtype=np.int64)
    deduped = len(texts) - len(rows)
    if len(rows) == 0:
        return _frame([], [], np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64), []), deduped
    skus, code = np.unique(sku[rows], return_inverse=True)             # code-point order
    code = code.reshape(-1)
    s, t = stars[rows], ts[rows]
    order = model_order(code, s, t, rows)
    n_skus = len(skus)
    n_reviews = np.bincount(code, minlength=n_skus).astype(np.int64)
    seg = np.zeros(n_skus + 1, dtype=np.int64)
    np.cumsum(n_reviews, out=seg[1:])
    ok = ~np.isnan(s)
    star_sum = np.bincount(code[ok], weights=s[ok], minlength=n_skus)   # one accumulator per sku, in row order
    star_cnt = np.bincount(code[ok], minlength=n_skus).astype(np.int64)
    last_ts = np.maximum.reduceat(t[order], seg[:-1])                   # NaT is the smallest int64
    keep = max(int(max_reviews_per_sku), 0)
    agg = [SEPARATOR.join(clean[rows[j]] for j in order[seg[k]:min(seg[k + 1], seg[k] + keep)]) for k in range(n_skus)]
    return _frame(skus, n_reviews, star_sum, star_cnt, last_ts, agg), deduped


# ---------------------------------------------------------------------------------- the device calls
class ProductsPrep:
    """rr_products_order_dev / rr_products_concat_dev on one GPU.  Every pointer argument is a device address (int); calls
    are queued on `stream` (a hipStream_t as int, None = the NULL stream) and must be stream-ordered per handle."""

    def __init__(self, device: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the products builder runs on the device only")
        self.device = int(device)
        h = C.c_void_p()
        _lib.check(_lib.load().rr_products_create(self.device, C.byref(h)), "rr_products_create")
        self._h = h

    def order(self, status: int, group: int, stars: int, ts: int, n: int, n_skus: int, perm: int, seg_off: int, n_reviews: int,
              star_sum: int, star_cnt: int, last_ts: int, stream: Optional[int] = None) -> None:
        _lib.check(_lib.load().rr_products_order_dev(self._h, C.c_void_p(status), C.c_void_p(group), C.c_void_p(stars), C.c_void_p(ts),
                                                     int(n), int(n_skus), C.c_void_p(perm), C.c_void_p(seg_off), C.c_void_p(n_reviews),
                                                     C.c_void_p(star_sum), C.c_void_p(star_cnt), C.c_void_p(last_ts),
                                                     C.c_void_p(stream)), "rr_products_order_dev")

    def concat(self, text: int, text_bytes: int, offsets: int, lens: int, n: int, perm: int, seg_off: int, n_skus: int,
               max_per_sku: int, out_text: int, out_bytes: int, out_off: int, count: int, stream: Optional[int] = None) -> None:
        _lib.check(_lib.load().rr_products_concat_dev(self._h, C.c_void_p(text), int(text_bytes), C.c_void_p(offsets), C.c_void_p(lens),
                                                      int(n), C.c_void_p(perm), C.c_void_p(seg_off), int(n_skus),
                                                      int(min(max(int(max_per_sku), 0), 2 ** 31 - 1)), C.c_void_p(out_text),
                                                      int(out_bytes), C.c_void_p(out_off), C.c_void_p(count), C.c_void_p(stream)),
                   "rr_products_concat_dev")

    def check(self) -> None:
        """Raises ValueError when a concat since the last check refused its arguments (waits for the device)."""
        bad = C.c_int32()
        _lib.check(_lib.load().rr_products_status(self._h, C.byref(bad)), "rr_products_status")

    def order_arrays(self, status, group, stars, ts, n_skus: int):
        """Host arrays in, host arrays out (tests and small callers): (perm[:m], seg_off, n_reviews, star_sum, star_cnt,
        last_ts)."""
        import torch
        n = len(status)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev) if n else torch.zeros(1, device=dev)
            d_st, d_g, d_s, d_t = up(status, np.int32), up(group, np.int32), up(stars, np.float64), up(ts, np.int64)
            d_perm = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
            d_seg = torch.full((n_skus + 1,), -7, dtype=torch.int64, device=dev)
            outs = [torch.full((max(n_skus, 1),), -7, dtype=dt, device=dev) for dt in (torch.int64, torch.float64, torch.int64, torch.int64)]
            st = torch.cuda.current_stream(dev)
            self.order(d_st.data_ptr(), d_g.data_ptr(), d_s.data_ptr(), d_t.data_ptr(), n, n_skus, d_perm.data_ptr(), d_seg.data_ptr(),
                       *[o.data_ptr() for o in outs], st.cuda_stream)
            st.synchronize()
            seg = d_seg.cpu().numpy()
            return (d_perm.cpu().numpy()[:int(seg[-1])], seg) + tuple(o.cpu().numpy()[:n_skus] for o in outs)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_products_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceProductText:
    """agg_text of every product where rr_products_concat_dev wrote it: ``d_text`` uint8 and ``d_off`` int64[n + 1] tensors
    on ``device`` (the layout ``DeviceDocTokenizer.tokenize_dev`` reads), ``n`` products, ``text_bytes`` bytes, ``skus`` in
    row order.  ``agg_text()`` copies the strings to the host the first time it is asked."""

    def __init__(self, skus, d_text, d_off, n: int, text_bytes: int, device: int):
        self.skus, self.d_text, self.d_off, self.n, self.text_bytes, self.device = list(skus), d_text, d_off, int(n), int(text_bytes), device
        self._texts: Optional[List[str]] = None

    def agg_text(self) -> List[str]:
        if self._texts is None:
            blob = self.d_text[:self.text_bytes].cpu().numpy()
            off = self.d_off.cpu().numpy()
            self._texts = _split_utf8(blob, off)
        return self._texts

    def with_text(self, products):
        """`products` with its agg_text column."""
        out = products.copy()
        out["agg_text"] = np.asarray(self.agg_text(), dtype=object) if self.n else out["sku"].iloc[:0]
        return out[list(COLUMNS)]


def _split_utf8(blob: np.ndarray, off: np.ndarray) -> List[str]:
    """Text i = blob[off[i] : off[i + 1]] as str."""
    n = len(off) - 1
    if n <= 0:
        return []
    try:
        import pyarrow as pa
        arr = pa.LargeStringArray.from_buffers(n, pa.py_buffer(np.ascontiguousarray(off, dtype=np.int64)),
                                               pa.py_buffer(np.ascontiguousarray(blob)))
        arr.validate(full=True)
        return arr.to_pylist()
    except Exception:                              # no pyarrow, or a lone surrogate's three bytes
        raw, o = blob.tobytes(), off.tolist()
        return [raw[o[i]:o[i + 1]].decode("utf-8", "surrogatepass") for i in range(n)]


def sku_ranks(sku: np.ndarray, alive: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(sorted distinct skus of the rows in `alive`, int32 rank of every row's sku among them; -1 where the sku has no row
    in `alive`).  One hash pass over the rows, and a sort of the distinct skus only."""
    import pandas as pd
    codes, uniq = pd.factorize(sku)
    has = np.zeros(len(uniq), dtype=bool)
    has[codes[alive]] = True
    idx = np.flatnonzero(has)
    idx = idx[np.argsort(np.asarray(uniq, dtype=object)[idx], kind="stable")]      # str comparisons: code-point order
    rank = np.full(len(uniq) + 1, -1, dtype=np.int32)
    rank[idx] = np.arange(len(idx), dtype=np.int32)
    return np.asarray(uniq, dtype=object)[idx], rank[codes]


def build_products(reviews, max_reviews_per_sku: int = MAX_REVIEWS_PER_SKU, device: int = 0, stats: Optional[dict] = None,
                   keep_device: bool = False, stage_bytes: Optional[int] = None):
    """nlp/10_product_prep.py:46-85 on the GPU -> (products, deduped); the same values as `model_build_products`.

    The raw text goes up through the pinned two-buffer staging of the review builder (embed._stage_rows) and is cleaned in
    place, block by block; the rows the kernel leaves to the host (longer than its window, malformed UTF-8) are cleaned by
    `normalize_text` here and written into their slots; duplicates are marked per sku; rr_products_order_dev orders the
    survivors and reduces the KPIs; rr_products_concat_dev writes agg_text.  keep_device=True -> (products WITHOUT agg_text,
    deduped, DeviceProductText): the text stays on the device, `.agg_text()` / `.with_text(products)` fetch it when asked.
    stats receives "short" and "duplicate" (rows dropped), "host_clean_docs" (rows cleaned on the host) and "seconds", the
    wall clock of the phases (each ends where the host waits for the device anyway)."""
    import torch
    from . import embed, textprep as T
    seconds: Dict[str, float] = {}
    clock = [time.perf_counter()]

    def lap(name):
        now = time.perf_counter()
        seconds[name] = seconds.get(name, 0.0) + now - clock[0]
        clock[0] = now

    if stats is not None:
        stats["seconds"] = seconds
    if int(max_reviews_per_sku) < 1:
        raise ValueError("max_reviews_per_sku must be at least 1")
    sku, texts, stars, ts = prepare_columns(reviews)
    n = len(texts)
    lap("prepare_columns")
    if n == 0:
        empty = _frame([], [], np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64), None if keep_device else [])
        if stats is not None:
            stats.update(short=0, duplicate=0, host_clean_docs=[])
        return (empty, 0, DeviceProductText([], None, None, 0, 0, device)) if keep_device else (empty, 0)
    raw, off = embed._utf8_column(texts)
    total = int(off[-1])
    lap("utf8_bytes")
    dev = torch.device("cuda", int(device))
    tp, pb = T.TextPrep(int(device)), ProductsPrep(int(device))
    try:
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            st_ptr = main.cuda_stream
            d_text = torch.empty(total + 16, dtype=torch.uint8, device=dev)
            d_off = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
            d_len = torch.empty(n, dtype=torch.int32, device=dev)
            d_st = torch.empty(n, dtype=torch.int32, device=dev)
            embed._stage_rows(raw, off, d_text, main, embed.STAGE_BYTES if stage_bytes is None else stage_bytes,
                              lambda a, b: tp.clean(d_text.data_ptr(), total, d_off.data_ptr() + 8 * a, b - a, False, d_text.data_ptr(),
                                                    d_len.data_ptr() + 4 * a, d_st.data_ptr() + 4 * a, st_ptr, max_chars=0))
            main.synchronize()
            tp.check()
            status, lens = d_st.cpu().numpy(), d_len.cpu().numpy()
            lap("copy_and_clean")

            host_clean = np.flatnonzero(status & T.NEEDS_HOST)
            cleaned = []
            for i in host_clean.tolist():
                t = normalize_text(texts[i])
                tb = t.encode("utf-8", "surrogatepass")
                cleaned.append(tb)
                lens[i] = len(tb)
                status[i] = T.SHORT if len(t) < MIN_CHARS else 0
            embed._write_host_rows(d_text, off, host_clean.tolist(), cleaned)
            if len(host_clean):
                d_len.copy_(torch.from_numpy(lens))
                d_st.copy_(torch.from_numpy(status))
            n_short = int(np.count_nonzero(status & T.SHORT))
            lap("host_clean")

            skus, group = sku_ranks(sku, status == 0)
            n_skus = len(skus)
            d_group = torch.from_numpy(group).to(dev)
            lap("sku_ranks")
            tp.dedup(d_text.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), d_group.data_ptr(), d_st.data_ptr(), n, 64, st_ptr)
            status = d_st.cpu().numpy()
            tp.check()
            keep = status == 0
            m = int(np.count_nonzero(keep))
            lap("dedup")

            d_stars, d_ts = torch.from_numpy(stars).to(dev), torch.from_numpy(ts).to(dev)
            d_perm = torch.empty(n, dtype=torch.int32, device=dev)
            d_seg = torch.empty(n_skus + 1, dtype=torch.int64, device=dev)
            d_kpi = torch.empty((4, max(n_skus, 1)), dtype=torch.int64, device=dev)      # n_reviews, star sum (as bits), count, last_ts
            pb.order(d_st.data_ptr(), d_group.data_ptr(), d_stars.data_ptr(), d_ts.data_ptr(), n, n_skus, d_perm.data_ptr(),
                     d_seg.data_ptr(), *[d_kpi[j].data_ptr() for j in range(4)], st_ptr)
            kpi = d_kpi.cpu().numpy()[:, :n_skus]
            lap("order_and_kpis")

            cap = int(lens[keep].astype(np.int64).sum()) + 2 * m
            d_out = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
            d_out_off = torch.empty(n_skus + 1, dtype=torch.int64, device=dev)
            d_count = torch.empty(1, dtype=torch.int64, device=dev)
            pb.concat(d_text.data_ptr(), total, d_off.data_ptr(), d_len.data_ptr(), n, d_perm.data_ptr(), d_seg.data_ptr(), n_skus,
                      max_reviews_per_sku, d_out.data_ptr(), cap, d_out_off.data_ptr(), d_count.data_ptr(), st_ptr)
            out_bytes = int(d_count.cpu()[0])
            pb.check()
            del d_text
            text = DeviceProductText(skus, d_out, d_out_off, n_skus, out_bytes, int(device))
            lap("concatenate")
            products = _frame(skus, kpi[0], kpi[1].view(np.float64), kpi[2], kpi[3], None if keep_device else text.agg_text())
            lap("frame")
    finally:
        tp.close()
        pb.close()
    if stats is not None:
        stats.update(short=n_short, duplicate=int(np.count_nonzero(status & T.DUP)), host_clean_docs=host_clean.tolist())
    return (products, n - m, text) if keep_device else (products, n - m)


# ---------------------------------------------------------------------------------- command line
def load_reviews(path):
    """nlp/10_product_prep.py:26-44: the columns it reads, and its filter on the RAW text's length."""
    import pandas as pd
    path = pathlib.Path(path)
    if not path.exists():
        raise FileNotFoundError(f"Missing input: {path}")
    df = pd.read_parquet(path)
    df = df[[c for c in ("id", "sku", "ts", "stars", "text") if c in df.columns]]
    miss = {"id", "sku", "text"} - set(df.columns)
    if miss:
        raise ValueError(f"{path} missing columns: {sorted(miss)} (need at least id, sku, text)")
    return df[df["text"].fillna("").astype(str).str.len() >= MIN_CHARS].copy()


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m review_recommender_amd.products",
                                 description="Create products.parquet from reviews_merged.parquet on the GPU (nlp/10_product_prep.py's flags).")
    ap.add_argument("--in", dest="inp", default=DEF_IN, help=f"Input reviews parquet (default: {DEF_IN})")
    ap.add_argument("--out", dest="out", default=DEF_OUT, help=f"Output products parquet (default: {DEF_OUT})")
    ap.add_argument("--max-reviews-per-sku", type=int, default=MAX_REVIEWS_PER_SKU,
                    help=f"Max reviews to concatenate per SKU (default: {MAX_REVIEWS_PER_SKU})")
    ap.add_argument("--device", type=int, default=0, help="GPU ordinal")
    args = ap.parse_args(argv)
    if args.max_reviews_per_sku < 1:
        ap.error("--max-reviews-per-sku must be at least 1")
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    outp = pathlib.Path(args.out)
    t0 = time.perf_counter()
    df = load_reviews(args.inp)
    stats: dict = {}
    t1 = time.perf_counter()
    products, deduped = build_products(df, args.max_reviews_per_sku, device=args.device, stats=stats)
    t2 = time.perf_counter()
    outp.parent.mkdir(parents=True, exist_ok=True)
    products.to_parquet(outp, index=False)
    t3 = time.perf_counter()
    print(f"[OK] products.parquet written: {outp}")                                  # nlp/10_product_prep.py:103-107
    print(f"     products: {len(products):,} | deduped review rows: {deduped:,}")
    print("     sample:")
    print(products[list(COLUMNS)].head(3).to_string(index=False))
    seconds = dict(stats["seconds"], read_file=t1 - t0, build_products=t2 - t1, write_file=t3 - t2)
    print(json.dumps({"seconds": {k: round(v, 6) for k, v in seconds.items()}}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
