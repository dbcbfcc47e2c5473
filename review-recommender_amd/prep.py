"""The BM25 half of ``nlp/12_product_prep.py:main`` with the tokenizer on the GPU.

    python -m review_recommender_amd.prep --data-dir data/processed

Reads ``products.parquet`` (else ``product_emb_meta.parquet``) from the directory, takes the text column by the reference's
fallbacks (nlp/12_product_prep.py:58-73: ``agg_text``, ``text``, ``merged_text``, ``description``; ``fillna("").astype(str)``),
tokenises it on the device (csrc/rr_doctok.hip) and writes ``product_bm25.pkl`` = ``{"skus", "corpus", "tokenizer":
"simple_en_v1"}`` with pickle protocol 4 (:85-89): the value the reference writes.  Turning the ids back into the token
lists of the pickle is host work (one object-array take and one split); its time is reported on a line of its own.
The topic-vector half of nlp/12 (:91-169) is not part of this build.

    python -m review_recommender_amd.prep --data-dir data/processed --reviews data/processed/reviews_merged.parquet

builds the product texts from the review table first (products.build_products, nlp/10_product_prep.py on the GPU) and
tokenises agg_text where the concatenation wrote it: the text is not copied to the host in between.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import pickle
import time

PRODUCTS_FILES = ("products.parquet", "product_emb_meta.parquet")      # nlp/12_product_prep.py:30-31, 53-56
TEXT_COLUMNS = ("agg_text", "text", "merged_text", "description")      # :62-66
BM25_FILE = "product_bm25.pkl"


def load_products(data_dir):
    """nlp/12_product_prep.py:53-73 -> a frame with ``sku`` and ``agg_text``."""
    import pandas as pd
    d = pathlib.Path(data_dir)
    path = next((d / f for f in PRODUCTS_FILES if (d / f).exists()), None)
    if path is None:
        raise FileNotFoundError(f"products.parquet or product_emb_meta.parquet not found in {d}")
    df = pd.read_parquet(path)
    if "sku" not in df.columns:
        raise ValueError(f"{path} must have column 'sku'")
    col = next((c for c in TEXT_COLUMNS if c in df.columns), None)
    if col is None:
        raise ValueError(f"No text column found in {path} (expect 'agg_text').")
    df = df[["sku", col]].copy()
    df[col] = df[col].fillna("").astype(str)
    return df.rename(columns={col: "agg_text"})


def build_bm25_blob_device(products, device: int = 0, seconds=None) -> dict:
    """``artifacts.build_bm25_blob(products)`` with the tokens made on the GPU: the same value.  `products`: a frame with
    ``sku`` and ``agg_text``, or the ``products.DeviceProductText`` of ``build_products(..., keep_device=True)``, whose text
    is read on its device where rr_products_concat_dev wrote it."""
    from .doctok import DeviceDocTokenizer, ids_to_corpus
    from .products import DeviceProductText
    on_device = isinstance(products, DeviceProductText)
    if on_device and products.n == 0:
        return {"skus": [], "corpus": [], "tokenizer": "simple_en_v1"}
    dt = DeviceDocTokenizer(products.device if on_device else device)
    try:
        t0 = time.perf_counter()
        if on_device:
            tok, off, vocab = dt.tokenize_dev(products.d_text, products.text_bytes, products.d_off, products.n)
        else:
            tok, off, vocab = dt.tokenize(products["agg_text"].fillna("").astype(str).tolist())
        tok, off = tok.cpu().numpy(), off.cpu().numpy()
        t1 = time.perf_counter()
        corpus = ids_to_corpus(tok, off, vocab)
        t2 = time.perf_counter()
    finally:
        dt.close()
    if seconds is not None:
        seconds.update(dt.seconds, device_tokenize_total=t1 - t0, ids_to_token_lists_host=t2 - t1)
    skus = [str(s) for s in products.skus] if on_device else products["sku"].astype(str).tolist()
    return {"skus": skus, "corpus": corpus, "tokenizer": "simple_en_v1"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Build product_bm25.pkl from the product table, tokenised on the GPU")
    ap.add_argument("--data-dir", type=str, default="data/processed")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reviews", type=str, default="",
                    help="a review table (reviews_merged.parquet): build the product texts from it on the GPU "
                         "(nlp/10_product_prep.py) instead of reading products.parquet, and tokenise them from device memory")
    ap.add_argument("--max-reviews-per-sku", type=int, default=80, help="with --reviews: reviews concatenated per sku")
    args = ap.parse_args(argv)
    if args.max_reviews_per_sku < 1:
        ap.error("--max-reviews-per-sku must be at least 1")
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    d = pathlib.Path(args.data_dir)
    seconds: dict = {}
    if args.reviews:
        from .products import build_products, load_reviews
        t0 = time.perf_counter()
        _, _, df = build_products(load_reviews(args.reviews), args.max_reviews_per_sku, device=args.device, keep_device=True)
        seconds["build_products"] = time.perf_counter() - t0
        d.mkdir(parents=True, exist_ok=True)
    else:
        df = load_products(d)
    blob = build_bm25_blob_device(df, args.device, seconds)
    t0 = time.perf_counter()
    with open(d / BM25_FILE, "wb") as f:
        pickle.dump(blob, f, protocol=4)
    seconds["pickle_write"] = time.perf_counter() - t0
    print(f"[ok] wrote {d / BM25_FILE}  docs={len(blob['skus']):,}", flush=True)
    print(f"[time] device tokenizer and vocabulary {seconds['device_tokenize_total']:.3f} s; "
          f"ids -> token lists on the host {seconds['ids_to_token_lists_host']:.3f} s", flush=True)
    print(json.dumps({"seconds": {k: round(v, 6) for k, v in seconds.items()}}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
