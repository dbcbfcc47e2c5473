"""Cross-encoder reranker and query encoder on the GPU (K5).

Drop-ins for the two sentence-transformers objects the reference holds:

  CrossEncoder(RERANK_MODEL).predict(pairs, batch_size=64, show_progress_bar=False) -> (len(pairs),) float32
      app/app_product_search.py:71-86,277-278; app/test.py:96-104,223-225
  SentenceTransformer(EMB_MODEL).encode([query], normalize_embeddings=True) -> (n, 384) float32
      app/app_product_search.py:53-69,250-251; app/test.py:91-94,232

Both run csrc/rr_ce.hip through the C ABI (rr_ce_create / rr_ce_forward_dev), in one of two precisions: "fp32" (default:
the reference's arithmetic: every fp32 operand as two fp16 numbers, three matrix-core products per fp32 product, within 1e-5
of `transformers`) or "bf16"
(the fast path: bf16 MFMA GEMMs + attention, fp32 residual stream).  Weights come from a local state dict (Hugging Face BERT names: a
`model.safetensors` / `pytorch_model.bin` directory, or a dict of arrays); text is tokenised by
wordpiece.WordPieceTokenizer from a local vocab.txt.  Without a vocabulary on disk the pre-tokenised entry
points (`predict_ids`, `encode_ids`) take token-id sequences directly.  Nothing is ever fetched.

The reference leaves one thing undeterminable offline: whether predict applies Identity or Sigmoid to the
single logit (it depends on the hub model's config).  `activation` is therefore a parameter,
default raw logits; min-max follows in run_search either way (app/app_product_search.py:279).
"""
from __future__ import annotations

import ctypes as C
import json
import pathlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .wordpiece import WordPieceTokenizer

OUT_LOGITS, OUT_CLS, OUT_HIDDEN, OUT_MEAN = 0, 1, 2, 3       # RR_CE_OUT_*
POOLINGS = {"cls": OUT_CLS, "mean": OUT_MEAN}    # QueryEncoder(pooling=...): the sentence vector's output mode
PRECISIONS = {"bf16": 0, "fp32": 1}              # RR_CE_PRECISION_*
HIDDEN, HEADS, FFN = 384, 12, 1536                  # the shape with kernels of its own in both precisions
MAX_HIDDEN, MAX_FFN = 1024, 4096                    # the family of every other shape (csrc/rr_ce_w.h)
FP32_MAX_TOKENS = 1 << 27                           # tokens per rr_ce_forward_dev call in fp32 precision (include/rr_hip.h)
OTHER_SHAPE_MAX_TOKENS = 65535 * 128                # ... at a shape other than 384 / 12 / 1536 (csrc/rr_ce_w.h)

_LAYER_KEYS = ("attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
               "attention.self.key.bias", "attention.self.value.weight", "attention.self.value.bias",
               "attention.output.dense.weight", "attention.output.dense.bias", "attention.output.LayerNorm.weight",
               "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias",
               "output.dense.weight", "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias")


def _np(v) -> np.ndarray:
    if hasattr(v, "detach"):
        v = v.detach().cpu().float().numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


def _find_prefix(sd: Dict) -> str:
    for p in ("bert.", "model.", ""):
        if p + "embeddings.word_embeddings.weight" in sd:
            return p
    raise ValueError("state dict holds no '[bert.]embeddings.word_embeddings.weight': not a BERT checkpoint")


def model_shape(sd: Dict, n_heads: Optional[int] = None, cfg: Optional[Dict] = None, precision: str = "fp32") -> Tuple[int, int, int]:
    """(hidden, n_heads, ffn) of a BERT state dict, checked against what rr_ce_create accepts (include/rr_hip.h) and
    refused in its words.  Needs neither a GPU nor the library.  hidden and ffn are read off the tensors; n_heads is the
    argument, else `num_attention_heads` of `cfg` (a config.json as a dict), else 12 at hidden 384 and hidden // 64
    anywhere else (BERT-base, bge-large, TinyBERT; a 32-wide head at another width has to be named).  384 / 12 / 1536
    runs in both precisions; every other shape needs hidden % 128 == 0 in [128, 1024], a head dim of 32 or 64,
    ffn % 128 == 0 in [128, 4096] and precision "fp32"."""
    p = _find_prefix(sd)
    hidden = int(sd[p + "embeddings.word_embeddings.weight"].shape[1])
    key = p + "encoder.layer.0.intermediate.dense.weight"
    if key not in sd:
        raise ValueError("state dict holds no encoder layers")
    ffn = int(sd[key].shape[0])
    if n_heads is None and cfg and cfg.get("num_attention_heads") is not None:
        n_heads = cfg["num_attention_heads"]
    if n_heads is None:
        n_heads = HEADS if hidden == HIDDEN else hidden // 64
    n_heads = int(n_heads)
    if (hidden, n_heads, ffn) != (HIDDEN, HEADS, FFN):
        if hidden < 128 or hidden > MAX_HIDDEN or hidden % 128:
            raise ValueError(f"rr_ce_create: hidden {hidden} is not a multiple of 128 in [128, {MAX_HIDDEN}]")
        if n_heads < 1 or hidden % n_heads or hidden // n_heads not in (32, 64):
            hd = hidden / n_heads if n_heads >= 1 else 0.0
            raise ValueError(f"rr_ce_create: head dim {hd:g} (hidden {hidden} / {n_heads} heads) is not 32 or 64")
        if ffn < 128 or ffn > MAX_FFN or ffn % 128:
            raise ValueError(f"rr_ce_create: ffn {ffn} is not a multiple of 128 in [128, {MAX_FFN}]")
        if precision == "bf16":
            raise ValueError(f"rr_ce_create: precision bf16 is built for hidden {HIDDEN} / {HEADS} heads / FFN {FFN} only; hidden "
                             f"{hidden} / {n_heads} heads / FFN {ffn} runs in precision fp32")
    return hidden, n_heads, ffn


class BertEncoderGPU:
    """A BERT encoder (+ optional sequence-classification head) resident on one GPU.  `.hidden`, `.n_heads`, `.ffn`: its
    block shape (`model_shape`)."""

    def __init__(self, state_dict: Dict, *, device: int = 0, ln_eps: float = 1e-12, with_head: bool = True,
                 max_tokens_per_call: int = 131_072, precision: str = "fp32", n_heads: Optional[int] = None):
        """``n_heads``: attention heads (default: 12 at hidden 384, hidden // 64 elsewhere; `model_shape`).
        ``precision``: "fp32" = the reference's arithmetic (fp32 weights and activations, products on the fp16 matrix
        cores as exact as an fp32 multiply-add chain: logits / embeddings within 1e-5 of `transformers`; a value beyond
        fp16's range switches the handle to the wide-range kernels, see `out_of_range`), "bf16" = the fast path (bf16
        operands, fp32 accumulation: 2.5e-2 on O(1) logits, ~2.7x the throughput).  include/rr_hip.h: RR_CE_PRECISION_*.
        A shape other than 384 / 12 / 1536 runs in "fp32" only, on the three-term kernels (any fp32 range: `out_of_range`
        stays False)."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.precision = precision
        sd = state_dict
        self.hidden, self.n_heads, self.ffn = model_shape(sd, n_heads, precision=precision)      # (before any device call)
        p = _find_prefix(sd)
        word = _np(sd[p + "embeddings.word_embeddings.weight"])
        pos = _np(sd[p + "embeddings.position_embeddings.weight"])
        typ = _np(sd[p + "embeddings.token_type_embeddings.weight"])
        n_layers = 0
        while f"{p}encoder.layer.{n_layers}.attention.self.query.weight" in sd:
            n_layers += 1
        if n_layers == 0:
            raise ValueError("state dict holds no encoder layers")
        has_head = with_head and "classifier.weight" in sd and (p + "pooler.dense.weight") in sd
        tensors: List[np.ndarray] = [word, pos, typ, _np(sd[p + "embeddings.LayerNorm.weight"]),
                                     _np(sd[p + "embeddings.LayerNorm.bias"])]
        for l in range(n_layers):
            tensors += [_np(sd[f"{p}encoder.layer.{l}.{k}"]) for k in _LAYER_KEYS]
        n_labels = 0
        if has_head:
            cw = _np(sd["classifier.weight"])
            n_labels = cw.shape[0]
            tensors += [_np(sd[p + "pooler.dense.weight"]), _np(sd[p + "pooler.dense.bias"]), cw,
                        _np(sd["classifier.bias"])]
        self.n_layers, self.n_labels, self.vocab, self.max_pos = n_layers, n_labels, word.shape[0], pos.shape[0]
        self.type_vocab, self.device = typ.shape[0], device
        self.max_tokens_per_call = int(max_tokens_per_call)
        self.wide_range = False                         # set_wide_range: which fp32-mode kernels the NEXT launch runs
        cfg = _lib.CEConfig(self.hidden, n_layers, self.n_heads, self.ffn, self.vocab, self.max_pos, self.type_vocab, n_labels, ln_eps,
                            PRECISIONS[precision])
        ptrs = (C.c_void_p * len(tensors))(*[t.ctypes.data for t in tensors])
        h = C.c_void_p()
        _lib.check(_lib.load().rr_ce_create(device, C.byref(cfg), ptrs, len(tensors), C.byref(h)), "rr_ce_create")
        self._h = h
        import torch
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no GPU visible: the encoder runs on the device only")
        self._torch = torch
        self._dev = torch.device("cuda", device)

    @property
    def handle(self):
        return self._h

    # ------------------------------------------------------------------ forward over token ids
    def _check(self, seqs):
        for ids, typ in seqs:
            if len(ids) < 1 or len(ids) > self.max_pos:
                raise ValueError(f"a sequence has {len(ids)} tokens; the model takes 1..{self.max_pos}")
            if len(typ) != len(ids):
                raise ValueError("token ids and token type ids differ in length")

    def _width(self, mode: int) -> int:
        widths = {OUT_LOGITS: self.n_labels, OUT_CLS: self.hidden, OUT_HIDDEN: self.hidden, OUT_MEAN: self.hidden}
        if mode not in widths:
            raise ValueError(f"rr_ce_forward_dev: unknown mode {mode}")
        return widths[mode]

    def forward_ids(self, seqs: Sequence[Tuple[Sequence[int], Sequence[int]]], mode: int = OUT_LOGITS) -> np.ndarray:
        """seqs: (token_ids, type_ids) per sequence (unpadded).  Returns logits (n, n_labels), CLS states (n, hidden), the mean over
        each sequence's tokens (n, hidden; OUT_MEAN, in `model_pool_mean`'s order) or the hidden states of all tokens (sum of lengths, hidden) by `mode`.  Sequences are packed back to back and
        processed in chunks of at most `max_tokens_per_call` tokens; inside a chunk they are sorted by length only for
        the launch bound (the result is independent of batch composition: there is no padding to attend to)."""
        torch = self._torch
        self._check(seqs)
        n = len(seqs)
        width = self._width(mode)
        lens = np.array([len(s[0]) for s in seqs], dtype=np.int64)
        if mode == OUT_LOGITS and self.n_labels == 0:
            raise ValueError("this encoder was loaded without a classification head")
        out = np.empty((int(lens.sum()) if mode == OUT_HIDDEN else n, width), dtype=np.float32)
        lib = _lib.load()
        cap = min(self.max_tokens_per_call, FP32_MAX_TOKENS) if self.precision == "fp32" else self.max_tokens_per_call
        if (self.hidden, self.n_heads, self.ffn) != (HIDDEN, HEADS, FFN):
            cap = min(cap, OTHER_SHAPE_MAX_TOKENS)
        start = 0
        tok_done = 0
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
            if ids.min() < 0 or ids.max() >= self.vocab or typ.min() < 0 or typ.max() >= self.type_vocab:
                raise ValueError("token id or token type id outside the embedding tables")
            pos = (np.arange(tot, dtype=np.int32) - np.repeat(cu[:-1], lens[start:end])).astype(np.int32)
            packed = np.concatenate([ids, typ, pos, cu]).astype(np.int32)
            with torch.cuda.device(self._dev):
                d = torch.from_numpy(packed).to(self._dev)
                rows = tot if mode == OUT_HIDDEN else len(part)
                d_out = torch.empty((rows, width), dtype=torch.float32, device=self._dev)
                base = d.data_ptr()
                _lib.check(lib.rr_ce_forward_dev(
                    self._h, C.c_void_p(base), C.c_void_p(base + 4 * tot), C.c_void_p(base + 8 * tot),
                    C.c_void_p(base + 12 * tot), len(part), tot, int(lens[start:end].max()), mode,
                    C.c_void_p(d_out.data_ptr()), C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)),
                    "rr_ce_forward_dev")
                res = d_out.cpu().numpy()
                if self.precision == "fp32" and self.out_of_range():
                    # an activation beyond fp16's 65504 (csrc/rr_ce_h2.hip): this handle continues on the wide-range kernels
                    self.set_wide_range(True)
                    _lib.check(lib.rr_ce_forward_dev(
                        self._h, C.c_void_p(base), C.c_void_p(base + 4 * tot), C.c_void_p(base + 8 * tot),
                        C.c_void_p(base + 12 * tot), len(part), tot, int(lens[start:end].max()), mode,
                        C.c_void_p(d_out.data_ptr()), C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)),
                        "rr_ce_forward_dev")
                    res = d_out.cpu().numpy()
            if mode == OUT_HIDDEN:
                out[tok_done:tok_done + tot] = res
            else:
                out[start:end] = res
            tok_done += tot
            start = end
        return out

    def forward_packed_dev(self, tok, typ, pos, cu, n_seqs: int, max_len: int, mode: int = OUT_LOGITS):
        """Forward over sequences that are already packed ON THE DEVICE (int32 torch tensors: token ids, type ids,
        position ids per token; cu_seqlens per sequence): returns a device tensor, no host hop.  Asynchronous on
        torch's current stream.  Used where the pairs are assembled on the GPU (rerank.RerankText.scores, bench.py's rerank mode).  `max_len` must
        be at least every sequence's length (`out_of_range` reports a shorter one as a ValueError)."""
        torch = self._torch
        n_tokens = int(tok.numel())
        width = self._width(mode)
        out = torch.empty((n_tokens if mode == OUT_HIDDEN else n_seqs, width), dtype=torch.float32, device=self._dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(_lib.load().rr_ce_forward_dev(
            self._h, p(tok), p(typ), p(pos), p(cu), int(n_seqs), n_tokens, int(max_len), mode, p(out),
            C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)), "rr_ce_forward_dev")
        return out

    def out_of_range(self) -> bool:
        """True when the LAST forward pass (waited for here) met a value beyond fp16's range: its logits / CLS rows are NaN
        (include/rr_hip.h: rr_ce_range_status).  `forward_ids` checks and reruns by itself; a caller of
        `forward_packed_dev` checks after it has synchronised, calls `set_wide_range(True)` and submits the batch again.
        Raises ValueError (naming max_len) instead when that pass had a sequence longer than the `max_len` it was given:
        its outputs are NaN, and the wide-range kernels would not help."""
        flag = C.c_int32()
        _lib.check(_lib.load().rr_ce_range_status(self._h, C.byref(flag)), "rr_ce_range_status")
        return bool(flag.value)

    def set_wide_range(self, on: bool = True) -> None:
        """fp32 precision only: three bf16 terms per operand and six products (any fp32 range) instead of two fp16 terms
        and three."""
        if on and not getattr(self, "_warned_wide", False):
            import warnings
            warnings.warn("encoder activations exceed the fp16 range: this handle switches to the bf16 three-term kernels")
            self._warned_wide = True
        _lib.check(_lib.load().rr_ce_set_wide_range(self._h, 1 if on else 0), "rr_ce_set_wide_range")
        self.wide_range = bool(on)

    def last_forward_ms(self) -> float:
        ms = C.c_float()
        _lib.check(_lib.load().rr_ce_last_forward_ms(self._h, C.byref(ms)), "rr_ce_last_forward_ms")
        return ms.value

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().rr_ce_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_state_dict_dir(path) -> Tuple[Dict, Optional[pathlib.Path], Dict]:
    """(state dict, vocab.txt path or None, config dict) from a local Hugging Face model directory
    (model.safetensors or pytorch_model.bin; sentence-transformers keeps the transformer in the directory root
    or in `0_Transformer/`)."""
    d = pathlib.Path(path)
    for sub in ("", "0_Transformer"):
        dd = d / sub
        if (dd / "model.safetensors").exists():
            from safetensors.numpy import load_file
            sd = load_file(str(dd / "model.safetensors"))
            break
        if (dd / "pytorch_model.bin").exists():
            import torch
            sd = torch.load(str(dd / "pytorch_model.bin"), map_location="cpu", weights_only=True)
            break
    else:
        raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {d}")
    vocab = dd / "vocab.txt"
    cfg = json.loads((dd / "config.json").read_text()) if (dd / "config.json").exists() else {}
    return sd, (vocab if vocab.exists() else None), cfg


_POOLING_FLAGS = {"pooling_mode_cls_token": "cls", "pooling_mode_mean_tokens": "mean"}


def pooling_of_dir(path) -> str:
    """"cls" or "mean": what a sentence-transformers model directory says about its pooling, `1_Pooling/config.json` beside
    the transformer (the directory root, or the parent of a `0_Transformer/` that was passed itself).  Host only.  No such
    file: "cls" (a bare Hugging Face directory; bge's pooling).  Exactly `pooling_mode_cls_token` set: "cls"; exactly
    `pooling_mode_mean_tokens`: "mean".  Anything else -- max, mean_sqrt_len, weightedmean, lasttoken, several modes
    concatenated, none at all -- is a ValueError that names the modes: the encoder has no kernel for them, and CLS rows
    returned in silence would be wrong vectors."""
    d = pathlib.Path(path)
    dirs = [d] + ([d.parent] if d.name == "0_Transformer" else [])
    f = next((x / "1_Pooling" / "config.json" for x in dirs if (x / "1_Pooling" / "config.json").exists()), None)
    if f is None:
        return "cls"
    cfg = json.loads(f.read_text())
    on = sorted(k for k, v in cfg.items() if k.startswith("pooling_mode_") and v)
    if len(on) == 1 and on[0] in _POOLING_FLAGS:
        return _POOLING_FLAGS[on[0]]
    raise ValueError(f"{f}: pooling {' + '.join(on) if on else '(no pooling_mode_* set)'} is not supported: the encoder pools "
                     "with pooling_mode_cls_token or pooling_mode_mean_tokens alone")


def model_pool_mean(hidden_rows, cu) -> np.ndarray:
    """The CPU statement of csrc/rr_ce_pool.hip's `ce_pool_mean`, bit for bit: (n_seqs, H) float32 means of the packed rows
    `hidden_rows` (sum of lengths, H) of the sequences `cu` (n_seqs + 1 offsets, every length >= 1), every operation one
    float32 rounding, in the kernel's order -- which depends on a sequence's own length only:
        p_j = 0, then p_j += row[t] for t = j, j + 8, j + 16, ... < len, in increasing t          (j = 0 .. 7)
        out = (((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))) / float32(len)"""
    h = np.ascontiguousarray(hidden_rows, dtype=np.float32)
    cu = np.asarray(cu, dtype=np.int64)
    if h.ndim != 2 or cu.ndim != 1 or len(cu) < 2 or cu[0] != 0 or cu[-1] != len(h) or (np.diff(cu) < 1).any():
        raise ValueError("model_pool_mean: rows (T, H) and cu_seqlens from 0 to T with every length >= 1")
    out = np.empty((len(cu) - 1, h.shape[1]), dtype=np.float32)
    for s in range(len(cu) - 1):
        rows = h[cu[s]:cu[s + 1]]
        p = np.zeros((8, h.shape[1]), dtype=np.float32)
        for t in range(0, len(rows), 8):                 # rows t .. t + 7 go to p_0 .. p_7: every p_j sees its rows in increasing t
            blk = rows[t:t + 8]
            p[:len(blk)] += blk
        tot = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
        out[s] = tot / np.float32(len(rows))
    return out


class CrossEncoder:
    """`sentence_transformers.CrossEncoder` on the calls the reference makes: `predict(pairs, batch_size=64,
    show_progress_bar=False)` -> float32 (len(pairs),) for a single-label model."""

    def __init__(self, state_dict: Dict, tokenizer: Optional[WordPieceTokenizer] = None, *, device: int = 0,
                 max_length: int = 512, activation: Optional[str] = None, ln_eps: float = 1e-12, precision: str = "fp32",
                 n_heads: Optional[int] = None):
        """``precision`` "fp32" (default: the reference reranks in fp32, app/app_product_search.py:277-278) or "bf16"
        (fast path, logits within 2.5e-2; hidden 384 / 12 heads / FFN 1536 only): see BertEncoderGPU, also for ``n_heads``."""
        self.model = BertEncoderGPU(state_dict, device=device, ln_eps=ln_eps, with_head=True, precision=precision, n_heads=n_heads)
        if self.model.n_labels < 1:
            raise ValueError("the state dict has no pooler / classifier: not a sequence-classification checkpoint")
        self.tokenizer = tokenizer
        self.max_length = min(int(max_length), self.model.max_pos)
        if activation not in (None, "identity", "sigmoid"):
            raise ValueError("activation must be None / 'identity' / 'sigmoid'")
        self.activation = activation

    @classmethod
    def from_pretrained_dir(cls, path, **kw) -> "CrossEncoder":
        sd, vocab, cfg = load_state_dict_dir(path)
        tok = WordPieceTokenizer.from_vocab_file(vocab) if vocab else None
        kw.setdefault("ln_eps", float(cfg.get("layer_norm_eps", 1e-12)))
        if cfg.get("num_attention_heads") is not None:
            kw.setdefault("n_heads", int(cfg["num_attention_heads"]))
        return cls(sd, tok, **kw)

    def _post(self, logits: np.ndarray) -> np.ndarray:
        x = logits[:, 0] if logits.shape[1] == 1 else logits
        if self.activation == "sigmoid":
            x = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)
        return x

    def predict_ids(self, seqs: Sequence[Tuple[Sequence[int], Sequence[int]]]) -> np.ndarray:
        """Scores of pre-tokenised `[CLS] query [SEP] text [SEP]` sequences (token ids, type ids)."""
        if len(seqs) == 0:
            return np.zeros(0, dtype=np.float32)
        return self._post(self.model.forward_ids(seqs, OUT_LOGITS))

    def tokenize_pairs(self, pairs: Sequence[Tuple[str, str]]):
        if self.tokenizer is None:
            raise ValueError("no vocabulary was loaded: pass pre-tokenised ids to predict_ids, or construct with a "
                             "WordPieceTokenizer (vocab.txt)")
        return [self.tokenizer.encode_pair(str(a), str(b), self.max_length) for a, b in pairs]

    def predict(self, pairs, batch_size: int = 64, show_progress_bar: bool = False, **_ignored) -> np.ndarray:
        """(query, text) string pairs -> scores.  `batch_size` only bounds host-side tokenisation here: the packed
        forward has no padding, so the scores do not depend on how pairs are batched (in the reference they do not
        either, up to fp32 rounding: padding positions are masked)."""
        if len(pairs) == 0:
            return np.zeros(0, dtype=np.float32)
        return self.predict_ids(self.tokenize_pairs(pairs))


class QueryEncoder:
    """`SentenceTransformer` on the call the reference makes: `encode([query], normalize_embeddings=True)` ->
    (n, hidden) float32 (384 for bge-small-en-v1.5; `.hidden`).  `.pooling`: "cls" (last_hidden_state[:, 0]: bge's pooling
    config, the default) or "mean" (the mean over a sequence's tokens: all-MiniLM, multi-qa-MiniLM, e5, gte), `.out_mode` the
    forward's output mode for it (OUT_CLS / OUT_MEAN); both pool on the device.  `from_pretrained_dir` reads the directory's
    `1_Pooling/config.json` (`pooling_of_dir`) and refuses every other pooling.  Not applied here: prompts / prefixes
    ("query: " of e5) -- the caller's -- and a `2_Normalize` module (`normalize_embeddings` is the caller's, and the
    reference always passes True)."""

    def __init__(self, state_dict: Dict, tokenizer: Optional[WordPieceTokenizer] = None, *, device: int = 0,
                 max_length: int = 512, ln_eps: float = 1e-12, precision: str = "fp32", n_heads: Optional[int] = None,
                 pooling: str = "cls"):
        """``pooling`` "cls" | "mean" (the class docstring).  ``precision`` "fp32" by default: the query vector feeds K1, whose answers are held to a 4e-7 tie band -- a bf16
        encoder would move dense scores by ~2e-3 (one short sequence per query: the fp32 forward costs microseconds)."""
        if pooling not in POOLINGS:
            raise ValueError(f"pooling must be one of {sorted(POOLINGS)}, not {pooling!r}")
        self.pooling, self.out_mode = pooling, POOLINGS[pooling]
        self.model = BertEncoderGPU(state_dict, device=device, ln_eps=ln_eps, with_head=False, precision=precision, n_heads=n_heads)
        self.hidden = self.model.hidden                 # the width of the vectors: an index's `dim`
        self.tokenizer = tokenizer
        self.max_length = min(int(max_length), self.model.max_pos)

    @classmethod
    def from_pretrained_dir(cls, path, **kw) -> "QueryEncoder":
        sd, vocab, cfg = load_state_dict_dir(path)
        tok = WordPieceTokenizer.from_vocab_file(vocab) if vocab else None
        kw.setdefault("ln_eps", float(cfg.get("layer_norm_eps", 1e-12)))
        if cfg.get("num_attention_heads") is not None:
            kw.setdefault("n_heads", int(cfg["num_attention_heads"]))
        if kw.get("pooling") in (None, "auto"):         # (not passed: the directory's; an unsupported one is refused there)
            kw["pooling"] = pooling_of_dir(path)
        return cls(sd, tok, **kw)

    def encode_ids(self, seqs, normalize_embeddings: bool = False) -> np.ndarray:
        e = self.model.forward_ids(seqs, self.out_mode)
        if normalize_embeddings:       # torch.nn.functional.normalize(p=2, dim=1, eps=1e-12)
            e = (e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)).astype(np.float32)
        return e

    def encode_dev(self, tok, typ, pos, cu, n_seqs: int, max_len: int):
        """Pooled rows (n_seqs, hidden), a DEVICE tensor, of sequences already packed on the device (embed.DeviceWordPiece makes
        them from text): `forward_packed_dev` with `.out_mode` (CLS rows or token means), asynchronous on torch's current
        stream, not normalised."""
        return self.model.forward_packed_dev(tok, typ, pos, cu, n_seqs, max_len, self.out_mode)

    def encode(self, sentences, normalize_embeddings: bool = False, **_ignored) -> np.ndarray:
        if self.tokenizer is None:
            raise ValueError("no vocabulary was loaded: pass pre-tokenised ids to encode_ids")
        single = isinstance(sentences, str)
        seqs = [self.tokenizer.encode_pair(s, None, self.max_length) for s in ([sentences] if single else sentences)]
        e = self.encode_ids(seqs, normalize_embeddings)
        return e[0] if single else e
