#!/usr/bin/env python3
"""Generates tests/golden/k5_mean_pooling.npz: MEAN-pooled sentence vectors of Hugging Face `transformers` BertModel on seeded
random weights, in the manner of make_k5_golden.py.

    python tests/golden/make_k5_pooling_golden.py          (build container only: needs `transformers` + torch CPU)

Two models, 2 layers each, the seeded numpy weights of review-recommender_amd/synth.py::bert_state_dict (no pooler, prefix ""):

  h384   hidden 384 / 12 heads / FFN 1536     (all-MiniLM's block shape: the encoder's kernels of both precisions)
  h128   hidden 128 /  2 heads / FFN  512     (the runtime-shape kernels)

over ONE vocabulary -- [PAD] [UNK] [CLS] [SEP] [MASK] + synth.WORDS, piece i = id i, so that " ".join(words[id]) of a sequence's
inner ids tokenises back to it -- and ONE set of eight sequences of 1, 2, 3, 9, 17, 64, 65 and 128 tokens ([CLS] alone, [CLS]
[SEP], then [CLS] words [SEP]), run as one PADDED batch with its attention mask, fp32 on CPU.  The expected rows are what
sentence-transformers' Pooling(pooling_mode_mean_tokens) + Normalize give:

    (h * mask).sum(1) / mask.sum(1).clamp(min=1e-9), then torch.nn.functional.normalize(p=2, dim=1)

Only seeds, token ids and outputs are stored (weights are regenerated from the seed).
"""
import pathlib
import sys

import numpy as np
import torch
from transformers import BertConfig, BertModel

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from review_recommender_amd import synth  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent
LENGTHS = (1, 2, 3, 9, 17, 64, 65, 128)
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
SHAPES = {"h384": (20253, 384, 12, 1536), "h128": (20254, 128, 2, 512)}       # seed, hidden, heads, ffn
N_LAYERS = 2


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    words = SPECIALS + list(synth.WORDS)
    assert len(set(words)) == len(words)
    vocab = len(words)
    rng = np.random.default_rng(6)
    seqs = []
    for n in LENGTHS:
        ids = np.concatenate([[2], rng.integers(len(SPECIALS), vocab, max(n - 2, 0)), [3]])[:n].astype(np.int32)
        seqs.append(ids)
    L = max(LENGTHS)
    ids = np.zeros((len(seqs), L), dtype=np.int64)
    mask = np.zeros((len(seqs), L), dtype=np.int64)
    for r, s in enumerate(seqs):
        ids[r, :len(s)], mask[r, :len(s)] = s, 1
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    cu = np.zeros(len(seqs) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in seqs], out=cu[1:])
    out = dict(n_layers=N_LAYERS, vocab=vocab, token_ids=np.concatenate(seqs).astype(np.int32), cu_seqlens=cu)
    for name, (seed, hidden, heads, ffn) in SHAPES.items():
        sd = synth.bert_state_dict(seed, n_layers=N_LAYERS, hidden=hidden, ffn=ffn, vocab=vocab, n_labels=0, prefix="")
        cfg = BertConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=N_LAYERS, num_attention_heads=heads,
                         intermediate_size=ffn, max_position_embeddings=512)
        enc = BertModel(cfg, add_pooling_layer=False).eval()
        missing = enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys), missing
        h = enc(input_ids=ids, token_type_ids=torch.zeros_like(ids), attention_mask=mask).last_hidden_state
        m = mask.unsqueeze(-1).to(h.dtype)
        mean = (h * m).sum(1) / m.sum(1).clamp(min=1e-9)
        emb = torch.nn.functional.normalize(mean, p=2, dim=1)
        out.update({f"{name}_seed": seed, f"{name}_shape": np.array([hidden, heads, ffn], dtype=np.int32),
                    f"{name}_mean_raw": mean.numpy().astype(np.float32), f"{name}_embeddings": emb.numpy().astype(np.float32)})
        print(name, "mean-pooled:", len(seqs), "sequences, |mean| =", np.linalg.norm(mean.numpy(), axis=1)[:3])
    np.savez_compressed(OUT / "k5_mean_pooling.npz", **out)


if __name__ == "__main__":
    main()
