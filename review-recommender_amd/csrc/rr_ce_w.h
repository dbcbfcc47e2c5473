// rr_ce_w.h -- K5 at encoder shapes other than hidden 384 / 12 heads / FFN 1536: the runtime-shape kernels of
// csrc/rr_ce_w.hip as rr_ce.hip's host side (ce_forward_w) launches them.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The family: hidden % 128 == 0 in [128, 1024], hidden / n_heads 32 or 64, ffn % 128 == 0 in [128, 4096].
#define CE_W_MAX_H 1024
#define CE_W_MAX_FFN 4096

// 0 when (hidden, n_heads, ffn) is in the family; else RR_E_INVALID with rr_set_error naming the offending number
// (`who` leads the message).  with_ffn = false: ffn is not looked at (the attention's kernel-test entry has none).
int ce_w_check_shape(const char* who, int hidden, int n_heads, int ffn, bool with_ffn);
// per-device opt-in to the attention's dynamic LDS (the current device)
int ce_w_set_attributes();
// h32 [T][hidden] = LayerNorm(word[tok] + type[typ] + pos[pos]) * g + b
void ce_w_embed_ln(const int32_t* tok, const int32_t* typ, const int32_t* pos, int T, int hidden, int vocab, int n_pos, int n_typ,
                   const float* we, const float* pe, const float* te, const float* g, const float* b, float eps, float* h32,
                   hipStream_t st);
// FFN-2 sums over K = ffn in chunks of at most this many columns, one ce_gemm_x3 launch each, and the residual LayerNorm adds
// the partial products (ce_forward_w): a one-accumulator sum over 4096 k is twice numpy float32's error, blocked it is not.
// An FFN of up to 2048 is one launch as before.
#define CE_W_KCHUNK 2048
// The largest call: ce_gemm_x3's grid has ceil(T / 128) rows of workgroups, and a grid's y extent ends at 65 535
#define CE_W_MAX_TOKENS (65535ll * 128)
// h32 [T][hidden] = LayerNorm(y + h32) * g + b, in place; y = the sum of `parts` arrays [T][hidden], `pstride` floats apart
void ce_w_add_ln(const float* y, int parts, int64_t pstride, float* h32, int T, int hidden, const float* g, const float* b, float eps,
                 hipStream_t st);
// ctx [T][hidden] = softmax(Q K^T / sqrt(hd)) V per (sequence, head), qkv [T][3 hidden] fp32 (Q unscaled, then K, then V);
// every sequence of cu_seqlens has 1 .. 512 tokens
void ce_w_attention(const float* qkv, const int32_t* cu, int n_seqs, int hidden, int n_heads, float* ctx, hipStream_t st);
// mode RR_CE_OUT_CLS: out [n_seqs][hidden] = h32[cu[seq]]; RR_CE_OUT_LOGITS: out [n_seqs][n_labels] = wc tanh(wp x + bp) + bc
// (the two [CLS]-row modes only: RR_CE_OUT_HIDDEN is a copy and RR_CE_OUT_MEAN is rr_ce_pool.h's ce_pool_mean, both in ce_forward_w)
void ce_w_head(const float* h32, const int32_t* cu, int n_seqs, int hidden, const float* wp, const float* bp, const float* wc,
               const float* bc, int n_labels, int mode, float* out, hipStream_t st);
