// rr_ce_pool.h -- K5's mean pooling (csrc/rr_ce_pool.hip) as rr_ce.hip's four forward passes launch it.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// out [n_seqs][hidden] = the mean over its tokens of every packed sequence of h32 [T][hidden] (cu_seqlens [n_seqs + 1], every
// length >= 1; hidden % 128 == 0).  `flag` non-NULL and raised on the device: every row of the call is NaN instead.
void ce_pool_mean(const float* h32, const int32_t* cu, int n_seqs, int hidden, float* out, const unsigned* flag, hipStream_t st);
