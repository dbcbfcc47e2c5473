// rr_ce_pool.hip -- K5's mean pooling (RR_CE_OUT_MEAN): the sentence vector of the BERT-family encoders that are published
// with `pooling_mode_mean_tokens` (all-MiniLM, multi-qa-MiniLM, e5, gte), at every width of the family (rr_ce_w.h).
//
//   ce_pool_mean   out[s][c] = (sum over t < len_s of h32[cu[s] + t][c]) / float(len_s), fp32
//
// sentence-transformers computes (h * mask).sum(1) / clamp(mask.sum(1), min = 1e-9) over a PADDED batch.  The packed rows have
// no padding, so the masked sum is the sum of a sequence's own rows, and every sequence has at least one token ([CLS]): the
// clamp never acts and is not written here.
//
// The ORDER of the sum is part of the contract (cross_encoder.model_pool_mean states it on the CPU, bit for bit).  It depends
// on the sequence's own length and on nothing else -- not on where the sequence sits in the batch, not on what else is in it:
//   p_j = 0.f, then p_j += h[t] for t = j, j + 8, j + 16, ... < len in increasing t         (j = 0 .. 7)
//   sum = ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))
//   out = sum / float(len)                                                                   (one IEEE division)
// No atomics, no fused multiply-add (there is no product), one workgroup per (sequence, 128-column slab).
//
// A streaming read of len x hidden x 4 bytes and a write of hidden x 4: thread group j = tid / 32 owns the tokens t = j mod 8,
// a thread 4 consecutive columns -- one 16-byte load per row, the 32 threads of a group a whole 512-byte slab row.  Four rows'
// loads are issued before the first is added, the additions stay in the order above.
#include <vector>

#include "rr_common.h"
#include "rr_ce_pool.h"

typedef float ce_pool_f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void ce_pool_mean_k(const float* __restrict__ h32, const int32_t* __restrict__ cu, int H,
                                                      float* __restrict__ out, const unsigned* __restrict__ flag) {
    __shared__ ce_pool_f4 part[8][32];
    const int tid = threadIdx.x, j = tid >> 5, c4 = tid & 31, seq = blockIdx.x, col = blockIdx.y * 128 + 4 * c4;
    if (flag && *flag) {                                   // (rr_ce_h2.hip: a value left the fp16 range: no finite answer)
        if (j == 0) {
            const float nan = __builtin_nanf("");
            *reinterpret_cast<ce_pool_f4*>(out + (int64_t)seq * H + col) = ce_pool_f4{nan, nan, nan, nan};
        }
        return;
    }
    const int t0 = cu[seq], len = cu[seq + 1] - t0;
    const float* src = h32 + (int64_t)t0 * H + col;
    ce_pool_f4 p = {0.f, 0.f, 0.f, 0.f};
    int t = j;
    for (; t + 24 < len; t += 32) {
        const ce_pool_f4 a = *reinterpret_cast<const ce_pool_f4*>(src + (int64_t)t * H);
        const ce_pool_f4 b = *reinterpret_cast<const ce_pool_f4*>(src + (int64_t)(t + 8) * H);
        const ce_pool_f4 c = *reinterpret_cast<const ce_pool_f4*>(src + (int64_t)(t + 16) * H);
        const ce_pool_f4 d = *reinterpret_cast<const ce_pool_f4*>(src + (int64_t)(t + 24) * H);
        p += a;
        p += b;
        p += c;
        p += d;
    }
    for (; t < len; t += 8) p += *reinterpret_cast<const ce_pool_f4*>(src + (int64_t)t * H);
    part[j][c4] = p;
    __syncthreads();
    if (j == 0) {
        const ce_pool_f4 s = ((part[0][c4] + part[1][c4]) + (part[2][c4] + part[3][c4])) +
                             ((part[4][c4] + part[5][c4]) + (part[6][c4] + part[7][c4]));
        const float n = (float)len;
        *reinterpret_cast<ce_pool_f4*>(out + (int64_t)seq * H + col) = ce_pool_f4{s.x / n, s.y / n, s.z / n, s.w / n};
    }
}

void ce_pool_mean(const float* h32, const int32_t* cu, int n_seqs, int hidden, float* out, const unsigned* flag, hipStream_t st) {
    hipLaunchKernelGGL(ce_pool_mean_k, dim3((unsigned)n_seqs, (unsigned)(hidden / 128)), dim3(256), 0, st, h32, cu, hidden, out, flag);
}

#ifdef RR_DEBUG_HARNESS
// tests/test_gpu_k5_pool_kernel.py, tools/pooling_time.py: ONE ce_pool_mean launch on caller rows (device pointers: h32 [T][hidden]
// fp32, cu_seqlens [n_seqs + 1]), through the launcher the forward passes call, no flag.  Checked here, on a host copy of cu,
// before anything is launched (the kernel trusts them): cu runs from 0 to T without a step back, every length is in [1, 512],
// hidden % 128 == 0 in [128, 1024].  Waits for the launch.
extern "C" int rr_debug_ce_pool_mean(const float* d_h32, int32_t T, const int32_t* d_cu, int32_t n_seqs, int32_t hidden, float* d_out) {
    RR_REQUIRE(d_h32 && d_cu && d_out, "rr_debug_ce_pool_mean: NULL argument");
    RR_REQUIRE(T >= 1 && n_seqs >= 1 && n_seqs <= T, "rr_debug_ce_pool_mean: %d sequences / %d tokens", n_seqs, T);
    RR_REQUIRE(hidden >= 128 && hidden <= 1024 && hidden % 128 == 0, "rr_debug_ce_pool_mean: hidden %d is not a multiple of 128 in [128, 1024]",
               hidden);
    std::vector<int32_t> cu((size_t)n_seqs + 1);
    RR_HIP_TRY(hipMemcpy(cu.data(), d_cu, sizeof(int32_t) * cu.size(), hipMemcpyDeviceToHost));
    RR_REQUIRE(cu[0] == 0 && cu[n_seqs] == T, "rr_debug_ce_pool_mean: cu_seqlens run from %d to %d, not from 0 to %d", cu[0], cu[n_seqs], T);
    for (int i = 0; i < n_seqs; ++i)
        RR_REQUIRE(cu[i + 1] - cu[i] >= 1 && cu[i + 1] - cu[i] <= 512, "rr_debug_ce_pool_mean: sequence %d has %d tokens, outside [1, 512]", i,
                   cu[i + 1] - cu[i]);
    ce_pool_mean(d_h32, d_cu, n_seqs, hidden, d_out, nullptr, nullptr);
    RR_HIP_TRY(hipGetLastError());
    RR_HIP_TRY(hipDeviceSynchronize());
    return RR_OK;
}

// tools/pooling_time.py: HIP-event times of `reps` ce_pool_mean launches (ms_pool[reps]) and, in the same run, of `reps`
// device-to-device hipMemcpyAsync of the same T x hidden floats into d_copy (ms_copy[reps]: what RR_CE_OUT_HIDDEN does with
// them), alternating, one event pair per launch after `warmup` untimed ones of each.  The arguments are rr_debug_ce_pool_mean's.
extern "C" int rr_debug_ce_pool_time(const float* d_h32, int32_t T, const int32_t* d_cu, int32_t n_seqs, int32_t hidden, float* d_out,
                                     float* d_copy, int32_t warmup, int32_t reps, float* ms_pool, float* ms_copy) {
    RR_REQUIRE(d_copy && ms_pool && ms_copy && warmup >= 0 && reps >= 1, "rr_debug_ce_pool_time: bad arguments");
    if (int rc = rr_debug_ce_pool_mean(d_h32, T, d_cu, n_seqs, hidden, d_out)) return rc;      // (checks everything; the first warm-up)
    const size_t bytes = sizeof(float) * (size_t)T * hidden;
    hipEvent_t e0, e1;
    RR_HIP_TRY(hipEventCreate(&e0));
    RR_HIP_TRY(hipEventCreate(&e1));
    int rc = RR_OK;
    for (int i = -warmup; i < reps && rc == RR_OK; ++i)      // the two alternate: a drift of the clocks meets both alike
        for (int what = 0; what < 2 && rc == RR_OK; ++what) {
            hipError_t e = hipEventRecord(e0, nullptr);
            if (what == 0) ce_pool_mean(d_h32, d_cu, n_seqs, hidden, d_out, nullptr, nullptr);
            else if (e == hipSuccess) e = hipMemcpyAsync(d_copy, d_h32, bytes, hipMemcpyDeviceToDevice, nullptr);
            if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e != hipSuccess) { rr_set_error("rr_debug_ce_pool_time: %s", hipGetErrorString(e)); rc = RR_E_HIP; }
            else if (i >= 0) (what == 0 ? ms_pool : ms_copy)[i] = ms;
        }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return rc;
}
#endif
