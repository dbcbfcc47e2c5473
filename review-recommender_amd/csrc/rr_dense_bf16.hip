// rr_dense_bf16.hip -- K1 over a bf16-stored matrix (BASELINE configs 4-5).
//
// The reference has no bf16 path.  The semantics here are the ones SURVEY 8d fixes: the matrix
// is rounded to bf16 ONCE (round-to-nearest-even, after the fp32 l2 normalisation), queries stay
// fp32, every product is an exact fp32 product of an exactly-representable bf16 row element and
// an fp32 query element, accumulation is fp32.  The oracle is the fp32 matvec over the rounded
// matrix upcast to fp32.  Storage halves the bytes per row (768 B at dim 384), so the HBM-bound
// scans run at twice the rows per second; the selection (rr_select) is unchanged.
//
// rr_scan_bf16<NB>      1..8 queries per matrix read, VALU.  Same shape as rr_scan_f32: a
//                       16-lane DPP row owns a matrix row, lane j loads 16 B (8 bf16) chunks
//                       j, j+16, j+32 (a wave instruction = four rows x 256 contiguous bytes),
//                       the per-row chain of rr_dense.h over them.
// Batches of 5 and more queries over the same storage run on the matrix cores: the filter scan
// (rr_dense_flt.hip) and the exact split-operand scans (rr_dense_x3.hip, rr_dense_x3w.hip).
#include "rr_common.h"
#include "rr_dense.h"

// ------------------------------------------------------------------ fp32 -> bf16 rows
// Round to nearest even on the f32 bits; NaN stays a (quiet) NaN.
__device__ __forceinline__ unsigned int rr_f32_to_bf16_bits(float f) {
    const unsigned int u = __float_as_uint(f);
    if (f != f) return (u >> 16) | 0x0040u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// One wave per row: optional l2 normalisation in fp32 (utils.py:40-44), then rounding.
__global__ void rr_rows_to_bf16(const float* __restrict__ src, int dim, unsigned short* __restrict__ dst,
                                int dim_pad, int64_t n_rows, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const float* p = src + row * dim;
    float scale = 1.f;
    if (eps > 0.f) {
        float ss = 0.f;
        for (int i = lane; i < dim; i += 64) ss = __builtin_fmaf(p[i], p[i], ss);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
        scale = fmaxf(sqrtf(ss), eps);
    }
    unsigned short* d = dst + row * dim_pad;
    for (int i = lane; i < dim_pad; i += 64) {
        const float v = i < dim ? (eps > 0.f ? p[i] / scale : p[i]) : 0.f;
        d[i] = (unsigned short)rr_f32_to_bf16_bits(v);
    }
}

int rr_store_rows_bf16_at(void* d_dst, int32_t dim, int32_t dim_pad, int64_t n, const float* d_rows_f32, float eps, hipStream_t st) {
    if (n == 0) return RR_OK;
    hipLaunchKernelGGL(rr_rows_to_bf16, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, d_rows_f32, dim,
                       reinterpret_cast<unsigned short*>(d_dst), dim_pad, n, eps);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

int rr_store_rows_bf16(rr_index* ix, int64_t first_row, int64_t n, float* d_rows_f32, float eps, hipStream_t st) {
    return rr_store_rows_bf16_at(reinterpret_cast<unsigned short*>(ix->d_matrix) + first_row * ix->dim_pad, ix->dim, ix->dim_pad, n,
                                 d_rows_f32, eps, st);
}

// ------------------------------------------------------------------ VALU scan, dim 384
template <int NB>
__global__ __launch_bounds__(RR_SCAN_THREADS, (NB <= 1 ? 4 : 2)) void rr_scan_bf16(
    const u32x4* __restrict__ mat, rr_scan_geom G, const float* __restrict__ queries,  // NB x 384
    float* __restrict__ sims, float* __restrict__ gmax, uint32_t* __restrict__ smax) {
    constexpr int ROWC = 48;                  // 16-byte chunks per row
    __shared__ f32x4 qs[NB][96];
    const int tid = threadIdx.x;
    for (int i = tid; i < NB * 96; i += RR_SCAN_THREADS) qs[i / 96][i % 96] = reinterpret_cast<const f32x4*>(queries)[i];
    __syncthreads();

    const int lane = tid & 63;
    const int sub = lane & 15;
    const int grp = lane >> 4;
    const int64_t wave = (int64_t)blockIdx.x * (RR_SCAN_THREADS / 64) + (tid >> 6);
    if (wave >= G.n_waves) return;
    const int64_t t0 = wave * G.tiles_per_wave;
    const int64_t t1 = t0 + G.tiles_per_wave < G.n_tiles ? t0 + G.tiles_per_wave : G.n_tiles;

    // chunk c = sub + 16*i holds elements 8c .. 8c+7 = float4 2c and 2c+1 of the query
    f32x4 qreg[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        qreg[2 * i] = (NB == 1) ? qs[0][2 * (sub + 16 * i)] : f32x4{0.f, 0.f, 0.f, 0.f};
        qreg[2 * i + 1] = (NB == 1) ? qs[0][2 * (sub + 16 * i) + 1] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    auto load_rows = [&](u32x4 (&dst)[3], int64_t row) {
        row = row < G.n_rows ? row : G.n_rows - 1;
        const u32x4* p = mat + row * ROWC + sub;
#pragma unroll
        for (int i = 0; i < 3; ++i) dst[i] = __builtin_nontemporal_load(p + 16 * i);
    };
    float gm[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) gm[b] = -INFINITY;

    u32x4 bufA[3], bufB[3];
    load_rows(bufA, t0 * 64 + grp);
#pragma unroll 1
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t row0 = tile * 64;
        float mine[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) mine[b] = 0.f;
#pragma unroll(NB == 1 ? 8 : 1)
        for (int it = 0; it < 16; it += 2) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                u32x4(&cur)[3] = half ? bufB : bufA;
                u32x4(&nxt)[3] = half ? bufA : bufB;
                load_rows(nxt, row0 + 4 * (it + half + 1) + grp);      // it + half == 15: next tile's first rows
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (NB > 1) asm volatile("" ::: "memory");          // keep one query slice live, re-read LDS
                    float acc = 0.f;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const f32x4 q0 = (NB == 1) ? qreg[2 * i] : qs[b][2 * (sub + 16 * i)];
                        const f32x4 q1 = (NB == 1) ? qreg[2 * i + 1] : qs[b][2 * (sub + 16 * i) + 1];
                        acc = rr_bf16_chunk(cur[i], q0, q1, acc);
                    }
                    acc = rr_row16_sum(acc);
                    mine[b] = (sub == it + half) ? acc : mine[b];
                }
            }
        }
        // (rr_finish_tile's work, written out: through the shared helper this kernel's registers and schedule change)
        const int64_t my_row = row0 + 4 * sub + grp;
        const bool valid = my_row < G.n_rows;
        const bool group_end = tile == t1 - 1;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float v = mine[b];
            v = rr_rank_last(v, valid);
            sims[(int64_t)b * G.n_pad + my_row] = v;
            const float m = rr_wave_max(v);
            gm[b] = fmaxf(gm[b], m);
            if (lane == 0) {
                gmax[(int64_t)b * G.n_tiles + tile] = m;
                if (group_end) smax[(int64_t)b * G.n_waves + wave] = rr_f2key(gm[b]);
            }
        }
    }
}

int rr_launch_scan_bf16(rr_index* ix, const float* d_q, int nb, hipStream_t st, rr_scan_geom* out) {
    static constexpr decltype(&rr_scan_bf16<1>) kern[4] = {rr_scan_bf16<1>, rr_scan_bf16<2>, rr_scan_bf16<4>, rr_scan_bf16<8>};
    static int waves[4];   // per kernel instance
    const int k = rr_nb_slot(nb);
    if (!waves[k]) waves[k] = rr_resident_waves((const void*)kern[k], RR_SCAN_THREADS, ix->device);
    const rr_scan_geom G = *out = rr_make_geom(ix, waves[k] / 4);
    hipLaunchKernelGGL(kern[k], dim3((G.n_waves + 3) / 4), dim3(RR_SCAN_THREADS), 0, st,
                       reinterpret_cast<const u32x4*>(ix->d_matrix), G, d_q, ix->d_sims, ix->d_gmax, ix->d_smax);
    return RR_OK;
}
