// rr_dense_bf16w.hip -- K1 over a bf16-stored matrix at a RUNTIME WIDTH: dim_pad = 64, 128, .. 1024 other than 384 (the
// 384-wide rr_scan_bf16 keeps every constant it has).  Semantics of rr_dense_bf16.hip: rows rounded once to bf16, queries
// and accumulation fp32, every product an exact fp32 product.
//
// The per-row chain is the one rr_dense.h defines (rr_bf16_chunk), at D / 8 chunks per row; at D = 384 it is rr_scan_bf16's.
// Three places run it here: rr_scan_bf16_generic (the single-query scan, and 2 .. 8 queries per read where the batched path
// declines), its listed form (flagged queries of a batched launch) and rr_rescore_chain_wb (rr_dense_fltw.hip).
#include "rr_x3.h"

// ------------------------------------------------------------------ the VALU scan
// Geometry and outputs of rr_scan_bf16: a wave owns a run of 64-row tiles, walks a tile in 16 steps of four rows (16 lanes
// per row), keeps row 4 it + grp in lane (it, grp) and ends the tile with rr_finish_tile.  The width is not known at compile
// time, so a row is not a register array: the wave's work is a stream of STAGES, stage = (4-row step, round i) = one 16-byte
// load per lane (four rows x 256 contiguous bytes per wave instruction), nr = ceil(units / 16) stages per step.  A ring of
// RING stages rotates by name (the loop body is unrolled RING times): while one stage is multiplied the loads of the next
// RING - 1 -- of this step's later rounds, then of the next rows, across tile seams -- are in flight; the compiler counts
// the waits.  16 nr stages per tile is a multiple of RING, so a tile always ends with the ring's last slot: rr_finish_tile
// stands once, behind the unrolled body.  The queries sit in LDS (fp32, memory order); the four rows of a wave read the same
// 16 addresses per ds_read_b128 (broadcast).  Registers: 32 ring + 8 query + 3 NB sums + addressing: no spills at NB = 8.
#define RR_BF16W_RING 8
static_assert(16 % RR_BF16W_RING == 0, "16 nr stages per tile must be a multiple of the ring: rr_finish_tile stands once, behind the unrolled body");
template <int NB>
__device__ __forceinline__ void rr_bf16w_scan_rows(const u32x4* __restrict__ mat, const rr_scan_geom& G, int units,
                                                   const f32x4 (*qs)[RR_FLTW_MAX_DIM / 4], float* __restrict__ sims,
                                                   float* __restrict__ gmax, uint32_t* __restrict__ smax) {
    constexpr int RING = RR_BF16W_RING;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int sub = lane & 15;
    const int grp = lane >> 4;
    const int64_t wave = (int64_t)blockIdx.x * (RR_SCAN_THREADS / 64) + (tid >> 6);
    if (wave >= G.n_waves) return;
    const int64_t t0 = wave * G.tiles_per_wave;
    const int64_t t1 = t0 + G.tiles_per_wave < G.n_tiles ? t0 + G.tiles_per_wave : G.n_tiles;
    const int nr = (units + 15) >> 4;                 // rounds per row; units is a multiple of 8: the last one is full or half full

    // the stage the next fetch brings: 4-row step pf_step (= 16 tile + it), round pf_i.  Past the run's end: the matrix's last
    // row again, never multiplied.  A chunk that does not exist: an address inside the row, never multiplied.
    int64_t pf_step = t0 * 16;
    int pf_i = 0;
    auto fetch = [&](u32x4& d) {
        int64_t row = pf_step * 4 + grp;
        row = row < G.n_rows ? row : G.n_rows - 1;
        int c = sub + 16 * pf_i;
        c = c < units ? c : (sub & 7);
        d = __builtin_nontemporal_load(mat + row * units + c);
        if (++pf_i == nr) {
            pf_i = 0;
            ++pf_step;
        }
    };

    float gm[NB], mine[NB], acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        gm[b] = -INFINITY;
        mine[b] = 0.f;
        acc[b] = 0.f;
    }
    int it = 0, i = 0;                                // the stage being multiplied: step `it` of its tile, round i
    auto multiply = [&](const u32x4& x) {
        const int c = sub + 16 * i;
        if (c < units) {
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = rr_bf16_chunk(x, qs[b][2 * c], qs[b][2 * c + 1], acc[b]);
        }
        if (++i == nr) {                              // (wave-uniform) the step's rows are complete
            i = 0;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float s = rr_row16_sum(acc[b]);
                mine[b] = (sub == it) ? s : mine[b];
                acc[b] = 0.f;
            }
            ++it;
        }
    };

    u32x4 ring[RING];
#pragma unroll
    for (int k = 0; k < RING; ++k) fetch(ring[k]);
    int64_t tile = t0;
#pragma unroll 1
    while (tile < t1) {
#pragma unroll
        for (int k = 0; k < RING; ++k) {
            multiply(ring[k]);
            fetch(ring[k]);
        }
        if (it == 16) {
            rr_finish_tile<NB>(G, tile, wave, t0, t1, lane, sub, grp, mine, gm, sims, gmax, smax);
#pragma unroll
            for (int b = 0; b < NB; ++b) mine[b] = 0.f;
            it = 0;
            ++tile;
        }
    }
}

// NB = 1, 2, 4, 8 queries per read of the matrix; queries: NB x dim_pad fp32, padded
template <int NB>
__global__ __launch_bounds__(RR_SCAN_THREADS) void rr_scan_bf16_generic(
    const u32x4* __restrict__ mat, rr_scan_geom G, int units, const float* __restrict__ queries,
    float* __restrict__ sims, float* __restrict__ gmax, uint32_t* __restrict__ smax) {
    __shared__ f32x4 qs[NB][RR_FLTW_MAX_DIM / 4];
    const int q4 = 2 * units;                         // float4s per query
    for (int i = threadIdx.x; i < NB * q4; i += RR_SCAN_THREADS)
        qs[i / q4][i % q4] = reinterpret_cast<const f32x4*>(queries)[i];
    __syncthreads();
    rr_bf16w_scan_rows<NB>(mat, G, units, qs, sims, gmax, smax);
}

// The LISTED form: the NB queries are the flagged ones ranked [skip, skip + NB) of a wide filter launch, read in place from
// the launch's padded queries (rr_scan_f32_generic_listed for bf16 rows).  The chain is the one above, so a flagged query's
// answer is bit for bit the single-query answer.  An empty slice: every workgroup returns at once.
template <int NB>
__global__ __launch_bounds__(RR_SCAN_THREADS) void rr_scan_bf16_generic_listed(
    const u32x4* __restrict__ mat, rr_scan_geom G, int units, const float* __restrict__ queries,
    float* __restrict__ sims, float* __restrict__ gmax, uint32_t* __restrict__ smax,
    const int32_t* __restrict__ flags, int nq_total, int skip, int32_t* __restrict__ list_out) {
    __shared__ f32x4 qs[NB][RR_FLTW_MAX_DIM / 4];
    const int tid = threadIdx.x;
    int list[NB];
    const int n = rr_flagged_slice<NB>(flags, nq_total, tid & 63, skip, list);
    rr_publish_list<NB>(list_out, n, list);
    if (n == 0) return;                               // (the whole workgroup: before the barrier)
    const int q4 = 2 * units;
#pragma unroll
    for (int b = 0; b < NB; ++b)
        for (int i = tid; i < q4; i += RR_SCAN_THREADS) qs[b][i] = reinterpret_cast<const f32x4*>(queries)[(int64_t)list[b] * q4 + i];
    __syncthreads();
    rr_bf16w_scan_rows<NB>(mat, G, units, qs, sims, gmax, smax);
}

// ------------------------------------------------------------------ host side
int rr_launch_scan_bf16w(rr_index* ix, const float* d_q, int nb, hipStream_t st, rr_scan_geom* out) {
    static constexpr decltype(&rr_scan_bf16_generic<1>) kern[4] = {rr_scan_bf16_generic<1>, rr_scan_bf16_generic<2>, rr_scan_bf16_generic<4>,
                                                                   rr_scan_bf16_generic<8>};
    static int waves[4];   // per kernel instance
    RR_REQUIRE(ix->dtype == RR_DTYPE_BF16 && ix->dim_pad <= RR_FLTW_MAX_DIM && ix->dim_pad % 64 == 0 &&
                   (nb == 1 || nb == 2 || nb == 4 || nb == 8),
               "rr_launch_scan_bf16w: 1, 2, 4 or 8 query slots on a bf16 index of width 64 .. %d expected", RR_FLTW_MAX_DIM);
    const int k = rr_nb_slot(nb);
    if (!waves[k]) waves[k] = rr_resident_waves((const void*)kern[k], RR_SCAN_THREADS, ix->device);
    const rr_scan_geom G = *out = rr_make_geom(ix, waves[k] / 4);
    hipLaunchKernelGGL(kern[k], dim3((G.n_waves + 3) / 4), dim3(RR_SCAN_THREADS), 0, st,
                       reinterpret_cast<const u32x4*>(ix->d_matrix), G, ix->dim_pad / 8, d_q, ix->d_sims, ix->d_gmax, ix->d_smax);
    return RR_OK;
}

// one listed launch into the index's score scratch (rr_dense_listed_fallback_wide); the geometry the listed selection reads
rr_scan_geom rr_launch_scan_bf16w_listed(rr_index* ix, const float* d_q, const int32_t* flags, int nq, int skip, hipStream_t st) {
    static int waves = 0;
    if (!waves) waves = rr_resident_waves((const void*)rr_scan_bf16_generic_listed<RR_SEL_LISTED>, RR_SCAN_THREADS, ix->device);
    rr_scan_geom G = rr_make_geom(ix, waves / 4);
    hipLaunchKernelGGL((rr_scan_bf16_generic_listed<RR_SEL_LISTED>), dim3((G.n_waves + 3) / 4), dim3(RR_SCAN_THREADS), 0, st,
                       reinterpret_cast<const u32x4*>(ix->d_matrix), G, ix->dim_pad / 8, d_q, ix->d_sims, ix->d_gmax, ix->d_smax,
                       flags, nq, skip, ix->d_flag_list);
    return G;
}
