// rr_dense_fltw.hip -- K1 batched scan at a RUNTIME WIDTH: the filter path of rr_dense_flt.hip for indexes of either storage
// dtype whose dim_pad is 64, 128, .. 1024 and not 384 (another embedding model: 768 or 1024 floats).  Same contract, same tail:
//
//   rr_fltw_prep_queries   pads the launch's queries, writes their bf16 planes and the error bound eps per slot
//   rr_scan_fltw           streams the bf16 filter plane of the fp32 rows once for up to RR_FLTW_MAXQ = 64 queries and leaves
//                          what rr_scan_flt16 leaves: one tile word per (32-row tile, query), one key per selection group
//   rr_select_mtiles       (rr_dense.hip, unchanged) the 8-row M-tiles that can hold a top-pool row
//   rr_rescore_chain_w     their rows with the per-row fmaf chain of rr_scan_f32_generic at nf = dim_pad / 64
//   rr_rescore_chain_wb    ... of a bf16 index with the chain of rr_scan_bf16_generic (rr_dense_bf16w.hip)
//   rr_select_rescored     (unchanged) exact top-pool, (score desc, row asc)
//   listed VALU passes     (rr_dense.hip: rr_dense_listed_fallback_wide) flagged queries, eight per pass
//
// so a query's answer is the exact top-pool of its per-row-chain scores, bitwise the same alone, in any batch, on any shard.
// The 384-wide kernels are not templated on the width: they keep every constant and every hand-placed wait they have.
// This scan is plain C++: the compiler counts the waits of a three-stage register ring.
//   A bf16 index has no plane: its rows ARE one (the scan streams ix->d_matrix), and the first term of the bound vanishes
// because rr_row_norm_max<true> reports a row delta of 0 at every width (it never touches the delta sum).
#include "rr_x3.h"

// ------------------------------------------------------------------ the error bound at width D
// eps = 1.01 (delta_rows ||q~|| + ||a||max ||q - q~|| + c(D) ||a||max ||q||): the formula of rr_flt_prep_queries term for
// term; only the accumulation coefficient depends on the width.  Both the scan and the rescoring chain add D products in
// fp32; a sum of n terms in ANY order is within gamma_n sum |a_k q_k| <= gamma_n ||a|| ||q|| of the exact one, gamma_n =
// n u / (1 - n u), u = 2^-24.  Two such sums stand between s~ and the chain score: 2 gamma_D.  At D = 384 the 384 path sets
// 2^-14 aside for 2 gamma_384 = 768 * 2^-24 (1 + 2.3e-5) = 2^-14 / 1.3333: a margin of 1.33.  Keeping that margin,
//     c(D) = 1.3333 * 2 * D * 2^-24 = 2^-14 * D / 384        for D >= 384,
// and 2^-14 below 384 (never less than what the 384 path grants: max(D, 384)).  At D = 1024, D u = 6.1e-5: the
// 1 / (1 - n u) of gamma moves the fourth digit of a 1.33 margin.
// (tests/test_fltw_bound.py parses the next two lines)
#define RR_FLTW_ACC_COEF 6.1035156e-5f      // 2^-14
#define RR_FLTW_ACC_DIM 384                 // c(D) = RR_FLTW_ACC_COEF * max(D, RR_FLTW_ACC_DIM) / RR_FLTW_ACC_DIM
__host__ __device__ static inline float rr_fltw_acc_coef(int dim_pad) {
    return RR_FLTW_ACC_COEF * (float)(dim_pad > RR_FLTW_ACC_DIM ? dim_pad : RR_FLTW_ACC_DIM) / (float)RR_FLTW_ACC_DIM;
}

// One workgroup (64 lanes) per query slot.  slot < nq reads the caller's row (src: nq rows of `dim` floats, `src_stride` floats
// apart), the rest is zeros; the padded fp32 row goes to `padded` (unless null: src is the padded buffer itself), its bf16
// image (round to nearest even, memory order) to `plane`, the bound to eps[slot].
__global__ __launch_bounds__(64) void rr_fltw_prep_queries(const float* __restrict__ src, int64_t src_stride, int dim, int nq,
                                                           float* __restrict__ padded, int dim_pad, unsigned short* __restrict__ plane,
                                                           float* __restrict__ eps, rr_flt_bounds B) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    float ss = 0.f, sr = 0.f, sd = 0.f;
    for (int pos = lane; pos < dim_pad; pos += 64) {
        const float x = (slot < nq && pos < dim) ? src[(int64_t)slot * src_stride + pos] : 0.f;
        if (padded) padded[(int64_t)slot * dim_pad + pos] = x;
        const __bf16 r = (__bf16)x;                                // round to nearest even
        const float xr = (float)r, d = x - xr;
        ss = __builtin_fmaf(x, x, ss);
        sr = __builtin_fmaf(xr, xr, sr);
        sd = __builtin_fmaf(d, d, sd);
        plane[(int64_t)slot * dim_pad + pos] = __builtin_bit_cast(unsigned short, r);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        ss += __shfl_xor(ss, m, 64);
        sr += __shfl_xor(sr, m, 64);
        sd += __shfl_xor(sd, m, 64);
    }
    // NaN / inf anywhere gives a NaN / inf bound: rr_select_mtiles flags the query (no filtering)
    if (lane == 0)
        eps[slot] = 1.01f * (B.row_delta * sqrtf(sr) + B.row_norm * sqrtf(sd) + rr_fltw_acc_coef(dim_pad) * B.row_norm * sqrtf(ss));
}

// ------------------------------------------------------------------ the scan
// v_mfma_f32_16x16x32_bf16 takes its A operand as a 16-rows x 64-B global_load_dwordx4 delivers it (lane l = row l & 15,
// dims 8 (l >> 4) .. + 7 of the K-step: see rr_scan_flt16), so a loaded register IS an operand.  ks_n = dim_pad / 32 K-steps
// per row, always even; a ring stage = two K-steps of a 32-row M-tile = one 128-byte line of each row = four registers.
// Three stages rotate by name (the loop body is written three times): while the MFMAs of one run, the loads of the next
// two are in flight; the compiler places the counted vmcnt waits.  The query planes sit in LDS fragment-major
// ([K-step][fragment of 16 queries][k quarter][query]: one conflict-free 1 KiB ds_read_b128 per fragment and K-step);
// QN = 32 NQ2 queries x dim_pad x 2 B: 128 KB at 64 queries x 1024, one workgroup per CU in 160 KB.
//   Per 32-row M-tile: 2 x NF x ks_n MFMAs, then the epilogue of rr_scan_flt16 -- C layout (lane l, register i): row 4 (l >> 4)
// + i of the 16-row half, query l & 15 of the fragment -- into one tile word per 32 queries' lane pair, stored at once
// (no store prefilter: sigma is 384-only and pays from 2M rows), and the group key when the M-tile closes a group.
//   Registers (launch bound: 512 threads, two waves per SIMD): 112 at 32 queries, 145 at 64 -- 12 ring, 16 NQ2 accumulators,
// the B fragments in flight, addressing -- no spills: one workgroup of eight waves per CU at 64 queries, two at 32.
template <int NQ2>
__global__ __launch_bounds__(512, 2) void rr_scan_fltw(
    const u32x4* __restrict__ mat, rr_scan_geom G, int ks_n, const u32x4* __restrict__ plane,   // [32*NQ2][4 ks_n] units, natural k order
    uint32_t* __restrict__ words, uint32_t* __restrict__ smax, const float* __restrict__ eps, int nq) {
    constexpr int THREADS = 512;
    constexpr int QN = 32 * NQ2;
    constexpr int NF = 2 * NQ2;                       // 16-query B fragments per K-step
    extern __shared__ u32x4 qs[];                     // [ks_n][NF][4][16]
    const int tid = threadIdx.x;
    const int ru = 4 * ks_n;                          // 16-byte units per bf16 row / query
    for (int i = tid; i < QN * ru; i += THREADS) {
        const int q = i / ru, unit = i % ru;          // unit = 4 * K-step + k quarter
        qs[(((unit >> 2) * NF + (q >> 4)) * 4 + (unit & 3)) * 16 + (q & 15)] = plane[i];
    }
    __syncthreads();

    const int lane = tid & 63;
    const int c = lane & 31, h = lane >> 5;           // tile words: query 32 t + c; M-tiles h and 2 + h
    const int64_t wave = (int64_t)blockIdx.x * (THREADS / 64) + (tid >> 6);
    if (wave >= G.n_waves) return;
    const int64_t t0 = wave * G.tiles_per_wave;
    const int64_t t1 = t0 + G.tiles_per_wave < G.n_tiles ? t0 + G.tiles_per_wave : G.n_tiles;
    const int64_t m0 = t0 * 2, m1 = t1 * 2;           // 32-row M-tiles of this wave

    const int lrow = lane & 15, lpc = lane >> 4;      // load = operand order: row of the 16-row half, 16-B piece (k quarter)
    // the stage the next fetch brings: (M-tile pf_mt, K-steps pf_k, pf_k + 1); past the end: the last M-tile again, never used
    int64_t pf_mt = m0;
    int pf_k = 0;
    auto fetch = [&](u32x4 (&d)[4]) {
        const int64_t mt = pf_mt < m1 ? pf_mt : m1 - 1;
        int64_t rx = mt * 32 + lrow, ry = rx + 16;
        rx = rx < G.n_rows ? rx : G.n_rows - 1;
        ry = ry < G.n_rows ? ry : G.n_rows - 1;
        const u32x4* px = mat + rx * ru + 4 * pf_k + lpc;
        const u32x4* py = mat + ry * ru + 4 * pf_k + lpc;
        d[0] = px[0];                                 // rows 0-15, K-step pf_k
        d[1] = py[0];                                 // rows 16-31
        d[2] = px[4];                                 // K-step pf_k + 1
        d[3] = py[4];
        pf_k += 2;
        if (pf_k >= ks_n) {
            pf_k = 0;
            ++pf_mt;
        }
    };

    float gm[NQ2];                                    // running maximum of the current group (sub-run of tiles)
#pragma unroll
    for (int t = 0; t < NQ2; ++t) gm[t] = -INFINITY;
    const uint32_t code_shift = 16u + 4u * (uint32_t)h;
    const float step = rr_flt_gap_step(eps, nq);
    const float inv_step = step > 0.f ? 0.9999f / step : 0.f;

    f32x4 acc[2][NF];
    auto clear_acc = [&]() {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int f = 0; f < NF; ++f) acc[r][f] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // the epilogue of rr_scan_flt16 for M-tile mt: lane l, accumulator (r, f), register i = row 16 r + 4 (l >> 4) + i, query 16 f + (l & 15)
    auto finish_mtile = [&](int64_t mt) {
        if (mt * 32 + 32 > G.n_rows) {                // the matrix's last, short M-tile: rows past the end (and NaNs) -> -inf
            const int64_t rbase = mt * 32 + 4 * (lane >> 4);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int f = 0; f < NF; ++f) acc[r][f] = rr_x3_canon(acc[r][f], rbase + 16 * r, G.n_rows);
        }
#pragma unroll
        for (int t = 0; t < NQ2; ++t) {
            // maxima of rows 4 (l >> 4) .. + 3 per (row half, fragment); v_permlane16_swap(x, y) leaves x = {x.row0, y.row0, x.row2,
            // y.row2}, y = {x.row1, y.row1, x.row3, y.row3} (rows of 16 lanes): max(x, y) of fragments 2 t and 2 t + 1 of row half r
            // holds, for query 32 t + (l & 31), the 8-row M-tile 2 r in lanes < 32 and 2 r + 1 above
            float uw[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const f32x4 va = acc[r][2 * t], vb = acc[r][2 * t + 1];
                const float x = fmaxf(fmaxf(va.x, va.y), fmaxf(va.z, va.w)), y = fmaxf(fmaxf(vb.x, vb.y), fmaxf(vb.z, vb.w));
                const auto rs = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                uw[r] = fmaxf(__uint_as_float(rs[0]), __uint_as_float(rs[1]));
            }
            const float u = uw[0], w = uw[1];         // M-tiles h and 2 + h
            const float mh = fmaxf(u, w);
            const auto rm = __builtin_amdgcn_permlane32_swap(__float_as_uint(mh), __float_as_uint(mh), false, false);
            const float m32 = fmaxf(__uint_as_float(rm[0]), __uint_as_float(rm[1]));        // the tile maximum, in both halves
            gm[t] = fmaxf(gm[t], m32);
            // the word: bf16 tile maximum rounded up + four 4-bit gap codes rounded down (rr_scan_flt)
            const uint32_t b = __float_as_uint(m32);
            uint32_t word = (b >> 31) ? (b >> 16) : ((b + 0xFFFFu) >> 16);
            const uint32_t cu = rr_flt_gap_code(m32, u, inv_step), cw = rr_flt_gap_code(m32, w, inv_step);
            const uint32_t mine = (cu | (cw << 8)) << code_shift;
            const auto rc = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);
            word |= rc[0] | rc[1];
            if (h == 0) words[mt * QN + 32 * t + c] = word;
        }
        // group k of the wave = tiles [t0 + k Cg, t0 + (k + 1) Cg) of its run
        const int in_run = (int)((mt >> 1) - t0), cg = (int)G.tiles_per_group;
        if ((mt & 1) == 1 && ((in_run + 1) % cg == 0 || mt == m1 - 1)) {
            const int64_t group = wave * G.gpw + in_run / cg;
#pragma unroll
            for (int t = 0; t < NQ2; ++t) {
                if (h == 0) smax[group * QN + 32 * t + c] = rr_f2key(gm[t]);
                gm[t] = -INFINITY;
            }
        }
    };

    int64_t mt = m0;                                  // the M-tile and K-step the next stage to be multiplied belongs to
    int ks = 0;
    auto multiply = [&](const u32x4 (&a)[4]) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bf16x8 a0 = __builtin_bit_cast(bf16x8, a[2 * k]), a1 = __builtin_bit_cast(bf16x8, a[2 * k + 1]);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const bf16x8 b = __builtin_bit_cast(bf16x8, qs[((ks + k) * NF + f) * 64 + lane]);
                acc[0][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[0][f], 0, 0, 0);
                acc[1][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[1][f], 0, 0, 0);
            }
        }
        ks += 2;
        if (ks >= ks_n) {
            finish_mtile(mt);
            clear_acc();
            ks = 0;
            ++mt;
        }
    };

    u32x4 sa[4], sb[4], sc[4];
    clear_acc();
    fetch(sa);
    fetch(sb);
#pragma unroll 1
    while (mt < m1) {
        fetch(sc);
        multiply(sa);
        if (mt >= m1) break;
        fetch(sa);
        multiply(sb);
        if (mt >= m1) break;
        fetch(sb);
        multiply(sc);
    }
    if (h == 0) {
        // groups of this wave that hold no tile (a short last run): key 0 = "nothing here"
        const int cg = (int)G.tiles_per_group;
        for (int k = (int)((t1 - t0 + cg - 1) / cg); k < G.gpw; ++k)
#pragma unroll
            for (int t = 0; t < NQ2; ++t) smax[(wave * G.gpw + k) * QN + 32 * t + c] = 0u;
    }
}

// ------------------------------------------------------------------ exact rescoring at a runtime width
// rr_rescore_chain's no-plane branch with nf = dim_pad / 64 at run time: the per-row chain (rr_dense.h) over each listed 8-row
// M-tile, so the scores are the single-query scan's bit for bit.  A wave takes two M-tiles per pass (four rows' loads in flight per lane and step of i).  sc[query][slot][8].
__global__ __launch_bounds__(256) void rr_rescore_chain_w(
    const f32x4* __restrict__ mat, int64_t n_rows, int nf, const float* __restrict__ queries,   // [nq][64 nf] fp32, padded
    const uint32_t* __restrict__ mtiles, const int32_t* __restrict__ count, const int32_t* __restrict__ fb, float* __restrict__ sc) {
    __shared__ f32x4 qs[RR_FLTW_MAX_DIM / 4];
    const int q = blockIdx.y;
    if (fb[q]) return;
    const int n = count[q];
    constexpr int U = 2;
    if ((int)blockIdx.x * 4 * U >= n) return;                      // (the whole workgroup: before the barrier)
    const int units = nf * 16;
    for (int i = threadIdx.x; i < units; i += 256) qs[i] = reinterpret_cast<const f32x4*>(queries + (int64_t)q * units * 4)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, grp = lane >> 4;
    mtiles += (int64_t)q * RR_X3_MCAP;
    sc += (int64_t)q * RR_X3_MCAP * 8;
    const int64_t last_row = n_rows - 1;
    for (int s0 = ((int)blockIdx.x * 4 + wave) * U; s0 < n; s0 += (int)gridDim.x * 4 * U) {
        uint32_t m8[U];
        const f32x4* p[U][2];
        float acc[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            m8[u] = mtiles[s0 + u < n ? s0 + u : n - 1];           // (a repeated last tile: its stores are masked)
#pragma unroll
            for (int it = 0; it < 2; ++it) {                       // four rows per step: lane (sub, grp) -> row 4 it + grp
                int64_t row = (int64_t)m8[u] * 8 + 4 * it + grp;
                row = row < last_row ? row : last_row;
                p[u][it] = mat + row * units + sub;
                acc[u][it] = 0.f;
            }
        }
        for (int i = 0; i < nf; ++i) {
            const f32x4 qq = qs[16 * i + sub];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int it = 0; it < 2; ++it) acc[u][it] = rr_f32_chunk(p[u][it][16 * i], qq, acc[u][it]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const float a = rr_row16_sum(acc[u][it]);
                const int64_t row = (int64_t)m8[u] * 8 + 4 * it + grp;
                if (sub == 0 && s0 + u < n) sc[(int64_t)(s0 + u) * 8 + 4 * it + grp] = rr_rank_last(a, row < n_rows);
            }
    }
}

// The same launch for the rows of a bf16 index (units = dim_pad / 8 chunks per row): the chain of rr_scan_bf16_generic (rr_dense.h).
// Same lists, same sc layout, same masking of the repeated last tile.
__global__ __launch_bounds__(256) void rr_rescore_chain_wb(
    const u32x4* __restrict__ mat, int64_t n_rows, int units, const float* __restrict__ queries,   // [nq][8 units] fp32, padded
    const uint32_t* __restrict__ mtiles, const int32_t* __restrict__ count, const int32_t* __restrict__ fb, float* __restrict__ sc) {
    __shared__ f32x4 qs[RR_FLTW_MAX_DIM / 4];
    const int q = blockIdx.y;
    if (fb[q]) return;
    const int n = count[q];
    constexpr int U = 2;
    if ((int)blockIdx.x * 4 * U >= n) return;                      // (the whole workgroup: before the barrier)
    for (int i = threadIdx.x; i < 2 * units; i += 256) qs[i] = reinterpret_cast<const f32x4*>(queries + (int64_t)q * units * 8)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, grp = lane >> 4;
    const int nr = (units + 15) >> 4;
    mtiles += (int64_t)q * RR_X3_MCAP;
    sc += (int64_t)q * RR_X3_MCAP * 8;
    const int64_t last_row = n_rows - 1;
    for (int s0 = ((int)blockIdx.x * 4 + wave) * U; s0 < n; s0 += (int)gridDim.x * 4 * U) {
        uint32_t m8[U];
        const u32x4* p[U][2];
        float acc[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            m8[u] = mtiles[s0 + u < n ? s0 + u : n - 1];           // (a repeated last tile: its stores are masked)
#pragma unroll
            for (int it = 0; it < 2; ++it) {                       // four rows per step: lane (sub, grp) -> row 4 it + grp
                int64_t row = (int64_t)m8[u] * 8 + 4 * it + grp;
                row = row < last_row ? row : last_row;
                p[u][it] = mat + row * units;
                acc[u][it] = 0.f;
            }
        }
        for (int i = 0; i < nr; ++i) {
            const int c = sub + 16 * i;
            if (c < units) {                                       // (a chunk past the row does not exist: nothing is read)
                const f32x4 q0 = qs[2 * c], q1 = qs[2 * c + 1];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int it = 0; it < 2; ++it) acc[u][it] = rr_bf16_chunk(p[u][it][c], q0, q1, acc[u][it]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const float a = rr_row16_sum(acc[u][it]);
                const int64_t row = (int64_t)m8[u] * 8 + 4 * it + grp;
                if (sub == 0 && s0 + u < n) sc[(int64_t)(s0 + u) * 8 + 4 * it + grp] = rr_rank_last(a, row < n_rows);
            }
    }
}

// ------------------------------------------------------------------ host side
static size_t rr_fltw_lds_bytes(const rr_index* ix, int nq2) { return (size_t)32 * nq2 * ix->dim_pad * 2; }

// geometry: one run per resident wave, quarter runs as selection groups (rr_flt_geom); the residency depends on the LDS a
// width takes, so it is asked per (query tiles, width) and kept
template <int NQ2>
static int rr_fltw_geom(rr_index* ix, rr_scan_geom* out) {
    static int waves_of[RR_FLTW_MAX_DIM / 64 + 1] = {0};
    const int w = ix->dim_pad / 64;
    const size_t lds = rr_fltw_lds_bytes(ix, NQ2);
    if (!waves_of[w]) {
        // (more than 64 KB of dynamic LDS has to be asked for; once, for the widest launch this instance can make)
        RR_HIP_TRY(hipFuncSetAttribute((const void*)rr_scan_fltw<NQ2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       32 * NQ2 * RR_FLTW_MAX_DIM * 2));
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)rr_scan_fltw<NQ2>, 512, lds) != hipSuccess || per_cu < 1)
            per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->device) != hipSuccess || cus < 1) cus = 256;
        const int waves = per_cu * cus * 8;
        waves_of[w] = waves > RR_MAX_SCAN_WAVES ? RR_MAX_SCAN_WAVES : waves;
    }
    rr_scan_geom G = rr_make_geom(ix, waves_of[w] / 4);
    G.qs = 32 * NQ2;
    G.mm_pairs = 3;
    G.gpw = RR_MAX_SCAN_WAVES / G.n_waves < 4 ? (RR_MAX_SCAN_WAVES / G.n_waves < 1 ? 1 : RR_MAX_SCAN_WAVES / G.n_waves) : 4;
    if (G.gpw > G.tiles_per_wave) G.gpw = (int32_t)G.tiles_per_wave;
    G.tiles_per_group = (G.tiles_per_wave + G.gpw - 1) / G.gpw;
    G.gpw = (int32_t)((G.tiles_per_wave + G.tiles_per_group - 1) / G.tiles_per_group);     // no empty trailing groups
    *out = G;
    return RR_OK;
}

static int rr_fltw_ensure_buffers(rr_index* ix) {
    if (!ix->d_wplanes) RR_HIP_TRY(hipMalloc(&ix->d_wplanes, (size_t)RR_FLTW_MAXQ * RR_FLTW_MAX_DIM * 2));
    if (!ix->d_flag_done) RR_HIP_TRY(hipMalloc((void**)&ix->d_flag_done, sizeof(int32_t) * RR_SEL_MAXQ));
    return RR_OK;
}

// preparation + ONE scan launch.  src / src_stride / src_dim: the launch's nq queries (the padded buffer itself: padded = null)
template <int NQ2>
static int rr_fltw_scan(rr_index* ix, const float* src, int64_t src_stride, int src_dim, float* padded, int nq, rr_flt_bounds nb,
                        hipStream_t st, rr_scan_geom* G) {
    int rc = rr_fltw_geom<NQ2>(ix, G);
    if (rc != RR_OK) return rc;
    constexpr int QN = 32 * NQ2;
    const rr_x3_scratch X = rr_x3_scratch_of(ix);
    unsigned short* plane = static_cast<unsigned short*>(ix->d_wplanes);
    hipLaunchKernelGGL(rr_fltw_prep_queries, dim3(QN), dim3(64), 0, st, src, src_stride, src_dim, nq, padded, ix->dim_pad, plane, X.eps, nb);
    const int slot = rr_scan_events_begin(ix, st);
    rr_scan_note(ix, 5, 16, nq, 1, 2);
    (void)hipEventRecord(ix->ev0, st);
    hipLaunchKernelGGL((rr_scan_fltw<NQ2>), dim3((G->n_waves + 7) / 8), dim3(512), rr_fltw_lds_bytes(ix, NQ2), st,
                       reinterpret_cast<const u32x4*>(ix->dtype == RR_DTYPE_BF16 ? ix->d_matrix : (void*)ix->d_shadow), *G, ix->dim_pad / 32,
                       reinterpret_cast<const u32x4*>(plane),
                       reinterpret_cast<uint32_t*>(ix->d_gmax), ix->d_smax, X.eps, nq);
    (void)hipEventRecord(ix->ev1, st);
    ix->timing_valid = true;
    rr_scan_events_end(ix, slot, st);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

// the rr_rescore_chain_w launch of the tail (the kernel-test harness launches through it as well)
static void rr_launch_rescore_chain_w(rr_index* ix, const float* d_q, int nq, hipStream_t st) {
    const rr_x3_scratch X = rr_x3_scratch_of(ix);
    if (ix->dtype == RR_DTYPE_BF16)
        hipLaunchKernelGGL(rr_rescore_chain_wb, dim3(16, nq), dim3(256), 0, st, reinterpret_cast<const u32x4*>(ix->d_matrix), ix->n_rows,
                           ix->dim_pad / 8, d_q, X.mtiles, X.count, X.fb, X.sc);
    else
        hipLaunchKernelGGL(rr_rescore_chain_w, dim3(16, nq), dim3(256), 0, st, reinterpret_cast<const f32x4*>(ix->d_matrix), ix->n_rows,
                           ix->dim_pad / 64, d_q, X.mtiles, X.count, X.fb, X.sc);
}

// what the path asks of the index before anything is launched (rr_dense_chunk_fltw and the debug door)
static int rr_fltw_ready(rr_index* ix, int pool, hipStream_t st, rr_flt_bounds* nb) {
    if ((ix->n_rows + 63) / 64 < 8 * (int64_t)pool) return RR_FLT_SMALL;      // (the small-index rule of rr_dense_chunk_flt)
    const bool bf16 = ix->dtype == RR_DTYPE_BF16;     // bf16 rows are the plane: none is allocated, the plane switches do not apply
    static const bool no_shadow = getenv("RR_NO_SHADOW") != nullptr;
    if (!bf16 && (!ix->use_shadow || no_shadow)) return RR_FLT_SMALL;         // no plane: the VALU scans (this path has no fp32 stream)
    int rc = rr_flt_get_bounds(ix, st, nb);
    if (rc != RR_OK) return rc;
    if (!(nb->row_norm < 3.0e18f)) return RR_FLT_NO_BOUND;
    if (!bf16) {
        rc = rr_flt_ensure_shadow(ix, st);
        if (rc != RR_OK) return rc;
        if (!ix->shadow_valid) return RR_FLT_SMALL;                           // no room for the plane
    }
    return rr_fltw_ensure_buffers(ix);
}

int rr_dense_chunk_fltw(rr_index* ix, const float* d_q, int nq, int pool, int64_t* d_rows, float* d_scores, hipStream_t st) {
    RR_REQUIRE(ix->dim_pad != 384 && ix->dim_pad <= RR_FLTW_MAX_DIM && ix->dim_pad % 64 == 0,
               "rr_dense_chunk_fltw: index of width 64 .. %d other than 384 expected", RR_FLTW_MAX_DIM);
    RR_REQUIRE(nq >= 1 && nq <= RR_FLTW_MAXQ, "rr_dense_chunk_fltw: %d queries outside 1..%d", nq, RR_FLTW_MAXQ);
    rr_flt_bounds nb;
    int rc = rr_fltw_ready(ix, pool, st, &nb);
    if (rc != RR_OK) return rc;
    rr_scan_geom G;
    rc = nq <= 32 ? rr_fltw_scan<1>(ix, d_q, ix->dim_pad, ix->dim_pad, nullptr, nq, nb, st, &G)
                  : rr_fltw_scan<2>(ix, d_q, ix->dim_pad, ix->dim_pad, nullptr, nq, nb, st, &G);
    if (rc != RR_OK) return rc;
    const rr_x3_scratch X = rr_x3_scratch_of(ix);
    rr_launch_select_mtiles(ix, G, nq, pool, st, X.eps);
    rr_launch_rescore_chain_w(ix, d_q, nq, st);
    rr_launch_select_rescored(ix, G, nq, pool, d_rows, d_scores, st);
    RR_HIP_TRY(hipGetLastError());
    return rr_dense_listed_fallback_wide(ix, d_q, nq, pool, d_rows, d_scores, X.fb, st);
}

#ifdef RR_DEBUG_HARNESS
#include "rr_debug.h"
#define RR_DEBUG_WORD_SENTINEL 0x5A5A7FC1u      // (the tokens of rr_dense_flt.hip, where they are explained)
// ONE rr_scan_fltw launch by itself (the product's preparation and launch code) into a scratch filled with sentinels, and its
// raw output on the host: rr_debug_flt_words for one set at a runtime width.  d_queries: device, nq x dim.  geom[16], eps[256],
// words [32-row tile][stride], keys [group][stride] as there; words == NULL: geometry only.  Leaves the launch for
// rr_debug_flt_select.
extern "C" int rr_debug_fltw_words(rr_index* ix, const float* d_queries, int32_t nq, int32_t pool, int64_t* geom, float* eps,
                                   uint32_t* words, int64_t words_cap, uint32_t* keys, int64_t keys_cap) {
    RR_REQUIRE(ix && geom && ix->d_matrix && ix->dim_pad != 384 && ix->dim_pad <= RR_FLTW_MAX_DIM,
               "rr_debug_fltw_words: index of width 64 .. %d other than 384 expected", RR_FLTW_MAX_DIM);
    RR_REQUIRE(nq >= 1 && nq <= RR_FLTW_MAXQ, "rr_debug_fltw_words: %d queries outside 1..%d", nq, RR_FLTW_MAXQ);
    RR_REQUIRE(ix->maxima_q >= RR_FLT_MAXQ && ix->cur_slot == 0, "rr_debug_fltw_words: run a batched search of 9 queries or more first (allocates the scratch)");
    const bool launch = words != nullptr;
    RR_REQUIRE(!launch || (d_queries && eps && keys), "rr_debug_fltw_words: NULL argument");
    std::lock_guard<std::mutex> lock(ix->mu);
    RR_HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = nullptr;
    rr_scan_geom G;
    int rc = nq <= 32 ? rr_fltw_geom<1>(ix, &G) : rr_fltw_geom<2>(ix, &G);
    if (rc != RR_OK) return rc;
    if (launch) {
        if (ix->dtype != RR_DTYPE_BF16) ix->use_shadow = 1;
        rr_flt_bounds nb;
        rc = rr_fltw_ready(ix, pool, st, &nb);
        RR_REQUIRE(rc == RR_OK, "rr_debug_fltw_words: the wide filter path does not run on this matrix (code %d)", rc);
        const size_t n_words = (size_t)4 * ((ix->n_rows + 63) / 64) * RR_FLT_MAXQ;
        RR_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ix->d_gmax, (int)RR_DEBUG_WORD_SENTINEL, n_words, st));
        RR_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ix->d_smax, (int)RR_DEBUG_KEY_SENTINEL, (size_t)2 * rr_flt_smax_set_stride(), st));
        rc = nq <= 32 ? rr_fltw_scan<1>(ix, d_queries, ix->dim, ix->dim, ix->d_q, nq, nb, st, &G)
                      : rr_fltw_scan<2>(ix, d_queries, ix->dim, ix->dim, ix->d_q, nq, nb, st, &G);
        if (rc != RR_OK) return rc;
    }
    const int64_t per_set_w = 2 * G.n_tiles * G.qs, per_set_k = (int64_t)G.n_waves * G.gpw * G.qs;
    const int64_t g[16] = {G.n_rows, G.n_tiles, G.tiles_per_wave, G.n_waves, G.gpw, G.tiles_per_group, G.qs, per_set_w, per_set_k, 1,
                           0, G.qs / 32, (int64_t)RR_DEBUG_WORD_SENTINEL, (int64_t)RR_DEBUG_KEY_SENTINEL, per_set_w, per_set_k};
    memcpy(geom, g, sizeof(g));
    if (!launch) return RR_OK;
    RR_REQUIRE(words_cap >= per_set_w && keys_cap >= per_set_k, "rr_debug_fltw_words: output arrays too small: %lld words, %lld keys wanted",
               (long long)per_set_w, (long long)per_set_k);
    RR_HIP_TRY(hipStreamSynchronize(st));
    RR_HIP_TRY(hipMemcpy(words, ix->d_gmax, sizeof(uint32_t) * per_set_w, hipMemcpyDeviceToHost));
    RR_HIP_TRY(hipMemcpy(keys, ix->d_smax, sizeof(uint32_t) * per_set_k, hipMemcpyDeviceToHost));
    RR_HIP_TRY(hipMemcpy(eps, rr_x3_scratch_of(ix).eps, sizeof(float) * RR_SEL_MAXQ, hipMemcpyDeviceToHost));
    rr_debug_flt_note_state(ix, G, nq);
    return RR_OK;
}

// ONE rr_rescore_chain_w launch (through rr_launch_rescore_chain_w, as the tail launches it) on caller lists: rr_debug_rescore_chain
// at a runtime width.  d_queries: device, [nq][dim_pad] fp32 (padded).  mtiles [nq][cap], count / fb [nq]; sc [nq][cap][8] comes
// back, started from RR_DEBUG_SC_SENTINEL.  Every argument is checked before anything is copied or launched.
extern "C" int rr_debug_fltw_rescore(rr_index* ix, const float* d_queries, int32_t nq, const uint32_t* mtiles, int64_t cap,
                                     const int32_t* count, const int32_t* fb, float* sc) {
    RR_REQUIRE(ix && d_queries && mtiles && count && fb && sc, "rr_debug_fltw_rescore: NULL argument");
    RR_REQUIRE(ix->d_matrix && ix->dim_pad != 384 && ix->dim_pad <= RR_FLTW_MAX_DIM,
               "rr_debug_fltw_rescore: index of width 64 .. %d other than 384 expected", RR_FLTW_MAX_DIM);
    RR_REQUIRE(nq >= 1 && nq <= RR_SEL_MAXQ && cap >= 1 && cap <= RR_X3_MCAP, "rr_debug_fltw_rescore: nq %d / cap %lld out of range", nq, (long long)cap);
    const int64_t n_mtiles = (ix->n_rows + 7) / 8;
    for (int q = 0; q < nq; ++q) {
        RR_REQUIRE(count[q] >= 0 && count[q] <= cap, "rr_debug_fltw_rescore: count[%d] = %d outside 0..cap", q, count[q]);
        for (int i = 0; i < count[q]; ++i)
            RR_REQUIRE((int64_t)mtiles[(int64_t)q * cap + i] < n_mtiles, "rr_debug_fltw_rescore: mtiles[%d][%d] = %u is not one of the %lld M-tiles",
                       q, i, mtiles[(int64_t)q * cap + i], (long long)n_mtiles);
    }
    std::lock_guard<std::mutex> lock(ix->mu);
    RR_HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = nullptr;
    const rr_x3_scratch X = rr_x3_scratch_of(ix);
    RR_HIP_TRY(hipMemcpy2D(X.mtiles, sizeof(uint32_t) * RR_X3_MCAP, mtiles, sizeof(uint32_t) * cap, sizeof(uint32_t) * cap, (size_t)nq,
                           hipMemcpyHostToDevice));
    RR_HIP_TRY(hipMemcpy(X.count, count, sizeof(int32_t) * nq, hipMemcpyHostToDevice));
    RR_HIP_TRY(hipMemcpy(X.fb, fb, sizeof(int32_t) * nq, hipMemcpyHostToDevice));
    for (int q = 0; q < nq; ++q)
        RR_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(X.sc + (int64_t)q * RR_X3_MCAP * 8), (int)RR_DEBUG_SC_SENTINEL, (size_t)cap * 8, st));
    rr_launch_rescore_chain_w(ix, d_queries, nq, st);
    RR_HIP_TRY(hipGetLastError());
    RR_HIP_TRY(hipStreamSynchronize(st));
    RR_HIP_TRY(hipMemcpy2D(sc, sizeof(float) * cap * 8, X.sc, sizeof(float) * RR_X3_MCAP * 8, sizeof(float) * cap * 8, (size_t)nq,
                           hipMemcpyDeviceToHost));
    return RR_OK;
}
#endif  // RR_DEBUG_HARNESS
