// rr_dense.h -- pieces of K1 shared by the fp32 and bf16 scan files.
#pragma once
#include "rr_common.h"

#define RR_SCAN_THREADS 256
#define RR_MAX_SCAN_WAVES 8192   // 2048 workgroups x 4 waves: upper bound of any resident grid
#define RR_MFMA_MAXQ 64          // queries per exact matrix-core scan launch
#define RR_FLT_MAXQ 128          // queries per filter-scan launch (rr_dense_flt.hip)
#define RR_SEL_MAXQ 256          // queries one selection / rescoring launch may cover: two filter-scan launches (sets)
#define RR_FLT_SAMP_CAP 8192      // sampled tiles of the store prefilter (rr_flt_sample)
#define RR_FLT_NO_BOUND 1000     // rr_dense_chunk_flt: no finite row-norm bound, use the exact scans
#define RR_FLT_SMALL 1001        // rr_dense_chunk_flt: too few tiles for the filter, use the VALU scans

// Geometry of one scan launch, shared by the scan and the selection.
struct rr_scan_geom {
    int64_t n_rows, n_tiles;
    int64_t tiles_per_wave;   // C: wave w owns tiles [w*C, min((w+1)*C, n_tiles)) = one "group"
    int32_t n_waves;          // waves of the launch; every one owns at least one tile
    int32_t qs;               // 0: scores are [query][n_pad], tile maxima [query][n_tiles] (rr_scan_f32)
                              // Q: scores are [row / 16][Q][16], tile maxima [tile][Q], group maxima [wave][Q]
                              //    (the stored pass of rr_scan_mfma_x3 with Q = 16 query slots, of rr_scan_x3w with
                              //    32 or 64: every store of a wave is one contiguous block of whole 128-B lines)
    int64_t n_pad;            // 64 * n_tiles
    int32_t mm_pairs;         // M-tile maxima of the two-pass path: 0 = [tile][Q][4] (rr_scan_mfma_x3),
                              // 1 = [32-row tile][Q][2] (rr_scan_x3w: whole lines per store),
                              // 3 = [32-row tile][Q] 4 bytes (rr_scan_flt): bf16 tile maximum rounded up + four 4-bit gaps of
                              //     its 8-ROW M-tiles; the listed ids and the rescoring scratch are then per 8 rows
    int32_t gpw;              // groups per wave (0 or 1: the wave's whole run is one group); rr_scan_flt cuts a run into
    int64_t tiles_per_group;  //   gpw sub-runs of tiles_per_group tiles, group g = wave * gpw + k: fewer tiles to open per group
};


// Splits the tiles into equal contiguous runs, one per wave of (at most) `resident_blocks` x 4 waves.
rr_scan_geom rr_make_geom(const rr_index* ix, int resident_blocks);
// Which kernel a scan launch ran (rr_index_last_scan_info): 1 rr_scan_f32, 2 rr_scan_bf16, 3 rr_scan_mfma_x3,
// 4 rr_scan_x3w, 5 rr_scan_flt (6 and 7 are retired: the removed f32-input MFMA scans); terms = bf16 MFMA terms per dimension.
static inline void rr_scan_note(rr_index* ix, int kernel, int variant, int nq, int terms, int elem_bytes = 0) {
    ix->last_scan[0] = kernel; ix->last_scan[1] = variant; ix->last_scan[2] = nq; ix->last_scan[3] = terms;
    ix->last_scan[4] = elem_bytes ? elem_bytes : (ix->dtype == RR_DTYPE_BF16 ? 2 : 4);
}
// any write to the matrix: the cached row-norm bound and the bf16 filter plane no longer describe it
static inline void rr_matrix_written(rr_index* ix) {
    ix->norm_bound = -1.f;
    ix->norm_kinds = -1;
    ix->shadow_valid = false;
}
// scan slots (rr_common.h: rr_scan_slot): which of the two sets of per-batch scan state the index fields describe
int rr_slot_activate(rr_index* ix, int slot);
void rr_slot_park(rr_index* ix);
// HIP-event pair around a scan launch (rr_index_scan_stats).
int rr_scan_events_begin(rr_index* ix, hipStream_t st);
void rr_scan_events_end(rr_index* ix, int slot, hipStream_t st);
// Exact top-pool of `nq` queries from the three score levels a scan left in the index scratch.
// `only_if` (device, one flag per query, may be null): queries whose flag is 0 are skipped.
int rr_dense_listed_fallback(rr_index* ix, const float* d_q, int nq, int pool, int64_t* d_rows, float* d_scores,
                             int32_t* flags, hipStream_t st);
void rr_launch_select(rr_index* ix, const rr_scan_geom& G, int nq, int pool, int64_t* d_rows,
                      float* d_scores, hipStream_t st, const int32_t* only_if = nullptr, int slices = 1,
                      int64_t sims_slice = 0, int64_t gmax_slice = 0, int64_t smax_slice = 0);
// The sliced launches (rr_dense_x3w_fallback_all: gridDim.y = slices of RR_MFMA_MAXQ queries, qs = RR_MFMA_MAXQ): how far slice
// y + 1's scores, tile maxima and group keys sit behind slice y's, in 4-byte words.  ONE definition for the scan that
// writes the slices, the selection that reads them and the kernel test that places them (rr_debug_select).
struct rr_select_slices { int64_t sims, gmax, smax; };
static inline rr_select_slices rr_select_slice_strides(const rr_scan_geom& G) {
    return rr_select_slices{(int64_t)RR_MFMA_MAXQ * G.n_pad, (int64_t)RR_MFMA_MAXQ * G.n_tiles, (int64_t)RR_MFMA_MAXQ * RR_MAX_SCAN_WAVES};
}
// The listed launch (rr_dense_listed_fallback): RR_SEL_LISTED workgroups; workgroup b serves query ix->d_flag_list[1 + b] of
// the call from score slot b when b < ix->d_flag_list[0], writes its answer at that query's place and takes its flag down.
#define RR_SEL_LISTED 8
void rr_launch_select_listed(rr_index* ix, const rr_scan_geom& G, int pool, int64_t* d_rows, float* d_scores, int32_t* flags,
                             hipStream_t st);
// group keys of the second set of a two-set launch (rr_dense_flt.hip) sit this many words behind the first set's
static inline int64_t rr_flt_smax_set_stride() { return (int64_t)RR_FLT_MAXQ * RR_MAX_SCAN_WAVES; }
// Two-pass selection of the split-operand scan (see rr_select_mtiles in rr_dense.hip).
#define RR_X3_MCAP 16384         // M-tiles (8 or 16 rows) one query may ask to have rescored
struct rr_x3_scratch {           // (every array RR_FLT_MAXQ queries long)
    // (every array RR_SEL_MAXQ queries long: a selection launch may follow two scan launches)
    uint32_t* mtiles;            // [q][RR_X3_MCAP] M-tile ids to rescore
    int32_t* count;              // [q] how many
    uint32_t* tau;               // [q] key threshold of the query's rows
    int32_t* fb;                 // [q] 1 = the query needs the stored-score fallback
    float* eps;                  // [q] filter scan: error bound of the query's approximate scores
    float* sc;                   // [q][RR_X3_MCAP][16] rescored rows
};
rr_x3_scratch rr_x3_scratch_of(const rr_index* ix);
size_t rr_x3_scratch_bytes();
// `eps` (device, per query, may be null): the scan's scores are approximations within eps of the scores
// the rescoring will produce; M-tiles are then opened down to tau - 2 eps and rows kept down to tau - eps.
// `nq_b` > 0: the launch covers TWO scan launches (sets) of the same geometry: queries [0, nq) come from set 0, [nq,
// nq + nq_b) from set 1, whose tile / group maxima sit `set_stride_words` 4-byte words behind set 0's and whose eps /
// sigma entries start at index RR_FLT_MAXQ.
// `floor` (device, per query of the launch, may be null): row shards -- a lower bound of the corpus-wide pool-th best score.
// `masks` (device, may be null): filter words of a prefiltered two-set scan -- only the marked words of an opened group are read.
void rr_launch_select_mtiles(rr_index* ix, const rr_scan_geom& G, int nq, int pool, hipStream_t st,
                             const float* eps = nullptr, const float* sigma = nullptr, int nq_b = 0,
                             int64_t mmax_set_stride = 0, int64_t smax_set_stride = 0, const float* floor = nullptr,
                             const uint64_t* masks = nullptr);     // rr_scan_fltq's stored-M-tile masks (prefiltered pair), or null
void rr_launch_select_rescored(rr_index* ix, const rr_scan_geom& G, int nq, int pool, int64_t* d_rows,
                               float* d_scores, hipStream_t st, bool floor_mode = false);
void rr_launch_group_kth(rr_index* ix, const rr_scan_geom& G, int nq_a, int nq_b, int kth, const float* eps, float* d_bound,
                         int64_t smax_set_stride, hipStream_t st);
// Waves a kernel can keep resident on the device (occupancy x CUs x waves per workgroup).
int rr_resident_waves(const void* kernel, int threads, int device);
// Query slots NB = 1, 2, 4 or 8 of the VALU scan launch that serves nq = 1 .. 8 queries (slots past nq hold zeros).
static inline int rr_valu_nb(int nq) { return nq <= 1 ? 1 : nq <= 2 ? 2 : nq <= 4 ? 4 : 8; }
// ... and that NB's place in a launcher's table of its four kernel instances
static inline int rr_nb_slot(int nb) { return nb == 1 ? 0 : nb == 2 ? 1 : nb == 4 ? 2 : 3; }
// One VALU scan launch of nb = 1, 2, 4 or 8 query slots into the index's score scratch; *out: the geometry its selection reads.
// fp32 rows of any width (rr_dense.hip), bf16 rows 384 wide (rr_dense_bf16.hip), bf16 rows at a runtime width (rr_dense_bf16w.hip:
// dim_pad 64 .. RR_FLTW_MAX_DIM other than 384).  rr_dense_chunk (rr_dense.hip) picks one by (dtype, width).
int rr_launch_scan_f32(rr_index* ix, const float* d_q, int nb, hipStream_t st, rr_scan_geom* out);
int rr_launch_scan_bf16(rr_index* ix, const float* d_q, int nb, hipStream_t st, rr_scan_geom* out);
int rr_launch_scan_bf16w(rr_index* ix, const float* d_q, int nb, hipStream_t st, rr_scan_geom* out);
// l2_normalize of rows [first, first + n) of an fp32 index, in place
int rr_l2norm_rows_f32(rr_index* ix, int64_t first_row, int64_t n, float eps, hipStream_t st);
// ... of n padded rows anywhere on the device (a staging copy): the same kernel
int rr_l2norm_rows_f32_at(float* d_rows, int32_t dim_pad, int64_t n, float eps, hipStream_t st);
// split-bf16 matrix-core scan (rr_dense_x3.hip): 5..64 queries, either storage dtype
int rr_dense_chunk_x3(rr_index* ix, const float* d_q, int nq, int pool, int64_t* d_rows,
                      float* d_scores, hipStream_t st);
// bf16 filter scan + exact per-row-chain rescoring, 5..128 queries (rr_dense_flt.hip); RR_FLT_NO_BOUND when
// the matrix has no finite row-norm bound
// `phase`: 0 = scan + selection; 1 = scan only, bound[q] (rr_group_kth with `kth`) written, state kept in the index;
// 2 = selection of the scan phase 1 left behind, with `floor` (row shards)
// `parts` (phase 2 only): which of the selection's three steps to launch -- 1 the M-tile lists, 2 the rescoring, 4 the
// ordering + the flagged queries' fallbacks (the parked scan stays valid until the last one has been launched)
int rr_dense_chunk_flt(rr_index* ix, const float* d_q, int nq, int pool, int64_t* d_rows,
                       float* d_scores, hipStream_t st, int phase = 0, int kth = 0, float* d_bound = nullptr,
                       const float* d_floor = nullptr, int parts = 7);
// Which non-finite squared row norms the matrix holds (one pass, cached; asked only when there is no finite bound): a NaN one
// = a row with a NaN element, a +inf one = a row with an inf element or whose squares overflow (and no NaN).  Both are reported.
#define RR_NORM_KIND_NAN 1
#define RR_NORM_KIND_INF 2
int rr_flt_norm_kinds(rr_index* ix, hipStream_t st, int* kinds);
// any other search on the index makes a parked phase-1 scan void
void rr_flt_drop_pending(rr_index* ix);
// fp32 rows (device, n x dim) -> the index's bf16 matrix rows [first, first + n), optional l2 normalise
int rr_store_rows_bf16(rr_index* ix, int64_t first_row, int64_t n, float* d_rows_f32, float eps, hipStream_t st);
// ... into n padded bf16 rows anywhere on the device (a staging copy): the same kernel
int rr_store_rows_bf16_at(void* d_dst, int32_t dim, int32_t dim_pad, int64_t n, const float* d_rows_f32, float eps, hipStream_t st);

// rr_api.hip: the address a kernel may use for p (device memory, or pinned host memory through its mapping)
int rr_device_visible(const void* p, const void** out, const char* what);

// rr_dense_flt.hip: rr_pad_queries and rr_flt_prep_queries in ONE launch (the front of a batched filter call): the padded
// fp32 queries into ix->d_q plus their bf16 planes and error bounds.  Returns RR_FLT_NO_BOUND (nothing launched) when the
// matrix has no finite row-norm bound: the caller pads the plain way.
int rr_flt_pad_prep(rr_index* ix, const float* d_queries, int nq, int slots, hipStream_t st);

// rr_dense_flt.hip: what the error bound of a filter scan takes from the matrix (cached in the index; one pass over the rows)
struct rr_flt_bounds {
    float row_norm;      // >= max over rows ||a||
    float row_delta;     // >= max over rows ||a - bf16(a)||   (0 for a bf16 matrix)
};
int rr_flt_get_bounds(rr_index* ix, hipStream_t st, rr_flt_bounds* out);
// the bf16 filter plane of an fp32 index (any width), built on first use; no room for it: ix->use_shadow = 0, RR_OK
int rr_flt_ensure_shadow(rr_index* ix, hipStream_t st);

// rr_dense_fltw.hip: the filter path at a runtime width -- fp32 storage, dim_pad in {64, 128, .. 1024} other than 384, up to
// RR_FLTW_MAXQ queries per launch over the bf16 plane + exact rescoring on the fp32 rows + the listed VALU passes for flagged
// queries.  RR_FLT_SMALL / RR_FLT_NO_BOUND as rr_dense_chunk_flt; RR_FLT_SMALL also when there is no plane (RR_NO_SHADOW, no room).
#define RR_FLTW_MAXQ 64
#define RR_FLTW_MAX_DIM 1024
// Smallest batch the wide path takes: more than W = RR_FLTW_MIN_Q - 1 = 1 queries.  Measured crossover (1M rows, pool 150,
// profiles/wide_dim_scan.json): with the routing started at W = 8 (one VALU read serves eight queries) the
// path won from its first batch, 9; taken from 2 on it needs 0.39 / 0.53 ms per call at width 768 / 1024 for ANY batch up
// to 64, against 0.68 / 0.87 ms of the VALU scan at 2 queries, 0.94 / 1.22 ms at 3 - 4 and 1.77 / 2.32 ms at 5 - 8.  A single
// query stays on the VALU scan, whose per-row chain defines the answer (0.55 / 0.73 ms).
#define RR_FLTW_MIN_Q 2
int rr_dense_chunk_fltw(rr_index* ix, const float* d_q, int nq, int pool, int64_t* d_rows, float* d_scores, hipStream_t st);
// rr_dense.hip: ceil(nq / 8) pairs of (listed generic VALU scan, listed selection) behind a wide filter launch: pair p serves
// the flagged queries ranked [8 p, 8 p + 8) of the launch with the single-query chain; a pair whose slice is empty returns at once
int rr_dense_listed_fallback_wide(rr_index* ix, const float* d_q, int nq, int pool, int64_t* d_rows, float* d_scores,
                                  const int32_t* flags, hipStream_t st);
// rr_dense_bf16w.hip: the listed scan of such a pair over the rows of a bf16 index (rr_scan_bf16_generic_listed); returns the
// geometry its selection reads
rr_scan_geom rr_launch_scan_bf16w_listed(rr_index* ix, const float* d_q, const int32_t* flags, int nq, int skip, hipStream_t st);

#ifdef __HIPCC__
// ------------------------------------------------------------------ device pieces the VALU scan files share
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// THE PER-ROW CHAIN.  A query's answer is the exact top-pool of these scores, whether the query is alone, in a batch, rescored
// behind a filter scan or on a shard; every kernel below computes them through the two steps here, so they agree by construction.
//   A row is dim_pad / 4 chunks of 16 bytes in fp32 storage (four floats), dim_pad / 8 in bf16 storage (eight bf16).  Lane j of
//   the 16 lanes of a row takes chunks j, j + 16, j + 32, .. in ascending order; a chunk past the row's end does not exist and
//   adds nothing (bf16 widths 64, 192, 320, ..: the last round is half full).  The lane's ONE accumulator starts at 0 and takes
//   each chunk's products in memory order, one fmaf each (no contraction, no reassociation); rr_row16_sum adds the 16 lanes.
//   A NaN score and a row past the end become -inf (rr_rank_last).
// Callers.  rr_f32_chunk: rr_scan_f32 (rr_dot_rows), rr_scan_f32_generic and its listed form (rr_f32w_scan_rows), rr_rescore_chain
// (both fp32 branches, rr_dense_flt.hip), rr_rescore_chain_w (rr_dense_fltw.hip).  rr_bf16_chunk: rr_scan_bf16, rr_scan_bf16_generic
// and its listed form (rr_bf16w_scan_rows), rr_rescore_chain (plane pass = the chain of a bf16 index), rr_rescore_chain_wb.
__device__ __forceinline__ float rr_f32_chunk(const f32x4 x, const f32x4 q, float acc) {
    acc = __builtin_fmaf(x.x, q.x, acc);
    acc = __builtin_fmaf(x.y, q.y, acc);
    acc = __builtin_fmaf(x.z, q.z, acc);
    acc = __builtin_fmaf(x.w, q.w, acc);
    return acc;
}
// q0 / q1: the eight query floats beside the chunk's eight bf16
__device__ __forceinline__ float rr_bf16_chunk(const u32x4 x, const f32x4 q0, const f32x4 q1, float acc) {
    acc = __builtin_fmaf(__uint_as_float(x.x << 16), q0.x, acc);
    acc = __builtin_fmaf(__uint_as_float(x.x & 0xFFFF0000u), q0.y, acc);
    acc = __builtin_fmaf(__uint_as_float(x.y << 16), q0.z, acc);
    acc = __builtin_fmaf(__uint_as_float(x.y & 0xFFFF0000u), q0.w, acc);
    acc = __builtin_fmaf(__uint_as_float(x.z << 16), q1.x, acc);
    acc = __builtin_fmaf(__uint_as_float(x.z & 0xFFFF0000u), q1.y, acc);
    acc = __builtin_fmaf(__uint_as_float(x.w << 16), q1.z, acc);
    acc = __builtin_fmaf(__uint_as_float(x.w & 0xFFFF0000u), q1.w, acc);
    return acc;
}
// NaN scores and pad rows rank last
__device__ __forceinline__ float rr_rank_last(float v, bool valid) { return (valid && v == v) ? v : -INFINITY; }

// End of a tile: lane (sub, grp) holds row row0 + 4*sub + grp for every query.
template <int NB>
__device__ __forceinline__ void rr_finish_tile(const rr_scan_geom& G, int64_t tile, int64_t wave,
                                               int64_t t0, int64_t t1, int lane, int sub, int grp,
                                               float (&mine)[NB], float (&gm)[NB],
                                               float* __restrict__ sims, float* __restrict__ gmax,
                                               uint32_t* __restrict__ smax) {
    const int64_t my_row = tile * 64 + 4 * sub + grp;
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
            if (group_end)
                smax[(int64_t)b * G.n_waves + wave] = rr_f2key(gm[b]);
        }
        if (group_end) gm[b] = -INFINITY;
    }
}

// A listed scan tells the selection behind it which queries it served: list_out[0] = how many (also when that is 0: the
// selection reads it), list_out[1 ..] = their numbers in the call.  One thread of the launch writes it.  (The runtime-width
// listed scans; rr_scan_f32<6, 8, true> writes the same block in place, where it keeps that kernel's instructions as they are.)
template <int NB>
__device__ __forceinline__ void rr_publish_list(int32_t* __restrict__ list_out, int n, const int (&list)[NB]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        list_out[0] = n;
#pragma unroll
        for (int b = 0; b < NB; ++b) list_out[1 + b] = list[b];
    }
}

// rr_flagged_list with a skip count: the queries whose flag is up, ranked by query number, ranks [skip, skip + NB).  Returns
// how many of them there are (0: the slice is empty); slots past the count repeat the last one.  (A sibling, not a new
// argument of rr_flagged_list: that one is compiled into rr_scan_f32<6, 8, true>, which every 384-wide batch launches.)
template <int NB>
__device__ __forceinline__ int rr_flagged_slice(const int32_t* __restrict__ flags, int nq, int lane, int skip, int (&list)[NB]) {
    int n = 0, seen = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) list[b] = 0;
    for (int i = 0; i < (nq + 63) / 64; ++i) {
        const int q = 64 * i + lane;
        unsigned long long m = __ballot(q < nq && flags[q] != 0);
        while (m && n < NB) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            if (seen++ < skip) continue;
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (j == n) list[j] = 64 * i + b;
            ++n;
        }
    }
#pragma unroll
    for (int j = 1; j < NB; ++j)
        if (j >= n && n > 0) list[j] = list[j - 1];
    return n;
}
#endif  // __HIPCC__
