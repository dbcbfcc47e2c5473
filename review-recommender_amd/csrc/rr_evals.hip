// rr_evals.hip -- IR metrics of a batch's answer where K3 left it (rr_ir_metrics_dev, include/rr_hip.h).
//
// Per query the eight columns of evals.model_ir_metrics (the reference's IRMetrics.evaluate_query, evals/
// performance_metrics.py:162-205) from K3's out_rows / order and the query's labels (a CSR over the queries, rows ascending
// inside a query), every float64 operation the one numpy makes:
//   ir_metrics   one wave per query, four queries per 256-thread workgroup.  Lane j takes rank j of the first 64: its row,
//                a binary search in the query's label segment, the grade and the relevance flag.  The hits at 5 / 10 / 20 and
//                the first hit are ballots; a query with k > 64 walks on in chunks of 64 only until its first hit.  The ten
//                DCG terms are divided in their lanes and added by lane 0 in numpy's order for a contiguous float64 sum.
//   ir_mean      the column means: a launch of its own behind the first (eight workgroups, one per column), fixed-order
//                float64 sums -- thread t adds rows t, t + 256, ... in ascending order, then a fixed tree over the 256
//                partial sums.  No floating-point atomics: two runs give the same bits.
// The library is built with -ffp-contract=off; every division below is IEEE (HIP's default for float64).
#include "rr_common.h"

#define EV_THREADS 256
#define EV_WAVES (EV_THREADS / 64)
#define EV_COLS 8

// Position of `row` in lab_row[lo, hi) (ascending), or -1.
__device__ __forceinline__ int64_t ev_find(const int64_t* __restrict__ lab_row, int64_t lo, int64_t hi, int64_t row) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t v = lab_row[mid];
        if (v == row) return mid;
        if (v < row) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// numpy's float64 sum of t[0 .. L) for L <= 10 (pairwise_sum under add.reduce: the identity 0.0 plus the block's sum).
__device__ __forceinline__ double ev_np_sum(const double* t, int L) {
    double res;
    if (L < 8) {
        res = 0.0;
        for (int i = 0; i < L; ++i) res += t[i];
    } else {
        res = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
        for (int i = 8; i < L; ++i) res += t[i];
    }
    return 0.0 + res;
}

__device__ __forceinline__ int ev_hits(unsigned long long mask, int c, int k) {
    const int L = c < k ? c : k;                       // <= 20: never the whole word
    return __popcll(mask & ((1ull << L) - 1ull));
}

__global__ __launch_bounds__(EV_THREADS) void ir_metrics(
        const int64_t* __restrict__ out_rows, const int32_t* __restrict__ order, int32_t nq, int32_t pool, int32_t k,
        const int64_t* __restrict__ lab_off, const int64_t* __restrict__ lab_row, const double* __restrict__ lab_grade,
        const uint8_t* __restrict__ lab_rel, int64_t n_labels, const int32_t* __restrict__ n_rel,
        const double* __restrict__ idcg, const double* __restrict__ log2tab, double* __restrict__ metrics) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * EV_WAVES + (threadIdx.x >> 6);
    if (b >= nq) return;                               // (whole waves leave; no barrier below)
    int64_t lo = lab_off[b], hi = lab_off[b + 1];
    // a segment that leaves the label arrays is cut to them: nothing outside [0, n_labels) is read
    lo = lo < 0 ? 0 : (lo > n_labels ? n_labels : lo);
    hi = hi < lo ? lo : (hi > n_labels ? n_labels : hi);
    const int64_t* rows_b = out_rows + b * (int64_t)pool;
    const int32_t* order_b = order + b * (int64_t)k;

    double grade = 0.0;
    bool rel = false;
    if (lane < k) {
        const int32_t pos = order_b[lane];
        if (pos >= 0 && pos < pool) {                  // (a position outside the pool names no row)
            const int64_t at = ev_find(lab_row, lo, hi, rows_b[pos]);
            if (at >= 0) { grade = lab_grade[at]; rel = lab_rel[at] != 0; }
        }
    }
    const unsigned long long hitmask = __ballot(rel);
    int first_hit = hitmask ? __ffsll((unsigned long long)hitmask) : 0;
    for (int base = 64; first_hit == 0 && base < k; base += 64) {      // wave-uniform: ends at the first hit
        bool r = false;
        const int j = base + lane;
        if (j < k) {
            const int32_t pos = order_b[j];
            if (pos >= 0 && pos < pool) {
                const int64_t at = ev_find(lab_row, lo, hi, rows_b[pos]);
                r = at >= 0 && lab_rel[at] != 0;
            }
        }
        const unsigned long long m = __ballot(r);
        if (m) first_hit = base + __ffsll((unsigned long long)m);
    }
    // the DCG terms, each one division in its lane, then all ten in lane 0
    const double term = lane < 10 ? grade / log2tab[lane] : 0.0;
    double t[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) t[i] = __shfl(term, i, 64);
    if (lane != 0) return;
    const int L5 = k < 5 ? k : 5, L10 = k < 10 ? k : 10;
    const double dcg5 = ev_np_sum(t, L5), dcg10 = ev_np_sum(t, L10);
    const double idcg5 = idcg[2 * b], idcg10 = idcg[2 * b + 1];
    const int nr = n_rel[b];
    double* m = metrics + b * EV_COLS;
    m[0] = idcg5 == 0.0 ? 0.0 : dcg5 / idcg5;
    m[1] = idcg10 == 0.0 ? 0.0 : dcg10 / idcg10;
    m[2] = first_hit ? 1.0 / (double)first_hit : 0.0;
    m[3] = nr <= 0 ? 0.0 : (double)ev_hits(hitmask, 10, k) / (double)nr;
    m[4] = nr <= 0 ? 0.0 : (double)ev_hits(hitmask, 20, k) / (double)nr;
    m[5] = (double)ev_hits(hitmask, 5, k) / (double)L5;
    m[6] = (double)ev_hits(hitmask, 10, k) / (double)L10;
    m[7] = (double)first_hit;
}

// mean[c] = (sum over the queries of metrics[q][c]) / nq, one workgroup per column, the same order on every run.
__global__ __launch_bounds__(EV_THREADS) void ir_mean(const double* __restrict__ metrics, int32_t nq, double* __restrict__ mean) {
    __shared__ double part[EV_THREADS];
    const int c = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int64_t q = t; q < nq; q += EV_THREADS) s += metrics[q * EV_COLS + c];
    part[t] = s;
    __syncthreads();
    for (int w = EV_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) part[t] = part[t] + part[t + w];
        __syncthreads();
    }
    if (t == 0) mean[c] = part[0] / (double)nq;
}

extern "C" int rr_ir_mean_dev(const double* d_metrics, int32_t nq, double* d_mean, void* stream) {
    RR_REQUIRE(nq >= 1, "rr_ir_mean_dev: %d queries (at least 1)", nq);
    RR_REQUIRE(d_metrics && d_mean, "rr_ir_mean_dev: NULL argument");
    hipLaunchKernelGGL(ir_mean, dim3(EV_COLS), dim3(EV_THREADS), 0, (hipStream_t)stream, d_metrics, nq, d_mean);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_ir_metrics_dev(const int64_t* d_out_rows, const int32_t* d_order, int32_t nq, int32_t pool, int32_t k,
                                 const int64_t* d_lab_off, const int64_t* d_lab_row, const double* d_lab_grade,
                                 const uint8_t* d_lab_rel, int64_t n_labels, const int32_t* d_n_rel, const double* d_idcg,
                                 const double* d_log2, double* d_metrics, double* d_mean, void* stream) {
    RR_REQUIRE(nq >= 1, "rr_ir_metrics_dev: %d queries (at least 1)", nq);
    RR_REQUIRE(pool >= 1 && pool <= RR_MAX_POOL, "rr_ir_metrics_dev: pool %d outside [1, %d]", pool, RR_MAX_POOL);
    RR_REQUIRE(k >= 1 && k <= pool, "rr_ir_metrics_dev: k %d outside [1, pool = %d]", k, pool);
    RR_REQUIRE(d_out_rows && d_order && d_lab_off && d_n_rel && d_idcg && d_log2 && d_metrics,
               "rr_ir_metrics_dev: NULL argument");
    RR_REQUIRE(n_labels >= 0, "rr_ir_metrics_dev: %lld labels", (long long)n_labels);
    RR_REQUIRE(n_labels == 0 || (d_lab_row && d_lab_grade && d_lab_rel), "rr_ir_metrics_dev: NULL label arrays for %lld labels",
               (long long)n_labels);
    const unsigned blocks = (unsigned)(((int64_t)nq + EV_WAVES - 1) / EV_WAVES);
    hipLaunchKernelGGL(ir_metrics, dim3(blocks), dim3(EV_THREADS), 0, (hipStream_t)stream, d_out_rows, d_order, nq, pool, k,
                       d_lab_off, d_lab_row, d_lab_grade, d_lab_rel, n_labels, d_n_rel, d_idcg, d_log2, d_metrics);
    RR_HIP_TRY(hipGetLastError());
    return d_mean ? rr_ir_mean_dev(d_metrics, nq, d_mean, stream) : RR_OK;
}
