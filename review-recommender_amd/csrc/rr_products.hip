// rr_products.hip -- products.parquet built on the device: the order of the reviews inside each sku, the per-sku KPIs and
// agg_text (gfx950).
//
// Stands in for nlp/10_product_prep.py:54-78 (groupby().agg, sort_values(["sku", "stars", "ts"], ascending=[True, False,
// False]), cumcount, groupby().apply(" \n".join)), behind rr_textprep_clean_chars_dev and rr_textprep_dedup_dev.
// products.model_build_products states in numpy what these kernels compute.
//
// rr_products_order_dev
//   pr_check      a survivor's group outside [0, n_skus) is refused before anything is sorted.
//   pr_keys       one 32-bit key word of every row, read through the permutation so far.  Five words, least significant
//                 first: ts low, ts high, stars low, stars high, group.  A key is an unsigned word whose ascending order is
//                 the order wanted: ts -> ~(ts ^ 2^63), so that NaT = INT64_MIN is all ones, above every time; stars ->
//                 -0.0 canonicalised to 0.0, the sign bit flipped (all bits for negatives), then complemented, NaN = all
//                 ones: below it sits -inf (~0x000F...F), so NaN is strictly last.  The group of a row that did not
//                 survive is n_skus: those rows end up behind every sku.
//   rr_radix_sort (rr_prims.h) stable, with the permutation as payload: 4 passes per word, 1-4 for the group.  The first
//                 permutation is the identity, so equal keys stay in row order.  Linear in n whatever a sku's length.
//   pr_kpis       a wave per sku: its segment = two lower bounds over the sorted group words; the stars of its rows are
//                 loaded 64 at a time and added ONE BY ONE in d_perm order (every lane runs the same chain over __shfl),
//                 so the sum does not depend on the launch; the maximum of ts is order-free.
// rr_products_concat_dev
//   pr_seg_bytes  a wave per sku: the bytes of its first min(length, max_per_sku) texts + 2 per separator; every offset,
//                 row and text span is checked here, a bad one counts in `bad` and gives 0 bytes.
//   rr_scan       (rr_prims.h) -> d_out_off, d_count.
//   pr_concat     a workgroup per sku, 256 texts per step: a block scan places them, a wave copies a text (and the
//                 separator in front of it).  Writes nothing when `bad` is set or the total exceeds the capacity.
// Every offset and byte count is int64.
#include <math.h>

#include "rr_prims.h"

#define PR_THREADS 256
#define PR_GRID_CAP 8192
#define PR_WORDS 5                      // ts low, ts high, stars low, stars high, group

struct rr_products {
    int device = 0;
    int32_t* d_bad = nullptr;           // what pr_seg_bytes / pr_concat refused (rr_products_status)
    int64_t* d_scratch = nullptr;       // order: keys, permutations, the sort's counts; concat: bytes per sku, chunk sums
    int64_t cap_words = 0;
    std::mutex mu;
};

static inline unsigned pr_grid(int64_t n, int64_t per) {
    const int64_t g = (n + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : (g > PR_GRID_CAP ? PR_GRID_CAP : g));
}

// ------------------------------------------------------------------------------------------------ order
__global__ __launch_bounds__(PR_THREADS) void pr_check(const int32_t* __restrict__ status, const int32_t* __restrict__ group,
                                                       int32_t n, int32_t n_skus, unsigned* __restrict__ err) {
    const int64_t stride = (int64_t)gridDim.x * PR_THREADS;
    unsigned bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x; i < n; i += stride)
        if (status[i] == 0 && (group[i] < 0 || group[i] >= n_skus)) bad = 1;
    if (bad) atomicOr(err, 1u);
}

__device__ __forceinline__ uint64_t pr_ts_key(int64_t ts) { return ~((uint64_t)ts ^ 0x8000000000000000ull); }

__device__ __forceinline__ uint64_t pr_stars_key(double x) {
    if (x != x) return ~0ull;
    if (x == 0.0) x = 0.0;                                   // -0.0 and 0.0 are equal stars
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint64_t ascending = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return ~ascending;
}

// key[i] = word `w` of row perm[i] (perm == NULL: row i, and iota[i] = i)
__global__ __launch_bounds__(PR_THREADS) void pr_keys(int w, const uint32_t* __restrict__ perm, const int32_t* __restrict__ status,
                                                      const int32_t* __restrict__ group, const double* __restrict__ stars,
                                                      const int64_t* __restrict__ ts, int32_t n, int32_t n_skus,
                                                      uint32_t* __restrict__ key, uint32_t* __restrict__ iota) {
    const int64_t stride = (int64_t)gridDim.x * PR_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t r = perm ? perm[i] : (uint32_t)i;
        uint32_t k;
        if (w == 4) k = status[r] == 0 ? (uint32_t)group[r] : (uint32_t)n_skus;
        else {
            const uint64_t q = w < 2 ? pr_ts_key(ts[r]) : pr_stars_key(stars[r]);
            k = (uint32_t)((w & 1) ? q >> 32 : q);
        }
        key[i] = k;
        if (!perm) iota[i] = (uint32_t)i;
    }
}

__device__ __forceinline__ int64_t pr_lower_bound(const uint32_t* __restrict__ sorted, int64_t n, uint32_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PR_THREADS) void pr_kpis(const uint32_t* __restrict__ sorted_group, const int32_t* __restrict__ perm,
                                                      const double* __restrict__ stars, const int64_t* __restrict__ ts, int32_t n,
                                                      int32_t n_skus, int64_t* __restrict__ seg_off, int64_t* __restrict__ n_reviews,
                                                      double* __restrict__ star_sum, int64_t* __restrict__ star_cnt,
                                                      int64_t* __restrict__ last_ts) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (PR_THREADS / 64);
    for (int64_t k = (int64_t)blockIdx.x * (PR_THREADS / 64) + (threadIdx.x >> 6); k < n_skus; k += n_waves) {
        const int64_t lo = pr_lower_bound(sorted_group, n, (uint32_t)k), hi = pr_lower_bound(sorted_group, n, (uint32_t)k + 1u);
        double acc = 0.0;
        long long cnt = 0, mx = INT64_MIN;
        for (int64_t base = lo; base < hi; base += 64) {
            const int64_t i = base + lane;
            double x = NAN;
            if (i < hi) {
                const int32_t r = perm[i];
                x = stars[r];
                const long long t = ts[r];
                mx = t > mx ? t : mx;
            }
            const int m = hi - base < 64 ? (int)(hi - base) : 64;
            for (int j = 0; j < m; ++j) {                   // one chain, in d_perm order, the same in every lane
                const double xj = __shfl(x, j, 64);
                if (xj == xj) { acc += xj; ++cnt; }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const long long o = __shfl_xor(mx, d, 64);
            mx = o > mx ? o : mx;
        }
        if (lane == 0) {
            seg_off[k] = lo;
            if (k == n_skus - 1) seg_off[n_skus] = hi;
            n_reviews[k] = hi - lo;
            star_sum[k] = acc;
            star_cnt[k] = cnt;
            last_ts[k] = mx;
        }
    }
}

// ------------------------------------------------------------------------------------------------ concatenate
__global__ __launch_bounds__(PR_THREADS) void pr_seg_bytes(const int64_t* __restrict__ text_off, const int32_t* __restrict__ len,
                                                           int64_t text_bytes, int32_t n, const int32_t* __restrict__ perm,
                                                           const int64_t* __restrict__ seg_off, int32_t n_skus, int32_t max_per_sku,
                                                           int64_t* __restrict__ seg_bytes, int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (PR_THREADS / 64);
    for (int64_t k = (int64_t)blockIdx.x * (PR_THREADS / 64) + (threadIdx.x >> 6); k < n_skus; k += n_waves) {
        const int64_t a = seg_off[k], b = seg_off[k + 1];
        const bool ok = a >= 0 && b >= a && b <= n;
        const int64_t kept = !ok ? 0 : (b - a < max_per_sku ? b - a : max_per_sku);
        long long sum = 0;
        int wrong = 0;
        for (int64_t j = lane; j < kept; j += 64) {
            const int32_t r = perm[a + j];
            if (r < 0 || r >= n) { wrong = 1; continue; }
            const int64_t o = text_off[r];
            const int32_t l = len[r];
            if (o < 0 || l < 0 || o > text_bytes - l) wrong = 1; else sum += l;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        const bool refuse = !ok || __ballot(wrong) != 0;
        if (lane == 0) {
            seg_bytes[k] = refuse ? 0 : sum + (kept > 0 ? 2 * (kept - 1) : 0);
            if (refuse) atomicAdd(bad, 1);
        }
    }
}

__global__ __launch_bounds__(PR_THREADS) void pr_concat(const uint8_t* __restrict__ text, const int64_t* __restrict__ text_off,
                                                        const int32_t* __restrict__ len, const int32_t* __restrict__ perm,
                                                        const int64_t* __restrict__ seg_off, int32_t n_skus, int32_t max_per_sku,
                                                        const int64_t* __restrict__ out_off, uint8_t* __restrict__ out,
                                                        int64_t out_bytes, const int32_t* __restrict__ refused,
                                                        int32_t* __restrict__ bad) {
    __shared__ long long s_ws[PR_THREADS / 64];
    __shared__ int64_t s_src[PR_THREADS], s_dst[PR_THREADS];
    __shared__ int32_t s_len[PR_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (`refused` = what pr_seg_bytes counted, `bad` = this kernel's own word: no workgroup reads what another one adds)
    if (*refused != 0) return;
    if (out_off[n_skus] > out_bytes) {                      // the capacity is too small: no workgroup writes anything
        if (blockIdx.x == 0 && tid == 0) atomicAdd(bad, 1);
        return;
    }
    const int k = blockIdx.x;
    const int64_t a = seg_off[k], end = out_off[k + 1];
    const int64_t kept = seg_off[k + 1] - a < max_per_sku ? seg_off[k + 1] - a : max_per_sku;
    int64_t pos = out_off[k];
    for (int64_t c = 0; c < kept; c += PR_THREADS) {
        const int64_t j = c + tid;
        int32_t l = 0;
        int64_t src = 0;
        if (j < kept) {
            const int32_t r = perm[a + j];
            l = len[r];
            src = text_off[r];
        }
        long long total;
        const long long at = rr_block_scan<long long, PR_THREADS>(j < kept ? l + (j > 0 ? 2 : 0) : 0, s_ws, &total);
        s_src[tid] = src; s_len[tid] = l; s_dst[tid] = pos + at;
        __syncthreads();
        const int cnt = kept - c < PR_THREADS ? (int)(kept - c) : PR_THREADS;
        for (int t = wave; t < cnt; t += PR_THREADS / 64) {
            int64_t d = s_dst[t];
            const int32_t tl = s_len[t];
            const bool sep = c + t > 0;
            if (d + (sep ? 2 : 0) + tl > end) continue;     // (cannot happen: pr_seg_bytes summed the same lengths)
            if (sep) {
                if (lane < 2) out[d + lane] = lane ? (uint8_t)'\n' : (uint8_t)' ';
                d += 2;
            }
            const uint8_t* s = text + s_src[t];
            for (int i = lane; i < tl; i += 64) out[d + i] = s[i];
        }
        pos += total;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int rr_products_destroy(rr_products* pb) {
    if (!pb) return RR_OK;
    hipSetDevice(pb->device);
    hipFree(pb->d_bad); hipFree(pb->d_scratch);
    delete pb;
    return RR_OK;
}

extern "C" int rr_products_create(int32_t device, rr_products** out) {
    RR_REQUIRE(out, "rr_products_create: NULL out");
    *out = nullptr;
    RR_HIP_TRY(hipSetDevice(device));
    rr_products* pb = new rr_products();
    pb->device = device;
    hipError_t e = hipMalloc((void**)&pb->d_bad, 8);         // [0] pr_seg_bytes, [1] pr_concat
    if (e == hipSuccess) e = hipMemset(pb->d_bad, 0, 8);
    if (e != hipSuccess) {
        rr_set_error("rr_products_create: %s", hipGetErrorString(e));
        rr_products_destroy(pb);
        return RR_E_HIP;
    }
    *out = pb;
    return RR_OK;
}

extern "C" int rr_products_order_dev(rr_products* pb, const int32_t* d_status, const int32_t* d_group, const double* d_stars,
                                     const int64_t* d_ts, int32_t n, int32_t n_skus, int32_t* d_perm, int64_t* d_seg_off,
                                     int64_t* d_n_reviews, double* d_star_sum, int64_t* d_star_cnt, int64_t* d_last_ts,
                                     void* stream) {
    RR_REQUIRE(pb && d_seg_off, "rr_products_order_dev: NULL argument");
    RR_REQUIRE(n >= 0 && n_skus >= 0, "rr_products_order_dev: %d rows, %d skus", n, n_skus);
    RR_REQUIRE(n == 0 || (d_status && d_group && d_stars && d_ts && d_perm), "rr_products_order_dev: NULL column with %d rows", n);
    RR_REQUIRE(n_skus == 0 || (d_n_reviews && d_star_sum && d_star_cnt && d_last_ts), "rr_products_order_dev: NULL output with %d skus",
               n_skus);
    std::lock_guard<std::mutex> lk(pb->mu);
    RR_HIP_TRY(hipSetDevice(pb->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t half = ((int64_t)n + 1) / 2, counts = rr_sort_counts(n), n_sums = rr_scan_sums_len(counts);
    int rc = rr_grow((void**)&pb->d_scratch, &pb->cap_words, 5 * half + 2 * counts + 1 + n_sums + 1, sizeof(int64_t),
                     "rr_products_order_dev");
    if (rc != RR_OK) return rc;
    uint32_t* ksrc = (uint32_t*)pb->d_scratch;
    uint32_t* K[2] = {ksrc + 2 * half, ksrc + 4 * half};
    uint32_t* P[2] = {ksrc + 6 * half, ksrc + 8 * half};
    int64_t* hist = pb->d_scratch + 5 * half;
    int64_t* offs = hist + counts;
    int64_t* sums = offs + counts + 1;
    unsigned* d_err = (unsigned*)(sums + n_sums);

    // the check, before anything is sorted or written
    if (n > 0) {
        RR_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(unsigned), st));
        hipLaunchKernelGGL(pr_check, dim3(pr_grid(n, PR_THREADS * 4)), dim3(PR_THREADS), 0, st, d_status, d_group, n, n_skus, d_err);
        RR_HIP_TRY(hipGetLastError());
        unsigned err = 0;
        RR_HIP_TRY(hipMemcpyAsync(&err, d_err, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        RR_HIP_TRY(hipStreamSynchronize(st));
        RR_REQUIRE(err == 0, "rr_products_order_dev: the group of a surviving row is outside [0, %d)", n_skus);
    }
    int res = 1;
    for (int w = 0; w < PR_WORDS && n > 0; ++w) {
        hipLaunchKernelGGL(pr_keys, dim3(pr_grid(n, PR_THREADS * 4)), dim3(PR_THREADS), 0, st, w, w == 0 ? nullptr : P[res], d_status,
                           d_group, d_stars, d_ts, n, n_skus, ksrc, P[1]);
        RR_HIP_TRY(hipGetLastError());
        const int passes = w < 4 ? 4 : rr_sort_passes((uint32_t)n_skus);
        // (the source permutation is buffer 1 in every round: an even number of passes ends there, and only the last
        // round may be odd)
        rc = rr_radix_sort<1>(st, n, passes, ksrc, P[1], nullptr, K, P, nullptr, hist, offs, sums);
        if (rc != RR_OK) return rc;
        res = (passes - 1) & 1;
    }
    if (n > 0) RR_HIP_TRY(hipMemcpyAsync(d_perm, P[res], sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    if (n_skus == 0) {
        RR_HIP_TRY(hipMemsetAsync(d_seg_off, 0, sizeof(int64_t), st));
        return RR_OK;
    }
    hipLaunchKernelGGL(pr_kpis, dim3(pr_grid(n_skus, PR_THREADS / 64)), dim3(PR_THREADS), 0, st, K[res], d_perm, d_stars, d_ts, n,
                       n_skus, d_seg_off, d_n_reviews, d_star_sum, d_star_cnt, d_last_ts);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_products_concat_dev(rr_products* pb, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                      const int32_t* d_len, int32_t n, const int32_t* d_perm, const int64_t* d_seg_off,
                                      int32_t n_skus, int32_t max_per_sku, uint8_t* d_out_text, int64_t out_bytes,
                                      int64_t* d_out_off, int64_t* d_count, void* stream) {
    RR_REQUIRE(pb && d_seg_off && d_out_off && d_count, "rr_products_concat_dev: NULL argument");
    RR_REQUIRE(n >= 0 && n_skus >= 0 && text_bytes >= 0 && out_bytes >= 0 && max_per_sku >= 1,
               "rr_products_concat_dev: %d rows, %d skus, %lld / %lld bytes, max_per_sku %d", n, n_skus, (long long)text_bytes,
               (long long)out_bytes, max_per_sku);
    RR_REQUIRE(n == 0 || (d_text_off && d_len && d_perm), "rr_products_concat_dev: NULL column with %d rows", n);
    RR_REQUIRE(d_text || text_bytes == 0, "rr_products_concat_dev: NULL text with %lld bytes", (long long)text_bytes);
    RR_REQUIRE(d_out_text || out_bytes == 0, "rr_products_concat_dev: NULL output with %lld bytes", (long long)out_bytes);
    std::lock_guard<std::mutex> lk(pb->mu);
    RR_HIP_TRY(hipSetDevice(pb->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_sums = rr_scan_sums_len(n_skus);
    int rc = rr_grow((void**)&pb->d_scratch, &pb->cap_words, (int64_t)n_skus + 1 + n_sums, sizeof(int64_t), "rr_products_concat_dev");
    if (rc != RR_OK) return rc;
    int64_t* seg_bytes = pb->d_scratch;
    int64_t* sums = seg_bytes + n_skus + 1;
    if (n_skus > 0) {
        hipLaunchKernelGGL(pr_seg_bytes, dim3(pr_grid(n_skus, PR_THREADS / 64)), dim3(PR_THREADS), 0, st, d_text_off, d_len, text_bytes,
                           n, d_perm, d_seg_off, n_skus, max_per_sku, seg_bytes, pb->d_bad);
        RR_HIP_TRY(hipGetLastError());
    }
    rr_scan(rr_f_i64{seg_bytes}, (int64_t)n_skus, sums, d_out_off, (int32_t*)nullptr, d_count, st);
    RR_HIP_TRY(hipGetLastError());
    if (n_skus > 0) {
        hipLaunchKernelGGL(pr_concat, dim3((unsigned)n_skus), dim3(PR_THREADS), 0, st, d_text, d_text_off, d_len, d_perm, d_seg_off,
                           n_skus, max_per_sku, d_out_off, d_out_text, out_bytes, pb->d_bad, pb->d_bad + 1);
        RR_HIP_TRY(hipGetLastError());
    }
    return RR_OK;
}

extern "C" int rr_products_status(rr_products* pb, int32_t* out_bad) {
    RR_REQUIRE(pb && out_bad, "rr_products_status: NULL argument");
    std::lock_guard<std::mutex> lk(pb->mu);
    RR_HIP_TRY(hipSetDevice(pb->device));
    int32_t bad[2] = {0, 0};
    RR_HIP_TRY(hipDeviceSynchronize());
    RR_HIP_TRY(hipMemcpy(bad, pb->d_bad, 8, hipMemcpyDeviceToHost));
    RR_HIP_TRY(hipMemset(pb->d_bad, 0, 8));
    *out_bad = bad[0] + bad[1];
    RR_REQUIRE(bad[0] == 0, "rr_products_concat_dev: %d sku(s) had segment offsets that decrease or leave the rows, a row outside "
               "the table or a text that leaves the text buffer (no text was written)", bad[0]);
    RR_REQUIRE(bad[1] == 0, "rr_products_concat_dev: the output buffer is too small for the concatenated text (no text was written)");
    return RR_OK;
}
