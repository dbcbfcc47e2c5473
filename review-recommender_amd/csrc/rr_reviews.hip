// rr_reviews.hip -- best review per candidate product.
//
// Replaces _best_snippets (app/app_product_search.py:320-370) / best_review_snippets
// (app/test.py:181-215): among the reviews of each candidate sku, the one whose embedding has
// the largest dot product with the query (`En @ qvec`, per-sku argmax = first maximum in file
// order).  The reference re-reads the whole reviews parquet per query; here the normalised review
// embeddings stay in HBM, grouped by product through a CSR (product row -> ascending review
// ids), so a query touches only the reviews of its <= pool candidates.
//
// Latency-bound: one 256-thread workgroup per (query, candidate); a 16-lane DPP row scores one
// review with the summation order of rr_scan_f32 (one fmaf chain per lane, rr_row16_sum).
#include "rr_common.h"

struct rr_reviews {
    int device = 0;
    int64_t n_reviews = 0, n_products = 0;
    int32_t dim = 0, dim_pad = 0;
    float* d_emb = nullptr;          // n_reviews x dim_pad, rows l2-normalised
    int64_t* d_indptr = nullptr;     // n_products + 1
    int32_t* d_ids = nullptr;        // review ids, ascending per product
    int32_t* d_cut = nullptr;        // [RR_MAX_BATCH] per-query review-id cut of rr_reviews_best_cut_dev
    // a shard of a larger table (rr_reviews_set_global_ids): review ids above are LOCAL, cuts and answers are GLOBAL ids
    int64_t nnz = 0;                 // entries of d_ids
    int64_t n_total = 0;             // reviews of the whole table (= n_reviews without a map)
    int32_t* d_global = nullptr;     // [n_reviews] local review id -> global review id, ascending; nullptr: local = global
    int32_t* d_gids = nullptr;       // global ids in CSR order (d_global[d_ids[j]]); d_ids itself without a map
    std::mutex mu;
};


__global__ __launch_bounds__(256) void rr_best_review(
    const f32x4* __restrict__ emb, int nf, const int64_t* __restrict__ indptr, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ gids, int64_t n_products, const float* __restrict__ queries, int dim,
    const int64_t* __restrict__ rows, int pool,
    int64_t row_offset, int32_t max_review_id_all, const int32_t* __restrict__ cuts,
    float* __restrict__ best_score, int32_t* __restrict__ best_id) {
    __shared__ uint64_t wbest[4];
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int sub = lane & 15, grp = lane >> 4;
    const int q = blockIdx.y, c = blockIdx.x;
    const int32_t max_review_id = cuts ? cuts[q] : max_review_id_all;
    const int64_t prod = rows[(int64_t)q * pool + c] - row_offset;
    uint64_t best = 0;                                    // (score key << 32) | ~global review id ; 0 = none
    if (prod >= 0 && prod < n_products) {
        const int64_t s = indptr[prod], e = indptr[prod + 1];
        const float* qv = queries + (int64_t)q * dim;
        for (int64_t base = s + 4 * w; base < e; base += 16) {   // 4 waves x 4 reviews per step
            const int64_t j = base + grp;
            const bool have = j < e;
            const int32_t rid = have ? ids[j] : 0;
            const int32_t gid = have ? gids[j] : 0;           // the id cuts compare with and the answer names (a shard: global)
            const f32x4* p = emb + (int64_t)rid * (nf * 16) + sub;
            float acc = 0.f;
            for (int i = 0; i < nf; ++i) {
                const f32x4 x = p[16 * i];
                const int k = 4 * (sub + 16 * i);
                const float q0 = k + 0 < dim ? qv[k + 0] : 0.f, q1 = k + 1 < dim ? qv[k + 1] : 0.f;
                const float q2 = k + 2 < dim ? qv[k + 2] : 0.f, q3 = k + 3 < dim ? qv[k + 3] : 0.f;
                acc = __builtin_fmaf(x.x, q0, acc);
                acc = __builtin_fmaf(x.y, q1, acc);
                acc = __builtin_fmaf(x.z, q2, acc);
                acc = __builtin_fmaf(x.w, q3, acc);
            }
            acc = rr_row16_sum(acc);
            if (have && gid <= max_review_id) {
                const float v = acc == acc ? acc : -INFINITY;   // np.argmax treats NaN as the maximum;
                                                                // a NaN review embedding is not expected
                const uint64_t key = ((uint64_t)rr_f2key(v) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)gid);
                best = key > best ? key : best;                 // larger score, then smaller review id (the map is ascending)
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = __shfl_xor(best, m, 64);
        best = o > best ? o : best;
    }
    if (lane == 0) wbest[w] = best;
    __syncthreads();
    if (tid == 0) {
        uint64_t b = wbest[0];
        for (int i = 1; i < 4; ++i) b = wbest[i] > b ? wbest[i] : b;
        const int64_t o = (int64_t)q * pool + c;
        best_score[o] = b ? rr_key2f((uint32_t)(b >> 32)) : 0.f;
        best_id[o] = b ? (int32_t)(0xFFFFFFFFu - (uint32_t)(b & 0xFFFFFFFFu)) : -1;
    }
}

// The reference scores only the first `max_rows` reviews, in file order, of all reviews whose sku is among
// the query's candidates (`sub_meta.iloc[:max_rows]`, app/app_product_search.py:342-345, app/test.py:200-203).
// File order = review id, so the cut is a review-id threshold: the max_rows-th smallest id in the union of
// the candidates' (ascending) lists; n_reviews (= keep all) when the union is not longer than max_rows.
// One workgroup per query: bisection on the id, counts by binary search in every candidate's list.
__global__ __launch_bounds__(256) void rr_reviews_cut(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ ids, int64_t n_products,
    const int64_t* __restrict__ rows, int pool, int64_t row_offset, int64_t max_rows, int64_t n_reviews,
    int32_t* __restrict__ cut) {
    __shared__ long long wsum[4];
    const int tid = threadIdx.x, q = blockIdx.x;
    auto count_le = [&](int64_t T) -> long long {      // reviews with id <= T among the candidates (block-wide)
        long long c = 0;
        for (int i = tid; i < pool; i += 256) {
            const int64_t prod = rows[(int64_t)q * pool + i] - row_offset;
            if (prod < 0 || prod >= n_products) continue;
            int64_t lo = indptr[prod], hi = indptr[prod + 1];
            const int64_t s = lo;
            while (lo < hi) {                             // first entry > T
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)ids[mid] <= T) lo = mid + 1; else hi = mid;
            }
            c += lo - s;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
        __syncthreads();
        if ((tid & 63) == 0) wsum[tid >> 6] = c;
        __syncthreads();
        return wsum[0] + wsum[1] + wsum[2] + wsum[3];
    };
    int32_t out;
    if (max_rows <= 0) out = -1;
    else if (count_le(n_reviews) <= max_rows) out = (int32_t)n_reviews;
    else {
        int64_t lo = 0, hi = n_reviews - 1;               // smallest T with count_le(T) >= max_rows
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (count_le(mid) >= max_rows) hi = mid; else lo = mid + 1;
        }
        out = (int32_t)lo;
    }
    if (tid == 0) cut[q] = out;
}

// ---- the cut across row shards -------------------------------------------------
// On row shards no rank sees every candidate's list, so the max_rows-th smallest review id of the union is found by a
// 256-way narrowing of an interval [lo, hi] of GLOBAL review ids that every rank holds per query: a round counts, on
// every rank, the reviews with id <= T_j among the merged pool's candidates the rank owns, for 256 thresholds T_j that
// cut the interval into 256 parts; the ranks' counts are summed by the caller (sharded.py: exchange_counts); the next
// launch reads the sums and narrows to the part that holds the max_rows-th id.  ceil(log256(n_total)) rounds end at
// lo = hi = the cut.  reviews.model_cut is the numpy statement of it.  state = [n_queries][2] int64 (lo, hi); a query
// whose union is not longer than max_rows is parked at lo = hi = n_total (keep all) by the first narrowing.

__device__ __forceinline__ int64_t rr_cut_threshold(int64_t lo, int64_t hi, int j) {
    return lo + ((int64_t)(j + 1) * (hi - lo + 1) + 255) / 256 - 1;     // T_255 = hi; T_j >= lo
}

// One narrowing of a query's interval from its 256 summed counts; block-wide (256 threads, thread j reads count j), every
// thread leaves with the same lo / hi.  Holds a __syncthreads.
__device__ __forceinline__ void rr_cut_narrow_step(const int64_t* __restrict__ sums_q, int64_t max_rows, int first,
                                                   int64_t n_total, int64_t& lo, int64_t& hi, int* wfirst) {
    const int tid = threadIdx.x;
    const unsigned long long m = __ballot(sums_q[tid] >= max_rows);
    if ((tid & 63) == 0) wfirst[tid >> 6] = m ? (tid & ~63) + (int)__builtin_ctzll(m) : 256;
    __syncthreads();
    const int js = min(min(wfirst[0], wfirst[1]), min(wfirst[2], wfirst[3]));   // first j with count >= max_rows
    if (lo >= n_total) return;                                      // parked: keep all
    if (first && sums_q[255] <= max_rows) { lo = hi = n_total; return; }
    if (js >= 256) return;                                          // (count(hi) >= max_rows holds from round 1 on)
    const int64_t nlo = js == 0 ? lo : rr_cut_threshold(lo, hi, js - 1) + 1;
    hi = rr_cut_threshold(lo, hi, js);
    lo = nlo;
}

__global__ void rr_reviews_cut_begin(int64_t* __restrict__ state, int n_queries, int64_t n_total) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n_queries) { state[2 * q] = 0; state[2 * q + 1] = n_total - 1; }
}

// One round on one rank, a workgroup per query: narrows with the previous round's sums when given, then thread j counts
// the reviews with global id <= T_j over the candidates this index owns (binary search in each ascending list; the
// candidates' list bounds are staged in LDS 256 at a time).
__global__ __launch_bounds__(256) void rr_reviews_cut_count(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ gids, int64_t n_products,
    const int64_t* __restrict__ rows, int pool, int64_t row_offset, int64_t max_rows, int64_t n_total,
    const int64_t* __restrict__ sums, int first, int64_t* __restrict__ state, int64_t* __restrict__ counts) {
    __shared__ int wfirst[4];
    __shared__ int64_t s_beg[256], s_end[256];
    const int tid = threadIdx.x, q = blockIdx.x;
    int64_t lo = state[2 * q], hi = state[2 * q + 1];
    if (sums) {
        rr_cut_narrow_step(sums + (int64_t)q * 256, max_rows, first, n_total, lo, hi, wfirst);   // (reads precede its barrier)
        if (tid == 0) { state[2 * q] = lo; state[2 * q + 1] = hi; }
    }
    const int64_t T = rr_cut_threshold(lo, hi, tid);
    long long c = 0;
    for (int base = 0; base < pool; base += 256) {
        __syncthreads();                                            // the previous 256 candidates have been read
        const int i = base + tid;
        int64_t s = 0, e = 0;
        if (i < pool) {
            const int64_t prod = rows[(int64_t)q * pool + i] - row_offset;
            if (prod >= 0 && prod < n_products) { s = indptr[prod]; e = indptr[prod + 1]; }   // rows of other shards: 0
        }
        s_beg[tid] = s; s_end[tid] = e;
        __syncthreads();
        const int n = min(256, pool - base);
        for (int k = 0; k < n; ++k) {
            int64_t a = s_beg[k], b = s_end[k];
            const int64_t s0 = a;
            while (a < b) {                                         // first entry > T
                const int64_t mid = (a + b) >> 1;
                if ((int64_t)gids[mid] <= T) a = mid + 1; else b = mid;
            }
            c += a - s0;
        }
    }
    counts[(int64_t)q * 256 + tid] = c;
}

// The narrowing alone: behind the last round (cuts = lo of every query), or as a step of its own (cuts == nullptr).
__global__ __launch_bounds__(256) void rr_reviews_cut_narrow(
    const int64_t* __restrict__ sums, int64_t max_rows, int first, int64_t n_total, int64_t* __restrict__ state,
    int32_t* __restrict__ cuts) {
    __shared__ int wfirst[4];
    const int q = blockIdx.x;
    int64_t lo = state[2 * q], hi = state[2 * q + 1];
    rr_cut_narrow_step(sums + (int64_t)q * 256, max_rows, first, n_total, lo, hi, wfirst);
    if (threadIdx.x == 0) {
        state[2 * q] = lo; state[2 * q + 1] = hi;
        if (cuts) cuts[q] = (int32_t)lo;
    }
}

__global__ void rr_reviews_map_ids(const int32_t* __restrict__ ids, const int32_t* __restrict__ global, int64_t nnz,
                                   int32_t* __restrict__ gids) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nnz) gids[j] = global[ids[j]];
}

__global__ void rr_reviews_l2norm(float* __restrict__ mat, int64_t n_rows, int dim_pad, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    float* p = mat + row * dim_pad;
    float ss = 0.f;
    for (int i = lane; i < dim_pad; i += 64) ss = __builtin_fmaf(p[i], p[i], ss);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    const float nrm = fmaxf(sqrtf(ss), eps);
    for (int i = lane; i < dim_pad; i += 64) p[i] = p[i] / nrm;
}

extern "C" int rr_reviews_destroy(rr_reviews* rv) {
    if (!rv) return RR_OK;
    hipSetDevice(rv->device);
    hipFree(rv->d_emb); hipFree(rv->d_indptr); hipFree(rv->d_ids); hipFree(rv->d_cut); hipFree(rv->d_global);
    if (rv->d_gids != rv->d_ids) hipFree(rv->d_gids);
    delete rv;
    return RR_OK;
}

// `emb` is host memory (rr_reviews_create) or device memory on `device` (rr_reviews_create_dev): the one difference is the
// direction of the copy into the padded matrix.
static int rr_reviews_make(const char* who, const float* emb, hipMemcpyKind kind, int64_t n_reviews, int32_t dim,
                           int64_t n_products, const int64_t* h_indptr, const int32_t* h_ids, int32_t device,
                           float normalize_eps, rr_reviews** out) {
    RR_REQUIRE(out, "%s: NULL out", who);
    *out = nullptr;
    RR_REQUIRE(emb && h_indptr && n_reviews >= 1 && n_reviews < (1ll << 31) && n_products >= 1 && dim >= 1,
               "%s: bad argument", who);
    const int64_t nnz = h_indptr[n_products];
    RR_REQUIRE(nnz >= 0 && nnz <= n_reviews && (nnz == 0 || h_ids), "%s: bad CSR", who);
    RR_HIP_TRY(hipSetDevice(device));
    rr_reviews* rv = new rr_reviews();
    rv->device = device; rv->n_reviews = n_reviews; rv->n_products = n_products; rv->n_total = n_reviews;
    rv->dim = dim; rv->dim_pad = (int32_t)rr_round_up(dim, 64);
    hipError_t e = hipMalloc((void**)&rv->d_emb, sizeof(float) * (size_t)n_reviews * rv->dim_pad);
    if (e == hipSuccess) e = hipMalloc((void**)&rv->d_indptr, sizeof(int64_t) * (size_t)(n_products + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&rv->d_ids, sizeof(int32_t) * (size_t)(nnz ? nnz : 1));
    if (e == hipSuccess) e = hipMalloc((void**)&rv->d_cut, sizeof(int32_t) * RR_MAX_BATCH);
    if (e == hipSuccess && rv->dim_pad != dim) e = hipMemset(rv->d_emb, 0, sizeof(float) * (size_t)n_reviews * rv->dim_pad);
    if (e == hipSuccess)
        e = hipMemcpy2D(rv->d_emb, sizeof(float) * rv->dim_pad, emb, sizeof(float) * dim, sizeof(float) * dim,
                        (size_t)n_reviews, kind);
    if (e == hipSuccess) e = hipMemcpy(rv->d_indptr, h_indptr, sizeof(int64_t) * (size_t)(n_products + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(rv->d_ids, h_ids, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess && normalize_eps > 0.f) {
        hipLaunchKernelGGL(rr_reviews_l2norm, dim3((unsigned)((n_reviews + 3) / 4)), dim3(256), 0, nullptr, rv->d_emb,
                           n_reviews, rv->dim_pad, normalize_eps);
        e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) {
        rr_set_error("%s: %s", who, hipGetErrorString(e));
        rr_reviews_destroy(rv);
        return RR_E_HIP;
    }
    rv->d_gids = rv->d_ids;
    rv->nnz = nnz;
    *out = rv;
    return RR_OK;
}

extern "C" int rr_reviews_create(const float* h_emb, int64_t n_reviews, int32_t dim, int64_t n_products,
                                 const int64_t* h_indptr, const int32_t* h_ids, int32_t device,
                                 float normalize_eps, rr_reviews** out) {
    return rr_reviews_make("rr_reviews_create", h_emb, hipMemcpyHostToDevice, n_reviews, dim, n_products, h_indptr, h_ids, device,
                           normalize_eps, out);
}

extern "C" int rr_reviews_create_dev(const float* d_emb, int64_t n_reviews, int32_t dim, int64_t n_products,
                                     const int64_t* h_indptr, const int32_t* h_ids, int32_t device,
                                     float normalize_eps, rr_reviews** out) {
    RR_HIP_TRY(hipSetDevice(device));
    RR_HIP_TRY(hipDeviceSynchronize());          // the rows may still be on their way on any stream
    return rr_reviews_make("rr_reviews_create_dev", d_emb, hipMemcpyDeviceToDevice, n_reviews, dim, n_products, h_indptr, h_ids,
                           device, normalize_eps, out);
}

extern "C" int rr_reviews_best_dev(rr_reviews* rv, const float* d_queries, int32_t n_queries,
                                   const int64_t* d_rows, int32_t pool, int64_t row_offset,
                                   int32_t max_review_id, float* d_best_score, int32_t* d_best_id, void* stream) {
    RR_REQUIRE(rv && d_queries && d_rows && d_best_score && d_best_id, "rr_reviews_best_dev: NULL argument");
    RR_REQUIRE(n_queries >= 1 && n_queries <= RR_MAX_BATCH && pool >= 1 && pool <= RR_MAX_POOL,
               "rr_reviews_best_dev: n_queries %d / pool %d out of range", n_queries, pool);
    RR_HIP_TRY(hipSetDevice(rv->device));
    hipLaunchKernelGGL(rr_best_review, dim3((unsigned)pool, (unsigned)n_queries), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(rv->d_emb), rv->dim_pad / 64, rv->d_indptr, rv->d_ids,
                       rv->d_gids, rv->n_products, d_queries, rv->dim, d_rows, pool, row_offset, max_review_id,
                       (const int32_t*)nullptr, d_best_score, d_best_id);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_reviews_best_cut_dev(rr_reviews* rv, const float* d_queries, int32_t n_queries,
                                       const int64_t* d_rows, int32_t pool, int64_t row_offset,
                                       int64_t max_rows, float* d_best_score, int32_t* d_best_id, void* stream) {
    RR_REQUIRE(rv && d_queries && d_rows && d_best_score && d_best_id, "rr_reviews_best_cut_dev: NULL argument");
    RR_REQUIRE(n_queries >= 1 && n_queries <= RR_MAX_BATCH && pool >= 1 && pool <= RR_MAX_POOL,
               "rr_reviews_best_cut_dev: n_queries %d / pool %d out of range", n_queries, pool);
    std::lock_guard<std::mutex> lk(rv->mu);
    RR_HIP_TRY(hipSetDevice(rv->device));
    hipLaunchKernelGGL(rr_reviews_cut, dim3((unsigned)n_queries), dim3(256), 0, (hipStream_t)stream, rv->d_indptr,
                       rv->d_gids, rv->n_products, d_rows, pool, row_offset, max_rows, rv->n_total, rv->d_cut);
    hipLaunchKernelGGL(rr_best_review, dim3((unsigned)pool, (unsigned)n_queries), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(rv->d_emb), rv->dim_pad / 64, rv->d_indptr, rv->d_ids,
                       rv->d_gids, rv->n_products, d_queries, rv->dim, d_rows, pool, row_offset, 0, (const int32_t*)rv->d_cut,
                       d_best_score, d_best_id);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_reviews_set_global_ids(rr_reviews* rv, const int32_t* h_global_ids, int64_t n_total) {
    RR_REQUIRE(rv && h_global_ids, "rr_reviews_set_global_ids: NULL argument");
    RR_REQUIRE(n_total >= rv->n_reviews && n_total < (1ll << 31),
               "rr_reviews_set_global_ids: n_total %lld outside [n_reviews %lld, 2^31)", (long long)n_total, (long long)rv->n_reviews);
    RR_REQUIRE(!rv->d_global, "rr_reviews_set_global_ids: the index has a map already");
    for (int64_t i = 0; i < rv->n_reviews; ++i)
        RR_REQUIRE(h_global_ids[i] >= 0 && h_global_ids[i] < n_total && (i == 0 || h_global_ids[i] > h_global_ids[i - 1]),
                   "rr_reviews_set_global_ids: the map must be strictly ascending inside [0, n_total) (entry %lld)", (long long)i);
    std::lock_guard<std::mutex> lk(rv->mu);
    RR_HIP_TRY(hipSetDevice(rv->device));
    int32_t *d_global = nullptr, *d_gids = nullptr;
    hipError_t e = hipMalloc((void**)&d_global, sizeof(int32_t) * (size_t)rv->n_reviews);
    if (e == hipSuccess) e = hipMalloc((void**)&d_gids, sizeof(int32_t) * (size_t)(rv->nnz ? rv->nnz : 1));
    if (e == hipSuccess) e = hipMemcpy(d_global, h_global_ids, sizeof(int32_t) * (size_t)rv->n_reviews, hipMemcpyHostToDevice);
    if (e == hipSuccess && rv->nnz) {
        hipLaunchKernelGGL(rr_reviews_map_ids, dim3((unsigned)((rv->nnz + 255) / 256)), dim3(256), 0, nullptr, rv->d_ids, d_global,
                           rv->nnz, d_gids);
        e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) {
        rr_set_error("rr_reviews_set_global_ids: %s", hipGetErrorString(e));
        hipFree(d_global); hipFree(d_gids);
        return RR_E_HIP;
    }
    rv->d_global = d_global; rv->d_gids = d_gids; rv->n_total = n_total;
    return RR_OK;
}

extern "C" int rr_reviews_cut_begin_dev(rr_reviews* rv, int32_t n_queries, int64_t* d_state, void* stream) {
    RR_REQUIRE(rv && d_state, "rr_reviews_cut_begin_dev: NULL argument");
    RR_REQUIRE(n_queries >= 1 && n_queries <= RR_MAX_BATCH, "rr_reviews_cut_begin_dev: n_queries %d out of range", n_queries);
    RR_HIP_TRY(hipSetDevice(rv->device));
    hipLaunchKernelGGL(rr_reviews_cut_begin, dim3((unsigned)((n_queries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_state,
                       n_queries, rv->n_total);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_reviews_cut_count_dev(rr_reviews* rv, int32_t n_queries, const int64_t* d_rows, int32_t pool,
                                        int64_t row_offset, int64_t max_rows, const int64_t* d_sums, int32_t first,
                                        int64_t* d_state, int64_t* d_counts, void* stream) {
    RR_REQUIRE(rv && d_rows && d_state && d_counts, "rr_reviews_cut_count_dev: NULL argument");
    RR_REQUIRE(n_queries >= 1 && n_queries <= RR_MAX_BATCH && pool >= 1 && pool <= RR_MAX_POOL && max_rows >= 1,
               "rr_reviews_cut_count_dev: n_queries %d / pool %d / max_rows %lld out of range", n_queries, pool, (long long)max_rows);
    RR_HIP_TRY(hipSetDevice(rv->device));
    hipLaunchKernelGGL(rr_reviews_cut_count, dim3((unsigned)n_queries), dim3(256), 0, (hipStream_t)stream, rv->d_indptr,
                       rv->d_gids, rv->n_products, d_rows, pool, row_offset, max_rows, rv->n_total, d_sums, first, d_state,
                       d_counts);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_reviews_cut_narrow_dev(rr_reviews* rv, int32_t n_queries, int64_t max_rows, const int64_t* d_sums,
                                         int32_t first, int64_t* d_state, int32_t* d_cuts, void* stream) {
    RR_REQUIRE(rv && d_sums && d_state, "rr_reviews_cut_narrow_dev: NULL argument");
    RR_REQUIRE(n_queries >= 1 && n_queries <= RR_MAX_BATCH && max_rows >= 1,
               "rr_reviews_cut_narrow_dev: n_queries %d / max_rows %lld out of range", n_queries, (long long)max_rows);
    RR_HIP_TRY(hipSetDevice(rv->device));
    hipLaunchKernelGGL(rr_reviews_cut_narrow, dim3((unsigned)n_queries), dim3(256), 0, (hipStream_t)stream, d_sums, max_rows,
                       first, rv->n_total, d_state, d_cuts);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_reviews_best_at_dev(rr_reviews* rv, const float* d_queries, int32_t n_queries, const int64_t* d_rows,
                                      int32_t pool, int64_t row_offset, const int32_t* d_cuts, float* d_best_score,
                                      int32_t* d_best_id, void* stream) {
    RR_REQUIRE(rv && d_queries && d_rows && d_cuts && d_best_score && d_best_id, "rr_reviews_best_at_dev: NULL argument");
    RR_REQUIRE(n_queries >= 1 && n_queries <= RR_MAX_BATCH && pool >= 1 && pool <= RR_MAX_POOL,
               "rr_reviews_best_at_dev: n_queries %d / pool %d out of range", n_queries, pool);
    RR_HIP_TRY(hipSetDevice(rv->device));
    hipLaunchKernelGGL(rr_best_review, dim3((unsigned)pool, (unsigned)n_queries), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(rv->d_emb), rv->dim_pad / 64, rv->d_indptr, rv->d_ids,
                       rv->d_gids, rv->n_products, d_queries, rv->dim, d_rows, pool, row_offset, 0, d_cuts,
                       d_best_score, d_best_id);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}
