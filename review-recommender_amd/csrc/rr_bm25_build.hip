// rr_bm25_build.hip -- the BM25 index built on the GPU from a token-id stream (gfx950).
//
// Replaces the host construction of BM25Corpus.from_corpus + BM25Index (a Python loop per
// token and an argsort per document, then a stable argsort over every (doc, term) entry).
//
// Input: tok[T] int32 term ids in document order, doc_off[n_src + 1] int64.  Output: exactly
// the arrays rr_bm25_create_dev adopts (csrc/rr_bm25.hip), plus df over the source corpus.
//
//   1. postings: a stable LSD radix sort of the tokens by term, doc id as payload.  The input
//      is in doc order, so the docs come out ascending within each term; a run-length pass
//      turns adjacent equal (term, doc) pairs into one entry (doc, tf).  post_indptr[t] is the
//      first entry of term t (a lower bound over the sorted entry terms), df its difference.
//   2. forward lists: the entries stably radix-sorted by doc, carrying (term, tf): terms come
//      out ascending within each document; doc_indptr is a lower bound over the sorted docs.
//
// The radix sort is rr_prims.h's (rr_radix_sort): 8-bit digits, ceil(bits(max key) / 8) passes (at least one), stable.
// Every element count and offset is int64 (T, nnz and byte offsets pass 2^31 and 4 GiB).
// The inputs are checked on the device (rb_check) before anything is scattered.
#include <vector>
#include <algorithm>

#include "rr_prims.h"

#define RB_THREADS RR_SORT_THREADS
#define RB_ROUNDS RR_SORT_ROUNDS
#define RB_TILE RR_SORT_TILE                 // elements per workgroup of the sort and the run-length pass
#define RB_GRID_CAP 8192                     // grid of the grid-stride kernels

#define RB_ERR_TERM 1u      // a term id outside [0, n_terms)
#define RB_ERR_OFF 2u       // doc_off decreases, or a document has 2^31 tokens or more
#define RB_ERR_ORDER 4u     // an order entry outside [-1, n_src)

static inline int64_t rb_tiles(int64_t n) { return (n + RB_TILE - 1) / RB_TILE; }
static inline unsigned rb_grid(int64_t n, int64_t per) {
    const int64_t g = (n + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : (g > RB_GRID_CAP ? RB_GRID_CAP : g));
}

// ------------------------------------------------------------------ checks
__global__ __launch_bounds__(RB_THREADS) void rb_check(const int32_t* __restrict__ tok, int64_t T, int64_t n_terms,
                                                       const int64_t* __restrict__ off, int64_t n_src,
                                                       const int64_t* __restrict__ order, int64_t n_order,
                                                       unsigned* __restrict__ err) {
    const int64_t stride = (int64_t)gridDim.x * RB_THREADS;
    unsigned bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; i < T; i += stride) {
        const int32_t t = tok[i];
        if (t < 0 || (int64_t)t >= n_terms) bad |= RB_ERR_TERM;
    }
    for (int64_t d = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; d < n_src; d += stride) {
        const int64_t len = off[d + 1] - off[d];
        if (len < 0 || len >= (1ll << 31)) bad |= RB_ERR_OFF;
    }
    for (int64_t r = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; r < n_order; r += stride) {
        const int64_t s = order[r];
        if (s < -1 || s >= n_src) bad |= RB_ERR_ORDER;
    }
    if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------ helpers
// doc[i] = d for every token i of document d (a wave per document: no limit on its length)
__global__ __launch_bounds__(RB_THREADS) void rb_doc_ids(const int64_t* __restrict__ off, int64_t n_docs,
                                                         uint32_t* __restrict__ doc) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (RB_THREADS / 64);
    for (int64_t d = (int64_t)blockIdx.x * (RB_THREADS / 64) + (threadIdx.x >> 6); d < n_docs; d += n_waves) {
        const int64_t e = off[d + 1];
        for (int64_t i = off[d] + lane; i < e; i += 64) doc[i] = (uint32_t)d;
    }
}

// doc_len[d] = off[d + 1] - off[d]
__global__ __launch_bounds__(RB_THREADS) void rb_doc_len(const int64_t* __restrict__ off, int64_t n_docs,
                                                         int32_t* __restrict__ len) {
    const int64_t stride = (int64_t)gridDim.x * RB_THREADS;
    for (int64_t d = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; d < n_docs; d += stride)
        len[d] = (int32_t)(off[d + 1] - off[d]);
}

// out[k] = first i in [0, n) with sorted[i] >= k, for k in [0, n_keys]
__global__ __launch_bounds__(RB_THREADS) void rb_lower_bounds(const uint32_t* __restrict__ sorted, int64_t n,
                                                              int64_t n_keys, int64_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * RB_THREADS;
    for (int64_t k = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; k <= n_keys; k += stride) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)sorted[mid] < k) lo = mid + 1; else hi = mid;
        }
        out[k] = lo;
    }
}

// df[t] = ptr[t + 1] - ptr[t]
__global__ __launch_bounds__(RB_THREADS) void rb_diff(const int64_t* __restrict__ ptr, int64_t n,
                                                      int64_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * RB_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; i < n; i += stride) out[i] = ptr[i + 1] - ptr[i];
}

// row lengths of the re-laid stream: row r (of [lo, lo + n)) is source document order[lo + r] (identity without order)
__global__ __launch_bounds__(RB_THREADS) void rb_row_len(const int64_t* __restrict__ order, int64_t lo, int64_t n,
                                                         const int64_t* __restrict__ off, int64_t* __restrict__ len) {
    const int64_t stride = (int64_t)gridDim.x * RB_THREADS;
    for (int64_t r = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; r < n; r += stride) {
        const int64_t s = order ? order[lo + r] : lo + r;
        len[r] = s >= 0 ? off[s + 1] - off[s] : 0;
    }
}

// copies every row's tokens to its place in the re-laid stream (a wave per row)
__global__ __launch_bounds__(RB_THREADS) void rb_gather_rows(const int64_t* __restrict__ order, int64_t lo, int64_t n,
                                                             const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ tok,
                                                             const int64_t* __restrict__ new_off,
                                                             int32_t* __restrict__ new_tok) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (RB_THREADS / 64);
    for (int64_t r = (int64_t)blockIdx.x * (RB_THREADS / 64) + (threadIdx.x >> 6); r < n; r += n_waves) {
        const int64_t s = order ? order[lo + r] : lo + r;
        if (s < 0) continue;
        const int64_t src = off[s], cnt = off[s + 1] - src, dst = new_off[r];
        for (int64_t i = lane; i < cnt; i += 64) new_tok[dst + i] = tok[src + i];
    }
}

// ------------------------------------------------------------------ run-length pass
// entry boundaries of the (term, doc)-sorted token stream
__device__ __forceinline__ bool rb_head(const uint32_t* __restrict__ K, const uint32_t* __restrict__ P, int64_t i) {
    return i == 0 || K[i] != K[i - 1] || P[i] != P[i - 1];
}

__global__ __launch_bounds__(RB_THREADS) void rb_rle_count(const uint32_t* __restrict__ K,
                                                           const uint32_t* __restrict__ P, int64_t n,
                                                           int64_t* __restrict__ cnt) {
    __shared__ unsigned c;
    if (threadIdx.x == 0) c = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RB_TILE;
    unsigned mine = 0;
    for (int r = 0; r < RB_ROUNDS; ++r) {
        const int64_t i = base + r * RB_THREADS + threadIdx.x;
        if (i < n && rb_head(K, P, i)) ++mine;
    }
    if (mine) atomicAdd(&c, mine);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}

// every run head writes its entry (doc, term, start position), entries in stream order
__global__ __launch_bounds__(RB_THREADS) void rb_rle_write(const uint32_t* __restrict__ K,
                                                           const uint32_t* __restrict__ P, int64_t n,
                                                           const int64_t* __restrict__ tile_off,
                                                           uint32_t* __restrict__ e_doc, uint32_t* __restrict__ e_term,
                                                           int64_t* __restrict__ e_pos) {
    __shared__ unsigned wc[RB_THREADS / 64];
    __shared__ int64_t run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) run = tile_off[blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * RB_TILE;
    for (int r = 0; r < RB_ROUNDS; ++r) {
        const int64_t i = base + r * RB_THREADS + tid;
        const bool h = i < n && rb_head(K, P, i);
        const uint64_t m = __ballot(h);
        if (lane == 0) wc[wave] = (unsigned)__popcll(m);
        __syncthreads();
        if (h) {
            int64_t e = run + __popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) e += wc[w];
            e_doc[e] = P[i];
            e_term[e] = K[i];
            e_pos[e] = i;
        }
        __syncthreads();
        if (tid == 0) run += wc[0] + wc[1] + wc[2] + wc[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(RB_THREADS) void rb_rle_tf(const int64_t* __restrict__ e_pos, int64_t nnz, int64_t n,
                                                        uint32_t* __restrict__ tf) {
    const int64_t stride = (int64_t)gridDim.x * RB_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x; e < nnz; e += stride)
        tf[e] = (uint32_t)((e + 1 < nnz ? e_pos[e + 1] : n) - e_pos[e]);
}

// ------------------------------------------------------------------ host side
namespace {

// device allocations of one build: whatever is not handed over is freed when the build ends (also on an error)
struct RbPool {
    hipStream_t st;
    std::vector<void*> live;
    int64_t* scan_sums = nullptr;   // chunk sums of the build's scans (rb_build sizes it for the largest of them)
    explicit RbPool(hipStream_t s) : st(s) {}
    template <typename T>
    int alloc(T** p, int64_t n) {
        *p = nullptr;
        if (hipMalloc((void**)p, sizeof(T) * (size_t)(n > 0 ? n : 1)) != hipSuccess) {
            hipGetLastError();
            rr_set_error("rr_bm25_build: out of device memory (%lld bytes)", (long long)(sizeof(T) * (size_t)n));
            return RR_E_NOMEM;
        }
        live.push_back((void*)*p);
        return RR_OK;
    }
    void release(void* p) {
        auto it = std::find(live.begin(), live.end(), p);
        if (it != live.end()) {
            hipStreamSynchronize(st);   // (the build's kernels may still read it)
            hipFree(p);
            live.erase(it);
        }
    }
    void keep(void* p) {
        auto it = std::find(live.begin(), live.end(), p);
        if (it != live.end()) live.erase(it);
    }
    ~RbPool() {
        hipStreamSynchronize(st);
        for (void* p : live) hipFree(p);
    }
};

#define RB_TRY(expr)                 \
    do {                             \
        const int _rc = (expr);      \
        if (_rc != RR_OK) return _rc; \
    } while (0)

using rb_f_i64 = rr_f_i64;   // what the build's scans sum: an int64 array

// the chunk sums of the scans of one rb_build_core over T tokens and of n_rows row lengths: the count matrix is the largest
int rb_alloc_scan_sums(RbPool& pool, int64_t T, int64_t n_rows) {
    return pool.alloc(&pool.scan_sums, rr_scan_sums_len(std::max(rr_sort_counts(T), n_rows)));
}

// rr_radix_sort of n keys (< 2^32, at most max_key) with its counts in the pool.  Returns the buffer index that holds the
// result.
template <int NP>
int rb_sort(hipStream_t st, RbPool& pool, int64_t n, uint32_t max_key, const uint32_t* ksrc, const uint32_t* p0src,
            const uint32_t* p1src, uint32_t* K[2], uint32_t* P0[2], uint32_t* P1[2], int* result) {
    const int passes = rr_sort_passes(max_key);
    *result = (passes - 1) & 1;
    if (n == 0) return RR_OK;
    int64_t *hist = nullptr, *offs = nullptr;
    RB_TRY(pool.alloc(&hist, rr_sort_counts(n)));
    RB_TRY(pool.alloc(&offs, rr_sort_counts(n) + 1));
    RB_TRY(rr_radix_sort<NP>(st, n, passes, ksrc, p0src, p1src, K, P0, P1, hist, offs, pool.scan_sums));
    pool.release(hist);
    pool.release(offs);
    return RR_OK;
}

struct RbCsr {
    int64_t nnz = 0;
    int64_t *post_indptr = nullptr, *doc_indptr = nullptr, *df = nullptr;
    uint32_t *post_docs = nullptr, *post_tf = nullptr, *doc_terms = nullptr, *doc_tf = nullptr;
    int32_t* doc_len = nullptr;
};

int rb_read_i64(hipStream_t st, const int64_t* d, int64_t* h) {
    RR_HIP_TRY(hipMemcpyAsync(h, d, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    RR_HIP_TRY(hipStreamSynchronize(st));
    return RR_OK;
}

// postings (+ df) and, if `forward`, the forward lists of the stream (tok[T], off[n_docs + 1]); the arrays it returns
// stay allocated in `pool`
int rb_build_core(hipStream_t st, RbPool& pool, const int32_t* tok, int64_t T, const int64_t* off, int64_t n_docs,
                  int64_t n_terms, bool forward, RbCsr* o) {
    // 1. tokens sorted by term, doc ids as payload (docs ascending per term: the input is in doc order)
    uint32_t *K[2] = {nullptr, nullptr}, *P[2] = {nullptr, nullptr};
    RB_TRY(pool.alloc(&K[0], T));
    RB_TRY(pool.alloc(&K[1], T));
    RB_TRY(pool.alloc(&P[0], T));
    RB_TRY(pool.alloc(&P[1], T));
    if (n_docs > 0) {
        hipLaunchKernelGGL(rb_doc_ids, dim3(rb_grid(n_docs, RB_THREADS / 64)), dim3(RB_THREADS), 0, st, off, n_docs, P[1]);
        RR_HIP_TRY(hipGetLastError());
    }
    int res = 0;
    // (pass 0 reads the doc ids from P[1] and writes P[0]: a source is never the buffer its pass writes)
    uint32_t* P1src = P[1];
    RB_TRY(rb_sort<1>(st, pool, T, (uint32_t)(n_terms > 0 ? n_terms - 1 : 0), (const uint32_t*)tok, P1src, nullptr,
                      K, P, nullptr, &res));
    pool.release(K[res ^ 1]);
    pool.release(P[res ^ 1]);
    const uint32_t *SK = K[res], *SP = P[res];

    // 2. run-length encode equal (term, doc) pairs into entries
    const int64_t nt = rb_tiles(T);
    int64_t* tile_off = nullptr;
    RB_TRY(pool.alloc(&tile_off, nt + 1));
    if (T > 0) {
        hipLaunchKernelGGL(rb_rle_count, dim3((unsigned)nt), dim3(RB_THREADS), 0, st, SK, SP, T, tile_off);
        RR_HIP_TRY(hipGetLastError());
    }
    rr_scan(rb_f_i64{tile_off}, nt, pool.scan_sums, tile_off, (int32_t*)nullptr, (int64_t*)nullptr, st);   // (in place)
    RR_HIP_TRY(hipGetLastError());
    int64_t nnz = 0;
    RB_TRY(rb_read_i64(st, tile_off + nt, &nnz));
    o->nnz = nnz;
    uint32_t* e_term = nullptr;
    int64_t* e_pos = nullptr;
    RB_TRY(pool.alloc(&o->post_docs, nnz));
    RB_TRY(pool.alloc(&e_term, nnz));
    RB_TRY(pool.alloc(&e_pos, nnz));
    if (T > 0) {
        hipLaunchKernelGGL(rb_rle_write, dim3((unsigned)nt), dim3(RB_THREADS), 0, st, SK, SP, T, tile_off, o->post_docs,
                           e_term, e_pos);
        RR_HIP_TRY(hipGetLastError());
    }
    RB_TRY(pool.alloc(&o->post_tf, nnz));
    if (nnz > 0) {
        hipLaunchKernelGGL(rb_rle_tf, dim3(rb_grid(nnz, RB_THREADS)), dim3(RB_THREADS), 0, st, e_pos, nnz, T, o->post_tf);
        RR_HIP_TRY(hipGetLastError());
    }
    pool.release(e_pos);
    pool.release(tile_off);
    pool.release(K[res]);
    pool.release(P[res]);

    // 3. post_indptr and df
    RB_TRY(pool.alloc(&o->post_indptr, n_terms + 1));
    RB_TRY(pool.alloc(&o->df, n_terms));
    hipLaunchKernelGGL(rb_lower_bounds, dim3(rb_grid(n_terms + 1, RB_THREADS)), dim3(RB_THREADS), 0, st, e_term, nnz,
                       n_terms, o->post_indptr);
    if (n_terms > 0)
        hipLaunchKernelGGL(rb_diff, dim3(rb_grid(n_terms, RB_THREADS)), dim3(RB_THREADS), 0, st, o->post_indptr, n_terms,
                           o->df);
    RR_HIP_TRY(hipGetLastError());
    if (!forward) {
        pool.release(e_term);
        return RR_OK;
    }

    // 4. forward lists: the entries stably sorted by doc, (term, tf) carried
    uint32_t *FK[2] = {nullptr, nullptr}, *FT[2] = {nullptr, nullptr}, *FF[2] = {nullptr, nullptr};
    for (int j = 0; j < 2; ++j) {
        RB_TRY(pool.alloc(&FK[j], nnz));
        RB_TRY(pool.alloc(&FT[j], nnz));
        RB_TRY(pool.alloc(&FF[j], nnz));
    }
    RB_TRY(rb_sort<2>(st, pool, nnz, (uint32_t)(n_docs > 0 ? n_docs - 1 : 0), o->post_docs, e_term, o->post_tf, FK, FT,
                      FF, &res));
    pool.release(FK[res ^ 1]);
    pool.release(FT[res ^ 1]);
    pool.release(FF[res ^ 1]);
    pool.release(e_term);
    o->doc_terms = FT[res];
    o->doc_tf = FF[res];
    RB_TRY(pool.alloc(&o->doc_indptr, n_docs + 1));
    hipLaunchKernelGGL(rb_lower_bounds, dim3(rb_grid(n_docs + 1, RB_THREADS)), dim3(RB_THREADS), 0, st, FK[res], nnz,
                       n_docs, o->doc_indptr);
    RB_TRY(pool.alloc(&o->doc_len, n_docs));
    if (n_docs > 0)
        hipLaunchKernelGGL(rb_doc_len, dim3(rb_grid(n_docs, RB_THREADS)), dim3(RB_THREADS), 0, st, off, n_docs,
                           o->doc_len);
    RR_HIP_TRY(hipGetLastError());
    RR_HIP_TRY(hipStreamSynchronize(st));
    pool.release(FK[res]);
    return RR_OK;
}

int rb_build(rr_bm25* bm, int32_t on_device, const int32_t* tok, int64_t T, const int64_t* doc_off, int64_t n_src,
             int64_t n_terms, const int64_t* order, int64_t n_order, int64_t lo, int64_t hi) {
    hipStream_t st = bm->stream;
    RbPool pool(st);
    // inputs on the device
    const int32_t* d_tok = tok;
    const int64_t* d_off = doc_off;
    const int64_t* d_order = order;
    if (!on_device) {
        int32_t* t = nullptr;
        int64_t *o = nullptr, *r = nullptr;
        RB_TRY(pool.alloc(&t, T));
        RB_TRY(pool.alloc(&o, n_src + 1));
        if (T > 0) RR_HIP_TRY(hipMemcpyAsync(t, tok, sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, st));
        RR_HIP_TRY(hipMemcpyAsync(o, doc_off, sizeof(int64_t) * (size_t)(n_src + 1), hipMemcpyHostToDevice, st));
        if (order) {
            RB_TRY(pool.alloc(&r, n_order));
            RR_HIP_TRY(hipMemcpyAsync(r, order, sizeof(int64_t) * (size_t)n_order, hipMemcpyHostToDevice, st));
        }
        d_tok = t; d_off = o; d_order = order ? r : nullptr;
    }
    // checks before any scatter: ids in range, doc_off monotone from 0 to T, order in [-1, n_src)
    unsigned* d_err = nullptr;
    RB_TRY(pool.alloc(&d_err, 1));
    RR_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(unsigned), st));
    const int64_t n_chk = std::max(T, std::max(n_src, order ? n_order : 0));
    hipLaunchKernelGGL(rb_check, dim3(rb_grid(n_chk, RB_THREADS * 4)), dim3(RB_THREADS), 0, st, d_tok, T, n_terms, d_off,
                       n_src, d_order, order ? n_order : 0, d_err);
    RR_HIP_TRY(hipGetLastError());
    unsigned err = 0;
    int64_t ends[2] = {-1, -1};
    RR_HIP_TRY(hipMemcpyAsync(&err, d_err, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    RR_HIP_TRY(hipMemcpyAsync(&ends[0], d_off, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    RR_HIP_TRY(hipMemcpyAsync(&ends[1], d_off + n_src, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    RR_HIP_TRY(hipStreamSynchronize(st));
    RR_REQUIRE(!(err & RB_ERR_TERM), "rr_bm25_build: a term id is outside [0, %lld)", (long long)n_terms);
    RR_REQUIRE(!(err & RB_ERR_OFF), "rr_bm25_build: doc_off decreases (or a document has 2^31 tokens or more)");
    RR_REQUIRE(!(err & RB_ERR_ORDER), "rr_bm25_build: an order entry is outside [-1, %lld)", (long long)n_src);
    RR_REQUIRE(ends[0] == 0 && ends[1] == T, "rr_bm25_build: doc_off runs from %lld to %lld, not from 0 to %lld",
               (long long)ends[0], (long long)ends[1], (long long)T);

    const int64_t n_rows = hi - lo;
    const bool relay = order != nullptr || lo != 0 || hi != n_src;
    RB_TRY(rb_alloc_scan_sums(pool, T, n_rows));
    RbCsr src, out;
    RB_TRY(rb_build_core(st, pool, d_tok, T, d_off, n_src, n_terms, !relay, &src));
    if (!relay) {
        out = src;
    } else {
        // df of the source corpus is kept; the rows are re-laid in order and built a second time
        pool.release(src.post_indptr); pool.release(src.post_docs); pool.release(src.post_tf);
        int64_t *len = nullptr, *new_off = nullptr;
        int32_t* new_tok = nullptr;
        RB_TRY(pool.alloc(&len, n_rows));
        RB_TRY(pool.alloc(&new_off, n_rows + 1));
        hipLaunchKernelGGL(rb_row_len, dim3(rb_grid(n_rows, RB_THREADS)), dim3(RB_THREADS), 0, st, d_order, lo, n_rows,
                           d_off, len);
        RR_HIP_TRY(hipGetLastError());
        rr_scan(rb_f_i64{len}, n_rows, pool.scan_sums, new_off, (int32_t*)nullptr, (int64_t*)nullptr, st);
        RR_HIP_TRY(hipGetLastError());
        pool.release(len);
        int64_t T2 = 0;
        RB_TRY(rb_read_i64(st, new_off + n_rows, &T2));
        RB_TRY(pool.alloc(&new_tok, T2));
        if (T2 > T) {   // an order that repeats rows: the second build's scans are the larger ones
            pool.release(pool.scan_sums);
            RB_TRY(rb_alloc_scan_sums(pool, T2, 0));
        }
        hipLaunchKernelGGL(rb_gather_rows, dim3(rb_grid(n_rows, RB_THREADS / 64)), dim3(RB_THREADS), 0, st, d_order, lo,
                           n_rows, d_off, d_tok, new_off, new_tok);
        RR_HIP_TRY(hipGetLastError());
        if (!on_device) { pool.release((void*)d_tok); d_tok = nullptr; }
        RB_TRY(rb_build_core(st, pool, new_tok, T2, new_off, n_rows, n_terms, true, &out));
        pool.release(out.df);
        out.df = src.df;
    }
    RR_HIP_TRY(hipStreamSynchronize(st));
    bm->nnz = out.nnz;
    bm->n_docs = n_rows;
    bm->n_terms = n_terms;
    bm->n_src = n_src;
    bm->length_sum = T;
    bm->d_post_indptr = out.post_indptr; bm->d_post_docs = (int32_t*)out.post_docs; bm->d_post_tf = (int32_t*)out.post_tf;
    bm->d_doc_indptr = out.doc_indptr; bm->d_doc_terms = (int32_t*)out.doc_terms; bm->d_doc_tf = (int32_t*)out.doc_tf;
    bm->d_doc_len = out.doc_len; bm->d_df = out.df;
    for (void* p : {(void*)out.post_indptr, (void*)out.post_docs, (void*)out.post_tf, (void*)out.doc_indptr,
                    (void*)out.doc_terms, (void*)out.doc_tf, (void*)out.doc_len, (void*)out.df})
        pool.keep(p);
    return RR_OK;
}

}  // namespace

extern "C" int rr_bm25_build(int32_t device, int32_t inputs_on_device, const int32_t* tok, int64_t n_tok,
                             const int64_t* doc_off, int64_t n_src, int64_t n_terms, const int64_t* order,
                             int64_t n_order, int64_t row_lo, int64_t row_hi, double k1, double b,
                             int64_t row_offset, void* stream, rr_bm25** out) {
    RR_REQUIRE(out, "rr_bm25_build: NULL out");
    *out = nullptr;
    RR_REQUIRE(n_tok >= 0 && (n_tok == 0 || tok) && doc_off, "rr_bm25_build: NULL token stream");
    RR_REQUIRE(n_src >= 1 && n_src < (1ll << 31), "rr_bm25_build: n_src %lld out of [1, 2^31)", (long long)n_src);
    RR_REQUIRE(n_terms >= 0 && n_terms < (1ll << 31), "rr_bm25_build: n_terms %lld out of [0, 2^31)", (long long)n_terms);
    const int64_t n_rows = order ? n_order : n_src;
    RR_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31), "rr_bm25_build: %lld rows out of [1, 2^31)", (long long)n_rows);
    RR_REQUIRE(row_lo >= 0 && row_lo < row_hi && row_hi <= n_rows,
               "rr_bm25_build: row range [%lld, %lld) is empty or outside [0, %lld)", (long long)row_lo,
               (long long)row_hi, (long long)n_rows);
    RR_HIP_TRY(hipSetDevice(device));
    rr_bm25* bm = new rr_bm25();
    bm->device = device; bm->k1 = k1; bm->b = b; bm->row_offset = row_offset;
    bm->avgdl = 0.0;
    if (hipStreamCreateWithFlags(&bm->stream, hipStreamNonBlocking) != hipSuccess) {
        rr_set_error("rr_bm25_build: hipStreamCreate failed");
        delete bm;
        return RR_E_HIP;
    }
    // the build runs on the handle's own stream: it first waits for what the caller's stream has queued (the work that
    // wrote the inputs, e.g. a tensor made just before the call); NULL = the device's null stream
    hipEvent_t ready = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ready, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(bm->stream, ready, 0);
    if (ready) hipEventDestroy(ready);
    if (e != hipSuccess) {
        rr_set_error("rr_bm25_build: ordering after the caller's stream failed: %s", hipGetErrorString(e));
        rr_bm25_destroy(bm);
        return RR_E_HIP;
    }
    const int rc = rb_build(bm, inputs_on_device, tok, n_tok, doc_off, n_src, n_terms, order, n_order, row_lo, row_hi);
    if (rc) { rr_bm25_destroy(bm); return rc; }
    *out = bm;
    return RR_OK;
}

extern "C" int rr_bm25_build_stats(rr_bm25* bm, int64_t* h_df, int64_t* h_sizes) {
    RR_REQUIRE(bm && h_sizes && (bm->n_terms == 0 || h_df), "rr_bm25_build_stats: NULL argument");
    RR_REQUIRE(bm->d_df, "rr_bm25_build_stats: the handle was not made by rr_bm25_build");
    std::lock_guard<std::mutex> lk(bm->mu);
    RR_HIP_TRY(hipSetDevice(bm->device));
    if (bm->n_terms) RR_HIP_TRY(hipMemcpy(h_df, bm->d_df, sizeof(int64_t) * (size_t)bm->n_terms, hipMemcpyDeviceToHost));
    h_sizes[0] = bm->n_docs; h_sizes[1] = bm->n_terms; h_sizes[2] = bm->nnz;
    h_sizes[3] = bm->n_src; h_sizes[4] = bm->length_sum;
    return RR_OK;
}

extern "C" int rr_bm25_set_idf(rr_bm25* bm, const double* h_idf, double avgdl) {
    RR_REQUIRE(bm && (bm->n_terms == 0 || h_idf), "rr_bm25_set_idf: NULL argument");
    RR_REQUIRE(bm->d_df, "rr_bm25_set_idf: the handle was not made by rr_bm25_build");
    RR_REQUIRE(avgdl > 0.0 || (avgdl == 0.0 && bm->nnz == 0), "rr_bm25_set_idf: avgdl must be positive");
    std::lock_guard<std::mutex> lk(bm->mu);
    RR_HIP_TRY(hipSetDevice(bm->device));
    if (!bm->d_idf) RR_HIP_TRY(hipMalloc((void**)&bm->d_idf, sizeof(double) * (size_t)(bm->n_terms ? bm->n_terms : 1)));
    if (bm->n_terms)
        RR_HIP_TRY(hipMemcpy(bm->d_idf, h_idf, sizeof(double) * (size_t)bm->n_terms, hipMemcpyHostToDevice));
    bm->avgdl = avgdl;
    return RR_OK;
}

extern "C" int rr_bm25_copy_csr(rr_bm25* bm, int64_t* doc_indptr, int32_t* doc_terms, int32_t* doc_tf,
                                int32_t* doc_len, int64_t* post_indptr, int32_t* post_docs, int32_t* post_tf) {
    RR_REQUIRE(bm, "rr_bm25_copy_csr: NULL handle");
    std::lock_guard<std::mutex> lk(bm->mu);
    RR_HIP_TRY(hipSetDevice(bm->device));
    const size_t nnz = (size_t)bm->nnz, nd = (size_t)bm->n_docs, nt = (size_t)bm->n_terms;
    struct { void* dst; const void* src; size_t bytes; } seg[7] = {
        {doc_indptr, bm->d_doc_indptr, 8 * (nd + 1)}, {doc_terms, bm->d_doc_terms, 4 * nnz},
        {doc_tf, bm->d_doc_tf, 4 * nnz}, {doc_len, bm->d_doc_len, 4 * nd},
        {post_indptr, bm->d_post_indptr, 8 * (nt + 1)}, {post_docs, bm->d_post_docs, 4 * nnz},
        {post_tf, bm->d_post_tf, 4 * nnz}};
    for (auto& s : seg)
        if (s.dst && s.bytes) RR_HIP_TRY(hipMemcpy(s.dst, s.src, s.bytes, hipMemcpyDefault));
    return RR_OK;
}
