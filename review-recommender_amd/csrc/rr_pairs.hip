// rr_pairs.hip -- the reranker's pairs on the device: from a batch's candidate rows and the token plane of the index to the
// packed `[CLS] query [SEP] text [SEP]` sequences rr_ce_forward_dev takes (gfx950).
//
// Stands in for what CrossEncoder.predict does in front of the model as run_search calls it (app/app_product_search.py:272-278,
// app/test.py:223-225): pairs (query, agg_text[:2000]) through the model's BertTokenizer, truncated `longest_first` to
// max_length.  The text side is tokenised ONCE per index (rerank.RerankText: the WordPiece ids of agg_text[:2000], the first
// max_length - 3 of them, uint16, back to back with int64 offsets: the token plane); per batch only lengths are compared and
// ids copied.  rerank.model_plane / rerank.model_pairs state in numpy what the plane and the two kernels here hold.
//
// Pair p of a batch's flattened list is (query b = p / rr_k, candidate j = p % rr_k) and reads d_rows[b * pool + j]; a call
// serves the pairs [first_pair, first_pair + n_pairs), which may begin and end inside a query.
//   rp_measure   one thread per pair: n_a = the query's ids, n_b = the document's ids in the plane, and the kept lengths
//                by the rule of WordPieceTokenizer.encode_pair, with avail = max_length - 3:
//                    cut only when n_a + n_b > avail; n1 = the shorter side, n2 = the longer (b on a tie);
//                    n2 = n1 if n1 > avail else max(n1, avail - n1); if n1 + n2 > avail still: n1 = avail / 2, n2 = n1 + avail % 2.
//                The plane holds min(n_b, avail) ids; the rule gives the same kept lengths for both whenever n_a <= avail
//                (tests/test_rerank_model.py sweeps it), so a longer query is the host's (rerank.pack_queries).
//   rr_scan      (rr_prims.h) the lengths keep_a + keep_b + 3 -> d_cu [n_pairs + 1]; the host reads back d_cu[n_pairs].
//   rp_write     one wave per pair, lanes striding over the sequence: [CLS], query ids, [SEP], text ids widened from uint16,
//                [SEP]; type 0 up to and including the first [SEP], 1 behind it; position = index inside the sequence.  A
//                wave instruction reads 128 contiguous bytes of the plane and stores 256 contiguous bytes to each of the
//                three id arrays.  What rp_measure answered is checked against the offsets again before anything is read
//                or written, so no d_keep / d_cu can take a wave outside the plane, the queries or the outputs.
#include "rr_prims.h"

#define RP_THREADS 256
#define RP_WAVES (RP_THREADS / 64)
#define RP_MAX_BLOCKS 2048                         // rp_write strides the pairs beyond this many workgroups
#define RP_MAX_TOKENS ((int64_t)1 << 27)           // rr_ce_forward_dev's fp32 call limit

struct rr_pairs {
    int device = 0;
    int32_t* d_bad = nullptr;           // [0] rows outside the plane / offsets that decrease (measure), [1] pairs rp_write refused
    int64_t* d_sums = nullptr;          // chunk sums of the scan
    int64_t cap_words = 0;
    std::mutex mu;
};

// The two kept lengths of a pair with n_a query and n_b text tokens (both >= 0).
__device__ __forceinline__ void rp_keep(int32_t n_a, int32_t n_b, int32_t avail, int32_t* keep_a, int32_t* keep_b) {
    if ((int64_t)n_a + n_b > avail) {
        const bool swap = n_a > n_b;                                // (a tie: b is the longer side)
        int32_t n1 = swap ? n_b : n_a, n2 = swap ? n_a : n_b;
        n2 = n1 > avail ? n1 : (n1 > avail - n1 ? n1 : avail - n1);
        if ((int64_t)n1 + n2 > avail) {
            n1 = avail / 2;
            n2 = n1 + avail % 2;
        }
        n_a = swap ? n2 : n1;
        n_b = swap ? n1 : n2;
    }
    *keep_a = n_a;
    *keep_b = n_b;
}

__global__ __launch_bounds__(RP_THREADS) void rp_measure(const int64_t* __restrict__ plane_off, int32_t n_docs, int64_t row_offset,
                                                         const int64_t* __restrict__ rows, int32_t pool, int32_t rr_k,
                                                         const int32_t* __restrict__ q_off, int32_t avail, int64_t first_pair,
                                                         int32_t n_pairs, int32_t* __restrict__ keep, int32_t* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x;
    if (i >= n_pairs) return;
    const int64_t p = first_pair + i;
    const int64_t b = p / rr_k, j = p % rr_k;
    int32_t wrong = 0;
    int64_t n_a = (int64_t)q_off[b + 1] - q_off[b];
    if (n_a < 0) { n_a = 0; wrong = 1; }
    int64_t n_b = 0;
    const int64_t r = rows[b * pool + j] - row_offset;
    if (r >= 0 && r < n_docs) {
        n_b = plane_off[r + 1] - plane_off[r];
        if (n_b < 0) { n_b = 0; wrong = 1; }
    } else {
        wrong = 1;                                                  // a row outside the plane: no text, [CLS] q [SEP] [SEP]
    }
    if (n_b > 0x3FFFFFFF) n_b = 0x3FFFFFFF;
    int32_t ka, kb;
    rp_keep((int32_t)n_a, (int32_t)n_b, avail, &ka, &kb);
    keep[2 * i] = ka;
    keep[2 * i + 1] = kb;
    if (wrong) atomicAdd(bad, 1);
}

struct rp_f_len {   // what the scan sums: the sequence lengths, and nothing at n (so that out32[n] = the total)
    const int32_t* keep;
    int64_t n;
    __device__ __forceinline__ long long operator()(int64_t i) const {
        return i < n ? (long long)keep[2 * i] + keep[2 * i + 1] + 3 : 0;
    }
};

__global__ __launch_bounds__(RP_THREADS) void rp_write(const uint16_t* __restrict__ plane_tok, const int64_t* __restrict__ plane_off,
                                                       int32_t n_docs, int64_t row_offset, const int64_t* __restrict__ rows,
                                                       int32_t pool, int32_t rr_k, const int32_t* __restrict__ q_tok,
                                                       const int32_t* __restrict__ q_off, int32_t cls_id, int32_t sep_id,
                                                       int64_t first_pair, int32_t n_pairs, const int32_t* __restrict__ keep,
                                                       const int32_t* __restrict__ cu, int64_t n_tokens, int32_t* __restrict__ tok,
                                                       int32_t* __restrict__ typ, int32_t* __restrict__ pos, int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * RP_WAVES;
    for (int64_t i = (int64_t)blockIdx.x * RP_WAVES + (threadIdx.x >> 6); i < n_pairs; i += waves) {   // (wave-uniform)
        const int64_t p = first_pair + i;
        const int64_t b = p / rr_k, j = p % rr_k;
        const int32_t ka = keep[2 * i], kb = keep[2 * i + 1];
        const int64_t c = cu[i];
        const int64_t len = (int64_t)ka + kb + 3;
        const int32_t q0 = q_off[b];
        int64_t t0 = 0;
        bool ok = ka >= 0 && kb >= 0 && c >= 0 && c + len <= n_tokens && q0 >= 0 && ka <= (int64_t)q_off[b + 1] - q0;
        if (ok && kb > 0) {
            const int64_t r = rows[b * pool + j] - row_offset;
            ok = r >= 0 && r < n_docs;
            if (ok) {
                t0 = plane_off[r];
                ok = t0 >= 0 && kb <= plane_off[r + 1] - t0;
            }
        }
        if (!ok) {                                                  // lengths that do not fit the offsets: nothing is written
            if (lane == 0) atomicAdd(bad + 1, 1);
            continue;
        }
        const int32_t* __restrict__ qs = q_tok + q0;
        const uint16_t* __restrict__ ts = plane_tok + t0;
        for (int32_t s = lane; s < (int32_t)len; s += 64) {
            int32_t id;
            if (s == 0) id = cls_id;
            else if (s <= ka) id = qs[s - 1];
            else if (s == ka + 1 || s == (int32_t)len - 1) id = sep_id;
            else id = (int32_t)ts[s - ka - 2];
            tok[c + s] = id;
            typ[c + s] = s > ka + 1 ? 1 : 0;
            pos[c + s] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int rr_pairs_destroy(rr_pairs* h) {
    if (!h) return RR_OK;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    hipFree(h->d_bad); hipFree(h->d_sums);
    delete h;
    return RR_OK;
}

extern "C" int rr_pairs_create(int32_t device, rr_pairs** out) {
    RR_REQUIRE(out, "rr_pairs_create: NULL out");
    *out = nullptr;
    RR_HIP_TRY(hipSetDevice(device));
    rr_pairs* h = new rr_pairs();
    h->device = device;
    hipError_t e = hipMalloc((void**)&h->d_bad, 8);
    if (e == hipSuccess) e = hipMemset(h->d_bad, 0, 8);
    if (e != hipSuccess) {
        rr_set_error("rr_pairs_create: %s", hipGetErrorString(e));
        rr_pairs_destroy(h);
        return RR_E_HIP;
    }
    *out = h;
    return RR_OK;
}

static int rp_check_range(const char* who, int32_t n_docs, int32_t pool, int32_t rr_k, int32_t n_queries, int64_t first_pair,
                          int32_t n_pairs) {
    RR_REQUIRE(n_docs >= 0 && n_queries >= 0 && pool >= 1, "%s: %d documents, %d queries, pool %d", who, n_docs, n_queries, pool);
    RR_REQUIRE(rr_k >= 1 && rr_k <= pool, "%s: rr_k %d outside 1..pool = %d", who, rr_k, pool);
    RR_REQUIRE(first_pair >= 0 && n_pairs >= 0 && first_pair + n_pairs <= (int64_t)n_queries * rr_k,
               "%s: pairs [%lld, %lld) outside the %d x %d of the batch", who, (long long)first_pair,
               (long long)(first_pair + n_pairs), n_queries, rr_k);
    return RR_OK;
}

extern "C" int rr_pairs_measure_dev(rr_pairs* h, const int64_t* d_plane_off, int32_t n_docs, int64_t row_offset,
                                    const int64_t* d_rows, int32_t pool, int32_t rr_k, const int32_t* d_q_off, int32_t n_queries,
                                    int32_t max_length, int64_t first_pair, int32_t n_pairs, int32_t* d_keep, int32_t* d_cu,
                                    void* stream) {
    RR_REQUIRE(h && d_plane_off && d_rows && d_q_off && d_keep && d_cu, "rr_pairs_measure_dev: NULL argument");
    int rc = rp_check_range("rr_pairs_measure_dev", n_docs, pool, rr_k, n_queries, first_pair, n_pairs);
    if (rc != RR_OK) return rc;
    RR_REQUIRE(max_length >= 3, "rr_pairs_measure_dev: max_length %d leaves no room for [CLS] [SEP] [SEP]", max_length);
    RR_REQUIRE((int64_t)n_pairs * max_length <= 0x7FFFFFFFll, "rr_pairs_measure_dev: %d pairs of up to %d tokens exceed the int32 "
               "offsets of d_cu", n_pairs, max_length);
    std::lock_guard<std::mutex> lk(h->mu);
    RR_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    rc = rr_grow((void**)&h->d_sums, &h->cap_words, rr_scan_sums_len((int64_t)n_pairs + 1), sizeof(int64_t), "rr_pairs_measure_dev");
    if (rc != RR_OK) return rc;
    if (n_pairs > 0) {
        hipLaunchKernelGGL(rp_measure, dim3((unsigned)((n_pairs + RP_THREADS - 1) / RP_THREADS)), dim3(RP_THREADS), 0, st, d_plane_off,
                           n_docs, row_offset, d_rows, pool, rr_k, d_q_off, max_length - 3, first_pair, n_pairs, d_keep, h->d_bad);
        RR_HIP_TRY(hipGetLastError());
    }
    rr_scan(rp_f_len{d_keep, (int64_t)n_pairs}, (int64_t)n_pairs + 1, h->d_sums, (int64_t*)nullptr, d_cu, (int64_t*)nullptr, st);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_pairs_write_dev(rr_pairs* h, const uint16_t* d_plane_tok, const int64_t* d_plane_off, int32_t n_docs,
                                  int64_t row_offset, const int64_t* d_rows, int32_t pool, int32_t rr_k, const int32_t* d_q_tok,
                                  const int32_t* d_q_off, int32_t n_queries, int32_t cls_id, int32_t sep_id, int64_t first_pair,
                                  int32_t n_pairs, const int32_t* d_keep, const int32_t* d_cu, int64_t n_tokens, int32_t* d_tok,
                                  int32_t* d_typ, int32_t* d_pos, void* stream) {
    RR_REQUIRE(h && d_plane_off && d_rows && d_q_off && d_keep && d_cu, "rr_pairs_write_dev: NULL argument");
    RR_REQUIRE(d_plane_tok && d_q_tok, "rr_pairs_write_dev: NULL plane or query ids (pass a buffer of at least one element when "
               "there are none)");
    int rc = rp_check_range("rr_pairs_write_dev", n_docs, pool, rr_k, n_queries, first_pair, n_pairs);
    if (rc != RR_OK) return rc;
    RR_REQUIRE(n_tokens >= 0 && n_tokens <= RP_MAX_TOKENS, "rr_pairs_write_dev: %lld tokens, more than the %lld one "
               "rr_ce_forward_dev call takes", (long long)n_tokens, (long long)RP_MAX_TOKENS);
    RR_REQUIRE((d_tok && d_typ && d_pos) || n_tokens == 0, "rr_pairs_write_dev: NULL output");
    if (n_pairs == 0 || n_tokens == 0) return RR_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    RR_HIP_TRY(hipSetDevice(h->device));
    int64_t blocks = ((int64_t)n_pairs + RP_WAVES - 1) / RP_WAVES;
    if (blocks > RP_MAX_BLOCKS) blocks = RP_MAX_BLOCKS;
    hipLaunchKernelGGL(rp_write, dim3((unsigned)blocks), dim3(RP_THREADS), 0, (hipStream_t)stream, d_plane_tok, d_plane_off, n_docs,
                       row_offset, d_rows, pool, rr_k, d_q_tok, d_q_off, cls_id, sep_id, first_pair, n_pairs, d_keep, d_cu, n_tokens,
                       d_tok, d_typ, d_pos, h->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_pairs_status(rr_pairs* h, int32_t* out_bad) {
    RR_REQUIRE(h && out_bad, "rr_pairs_status: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    RR_HIP_TRY(hipSetDevice(h->device));
    int32_t bad[2] = {0, 0};
    RR_HIP_TRY(hipDeviceSynchronize());
    RR_HIP_TRY(hipMemcpy(bad, h->d_bad, 8, hipMemcpyDeviceToHost));
    RR_HIP_TRY(hipMemset(h->d_bad, 0, 8));
    *out_bad = bad[0] + bad[1];
    RR_REQUIRE(bad[0] == 0, "rr_pairs_measure_dev: %d pair(s) whose candidate row lies outside the plane (no text was read: the "
               "sequence is [CLS] query [SEP] [SEP]) or whose offsets decrease", bad[0]);
    RR_REQUIRE(bad[1] == 0, "rr_pairs_write_dev: %d pair(s) whose kept lengths or offsets do not fit the plane, the queries or "
               "the outputs (nothing was written for them)", bad[1]);
    return RR_OK;
}
