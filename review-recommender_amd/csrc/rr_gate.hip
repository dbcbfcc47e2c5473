// rr_gate.hip -- the attribute gate on the device: the gate plane of the product texts, built once per index, and the match
// of a batch's query terms against the texts of its candidates (gfx950).
//
// Stands in for calculate_gate_factor (utils.py:88-101 = _gate_factor app/app_product_search.py:228-236) as both front-ends
// call it (app/app_product_search.py:297-302, app/test.py:292-297): a group of terms hits when any of its terms occurs as a
// substring of agg_text[:6000].lower(), and the factor is penalty ** (groups that missed).  gate.model_gate_plane and
// gate.model_gate_hits state in Python what the two halves compute.
//
// THE PLANE.  For every document the byte image of its first max_chars code points (code points = the bytes that are not
// 10xxxxxx), such that for every string s of ASCII characters: s in text[:max_chars].lower() <=> s's bytes occur in the
// image.  Byte by byte over the UTF-8 text:
//   A-Z                 -> a-z;
//   C4 B0    (U+0130)   -> 69 B0: str.lower() gives 'i' + U+0307, i.e. an 'i' with a non-ASCII character behind it;
//   E2 84 AA (U+212A)   -> 6B: str.lower() gives 'k'; the two continuation bytes are dropped, so its neighbours are adjacent;
//   every other byte    -> itself (every byte of every other non-ASCII character is >= 0x80).
// U+0130 and U+212A are the only two code points outside ASCII whose lower() holds an ASCII character
// (tests/test_gate_model.py derives the list).  The image need not be valid UTF-8.
//   gt_plane<false>  a workgroup per document, GT_STEP bytes per step, GT_PER consecutive bytes per thread: ONE block scan per
//                    step carries the code points so far (high word) and the bytes emitted so far (low word); the thread that
//                    holds the first byte of code point max_chars + 1 knows the image's length.  The walk stops at the step
//                    that holds it: a 100 KB document is read to its 6000th code point.
//   rr_scan          (rr_prims.h) lengths -> d_plane_off [n + 1] and the total, the only number the host reads back.
//   gt_plane<true>   the same walk, writing.
//
// THE MATCH (gt_match).  One wave per (query, candidate), GT_WAVES candidates of one query per workgroup.
//   - the query's terms are staged in LDS once per workgroup, with head[first byte] -> the first term that starts with it
//     and next[term] -> the next one: the first-byte filter of a text position is one LDS byte, and only the terms that
//     share the byte are compared;
//   - the image is read in ALIGNED 16-byte words, 64 of them per step (GT_MSTEP bytes) plus the GT_MAX_TERM bytes behind
//     them, into the wave's LDS window.  A word is loaded only when it holds a byte of the document; the bytes of a
//     boundary word that lie in front of the document's first byte or behind its last are replaced by FF, which no term
//     byte equals (terms are ASCII): a neighbouring document can never complete a match, and no compare needs a length
//     check.  The plane has GT_SLACK bytes behind its last document, so the last word may be read whole;
//   - every lane tests the 16 start positions of its own word; a group that has hit is not compared again, and a wave
//     whose groups have all hit reads no more text (the exit is wave-uniform; the step loop itself runs the workgroup's
//     longest document so that the barriers around the window are uniform);
//   - the result is the OR of the lanes' masks: no order of anything depends on the data.
// The kernel does no floating point: d_gate = d_factor[query][groups missed], a table the host fills with the
// reference's own arithmetic.
#include "rr_prims.h"

#define GT_THREADS 256
#define GT_PER 16                                  // consecutive bytes per thread (plane), bytes per load (match)
#define GT_STEP (GT_THREADS * GT_PER)              // bytes of a document per step of the plane kernels
#define GT_WAVES 4                                 // candidates per workgroup of the match
#define GT_MSTEP (64 * GT_PER)                     // bytes of an image per step of a wave of the match
#define GT_MAX_TERM 64                             // longest term, bytes
#define GT_TERM_BYTES 1024                         // term bytes per query
#define GT_MAX_TERMS 64                            // terms per query
#define GT_MAX_GROUPS 6                            // groups per query (text.MAX_GATE_GROUPS)
#define GT_SLACK 16                                // readable bytes behind the plane's last document
#define GT_WIN_WORDS (64 + GT_MAX_TERM / GT_PER)   // 16-byte words of a wave's window

struct rr_gate {
    int device = 0;
    int32_t* d_bad = nullptr;           // [0] documents the plane kernels refused, [1] rows / queries the match refused
    int64_t* d_scratch = nullptr;       // image lengths [n], chunk sums of the scan
    int64_t cap_words = 0;
    std::mutex mu;
};

// ------------------------------------------------------------------------------------------------ the plane
template <bool WRITE>
__global__ __launch_bounds__(GT_THREADS) void gt_plane(const uint8_t* __restrict__ text, int64_t text_bytes,
                                                       const int64_t* __restrict__ text_off, int32_t n_docs, int32_t max_chars,
                                                       int64_t* __restrict__ lens, const int64_t* __restrict__ out_off,
                                                       uint8_t* __restrict__ out, int64_t out_bytes, int32_t* __restrict__ bad) {
    __shared__ long long s_ws[GT_THREADS / 64];
    const int tid = threadIdx.x, doc = blockIdx.x;
    int64_t b0, len;
    if (!rr_doc_span(text_off, doc, text_bytes, &b0, &len)) {     // nothing of it is read; its image is empty
        if (!WRITE && tid == 0) { lens[doc] = 0; atomicAdd(bad, 1); }
        return;
    }
    int64_t dst = 0, dst_end = 0;
    if (WRITE) {
        if (out_off[n_docs] > out_bytes) {                          // the capacity is too small: no workgroup writes anything
            if (doc == 0 && tid == 0) atomicAdd(bad, 1);
            return;
        }
        dst = out_off[doc];
        dst_end = out_off[doc + 1];
    }
    const uint8_t* __restrict__ src = text + b0;
    long long base = 0;                                             // code points so far << 32 | bytes emitted so far
    bool cut_seen = false;
    for (int64_t s0 = 0; s0 < len; s0 += GT_STEP) {
        const int64_t i0 = s0 + (int64_t)tid * GT_PER;
        uint8_t c[GT_PER];
        unsigned drop = 0, lead = 0;                                // bit k: byte k is the tail of a U+212A / starts a code point
        int kept = 0;
#pragma unroll
        for (int k = 0; k < GT_PER; ++k) {
            const int64_t i = i0 + k;
            uint8_t b = 0x80;                                       // (behind the document: counts as nothing)
            bool dr = true;
            if (i < len) {
                b = src[i];
                dr = false;
                lead |= ((b & 0xC0) != 0x80 ? 1u : 0u) << k;
                if (b >= 'A' && b <= 'Z') b += 32;
                else if (b == 0xC4) { if (i + 1 < len && src[i + 1] == 0xB0) b = 'i'; }
                else if (b == 0xE2) { if (i + 2 < len && src[i + 1] == 0x84 && src[i + 2] == 0xAA) b = 'k'; }
                else if (b == 0x84) dr = i >= 1 && i + 1 < len && src[i - 1] == 0xE2 && src[i + 1] == 0xAA;
                else if (b == 0xAA) dr = i >= 2 && src[i - 2] == 0xE2 && src[i - 1] == 0x84;
            }
            c[k] = b;
            drop |= (dr ? 1u : 0u) << k;
            kept += dr ? 0 : 1;
        }
        long long total;
        const long long at = base + rr_block_scan<long long, GT_THREADS>(((long long)__popc(lead) << 32) | kept, s_ws, &total);
        long long cp = at >> 32;                                    // code points in front of this thread's bytes
        int64_t pos = (int64_t)(at & 0xFFFFFFFFll);                 // image bytes in front of them
        bool open = cp <= max_chars;                                // (false: the cut lies in front of this thread)
#pragma unroll
        for (int k = 0; k < GT_PER; ++k) {
            const bool in = open && i0 + k < len;
            cp += in ? (lead >> k) & 1u : 0u;
            if (in && cp > max_chars) {                             // the first byte of code point max_chars + 1: the cut
                if (!WRITE) lens[doc] = pos;
                open = false;
            } else if (in && !((drop >> k) & 1u)) {
                if (WRITE && dst + pos < dst_end) out[dst + pos] = c[k];
                ++pos;
            }
        }
        base += total;
        if ((base >> 32) > max_chars) { cut_seen = true; break; }  // (the same in every thread)
    }
    if (!WRITE && !cut_seen && tid == 0) lens[doc] = base & 0xFFFFFFFFll;
}

// ------------------------------------------------------------------------------------------------ the match
__global__ __launch_bounds__(GT_THREADS) void gt_match(const uint8_t* __restrict__ plane, const int64_t* __restrict__ plane_off,
                                                       int64_t plane_bytes, int32_t n_docs, int64_t row_offset, const int64_t* __restrict__ rows,
                                                       int32_t pool, const uint8_t* __restrict__ term_bytes,
                                                       const int32_t* __restrict__ term_off, const int32_t* __restrict__ term_group,
                                                       const int32_t* __restrict__ q_term, const int32_t* __restrict__ q_groups,
                                                       const float* __restrict__ factor, float* __restrict__ gate,
                                                       int32_t* __restrict__ hits_out, int32_t* __restrict__ bad) {
    __shared__ uint4 s_win[GT_WAVES][GT_WIN_WORDS];
    __shared__ uint8_t s_tb[GT_TERM_BYTES];
    __shared__ int32_t s_toff[GT_MAX_TERMS + 1];
    __shared__ int8_t s_tgrp[GT_MAX_TERMS], s_next[GT_MAX_TERMS], s_head[128];
    __shared__ int32_t s_steps[GT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    const int cand = blockIdx.x * GT_WAVES + wave;                  // (wave-uniform)

    // ---- the query's terms, once per workgroup
    const int t0 = q_term[q], t1 = q_term[q + 1];
    int n_groups = q_groups[q], n_terms = t1 - t0;
    const int tb0 = term_off[t0];
    int wrong = n_groups < 0 || n_groups > GT_MAX_GROUPS || n_terms < 0 || n_terms > GT_MAX_TERMS;
    if (!wrong) {
        const int nb = term_off[t1] - tb0;
        wrong = nb < 0 || nb > GT_TERM_BYTES;
        if (!wrong) {
            for (int i = tid; i < nb; i += GT_THREADS) {
                const uint8_t b = term_bytes[tb0 + i];
                s_tb[i] = b;
                wrong |= b >= 0x80;
            }
            if (tid < n_terms) {
                const int o = term_off[t0 + tid] - tb0, m = term_off[t0 + tid + 1] - tb0 - o, g = term_group[t0 + tid];
                wrong |= o < 0 || m < 1 || m > GT_MAX_TERM || o + m > nb || g < 0 || g >= n_groups;
                s_toff[tid] = o;
                s_tgrp[tid] = (int8_t)g;
                if (tid == n_terms - 1) s_toff[n_terms] = o + m;
            }
        }
    }
    if (tid < 128) s_head[tid] = -1;
    wrong = __syncthreads_or(wrong);
    if (wrong) {                                                    // a packing the kernel cannot hold: the query is not gated
        n_groups = 0;
        n_terms = 0;
        if (blockIdx.x == 0 && tid == 0) atomicAdd(bad + 1, 1);
    }
    if (tid < n_terms) {                                            // the chains of the terms that share a first byte, ascending
        const uint8_t f = s_tb[s_toff[tid]];
        int nx = -1;
        bool first = true;
        for (int t = 0; t < n_terms; ++t) {
            const bool same = s_tb[s_toff[t]] == f;
            if (same && t < tid) first = false;
            if (same && t > tid && nx < 0) nx = t;
        }
        s_next[tid] = (int8_t)nx;
        if (first) s_head[f] = (int8_t)tid;
    }

    // ---- this wave's document
    int64_t a = 0, b = 0;
    bool have = false;
    if (cand < pool && n_groups > 0) {
        const int64_t r = rows[(int64_t)q * pool + cand] - row_offset;
        bool ok = r >= 0 && r < n_docs;
        if (ok) {
            a = plane_off[r];
            b = plane_off[r + 1];
            ok = a >= 0 && b >= a && b <= plane_bytes;
            have = ok && b > a;
        }
        if (!ok && lane == 0) atomicAdd(bad + 1, 1);               // a row outside the plane (or offsets that leave it): no text is read
    }
    const int64_t w0 = a & ~(int64_t)(GT_PER - 1);                  // the aligned word that holds the first byte
    const int my_steps = have ? (int)((b - w0 + GT_MSTEP - 1) / GT_MSTEP) : 0;
    if (lane == 0) s_steps[wave] = my_steps;
    __syncthreads();
    int steps = 0;
#pragma unroll
    for (int w = 0; w < GT_WAVES; ++w) steps = s_steps[w] > steps ? s_steps[w] : steps;

    const unsigned all = (1u << n_groups) - 1u;
    unsigned hit = 0;                                               // (wave-uniform)
    uint8_t* win = (uint8_t*)s_win[wave];
    for (int st = 0; st < steps; ++st) {
        const bool active = st < my_steps && hit != all;
        uint4 mine = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (active) {
            // words lane (this step) and, in the lanes below GT_MAX_TERM / GT_PER, 64 + lane (what a match may run into)
            for (int part = 0; part < 2; ++part) {
                if (part == 1 && lane >= GT_MAX_TERM / GT_PER) break;
                const int wi = part * 64 + lane;
                const int64_t w = w0 + (int64_t)st * GT_MSTEP + (int64_t)wi * GT_PER;
                uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
                if (w < b && w + GT_PER > a) {                      // it holds a byte of this document
                    v = *(const uint4*)(plane + w);
                    if (w < a || w + GT_PER > b) {                  // a boundary word: the neighbours' bytes become FF
                        uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int k = 0; k < GT_PER; ++k)
                            if (w + k < a || w + k >= b) d[k >> 2] |= 0xFFu << (8 * (k & 3));
                        v = make_uint4(d[0], d[1], d[2], d[3]);
                    }
                }
                s_win[wave][wi] = v;
                if (part == 0) mine = v;
            }
        }
        __syncthreads();
        if (active) {
            unsigned found = 0;
            const uint32_t d[4] = {mine.x, mine.y, mine.z, mine.w};
#pragma unroll
            for (int k = 0; k < GT_PER; ++k) {
                const uint32_t c = (d[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                if (c >= 0x80u) continue;
                const uint8_t* at = win + lane * GT_PER + k;
                for (int t = s_head[c]; t >= 0; t = s_next[t]) {
                    const unsigned gbit = 1u << s_tgrp[t];
                    if ((hit | found) & gbit) continue;
                    const int o = s_toff[t], m = s_toff[t + 1] - o;
                    int j = 1;
                    while (j < m && at[j] == s_tb[o + j]) ++j;      // (at[j] stays inside the window: j < GT_MAX_TERM)
                    if (j == m) found |= gbit;
                }
            }
#pragma unroll
            for (int dlt = 32; dlt >= 1; dlt >>= 1) found |= __shfl_xor(found, dlt, 64);
            hit |= found;
        }
        __syncthreads();                                            // (the window is overwritten by the next step)
    }
    if (cand < pool && lane == 0) {
        const int64_t o = (int64_t)q * pool + cand;
        gate[o] = factor[q * (GT_MAX_GROUPS + 1) + (n_groups - __popc(hit))];
        if (hits_out) hits_out[o] = (int32_t)hit;
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int rr_gate_destroy(rr_gate* g) {
    if (!g) return RR_OK;
    hipSetDevice(g->device);
    hipDeviceSynchronize();
    hipFree(g->d_bad); hipFree(g->d_scratch);
    delete g;
    return RR_OK;
}

extern "C" int rr_gate_create(int32_t device, rr_gate** out) {
    RR_REQUIRE(out, "rr_gate_create: NULL out");
    *out = nullptr;
    RR_HIP_TRY(hipSetDevice(device));
    rr_gate* g = new rr_gate();
    g->device = device;
    hipError_t e = hipMalloc((void**)&g->d_bad, 8);
    if (e == hipSuccess) e = hipMemset(g->d_bad, 0, 8);
    if (e != hipSuccess) {
        rr_set_error("rr_gate_create: %s", hipGetErrorString(e));
        rr_gate_destroy(g);
        return RR_E_HIP;
    }
    *out = g;
    return RR_OK;
}

extern "C" int rr_gate_limits(int32_t* out_plane_step, int32_t* out_match_step, int32_t* out_per_thread, int32_t* out_max_term,
                              int32_t* out_term_bytes, int32_t* out_max_terms, int32_t* out_slack) {
    RR_REQUIRE(out_plane_step && out_match_step && out_per_thread && out_max_term && out_term_bytes && out_max_terms && out_slack,
               "rr_gate_limits: NULL argument");
    *out_plane_step = GT_STEP; *out_match_step = GT_MSTEP; *out_per_thread = GT_PER; *out_max_term = GT_MAX_TERM;
    *out_term_bytes = GT_TERM_BYTES; *out_max_terms = GT_MAX_TERMS; *out_slack = GT_SLACK;
    return RR_OK;
}

static int gt_check_text(const char* who, rr_gate* g, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                         int32_t n_docs, int32_t max_chars) {
    RR_REQUIRE(g && d_text_off, "%s: NULL argument", who);
    RR_REQUIRE(n_docs >= 0 && text_bytes >= 0 && max_chars >= 0, "%s: %d documents, %lld bytes, max_chars %d", who, n_docs,
               (long long)text_bytes, max_chars);
    RR_REQUIRE(d_text || text_bytes == 0, "%s: NULL text with %lld bytes", who, (long long)text_bytes);
    return RR_OK;
}

extern "C" int rr_gate_measure_dev(rr_gate* g, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                   int32_t n_docs, int32_t max_chars, int64_t* d_plane_off, int64_t* d_total, void* stream) {
    int rc = gt_check_text("rr_gate_measure_dev", g, d_text, text_bytes, d_text_off, n_docs, max_chars);
    if (rc != RR_OK) return rc;
    RR_REQUIRE(d_plane_off && d_total, "rr_gate_measure_dev: NULL output");
    std::lock_guard<std::mutex> lk(g->mu);
    RR_HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    rc = rr_grow((void**)&g->d_scratch, &g->cap_words, (int64_t)n_docs + 1 + rr_scan_sums_len(n_docs), sizeof(int64_t),
                 "rr_gate_measure_dev");
    if (rc != RR_OK) return rc;
    int64_t* lens = g->d_scratch;
    int64_t* sums = lens + n_docs + 1;
    if (n_docs > 0) {
        hipLaunchKernelGGL(gt_plane<false>, dim3((unsigned)n_docs), dim3(GT_THREADS), 0, st, d_text, text_bytes, d_text_off, n_docs,
                           max_chars, lens, (const int64_t*)nullptr, (uint8_t*)nullptr, (int64_t)0, g->d_bad);
        RR_HIP_TRY(hipGetLastError());
    }
    rr_scan(rr_f_i64{lens}, (int64_t)n_docs, sums, d_plane_off, (int32_t*)nullptr, d_total, st);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_gate_write_dev(rr_gate* g, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off, int32_t n_docs,
                                 int32_t max_chars, const int64_t* d_plane_off, uint8_t* d_plane, int64_t plane_bytes,
                                 void* stream) {
    int rc = gt_check_text("rr_gate_write_dev", g, d_text, text_bytes, d_text_off, n_docs, max_chars);
    if (rc != RR_OK) return rc;
    RR_REQUIRE(d_plane_off && plane_bytes >= 0 && (d_plane || plane_bytes == 0), "rr_gate_write_dev: NULL plane or offsets");
    if (n_docs == 0) return RR_OK;
    std::lock_guard<std::mutex> lk(g->mu);
    RR_HIP_TRY(hipSetDevice(g->device));
    hipLaunchKernelGGL(gt_plane<true>, dim3((unsigned)n_docs), dim3(GT_THREADS), 0, (hipStream_t)stream, d_text, text_bytes,
                       d_text_off, n_docs, max_chars, (int64_t*)nullptr, d_plane_off, d_plane, plane_bytes, g->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_gate_factors_dev(rr_gate* g, const uint8_t* d_plane, const int64_t* d_plane_off, int64_t plane_bytes, int32_t n_docs,
                                   int64_t row_offset, const int64_t* d_rows, int32_t n_queries, int32_t pool,
                                   const uint8_t* d_term_bytes, const int32_t* d_term_off, const int32_t* d_term_group,
                                   const int32_t* d_q_term, const int32_t* d_q_groups, const float* d_factor, float* d_gate,
                                   int32_t* d_hits, void* stream) {
    RR_REQUIRE(g && d_plane_off && d_rows && d_term_off && d_q_term && d_q_groups && d_factor && d_gate,
               "rr_gate_factors_dev: NULL argument");
    RR_REQUIRE(d_plane && d_term_bytes && d_term_group, "rr_gate_factors_dev: NULL plane or terms (pass a buffer of at least one "
               "element when there are none)");
    RR_REQUIRE(n_docs >= 0 && plane_bytes >= 0 && n_queries >= 0 && n_queries <= 65535 && pool >= 1, "rr_gate_factors_dev: %d "
               "documents, %lld bytes, %d queries, pool %d", n_docs, (long long)plane_bytes, n_queries, pool);
    RR_REQUIRE(((uintptr_t)d_plane & (GT_PER - 1)) == 0, "rr_gate_factors_dev: the plane must be %d-byte aligned", GT_PER);
    if (n_queries == 0) return RR_OK;
    std::lock_guard<std::mutex> lk(g->mu);
    RR_HIP_TRY(hipSetDevice(g->device));
    hipLaunchKernelGGL(gt_match, dim3((unsigned)((pool + GT_WAVES - 1) / GT_WAVES), (unsigned)n_queries), dim3(GT_THREADS), 0,
                       (hipStream_t)stream, d_plane, d_plane_off, plane_bytes, n_docs, row_offset, d_rows, pool, d_term_bytes, d_term_off,
                       d_term_group, d_q_term, d_q_groups, d_factor, d_gate, d_hits, g->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_gate_status(rr_gate* g, int32_t* out_bad) {
    RR_REQUIRE(g && out_bad, "rr_gate_status: NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    RR_HIP_TRY(hipSetDevice(g->device));
    int32_t bad[2] = {0, 0};
    RR_HIP_TRY(hipDeviceSynchronize());
    RR_HIP_TRY(hipMemcpy(bad, g->d_bad, 8, hipMemcpyDeviceToHost));
    RR_HIP_TRY(hipMemset(g->d_bad, 0, 8));
    *out_bad = bad[0] + bad[1];
    RR_REQUIRE(bad[0] == 0, "rr_gate_measure_dev / rr_gate_write_dev: %d document(s) had text offsets that decrease or leave the "
               "text (their images are empty), or the plane buffer was too small (nothing was written)", bad[0]);
    RR_REQUIRE(bad[1] == 0, "rr_gate_factors_dev: %d candidate row(s) outside the plane (no text was read for them: every group "
               "missed) or queries whose packed terms exceed rr_gate_limits (not gated)", bad[1]);
    return RR_OK;
}
