// rr_prims.h -- what the index builders share (rr_wordpiece.hip, rr_textprep.hip, rr_doctok.hip, rr_bm25_build.hip,
// rr_products.hip) and the query front (rr_query.hip): the workgroup scan, the device-wide scan, the stable radix sort, the
// vocabulary table, and the small helpers every builder needs once.
#pragma once

#include "rr_common.h"

// ---------------------------------------------------------------- host helpers
// Grows *p to `want` elements of `elem` bytes (the old contents are dropped; hipFree waits for the kernels that use them).
static inline int rr_grow(void** p, int64_t* cap, int64_t want, size_t elem, const char* who) {
    if (want <= *cap) return RR_OK;
    if (*p) RR_HIP_TRY(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    if (hipMalloc(p, elem * (size_t)want) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        rr_set_error("%s: no memory for %lld x %zu bytes", who, (long long)want, elem);
        return RR_E_NOMEM;
    }
    *cap = want;
    return RR_OK;
}

// The documents whose offsets the kernels refused since the last call: waits for the device, reads the counter, clears it.
static inline int rr_take_bad_docs(int32_t* d_bad, int32_t* out) {
    RR_HIP_TRY(hipDeviceSynchronize());
    RR_HIP_TRY(hipMemcpy(out, d_bad, 4, hipMemcpyDeviceToHost));
    RR_HIP_TRY(hipMemset(d_bad, 0, 4));
    return RR_OK;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ uint64_t rr_mix64(uint64_t x) {             // murmur3's 64-bit finaliser
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}

// Document `doc` of a packed text: its first byte and its length.  false = the offsets decrease or leave the text, and
// nothing of it may be read.
__device__ __forceinline__ bool rr_doc_span(const int64_t* __restrict__ text_off, int doc, int64_t text_bytes, int64_t* b0,
                                            int64_t* len) {
    const int64_t a = text_off[doc], b = text_off[doc + 1];
    *b0 = a;
    *len = b - a;
    return a >= 0 && b >= a && b <= text_bytes;
}

// The character that starts at s[i] (i < len, s[i] not 10xxxxxx): its length in bytes and code point; 0 = malformed
// (a byte that starts nothing, too few or wrong continuation bytes before s[len], overlong, surrogate, > 10FFFF).
__device__ __forceinline__ int rr_utf8_decode(const uint8_t* s, int i, int len, uint32_t* cp) {
    const uint32_t b = s[i];
    if (b < 0x80u) { *cp = b; return 1; }
    int n;
    uint32_t c, lowest;
    if (b >= 0xC2u && b <= 0xDFu) { n = 2; c = b & 0x1Fu; lowest = 0x80u; }
    else if ((b & 0xF0u) == 0xE0u) { n = 3; c = b & 0x0Fu; lowest = 0x800u; }
    else if (b >= 0xF0u && b <= 0xF4u) { n = 4; c = b & 0x07u; lowest = 0x10000u; }
    else return 0;
    if (i + n > len) return 0;
    for (int k = 1; k < n; ++k) {
        const uint32_t t = s[i + k];
        if ((t & 0xC0u) != 0x80u) return 0;
        c = (c << 6) | (t & 0x3Fu);
    }
    if (c < lowest || c > 0x10FFFFu || (c >= 0xD800u && c <= 0xDFFFu)) return 0;
    *cp = c;
    return n;
}

// ---------------------------------------------------------------- the workgroup scan
// Exclusive sum of one T (int or long long) per thread over a workgroup of NT threads; *total = the sum, in every thread.
// Every thread of the workgroup calls it.  wave_sums: LDS [NT / 64]; the leading barrier lets back-to-back calls share it.
template <typename T, int NT>
__device__ __forceinline__ T rr_block_scan(T v, T* wave_sums, T* total) {
    static_assert(NT % 64 == 0 && NT >= 64 && NT <= 1024, "a workgroup of whole waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    __syncthreads();                       // (wave_sums may still be read from the previous scan)
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const T s = wave_sums[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return before + incl - v;
}

// ---------------------------------------------------------------- the device-wide scan
// Exclusive int64 scan of f(0) .. f(n - 1): rr_scan_sum (a sum per chunk of RR_SCAN_CHUNK elements, one workgroup each),
// rr_scan_sums (one workgroup scans the chunk sums in place), rr_scan_apply (every chunk again, from its sum onwards).
#define RR_SCAN_CHUNK 4096

static inline int64_t rr_scan_sums_len(int64_t n) { return n / RR_SCAN_CHUNK + 1; }   // the `sums` rr_scan needs for n elements

template <class F>
__global__ __launch_bounds__(256) void rr_scan_sum(F f, int64_t n, int64_t* __restrict__ sums) {
    __shared__ long long s_ws[4];
    const int64_t c0 = (int64_t)blockIdx.x * RR_SCAN_CHUNK;
    long long v = 0;
    for (int r = 0; r < RR_SCAN_CHUNK / 256; ++r) {
        const int64_t i = c0 + r * 256 + threadIdx.x;
        if (i < n) v += f(i);
    }
    long long total;
    rr_block_scan<long long, 256>(v, s_ws, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

template <int NT>   // (a template, so that only the sources that scan carry the kernel)
__global__ __launch_bounds__(NT) void rr_scan_sums(int64_t* __restrict__ sums, int64_t nb, int64_t* __restrict__ total_out) {
    __shared__ long long s_ws[NT / 64];
    long long carry = 0;
    for (int64_t base = 0; base < nb; base += NT) {
        const int64_t i = base + threadIdx.x;
        const long long v = i < nb ? sums[i] : 0;
        long long total;
        const long long at = rr_block_scan<long long, NT>(v, s_ws, &total);
        if (i < nb) sums[i] = carry + at;
        carry += total;
    }
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}

// out64[i] / out32[i] = the exclusive sum in front of element i; out64[n] = the total.  (No __restrict__ on the outputs:
// see rr_scan.)
template <class F>
__global__ __launch_bounds__(256) void rr_scan_apply(F f, int64_t n, const int64_t* __restrict__ sums, int64_t nb, int64_t* out64,
                                                     int32_t* out32) {
    __shared__ long long s_ws[4];
    const int64_t c0 = (int64_t)blockIdx.x * RR_SCAN_CHUNK;
    long long carry = sums[blockIdx.x];
    for (int r = 0; r < RR_SCAN_CHUNK / 256; ++r) {
        const int64_t i = c0 + r * 256 + threadIdx.x;
        const long long v = i < n ? f(i) : 0;
        long long total;
        const long long at = rr_block_scan<long long, 256>(v, s_ws, &total);
        if (i < n) {
            if (out64) out64[i] = carry + at;
            if (out32) out32[i] = (int32_t)(carry + at);
        }
        carry += total;
    }
    if (out64 && blockIdx.x == nb - 1 && threadIdx.x == 0) out64[n] = carry;
}

// Exclusive scan of f over [0, n) on `st`: out64 [n + 1] and / or out32 [n] (either may be NULL), *total (may be NULL);
// `sums`: rr_scan_sums_len(n) words of the caller's.  An output may be the array f reads: a thread writes only the element
// it has just read, every read of rr_scan_sum is over before rr_scan_apply starts, and out64[n] lies behind the input.
template <class F>
static void rr_scan(F f, int64_t n, int64_t* sums, int64_t* out64, int32_t* out32, int64_t* total, hipStream_t st) {
    const int64_t nb = (n + RR_SCAN_CHUNK - 1) / RR_SCAN_CHUNK;
    if (nb == 0) {
        if (out64) hipMemsetAsync(out64, 0, sizeof(int64_t), st);
        if (total) hipMemsetAsync(total, 0, sizeof(int64_t), st);
        return;
    }
    hipLaunchKernelGGL(rr_scan_sum<F>, dim3((unsigned)nb), dim3(256), 0, st, f, n, sums);
    hipLaunchKernelGGL(rr_scan_sums<1024>, dim3(1), dim3(1024), 0, st, sums, nb, total);
    if (out64 || out32) hipLaunchKernelGGL(rr_scan_apply<F>, dim3((unsigned)nb), dim3(256), 0, st, f, n, sums, nb, out64, out32);
}

// ---------------------------------------------------------------- the stable radix sort
// LSD, 8-bit digits, 32-bit keys with up to two 32-bit payload arrays.  A pass is
//   rr_sort_hist     per-tile digit counts (a tile = RR_SORT_TILE elements, one workgroup);
//   rr_scan          exclusive scan of the digit-major count matrix (int64) -> where every (digit, tile) run starts;
//   rr_sort_scatter  the tile in rounds of 256 elements, in input order: a wave's lanes with the same digit find each other
//                    with eight __ballot masks, rank themselves with a popcount below their lane, and add the counts of the
//                    waves before them.  The order of the writes does not depend on atomics (stable).
// Every element count and offset is int64.
#define RR_SORT_THREADS 256
#define RR_SORT_ROUNDS 16
#define RR_SORT_TILE (RR_SORT_THREADS * RR_SORT_ROUNDS)

static inline int64_t rr_sort_tiles(int64_t n) { return (n + RR_SORT_TILE - 1) / RR_SORT_TILE; }
// the words a sort of n elements needs besides its buffers: `hist` and `offs` (one more) of rr_sort_counts(n) int64 each,
// and rr_scan_sums_len(rr_sort_counts(n)) chunk sums
static inline int64_t rr_sort_counts(int64_t n) { return 256 * rr_sort_tiles(n); }

static inline int rr_sort_passes(uint32_t max_key) {   // at least one
    int bits = 0;
    while (bits < 32 && (max_key >> bits)) ++bits;
    return bits ? (bits + 7) / 8 : 1;
}

template <int ROUNDS>   // (templates, so that only the sources that sort carry the kernels)
__global__ __launch_bounds__(RR_SORT_THREADS) void rr_sort_hist(const uint32_t* __restrict__ key, int64_t n, int shift,
                                                                int64_t n_tiles, int64_t* __restrict__ hist) {
    __shared__ unsigned cnt[256];
    const int tid = threadIdx.x;
    cnt[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (RR_SORT_THREADS * ROUNDS);
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t i = base + r * RR_SORT_THREADS + tid;
        if (i < n) atomicAdd(&cnt[(key[i] >> shift) & 255u], 1u);     // (a count: the same whatever the order)
    }
    __syncthreads();
    hist[(int64_t)tid * n_tiles + blockIdx.x] = cnt[tid];               // digit-major: the scan gives stable offsets
}

// the mask of the active lanes of this wave that hold the same 8-bit digit
__device__ __forceinline__ uint64_t rr_match8(unsigned d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const uint64_t bb = __ballot((d >> b) & 1u);
        m &= ((d >> b) & 1u) ? bb : ~bb;
    }
    return m;
}

template <int NP>
__global__ __launch_bounds__(RR_SORT_THREADS) void rr_sort_scatter(const uint32_t* __restrict__ kin,
                                                                   const uint32_t* __restrict__ p0in,
                                                                   const uint32_t* __restrict__ p1in, int64_t n, int shift,
                                                                   int64_t n_tiles, const int64_t* __restrict__ offs,
                                                                   uint32_t* __restrict__ kout, uint32_t* __restrict__ p0out,
                                                                   uint32_t* __restrict__ p1out) {
    __shared__ int64_t run[256];                        // next output position of every digit
    __shared__ unsigned wc[RR_SORT_THREADS / 64][256];  // this round: elements of every digit per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    run[tid] = offs[(int64_t)tid * n_tiles + blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * RR_SORT_TILE;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int r = 0; r < RR_SORT_ROUNDS; ++r) {
#pragma unroll
        for (int w = 0; w < RR_SORT_THREADS / 64; ++w) wc[w][tid] = 0;
        __syncthreads();
        const int64_t i = base + r * RR_SORT_THREADS + tid;
        const bool valid = i < n;
        const uint32_t k = valid ? kin[i] : 0u;
        const unsigned d = (k >> shift) & 255u;
        const uint64_t m = rr_match8(d, valid);
        const int rank = __popcll(m & below);
        if (valid && rank == 0) wc[wave][d] = (unsigned)__popcll(m);
        __syncthreads();
        if (valid) {
            int64_t pos = run[d] + rank;
            for (int w = 0; w < wave; ++w) pos += wc[w][d];
            kout[pos] = k;
            if (NP >= 1) p0out[pos] = p0in[i];
            if (NP >= 2) p1out[pos] = p1in[i];
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (int w = 0; w < RR_SORT_THREADS / 64; ++w) add += wc[w][tid];
        run[tid] += add;
    }
}

struct rr_f_i64 {   // what a scan over an int64 array sums
    const int64_t* in;
    __device__ __forceinline__ long long operator()(int64_t i) const { return in[i]; }
};

// Stable sort of n keys by their low 8 * passes bits with NP payload arrays: pass p reads the source (p == 0) or buffer
// (p - 1) & 1 and writes buffer p & 1; the sources are never written, and a source may be buffer 1 (pass 0 writes buffer 0
// and nothing reads the source after it).  The result is in buffer (passes - 1) & 1.  hist, offs, scan_sums: see
// rr_sort_counts.
template <int NP>
static int rr_radix_sort(hipStream_t st, int64_t n, int passes, const uint32_t* ksrc, const uint32_t* p0src,
                         const uint32_t* p1src, uint32_t* const K[2], uint32_t* const P0[2], uint32_t* const P1[2],
                         int64_t* hist, int64_t* offs, int64_t* scan_sums) {
    if (n == 0) return RR_OK;
    const int64_t nt = rr_sort_tiles(n), m = 256 * nt;
    for (int p = 0; p < passes; ++p) {
        const uint32_t* kin = p == 0 ? ksrc : K[(p - 1) & 1];
        const uint32_t* a_in = p == 0 ? p0src : (NP >= 1 ? P0[(p - 1) & 1] : nullptr);
        const uint32_t* b_in = p == 0 ? p1src : (NP >= 2 ? P1[(p - 1) & 1] : nullptr);
        hipLaunchKernelGGL(rr_sort_hist<RR_SORT_ROUNDS>, dim3((unsigned)nt), dim3(RR_SORT_THREADS), 0, st, kin, n, 8 * p, nt,
                           hist);
        RR_HIP_TRY(hipGetLastError());
        rr_scan(rr_f_i64{hist}, m, scan_sums, offs, (int32_t*)nullptr, (int64_t*)nullptr, st);
        hipLaunchKernelGGL((rr_sort_scatter<NP>), dim3((unsigned)nt), dim3(RR_SORT_THREADS), 0, st, kin, a_in, b_in, n, 8 * p,
                           nt, offs, K[p & 1], NP >= 1 ? P0[p & 1] : nullptr, NP >= 2 ? P1[p & 1] : nullptr);
        RR_HIP_TRY(hipGetLastError());
    }
    return RR_OK;
}

// ---------------------------------------------------------------- the vocabulary table
// An open-addressing table over a list of strings (bytes + int64 offsets; string p has id p), built on the host and probed
// on the device: the WordPiece pieces (rr_wordpiece.hip) and the BM25 vocabulary of the query front (rr_query.hip).  A
// string is found by the polynomial hash of its bytes and a KEY word, its length in bytes plus whatever else tells two
// strings of the same bytes apart (WordPiece: the ## form << 16).  The slots are what the Python side and the tests read
// as [n_slots][4] int32.
#define RR_TAB_BASE 0x01000193u                        // odd: the polynomial hash is taken mod 2^32

struct rr_tab_entry {    // one slot, 16 bytes; id < 0 = empty
    uint32_t hash;       // polynomial hash of the bytes compared
    int32_t off;         // their first byte in the list's bytes
    int32_t key;
    int32_t id;
};

__host__ __device__ static inline uint32_t rr_tab_slot_of(uint32_t hash, int32_t key) {
    uint32_t h = hash ^ ((uint32_t)key * 0x9E3779B1u);
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;     // murmur3's finaliser
    return h;
}

static inline int32_t rr_tab_slots_for(int32_t n) {    // a power of two, at least 64 and at least 2 n (n <= 2^28)
    int32_t slots = 64;
    while (slots < 2 * (int64_t)n) slots <<= 1;
    return slots;
}

// Fills `slots` from the n strings.  filter(a, b, &first, &key) says of the string at bytes [a, b) whether it is kept, and
// if so which bytes are compared, [first, b), and under which key.  A string listed twice keeps its LAST id (what a dict
// built from the list holds).  Returns the strings kept, or -1 when n_slots is too small.
template <class Filter>
static int64_t rr_tab_fill(const uint8_t* bytes, const int64_t* off, int32_t n, int32_t n_slots, rr_tab_entry* slots,
                           Filter filter) {
    for (int32_t s = 0; s < n_slots; ++s) slots[s] = rr_tab_entry{0u, 0, 0, -1};
    int64_t kept = 0;
    for (int32_t p = 0; p < n; ++p) {
        int64_t a = 0;
        const int64_t b = off[p + 1];
        int32_t key = 0;
        if (!filter(off[p], b, &a, &key)) continue;
        uint32_t h = 0;
        for (int64_t i = a; i < b; ++i) h = h * RR_TAB_BASE + bytes[i];
        if (2 * (kept + 1) > n_slots) return -1;
        uint32_t s = rr_tab_slot_of(h, key) & (uint32_t)(n_slots - 1);
        bool dup = false;
        while (slots[s].id >= 0) {
            if (slots[s].hash == h && slots[s].key == key && memcmp(bytes + slots[s].off, bytes + a, (size_t)(b - a)) == 0) {
                dup = true;
                break;
            }
            s = (s + 1) & (uint32_t)(n_slots - 1);
        }
        slots[s] = rr_tab_entry{h, (int32_t)a, key, p};
        if (!dup) ++kept;
    }
    return kept;
}

// The id of the string of `len` bytes at `word` with this hash and key, or -1.  One 16-byte load per slot; hash and key are
// compared before the bytes.  (The table is at most half full: an empty slot ends the walk.)
__device__ __forceinline__ int rr_tab_lookup(const rr_tab_entry* __restrict__ table, uint32_t mask, const uint8_t* __restrict__ bytes,
                                             uint32_t hash, int32_t key, int len, const uint8_t* word) {
    uint32_t s = rr_tab_slot_of(hash, key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes) {
        const int4 raw = *reinterpret_cast<const int4*>(table + s);
        if (raw.w < 0) return -1;
        if ((uint32_t)raw.x == hash && raw.z == key) {
            const uint8_t* p = bytes + raw.y;
            int k = 0;
            while (k < len && p[k] == word[k]) ++k;
            if (k == len) return raw.w;
        }
        s = (s + 1) & mask;
    }
    return -1;
}

#endif  // __HIPCC__
