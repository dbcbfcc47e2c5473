// rr_doctok.hip -- the index-time tokenizer of the BM25 corpus and its vocabulary, on the device.
//
// Stands in for nlp/12_product_prep.py:42-49,75-83 (s.lower(), re.findall(r"[a-z0-9]+(?:'[a-z0-9]+)?"), the STOP set,
// len(t) > 1, the first 5000 tokens) and for pd.factorize(sort=False) over the tokens (bm25.factorize_corpus).
// doctok.model_tokenize states in plain Python what the walk kernel computes.
//
// Characters.  A byte is an ALNUM (0-9, a-z, A-Z lower-cased), an APOSTROPHE or a SEPARATOR.  Exactly two code points
// outside ASCII lower-case onto ASCII: U+212A KELVIN SIGN (E2 84 AA) is the alnum 'k' (its two continuation bytes are
// SKIPPED: they have no width), and U+0130 (C4 B0) is the alnum 'i' followed by a separator (U+0307), so C4 in front of B0
// is 'i' and B0 is what every other byte >= 0x80 is: a separator.  Nothing needs the host.
//
// The regex as an automaton over those classes (state: 0 outside, 1 in a token's first run, 2 behind the apostrophe that
// follows a first run, 3 in the second run):
//        alnum  apostrophe  separator
//   0      1        0          0          a token STARTS exactly where 0 reads an alnum
//   1      1        2          0
//   2      3        0          0
//   3      3        0          0          (a'b'c -> a'b, c: the apostrophe behind a second run joins nothing)
// A class is a map {0..3} -> {0..3} (8 bits) and maps compose, so the state in front of every byte of a tile comes from a
// scan of composed maps: each thread composes its RR_DT_PER bytes, a block scan composes the threads, and the state at the
// end of the tile is carried to the next (the chain's parity, the pending apostrophe and "inside a run" are all in it).
//
// rr_dt_walk<EMIT>   one workgroup per document, tiles of RR_DT_TILE bytes through LDS (16 bytes of the neighbours on
//                    either side, so the two multi-byte characters may straddle a tile edge).  The thread that holds a
//                    token's FIRST byte walks the token forward (LDS inside the tile's window, global memory beyond it: a
//                    token may be longer than any tile), maps its bytes, hashes them and applies the stop set (tokens of
//                    <= 8 bytes packed in one 64-bit word, compared with the packed stop words) and len > 1.  A block
//                    scan of the kept tokens gives each its index in the document; indices >= 5000 are dropped and the
//                    walk stops at the tile that reaches the cap.  EMIT = false counts, EMIT = true writes: the mapped
//                    bytes of a token go to the ARENA at the offset its first byte has in the text (a mapped token is
//                    never longer than its raw bytes, so tokens do not overlap and the arena is exactly as long as the
//                    text: no second prefix sum), and (arena offset, length, hash) to the token's global position
//                    doc_off[d] + index.  Between the passes: an int64 prefix sum over the documents.
// rr_dt_insert       one thread per token: open addressing, linear probing in a table of 2 T slots of one 64-bit word,
//                    the SMALLEST position seen of the term that owns the slot.  An empty slot is claimed by
//                    compare-and-swap; an occupied one is compared BYTE BY BYTE with the token its word names (any member
//                    of a term stands for it), then atomicMin.  A slot never changes its term, so equal tokens always
//                    meet in one slot, whichever of them claimed it.  The probe loop is bounded by the table's size.
// first / id         first[p] = (table[slot[p]] == p); the exclusive int64 scan of first is the term id in
//                    first-appearance order; a second sweep copies it to every token of the term.
// rr_dt_term_pos, rr_dt_gather    the vocabulary's bytes and offsets in id order, for the host.
// The prefix sums over documents, tokens and terms are rr_scan (rr_prims.h), the device-wide exclusive int64 scan.
#include "rr_prims.h"

#define RR_DT_THREADS 256
#define RR_DT_PER 16                                   // consecutive bytes per thread
#define RR_DT_TILE (RR_DT_THREADS * RR_DT_PER)         // 4096 bytes per step of the walk
#define RR_DT_HALO 16                                  // bytes of the neighbouring tiles held in LDS on either side
#define RR_DT_CAP 5000                                 // nlp/12_product_prep.py:78 (text.INDEX_TOKEN_CAP)
#define RR_DT_MAX_STOP 64
#define RR_DT_EMPTY 0xFFFFFFFFFFFFFFFFull

// control words on the device
#define RR_DT_C_BAD 0        // documents whose offsets decrease or leave the text (or with a token of >= 2^31 bytes)
#define RR_DT_C_T 1          // tokens counted by the last count call
#define RR_DT_C_FULL 2       // tokens that found no slot (cannot happen with 2 T slots; reported, never waited for)
#define RR_DT_C_TERMS 3
#define RR_DT_C_VBYTES 4
#define RR_DT_C_WORDS 8

struct rr_doctok {
    int device = 0;
    uint64_t* d_stop = nullptr;      // [RR_DT_MAX_STOP] stop words packed little-endian
    int32_t n_stop = 0;
    int64_t* d_ctl = nullptr;        // [RR_DT_C_WORDS]
    int32_t* d_cnt = nullptr;        // [cap_docs] kept tokens per document
    int64_t cap_docs = 0;
    uint8_t* d_arena = nullptr;      // [cap_arena] mapped token bytes at their text offsets
    int64_t cap_arena = 0;
    int64_t* d_pos = nullptr;        // [cap_tok] arena offset of a token
    int32_t* d_len = nullptr;        // [cap_tok]
    uint64_t* d_hash = nullptr;      // [cap_tok]
    int64_t* d_slot = nullptr;       // [cap_tok] the slot a token ended in
    int64_t cap_tok = 0;
    unsigned long long* d_table = nullptr;   // [cap_slots]
    int64_t cap_slots = 0;
    int64_t* d_sums = nullptr;       // [cap_sums] chunk sums of the scans
    int64_t cap_sums = 0;
    // what the calls so far established (rr_doctok_sizes commits a count)
    int32_t counted_docs = -1;       // documents / text bytes of the count call that waits for rr_doctok_sizes
    int64_t counted_bytes = -1;
    int32_t n_docs = -1;             // ... and of the last committed one
    int64_t text_bytes = 0, T = 0, n_terms = 0, vocab_bytes = 0, slots = 0;
    bool emitted = false, vocab_pending = false, vocab_done = false;
    std::mutex mu;
};

// ------------------------------------------------------------------------------------------------ the automaton
#define RR_DT_SEP 0
#define RR_DT_ALNUM 1
#define RR_DT_APOS 2
#define RR_DT_SKIP 3
#define RR_DT_IDENTITY 0xE4u

__device__ __forceinline__ uint32_t rr_dt_map_of(int cls) {        // the class's transition, 2 bits per state
    return cls == RR_DT_ALNUM ? 0xF5u : cls == RR_DT_APOS ? 0x08u : cls == RR_DT_SKIP ? RR_DT_IDENTITY : 0x00u;
}
__device__ __forceinline__ uint32_t rr_dt_apply_map(uint32_t map, uint32_t s) { return (map >> (2 * s)) & 3u; }
__device__ __forceinline__ uint32_t rr_dt_compose(uint32_t first, uint32_t then) {
    return rr_dt_apply_map(then, rr_dt_apply_map(first, 0)) | (rr_dt_apply_map(then, rr_dt_apply_map(first, 1)) << 2) |
           (rr_dt_apply_map(then, rr_dt_apply_map(first, 2)) << 4) | (rr_dt_apply_map(then, rr_dt_apply_map(first, 3)) << 6);
}
__device__ __forceinline__ bool rr_dt_ascii_alnum(uint32_t b) {
    return (b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z');
}

// The document's bytes around one tile: LDS for [base - HALO, base + TILE + HALO), global memory beyond; 0 outside the
// document (a separator, like NUL inside it).
struct rr_dt_view {
    const uint8_t* lds;      // lds[k] = document byte base - HALO + k
    const uint8_t* src;      // the document in global memory
    int64_t base, len;
    __device__ __forceinline__ uint32_t at(int64_t i) const {
        const int64_t k = i - base + RR_DT_HALO;
        if (k >= 0 && k < RR_DT_TILE + 2 * RR_DT_HALO) return lds[k];
        return (i >= 0 && i < len) ? src[i] : 0u;
    }
    __device__ __forceinline__ bool alnum_at(int64_t i) const {
        const uint32_t b = at(i);
        return rr_dt_ascii_alnum(b) || (b == 0xC4u && at(i + 1) == 0xB0u) || (b == 0xE2u && at(i + 1) == 0x84u && at(i + 2) == 0xAAu);
    }
};

template <bool EMIT>
__global__ __launch_bounds__(RR_DT_THREADS) void rr_dt_walk(
    const uint8_t* __restrict__ text, int64_t text_bytes, const int64_t* __restrict__ text_off,
    const uint64_t* __restrict__ stop, int32_t n_stop, int32_t* __restrict__ cnt, int64_t* __restrict__ ctl,
    const int64_t* __restrict__ doc_off, int64_t T, uint8_t* __restrict__ arena, int64_t* __restrict__ tok_pos,
    int32_t* __restrict__ tok_len, uint64_t* __restrict__ tok_hash) {
    __shared__ __attribute__((aligned(16))) uint8_t s_t[RR_DT_TILE + 2 * RR_DT_HALO];
    __shared__ uint64_t s_stop[RR_DT_MAX_STOP];
    __shared__ long long s_ws[RR_DT_THREADS / 64];
    __shared__ uint32_t s_maps[RR_DT_THREADS / 64];
    // EMIT: the kept tokens of a thread's slice, until the block scan has given them their indices
    __shared__ int s_len[EMIT ? RR_DT_PER / 2 : 1][RR_DT_THREADS];
    __shared__ uint64_t s_hash[EMIT ? RR_DT_PER / 2 : 1][RR_DT_THREADS];
    __shared__ uint8_t s_at[EMIT ? RR_DT_PER / 2 : 1][RR_DT_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int doc = blockIdx.x;
    int64_t b0, len;
    if (!rr_doc_span(text_off, doc, text_bytes, &b0, &len)) {   // offsets that leave the text: nothing is read
        if (!EMIT && tid == 0) { cnt[doc] = 0; atomicAdd((unsigned long long*)&ctl[RR_DT_C_BAD], 1ull); }
        return;
    }
    const uint8_t* src = text + b0;
    if (tid < RR_DT_MAX_STOP) s_stop[tid] = tid < n_stop ? stop[tid] : 0ull;
    const int64_t out0 = EMIT ? doc_off[doc] : 0;
    uint32_t state = 0;                                    // the automaton in front of the tile (the same in every thread)
    int64_t kept = 0;                                      // tokens kept before the tile
    int too_long = 0;
    for (int64_t base = 0; base < len && kept < RR_DT_CAP; base += RR_DT_TILE) {
        __syncthreads();                                   // the previous tile's readers are done
        const int64_t want = len - base + RR_DT_HALO;      // window bytes up to the document's end
        const int fill = want < RR_DT_TILE + 2 * RR_DT_HALO ? (int)want + RR_DT_HALO : RR_DT_TILE + 2 * RR_DT_HALO;
        for (int k = tid; k < fill && k < RR_DT_TILE + 2 * RR_DT_HALO; k += RR_DT_THREADS) {
            const int64_t i = base - RR_DT_HALO + k;
            s_t[k] = (i >= 0 && i < len) ? src[i] : (uint8_t)0;
        }
        __syncthreads();
        rr_dt_view v{s_t, src, base, len};
        const int k0 = RR_DT_HALO + tid * RR_DT_PER;       // this thread's slice in the window
        const int64_t i0 = base + (int64_t)tid * RR_DT_PER;
        uint32_t cls = 0;                                  // 2 bits per byte of the slice
        uint32_t map = RR_DT_IDENTITY;
        if (i0 < len) {
            const uint4 w4 = *(const uint4*)&s_t[k0];
            const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int j = 0; j < RR_DT_PER; ++j) {
                const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                const int k = k0 + j;
                int c = RR_DT_SEP;
                if (i0 + j < len) {
                    if (rr_dt_ascii_alnum(b)) c = RR_DT_ALNUM;
                    else if (b == '\'') c = RR_DT_APOS;
                    else if (b >= 0x80u) {                 // (bytes behind the document's end are 0 in the window)
                        if (b == 0xC4u) c = s_t[k + 1] == 0xB0u ? RR_DT_ALNUM : RR_DT_SEP;
                        else if (b == 0xE2u) c = (s_t[k + 1] == 0x84u && s_t[k + 2] == 0xAAu) ? RR_DT_ALNUM : RR_DT_SEP;
                        else if (b == 0x84u) c = (s_t[k - 1] == 0xE2u && s_t[k + 1] == 0xAAu) ? RR_DT_SKIP : RR_DT_SEP;
                        else if (b == 0xAAu) c = (s_t[k - 2] == 0xE2u && s_t[k - 1] == 0x84u) ? RR_DT_SKIP : RR_DT_SEP;
                    }
                }
                cls |= (uint32_t)c << (2 * j);
                map = rr_dt_compose(map, rr_dt_map_of(c));
            }
        } else {
            map = 0x00u;                                   // behind the end: separators
        }
        // the state in front of this thread's slice: a scan of composed maps
        uint32_t incl = map;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if (lane >= d) incl = rr_dt_compose(t, incl);
        }
        uint32_t excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = RR_DT_IDENTITY;
        if (lane == 63) s_maps[wave] = incl;
        __syncthreads();
        uint32_t s = state, tile_end = state;
#pragma unroll
        for (int wv = 0; wv < RR_DT_THREADS / 64; ++wv) {
            if (wv < wave) s = rr_dt_apply_map(s_maps[wv], s);
            tile_end = rr_dt_apply_map(s_maps[wv], tile_end);
        }
        s = rr_dt_apply_map(excl, s);
        state = tile_end;

        // the tokens that start in this slice (at most every other byte starts one)
        uint32_t starts = 0;
#pragma unroll
        for (int j = 0; j < RR_DT_PER; ++j) {
            const int c = (cls >> (2 * j)) & 3;
            if (c == RR_DT_ALNUM && s == 0) starts |= 1u << j;
            s = rr_dt_apply_map(rr_dt_map_of(c), s);
        }
        int mine = 0;                                      // kept tokens of this slice
        while (starts) {
            const int j = __ffs(starts) - 1;
            starts &= starts - 1;
            const int64_t i = i0 + j;
            int64_t p = i, n = 0;
            uint64_t key = 0, h = 0xCBF29CE484222325ull;
            bool second = false;
            for (;;) {
                const uint32_t b = v.at(p);
                uint32_t ch;
                int adv = 1;
                if ((b >= '0' && b <= '9') || (b >= 'a' && b <= 'z')) ch = b;
                else if (b >= 'A' && b <= 'Z') ch = b | 0x20u;
                else if (b == 0xC4u && v.at(p + 1) == 0xB0u) ch = 'i';                 // (B0 then ends the run)
                else if (b == 0xE2u && v.at(p + 1) == 0x84u && v.at(p + 2) == 0xAAu) { ch = 'k'; adv = 3; }
                else if (b == '\'' && !second && v.alnum_at(p + 1)) { ch = '\''; second = true; }
                else break;
                if (n < 8) key |= (uint64_t)ch << (8 * n);
                h = (h ^ ch) * 0x100000001B3ull;
                if (EMIT) arena[b0 + i + n] = (uint8_t)ch;     // n <= p - i: inside the token's own raw bytes
                ++n;
                p += adv;
            }
            bool keep = n > 1;
            if (keep && n <= 8)
                for (int q = 0; q < n_stop; ++q) keep = keep && s_stop[q] != key;
            if (n > 0x7FFFFFFFll) { too_long = 1; keep = false; }
            if (keep) {
                if (EMIT) {
                    s_len[mine][tid] = (int)n;
                    s_hash[mine][tid] = rr_mix64(h ^ (uint64_t)n);
                    s_at[mine][tid] = (uint8_t)j;
                }
                ++mine;
            }
        }
        long long total;
        const long long at = rr_block_scan<long long, RR_DT_THREADS>(mine, s_ws, &total);
        if (EMIT) {
            for (int m = 0; m < mine; ++m) {               // (a thread reads back only what it wrote itself)
                const int64_t idx = kept + at + m, o = out0 + idx;
                if (idx < RR_DT_CAP && o >= 0 && o < T) {
                    tok_pos[o] = b0 + i0 + s_at[m][tid];
                    tok_len[o] = s_len[m][tid];
                    tok_hash[o] = s_hash[m][tid];
                }
            }
        }
        kept += total;
    }
    if (!EMIT) {
        if (tid == 0) cnt[doc] = (int32_t)(kept < RR_DT_CAP ? kept : RR_DT_CAP);
        if (too_long) atomicAdd((unsigned long long*)&ctl[RR_DT_C_BAD], 1ull);
    }
}

// ------------------------------------------------------------------------------------------------ what the scans sum
struct rr_dt_f_cnt {                                       // kept tokens of a document
    const int32_t* cnt;
    __device__ __forceinline__ long long operator()(int64_t i) const { return cnt[i]; }
};
struct rr_dt_f_first {                                     // 1 where a term appears for the first time
    const int64_t* slot;
    const unsigned long long* table;
    __device__ __forceinline__ long long operator()(int64_t p) const {
        const int64_t s = slot[p];
        return (s >= 0 && table[s] == (unsigned long long)p) ? 1 : 0;
    }
};
struct rr_dt_f_first_len {                                 // ... and there, the term's bytes
    const int64_t* slot;
    const unsigned long long* table;
    const int32_t* len;
    __device__ __forceinline__ long long operator()(int64_t p) const {
        const int64_t s = slot[p];
        return (s >= 0 && table[s] == (unsigned long long)p) ? len[p] : 0;
    }
};
struct rr_dt_f_term_len {                                  // bytes of term id
    const int64_t* term_pos;
    const int32_t* len;
    __device__ __forceinline__ long long operator()(int64_t id) const { return len[term_pos[id]]; }
};

// ------------------------------------------------------------------------------------------------ the vocabulary
__global__ __launch_bounds__(256) void rr_dt_insert(const uint8_t* __restrict__ arena, const int64_t* __restrict__ tok_pos,
                                                    const int32_t* __restrict__ tok_len, const uint64_t* __restrict__ tok_hash,
                                                    int64_t T, int32_t hash_bits, int64_t slots, unsigned long long* table,
                                                    int64_t* __restrict__ slot_of, int64_t* __restrict__ ctl) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= T) return;
    const int len = tok_len[p];
    const uint8_t* mine = arena + tok_pos[p];
    uint64_t h = tok_hash[p];
    if (hash_bits < 64) h &= (1ull << hash_bits) - 1;       // tests: almost every probe collides
    int64_t slot = (int64_t)(h % (uint64_t)slots);
    int64_t found = -1;
    for (int64_t probes = 0; probes < slots; ++probes) {    // bounded: a full table is reported, not waited for
        // a plain look first: a slot's word only ever moves to a smaller position of the SAME term, so an old value still
        // names the term; only "empty" has to be confirmed by the compare-and-swap
        unsigned long long old = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == RR_DT_EMPTY) old = atomicCAS(&table[slot], RR_DT_EMPTY, (unsigned long long)p);
        if (old == RR_DT_EMPTY || old == (unsigned long long)p) { found = slot; break; }   // claimed: p is the term's first so far
        const int64_t q = (int64_t)old;                     // a token of the term that owns the slot (q < T: only positions are stored)
        bool same = tok_len[q] == len;
        if (same) {
            const uint8_t* other = arena + tok_pos[q];
            for (int k = 0; k < len; ++k)
                if (mine[k] != other[k]) { same = false; break; }
        }
        if (same) {
            if ((unsigned long long)p < old) atomicMin(&table[slot], (unsigned long long)p);   // (old >= the slot's word now)
            found = slot;
            break;
        }
        slot = slot + 1 == slots ? 0 : slot + 1;
    }
    slot_of[p] = found;
    if (found < 0) atomicAdd((unsigned long long*)&ctl[RR_DT_C_FULL], 1ull);
}

// tok[p] holds the exclusive count of first appearances in front of p: the id where p is one.  Every other token takes
// the id of its term's first (that entry is rewritten with its own value only: in place is safe).
__global__ __launch_bounds__(256) void rr_dt_assign(const int64_t* __restrict__ slot_of, const unsigned long long* __restrict__ table,
                                                    int64_t T, int32_t* tok) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= T) return;
    const int64_t s = slot_of[p];
    if (s < 0) { tok[p] = -1; return; }
    const int64_t q = (int64_t)table[s];
    if (q != p) tok[p] = tok[q];
}

__global__ __launch_bounds__(256) void rr_dt_term_pos(const int64_t* __restrict__ slot_of, const unsigned long long* __restrict__ table,
                                                      const int32_t* __restrict__ tok, int64_t T, int64_t n_terms,
                                                      int64_t* __restrict__ term_pos) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= T) return;
    const int64_t s = slot_of[p];
    if (s >= 0 && table[s] == (unsigned long long)p && tok[p] >= 0 && tok[p] < n_terms) term_pos[tok[p]] = p;
}

__global__ __launch_bounds__(256) void rr_dt_gather(const uint8_t* __restrict__ arena, const int64_t* __restrict__ tok_pos,
                                                    const int32_t* __restrict__ tok_len, const int64_t* __restrict__ term_pos,
                                                    const int64_t* __restrict__ voc_off, int64_t n_terms, int64_t vocab_bytes,
                                                    uint8_t* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n_terms) return;
    const int64_t p = term_pos[id], o = voc_off[id];
    const int len = tok_len[p];
    if (o < 0 || o + len > vocab_bytes) return;             // (the offsets are this library's own scan of the same lengths)
    const uint8_t* s = arena + tok_pos[p];
    for (int k = 0; k < len; ++k) out[o + k] = s[k];
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int rr_doctok_destroy(rr_doctok* dt) {
    if (!dt) return RR_OK;
    hipSetDevice(dt->device);
    hipFree(dt->d_stop); hipFree(dt->d_ctl); hipFree(dt->d_cnt); hipFree(dt->d_arena); hipFree(dt->d_pos); hipFree(dt->d_len);
    hipFree(dt->d_hash); hipFree(dt->d_slot); hipFree(dt->d_table); hipFree(dt->d_sums);
    delete dt;
    return RR_OK;
}

extern "C" int rr_doctok_create(int32_t device, const uint8_t* h_stop_bytes, const int64_t* h_stop_off, int32_t n_stop,
                                rr_doctok** out) {
    RR_REQUIRE(out, "rr_doctok_create: NULL out");
    *out = nullptr;
    RR_REQUIRE(n_stop >= 0 && n_stop <= RR_DT_MAX_STOP, "rr_doctok_create: %d stop words outside [0, %d]", n_stop, RR_DT_MAX_STOP);
    RR_REQUIRE(n_stop == 0 || (h_stop_bytes && h_stop_off), "rr_doctok_create: NULL stop words");
    uint64_t keys[RR_DT_MAX_STOP] = {};
    for (int s = 0; s < n_stop; ++s) {
        const int64_t a = h_stop_off[s], b = h_stop_off[s + 1];
        RR_REQUIRE(a >= 0 && b - a >= 1 && b - a <= 8, "rr_doctok_create: stop word %d has %lld bytes, outside [1, 8]", s, (long long)(b - a));
        for (int64_t k = a; k < b; ++k) {
            RR_REQUIRE(h_stop_bytes[k] != 0, "rr_doctok_create: NUL in stop word %d", s);
            keys[s] |= (uint64_t)h_stop_bytes[k] << (8 * (k - a));
        }
    }
    RR_HIP_TRY(hipSetDevice(device));
    rr_doctok* dt = new rr_doctok();
    dt->device = device;
    dt->n_stop = n_stop;
    hipError_t e = hipMalloc((void**)&dt->d_stop, sizeof(keys));
    if (e == hipSuccess) e = hipMemcpy(dt->d_stop, keys, sizeof(keys), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&dt->d_ctl, sizeof(int64_t) * RR_DT_C_WORDS);
    if (e == hipSuccess) e = hipMemset(dt->d_ctl, 0, sizeof(int64_t) * RR_DT_C_WORDS);
    if (e != hipSuccess) {
        rr_set_error("rr_doctok_create: %s", hipGetErrorString(e));
        rr_doctok_destroy(dt);
        return RR_E_HIP;
    }
    *out = dt;
    return RR_OK;
}

extern "C" int rr_doctok_limits(int32_t* out_tile, int32_t* out_per_thread, int32_t* out_token_cap) {
    RR_REQUIRE(out_tile && out_per_thread && out_token_cap, "rr_doctok_limits: NULL argument");
    *out_tile = RR_DT_TILE; *out_per_thread = RR_DT_PER; *out_token_cap = RR_DT_CAP;
    return RR_OK;
}

static int rr_dt_check_text(const char* who, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off, int32_t n_docs) {
    RR_REQUIRE(n_docs >= 0 && text_bytes >= 0, "%s: %d documents, %lld bytes", who, n_docs, (long long)text_bytes);
    RR_REQUIRE(d_text_off || n_docs == 0, "%s: NULL offsets", who);
    RR_REQUIRE(d_text || text_bytes == 0, "%s: NULL text with %lld bytes", who, (long long)text_bytes);
    return RR_OK;
}

extern "C" int rr_doctok_count_dev(rr_doctok* dt, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                   int32_t n_docs, int64_t* d_doc_off, void* stream) {
    RR_REQUIRE(dt && d_doc_off, "rr_doctok_count_dev: NULL argument");
    int rc = rr_dt_check_text("rr_doctok_count_dev", d_text, text_bytes, d_text_off, n_docs);
    if (rc != RR_OK) return rc;
    std::lock_guard<std::mutex> lk(dt->mu);
    RR_HIP_TRY(hipSetDevice(dt->device));
    hipStream_t st = (hipStream_t)stream;
    rc = rr_grow((void**)&dt->d_cnt, &dt->cap_docs, n_docs > 0 ? n_docs : 1, sizeof(int32_t), "rr_doctok_count_dev");
    if (rc == RR_OK) rc = rr_grow((void**)&dt->d_sums, &dt->cap_sums, rr_scan_sums_len(n_docs), sizeof(int64_t), "rr_doctok_count_dev");
    if (rc != RR_OK) return rc;
    if (n_docs > 0)
        hipLaunchKernelGGL(rr_dt_walk<false>, dim3((unsigned)n_docs), dim3(RR_DT_THREADS), 0, st, d_text, text_bytes, d_text_off,
                           dt->d_stop, dt->n_stop, dt->d_cnt, dt->d_ctl, (const int64_t*)nullptr, (int64_t)0, (uint8_t*)nullptr,
                           (int64_t*)nullptr, (int32_t*)nullptr, (uint64_t*)nullptr);
    rr_scan(rr_dt_f_cnt{dt->d_cnt}, (int64_t)n_docs, dt->d_sums, d_doc_off, (int32_t*)nullptr, dt->d_ctl + RR_DT_C_T, st);
    RR_HIP_TRY(hipGetLastError());
    dt->counted_docs = n_docs;
    dt->counted_bytes = text_bytes;
    return RR_OK;
}

extern "C" int rr_doctok_sizes(rr_doctok* dt, int64_t* out_sizes) {
    RR_REQUIRE(dt && out_sizes, "rr_doctok_sizes: NULL argument");
    std::lock_guard<std::mutex> lk(dt->mu);
    RR_HIP_TRY(hipSetDevice(dt->device));
    RR_HIP_TRY(hipDeviceSynchronize());
    int64_t ctl[RR_DT_C_WORDS];
    RR_HIP_TRY(hipMemcpy(ctl, dt->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    if (ctl[RR_DT_C_BAD] || ctl[RR_DT_C_FULL]) {
        const int64_t zero[3] = {0, 0, 0};
        RR_HIP_TRY(hipMemcpy(dt->d_ctl, zero, sizeof(zero), hipMemcpyHostToDevice));   // bad, T, full
    }
    if (ctl[RR_DT_C_BAD]) {                                  // the count is dropped; what an earlier call established stays
        dt->counted_docs = -1;
        out_sizes[0] = ctl[RR_DT_C_BAD];
        RR_REQUIRE(false, "rr_doctok_sizes: %lld document(s) had text offsets that decrease or leave the text, or a token of "
                   "2^31 bytes or more (no text was read for bad offsets; the count is dropped)", (long long)ctl[RR_DT_C_BAD]);
    }
    if (ctl[RR_DT_C_FULL]) {
        dt->vocab_pending = false;
        RR_REQUIRE(false, "rr_doctok_sizes: %lld token(s) found no slot in the vocabulary table", (long long)ctl[RR_DT_C_FULL]);
    }
    if (dt->counted_docs >= 0) {                             // commit the count: a new token stream, not yet emitted
        dt->n_docs = dt->counted_docs;
        dt->text_bytes = dt->counted_bytes;
        dt->T = ctl[RR_DT_C_T];
        dt->n_terms = dt->vocab_bytes = 0;
        dt->emitted = dt->vocab_pending = dt->vocab_done = false;
        dt->counted_docs = -1;
    }
    if (dt->vocab_pending) {
        RR_REQUIRE(ctl[RR_DT_C_TERMS] <= 0x7FFFFFFFll, "rr_doctok_sizes: %lld terms do not fit int32 ids", (long long)ctl[RR_DT_C_TERMS]);
        dt->n_terms = ctl[RR_DT_C_TERMS];
        dt->vocab_bytes = ctl[RR_DT_C_VBYTES];
        dt->vocab_pending = false;
        dt->vocab_done = true;
    }
    out_sizes[0] = dt->T;
    out_sizes[1] = dt->text_bytes;                           // the arena: token bytes sit at their text offsets
    out_sizes[2] = dt->n_terms;
    out_sizes[3] = dt->vocab_bytes;
    return RR_OK;
}

extern "C" int rr_doctok_emit_dev(rr_doctok* dt, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                  int32_t n_docs, const int64_t* d_doc_off, void* stream) {
    RR_REQUIRE(dt && d_doc_off, "rr_doctok_emit_dev: NULL argument");
    int rc = rr_dt_check_text("rr_doctok_emit_dev", d_text, text_bytes, d_text_off, n_docs);
    if (rc != RR_OK) return rc;
    std::lock_guard<std::mutex> lk(dt->mu);
    RR_REQUIRE(dt->counted_docs < 0 && dt->n_docs == n_docs && dt->text_bytes == text_bytes,
               "rr_doctok_emit_dev: call rr_doctok_count_dev and rr_doctok_sizes on the same text first");
    RR_HIP_TRY(hipSetDevice(dt->device));
    const int64_t T = dt->T;
    const int64_t t1 = T > 0 ? T : 1;
    rc = rr_grow((void**)&dt->d_arena, &dt->cap_arena, text_bytes > 0 ? text_bytes : 1, 1, "rr_doctok_emit_dev");
    if (rc == RR_OK && t1 > dt->cap_tok) {                    // the four token arrays grow together
        int64_t c0 = dt->cap_tok, c1 = dt->cap_tok, c2 = dt->cap_tok, c3 = dt->cap_tok;
        rc = rr_grow((void**)&dt->d_pos, &c0, t1, sizeof(int64_t), "rr_doctok_emit_dev");
        if (rc == RR_OK) rc = rr_grow((void**)&dt->d_len, &c1, t1, sizeof(int32_t), "rr_doctok_emit_dev");
        if (rc == RR_OK) rc = rr_grow((void**)&dt->d_hash, &c2, t1, sizeof(uint64_t), "rr_doctok_emit_dev");
        if (rc == RR_OK) rc = rr_grow((void**)&dt->d_slot, &c3, t1, sizeof(int64_t), "rr_doctok_emit_dev");
        dt->cap_tok = rc == RR_OK ? t1 : 0;
        if (rc != RR_OK) {                                    // all or nothing
            hipFree(dt->d_pos); hipFree(dt->d_len); hipFree(dt->d_hash); hipFree(dt->d_slot);
            dt->d_pos = nullptr; dt->d_len = nullptr; dt->d_hash = nullptr; dt->d_slot = nullptr;
        }
    }
    if (rc != RR_OK) return rc;
    dt->vocab_done = dt->vocab_pending = false;
    if (n_docs > 0 && T > 0)
        hipLaunchKernelGGL(rr_dt_walk<true>, dim3((unsigned)n_docs), dim3(RR_DT_THREADS), 0, (hipStream_t)stream, d_text, text_bytes,
                           d_text_off, dt->d_stop, dt->n_stop, (int32_t*)nullptr, dt->d_ctl, d_doc_off, T, dt->d_arena, dt->d_pos,
                           dt->d_len, dt->d_hash);
    RR_HIP_TRY(hipGetLastError());
    dt->emitted = true;
    return RR_OK;
}

extern "C" int rr_doctok_vocab_dev(rr_doctok* dt, int32_t hash_bits, int32_t* d_tok, void* stream) {
    RR_REQUIRE(dt, "rr_doctok_vocab_dev: NULL handle");
    RR_REQUIRE(hash_bits >= 1 && hash_bits <= 64, "rr_doctok_vocab_dev: hash_bits %d outside [1, 64]", hash_bits);
    std::lock_guard<std::mutex> lk(dt->mu);
    RR_REQUIRE(dt->emitted && dt->counted_docs < 0, "rr_doctok_vocab_dev: no emitted token stream on this handle");
    const int64_t T = dt->T;
    RR_REQUIRE(d_tok || T == 0, "rr_doctok_vocab_dev: NULL ids for %lld tokens", (long long)T);
    RR_REQUIRE(T <= (int64_t)0x7FFFFFFF * 256, "rr_doctok_vocab_dev: %lld tokens", (long long)T);
    RR_HIP_TRY(hipSetDevice(dt->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t slots = 2 * T > 64 ? 2 * T : 64;            // twice the tokens: it cannot fill
    int rc = rr_grow((void**)&dt->d_table, &dt->cap_slots, slots, sizeof(unsigned long long), "rr_doctok_vocab_dev");
    if (rc == RR_OK) rc = rr_grow((void**)&dt->d_sums, &dt->cap_sums, rr_scan_sums_len(T), sizeof(int64_t), "rr_doctok_vocab_dev");
    if (rc != RR_OK) return rc;
    dt->slots = slots;
    dt->vocab_done = false;
    if (T == 0) {
        RR_HIP_TRY(hipMemsetAsync(dt->d_ctl + RR_DT_C_TERMS, 0, 2 * sizeof(int64_t), st));
    } else {
        const unsigned grid = (unsigned)((T + 255) / 256);
        RR_HIP_TRY(hipMemsetAsync(dt->d_table, 0xFF, sizeof(unsigned long long) * (size_t)slots, st));
        hipLaunchKernelGGL(rr_dt_insert, dim3(grid), dim3(256), 0, st, dt->d_arena, dt->d_pos, dt->d_len, dt->d_hash, T, hash_bits,
                           slots, dt->d_table, dt->d_slot, dt->d_ctl);
        rr_scan(rr_dt_f_first_len{dt->d_slot, dt->d_table, dt->d_len}, T, dt->d_sums, (int64_t*)nullptr, (int32_t*)nullptr,
                   dt->d_ctl + RR_DT_C_VBYTES, st);
        rr_scan(rr_dt_f_first{dt->d_slot, dt->d_table}, T, dt->d_sums, (int64_t*)nullptr, d_tok, dt->d_ctl + RR_DT_C_TERMS, st);
        hipLaunchKernelGGL(rr_dt_assign, dim3(grid), dim3(256), 0, st, dt->d_slot, dt->d_table, T, d_tok);
    }
    RR_HIP_TRY(hipGetLastError());
    dt->vocab_pending = true;
    return RR_OK;
}

extern "C" int rr_doctok_copy_vocab(rr_doctok* dt, const int32_t* d_tok, uint8_t* h_bytes, int64_t* h_off) {
    RR_REQUIRE(dt && h_off, "rr_doctok_copy_vocab: NULL argument");
    std::lock_guard<std::mutex> lk(dt->mu);
    RR_REQUIRE(dt->vocab_done, "rr_doctok_copy_vocab: call rr_doctok_vocab_dev and rr_doctok_sizes first");
    const int64_t T = dt->T, n = dt->n_terms, vb = dt->vocab_bytes;
    if (n == 0) { h_off[0] = 0; return RR_OK; }
    RR_REQUIRE(d_tok && (h_bytes || vb == 0), "rr_doctok_copy_vocab: NULL argument");
    RR_HIP_TRY(hipSetDevice(dt->device));
    int64_t *d_term_pos = nullptr, *d_voc_off = nullptr;
    uint8_t* d_bytes = nullptr;
    hipError_t e = hipMalloc((void**)&d_term_pos, sizeof(int64_t) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void**)&d_voc_off, sizeof(int64_t) * (size_t)(n + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&d_bytes, (size_t)(vb > 0 ? vb : 1));
    int rc = RR_OK;
    if (e == hipSuccess) rc = rr_grow((void**)&dt->d_sums, &dt->cap_sums, rr_scan_sums_len(n), sizeof(int64_t), "rr_doctok_copy_vocab");
    if (e == hipSuccess && rc == RR_OK) {
        hipStream_t st = nullptr;
        hipLaunchKernelGGL(rr_dt_term_pos, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, dt->d_slot, dt->d_table, d_tok, T, n,
                           d_term_pos);
        rr_scan(rr_dt_f_term_len{d_term_pos, dt->d_len}, n, dt->d_sums, d_voc_off, (int32_t*)nullptr, (int64_t*)nullptr, st);
        hipLaunchKernelGGL(rr_dt_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dt->d_arena, dt->d_pos, dt->d_len,
                           d_term_pos, d_voc_off, n, vb, d_bytes);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(h_off, d_voc_off, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost);
        if (e == hipSuccess && vb > 0) e = hipMemcpy(h_bytes, d_bytes, (size_t)vb, hipMemcpyDeviceToHost);
    }
    hipFree(d_term_pos); hipFree(d_voc_off); hipFree(d_bytes);
    if (e != hipSuccess) {
        rr_set_error("rr_doctok_copy_vocab: %s", hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? RR_E_NOMEM : RR_E_HIP;
    }
    return rc;
}

extern "C" int rr_doctok_copy_tokens(rr_doctok* dt, int64_t* h_pos, int32_t* h_len, uint8_t* h_arena) {
    RR_REQUIRE(dt, "rr_doctok_copy_tokens: NULL handle");
    std::lock_guard<std::mutex> lk(dt->mu);
    RR_REQUIRE(dt->emitted, "rr_doctok_copy_tokens: no emitted token stream on this handle");
    RR_HIP_TRY(hipSetDevice(dt->device));
    RR_HIP_TRY(hipDeviceSynchronize());
    if (dt->T > 0) {
        RR_REQUIRE(h_pos && h_len, "rr_doctok_copy_tokens: NULL argument");
        RR_HIP_TRY(hipMemcpy(h_pos, dt->d_pos, sizeof(int64_t) * (size_t)dt->T, hipMemcpyDeviceToHost));
        RR_HIP_TRY(hipMemcpy(h_len, dt->d_len, sizeof(int32_t) * (size_t)dt->T, hipMemcpyDeviceToHost));
    }
    if (h_arena && dt->text_bytes > 0 && dt->T > 0)
        RR_HIP_TRY(hipMemcpy(h_arena, dt->d_arena, (size_t)dt->text_bytes, hipMemcpyDeviceToHost));
    return RR_OK;
}
