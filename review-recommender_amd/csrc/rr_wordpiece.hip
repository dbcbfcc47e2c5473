// rr_wordpiece.hip -- BERT WordPiece tokenisation of ASCII documents on the device (include/rr_hip.h: rr_wp_*).
//
// What `BertTokenizer` (BasicTokenizer + greedy longest-match WordPiece, lower-casing) does to a text whose bytes are all
// below 0x80, where every Unicode rule reduces to a byte rule (review-recommender_amd/wordpiece.py is the host form):
//   deleted   0x00-0x08 0x0B 0x0C 0x0E-0x1F 0x7F      (control characters: the neighbours join into one word)
//   blank     space \t \n \r                          (separates words)
//   punct     33-47 58-64 91-96 123-126               (a word of its own)
//   the rest  A-Z lower-cased, runs form words
// A document with a byte >= 0x80 is NOT tokenised here (NFC / NFD, Mn stripping, CJK isolation, Unicode categories stay on the
// host): it gets needs_host = 1 and the placeholder [CLS] [SEP].
//
// rr_wp_tokenize   one workgroup per document.  The first RR_WP_WINDOW bytes are classified, lower-cased and compacted
//                  (deleted bytes dropped) into LDS with a workgroup scan; every word start is then taken by one thread,
//                  which writes the word's rolling prefix hashes into LDS (hash of any substring = two reads and a
//                  multiply) and matches greedily, longest candidate first, against an open-addressing table of the
//                  pieces in global memory (1 MB for 30 522 pieces: L2-resident).  A probe that finds the hash ALWAYS compares length, form
//                  (## or not) and bytes.  Piece ids are left at the compacted position where the piece starts; a second
//                  workgroup scan ranks them and the first max_length - 2 go to the document's row of a scratch
//                  [n_docs][max_length].  A document longer than the window is answered from the window when the words
//                  that END inside it already give max_length - 2 pieces (nothing behind can change them); otherwise
//                  needs_host = 1.
// rr_wp_scan       cu_seqlens = running sum of the lengths, and the longest one (one workgroup, chunks of 1024).
// rr_wp_pack       scratch rows -> packed token / type / position ids.
#include <vector>

#include "rr_common.h"

#define RR_WP_THREADS 256
#define RR_WP_PER 16                                   // bytes per thread of the window
#define RR_WP_WINDOW (RR_WP_THREADS * RR_WP_PER)       // 4096: every document of up to 4 000 bytes fits
#define RR_WP_MAX_WORD 255                             // upper limit of max_chars_per_word (powers of the hash base in LDS)
#define RR_WP_BASE 0x01000193u                         // odd: the polynomial hash is taken mod 2^32

struct rr_wp_entry {     // one slot of the table; id < 0 = empty
    uint32_t hash;       // polynomial hash of the piece's bytes (without ##)
    int32_t off;         // first byte in d_bytes
    int32_t len_form;    // length | continuation form (##) << 16
    int32_t id;
};

struct rr_wp {
    int device = 0;
    int32_t unk = 0, cls = 0, sep = 0, max_chars = 100;
    int32_t n_slots = 0;             // power of two, at least twice the pieces kept
    int32_t n_kept = 0;
    rr_wp_entry* d_table = nullptr;
    uint8_t* d_bytes = nullptr;
    int32_t* d_rows = nullptr;       // scratch [cap_docs][cap_len] token ids per document, then [cap_docs] lengths
    int64_t cap_words = 0;
    int32_t* d_bad = nullptr;        // documents whose offsets were refused by the kernel (rr_wp_status)
    std::mutex mu;
};

__host__ __device__ static inline uint32_t rr_wp_slot_of(uint32_t hash, int32_t len_form) {
    uint32_t h = hash ^ ((uint32_t)len_form * 0x9E3779B1u);
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;     // murmur3's finaliser
    return h;
}

// The table on the host: every piece that can match ASCII text (no byte >= 0x80, 1 .. max_chars characters after the ##).
// out_slots (may be NULL): 4 int32 per slot = rr_wp_entry.  Returns the pieces kept, or -1 when n_slots is too small.
static int64_t rr_wp_fill_table(const uint8_t* bytes, const int64_t* off, int32_t n_pieces, int32_t max_chars, int32_t n_slots,
                                rr_wp_entry* slots) {
    for (int32_t s = 0; s < n_slots; ++s) slots[s] = rr_wp_entry{0u, 0, 0, -1};
    int64_t kept = 0;
    for (int32_t p = 0; p < n_pieces; ++p) {
        int64_t a = off[p], b = off[p + 1];
        const int form = (b - a > 2 && bytes[a] == '#' && bytes[a + 1] == '#') ? 1 : 0;
        if (form) a += 2;
        if (b - a < 1 || b - a > max_chars) continue;
        bool ascii = true;
        uint32_t h = 0;
        for (int64_t i = a; i < b; ++i) {
            ascii = ascii && bytes[i] < 0x80;
            h = h * RR_WP_BASE + bytes[i];
        }
        if (!ascii) continue;
        if (2 * (kept + 1) > n_slots) return -1;
        const int32_t lf = (int32_t)(b - a) | (form << 16);
        uint32_t s = rr_wp_slot_of(h, lf) & (uint32_t)(n_slots - 1);
        bool dup = false;
        while (slots[s].id >= 0) {         // a piece listed twice keeps its LAST id (what a dict built from vocab.txt holds)
            if (slots[s].hash == h && slots[s].len_form == lf && memcmp(bytes + slots[s].off, bytes + a, (size_t)(b - a)) == 0) {
                dup = true;
                break;
            }
            s = (s + 1) & (uint32_t)(n_slots - 1);
        }
        slots[s] = rr_wp_entry{h, (int32_t)a, lf, p};
        if (!dup) ++kept;
    }
    return kept;
}

static int rr_wp_check_pieces(const char* who, const uint8_t* h_piece_bytes, const int64_t* h_piece_off, int32_t n_pieces,
                              int32_t max_chars_per_word) {
    RR_REQUIRE(h_piece_bytes && h_piece_off, "%s: NULL argument", who);
    RR_REQUIRE(n_pieces >= 1 && n_pieces <= (1 << 24), "%s: %d pieces outside [1, 2^24]", who, n_pieces);
    RR_REQUIRE(max_chars_per_word >= 1 && max_chars_per_word <= RR_WP_MAX_WORD, "%s: max_chars_per_word %d outside [1, %d]", who,
               max_chars_per_word, RR_WP_MAX_WORD);
    RR_REQUIRE(h_piece_off[0] == 0, "%s: piece offsets must start at 0", who);
    for (int32_t p = 0; p < n_pieces; ++p)
        RR_REQUIRE(h_piece_off[p + 1] >= h_piece_off[p], "%s: piece offsets decrease at piece %d", who, p);
    RR_REQUIRE(h_piece_off[n_pieces] < (1ll << 31), "%s: %lld piece bytes (limit 2^31)", who, (long long)h_piece_off[n_pieces]);
    return RR_OK;
}

static int32_t rr_wp_slots_for(int32_t n_pieces) {
    int32_t n = 64;
    while (n < 2 * (int64_t)n_pieces) n <<= 1;
    return n;
}

extern "C" int rr_wp_table_slots(int32_t n_pieces, int32_t* out_slots) {
    RR_REQUIRE(out_slots && n_pieces >= 1 && n_pieces <= (1 << 24), "rr_wp_table_slots: %d pieces outside [1, 2^24]", n_pieces);
    *out_slots = rr_wp_slots_for(n_pieces);
    return RR_OK;
}

extern "C" int rr_wp_build_table(const uint8_t* h_piece_bytes, const int64_t* h_piece_off, int32_t n_pieces,
                                 int32_t max_chars_per_word, int32_t n_slots, int32_t* h_slots, int32_t* out_kept) {
    int rc = rr_wp_check_pieces("rr_wp_build_table", h_piece_bytes, h_piece_off, n_pieces, max_chars_per_word);
    if (rc) return rc;
    RR_REQUIRE(h_slots && out_kept, "rr_wp_build_table: NULL output");
    RR_REQUIRE(n_slots == rr_wp_slots_for(n_pieces), "rr_wp_build_table: n_slots %d, rr_wp_table_slots says %d", n_slots,
               rr_wp_slots_for(n_pieces));
    const int64_t kept = rr_wp_fill_table(h_piece_bytes, h_piece_off, n_pieces, max_chars_per_word, n_slots,
                                          reinterpret_cast<rr_wp_entry*>(h_slots));
    RR_REQUIRE(kept >= 0, "rr_wp_build_table: table overflow");
    *out_kept = (int32_t)kept;
    return RR_OK;
}

extern "C" int rr_wp_destroy(rr_wp* wp) {
    if (!wp) return RR_OK;
    hipSetDevice(wp->device);
    hipDeviceSynchronize();
    hipFree(wp->d_table); hipFree(wp->d_bytes); hipFree(wp->d_rows); hipFree(wp->d_bad);
    delete wp;
    return RR_OK;
}

extern "C" int rr_wp_create(int32_t device, const uint8_t* h_piece_bytes, const int64_t* h_piece_off, int32_t n_pieces,
                            int32_t unk_id, int32_t cls_id, int32_t sep_id, int32_t max_chars_per_word, rr_wp** out) {
    RR_REQUIRE(out, "rr_wp_create: NULL out");
    *out = nullptr;
    int rc = rr_wp_check_pieces("rr_wp_create", h_piece_bytes, h_piece_off, n_pieces, max_chars_per_word);
    if (rc) return rc;
    RR_REQUIRE(unk_id >= 0 && unk_id < n_pieces && cls_id >= 0 && cls_id < n_pieces && sep_id >= 0 && sep_id < n_pieces,
               "rr_wp_create: special ids (%d, %d, %d) outside [0, %d)", unk_id, cls_id, sep_id, n_pieces);
    int ndev = 0;
    RR_HIP_TRY(hipGetDeviceCount(&ndev));
    RR_REQUIRE(device >= 0 && device < ndev, "rr_wp_create: device %d not in [0,%d)", device, ndev);
    RR_HIP_TRY(hipSetDevice(device));
    const int32_t n_slots = rr_wp_slots_for(n_pieces);
    std::vector<rr_wp_entry> slots((size_t)n_slots);
    const int64_t kept = rr_wp_fill_table(h_piece_bytes, h_piece_off, n_pieces, max_chars_per_word, n_slots, slots.data());
    RR_REQUIRE(kept >= 0, "rr_wp_create: table overflow");
    rr_wp* wp = new rr_wp();
    wp->device = device;
    wp->unk = unk_id; wp->cls = cls_id; wp->sep = sep_id; wp->max_chars = max_chars_per_word;
    wp->n_slots = n_slots;
    wp->n_kept = (int32_t)kept;
    const size_t nbytes = (size_t)h_piece_off[n_pieces];
    hipError_t e = hipMalloc((void**)&wp->d_table, sizeof(rr_wp_entry) * (size_t)n_slots);
    if (e == hipSuccess) e = hipMalloc((void**)&wp->d_bytes, nbytes + 16);
    if (e == hipSuccess) e = hipMalloc((void**)&wp->d_bad, 4);
    if (e == hipSuccess) e = hipMemset(wp->d_bad, 0, 4);
    if (e == hipSuccess) e = hipMemcpy(wp->d_table, slots.data(), sizeof(rr_wp_entry) * (size_t)n_slots, hipMemcpyHostToDevice);
    if (e == hipSuccess && nbytes) e = hipMemcpy(wp->d_bytes, h_piece_bytes, nbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        rr_set_error("rr_wp_create: %s", hipGetErrorString(e));
        rr_wp_destroy(wp);
        return RR_E_HIP;
    }
    *out = wp;
    return RR_OK;
}

// ------------------------------------------------------------------ device side
// 0 deleted, 1 blank, 2 punctuation, 3 word character
__device__ __forceinline__ int rr_wp_class(unsigned c) {
    if (c == 0x20u || c == 0x09u || c == 0x0Au || c == 0x0Du) return 1;
    if (c < 0x20u || c == 0x7Fu) return 0;
    if ((c >= 33u && c <= 47u) || (c >= 58u && c <= 64u) || (c >= 91u && c <= 96u) || (c >= 123u && c <= 126u)) return 2;
    return 3;
}

// Exclusive sum of one int per thread over the workgroup (RR_WP_THREADS = 4 waves); *total = the sum, in every thread.
__device__ __forceinline__ int rr_wp_block_scan(int v, int* wave_sums, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    __syncthreads();                       // (wave_sums may still be read from the previous scan)
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RR_WP_THREADS / 64; ++w) {
        const int s = wave_sums[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return before + incl - v;
}

__device__ __forceinline__ int rr_wp_lookup(const rr_wp_entry* __restrict__ table, uint32_t mask, const uint8_t* __restrict__ bytes,
                                            uint32_t hash, int len, int form, const uint8_t* word /* LDS */) {
    const int32_t lf = len | (form << 16);
    uint32_t s = rr_wp_slot_of(hash, lf) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes) {
        const int4 raw = *reinterpret_cast<const int4*>(table + s);
        if (raw.w < 0) return -1;
        if ((uint32_t)raw.x == hash && raw.z == lf) {
            const uint8_t* p = bytes + raw.y;
            int k = 0;
            while (k < len && p[k] == word[k]) ++k;
            if (k == len) return raw.w;
        }
        s = (s + 1) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(RR_WP_THREADS) void rr_wp_tokenize(
    const uint8_t* __restrict__ text, int64_t text_bytes, const int64_t* __restrict__ text_off, int32_t n_docs, int32_t max_length,
    const rr_wp_entry* __restrict__ table, uint32_t mask, const uint8_t* __restrict__ bytes, int32_t unk, int32_t cls, int32_t sep,
    int32_t max_chars, int32_t* __restrict__ rows /* [n_docs][max_length] */, int32_t* __restrict__ lens /* [n_docs] */,
    int32_t* __restrict__ needs_host, int32_t* __restrict__ bad) {
    __shared__ uint8_t s_ch[RR_WP_WINDOW];          // compacted, lower-cased characters
    __shared__ uint8_t s_cl[RR_WP_WINDOW];          // their classes
    __shared__ uint8_t s_pf[RR_WP_WINDOW];          // 1 = a piece starts here
    __shared__ uint32_t s_ph[RR_WP_WINDOW + 1];     // prefix hashes, per word
    __shared__ int32_t s_id[RR_WP_WINDOW];          // the piece that starts here
    __shared__ uint32_t s_pw[RR_WP_MAX_WORD + 1];   // powers of the base
    __shared__ int s_ws[RR_WP_THREADS / 64];
    const int tid = threadIdx.x;
    const int doc = blockIdx.x;
    int32_t* row = rows + (int64_t)doc * max_length;
    const int64_t b0 = text_off[doc], b1 = text_off[doc + 1];
    if (b0 < 0 || b1 < b0 || b1 > text_bytes) {            // offsets that leave the text: nothing is read (rr_wp_status reports it)
        if (tid == 0) {
            row[0] = cls; row[1] = sep; lens[doc] = 2; needs_host[doc] = 1;
            atomicAdd(bad, 1);
        }
        return;
    }
    const int64_t len = b1 - b0;
    const uint8_t* src = text + b0;
    if (tid <= max_chars) {
        uint32_t p = 1;
        for (int k = 0; k < tid; ++k) p *= RR_WP_BASE;
        s_pw[tid] = p;
    }
    int high = 0;
    for (int64_t i = tid; i < len; i += RR_WP_THREADS) high |= src[i] & 0x80;
    if (__syncthreads_or(high)) {
        if (tid == 0) { row[0] = cls; row[1] = sep; lens[doc] = 2; needs_host[doc] = 1; }
        return;
    }
    const bool cut = len > RR_WP_WINDOW;
    const int wlen = cut ? RR_WP_WINDOW : (int)len;

    // classify, lower-case, compact
    unsigned ch[RR_WP_PER];
    int keep = 0;
#pragma unroll
    for (int j = 0; j < RR_WP_PER; ++j) {
        const int i = tid * RR_WP_PER + j;
        const unsigned c = i < wlen ? src[i] : 0u;
        ch[j] = c;
        keep += (i < wlen && rr_wp_class(c) != 0) ? 1 : 0;
    }
    int n = 0;
    int at = rr_wp_block_scan(keep, s_ws, &n);
#pragma unroll
    for (int j = 0; j < RR_WP_PER; ++j) {
        const int i = tid * RR_WP_PER + j;
        const int k = rr_wp_class(ch[j]);
        if (i < wlen && k != 0) {
            s_ch[at] = (uint8_t)((ch[j] >= 'A' && ch[j] <= 'Z') ? ch[j] + 32u : ch[j]);
            s_cl[at] = (uint8_t)k;
            s_pf[at] = 0;
            ++at;
        }
    }
    __syncthreads();

    // one thread per word
    for (int i = tid; i < n; i += RR_WP_THREADS) {
        const int k = s_cl[i];
        if (k == 2) {
            const int id = rr_wp_lookup(table, mask, bytes, (uint32_t)s_ch[i], 1, 0, s_ch + i);
            s_id[i] = id < 0 ? unk : id;
            s_pf[i] = 1;
        } else if (k == 3 && (i == 0 || s_cl[i - 1] != 3)) {
            int e = i + 1;
            while (e < n && s_cl[e] == 3) ++e;
            if (cut && e == n) continue;                 // the window may have cut this word: it does not count
            if (e - i > max_chars) {
                s_id[i] = unk;
                s_pf[i] = 1;
                continue;
            }
            uint32_t h = 0;
            s_ph[i] = 0;
            for (int p = i; p < e; ++p) {
                h = h * RR_WP_BASE + s_ch[p];
                s_ph[p + 1] = h;
            }
            int start = i;
            bool whole = true;
            while (start < e) {
                int end = e, id = -1;
                for (; end > start; --end) {
                    const uint32_t hh = s_ph[end] - s_ph[start] * s_pw[end - start];
                    id = rr_wp_lookup(table, mask, bytes, hh, end - start, start > i ? 1 : 0, s_ch + start);
                    if (id >= 0) break;
                }
                if (id < 0) { whole = false; break; }
                s_id[start] = id;
                s_pf[start] = 1;
                start = end;
            }
            if (!whole) {                                // any unmatched remainder: the whole word is one [UNK]
                for (int p = i + 1; p < e; ++p) s_pf[p] = 0;
                s_id[i] = unk;
                s_pf[i] = 1;
            }
        }
    }
    __syncthreads();

    // rank the pieces, keep the first max_length - 2
    int mine = 0;
#pragma unroll
    for (int j = 0; j < RR_WP_PER; ++j) {
        const int i = tid * RR_WP_PER + j;
        mine += (i < n && s_pf[i]) ? 1 : 0;
    }
    int total = 0;
    int rank = rr_wp_block_scan(mine, s_ws, &total);
    const int room = max_length - 2;
    if (cut && total < room) {                           // the window was not enough to fill the sequence
        if (tid == 0) { row[0] = cls; row[1] = sep; lens[doc] = 2; needs_host[doc] = 1; }
        return;
    }
#pragma unroll
    for (int j = 0; j < RR_WP_PER; ++j) {
        const int i = tid * RR_WP_PER + j;
        if (i < n && s_pf[i]) {
            if (rank < room) row[1 + rank] = s_id[i];
            ++rank;
        }
    }
    if (tid == 0) {
        const int kept = total < room ? total : room;
        row[0] = cls;
        row[1 + kept] = sep;
        lens[doc] = kept + 2;
        needs_host[doc] = 0;
    }
}

__global__ __launch_bounds__(1024) void rr_wp_scan(const int32_t* __restrict__ lens, int32_t n_docs, int32_t* __restrict__ cu,
                                                   int32_t* __restrict__ max_len) {
    __shared__ int s_w[16];
    __shared__ int s_m[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0, longest = 0;
    if (tid == 0) cu[0] = 0;
    for (int base = 0; base < n_docs; base += 1024) {
        const int i = base + tid;
        const int v = i < n_docs ? lens[i] : 0;
        longest = v > longest ? v : longest;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        __syncthreads();
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? s_w[w] : 0;
            all += s_w[w];
        }
        if (i < n_docs) cu[i + 1] = carry + before + incl;
        carry += all;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int t = __shfl_xor(longest, m, 64);
        longest = t > longest ? t : longest;
    }
    __syncthreads();
    if (lane == 0) s_m[wave] = longest;
    __syncthreads();
    if (tid == 0) {
        int m = 0;
        for (int w = 0; w < 16; ++w) m = s_m[w] > m ? s_m[w] : m;
        *max_len = m;
    }
}

__global__ __launch_bounds__(256) void rr_wp_pack(const int32_t* __restrict__ rows, const int32_t* __restrict__ lens,
                                                  const int32_t* __restrict__ cu, int32_t max_length, int64_t capacity,
                                                  int32_t* __restrict__ tok, int32_t* __restrict__ typ, int32_t* __restrict__ pos) {
    const int doc = blockIdx.x;
    const int n = lens[doc];
    const int64_t at = cu[doc];
    const int32_t* row = rows + (int64_t)doc * max_length;
    for (int j = threadIdx.x; j < n; j += 256) {
        const int64_t o = at + j;
        if (o < capacity) {            // token_capacity bounds the writes; cu_seqlens[n_docs] tells what was needed
            tok[o] = row[j];
            typ[o] = 0;
            pos[o] = j;
        }
    }
}

extern "C" int rr_wp_encode_dev(rr_wp* wp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off, int32_t n_docs,
                                int32_t max_length, int64_t token_capacity, int32_t* d_token_ids, int32_t* d_type_ids,
                                int32_t* d_pos_ids, int32_t* d_cu_seqlens, int32_t* d_needs_host, int32_t* d_max_len, void* stream) {
    RR_REQUIRE(wp && d_text_off && d_token_ids && d_type_ids && d_pos_ids && d_cu_seqlens && d_needs_host && d_max_len,
               "rr_wp_encode_dev: NULL argument");
    RR_REQUIRE(d_text || text_bytes == 0, "rr_wp_encode_dev: NULL text with %lld bytes", (long long)text_bytes);
    RR_REQUIRE(n_docs >= 1 && n_docs <= (1 << 24), "rr_wp_encode_dev: %d documents outside [1, 2^24]", n_docs);
    RR_REQUIRE(max_length >= 2 && max_length <= 65536, "rr_wp_encode_dev: max_length %d outside [2, 65536] ([CLS] and [SEP] need two)",
               max_length);
    RR_REQUIRE(text_bytes >= 0 && text_bytes < (1ll << 31), "rr_wp_encode_dev: %lld text bytes in one call (limit 2^31)",
               (long long)text_bytes);
    RR_REQUIRE(token_capacity >= 2 * (int64_t)n_docs, "rr_wp_encode_dev: token_capacity %lld cannot hold [CLS] [SEP] of %d documents",
               (long long)token_capacity, n_docs);
    RR_REQUIRE((int64_t)n_docs * max_length < (1ll << 31), "rr_wp_encode_dev: %d documents x max_length %d reach 2^31 tokens", n_docs,
               max_length);
    std::lock_guard<std::mutex> lk(wp->mu);
    RR_HIP_TRY(hipSetDevice(wp->device));
    const int64_t words = (int64_t)n_docs * max_length + n_docs;
    if (words > wp->cap_words) {          // grown on the first call of a size (hipFree waits for the kernels that use the old one)
        if (wp->d_rows) RR_HIP_TRY(hipFree(wp->d_rows));
        wp->d_rows = nullptr;
        wp->cap_words = 0;
        if (hipMalloc((void**)&wp->d_rows, sizeof(int32_t) * (size_t)words) != hipSuccess) {
            (void)hipGetLastError();
            rr_set_error("rr_wp_encode_dev: no memory for %lld scratch words", (long long)words);
            return RR_E_NOMEM;
        }
        wp->cap_words = words;
    }
    int32_t* d_lens = wp->d_rows + (int64_t)n_docs * max_length;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rr_wp_tokenize, dim3((unsigned)n_docs), dim3(RR_WP_THREADS), 0, st, d_text, text_bytes, d_text_off, n_docs,
                       max_length, wp->d_table, (uint32_t)(wp->n_slots - 1), wp->d_bytes, wp->unk, wp->cls, wp->sep, wp->max_chars,
                       wp->d_rows, d_lens, d_needs_host, wp->d_bad);
    hipLaunchKernelGGL(rr_wp_scan, dim3(1), dim3(1024), 0, st, d_lens, n_docs, d_cu_seqlens, d_max_len);
    hipLaunchKernelGGL(rr_wp_pack, dim3((unsigned)n_docs), dim3(256), 0, st, wp->d_rows, d_lens, d_cu_seqlens, max_length,
                       token_capacity, d_token_ids, d_type_ids, d_pos_ids);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_wp_status(rr_wp* wp, int32_t* out_bad_docs) {
    RR_REQUIRE(wp && out_bad_docs, "rr_wp_status: NULL argument");
    std::lock_guard<std::mutex> lk(wp->mu);
    RR_HIP_TRY(hipSetDevice(wp->device));
    RR_HIP_TRY(hipDeviceSynchronize());
    int32_t bad = 0;
    RR_HIP_TRY(hipMemcpy(&bad, wp->d_bad, 4, hipMemcpyDeviceToHost));
    RR_HIP_TRY(hipMemset(wp->d_bad, 0, 4));
    *out_bad_docs = bad;
    RR_REQUIRE(bad == 0, "rr_wp_status: %d document(s) had text offsets that decrease or leave the text (they were answered "
               "[CLS] [SEP] with needs_host = 1)", bad);
    return RR_OK;
}
