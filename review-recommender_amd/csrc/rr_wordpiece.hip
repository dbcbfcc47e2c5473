// rr_wordpiece.hip -- BERT WordPiece tokenisation of UTF-8 text on the device (include/rr_hip.h: rr_wp_*).
//
// What `BertTokenizer` (BasicTokenizer + greedy longest-match WordPiece, lower-casing) does to a text
// (review-recommender_amd/wordpiece.py is the host form, wp_unicode.model_tokenize the model of the kernel's flags).
//
// rr_wp_tokenize_utf8   one workgroup per document.  The raw window (at most RR_WP_WINDOW bytes, ending on a character
//                  boundary) is staged in LDS, then decoded, validated and mapped per character (rr_wpu_char_at):
//                    b < 0x80   every Unicode rule reduces to a byte rule --
//                                 deleted   0x00-0x08 0x0B 0x0C 0x0E-0x1F 0x7F   (control characters: the neighbours join)
//                                 blank     space \t \n \r                       (separates words)
//                                 punct     33-47 58-64 91-96 123-126            (a word of its own)
//                                 the rest  A-Z lower-cased, runs form words;
//                    the rest   the Unicode table (wp_unicode.py) gives the code point its class and its mapped form
//                               (lower-cased, NFD, Mn stripped: 0 .. 3 code points), which is re-encoded as UTF-8.
//                  A workgroup scan over the mapped byte counts compacts the mapped text into LDS.  Each LDS byte carries
//                  the kind of its character (1 blank, 2 a word of its own: punctuation and CJK, 3 word character) and
//                  RR_WPU_FIRST on the first byte of a character.  Every word start is then taken by one thread, which
//                  writes the word's rolling prefix hashes into LDS (hash of any substring = two reads and a multiply)
//                  and matches greedily, longest candidate first (candidates end on character boundaries, the word length
//                  is counted in characters, a kind-2 word is one character of 1 .. 4 bytes), against the table of the
//                  pieces in global memory (rr_prims.h: the vocabulary table; 1 MB for 30 522 pieces: L2-resident).  A
//                  probe that finds the hash ALWAYS compares length, form (## or not) and bytes.  Piece ids are left at
//                  the compacted position where the piece starts; a second workgroup scan ranks them and the first
//                  max_length - 2 go to the document's row of a scratch [n_docs][max_length].  A document longer than
//                  the window is answered from the window when the words that END inside it already give max_length - 2
//                  pieces (nothing behind can change them).
//                  needs_host = 1 (placeholder [CLS] [SEP]) only when, in the bytes read: the UTF-8 is malformed; a hard
//                  code point occurs (its mapping depends on its neighbours); the mapped text is longer than
//                  RR_WP_WINDOW bytes (the LDS bound); or the window did not give max_length - 2 pieces.
// rr_wp_scan       cu_seqlens = running sum of the lengths, and the longest one (one workgroup, chunks of 1024).
// rr_wp_pack       scratch rows -> packed token / type / position ids.
#include <vector>

#include "rr_prims.h"

#define RR_WP_THREADS 256
#define RR_WP_PER 16                                   // bytes per thread of the window
#define RR_WP_WINDOW (RR_WP_THREADS * RR_WP_PER)       // 4096: every document of up to 4 000 bytes fits
#define RR_WP_MAX_WORD 255                             // upper limit of max_chars_per_word (powers of the hash base in LDS)

struct rr_wp {
    int device = 0;
    int32_t unk = 0, cls = 0, sep = 0, max_chars = 100;
    int32_t n_slots = 0;             // power of two, at least twice the pieces kept
    int32_t n_kept = 0;
    rr_tab_entry* d_table = nullptr; // the pieces (rr_prims.h): hash of the bytes without ##, key = length | ## form << 16
    uint8_t* d_bytes = nullptr;
    int32_t* d_rows = nullptr;       // scratch [cap_docs][cap_len] token ids per document, then [cap_docs] lengths
    int64_t cap_words = 0;
    int32_t* d_bad = nullptr;        // documents whose offsets were refused by the kernel (rr_wp_status)
    uint16_t* d_st1 = nullptr;       // the Unicode table: block -> block of d_st2
    uint32_t* d_st2 = nullptr;       //   one entry per code point (RR_WPU_* below)
    uint32_t* d_pool = nullptr;      //   mapped code points of the entries that are not identities
    std::mutex mu;
};

// The table on the host: every piece that can match mapped text, 1 .. max_chars CHARACTERS (the bytes that are not
// 10xxxxxx) after the ##.  Returns the pieces kept, or -1 when n_slots is too small.
static int64_t rr_wp_fill_table(const uint8_t* bytes, const int64_t* off, int32_t n_pieces, int32_t max_chars, int32_t n_slots,
                                rr_tab_entry* slots) {
    return rr_tab_fill(bytes, off, n_pieces, n_slots, slots, [=](int64_t a, int64_t b, int64_t* first, int32_t* key) {
        const int form = (b - a > 2 && bytes[a] == '#' && bytes[a + 1] == '#') ? 1 : 0;
        if (form) a += 2;
        if (b - a < 1 || b - a > 4 * (int64_t)max_chars) return false;
        int64_t chars = 0;
        for (int64_t i = a; i < b; ++i) chars += (bytes[i] & 0xC0) != 0x80;
        if (chars > max_chars) return false;
        *first = a;
        *key = (int32_t)(b - a) | (form << 16);
        return true;
    });
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

extern "C" int rr_wp_table_slots(int32_t n_pieces, int32_t* out_slots) {
    RR_REQUIRE(out_slots && n_pieces >= 1 && n_pieces <= (1 << 24), "rr_wp_table_slots: %d pieces outside [1, 2^24]", n_pieces);
    *out_slots = rr_tab_slots_for(n_pieces);
    return RR_OK;
}

extern "C" int rr_wp_build_table_utf8(const uint8_t* h_piece_bytes, const int64_t* h_piece_off, int32_t n_pieces,
                                      int32_t max_chars_per_word, int32_t n_slots, int32_t* h_slots, int32_t* out_kept) {
    int rc = rr_wp_check_pieces("rr_wp_build_table_utf8", h_piece_bytes, h_piece_off, n_pieces, max_chars_per_word);
    if (rc) return rc;
    RR_REQUIRE(h_slots && out_kept, "rr_wp_build_table_utf8: NULL output");
    RR_REQUIRE(n_slots == rr_tab_slots_for(n_pieces), "rr_wp_build_table_utf8: n_slots %d, rr_wp_table_slots says %d", n_slots,
               rr_tab_slots_for(n_pieces));
    const int64_t kept = rr_wp_fill_table(h_piece_bytes, h_piece_off, n_pieces, max_chars_per_word, n_slots,
                                          reinterpret_cast<rr_tab_entry*>(h_slots));
    RR_REQUIRE(kept >= 0, "rr_wp_build_table_utf8: table overflow");
    *out_kept = (int32_t)kept;
    return RR_OK;
}

extern "C" int rr_wp_destroy(rr_wp* wp) {
    if (!wp) return RR_OK;
    hipSetDevice(wp->device);
    hipDeviceSynchronize();
    hipFree(wp->d_table); hipFree(wp->d_bytes); hipFree(wp->d_rows); hipFree(wp->d_bad);
    hipFree(wp->d_st1); hipFree(wp->d_st2); hipFree(wp->d_pool);
    delete wp;
    return RR_OK;
}

// One entry of stage2 (review-recommender_amd/wp_unicode.py builds the table from the interpreter's unicodedata):
#define RR_WPU_BLOCK 128                               // code points per block of stage2
#define RR_WPU_STAGE1 (0x110000 / RR_WPU_BLOCK)        // 8704 blocks cover U+0000 .. U+10FFFF
#define RR_WPU_DELETED 0                               // bits 0-2: the class of the raw code point
#define RR_WPU_BLANK 1
#define RR_WPU_CJK 2                                   //   every mapped code point is a word of its own
#define RR_WPU_OTHER 3
#define RR_WPU_HARD 4                                  //   depends on its neighbours: the document stays with the host
#define RR_WPU_N(e) (((e) >> 3) & 3u)                  // bits 3-4: mapped code points (0 .. 3)
#define RR_WPU_IDENTITY(e) (((e) >> 5) & 1u)           // bit 5: the mapped form is the code point itself
#define RR_WPU_PUNCT(e, j) (((e) >> (6 + (j))) & 1u)   // bits 6-8: mapped code point j is punctuation (a word of its own)
#define RR_WPU_POOL(e) ((e) >> 9)                      // bits 9-31: first mapped code point in the pool

// Everything the kernel will index with text it does not control is checked HERE, once: no stage1 block leaves stage2, no
// entry leaves the pool, and every mapped code point has a UTF-8 form of at most 4 bytes.
static int rr_wpu_check_tables(const uint16_t* stage1, int32_t n_stage1, const uint32_t* stage2, int32_t n_stage2,
                               const uint32_t* pool, int32_t n_pool) {
    const char* who = "rr_wp_create_utf8";
    RR_REQUIRE(stage1 && stage2 && pool, "%s: NULL Unicode table", who);
    RR_REQUIRE(n_stage1 == RR_WPU_STAGE1, "%s: stage1 has %d blocks, U+0000..U+10FFFF in blocks of %d are %d", who, n_stage1,
               RR_WPU_BLOCK, RR_WPU_STAGE1);
    RR_REQUIRE(n_stage2 >= RR_WPU_BLOCK && n_stage2 % RR_WPU_BLOCK == 0 && n_stage2 <= (1 << 16) * RR_WPU_BLOCK,
               "%s: stage2 has %d entries (whole blocks of %d, at most 65536 of them)", who, n_stage2, RR_WPU_BLOCK);
    RR_REQUIRE(n_pool >= 1 && n_pool < (1 << 23), "%s: %d pool entries outside [1, 2^23)", who, n_pool);
    for (int32_t b = 0; b < n_stage1; ++b)
        RR_REQUIRE((int32_t)stage1[b] < n_stage2 / RR_WPU_BLOCK, "%s: stage1[%d] = %d leaves stage2 (%d blocks)", who, b,
                   (int)stage1[b], n_stage2 / RR_WPU_BLOCK);
    for (int32_t i = 0; i < n_stage2; ++i) {
        const uint32_t e = stage2[i];
        RR_REQUIRE((e & 7u) <= RR_WPU_HARD, "%s: stage2[%d] has class %u", who, i, e & 7u);
        if (((e & 7u) == RR_WPU_CJK || (e & 7u) == RR_WPU_OTHER) && !RR_WPU_IDENTITY(e))
            RR_REQUIRE((int64_t)RR_WPU_POOL(e) + RR_WPU_N(e) <= n_pool, "%s: stage2[%d] leaves the pool", who, i);
    }
    for (int32_t i = 0; i < n_pool; ++i)
        RR_REQUIRE(pool[i] <= 0x10FFFFu && !(pool[i] >= 0xD800u && pool[i] <= 0xDFFFu),
                   "%s: pool[%d] = 0x%X is no Unicode scalar value", who, i, pool[i]);
    return RR_OK;
}

extern "C" int rr_wp_create_utf8(int32_t device, const uint8_t* h_piece_bytes, const int64_t* h_piece_off, int32_t n_pieces,
                                 int32_t unk_id, int32_t cls_id, int32_t sep_id, int32_t max_chars_per_word,
                                 const uint16_t* h_stage1, int32_t n_stage1, const uint32_t* h_stage2, int32_t n_stage2,
                                 const uint32_t* h_pool, int32_t n_pool, rr_wp** out) {
    const char* who = "rr_wp_create_utf8";
    RR_REQUIRE(out, "%s: NULL out", who);
    *out = nullptr;
    int rc = rr_wp_check_pieces(who, h_piece_bytes, h_piece_off, n_pieces, max_chars_per_word);
    if (rc) return rc;
    RR_REQUIRE(unk_id >= 0 && unk_id < n_pieces && cls_id >= 0 && cls_id < n_pieces && sep_id >= 0 && sep_id < n_pieces,
               "%s: special ids (%d, %d, %d) outside [0, %d)", who, unk_id, cls_id, sep_id, n_pieces);
    rc = rr_wpu_check_tables(h_stage1, n_stage1, h_stage2, n_stage2, h_pool, n_pool);
    if (rc) return rc;
    int ndev = 0;
    RR_HIP_TRY(hipGetDeviceCount(&ndev));
    RR_REQUIRE(device >= 0 && device < ndev, "%s: device %d not in [0,%d)", who, device, ndev);
    RR_HIP_TRY(hipSetDevice(device));
    const int32_t n_slots = rr_tab_slots_for(n_pieces);
    std::vector<rr_tab_entry> slots((size_t)n_slots);
    const int64_t kept = rr_wp_fill_table(h_piece_bytes, h_piece_off, n_pieces, max_chars_per_word, n_slots, slots.data());
    RR_REQUIRE(kept >= 0, "%s: table overflow", who);
    rr_wp* wp = new rr_wp();
    wp->device = device;
    wp->unk = unk_id; wp->cls = cls_id; wp->sep = sep_id; wp->max_chars = max_chars_per_word;
    wp->n_slots = n_slots;
    wp->n_kept = (int32_t)kept;
    const size_t nbytes = (size_t)h_piece_off[n_pieces];
    const size_t b1 = sizeof(uint16_t) * (size_t)n_stage1, b2 = sizeof(uint32_t) * (size_t)n_stage2, bp = sizeof(uint32_t) * (size_t)n_pool;
    hipError_t e = hipMalloc((void**)&wp->d_table, sizeof(rr_tab_entry) * (size_t)n_slots);
    if (e == hipSuccess) e = hipMalloc((void**)&wp->d_bytes, nbytes + 16);
    if (e == hipSuccess) e = hipMalloc((void**)&wp->d_bad, 4);
    if (e == hipSuccess) e = hipMemset(wp->d_bad, 0, 4);
    if (e == hipSuccess) e = hipMemcpy(wp->d_table, slots.data(), sizeof(rr_tab_entry) * (size_t)n_slots, hipMemcpyHostToDevice);
    if (e == hipSuccess && nbytes) e = hipMemcpy(wp->d_bytes, h_piece_bytes, nbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&wp->d_st1, b1);
    if (e == hipSuccess) e = hipMalloc((void**)&wp->d_st2, b2);
    if (e == hipSuccess) e = hipMalloc((void**)&wp->d_pool, bp);
    if (e == hipSuccess) e = hipMemcpy(wp->d_st1, h_stage1, b1, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(wp->d_st2, h_stage2, b2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(wp->d_pool, h_pool, bp, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        rr_set_error("%s: %s", who, hipGetErrorString(e));
        rr_wp_destroy(wp);
        return RR_E_HIP;
    }
    *out = wp;
    return RR_OK;
}

// ------------------------------------------------------------------ device side
// a byte below 0x80: 0 deleted, 1 blank, 2 punctuation, 3 word character
__device__ __forceinline__ int rr_wp_class(unsigned c) {
    if (c == 0x20u || c == 0x09u || c == 0x0Au || c == 0x0Du) return 1;
    if (c < 0x20u || c == 0x7Fu) return 0;
    if ((c >= 33u && c <= 47u) || (c >= 58u && c <= 64u) || (c >= 91u && c <= 96u) || (c >= 123u && c <= 126u)) return 2;
    return 3;
}

#define RR_WPU_FIRST 0x10                              // s_cl: the first byte of a character
#define RR_WPU_MAX_BYTES (4 * RR_WP_MAX_WORD)          // a word of max_chars characters: powers of the hash base in LDS

__device__ __forceinline__ int rr_wpu_utf8_len(uint32_t cp) { return cp < 0x80u ? 1 : cp < 0x800u ? 2 : cp < 0x10000u ? 3 : 4; }

// The character that STARTS at raw[i] (LDS; i < wlen): its mapped code points m[0 .. *nm) with their kinds, and the bytes
// of their UTF-8 forms (the return value).  A continuation byte starts nothing (0) and only checks that a lead byte covers
// it.  *flags |= 1: malformed UTF-8; |= 2: a hard code point.
__device__ __forceinline__ int rr_wpu_char_at(const uint8_t* raw, int i, int wlen, const uint16_t* __restrict__ st1,
                                              const uint32_t* __restrict__ st2, const uint32_t* __restrict__ pool, uint32_t* m,
                                              int* kind, int* nm, int* flags) {
    const unsigned b = raw[i];
    *nm = 0;
    if (b < 0x80u) {
        const int k = rr_wp_class(b);
        if (k == 0) return 0;
        m[0] = (b >= 'A' && b <= 'Z') ? b + 32u : b;
        kind[0] = k;
        *nm = 1;
        return 1;
    }
    if (b < 0xC0u) {
        int k = 1;
        while (k <= 3 && i - k >= 0 && (raw[i - k] & 0xC0u) == 0x80u) ++k;
        if (k > 3 || i - k < 0) { *flags |= 1; return 0; }
        const unsigned l = raw[i - k];
        const int need = l >= 0xF0u ? 4 : l >= 0xE0u ? 3 : l >= 0xC0u ? 2 : 1;
        if (need <= k) *flags |= 1;
        return 0;
    }
    uint32_t cp;
    if (!rr_utf8_decode(raw, i, wlen, &cp)) { *flags |= 1; return 0; }
    const uint32_t e = st2[(uint32_t)st1[cp >> 7] * RR_WPU_BLOCK + (cp & (RR_WPU_BLOCK - 1))];
    const unsigned cls = e & 7u;
    if (cls == RR_WPU_HARD) { *flags |= 2; return 0; }
    if (cls == RR_WPU_DELETED) return 0;
    if (cls == RR_WPU_BLANK) {
        m[0] = 0x20u;
        kind[0] = 1;
        *nm = 1;
        return 1;
    }
    const int n = (int)RR_WPU_N(e);
    int bytes = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < n) {
            const uint32_t x = RR_WPU_IDENTITY(e) ? cp : pool[RR_WPU_POOL(e) + j];
            m[j] = x;
            kind[j] = (cls == RR_WPU_CJK || RR_WPU_PUNCT(e, j)) ? 2 : 3;
            bytes += rr_wpu_utf8_len(x);
        }
    }
    *nm = n;
    return bytes;
}

__global__ __launch_bounds__(RR_WP_THREADS) void rr_wp_tokenize_utf8(
    const uint8_t* __restrict__ text, int64_t text_bytes, const int64_t* __restrict__ text_off, int32_t n_docs, int32_t max_length,
    const rr_tab_entry* __restrict__ table, uint32_t mask, const uint8_t* __restrict__ bytes, int32_t unk, int32_t cls, int32_t sep,
    int32_t max_chars, const uint16_t* __restrict__ st1, const uint32_t* __restrict__ st2, const uint32_t* __restrict__ pool,
    int32_t* __restrict__ rows /* [n_docs][max_length] */, int32_t* __restrict__ lens /* [n_docs] */,
    int32_t* __restrict__ needs_host, int32_t* __restrict__ bad) {
    __shared__ uint8_t s_ch[RR_WP_WINDOW];          // the mapped text, UTF-8, compacted
    __shared__ uint8_t s_cl[RR_WP_WINDOW];          // kind of the byte's character | RR_WPU_FIRST
    __shared__ uint8_t s_pf[RR_WP_WINDOW];          // 1 = a piece starts here
    __shared__ uint32_t s_ph[RR_WP_WINDOW + 1];     // prefix hashes, per word
    __shared__ int32_t s_id[RR_WP_WINDOW];          // the piece that starts here; before the words: the raw window
    __shared__ uint32_t s_pw[RR_WPU_MAX_BYTES + 1]; // powers of the base
    __shared__ int s_ws[RR_WP_THREADS / 64];
    uint8_t* s_raw = reinterpret_cast<uint8_t*>(s_id);
    const int tid = threadIdx.x;
    const int doc = blockIdx.x;
    int32_t* row = rows + (int64_t)doc * max_length;
    int64_t b0, len;
    if (!rr_doc_span(text_off, doc, text_bytes, &b0, &len)) {   // offsets that leave the text: nothing is read (rr_wp_status reports it)
        if (tid == 0) {
            row[0] = cls; row[1] = sep; lens[doc] = 2; needs_host[doc] = 1;
            atomicAdd(bad, 1);
        }
        return;
    }
    const uint8_t* src = text + b0;
    for (int k = tid; k <= 4 * max_chars; k += RR_WP_THREADS) {     // base^k by squaring
        uint32_t p = 1, q = RR_TAB_BASE;
        for (int e = k; e; e >>= 1) {
            if (e & 1) p *= q;
            q *= q;
        }
        s_pw[k] = p;
    }
    const bool cut = len > RR_WP_WINDOW;
    int wlen = cut ? RR_WP_WINDOW : (int)len;
    if (cut) {                                             // the window ends on a character boundary (src[wlen] is inside the text)
        for (int k = 0; k < 3 && wlen > 0 && (src[wlen] & 0xC0u) == 0x80u; ++k) --wlen;
    }
#pragma unroll
    for (int j = 0; j < RR_WP_PER; ++j) {
        const int i = tid * RR_WP_PER + j;
        if (i < wlen) s_raw[i] = src[i];
    }
    __syncthreads();

    // decode, classify, map: bytes of mapped text per thread
    uint32_t m[3];
    int kind[3];
    int nm = 0, flags = 0, mine = 0;
    for (int j = 0; j < RR_WP_PER; ++j) {
        const int i = tid * RR_WP_PER + j;
        if (i < wlen) mine += rr_wpu_char_at(s_raw, i, wlen, st1, st2, pool, m, kind, &nm, &flags);
    }
    if (__syncthreads_or(flags)) {                         // malformed UTF-8 or a hard code point: the host's
        if (tid == 0) { row[0] = cls; row[1] = sep; lens[doc] = 2; needs_host[doc] = 1; }
        return;
    }
    int n = 0;
    int at = rr_block_scan<int, RR_WP_THREADS>(mine, s_ws, &n);
    if (n > RR_WP_WINDOW) {                                // the mapped text does not fit the LDS buffers
        if (tid == 0) { row[0] = cls; row[1] = sep; lens[doc] = 2; needs_host[doc] = 1; }
        return;
    }
    for (int j = 0; j < RR_WP_PER; ++j) {
        const int i = tid * RR_WP_PER + j;
        if (i >= wlen) break;
        rr_wpu_char_at(s_raw, i, wlen, st1, st2, pool, m, kind, &nm, &flags);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (q < nm) {
                const uint32_t x = m[q];
                const int l = rr_wpu_utf8_len(x);
                if (l == 1) {
                    s_ch[at] = (uint8_t)x;
                } else if (l == 2) {
                    s_ch[at] = (uint8_t)(0xC0u | (x >> 6));
                    s_ch[at + 1] = (uint8_t)(0x80u | (x & 0x3Fu));
                } else if (l == 3) {
                    s_ch[at] = (uint8_t)(0xE0u | (x >> 12));
                    s_ch[at + 1] = (uint8_t)(0x80u | ((x >> 6) & 0x3Fu));
                    s_ch[at + 2] = (uint8_t)(0x80u | (x & 0x3Fu));
                } else {
                    s_ch[at] = (uint8_t)(0xF0u | (x >> 18));
                    s_ch[at + 1] = (uint8_t)(0x80u | ((x >> 12) & 0x3Fu));
                    s_ch[at + 2] = (uint8_t)(0x80u | ((x >> 6) & 0x3Fu));
                    s_ch[at + 3] = (uint8_t)(0x80u | (x & 0x3Fu));
                }
                for (int r = 0; r < l; ++r) {
                    s_cl[at + r] = (uint8_t)(kind[q] | (r == 0 ? RR_WPU_FIRST : 0));
                    s_pf[at + r] = 0;
                }
                at += l;
            }
        }
    }
    __syncthreads();                                       // (s_raw is dead from here: s_id takes its place)

    // one thread per word
    for (int i = tid; i < n; i += RR_WP_THREADS) {
        const int c = s_cl[i];
        if (!(c & RR_WPU_FIRST)) continue;
        const int k = c & 7;
        if (k == 2) {                                      // one character, 1 .. 4 bytes
            const unsigned b = s_ch[i];
            const int l = b < 0x80u ? 1 : b < 0xE0u ? 2 : b < 0xF0u ? 3 : 4;
            uint32_t h = 0;
            for (int p = 0; p < l; ++p) h = h * RR_TAB_BASE + s_ch[i + p];
            const int id = rr_tab_lookup(table, mask, bytes, h, l, l, s_ch + i);
            s_id[i] = id < 0 ? unk : id;
            s_pf[i] = 1;
        } else if (k == 3 && (i == 0 || (s_cl[i - 1] & 7) != 3)) {
            int e = i + 1, chars = 1;
            while (e < n && (s_cl[e] & 7) == 3) {
                chars += (s_cl[e] & RR_WPU_FIRST) ? 1 : 0;
                ++e;
            }
            if (cut && e == n) continue;                 // the window may have cut this word: it does not count
            if (chars > max_chars) {
                s_id[i] = unk;
                s_pf[i] = 1;
                continue;
            }
            uint32_t h = 0;
            s_ph[i] = 0;
            for (int p = i; p < e; ++p) {
                h = h * RR_TAB_BASE + s_ch[p];
                s_ph[p + 1] = h;
            }
            int start = i;
            bool whole = true;
            while (start < e) {
                int end = e, id = -1;
                for (; end > start; --end) {
                    if (end < e && !(s_cl[end] & RR_WPU_FIRST)) continue;      // candidates end on character boundaries
                    const uint32_t hh = s_ph[end] - s_ph[start] * s_pw[end - start];
                    id = rr_tab_lookup(table, mask, bytes, hh, (end - start) | (start > i ? 1 << 16 : 0), end - start, s_ch + start);
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
    mine = 0;
#pragma unroll
    for (int j = 0; j < RR_WP_PER; ++j) {
        const int i = tid * RR_WP_PER + j;
        mine += (i < n && s_pf[i]) ? 1 : 0;
    }
    int total = 0;
    int rank = rr_block_scan<int, RR_WP_THREADS>(mine, s_ws, &total);
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
        int all;
        const int at = rr_block_scan<int, 1024>(v, s_w, &all);
        if (i < n_docs) cu[i + 1] = carry + at + v;
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
    // grown on the first call of a size
    const int rc = rr_grow((void**)&wp->d_rows, &wp->cap_words, words, sizeof(int32_t), "rr_wp_encode_dev");
    if (rc != RR_OK) return rc;
    int32_t* d_lens = wp->d_rows + (int64_t)n_docs * max_length;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rr_wp_tokenize_utf8, dim3((unsigned)n_docs), dim3(RR_WP_THREADS), 0, st, d_text, text_bytes, d_text_off,
                       n_docs, max_length, wp->d_table, (uint32_t)(wp->n_slots - 1), wp->d_bytes, wp->unk, wp->cls, wp->sep,
                       wp->max_chars, wp->d_st1, wp->d_st2, wp->d_pool, wp->d_rows, d_lens, d_needs_host, wp->d_bad);
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
    const int rc = rr_take_bad_docs(wp->d_bad, out_bad_docs);
    if (rc != RR_OK) return rc;
    const int32_t bad = *out_bad_docs;
    RR_REQUIRE(bad == 0, "rr_wp_status: %d document(s) had text offsets that decrease or leave the text (they were answered "
               "[CLS] [SEP] with needs_host = 1)", bad);
    return RR_OK;
}
