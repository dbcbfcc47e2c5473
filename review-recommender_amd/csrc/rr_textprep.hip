// rr_textprep.hip -- review text cleaned, filtered and deduplicated on the device, in front of the tokenizer.
//
// Stands in for nlp/11_build_product_embeddings.py:110-118 (normalize_text, the length filter, looks_spammy,
// drop_duplicates(subset=["sku", "__txt"])).  textprep.model_clean states in plain Python what rr_tp_clean computes.
//
// rr_tp_clean     one workgroup per document.  The raw document (at most RR_TP_WINDOW bytes) is copied to LDS and walked in
//                 tiles of RR_TP_TILE bytes, RR_TP_PER consecutive bytes per thread.  Every byte that STARTS a character is
//                 decoded (reads behind a lead byte are bounded by the document's end) and classed whitespace / other.  A
//                 character that is not whitespace emits its bytes, with one space in front when the character before it
//                 is whitespace: that is strip() and the collapse of \s+ at once.  The state at the start of a thread's
//                 slice (was the previous character whitespace?) is read from the raw bytes in LDS, so it does not matter
//                 where a tile or a slice ends.  A block scan over (code points, bytes) packed in one int gives every
//                 character its place in the output and its code-point index; whatever has an index >= max_chars (4000 for
//                 nlp/11, none for nlp/10) is not written (the cut comes after the collapse, so the text may end in a space).  The normalised text is a
//                 second LDS buffer; the three spam rules then run over THAT buffer with plain bounded look-ahead, so a
//                 phrase, a URL prefix or a run of ten has no edge to straddle:
//                   URL_RE     candidates = "http://", "https://", "www." (ASCII, any case) followed by a byte that is not a
//                              space; after the collapse a match runs to its token's end, so two matches <=> a space lies
//                              between the first and the last candidate;
//                   PROMO_RE   three literal phrases, and min(end of "i received this") <= max(start of "free");
//                   REPEAT_RE  a character of L bytes at p with s[p + k] == s[p + k + L] for k < 9 L.
// rr_tp_insert    one wave per surviving document: 64-bit hash of (group, bytes), linear probing in a table of >= 2n slots;
//                 an empty slot is claimed by compare-and-swap on its representative document, an occupied one is compared
//                 BYTE BY BYTE with its representative (a hash never decides); atomicMin of the document index per slot.
// rr_tp_mark      a survivor whose slot's minimum is another document is a duplicate.  Slots are never emptied and a
//                 representative never changes, so equal documents always end in the same slot: the result does not depend
//                 on which of them claimed it.
// rr_tp_rank      survivors' ranks and byte offsets (one workgroup, chunks of 1024, as rr_wp_scan).
// rr_tp_gather    one workgroup per survivor copies its text behind its predecessor's.
// rr_tp_head      the first max_chars code points of documents of any length, normalised or raw (see there).
#include "rr_prims.h"

#define RR_TP_THREADS 256
#define RR_TP_PER 16                                   // consecutive bytes per thread
#define RR_TP_TILE (RR_TP_THREADS * RR_TP_PER)         // 4096 bytes per step of the walk
#define RR_TP_WINDOW (4 * RR_TP_TILE)                  // 16384: 4000 characters of 3 bytes fit with room to spare
#define RR_TP_MAX_CHARS 4000                           // nlp/11_build_product_embeddings.py:22-23
#define RR_TP_MIN_CHARS 10

struct rr_textprep {
    int device = 0;
    int32_t* d_bad = nullptr;        // [0] documents whose offsets a kernel refused (rr_textprep_status), [1] the running head call was refused
    int32_t* d_scratch = nullptr;    // dedup: representative [slots], minimum [slots], slot of document [n]; compact: rank [n]
    int64_t cap_words = 0;
    std::mutex mu;
};

__device__ __forceinline__ bool rr_tp_is_space(uint32_t c) {          // str.isspace() == re's \s for str patterns
    return (c >= 0x09u && c <= 0x0Du) || (c >= 0x1Cu && c <= 0x20u) || c == 0x85u || c == 0xA0u || c == 0x1680u ||
           (c >= 0x2000u && c <= 0x200Au) || c == 0x2028u || c == 0x2029u || c == 0x202Fu || c == 0x205Fu || c == 0x3000u;
}

// s[p .. p + m) equals the lower-case ASCII literal `lit`, letters A-Z of s folded; false when it would leave s[0 .. n).
__device__ __forceinline__ bool rr_tp_match(const uint8_t* s, int p, int n, const char* lit, int m) {
    if (p + m > n) return false;
    for (int k = 0; k < m; ++k) {
        uint32_t c = s[p + k];
        if (c >= 'A' && c <= 'Z') c |= 0x20u;
        if (c != (uint32_t)(uint8_t)lit[k]) return false;
    }
    return true;
}

__global__ __launch_bounds__(RR_TP_THREADS) void rr_tp_clean(
    const uint8_t* text /* no __restrict__: `out` may be the same buffer */, int64_t text_bytes,
    const int64_t* __restrict__ text_off, int32_t spam, int32_t max_chars, uint8_t* out, int32_t* __restrict__ out_len, int32_t* __restrict__ status, int32_t* __restrict__ bad) {
    __shared__ uint8_t s_raw[RR_TP_WINDOW];
    __shared__ uint8_t s_out[RR_TP_WINDOW];
    __shared__ int s_ws[RR_TP_THREADS / 64];
    __shared__ int s_end, s_cps, s_claimed, s_umin, s_umax, s_emin, s_fmax;
    const int tid = threadIdx.x;
    const int doc = blockIdx.x;
    int64_t b0, len64;
    if (!rr_doc_span(text_off, doc, text_bytes, &b0, &len64)) {   // offsets that leave the text: nothing is read, no text is written
        if (tid == 0) {
            out_len[doc] = 0; status[doc] = RR_TP_NEEDS_HOST;
            atomicAdd(bad, 1);
        }
        return;
    }
    if (len64 > RR_TP_WINDOW) {                          // longer than the window: the host cleans it
        if (tid == 0) { out_len[doc] = 0; status[doc] = RR_TP_NEEDS_HOST; }
        return;
    }
    const int len = (int)len64;
    const uint8_t* src = text + b0;
    for (int i = tid; i < len; i += RR_TP_THREADS) s_raw[i] = src[i];
    if (tid == 0) { s_end = 0; s_cps = 0; s_claimed = 0; s_umin = RR_TP_WINDOW; s_umax = -1; s_emin = RR_TP_WINDOW; s_fmax = -1; }
    __syncthreads();

    uint32_t first = 0;
    const int phantom = (len > 0 && (s_raw[0] & 0xC0u) != 0x80u && rr_utf8_decode(s_raw, 0, len, &first) && rr_tp_is_space(first)) ? 1 : 0;
    int carry_cp = 0, carry_by = 0;                        // emitted before this tile (the same in every thread)
    int malformed = 0, hard = 0, claimed = 0, my_end = 0, my_cps = 0;
    for (int base = 0; base < len; base += RR_TP_TILE) {
        const int i0 = base + tid * RR_TP_PER;
        // was the character before this slice whitespace?  (the start of the text counts as "no": its space is the phantom)
        bool prev_ws = false;
        if (i0 > 0 && i0 < len) {
            int k = i0 - 1;
            for (int back = 0; back < 3 && k > 0 && (s_raw[k] & 0xC0u) == 0x80u; ++back) --k;
            uint32_t c;
            prev_ws = (s_raw[k] & 0xC0u) != 0x80u && rr_utf8_decode(s_raw, k, len, &c) && rr_tp_is_space(c);
        }
        uint8_t info[RR_TP_PER];                           // bytes to emit (0 = none) | 8 = a space in front
        int packed = 0;                                    // code points << 16 | bytes of this slice
#pragma unroll
        for (int j = 0; j < RR_TP_PER; ++j) {
            const int i = i0 + j;
            info[j] = 0;
            if (i < len && (s_raw[i] & 0xC0u) != 0x80u) {
                uint32_t c;
                const int n = rr_utf8_decode(s_raw, i, len, &c);
                if (n == 0) { malformed = 1; prev_ws = false; }
                else {
                    claimed += n;
                    if (c == 0x130u || c == 0x131u || c == 0x17Fu) hard = 1;
                    if (rr_tp_is_space(c)) prev_ws = true;
                    else {
                        info[j] = (uint8_t)(n | (prev_ws ? 8 : 0));
                        packed += ((prev_ws ? 2 : 1) << 16) | (n + (prev_ws ? 1 : 0));
                        prev_ws = false;
                    }
                }
            }
        }
        int total;
        int at = rr_block_scan<int, RR_TP_THREADS>(packed, s_ws, &total);
        int g_cp = carry_cp + (at >> 16), g_by = carry_by + (at & 0xFFFF);
#pragma unroll
        for (int j = 0; j < RR_TP_PER; ++j) {
            if (!info[j]) continue;
            const int n = info[j] & 7;
            int sp = info[j] >> 3;
            int cp = g_cp, by = g_by;
            g_cp += 1 + sp; g_by += n + sp;                // what the scan counted for this character
            if (cp == 0) sp = 0;                           // the first character of the result: the space in front of it is stripped
            else { cp -= phantom; by -= phantom; }         // (and was counted: everything behind it moves up)
            if (sp && cp < max_chars && by >= 0 && by < RR_TP_WINDOW) {
                s_out[by] = ' ';
                my_end = by + 1 > my_end ? by + 1 : my_end;
                my_cps = cp + 1 > my_cps ? cp + 1 : my_cps;
            }
            cp += sp; by += sp;
            if (cp < max_chars && by >= 0 && by + n <= RR_TP_WINDOW) {
                const int i = i0 + j;
                for (int k = 0; k < n; ++k) s_out[by + k] = s_raw[i + k];
                my_end = by + n > my_end ? by + n : my_end;
                my_cps = cp + 1 > my_cps ? cp + 1 : my_cps;
            }
        }
        carry_cp += total >> 16;
        carry_by += total & 0xFFFF;
    }
    atomicMax(&s_end, my_end);
    atomicMax(&s_cps, my_cps);
    atomicAdd(&s_claimed, claimed);
    const int any_bad = __syncthreads_or(malformed);
    const int any_hard = __syncthreads_or(hard);
    // every byte belongs to exactly one well-formed character <=> the starts are well formed and their lengths add up
    if (any_bad || s_claimed != len || (spam && any_hard)) {
        if (tid == 0) { out_len[doc] = 0; status[doc] = RR_TP_NEEDS_HOST; }
        return;
    }
    const int n = s_end;
    int st = s_cps < RR_TP_MIN_CHARS ? RR_TP_SHORT : 0;

    if (spam) {
        int hit = 0;
        for (int p = tid; p < n; p += RR_TP_THREADS) {
            uint32_t c = s_out[p];
            if (c >= 'A' && c <= 'Z') c |= 0x20u;
            int q = -1;                                    // the byte behind a URL prefix that starts here
            switch (c) {
            case 'h':
                if (rr_tp_match(s_out, p, n, "http://", 7)) q = p + 7;
                else if (rr_tp_match(s_out, p, n, "https://", 8)) q = p + 8;
                break;
            case 'w': if (rr_tp_match(s_out, p, n, "www.", 4)) q = p + 4; break;
            case 'd': hit |= rr_tp_match(s_out, p, n, "discount code", 13); break;
            case 'u': hit |= rr_tp_match(s_out, p, n, "use code", 8); break;
            case 's': hit |= rr_tp_match(s_out, p, n, "sponsored", 9); break;
            case 'i': if (rr_tp_match(s_out, p, n, "i received this", 15)) atomicMin(&s_emin, p + 15); break;
            case 'f': if (rr_tp_match(s_out, p, n, "free", 4)) atomicMax(&s_fmax, p); break;
            default: break;
            }
            if (q >= 0 && q < n && s_out[q] != ' ') { atomicMin(&s_umin, p); atomicMax(&s_umax, p); }
            if ((c & 0xC0u) != 0x80u) {                     // ten equal characters from here on
                const int L = c < 0x80u ? 1 : c < 0xE0u ? 2 : c < 0xF0u ? 3 : 4;
                if (p + 10 * L <= n) {
                    int k = 0;
                    while (k < 9 * L && s_out[p + k] == s_out[p + k + L]) ++k;
                    hit |= k == 9 * L;
                }
            }
        }
        hit = __syncthreads_or(hit);
        if (s_emin <= s_fmax) hit = 1;                      // "i received this" ... "free"
        int between = 0;                                    // two URL matches <=> a space between the outermost candidates
        for (int p = s_umin + tid; p < s_umax; p += RR_TP_THREADS) between |= s_out[p] == ' ';
        if (__syncthreads_or(between)) hit = 1;
        if (hit) st |= RR_TP_SPAM;
    }
    uint8_t* dst = out + b0;
    for (int p = tid; p < n; p += RR_TP_THREADS) dst[p] = s_out[p];
    if (tid == 0) { out_len[doc] = n; status[doc] = st; }
}

// ------------------------------------------------------------------------------------------------ heads of long documents
// The first max_chars code points of a document of ANY length (textprep.model_head states the rules): normalised
// (nlp/11's normalize_text read as a prefix computation) or raw (str[:k]).  Measure / scan / write, as rr_gate.hip's plane:
//   rr_tp_head_check      one thread per output document: its source row, its text span and (write) its output span.  One
//                         refused document sets the call's flag and NO workgroup of the call reads or writes text.
//   rr_tp_head<false>     one workgroup per document walks it in tiles of RR_TP_TILE bytes, RR_TP_PER consecutive bytes per
//                         thread.  A tile is classified from LDS with RR_TP_HALO bytes on each side: the character that starts
//                         in the tile is decoded by the thread that owns its first byte (reading on into the right halo), and
//                         what a slice needs to know about the bytes in front of it -- is the character before it whitespace,
//                         how many continuation bytes of it are still due -- is read from the three bytes in front of the slice
//                         (the left halo for the first thread: the pending space crosses a tile edge there, not in a register).
//                         One block scan over (emissions << 16 | bytes) places every emission; the emitted count and bytes are
//                         carried from tile to tile, and "something was emitted" is count > 0.  The walk leaves its loop at the
//                         first tile in which the count reaches max_chars.  A malformed byte counts only while the emissions in
//                         front of it are fewer than max_chars: that is "decoded while fewer than max_chars were emitted", and
//                         it does not depend on where a tile ends.
//   rr_tp_head<true>      the same walk for the documents whose status word is 0, writing at d_out_off.
#define RR_TP_HALO 3
#define RR_TP_HEAD_MAX_CHARS (1 << 28)                  // 4 bytes per code point stay below 2^31

__global__ void rr_tp_head_check(int64_t text_bytes, const int64_t* __restrict__ text_off, const int32_t* __restrict__ doc_rows,
                                 int32_t n_docs, int32_t n_src_docs, const int32_t* __restrict__ out_len,
                                 const int32_t* __restrict__ status, const int64_t* __restrict__ out_off, int64_t out_bytes,
                                 int32_t* __restrict__ bad) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_docs) return;
    const int64_t src = doc_rows ? (int64_t)doc_rows[j] : j;
    bool ok = src >= 0 && src < n_src_docs;
    if (ok) {
        int64_t b0, len;
        ok = rr_doc_span(text_off, (int)src, text_bytes, &b0, &len);
    }
    if (ok && out_off) {
        const int64_t o0 = out_off[j], o1 = out_off[j + 1];
        ok = o0 >= 0 && o1 >= o0 && o1 <= out_bytes && (status[j] != 0 || o1 - o0 >= out_len[j]);
    }
    if (!ok) { atomicAdd(bad, 1); bad[1] = 1; }             // (a count and a flag: the same whatever the order)
}

template <bool WRITE>
__global__ __launch_bounds__(RR_TP_THREADS) void rr_tp_head(
    const uint8_t* __restrict__ text, const int64_t* __restrict__ text_off, const int32_t* __restrict__ doc_rows, int32_t max_chars,
    int32_t normalize, int32_t min_chars, int32_t* out_len, int32_t* status, const int64_t* __restrict__ out_off,
    uint8_t* __restrict__ out, const int32_t* __restrict__ bad) {
    __shared__ uint8_t s_raw[RR_TP_TILE + 2 * RR_TP_HALO];   // s_raw[RR_TP_HALO + k] = byte base + k of the document
    __shared__ int s_ws[RR_TP_THREADS / 64];
    __shared__ int s_len;
    const int tid = threadIdx.x;
    const int doc = blockIdx.x;
    if (bad[1]) {                                             // the call was refused: nothing is read or written
        if (!WRITE && tid == 0) { out_len[doc] = 0; status[doc] = RR_TP_NEEDS_HOST; }
        return;
    }
    if (WRITE && status[doc] != 0) return;
    const int src_doc = doc_rows ? doc_rows[doc] : doc;
    const int64_t b0 = text_off[src_doc], len = text_off[src_doc + 1] - b0;
    const uint8_t* __restrict__ src = text + b0;
    uint8_t* dst = nullptr;
    int room = 0;                                             // bytes this document may write
    if (WRITE) {
        dst = out + out_off[doc];
        const int64_t r = out_off[doc + 1] - out_off[doc];
        room = r > INT32_MAX ? INT32_MAX : (int)r;
    }
    if (tid == 0) s_len = -1;
    int phantom = 0;                                          // the document begins with whitespace
    int carry_cp = 0, carry_by = 0;                           // emitted before this tile (the same in every thread)
    int malformed = 0;
    for (int64_t base = 0; base < len && carry_cp < max_chars; base += RR_TP_TILE) {
        __syncthreads();                                      // (the previous tile is still being copied from)
        for (int i = tid; i < RR_TP_TILE + 2 * RR_TP_HALO; i += RR_TP_THREADS) {
            const int64_t d = base - RR_TP_HALO + i;
            s_raw[i] = d >= 0 && d < len ? src[d] : (uint8_t)0;
        }
        __syncthreads();
        const int64_t left = len - base;
        const int own_end = RR_TP_HALO + (int)(left < RR_TP_TILE ? left : RR_TP_TILE);                    // bytes of this tile
        const int dec_end = RR_TP_HALO + (int)(left < RR_TP_TILE + RR_TP_HALO ? left : RR_TP_TILE + RR_TP_HALO);
        const int first = base == 0 ? RR_TP_HALO : 0;        // the first byte of s_raw that belongs to the document
        if (base == 0) {
            uint32_t c;
            phantom = normalize && (s_raw[RR_TP_HALO] & 0xC0u) != 0x80u && rr_utf8_decode(s_raw, RR_TP_HALO, dec_end, &c) &&
                      rr_tp_is_space(c) ? 1 : 0;
        }
        const int p0 = RR_TP_HALO + tid * RR_TP_PER;
        // the character in front of this slice: is it whitespace, and how many of its bytes lie in the slice?
        bool prev_ws = false;
        int due = 0;
        if (p0 < own_end) {
            int k = p0 - 1;
            while (k >= first && k > p0 - 1 - RR_TP_HALO && (s_raw[k] & 0xC0u) == 0x80u) --k;
            if (k >= first && k >= p0 - RR_TP_HALO && (s_raw[k] & 0xC0u) != 0x80u) {
                uint32_t c;
                const int n = rr_utf8_decode(s_raw, k, dec_end, &c);
                if (n) { prev_ws = normalize && rr_tp_is_space(c); due = k + n - p0 > 0 ? k + n - p0 : 0; }
            }
        }
        uint8_t info[RR_TP_PER];                              // bytes to emit (0 = none) | 8 = a space in front
        unsigned events = 0;                                  // bit j: byte j is malformed (starts nothing, or a stray 10xxxxxx)
        int packed = 0;                                       // emissions << 16 | bytes of this slice
#pragma unroll
        for (int j = 0; j < RR_TP_PER; ++j) {
            const int i = p0 + j;
            info[j] = 0;
            if (i >= own_end) continue;
            if ((s_raw[i] & 0xC0u) == 0x80u) {
                if (due > 0) --due;
                else events |= 1u << j;
                continue;
            }
            uint32_t c;
            const int n = rr_utf8_decode(s_raw, i, dec_end, &c);
            due = n > 0 ? n - 1 : 0;
            if (n == 0) { events |= 1u << j; prev_ws = false; }
            else if (normalize && rr_tp_is_space(c)) prev_ws = true;
            else {
                info[j] = (uint8_t)(n | (prev_ws ? 8 : 0));
                packed += ((prev_ws ? 2 : 1) << 16) | (n + (prev_ws ? 1 : 0));
                prev_ws = false;
            }
        }
        int total;
        const int at = rr_block_scan<int, RR_TP_THREADS>(packed, s_ws, &total);
        // the space in front of the document's first character was counted and is not emitted: it and everything behind
        // it in this tile move up by one
        const int ph = phantom && carry_cp == 0 ? 1 : 0;
        int cp = carry_cp + (at >> 16) - ph, by = carry_by + (at & 0xFFFF) - ph;
#pragma unroll
        for (int j = 0; j < RR_TP_PER; ++j) {
            if ((events >> j) & 1u) malformed |= (cp < 0 ? 0 : cp) < max_chars;     // met while the walk was still decoding
            if (!info[j]) continue;
            const int n = info[j] & 7;
            int sp = info[j] >> 3;
            int c_at = cp, b_at = by;
            cp += 1 + sp; by += n + sp;                       // what the scan counted for this character
            if (c_at < 0) { sp = 0; c_at = 0; b_at = 0; }     // the first character of the head: its space is stripped
            if (sp) {
                if (c_at < max_chars) {
                    if (WRITE && b_at + 1 <= room) dst[b_at] = ' ';
                    if (c_at == max_chars - 1) s_len = b_at + 1;                   // the space is the last emission
                }
                ++c_at; ++b_at;
            }
            if (c_at < max_chars) {
                if (WRITE && b_at + n <= room)
                    for (int k = 0; k < n; ++k) dst[b_at + k] = s_raw[p0 + j + k];
                if (c_at == max_chars - 1) s_len = b_at + n;
            }
        }
        const int t_cp = total >> 16, t_by = total & 0xFFFF;
        carry_cp += t_cp - (ph && t_cp > 0 ? 1 : 0);
        carry_by += t_by - (ph && t_cp > 0 ? 1 : 0);
    }
    if (WRITE) return;
    const int any_bad = __syncthreads_or(malformed);          // (also orders s_len)
    if (tid == 0) {
        const int emitted = carry_cp < max_chars ? carry_cp : max_chars;
        if (any_bad) { out_len[doc] = 0; status[doc] = RR_TP_NEEDS_HOST; }
        else {
            out_len[doc] = s_len >= 0 ? s_len : carry_by;
            status[doc] = min_chars > 0 && emitted < min_chars ? RR_TP_SHORT : 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ dedup
__global__ __launch_bounds__(256) void rr_tp_insert(
    const uint8_t* __restrict__ text, int64_t text_bytes, const int64_t* __restrict__ text_off, const int32_t* __restrict__ lens,
    const int32_t* __restrict__ group, const int32_t* __restrict__ status, int32_t n_docs, int32_t hash_bits, uint32_t mask,
    int32_t* rep, int32_t* minimum, int32_t* __restrict__ slot_of, int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t doc64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (doc64 >= n_docs) return;
    const int doc = (int)doc64;
    if (status[doc] != 0) { if (lane == 0) slot_of[doc] = -1; return; }
    const int64_t b0 = text_off[doc];
    const int len = lens[doc];
    if (b0 < 0 || len < 0 || b0 + len > text_bytes) {       // a survivor whose text leaves the buffer: not read, reported
        if (lane == 0) { slot_of[doc] = -1; atomicAdd(bad, 1); }
        return;
    }
    const uint8_t* p = text + b0;
    const int32_t g = group[doc];
    uint64_t h = 0;                                         // a SUM of mixed 8-byte words: the lanes can add in any order
    for (int c = lane; 8 * c < len; c += 64) {
        uint64_t w = 0;
        for (int k = 0; k < 8 && 8 * c + k < len; ++k) w |= (uint64_t)p[8 * c + k] << (8 * k);
        h += rr_mix64(w + (uint64_t)(c + 1) * 0x9E3779B97F4A7C15ull);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) h += __shfl_xor(h, m, 64);
    h = rr_mix64(h ^ rr_mix64(((uint64_t)(uint32_t)g << 32) | (uint32_t)len));
    if (hash_bits < 64) h &= (1ull << hash_bits) - 1;       // tests: almost every probe collides
    uint32_t slot = (uint32_t)h & mask;
    for (;;) {
        int old = 0;
        if (lane == 0) old = atomicCAS(&rep[slot], -1, doc);
        old = __shfl(old, 0, 64);
        if (old == -1 || old == doc) break;                 // claimed: this document represents the slot
        bool same = group[old] == g && lens[old] == len;    // (representatives passed the bounds check above)
        if (same) {
            const uint8_t* q = text + text_off[old];
            int diff = 0;
            for (int i = lane; i < len; i += 64) diff |= p[i] != q[i];
            same = __ballot(diff) == 0;
        }
        if (same) break;
        slot = (slot + 1) & mask;                           // fewer documents than half the slots: an empty one comes
    }
    if (lane == 0) { slot_of[doc] = (int32_t)slot; atomicMin(&minimum[slot], doc); }
}

__global__ void rr_tp_mark(const int32_t* __restrict__ slot_of, const int32_t* __restrict__ minimum, int32_t n_docs,
                           int32_t* __restrict__ status) {
    const int64_t doc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (doc >= n_docs) return;
    const int32_t s = slot_of[doc];
    if (s >= 0 && minimum[s] != (int32_t)doc) status[doc] |= RR_TP_DUP;
}

// ------------------------------------------------------------------------------------------------ compact
__global__ __launch_bounds__(1024) void rr_tp_rank(const int32_t* __restrict__ status, const int32_t* __restrict__ lens, int32_t n_docs,
                                                   int32_t* __restrict__ rank, int64_t* __restrict__ out_off,
                                                   int32_t* __restrict__ src_row, int64_t* __restrict__ count) {
    __shared__ long long s_ws[16];
    const int tid = threadIdx.x;
    const long long bytes_mask = (1ll << 48) - 1;          // one scan of survivors << 48 | bytes: a chunk's bytes stay below 2^41
    int carry_c = 0;
    long long carry_b = 0;
    for (int64_t base = 0; base < n_docs; base += 1024) {
        const int64_t i = base + tid;
        const bool keep = i < n_docs && status[i] == 0;
        const long long b = keep ? (lens[i] > 0 ? lens[i] : 0) : 0;
        long long all;
        const long long at = rr_block_scan<long long, 1024>(((long long)keep << 48) | b, s_ws, &all);
        if (i < n_docs) {
            const int r = carry_c + (int)(at >> 48);
            rank[i] = keep ? r : -1;
            if (keep) { out_off[r] = carry_b + (at & bytes_mask); src_row[r] = (int32_t)i; }
        }
        carry_c += (int)(all >> 48);
        carry_b += all & bytes_mask;
    }
    if (tid == 0) { out_off[carry_c] = carry_b; count[0] = carry_c; count[1] = carry_b; }
}

__global__ __launch_bounds__(256) void rr_tp_gather(const uint8_t* __restrict__ text, int64_t text_bytes, const int64_t* __restrict__ text_off,
                                                    const int32_t* __restrict__ lens, const int32_t* __restrict__ rank,
                                                    const int64_t* __restrict__ out_off, uint8_t* __restrict__ out_text,
                                                    int64_t out_bytes, int32_t* __restrict__ bad) {
    const int doc = blockIdx.x;
    const int32_t r = rank[doc];
    if (r < 0) return;
    const int64_t b0 = text_off[doc], o0 = out_off[r];
    const int len = lens[doc];
    if (len <= 0) return;
    if (b0 < 0 || b0 + len > text_bytes || o0 + len > out_bytes) {     // nothing is read or written outside the two buffers
        if (threadIdx.x == 0) atomicAdd(bad, 1);
        return;
    }
    for (int i = threadIdx.x; i < len; i += 256) out_text[o0 + i] = text[b0 + i];
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int rr_textprep_destroy(rr_textprep* tp) {
    if (!tp) return RR_OK;
    hipSetDevice(tp->device);
    hipFree(tp->d_bad); hipFree(tp->d_scratch);
    delete tp;
    return RR_OK;
}

extern "C" int rr_textprep_create(int32_t device, rr_textprep** out) {
    RR_REQUIRE(out, "rr_textprep_create: NULL out");
    *out = nullptr;
    RR_HIP_TRY(hipSetDevice(device));
    rr_textprep* tp = new rr_textprep();
    tp->device = device;
    hipError_t e = hipMalloc((void**)&tp->d_bad, 8);
    if (e == hipSuccess) e = hipMemset(tp->d_bad, 0, 8);
    if (e != hipSuccess) {
        rr_set_error("rr_textprep_create: %s", hipGetErrorString(e));
        rr_textprep_destroy(tp);
        return RR_E_HIP;
    }
    *out = tp;
    return RR_OK;
}

extern "C" int rr_textprep_limits(int32_t* out_window, int32_t* out_tile, int32_t* out_per_thread) {
    RR_REQUIRE(out_window && out_tile && out_per_thread, "rr_textprep_limits: NULL argument");
    *out_window = RR_TP_WINDOW; *out_tile = RR_TP_TILE; *out_per_thread = RR_TP_PER;
    return RR_OK;
}

extern "C" int rr_textprep_clean_chars_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                           int32_t n_docs, int32_t spam, int32_t max_chars, uint8_t* d_out, int32_t* d_out_len,
                                           int32_t* d_status, void* stream) {
    RR_REQUIRE(tp && d_text_off && d_out_len && d_status, "rr_textprep_clean_dev: NULL argument");
    RR_REQUIRE(n_docs >= 0 && text_bytes >= 0, "rr_textprep_clean_dev: %d documents, %lld bytes", n_docs, (long long)text_bytes);
    RR_REQUIRE((d_text && d_out) || text_bytes == 0, "rr_textprep_clean_dev: NULL text with %lld bytes", (long long)text_bytes);
    RR_REQUIRE(max_chars >= 0, "rr_textprep_clean_dev: max_chars %d is negative", max_chars);
    if (n_docs == 0) return RR_OK;
    std::lock_guard<std::mutex> lk(tp->mu);
    RR_HIP_TRY(hipSetDevice(tp->device));
    hipLaunchKernelGGL(rr_tp_clean, dim3((unsigned)n_docs), dim3(RR_TP_THREADS), 0, (hipStream_t)stream, d_text, text_bytes,
                       d_text_off, spam ? 1 : 0, max_chars > 0 ? max_chars : INT32_MAX, d_out, d_out_len, d_status, tp->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_textprep_clean_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                     int32_t n_docs, int32_t spam, uint8_t* d_out, int32_t* d_out_len, int32_t* d_status,
                                     void* stream) {
    return rr_textprep_clean_chars_dev(tp, d_text, text_bytes, d_text_off, n_docs, spam, RR_TP_MAX_CHARS, d_out, d_out_len, d_status,
                                       stream);
}

extern "C" int rr_textprep_status(rr_textprep* tp, int32_t* out_bad_docs) {
    RR_REQUIRE(tp && out_bad_docs, "rr_textprep_status: NULL argument");
    std::lock_guard<std::mutex> lk(tp->mu);
    RR_HIP_TRY(hipSetDevice(tp->device));
    const int rc = rr_take_bad_docs(tp->d_bad, out_bad_docs);
    if (rc != RR_OK) return rc;
    const int32_t bad = *out_bad_docs;
    RR_REQUIRE(bad == 0, "rr_textprep_status: %d document(s) had text offsets that decrease or leave the text, or (head calls) a source "
               "row outside the documents or an output span outside its buffer (no text was read or written for them)", bad);
    return RR_OK;
}

static int rr_tp_head_args(const char* who, rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                           int32_t n_src_docs, int32_t n_docs, int32_t max_chars, int32_t min_chars, const void* d_out_len,
                           const void* d_status) {
    RR_REQUIRE(tp && d_text_off && d_out_len && d_status, "%s: NULL argument", who);
    RR_REQUIRE(n_docs >= 0 && n_src_docs >= 0 && text_bytes >= 0, "%s: %d of %d documents, %lld bytes", who, n_docs, n_src_docs,
               (long long)text_bytes);
    RR_REQUIRE(d_text || text_bytes == 0, "%s: NULL text with %lld bytes", who, (long long)text_bytes);
    RR_REQUIRE(max_chars >= 0 && max_chars <= RR_TP_HEAD_MAX_CHARS && min_chars >= 0, "%s: max_chars %d outside [0, 2^28] or min_chars %d negative",
               who, max_chars, min_chars);
    return RR_OK;
}

extern "C" int rr_textprep_head_measure_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                            int32_t n_src_docs, const int32_t* d_doc_rows, int32_t n_docs, int32_t max_chars,
                                            int32_t normalize, int32_t min_chars, int32_t* d_out_len, int32_t* d_status,
                                            void* stream) {
    const int rc = rr_tp_head_args("rr_textprep_head_measure_dev", tp, d_text, text_bytes, d_text_off, n_src_docs, n_docs, max_chars,
                                   min_chars, d_out_len, d_status);
    if (rc != RR_OK) return rc;
    if (n_docs == 0) return RR_OK;
    std::lock_guard<std::mutex> lk(tp->mu);
    RR_HIP_TRY(hipSetDevice(tp->device));
    hipStream_t st = (hipStream_t)stream;
    RR_HIP_TRY(hipMemsetAsync(tp->d_bad + 1, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(rr_tp_head_check, dim3((unsigned)((n_docs + 255) / 256)), dim3(256), 0, st, text_bytes, d_text_off, d_doc_rows,
                       n_docs, n_src_docs, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int64_t*)nullptr, (int64_t)0,
                       tp->d_bad);
    hipLaunchKernelGGL(rr_tp_head<false>, dim3((unsigned)n_docs), dim3(RR_TP_THREADS), 0, st, d_text, d_text_off, d_doc_rows, max_chars,
                       normalize ? 1 : 0, min_chars, d_out_len, d_status, (const int64_t*)nullptr, (uint8_t*)nullptr,
                       (const int32_t*)tp->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

struct rr_tp_f_head_len {   // what the scan of the heads' offsets sums: the bytes of a surviving head
    const int32_t* len;
    const int32_t* status;
    __device__ __forceinline__ long long operator()(int64_t i) const { return status[i] == 0 && len[i] > 0 ? len[i] : 0; }
};

extern "C" int rr_textprep_head_offsets_dev(rr_textprep* tp, const int32_t* d_out_len, const int32_t* d_status, int32_t n_docs,
                                            int64_t* d_out_off, void* stream) {
    RR_REQUIRE(tp && d_out_len && d_status && d_out_off && n_docs >= 0, "rr_textprep_head_offsets_dev: NULL argument or %d documents",
               n_docs);
    std::lock_guard<std::mutex> lk(tp->mu);
    RR_HIP_TRY(hipSetDevice(tp->device));
    const int rc = rr_grow((void**)&tp->d_scratch, &tp->cap_words, 2 * rr_scan_sums_len(n_docs), sizeof(int32_t),
                           "rr_textprep_head_offsets_dev");
    if (rc != RR_OK) return rc;
    rr_scan(rr_tp_f_head_len{d_out_len, d_status}, (int64_t)n_docs, (int64_t*)tp->d_scratch, d_out_off, (int32_t*)nullptr,
            (int64_t*)nullptr, (hipStream_t)stream);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_textprep_head_write_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                          int32_t n_src_docs, const int32_t* d_doc_rows, int32_t n_docs, int32_t max_chars,
                                          int32_t normalize, int32_t min_chars, const int32_t* d_out_len, const int32_t* d_status,
                                          uint8_t* d_out_text, int64_t out_bytes, const int64_t* d_out_off, void* stream) {
    const int rc = rr_tp_head_args("rr_textprep_head_write_dev", tp, d_text, text_bytes, d_text_off, n_src_docs, n_docs, max_chars,
                                   min_chars, d_out_len, d_status);
    if (rc != RR_OK) return rc;
    RR_REQUIRE(d_out_off && out_bytes >= 0 && (d_out_text || out_bytes == 0), "rr_textprep_head_write_dev: NULL output with %lld bytes",
               (long long)out_bytes);
    if (n_docs == 0) return RR_OK;
    std::lock_guard<std::mutex> lk(tp->mu);
    RR_HIP_TRY(hipSetDevice(tp->device));
    hipStream_t st = (hipStream_t)stream;
    RR_HIP_TRY(hipMemsetAsync(tp->d_bad + 1, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(rr_tp_head_check, dim3((unsigned)((n_docs + 255) / 256)), dim3(256), 0, st, text_bytes, d_text_off, d_doc_rows,
                       n_docs, n_src_docs, d_out_len, d_status, d_out_off, out_bytes, tp->d_bad);
    hipLaunchKernelGGL(rr_tp_head<true>, dim3((unsigned)n_docs), dim3(RR_TP_THREADS), 0, st, d_text, d_text_off, d_doc_rows, max_chars,
                       normalize ? 1 : 0, min_chars, const_cast<int32_t*>(d_out_len), const_cast<int32_t*>(d_status), d_out_off,
                       d_out_text, (const int32_t*)tp->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_textprep_dedup_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                     const int32_t* d_len, const int32_t* d_group, int32_t* d_status, int32_t n_docs,
                                     int32_t hash_bits, void* stream) {
    RR_REQUIRE(tp && d_text_off && d_len && d_group && d_status, "rr_textprep_dedup_dev: NULL argument");
    RR_REQUIRE(n_docs >= 0 && n_docs <= (1 << 29), "rr_textprep_dedup_dev: %d documents outside [0, 2^29]", n_docs);
    RR_REQUIRE(d_text || text_bytes == 0, "rr_textprep_dedup_dev: NULL text with %lld bytes", (long long)text_bytes);
    RR_REQUIRE(text_bytes >= 0 && hash_bits >= 1 && hash_bits <= 64, "rr_textprep_dedup_dev: hash_bits %d outside [1, 64]", hash_bits);
    if (n_docs == 0) return RR_OK;
    int64_t slots = 64;
    while (slots < 2 * (int64_t)n_docs) slots <<= 1;
    std::lock_guard<std::mutex> lk(tp->mu);
    RR_HIP_TRY(hipSetDevice(tp->device));
    int rc = rr_grow((void**)&tp->d_scratch, &tp->cap_words, 2 * slots + n_docs, sizeof(int32_t), "rr_textprep_dedup_dev");
    if (rc != RR_OK) return rc;
    int32_t *rep = tp->d_scratch, *minimum = rep + slots, *slot_of = minimum + slots;
    hipStream_t st = (hipStream_t)stream;
    RR_HIP_TRY(hipMemsetAsync(rep, 0xFF, sizeof(int32_t) * (size_t)slots, st));          // -1 = empty
    RR_HIP_TRY(hipMemsetAsync(minimum, 0x7F, sizeof(int32_t) * (size_t)slots, st));      // above every document index
    hipLaunchKernelGGL(rr_tp_insert, dim3((unsigned)((n_docs + 3) / 4)), dim3(256), 0, st, d_text, text_bytes, d_text_off, d_len,
                       d_group, d_status, n_docs, hash_bits, (uint32_t)(slots - 1), rep, minimum, slot_of, tp->d_bad);
    hipLaunchKernelGGL(rr_tp_mark, dim3((unsigned)((n_docs + 255) / 256)), dim3(256), 0, st, slot_of, minimum, n_docs, d_status);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_textprep_compact_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                       const int32_t* d_len, const int32_t* d_status, int32_t n_docs, uint8_t* d_out_text,
                                       int64_t out_bytes, int64_t* d_out_off, int32_t* d_src_row, int64_t* d_count, void* stream) {
    RR_REQUIRE(tp && d_text_off && d_len && d_status && d_out_off && d_src_row && d_count, "rr_textprep_compact_dev: NULL argument");
    RR_REQUIRE(n_docs >= 0 && text_bytes >= 0 && out_bytes >= 0, "rr_textprep_compact_dev: %d documents, %lld / %lld bytes", n_docs,
               (long long)text_bytes, (long long)out_bytes);
    RR_REQUIRE((d_text && d_out_text) || text_bytes == 0 || out_bytes == 0, "rr_textprep_compact_dev: NULL text");
    std::lock_guard<std::mutex> lk(tp->mu);
    RR_HIP_TRY(hipSetDevice(tp->device));
    int rc = rr_grow((void**)&tp->d_scratch, &tp->cap_words, n_docs > 0 ? n_docs : 1, sizeof(int32_t), "rr_textprep_compact_dev");
    if (rc != RR_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rr_tp_rank, dim3(1), dim3(1024), 0, st, d_status, d_len, n_docs, tp->d_scratch, d_out_off, d_src_row, d_count);
    if (n_docs > 0 && d_text && d_out_text)
        hipLaunchKernelGGL(rr_tp_gather, dim3((unsigned)n_docs), dim3(256), 0, st, d_text, text_bytes, d_text_off, d_len,
                           tp->d_scratch, d_out_off, d_out_text, out_bytes, tp->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}
