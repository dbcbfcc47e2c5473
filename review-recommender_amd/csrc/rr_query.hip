// rr_query.hip -- the query text of a batch on the device: BM25 term ids, gate groups and reranker query ids, written in the
// layouts their consumers already read (rr_bm25_scores_at_dev, rr_gate_factors_dev, rr_pairs_*_dev) (gfx950).
//
// Stands in for what SearchEngine.run_search_batch does per query in Python: text.tokenize_query + BM25Index.term_ids,
// text.build_gate_groups + gate.pack_groups, tokenizer.text_ids + rerank.pack_queries.  querytext.model_front states in
// plain Python what the kernels compute.
//
// INPUT.  The UTF-8 bytes of the B queries back to back with B + 1 int64 offsets, the layout rr_wp_encode_dev reads: one
// staged buffer per batch serves both.
//
// THE IMAGE.  A wave per query (a workgroup of 64 threads), queries of up to QF_MAX_QUERY bytes; lane l holds byte k * 64 + l
// of step k, so a ballot over a step is a 64-bit word of a bit mask in text order.  The raw bytes become the gate plane's
// image of the query (rr_gate.hip: A-Z -> a-z, C4 B0 -> 69 B0, E2 84 AA -> 6B with its two tails dropped): an ASCII string
// occurs in it exactly when it occurs in query.lower().  The colour groups are substring matches against that image.
//
// THE TOKENS are those of [a-z0-9]+(?:'[a-z0-9]+)? over the image with every other byte (NUL and every byte >= 0x80
// included) a separator -- the byte rules of rr_doctok.hip, with the query-time stop list, one-byte tokens kept and no cap.
// From the masks A (alnum) and Q (apostrophe): J = the apostrophes with an alnum on both sides; a stretch = a maximal piece of
// A | J; the j-th J of a stretch joins its neighbours when j is even (greedy, left to right: a'b'c -> a'b, c).  The parity
// comes from a prefix xor of J and the parity at the stretch's first byte, smeared over the stretch by the carry of an
// addition (inside + start bits); token bytes T = A | joining J, a token = a maximal run of T.  One lane does the 16 words.
//   - a token's owner is the lane that holds its first byte: length from T, stop list by its packed bytes, ordinal among the
//     kept tokens by popcounts, vocabulary id by the open-addressing table (hash first, then the bytes);
//   - the gate groups: colours present (substring), then per kept token its SYNONYMS group when it is a key, else {token}
//     when it has min_keyword_len bytes; duplicates by set equality go (static groups by their canonical index, a keyword that
//     equals a singleton static group becomes that group), the first max_groups stay.
// The kernel does no floating point: the factor table stays the host's.
//
// TWO LAUNCHES.  qf_front<false> writes per query its counts (ids, terms, term bytes, reranker ids) and its needs_host flags;
// qf_front<true> runs the same walk, sums the counts of the queries in front of it by itself (B is small) and writes.  A
// flagged query writes nothing but its (empty) offsets.  qf_strip takes [CLS] / [SEP] off what rr_wp_encode_dev made of the
// same bytes.  Every store is checked against its capacity first.
//
// THE VECTORS.  qv_normalize turns the query encoder's CLS rows into the unit vectors K1 reads, with numpy's float32
// roundings bit for bit (the only floating point of this file; see its own comment below); qv_flag joins the flags of the
// encoder's WordPiece pass to needs_host.
#include <vector>

#include "rr_prims.h"

#define QF_THREADS 64
#define QF_MAX_QUERY 1024                          // bytes of a query the kernel holds
#define QF_WORDS (QF_MAX_QUERY / 64)
#define QF_MAX_TOKEN 64                            // bytes of a token (= the gate's longest term)
#define QF_MAX_GROUPS 6                            // text.MAX_GATE_GROUPS; the factor table has QF_MAX_GROUPS + 1 entries
#define QF_MAX_STOP 8                              // bytes of a stop word (packed in one 64-bit word)
#define QF_GATE_TERMS 64                           // rr_gate_limits: terms and term bytes per query
#define QF_GATE_BYTES 1024
#define QF_MAX_STATIC 64                           // static groups (colours + synonyms), colours at most 32

#define QF_FLAG_QUERY 1                            // needs_host bits: the query is longer than QF_MAX_QUERY bytes,
#define QF_FLAG_TOKEN 2                            // a token is longer than QF_MAX_TOKEN bytes,
#define QF_FLAG_RERANK 4                           // more than max_length - 3 reranker ids,
#define QF_FLAG_WP 8                               // the WordPiece kernel handed the query back,
#define QF_FLAG_SPAN 16                            // the offsets decrease or leave the text (counted by rr_query_status)

struct qf_tables {       // the per-index tables on the device
    const rr_tab_entry* table;  // the BM25 vocabulary (rr_prims.h: the vocabulary table), key = length in bytes
    uint32_t mask;       // slots - 1
    const uint8_t* vbytes;
    const uint64_t* stop;       // stop words, packed little endian
    const uint8_t* tbytes;      // static groups: term bytes, term offsets [terms + 1], group -> first term [groups + 1],
    const int32_t* toff;
    const int32_t* goff;
    const int32_t* canon;       // group -> the first group with the same terms
    const int32_t* single;      // group -> its only term when it has one and is canonical, else -1
    const uint8_t* kbytes;      // the synonym groups' keys
    const int32_t* koff;
    int32_t n_stop, n_colors, n_syn, max_groups, min_keyword;
};

struct rr_query {
    int device = 0;
    qf_tables t = {};
    int32_t* d_bad = nullptr;           // [0] queries whose offsets were refused, [1] stores a capacity refused
    void* d_mem[9] = {};
    std::mutex mu;
};

static inline bool qf_token_byte(uint8_t c) { return (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '\''; }

// The table on the host: every entry a device-tokenised query token can equal (1 .. QF_MAX_TOKEN bytes of [a-z0-9']).
// Returns the entries kept, or -1 when n_slots is too small.
static int64_t qf_fill_table(const uint8_t* bytes, const int64_t* off, int32_t n_entries, int32_t n_slots, rr_tab_entry* slots) {
    return rr_tab_fill(bytes, off, n_entries, n_slots, slots, [=](int64_t a, int64_t b, int64_t* first, int32_t* key) {
        if (b - a < 1 || b - a > QF_MAX_TOKEN) return false;
        for (int64_t i = a; i < b; ++i)
            if (!qf_token_byte(bytes[i])) return false;
        *first = a;
        *key = (int32_t)(b - a);
        return true;
    });
}

// ------------------------------------------------------------------------------------------------ device helpers
__device__ __forceinline__ bool qf_same(const uint8_t* a, const uint8_t* b, int m) {
    int j = 0;
    while (j < m && a[j] == b[j]) ++j;
    return j == m;
}

__device__ static int32_t qf_lookup(const qf_tables& tb, const uint8_t* p, int m) {
    uint32_t h = 0;
    for (int j = 0; j < m; ++j) h = h * RR_TAB_BASE + p[j];
    return rr_tab_lookup(tb.table, tb.mask, tb.vbytes, h, m, m, p);
}

// The synonym group whose key the token is, or -1.
__device__ static int qf_key_of(const qf_tables& tb, const uint8_t* p, int m) {
    for (int j = 0; j < tb.n_syn; ++j) {
        const int o = tb.koff[j];
        if (tb.koff[j + 1] - o == m && qf_same(tb.kbytes + o, p, m)) return j;
    }
    return -1;
}

// The canonical static group that is exactly {token}, or -1.
__device__ static int qf_single_of(const qf_tables& tb, const uint8_t* p, int m) {
    for (int g = 0; g < tb.n_colors + tb.n_syn; ++g) {
        const int t = tb.single[g];
        if (t < 0) continue;
        const int o = tb.toff[t];
        if (tb.toff[t + 1] - o == m && qf_same(tb.tbytes + o, p, m)) return g;
    }
    return -1;
}

// Length of the run of T that starts at bit `bit` of word k (a run of more than 64 bytes answers some length above 64).
__device__ __forceinline__ int qf_run(const uint64_t* T, int k, int bit) {
    const uint64_t v = ~(T[k] >> bit);
    int m = v ? __builtin_ctzll(v) : 64;
    if (m == 64 - bit) {
        const uint64_t v2 = ~T[k + 1];
        m += v2 ? __builtin_ctzll(v2) : 64;
    }
    return m;
}

__device__ __forceinline__ int qf_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ the front end
template <bool WRITE>
__global__ __launch_bounds__(QF_THREADS) void qf_front(
    const uint8_t* __restrict__ text, int64_t text_bytes, const int64_t* __restrict__ text_off, int32_t n_queries,
    const int32_t* __restrict__ wp_cu, const int32_t* __restrict__ wp_needs, int32_t avail, qf_tables tb,
    int32_t* __restrict__ counts, int32_t* __restrict__ needs_host, int32_t* __restrict__ ids, int32_t* __restrict__ ids_off,
    int64_t cap_ids, int32_t* __restrict__ term_off, int32_t* __restrict__ term_group, int32_t* __restrict__ q_term,
    int32_t* __restrict__ q_groups, uint8_t* __restrict__ term_bytes, int64_t cap_terms, int64_t cap_tbytes,
    int32_t* __restrict__ bad) {
    __shared__ uint8_t s_raw[QF_MAX_QUERY];
    __shared__ uint8_t s_img[QF_MAX_QUERY];
    __shared__ uint64_t s_A[QF_WORDS + 1], s_Q[QF_WORDS + 1], s_T[QF_WORDS + 1], s_G[QF_WORDS];
    const int lane = threadIdx.x, q = blockIdx.x;
    const uint64_t below = (1ull << lane) - 1ull;

    const int64_t a = text_off[q], b = text_off[q + 1];
    int flags = 0, n_rr = 0;
    int64_t id_base = 0, term_base = 0, tb_base = 0;
    if (WRITE) {
        flags = needs_host[q];
        int s0 = 0, s1 = 0, s2 = 0;
        for (int i = lane; i < q; i += QF_THREADS) {
            s0 += counts[4 * i];
            s1 += counts[4 * i + 1];
            s2 += counts[4 * i + 2];
        }
        id_base = qf_wave_sum(s0);
        term_base = qf_wave_sum(s1);
        tb_base = qf_wave_sum(s2);
    } else {
        if (!(a >= 0 && b >= a && b <= text_bytes)) {              // nothing of it is read
            flags |= QF_FLAG_SPAN;
            if (lane == 0) atomicAdd(bad, 1);
        } else if (b - a > QF_MAX_QUERY) {
            flags |= QF_FLAG_QUERY;
        }
        if (wp_cu) {
            if (wp_needs[q]) {
                flags |= QF_FLAG_WP;
            } else {
                n_rr = wp_cu[q + 1] - wp_cu[q] - 2;                // without [CLS] and [SEP]
                n_rr = n_rr < 0 ? 0 : n_rr;
                if (n_rr > avail) flags |= QF_FLAG_RERANK;
            }
        }
    }

    int n_ids = 0, n_groups = 0, n_terms = 0, n_tbytes = 0;
    int sel_a[QF_MAX_GROUPS], sel_m[QF_MAX_GROUPS];                 // a group: static (m = 0, a = its index) or {token} (a = first byte, m = length)
#pragma unroll
    for (int g = 0; g < QF_MAX_GROUPS; ++g) sel_a[g] = sel_m[g] = 0;

    const bool walk = WRITE ? flags == 0 : !(flags & (QF_FLAG_SPAN | QF_FLAG_QUERY));     // (the same in every lane)
    if (walk) {
        // ---- the image
        const int len = (int)(b - a);
        const int raw_words = (len + 63) >> 6;
        for (int k = 0; k < raw_words; ++k) {
            const int i = k * 64 + lane;
            s_raw[i] = i < len ? text[a + i] : (uint8_t)0;
        }
        __syncthreads();
        int n = 0;
        for (int k = 0; k < raw_words; ++k) {
            const int i = k * 64 + lane;
            const bool in = i < len;
            uint8_t c = in ? s_raw[i] : (uint8_t)0;
            bool dr = false;
            if (in) {
                if (c >= 'A' && c <= 'Z') c += 32;
                else if (c == 0xC4) { if (i + 1 < len && s_raw[i + 1] == 0xB0) c = 'i'; }
                else if (c == 0xE2) { if (i + 2 < len && s_raw[i + 1] == 0x84 && s_raw[i + 2] == 0xAA) c = 'k'; }
                else if (c == 0x84) dr = i >= 1 && i + 1 < len && s_raw[i - 1] == 0xE2 && s_raw[i + 1] == 0xAA;
                else if (c == 0xAA) dr = i >= 2 && s_raw[i - 2] == 0xE2 && s_raw[i - 1] == 0x84;
            }
            const bool kept = in && !dr;
            const uint64_t kb = __ballot(kept);
            if (kept) s_img[n + __popcll(kb & below)] = c;
            n += __popcll(kb);
        }
        __syncthreads();
        const int words = (n + 63) >> 6;

        // ---- the token bytes
        for (int k = 0; k < words; ++k) {
            const int i = k * 64 + lane;
            const uint8_t c = i < n ? s_img[i] : (uint8_t)' ';
            const uint64_t A = __ballot((c >= 'a' && c <= 'z') || (c >= '0' && c <= '9'));
            const uint64_t Q = __ballot(c == '\'');
            if (lane == 0) { s_A[k] = A; s_Q[k] = Q; }
        }
        if (lane == 0) s_A[words] = s_Q[words] = 0;
        __syncthreads();
        if (lane == 0) {
            uint64_t prev_a = 0, prev_in = 0, odd = 0, carry = 0;
            for (int k = 0; k < words; ++k) {
                const uint64_t A = s_A[k];
                const uint64_t J = s_Q[k] & ((A << 1) | (prev_a >> 63)) & ((A >> 1) | (s_A[k + 1] << 63));
                const uint64_t in = A | J;
                const uint64_t start = in & ~((in << 1) | (prev_in >> 63));
                uint64_t x = J;                                     // bit i: the parity of the J in [0, i] of this word
                x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
                const uint64_t par = (x << 1) ^ odd;                // bit i: the parity of the J in front of byte i of the query
                odd ^= (x >> 63) ? ~0ull : 0ull;
                const uint64_t t1 = in + (start & par), t2 = t1 + carry;       // the carry clears the stretches that start odd
                carry = (t1 < in || t2 < t1) ? 1 : 0;
                const uint64_t fill = in & ~t2;                     // bit i: the parity at the first byte of i's stretch
                s_T[k] = A | (J & ~(par ^ fill));
                prev_a = A;
                prev_in = in;
            }
            s_T[words] = 0;
        }
        __syncthreads();

        // ---- the tokens: stop list, ordinals, vocabulary ids, group candidates
        bool too_long = false;
        for (int k = 0; k < words; ++k) {
            const int i = k * 64 + lane;
            const uint64_t Tw = s_T[k];
            const bool before = lane ? ((Tw >> (lane - 1)) & 1) : (k ? (s_T[k - 1] >> 63) : 0);
            const bool first = ((Tw >> lane) & 1) && !before;
            int m = 0;
            bool keep = false, cand = false;
            if (first) {
                m = qf_run(s_T, k, lane);
                if (m > QF_MAX_TOKEN) {
                    too_long = true;
                } else {
                    keep = true;
                    if (m <= QF_MAX_STOP) {
                        uint64_t w = 0;
                        for (int j = 0; j < m; ++j) w |= (uint64_t)s_img[i + j] << (8 * j);
                        for (int s = 0; s < tb.n_stop; ++s) keep = keep && tb.stop[s] != w;
                    }
                    cand = keep && (m >= tb.min_keyword || qf_key_of(tb, s_img + i, m) >= 0);
                }
            }
            const uint64_t K = __ballot(keep), G = __ballot(cand);
            if (WRITE && keep) {
                const int64_t o = id_base + n_ids + __popcll(K & below);
                if (o < cap_ids) ids[o] = qf_lookup(tb, s_img + i, m);
                else atomicAdd(bad + 1, 1);
            }
            if (lane == 0) s_G[k] = G;
            n_ids += __popcll(K);
        }
        if (__ballot(too_long)) flags |= QF_FLAG_TOKEN;
        __syncthreads();

        if (!(flags & QF_FLAG_TOKEN)) {
            // ---- the colour groups: a substring of the image
            for (int c = 0; c < tb.n_colors && n_groups < tb.max_groups; ++c) {
                bool hit = false;
                for (int t = tb.goff[c]; t < tb.goff[c + 1] && !hit; ++t) {
                    const int o = tb.toff[t], m = tb.toff[t + 1] - o;
                    bool f = false;
                    for (int k = 0; k < words; ++k) {
                        const int i = k * 64 + lane;
                        if (i + m <= n && s_img[i] == tb.tbytes[o]) f = f || qf_same(s_img + i, tb.tbytes + o, m);
                    }
                    hit = __ballot(f) != 0;
                }
                if (!hit) continue;
                const int sid = tb.canon[c];
                bool dup = false;
#pragma unroll
                for (int g = 0; g < QF_MAX_GROUPS; ++g) dup = dup || (g < n_groups && sel_m[g] == 0 && sel_a[g] == sid);
                if (dup) continue;
#pragma unroll
                for (int g = 0; g < QF_MAX_GROUPS; ++g)
                    if (g == n_groups) { sel_a[g] = sid; sel_m[g] = 0; }
                ++n_groups;
            }
            // ---- the tokens' groups, in text order (every lane walks the same bits)
            for (int k = 0; k < words && n_groups < tb.max_groups; ++k) {
                uint64_t G = s_G[k];
                while (G && n_groups < tb.max_groups) {
                    const int bit = __builtin_ctzll(G);
                    G &= G - 1;
                    const int at = k * 64 + bit, m = qf_run(s_T, k, bit);
                    const int key = qf_key_of(tb, s_img + at, m);
                    int sid = key >= 0 ? tb.canon[tb.n_colors + key] : qf_single_of(tb, s_img + at, m);
                    bool dup = false;
#pragma unroll
                    for (int g = 0; g < QF_MAX_GROUPS; ++g) {
                        if (g >= n_groups) continue;
                        if (sid >= 0) dup = dup || (sel_m[g] == 0 && sel_a[g] == sid);
                        else dup = dup || (sel_m[g] == m && qf_same(s_img + sel_a[g], s_img + at, m));
                    }
                    if (dup) continue;
#pragma unroll
                    for (int g = 0; g < QF_MAX_GROUPS; ++g)
                        if (g == n_groups) { sel_a[g] = sid >= 0 ? sid : at; sel_m[g] = sid >= 0 ? 0 : m; }
                    ++n_groups;
                }
            }
            // ---- the terms
#pragma unroll
            for (int g = 0; g < QF_MAX_GROUPS; ++g) {
                if (g >= n_groups) continue;
                const bool fixed = sel_m[g] == 0;
                const int t0 = fixed ? tb.goff[sel_a[g]] : 0, t1 = fixed ? tb.goff[sel_a[g] + 1] : 1;
                for (int t = t0; t < t1; ++t) {
                    const int o = fixed ? tb.toff[t] : sel_a[g], m = fixed ? tb.toff[t + 1] - o : sel_m[g];
                    if (WRITE) {
                        const int64_t out = term_base + n_terms, at = tb_base + n_tbytes;
                        if (out < cap_terms && at + m <= cap_tbytes) {
                            if (lane == 0) { term_off[out] = (int32_t)at; term_group[out] = g; }
                            if (lane < m) term_bytes[at + lane] = fixed ? tb.tbytes[o + lane] : s_img[o + lane];
                        } else if (lane == 0) {
                            atomicAdd(bad + 1, 1);
                        }
                    }
                    ++n_terms;
                    n_tbytes += m;
                }
            }
        }
    }

    if (!WRITE) {
        if (flags) n_ids = n_terms = n_tbytes = n_rr = 0;          // a flagged query gets no ids, no groups and no reranker ids
        if (lane == 0) {
            counts[4 * q] = n_ids;
            counts[4 * q + 1] = n_terms;
            counts[4 * q + 2] = n_tbytes;
            counts[4 * q + 3] = n_rr;
            needs_host[q] = flags;
        }
    } else if (lane == 0) {
        if (flags) n_ids = n_terms = n_tbytes = n_groups = 0;
        ids_off[q] = (int32_t)id_base;
        q_term[q] = (int32_t)term_base;
        q_groups[q] = n_groups;
        if (term_base + n_terms <= cap_terms) term_off[term_base + n_terms] = (int32_t)(tb_base + n_tbytes);
        if (q == n_queries - 1) {
            ids_off[n_queries] = (int32_t)(id_base + n_ids);
            q_term[n_queries] = (int32_t)(term_base + n_terms);
        }
    }
}

// The reranker's query ids: what rr_wp_encode_dev made of the same bytes ([CLS] pieces [SEP] per query), without the two
// specials, back to back; a flagged query has none (its count is 0).
__global__ __launch_bounds__(QF_THREADS) void qf_strip(const int32_t* __restrict__ wp_tok, const int32_t* __restrict__ wp_cu,
                                                       int64_t wp_cap, int32_t n_queries, const int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ rr_off, int32_t* __restrict__ rr_ids, int64_t cap_rr,
                                                       int32_t* __restrict__ bad) {
    const int lane = threadIdx.x, q = blockIdx.x;
    int s = 0;
    for (int i = lane; i < q; i += QF_THREADS) s += counts[4 * i + 3];
    const int64_t base = qf_wave_sum(s);
    const int n = counts[4 * q + 3];
    const int64_t src = (int64_t)wp_cu[q] + 1;
    for (int j = lane; j < n; j += QF_THREADS) {
        if (base + j < cap_rr && src >= 1 && src + j < wp_cap) rr_ids[base + j] = wp_tok[src + j];
        else atomicAdd(bad + 1, 1);
    }
    if (lane == 0) {
        rr_off[q] = (int32_t)base;
        if (q == n_queries - 1) rr_off[n_queries] = (int32_t)(base + n);
    }
}

// ------------------------------------------------------------------------------------------------ the query vectors
// The encoder's CLS rows to the unit vectors K1 reads, with the roundings of numpy's float32
//   e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), eps)
// bit for bit (querytext.model_query_vectors states them in plain Python; include/rr_hip.h lists them).  A wave per query:
//   1. lane 0 walks numpy's pairwise split of `dim` terms (a piece of more than 128 is cut at n/2 - (n/2) % 8) and lists the
//      pieces left to right with their depth: at most 128 pieces, seven splits deep, for dim <= 8192;
//   2. eight lanes per piece carry its eight accumulators (lane j adds the squares j, j + 8, ... of the piece in order), three
//      cross-lane adds make ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)) -- float addition commutes, so every lane of the eight holds
//      that value -- and lane 0 of the eight adds the piece's tail of n % 8 squares.  Eight pieces per pass: dim 384 is four
//      pieces of 96 on 32 lanes, one pass;
//   3. lane 0 folds the pieces' sums in the order of the splits (two neighbours of one depth are the halves of one split:
//      left + right, one level up), takes the square root and numpy's maximum with eps; every lane divides its elements.
// No FMA may form between a square and the addition that takes it: the build passes -ffp-contract=off, and the pragma below
// holds the kernel to it whatever the flags say.  sqrtf and the quotient are HIP's correctly rounded defaults; float32
// denormals are kept (the default for gfx9 compute kernels).  The row is read in full before anything is written, so it may
// be normalised in place.
#define QV_BLOCK 128                               // numpy's PW_BLOCKSIZE
#define QV_MAX_DIM 8192                            // rr_index_create's widest row
#define QV_MAX_LEAVES 128                          // a piece of a split has at least 64 terms
#define QV_MAX_DEPTH 16                            // (seven splits for dim <= 8192)

__global__ __launch_bounds__(QF_THREADS) void qv_normalize(const float* rows, int32_t dim, float eps, const int32_t* needs_host,
                                                           float* out) {
#pragma clang fp contract(off)
    __shared__ int32_t leaf_first[QV_MAX_LEAVES + 1];
    __shared__ int32_t leaf_depth[QV_MAX_LEAVES];
    __shared__ float leaf_sum[QV_MAX_LEAVES];
    __shared__ int32_t st_n[QV_MAX_DEPTH], st_d[QV_MAX_DEPTH];
    __shared__ float st_s[QV_MAX_DEPTH];
    __shared__ int32_t n_leaves;
    __shared__ float denom;
    const int lane = threadIdx.x, q = blockIdx.x;
    const float* row = rows + (int64_t)q * dim;
    float* dst = out + (int64_t)q * dim;
    if (needs_host && needs_host[q] != 0) {        // (the whole wave: K1 runs on a defined vector, the caller replaces the answer)
        for (int i = lane; i < dim; i += QF_THREADS) dst[i] = 0.f;
        return;
    }
    if (lane == 0) {
        int sp = 0, nl = 0, first = 0, m = dim, d = 0;
        for (;;) {
            while (m > QV_BLOCK) {                 // the right half waits on the stack
                int n2 = m / 2;
                n2 -= n2 % 8;
                ++d;
                st_n[sp] = m - n2; st_d[sp] = d; ++sp;
                m = n2;
            }
            leaf_first[nl] = first; leaf_depth[nl] = d; ++nl;
            first += m;
            if (sp == 0) break;
            --sp;
            m = st_n[sp]; d = st_d[sp];
        }
        leaf_first[nl] = first;
        n_leaves = nl;
    }
    __syncthreads();
    const int nl = n_leaves, j = lane & 7;
    for (int l = lane >> 3; l < nl; l += QF_THREADS / 8) {
        const int first = leaf_first[l], m = leaf_first[l + 1] - first;
        const float* a = row + first;
        float r = 0.f, x;
        if (m < 8) {                               // (dim < 8 only: one piece, summed in order from 0)
            if (j == 0)
                for (int i = 0; i < m; ++i) { x = a[i]; x = x * x; r = r + x; }
        } else {
            const int body = m - (m & 7);
            x = a[j]; r = x * x;
            for (int i = 8; i < body; i += 8) { x = a[i + j]; x = x * x; r = r + x; }
            r = r + __shfl_xor(r, 1);
            r = r + __shfl_xor(r, 2);
            r = r + __shfl_xor(r, 4);
            if (j == 0)
                for (int i = body; i < m; ++i) { x = a[i]; x = x * x; r = r + x; }
        }
        if (j == 0) leaf_sum[l] = r;
    }
    __syncthreads();
    if (lane == 0) {
        int sp = 0;
        for (int l = 0; l < nl; ++l) {
            float s = leaf_sum[l];
            int d = leaf_depth[l];
            while (sp > 0 && st_d[sp - 1] == d) { --sp; s = st_s[sp] + s; --d; }
            st_s[sp] = s; st_d[sp] = d; ++sp;
        }
        const float norm = sqrtf(st_s[0]);
        denom = (norm > eps || norm != norm) ? norm : eps;       // numpy's maximum: a NaN norm stays (fmaxf would drop it)
    }
    __syncthreads();
    const float den = denom;
    for (int i = lane; i < dim; i += QF_THREADS) dst[i] = row[i] / den;
}

extern "C" int rr_query_vectors_dev(const float* d_rows, int32_t n_queries, int32_t dim, float eps, const int32_t* d_needs_host,
                                    float* d_out, void* stream) {
    RR_REQUIRE(n_queries >= 0 && n_queries <= 65535, "rr_query_vectors_dev: %d queries outside [0, 65535]", n_queries);
    RR_REQUIRE(dim >= 1 && dim <= QV_MAX_DIM, "rr_query_vectors_dev: dim %d outside [1, %d]", dim, QV_MAX_DIM);
    RR_REQUIRE(d_rows && d_out, "rr_query_vectors_dev: NULL argument");
    RR_REQUIRE(eps == eps, "rr_query_vectors_dev: eps is NaN");
    if (n_queries == 0) return RR_OK;
    hipLaunchKernelGGL(qv_normalize, dim3((unsigned)n_queries), dim3(QF_THREADS), 0, (hipStream_t)stream, d_rows, dim, eps,
                       d_needs_host, d_out);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

// needs_host[q] |= bit where src[q] != 0: the flags of the query encoder's WordPiece pass join the front's.
__global__ __launch_bounds__(QF_THREADS) void qv_flag(const int32_t* __restrict__ src, int32_t n, int32_t bit,
                                                      int32_t* __restrict__ needs_host) {
    const int q = blockIdx.x * QF_THREADS + threadIdx.x;
    if (q < n && src[q] != 0) needs_host[q] |= bit;
}

extern "C" int rr_query_flag_dev(const int32_t* d_src, int32_t n_queries, int32_t bit, int32_t* d_needs_host, void* stream) {
    RR_REQUIRE(n_queries >= 0 && n_queries <= 65535, "rr_query_flag_dev: %d queries outside [0, 65535]", n_queries);
    RR_REQUIRE(d_src && d_needs_host, "rr_query_flag_dev: NULL argument");
    RR_REQUIRE(bit >= 1 && bit <= (1 << 30) && (bit & (bit - 1)) == 0, "rr_query_flag_dev: %d is not one bit of 1 .. 2^30", bit);
    if (n_queries == 0) return RR_OK;
    hipLaunchKernelGGL(qv_flag, dim3((unsigned)((n_queries + QF_THREADS - 1) / QF_THREADS)), dim3(QF_THREADS), 0,
                       (hipStream_t)stream, d_src, n_queries, bit, d_needs_host);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int rr_query_limits(int32_t* out_max_query, int32_t* out_max_token, int32_t* out_max_groups, int32_t* out_max_stop) {
    RR_REQUIRE(out_max_query && out_max_token && out_max_groups && out_max_stop, "rr_query_limits: NULL argument");
    *out_max_query = QF_MAX_QUERY; *out_max_token = QF_MAX_TOKEN; *out_max_groups = QF_MAX_GROUPS; *out_max_stop = QF_MAX_STOP;
    return RR_OK;
}

extern "C" int rr_query_table_slots(int32_t n_entries, int32_t* out_slots) {
    RR_REQUIRE(out_slots && n_entries >= 0 && n_entries <= (1 << 28), "rr_query_table_slots: %d entries outside [0, 2^28]", n_entries);
    *out_slots = rr_tab_slots_for(n_entries);
    return RR_OK;
}

static int qf_check_vocab(const char* who, const uint8_t* bytes, const int64_t* off, int32_t n_entries) {
    RR_REQUIRE(off && (bytes || n_entries == 0 || off[n_entries] == 0), "%s: NULL argument", who);
    RR_REQUIRE(n_entries >= 0 && n_entries <= (1 << 28), "%s: %d entries outside [0, 2^28]", who, n_entries);
    RR_REQUIRE(off[0] == 0, "%s: entry offsets must start at 0", who);
    for (int32_t p = 0; p < n_entries; ++p)
        RR_REQUIRE(off[p + 1] >= off[p], "%s: entry offsets decrease at entry %d", who, p);
    RR_REQUIRE(off[n_entries] < (1ll << 31), "%s: %lld vocabulary bytes (limit 2^31)", who, (long long)off[n_entries]);
    return RR_OK;
}

extern "C" int rr_query_build_table(const uint8_t* h_bytes, const int64_t* h_off, int32_t n_entries, int32_t n_slots,
                                    int32_t* h_slots, int32_t* out_kept) {
    int rc = qf_check_vocab("rr_query_build_table", h_bytes, h_off, n_entries);
    if (rc) return rc;
    RR_REQUIRE(h_slots && out_kept, "rr_query_build_table: NULL output");
    RR_REQUIRE(n_slots == rr_tab_slots_for(n_entries), "rr_query_build_table: n_slots %d, rr_query_table_slots says %d", n_slots,
               rr_tab_slots_for(n_entries));
    const int64_t kept = qf_fill_table(h_bytes, h_off, n_entries, n_slots, reinterpret_cast<rr_tab_entry*>(h_slots));
    RR_REQUIRE(kept >= 0, "rr_query_build_table: table overflow");
    *out_kept = (int32_t)kept;
    return RR_OK;
}

extern "C" int rr_query_destroy(rr_query* h) {
    if (!h) return RR_OK;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    hipFree(h->d_bad);
    for (void* p : h->d_mem) hipFree(p);
    delete h;
    return RR_OK;
}

// A list of n strings (bytes + int32 offsets): non-empty ASCII without NUL, at most max_len bytes each.
static int qf_check_strings(const char* what, const uint8_t* bytes, const int32_t* off, int32_t n, int32_t max_len) {
    RR_REQUIRE(off && off[0] == 0 && (bytes || n == 0), "rr_query_create: NULL or misplaced %s", what);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t m = off[i + 1] - off[i];
        RR_REQUIRE(m >= 1 && m <= max_len, "rr_query_create: %s %d has %d bytes (1 .. %d)", what, i, m, max_len);
        for (int32_t j = off[i]; j < off[i + 1]; ++j)
            RR_REQUIRE(bytes[j] >= 1 && bytes[j] < 0x80, "rr_query_create: %s %d is not ASCII", what, i);
    }
    return RR_OK;
}

extern "C" int rr_query_create(int32_t device, const uint8_t* h_vocab_bytes, const int64_t* h_vocab_off, int32_t n_vocab,
                               const uint8_t* h_stop_bytes, const int32_t* h_stop_off, int32_t n_stop, const uint8_t* h_term_bytes,
                               const int32_t* h_term_off, const int32_t* h_group_off, int32_t n_colors, int32_t n_syn,
                               const uint8_t* h_key_bytes, const int32_t* h_key_off, int32_t max_groups, int32_t min_keyword_len,
                               rr_query** out) {
    RR_REQUIRE(out, "rr_query_create: NULL out");
    *out = nullptr;
    int rc = qf_check_vocab("rr_query_create", h_vocab_bytes, h_vocab_off, n_vocab);
    if (rc) return rc;
    RR_REQUIRE(n_stop >= 0 && n_stop <= 1024 && n_colors >= 0 && n_colors <= 32 && n_syn >= 0 && n_colors + n_syn <= QF_MAX_STATIC,
               "rr_query_create: %d stop words, %d colour groups, %d synonym groups", n_stop, n_colors, n_syn);
    RR_REQUIRE(max_groups >= 1 && max_groups <= QF_MAX_GROUPS && min_keyword_len >= 1,
               "rr_query_create: max_groups %d outside [1, %d] or min_keyword_len %d < 1", max_groups, QF_MAX_GROUPS, min_keyword_len);
    const int32_t n_static = n_colors + n_syn;
    RR_REQUIRE(h_group_off && h_group_off[0] == 0, "rr_query_create: NULL or misplaced group offsets");
    for (int32_t g = 0; g < n_static; ++g)
        RR_REQUIRE(h_group_off[g + 1] > h_group_off[g], "rr_query_create: static group %d has no terms", g);
    const int32_t n_terms = h_group_off[n_static];
    if ((rc = qf_check_strings("stop word", h_stop_bytes, h_stop_off, n_stop, QF_MAX_STOP))) return rc;
    if ((rc = qf_check_strings("gate term", h_term_bytes, h_term_off, n_terms, QF_MAX_TOKEN))) return rc;
    if ((rc = qf_check_strings("synonym key", h_key_bytes, h_key_off, n_syn, QF_MAX_TOKEN))) return rc;
    auto term = [&](int32_t t) { return std::string((const char*)h_term_bytes + h_term_off[t], (size_t)(h_term_off[t + 1] - h_term_off[t])); };
    std::vector<int32_t> canon_mem((size_t)n_static + 1), single_mem((size_t)n_static + 1);
    int32_t* canon = canon_mem.data();
    int32_t* single = single_mem.data();
    for (int32_t g = 0; g < n_static; ++g) {
        const int32_t t0 = h_group_off[g], t1 = h_group_off[g + 1];
        // no unflagged query may reach a limit of rr_gate_limits: max_groups groups of these sizes, or of one token each
        RR_REQUIRE((t1 - t0) * max_groups <= QF_GATE_TERMS, "rr_query_create: static group %d has %d terms: %d such groups exceed "
                   "the gate's %d terms per query", g, t1 - t0, max_groups, QF_GATE_TERMS);
        RR_REQUIRE((h_term_off[t1] - h_term_off[t0]) * max_groups <= QF_GATE_BYTES, "rr_query_create: static group %d has %d term "
                   "bytes: %d such groups exceed the gate's %d per query", g, h_term_off[t1] - h_term_off[t0], max_groups, QF_GATE_BYTES);
        for (int32_t t = t0 + 1; t < t1; ++t)
            RR_REQUIRE(term(t - 1) < term(t), "rr_query_create: the terms of static group %d are not sorted and distinct", g);
        canon[g] = g;
        for (int32_t f = 0; f < g && canon[g] == g; ++f) {
            bool same = h_group_off[f + 1] - h_group_off[f] == t1 - t0;
            for (int32_t t = 0; same && t < t1 - t0; ++t) same = term(h_group_off[f] + t) == term(t0 + t);
            if (same) canon[g] = f;
        }
        single[g] = (t1 - t0 == 1 && canon[g] == g) ? t0 : -1;
    }
    RR_REQUIRE(max_groups * QF_MAX_TOKEN <= QF_GATE_BYTES, "rr_query_create: %d keyword groups exceed the gate's term bytes", max_groups);

    const int32_t n_slots = rr_tab_slots_for(n_vocab);
    std::vector<rr_tab_entry> slot_mem((size_t)n_slots);
    const int64_t kept = qf_fill_table(h_vocab_bytes, h_vocab_off, n_vocab, n_slots, slot_mem.data());
    RR_REQUIRE(kept >= 0, "rr_query_create: table overflow");
    std::vector<uint64_t> stop_mem((size_t)n_stop + 1);
    for (int32_t s = 0; s < n_stop; ++s) {
        uint64_t w = 0;
        for (int32_t j = h_stop_off[s]; j < h_stop_off[s + 1]; ++j) w |= (uint64_t)h_stop_bytes[j] << (8 * (j - h_stop_off[s]));
        stop_mem[s] = w;
    }

    RR_HIP_TRY(hipSetDevice(device));
    rr_query* h = new rr_query();
    h->device = device;
    hipError_t e = hipMalloc((void**)&h->d_bad, 8);
    if (e == hipSuccess) e = hipMemset(h->d_bad, 0, 8);
    int slot = 0;
    auto up = [&](const void* src, size_t bytes) -> const void* {  // (at least one byte: no table pointer is NULL)
        void* d = nullptr;
        if (e == hipSuccess) e = hipMalloc(&d, bytes ? bytes : 1);
        if (e == hipSuccess && bytes) e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        h->d_mem[slot++] = d;
        return d;
    };
    qf_tables& t = h->t;
    t.table = (const rr_tab_entry*)up(slot_mem.data(), slot_mem.size() * sizeof(rr_tab_entry));
    t.mask = (uint32_t)(n_slots - 1);
    t.vbytes = (const uint8_t*)up(h_vocab_bytes, (size_t)h_vocab_off[n_vocab]);
    t.stop = (const uint64_t*)up(stop_mem.data(), (size_t)n_stop * 8);
    t.tbytes = (const uint8_t*)up(h_term_bytes, (size_t)h_term_off[n_terms]);
    t.toff = (const int32_t*)up(h_term_off, (size_t)(n_terms + 1) * 4);
    t.goff = (const int32_t*)up(h_group_off, (size_t)(n_static + 1) * 4);
    t.canon = (const int32_t*)up(canon, (size_t)n_static * 4);
    t.single = (const int32_t*)up(single, (size_t)n_static * 4);
    // the keys' bytes and offsets share one block: [offsets int32 (n_syn + 1)] [bytes]
    std::vector<uint8_t> key_mem((size_t)(n_syn + 1) * 4 + (size_t)h_key_off[n_syn]);
    memcpy(key_mem.data(), h_key_off, (size_t)(n_syn + 1) * 4);
    if (h_key_off[n_syn]) memcpy(key_mem.data() + (size_t)(n_syn + 1) * 4, h_key_bytes, (size_t)h_key_off[n_syn]);
    const uint8_t* d_keys = (const uint8_t*)up(key_mem.data(), key_mem.size());
    t.koff = (const int32_t*)d_keys;
    t.kbytes = d_keys ? d_keys + (size_t)(n_syn + 1) * 4 : nullptr;
    t.n_stop = n_stop; t.n_colors = n_colors; t.n_syn = n_syn; t.max_groups = max_groups; t.min_keyword = min_keyword_len;
    if (e != hipSuccess) {
        rr_set_error("rr_query_create: %s", hipGetErrorString(e));
        rr_query_destroy(h);
        return RR_E_HIP;
    }
    *out = h;
    return RR_OK;
}

extern "C" int rr_query_front_dev(rr_query* h, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                  int32_t n_queries, const int32_t* d_wp_cu, const int32_t* d_wp_needs_host, int32_t max_length,
                                  int32_t* d_counts, int32_t* d_needs_host, int32_t* d_ids, int32_t* d_ids_off, int64_t cap_ids,
                                  int32_t* d_term_off, int32_t* d_term_group, int32_t* d_q_term, int32_t* d_q_groups,
                                  uint8_t* d_term_bytes, int64_t cap_terms, int64_t cap_term_bytes, void* stream) {
    RR_REQUIRE(h && d_text_off && d_counts && d_needs_host && d_ids && d_ids_off && d_term_off && d_term_group && d_q_term &&
               d_q_groups && d_term_bytes, "rr_query_front_dev: NULL argument");
    RR_REQUIRE(d_text || text_bytes == 0, "rr_query_front_dev: NULL text with %lld bytes", (long long)text_bytes);
    RR_REQUIRE(n_queries >= 1 && n_queries <= 65535, "rr_query_front_dev: %d queries outside [1, 65535]", n_queries);
    RR_REQUIRE(text_bytes >= 0 && text_bytes < (1ll << 31), "rr_query_front_dev: %lld text bytes in one call (limit 2^31)",
               (long long)text_bytes);
    RR_REQUIRE(cap_ids >= 0 && cap_terms >= 0 && cap_term_bytes >= 0, "rr_query_front_dev: a negative capacity");
    RR_REQUIRE((d_wp_cu == nullptr) == (d_wp_needs_host == nullptr), "rr_query_front_dev: pass both WordPiece arrays or neither");
    RR_REQUIRE(!d_wp_cu || max_length >= 3, "rr_query_front_dev: max_length %d leaves no room for [CLS] [SEP] [SEP]", max_length);
    std::lock_guard<std::mutex> lk(h->mu);
    RR_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(qf_front<false>, dim3((unsigned)n_queries), dim3(QF_THREADS), 0, st, d_text, text_bytes, d_text_off,
                       n_queries, d_wp_cu, d_wp_needs_host, max_length - 3, h->t, d_counts, d_needs_host, d_ids, d_ids_off, cap_ids,
                       d_term_off, d_term_group, d_q_term, d_q_groups, d_term_bytes, cap_terms, cap_term_bytes, h->d_bad);
    hipLaunchKernelGGL(qf_front<true>, dim3((unsigned)n_queries), dim3(QF_THREADS), 0, st, d_text, text_bytes, d_text_off,
                       n_queries, d_wp_cu, d_wp_needs_host, max_length - 3, h->t, d_counts, d_needs_host, d_ids, d_ids_off, cap_ids,
                       d_term_off, d_term_group, d_q_term, d_q_groups, d_term_bytes, cap_terms, cap_term_bytes, h->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_query_strip_dev(rr_query* h, const int32_t* d_wp_tok, const int32_t* d_wp_cu, int64_t wp_capacity,
                                  int32_t n_queries, const int32_t* d_counts, int32_t* d_rr_off, int32_t* d_rr_ids, int64_t cap_rr,
                                  void* stream) {
    RR_REQUIRE(h && d_wp_tok && d_wp_cu && d_counts && d_rr_off && d_rr_ids, "rr_query_strip_dev: NULL argument");
    RR_REQUIRE(n_queries >= 1 && n_queries <= 65535, "rr_query_strip_dev: %d queries outside [1, 65535]", n_queries);
    RR_REQUIRE(wp_capacity >= 0 && cap_rr >= 0, "rr_query_strip_dev: a negative capacity");
    std::lock_guard<std::mutex> lk(h->mu);
    RR_HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(qf_strip, dim3((unsigned)n_queries), dim3(QF_THREADS), 0, (hipStream_t)stream, d_wp_tok, d_wp_cu, wp_capacity,
                       n_queries, d_counts, d_rr_off, d_rr_ids, cap_rr, h->d_bad);
    RR_HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_query_status(rr_query* h, int32_t* out_bad) {
    RR_REQUIRE(h && out_bad, "rr_query_status: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    RR_HIP_TRY(hipSetDevice(h->device));
    int32_t bad[2] = {0, 0};
    RR_HIP_TRY(hipDeviceSynchronize());
    RR_HIP_TRY(hipMemcpy(bad, h->d_bad, 8, hipMemcpyDeviceToHost));
    RR_HIP_TRY(hipMemset(h->d_bad, 0, 8));
    *out_bad = bad[0] + bad[1];
    RR_REQUIRE(bad[0] == 0, "rr_query_front_dev: %d query(ies) had text offsets that decrease or leave the text (nothing of them "
               "was read; they are flagged)", bad[0]);
    RR_REQUIRE(bad[1] == 0, "rr_query_front_dev / rr_query_strip_dev: %d store(s) did not fit the capacities given (they were "
               "not made)", bad[1]);
    return RR_OK;
}
