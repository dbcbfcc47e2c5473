// rr_debug.h -- ablation (timing-only) and kernel-test harness of the scan kernels.  NOT part of the product ABI (include/rr_hip.h):
// compiled only with -DRR_DEBUG_HARNESS into librr_hip_dbg.so (build.py: build_library(debug=True)), which the
// tools/ scripts load through RR_DEBUG_HARNESS=1.  The ablated kernels leave garbage in the scan scratch and some of
// them give up the register-liveness contract of the asynchronous ring loads -- never part of a search.
#pragma once
#ifdef RR_DEBUG_HARNESS
#include "rr_common.h"
#include "rr_dense.h"
// The two sentinels rr_dense_x3w.hip shares with rr_dense_flt.hip, where they are defined (the same tokens) and explained.
#define RR_DEBUG_KEY_SENTINEL 0xFFC00001u
#define RR_DEBUG_SC_SENTINEL 0x7FC5A5A5u
// rr_dense_x3.hip: the 16-slot launches of rr_debug_x3_scan / rr_debug_x3_rescore (rr_dense_x3w.hip)
void rr_debug_x3_scan16(rr_index* ix, const float* d_q, int mode, rr_scan_geom* G, hipStream_t st);
void rr_debug_x3_rescore16(rr_index* ix, const float* d_q, int nq, hipStream_t st);
// rr_dense_flt.hip: the one-set launch rr_debug_fltw_words (rr_dense_fltw.hip) leaves for rr_debug_flt_select
void rr_debug_flt_note_state(rr_index* ix, const rr_scan_geom& G, int nq);
extern "C" {
// tests/test_gpu_fltw_kernels.py: rr_debug_flt_words / rr_debug_rescore_chain at a runtime width (fp32 storage, dim_pad 64 .. 1024
// other than 384): ONE rr_scan_fltw launch for one set of up to 64 queries -- geometry, eps, every word and key -- which
// rr_debug_flt_select and rr_debug_select_traces then work on; ONE rr_rescore_chain_w launch on caller lists.  See the definitions.
int rr_debug_fltw_words(rr_index* ix, const float* d_queries, int32_t nq, int32_t pool, int64_t* geom, float* eps, uint32_t* words,
                        int64_t words_cap, uint32_t* keys, int64_t keys_cap);
int rr_debug_fltw_rescore(rr_index* ix, const float* d_queries, int32_t nq, const uint32_t* mtiles, int64_t cap, const int32_t* count,
                          const int32_t* fb, float* sc);
// tools/x3w_ablate.py: variants of the 64-query fp32 split-operand scan (bit 0: no operand split, bit 1: no B-fragment
// reads, bit 2: no MFMA, bit 3: no lane swap)
int rr_debug_scan_x3w(rr_index* ix, int32_t variant, int32_t reps, float* out_ms);
// tools/flt_ablate.py: variants of the filter scans (the list is in rr_dense_flt.hip)
int rr_debug_scan_flt(rr_index* ix, int32_t variant, int32_t reps, float* out_ms);
// the hand-scheduled loop of rr_scan_fltq against its C++ bodies, tile word by tile word (out: 7 values, see the definition)
int rr_debug_fltq_compare(rr_index* ix, int64_t* out);
// tests/test_gpu_flt_words.py: ONE filter scan by itself (product preparation, product launch code) into a scratch filled
// with sentinels, and its raw output -- geometry, eps, sigma, every tile word and group key -- on the host; then the
// product's selection on those words; the path trace of every query of the last selection.  See the definitions.
int rr_debug_flt_words(rr_index* ix, const float* d_queries, int32_t nq_a, int32_t nq_b, int32_t scan, int32_t prefilter, int32_t pool,
                       int64_t* geom, float* eps, float* sigma, uint32_t* words, int64_t words_cap, uint32_t* keys, int64_t keys_cap);
int rr_debug_flt_select(rr_index* ix, int32_t pool, uint32_t* mtiles, int64_t cap, int32_t* count, uint32_t* tau, uint32_t* open,
                        int32_t* fb);
int rr_debug_select_traces(rr_index* ix, int32_t nq, int32_t* out);
// tests/test_gpu_fltq_prefilter.py: the two-set scan's prefiltered pair (launch A over the first groups, rr_fltq_sigma, launch B
// with thresholds and masks) through the product's launch code into sentinel-filled scratch -- geometry, eps, sigma, every
// word, key and mask; rr_debug_flt_select then runs the product's selection on what the pair left.  mlcap > 0: the LDS
// list of rr_select_mtiles' mask path holds only that many M-tiles from then on (0: the product's).  See the definitions.
int rr_debug_fltq_prefiltered(rr_index* ix, const float* d_queries, int32_t nq_a, int32_t nq_b, int32_t pool, int32_t flags,
                              uint32_t fill_word, int64_t* geom, float* eps, float* sigma, uint32_t* words, int64_t words_cap,
                              uint32_t* keys, int64_t keys_cap, uint64_t* masks, int64_t masks_cap);
int rr_debug_select_mlcap(int32_t mlcap);
// tests/test_gpu_rescore_kernels.py: ONE rr_rescore_chain / ONE rr_select_rescored launch (the product's launch helpers) on
// caller lists placed in the selection scratch, into outputs filled with sentinels.  mtiles [nq][cap], count / fb / tau (keys) /
// eps [nq]; sc [nq][cap][8] out of the rescoring, [nq][cap][rows_per_mtile] into the selection; rows / scores [nq][pool],
// fb_out / n_cand [nq].  Every argument is checked before anything is launched.  See the definitions.
int rr_debug_rescore_chain(rr_index* ix, const float* d_queries, int32_t nq, int32_t grid_x, int32_t use_plane, const uint32_t* mtiles,
                           int64_t cap, const int32_t* count, const int32_t* fb, const uint32_t* tau, const float* eps, float* sc);
int rr_debug_select_rescored(rr_index* ix, int32_t nq, int32_t pool, int32_t rows_per_mtile, int32_t floor_mode, const uint32_t* mtiles,
                             int64_t cap, const int32_t* count, const int32_t* fb, const uint32_t* tau, const float* sc, int64_t* rows,
                             float* scores, int32_t* fb_out, int32_t* n_cand);
// tests/test_gpu_select_kernels.py: ONE rr_select / rr_group_kth / rr_select_mtiles launch (rr_dense.hip) on CALLER levels --
// scores, tile or M-tile maxima, group keys made on the host for any geometry (tests/select_model.py) -- placed in the
// index's scan scratch, through the launch helpers the product calls (rr_launch_select, rr_launch_select_listed,
// rr_launch_group_kth, rr_launch_select_mtiles), into outputs filled with sentinels and copied back whole.  None of them
// reads a matrix: an index created without one will do.  Every argument and every size is checked against the scratch
// before anything is copied or launched.
//   rr_debug_select: n_tiles = ceil(n_rows / 64), n_pad = 64 n_tiles, n_waves = ceil(n_tiles / tiles_per_wave) <=
//     RR_MAX_SCAN_WAVES; qs 0 | 16 | 32 | 64 and the levels in the layout rr_scan_geom::qs documents, S slots of them (S = qs,
//     or nq when qs = 0).  form 0: nq queries, no flags; 1: flags[nq] as `only_if`; 2: the sliced launch, qs = 64, `slices`
//     2..4 blocks of levels (the entry puts block y at rr_select_slice_strides), nq = the call's queries (it ends inside the
//     last slice), flags[nq]; 3: the listed launch, qlist[1 + RR_SEL_LISTED] = count + the listed queries of a call of nq,
//     RR_SEL_LISTED slots of levels (qs = 0) or qs of them, flags[nq] the call's flags.  rows / score_bits [nq][pool],
//     trace [nq][16], flags_out [nq] (forms 1..3: the flags after the launch).  Trace words 11..13 of a query that took
//     rr_select_slow: tiles listed (n_tiles when it took all), n_cand before step 3b, whether step 3b ran; word 14 of a
//     query the fast path served: 1 = the rank sort ordered its candidates, 2 = the bitonic sort.
//   rr_debug_group_kth: keys [set][n_waves gpw][qs] (qs > 0: the only layout the kernel reads), eps [RR_SEL_MAXQ] with set
//     1's entries at RR_FLT_MAXQ, the product's set stride (rr_flt_smax_set_stride); bound_bits [nq_a + nq_b].
//   rr_debug_select_mtiles: ONE set, no sigma, mm_pairs 0 ([tile][qs][4]) or 1 ([32-row tile][qs][2]) with plain float
//     maxima (mm_pairs 3, the filter scan's words, stays with rr_debug_flt_select), keys [n_waves gpw][qs]; eps [nq] and
//     floor [nq] each NULL or given.  The threshold and floor code is shared by all three forms, which is why it is tested
//     here, on plain maxima -- but `eps` with plain maxima is a combination the PRODUCT never launches (its split-operand
//     scans pass no eps, its filter scan passes words).  mtiles [nq][RR_X3_MCAP], count / tau / fb [nq], trace [nq][16]
//     (word 6 = `open`).
int rr_debug_select(rr_index* ix, int64_t n_rows, int64_t tiles_per_wave, int32_t qs, int32_t nq, int32_t pool, int32_t form, int32_t slices,
                    const float* sims, const float* gmax, const uint32_t* smax, const int32_t* flags, const int32_t* qlist, int64_t* rows,
                    uint32_t* score_bits, int32_t* trace, int32_t* flags_out);
int rr_debug_group_kth(rr_index* ix, int32_t n_waves, int32_t gpw, int32_t qs, int32_t kth, int32_t nq_a, int32_t nq_b, const uint32_t* keys,
                       const float* eps, uint32_t* bound_bits);
int rr_debug_select_mtiles(rr_index* ix, int64_t n_rows, int64_t tiles_per_wave, int32_t gpw, int64_t tiles_per_group, int32_t qs,
                           int32_t mm_pairs, int32_t nq, int32_t pool, const float* mmax, const uint32_t* keys, const float* eps,
                           const float* floor, uint32_t* mtiles, int32_t* count, uint32_t* tau, int32_t* fb, int32_t* trace);
// tests/test_gpu_x3_scan_kernels.py: ONE split-operand scan launch (rr_scan_mfma_x3 / rr_scan_x3w, routed by nq as the product
// routes; mode 0 normal scan, 1 stored pass, 2 stored pass as the fallback launches it: flags + in-kernel query split) into
// scratch filled with sentinels, and its raw words on the host; ONE rescoring launch (rr_rescore_x3 / rr_rescore_x3w) on
// caller lists of 16-row M-tiles.  Both go through the launch helpers the product calls.  See the definitions (rr_dense_x3w.hip).
int rr_debug_x3_scan(rr_index* ix, const float* d_queries, int32_t nq, int32_t mode, const int32_t* flags, int64_t* geom,
                     uint32_t* sims, int64_t sims_cap, uint32_t* gmax, int64_t gmax_cap, uint32_t* smax, int64_t smax_cap,
                     unsigned short* planes);
int rr_debug_x3_rescore(rr_index* ix, const float* d_queries, int32_t nq, const uint32_t* mtiles, int64_t cap, const int32_t* count,
                        const int32_t* fb, float* sc);
// tests/test_gpu_valu_scan_kernels.py: ONE VALU scan launch -- the per-row fmaf chain every other dense path is held against --
// on the index's own matrix, and its raw levels on the host.  The routing is the product's: fp32 rows at 384 rr_scan_f32<6, NB>,
// at another width rr_scan_f32_generic<NB>; bf16 rows rr_scan_bf16<NB> / rr_scan_bf16_generic<NB>.  form 0 (plain): nq = 1..8
// queries, NB = 1 / 2 / 4 / 8 as rr_dense_chunk chooses it (rr_valu_nb), flags NULL, skip 0.
// form 1 (listed): nq = the call's queries (1..RR_SEL_MAXQ), flags[nq] (host), the launch of rr_dense_listed_fallback (fp32 384,
// skip 0) or of one pair of rr_dense_listed_fallback_wide (another width, either dtype: the flagged queries ranked [skip,
// skip + 8)); a bf16 index of width 384 has no listed form.  d_queries: device, nq x dim, unpadded, as rr_dense_topk_dev takes
// them: they go through rr_pad_queries into ix->d_q (slots past nq zero); the scratch comes from rr_ensure_scratch(ix, 8); the
// launch goes through rr_launch_scan_f32, rr_launch_scan_bf16, rr_launch_scan_bf16w (the product's own), rr_launch_scan_listed,
// rr_launch_scan_generic_listed or rr_launch_scan_bf16w_listed.  Before the launch the score scratch and the tile maxima are
// filled whole with RR_DEBUG_SC_SENTINEL, the group keys and the 16 words of the flagged list with RR_DEBUG_KEY_SENTINEL;
// afterwards the first sims_cap / gmax_cap / smax_cap words come back as they are (no more than the buffers hold: geom[7..9])
// and list_out[1 + RR_SEL_LISTED] (form 0: optional, and still the sentinel).  No selection is launched.  geom[10]: n_rows, n_tiles, n_pad, tiles_per_wave,
// n_waves, NB, kernel (rr_scan_note's 1 = fp32 rows, 2 = bf16 rows; + 10 at a runtime width; + 100 listed), words of the score
// scratch, of the tile-maxima buffer, of the key buffer.  Every argument and size is checked before anything is copied or
// launched: a bad one gives RR_E_INVALID.
int rr_debug_valu_scan(rr_index* ix, const float* d_queries, int32_t nq, int32_t form, const int32_t* flags, int32_t skip, int64_t* geom,
                       uint32_t* sims, int64_t sims_cap, uint32_t* gmax, int64_t gmax_cap, uint32_t* smax, int64_t smax_cap,
                       int32_t* list_out);
// tools/k5_stamps.py: in-kernel phase clocks of the last ce_ffn_fused launch (rr_ce.hip)
int rr_debug_ce_ffn_stamps(unsigned long long* out20);
// tools/k5_h2_stamps.py: phase clocks of one workgroup of the last FFN1 ce_gemm_h2 launch (rr_ce_h2.hip)
int rr_debug_ce_h2_stamps(unsigned long long* out16);
// tests/test_gpu_k5.py: one ce_gemm_h2 product on caller data (pack -> GEMM -> fp32), see the definition
int rr_debug_ce_h2_gemm(int32_t epi, int32_t M, int32_t N, int32_t K, const float* d_x, const float* d_w, const float* d_bias, int32_t qcols,
                        float* d_out, int32_t* flag_out);
// tests/test_gpu_k5_h2_kernels.py: the fp32 mode's attention (pack -> ce_attention_h2 / _small -> fp32) and add-LayerNorm (fp32
// rows + the unpacked h2 image) by themselves, see the definitions
int rr_debug_ce_h2_attention(const float* d_qkv, int32_t n_tokens, const int32_t* d_cu, int32_t n_seqs, int32_t max_len, int32_t cls_only,
                             int32_t kernel, float* d_ctx, int32_t* flag_out);
int rr_debug_ce_h2_add_ln(const float* d_y, const float* d_h, int32_t T, const float* d_g, const float* d_b, float eps, float* d_out32,
                          float* d_outh2, int32_t* flag_out);
// tests/test_gpu_k5_x3_kernels.py: the wide-range kernels of rr_ce.hip (ce_gemm_x3, ce_attention_x3, ce_add_ln_f32) one launch
// at a time on caller data, launched as ce_forward_x3 launches them.  The attention takes qkv [T][1152] with Q unscaled and
// writes ctx [T][384]; the add-LayerNorm updates d_h in place.  See the definitions.
int rr_debug_ce_x3_gemm(int32_t gelu, int32_t M, int32_t N, int32_t K, const float* d_x, const float* d_w, const float* d_bias, float* d_out);
int rr_debug_ce_x3_attention(const float* d_qkv, int32_t T, const int32_t* d_cu, int32_t n_seqs, float* d_ctx);
int rr_debug_ce_x3_add_ln(const float* d_y, float* d_h, int32_t T, const float* d_g, const float* d_b, float eps);
// tests/test_gpu_k5_bf16_kernels.py: the bf16 path's kernels of rr_ce.hip (ce_embed_ln, ce_proj_ts, ce_attention, ce_ffn_fused) one
// launch at a time on caller data, through the launch helpers of ce_forward_bf16 and with the weights of a handle created in
// RR_CE_PRECISION_BF16 (`layer` picks the layer).  bf16 rows are bit patterns: hb / ctx [T][384], qkv [T][1152] (Q unscaled).
// The attention writes ctx [T][384], or -- d_ctx_cls non-NULL -- only ctx_cls [n_seqs][384]; the FFN updates d_h32 in place and
// writes d_hb.  See the definitions.
int rr_debug_ce_embed_ln(rr_ce* ce, const int32_t* d_tok, const int32_t* d_typ, const int32_t* d_pos, int32_t T, float* d_h32,
                         unsigned short* d_hb);
int rr_debug_ce_bf16_proj(rr_ce* ce, int32_t layer, const unsigned short* d_hb, int32_t T, unsigned short* d_qkv);
int rr_debug_ce_bf16_attention(const unsigned short* d_qkv, int32_t T, const int32_t* d_cu, int32_t n_seqs, int32_t max_len,
                               unsigned short* d_ctx, unsigned short* d_ctx_cls);
int rr_debug_ce_bf16_ffn(rr_ce* ce, int32_t layer, const unsigned short* d_ctx, float* d_h32, unsigned short* d_hb, int32_t M);
// tests/test_gpu_k5_wide_kernels.py: the runtime-shape kernels of rr_ce_w.hip (ce_attention_x3w, ce_add_ln_w, ce_embed_ln_w) one
// launch at a time on caller data, through the launchers ce_forward_w calls.  The attention takes qkv [T][3 hidden] with Q
// unscaled and writes ctx [T][hidden] (hidden % 128 == 0 in [128, 1024], hidden / n_heads 32 or 64); the add-LayerNorm updates
// d_h in place; the embedding LayerNorm takes the tables of a handle of either precision and any shape and writes
// h32 [T][hidden].  See the definitions.
int rr_debug_ce_w_attention(const float* d_qkv, int32_t T, const int32_t* d_cu, int32_t n_seqs, int32_t hidden, int32_t n_heads, float* d_ctx);
int rr_debug_ce_w_add_ln(const float* d_y, float* d_h, int32_t T, int32_t hidden, const float* d_g, const float* d_b, float eps);
int rr_debug_ce_w_embed_ln(rr_ce* ce, const int32_t* d_tok, const int32_t* d_typ, const int32_t* d_pos, int32_t T, float* d_h32);
// tests/test_gpu_k5_pool_kernel.py: ONE ce_pool_mean launch (rr_ce_pool.hip: RR_CE_OUT_MEAN's kernel) on caller rows h32 [T][hidden]
// and cu_seqlens [n_seqs + 1] (device pointers), through the launcher the forward passes call: out [n_seqs][hidden].  A host
// copy of cu is checked before anything is launched -- it runs from 0 to T, every length is in [1, 512] -- and hidden is a
// multiple of 128 in [128, 1024]: RR_E_INVALID otherwise.  tools/pooling_time.py: rr_debug_ce_pool_time, the same launch and a
// device-to-device copy of the same rows under HIP events (ms_pool / ms_copy [reps]).  See the definitions.
int rr_debug_ce_pool_mean(const float* d_h32, int32_t T, const int32_t* d_cu, int32_t n_seqs, int32_t hidden, float* d_out);
int rr_debug_ce_pool_time(const float* d_h32, int32_t T, const int32_t* d_cu, int32_t n_seqs, int32_t hidden, float* d_out, float* d_copy,
                          int32_t warmup, int32_t reps, float* ms_pool, float* ms_copy);
}
#endif
