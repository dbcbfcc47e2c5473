/*
 * rr_hip.h -- C ABI of librr_hip.so, the MI355X (gfx950) hybrid-retrieval hot path.
 *
 * The reference (Ntropy86/review-recommender) is pure Python and has no FFI of
 * its own; its boundary for this path is a set of Python callables (SURVEY.md
 * section 8b).  Each entry point below names the reference callable it stands
 * in for.  A Python front-end binds these with ctypes (INTEGRATION.md shows
 * the stub); the product wrapper is review-recommender_amd/_lib.py.
 *
 * Conventions
 *   - every function returns 0 on success, a negative RR_E_* code otherwise;
 *     rr_last_error() returns a thread-local message for the last failure;
 *   - the caller owns every host buffer (C-contiguous, sizes as documented);
 *     the library owns device memory behind opaque handles;
 *   - "h_" parameters are host pointers, "d_" parameters are device pointers
 *     on the handle's device (e.g. a torch tensor's data_ptr(), used by the
 *     multi-GPU exchange so RCCL can move the buffers without a host hop);
 *   - rows are int64 indices into the index's row space; a shard created with
 *     a row offset reports GLOBAL rows (local row + offset);
 *   - handles may be used from several host threads; calls on one handle are
 *     serialised by an internal mutex (Streamlit shares cached handles across
 *     session threads: app/app_product_search.py:53,71,119).
 *   - there is no CPU fallback anywhere behind this ABI.
 */
#ifndef RR_HIP_H
#define RR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_OK            0
#define RR_E_INVALID    -1   /* bad argument (shape, NULL, range) */
#define RR_E_HIP        -2   /* a HIP runtime call failed */
#define RR_E_NOMEM      -3
#define RR_E_STATE      -4   /* handle not ready for this call (e.g. meta not set) */

#define RR_DTYPE_F32     0
#define RR_DTYPE_BF16    1   /* storage only (dim 1 .. 1024): queries, products and accumulation stay fp32 */

#define RR_MAX_POOL   2048   /* upper bound for pool / k */
#define RR_MAX_BATCH  1024
#define RR_MAX_QTERMS   64   /* query tokens the BM25 candidate kernel stages per pass (longer queries take several passes) */

typedef struct rr_index rr_index;   /* dense matrix + per-row metadata of one shard */
typedef struct rr_bm25  rr_bm25;    /* BM25 postings (CSR by term) + forward CSR by doc */

const char* rr_last_error(void);
int rr_version(void);
int rr_device_count(int* out);

/* ------------------------------------------------------------------ index */

/* Device-resident copy of product_emb.npy (nlp/11_build_product_embeddings.py:82-85):
 * n_rows x dim, row-major.  h_matrix may be NULL (fill later with
 * rr_index_upload_rows / rr_index_adopt_device).  row_offset is added to every
 * row this shard reports.  dim is padded internally to a multiple of 64.
 * Widths: RR_DTYPE_F32 takes dim 1 .. 8192, RR_DTYPE_BF16 dim 1 .. 1024 (2 bytes per element and no filter plane beside the
 * rows: a third of what an fp32 index of the same rows takes once it has searched a batch).  A padded width of 384 is served
 * by the 384-wide kernels; every other padded width up to 1024 by the runtime-width ones (csrc/rr_dense_bf16w.hip,
 * csrc/rr_dense_fltw.hip), with the same contract: a query's answer is the exact top-pool of its per-row-chain scores,
 * bitwise the same alone, in any batch and on any shard.  An adopted bf16 matrix is n_rows x dim_padded() bf16. */
int rr_index_create(const void* h_matrix, int64_t n_rows, int32_t dim, int32_t dtype,
                    int32_t device, int64_t row_offset, rr_index** out);
int rr_index_upload_rows(rr_index* ix, int64_t first_row, int64_t n_rows, const void* h_rows);
/* fp32 host rows into an index of either dtype: rows are optionally l2-normalised in fp32
 * (normalize_eps > 0: utils.py:40-44) and then stored; a bf16 index rounds them once, to nearest
 * even, AFTER the normalisation ("round V (RNE) to bf16 once"). */
int rr_index_upload_rows_f32(rr_index* ix, int64_t first_row, int64_t n_rows, const float* h_rows,
                             float normalize_eps);
/* Use a caller-owned device matrix (n_rows x dim_padded(), already padded) without copying.  The index keeps facts
 * derived from the matrix content (row-norm bounds of the filter scan, the bf16 filter plane): writes made through this
 * ABI invalidate them; after writing to an ADOPTED matrix yourself (e.g. an in-place torch update) call
 * rr_index_matrix_changed, or batched searches filter on the old rows. */
int rr_index_adopt_device(rr_index* ix, const void* d_matrix);
/* The device-source twin of rr_index_upload_rows_f32 (what nlp/11_build_product_embeddings.py:82-85 leaves in
 * product_emb.npy, without the file): d_rows [n][dim] fp32, unpadded, on the index's device.  The same kernels as the host
 * upload, so the same bits: optional x / max(||x||, eps) in fp32, a bf16 index rounds once afterwards, padding columns are
 * zero, the row-norm bounds and the bf16 filter plane are dropped; refused on an adopted matrix.
 * d_row_ids == NULL: rows [first_row, first_row + n), everything queued on `stream` behind whatever produces d_rows there.
 * The call takes the handle's mutex; the FIRST store into an index that has no matrix yet allocates it and waits for its
 * padding to be zeroed; after that there is no host wait.  A search on ANOTHER stream (rr_dense_topk uses the index's own)
 * must follow a synchronisation of `stream`.
 * d_row_ids != NULL (device, n LOCAL row numbers; first_row is ignored): row i goes to row d_row_ids[i] -- a builder's second
 * pass drops late rows into their places.  This form allocates a staging copy, waits for `stream` and reports ids outside
 * the index as RR_E_INVALID (those rows are skipped). */
int rr_index_store_rows_dev(rr_index* ix, const float* d_rows, int64_t n, int64_t first_row, const int64_t* d_row_ids,
                            float normalize_eps, void* stream);
/* Rows [first_row, first_row + n) of an fp32 index back to the host, unpadded (waits for the device). */
int rr_index_download_rows_f32(rr_index* ix, int64_t first_row, int64_t n, float* h_rows);
/* The same rows into DEVICE memory ([n][dim] fp32, unpadded), queued on `stream`: order it behind the stores yourself. */
int rr_index_copy_rows_dev(rr_index* ix, int64_t first_row, int64_t n, float* d_rows, void* stream);
int rr_index_matrix_changed(rr_index* ix);
int rr_index_dim_padded(const rr_index* ix, int32_t* out);
/* l2_normalize (utils.py:40-44) of every row, in place on the device. */
int rr_index_l2_normalize(rr_index* ix, float eps);
/* n_reviews / avg_stars of product_emb_meta.parquet (nlp/11...:86-90), row-aligned,
 * plus log1p(n_reviews) as numpy computes it (kept so the volume prior and trust
 * reproduce the reference bit for bit).  avg_stars may hold NaN. */
int rr_index_set_meta(rr_index* ix, const double* h_n_reviews, const double* h_avg_stars,
                      const double* h_log1p_n);
int rr_index_destroy(rr_index* ix);

/* ------------------------------------------------------------ K1 dense top-k */

/* cosine_similarity_search (utils.py:111-124; _cosine_pool app/app_product_search.py:192-195;
 * cosine_search app/test.py:125-132), batched: for each of n_queries query vectors
 * (n_queries x dim fp32, host) the top `pool` rows by dot product, ordered
 * (score desc, row asc); pool is clamped to n_rows like utils.py:116-117 and the
 * clamped value is written to *pool_out.  out_rows / out_scores: n_queries x pool. */
int rr_dense_topk(rr_index* ix, const float* h_queries, int32_t n_queries, int32_t pool,
                  int64_t* h_out_rows, float* h_out_scores, int32_t* pool_out);
/* Same with device-resident queries and outputs, asynchronous on `stream`
 * (a hipStream_t passed as void*; NULL = the device's default stream, which is what
 * torch.cuda.current_stream().cuda_stream is unless the caller switched streams). */
int rr_dense_topk_dev(rr_index* ix, const float* d_queries, int32_t n_queries, int32_t pool,
                      int64_t* d_out_rows, float* d_out_scores, void* stream);
/* Timing of the last dense scan kernel on this handle (HIP events, ms). */
int rr_index_last_scan_ms(rr_index* ix, float* out_ms);
/* Every scan launch is bracketed by a HIP event pair on its stream (ring of 512).
 * Drains the pairs recorded since the last call: total ms and launch count. */
int rr_index_scan_stats(rr_index* ix, double* out_total_ms, int64_t* out_launches);
/* Which scan kernel the last scan launch on this handle ran: out8[0] = 1 rr_scan_f32, 2 rr_scan_bf16,
 * 3 rr_scan_mfma_x3, 4 rr_scan_x3w, 5 the filter scans (rr_scan_flt over fp32 rows; over a bf16 stream rr_scan_flt16
 * and, for two query sets in one launch, rr_scan_fltq); 6 and 7 are retired (the removed f32-input MFMA scans); [1] = its template
 * variant (query tiles / query slots; filter scans: 9 = rr_scan_fltq; 16 = rr_scan_fltw, the runtime-width scan of an index of either dtype whose
 * padded width is 64 .. 1024 and not 384 (csrc/rr_dense_fltw.hip); 8 was the two-set rr_scan_flt16, no longer reported);
 * [2] = queries in that launch; [3] = bf16 MFMA terms per dimension
 * (0: not a bf16 matrix-core kernel); [4] = bytes per matrix element the scan streamed (2 = bf16 rows or the bf16
 * filter plane, 4 = fp32 rows).  bench.py names the roofline kernel and its algorithmic bytes from this. */
int rr_index_last_scan_info(rr_index* ix, int32_t* out8);
/* Path taken by the last top-pool selection for its first query: out16[0] = 2: M-tile maxima + rescoring
 * (the batched paths), 1: stored scores through the LDS-resident 3-level selection, 0: generic radix
 * fallback; [1..3] = groups opened, (M-)tiles opened, candidate rows; [4..] = shader-clock cycles of the
 * selection's phases (-1: unused).  Diagnostic: lets tests assert which path ran. */
int rr_index_select_trace(rr_index* ix, int32_t* out16);
/* Diagnostic switch of the batched (5..64 query) scan.  RR_SCAN_MODE_DEFAULT: the scan keeps only
 * M-tile maxima and the candidate M-tiles are rescored (select trace out16[0] == 2), with the
 * stored-score pass as per-query fallback.  RR_SCAN_MODE_STORED: always the single pass that
 * stores every score.  Both return identical rows and scores; tests compare them. */
/* The bf16 filter plane of an fp32 index (default on): the batched filter scan (5..128 queries per launch) streams a
 * once-rounded bf16 copy of the matrix (n_rows x 384 x 2 bytes of extra HBM, built lazily at the first batched search
 * and dropped by any write to the matrix) instead of the fp32 rows -- half the bytes per launch for the same approximate
 * scores and the same error bound -- and candidates are rescored on the fp32 rows exactly as before: identical answers.
 * enable = 0 frees the plane and scans the fp32 rows.  Environment RR_NO_SHADOW=1 does the same process-wide.
 * A bf16 index never has a plane, at any width (its rows are one): neither switch applies to it. */
int rr_index_set_shadow(rr_index* ix, int32_t enable);
#define RR_SCAN_MODE_DEFAULT 0
#define RR_SCAN_MODE_STORED 1
int rr_index_set_scan_mode(rr_index* ix, int32_t mode);

/* ------------------------------------------------------------ K2 BM25 */

/* BM25Okapi(corpus) of rank_bm25 as used at app/app_product_search.py:142 and
 * app/test.py:156, over integer term ids.  Inputs (host):
 *   post_indptr[n_terms+1], post_docs[nnz] (ascending per term), post_tf[nnz]
 *   doc_indptr[n_docs+1],  doc_terms[nnz] (ascending per doc),  doc_tf[nnz]
 *   doc_len[n_docs] (token count incl. duplicates), idf[n_terms] (float64, with
 *   the epsilon floor already applied), avgdl, k1, b.
 * doc ids are LOCAL rows of the shard; idf / avgdl are corpus-wide. */
int rr_bm25_create(int32_t device, int64_t n_docs, int64_t n_terms, int64_t nnz,
                   const int64_t* post_indptr, const int32_t* post_docs, const int32_t* post_tf,
                   const int64_t* doc_indptr, const int32_t* doc_terms, const int32_t* doc_tf,
                   const int32_t* doc_len, const double* idf, double avgdl, double k1, double b,
                   int64_t row_offset, rr_bm25** out);
/* Same, with every array already resident on `device` (caller-owned, not copied, must
 * outlive the handle): used when the corpus is built on the GPU. */
int rr_bm25_create_dev(int32_t device, int64_t n_docs, int64_t n_terms, int64_t nnz,
                       const int64_t* d_post_indptr, const int32_t* d_post_docs, const int32_t* d_post_tf,
                       const int64_t* d_doc_indptr, const int32_t* d_doc_terms, const int32_t* d_doc_tf,
                       const int32_t* d_doc_len, const double* d_idf, double avgdl, double k1, double b,
                       int64_t row_offset, rr_bm25** out);
int rr_bm25_destroy(rr_bm25* bm);
/* BM25Okapi.get_scores(tokens) (app/app_product_search.py:206): float64[n_docs],
 * tokens applied in order, duplicates counted again, ids < 0 = unknown token. */
int rr_bm25_get_scores(rr_bm25* bm, const int32_t* h_term_ids, int32_t n_terms_in_query,
                       double* h_out_scores);
/* _bm25_for_candidates (app/app_product_search.py:201-208) / bm25_scores (app/test.py:168-173)
 * without the N-long intermediate: BM25 of each query at its candidate rows only.
 *   h_term_ids[term_off[q] .. term_off[q+1]) are query q's token ids;
 *   rows: n_queries x pool GLOBAL rows (rows outside this shard score 0);
 *   out : n_queries x pool float32 (float64 accumulate, cast like np.float32).
 * mode 0 = forward CSR (doc -> terms), mode 1 = postings lists (binary search). */
int rr_bm25_scores_at(rr_bm25* bm, const int32_t* h_term_ids, const int32_t* h_term_off,
                      int32_t n_queries, const int64_t* h_rows, int32_t pool, int32_t mode,
                      float* h_out);
int rr_bm25_scores_at_dev(rr_bm25* bm, const int32_t* d_term_ids, const int32_t* d_term_off,
                          int32_t n_queries, const int64_t* d_rows, int32_t pool, int32_t mode,
                          float* d_out, void* stream);

/* BM25Okapi(corpus) built on the GPU (csrc/rr_bm25_build.hip) from a token-id stream instead of
 * host CSR arrays.  Input contract:
 *   tok[n_tok] int32 term ids in document order, each in [0, n_terms);
 *   doc_off[n_src+1] int64, monotone, doc_off[0] = 0, doc_off[n_src] = n_tok (document d is
 *   tok[doc_off[d] .. doc_off[d+1]), fewer than 2^31 tokens);
 *   order[n_order] (optional, NULL = the source documents in order): output row j is source
 *   document order[j], -1 = an empty document, duplicates allowed;
 *   [row_lo, row_hi): the output rows this handle holds (a shard), local row 0 = row_lo.
 * inputs_on_device = 1: tok / doc_off / order are device pointers on `device`; 0: host pointers.
 * stream: the caller's stream (NULL = the device's null stream).  The build runs on the handle's
 * own stream after everything queued on `stream` so far: inputs written by work queued there
 * (e.g. torch's current stream) are complete before they are read.  Work on OTHER streams must
 * be finished, or ordered before `stream`, by the caller.  The call returns when the build is done.
 * The inputs are checked on the device before any scatter: an id out of range, a decreasing
 * doc_off or an order entry out of [-1, n_src) returns RR_E_INVALID and creates no handle.
 * The handle owns its arrays (rr_bm25_destroy frees them).  It scores only after
 * rr_bm25_set_idf: df and the length sum are those of the whole SOURCE corpus (also for a
 * shard or a selection), and idf / avgdl are computed from them on the host. */
int rr_bm25_build(int32_t device, int32_t inputs_on_device, const int32_t* tok, int64_t n_tok,
                  const int64_t* doc_off, int64_t n_src, int64_t n_terms, const int64_t* order,
                  int64_t n_order, int64_t row_lo, int64_t row_hi, double k1, double b,
                  int64_t row_offset, void* stream, rr_bm25** out);
/* h_df[n_terms]: documents of the source corpus holding each term; h_sizes[5] = n_docs (rows
 * held), n_terms, nnz, n_src, sum of the source document lengths. */
int rr_bm25_build_stats(rr_bm25* bm, int64_t* h_df, int64_t* h_sizes);
/* idf[n_terms] (float64, epsilon floor applied) and avgdl of a built handle (avgdl may be 0 only
 * when the index holds no entry). */
int rr_bm25_set_idf(rr_bm25* bm, const double* h_idf, double avgdl);
/* Copies the CSR arrays out (sizes as for rr_bm25_create); any destination may be NULL (skipped),
 * a host buffer or a device buffer (blocking copies: a device buffer must have no work pending
 * on another stream). */
int rr_bm25_copy_csr(rr_bm25* bm, int64_t* doc_indptr, int32_t* doc_terms, int32_t* doc_tf,
                     int32_t* doc_len, int64_t* post_indptr, int32_t* post_docs, int32_t* post_tf);

/* ------------------------------------------------------------ K3 fuse + top-k */

/* Candidates K3 takes per query (rr_fuse_params.n_candidates).  A search over `world` row shards merges
 * world x pool of them, so world x pool <= 4096: 8 shards take a pool of at most 512
 * (ShardedSearcher refuses a larger one with ValueError before any launch or collective). */
#define RR_MAX_CANDIDATES 4096

typedef struct rr_fuse_params {
    double w_dense, w_bm25, w_rerank, w_prior, w_best;  /* run_search weights */
    double prior_C;          /* Bayesian prior strength (prior_C) */
    int32_t min_reviews;     /* trust ramp (min_reviews) */
    int32_t trust_sat;       /* 80 in the app (app/app_product_search.py:303) */
    int32_t apply_trust;     /* 1 = app flavour, 0 = CLI flavour (app/test.py:308) */
    int32_t rerank_active;   /* 1 when rerank_k > 0: _rerank column is float32 */
    int32_t rerank_k;        /* first rerank_k pool rows carry reranker scores */
    int32_t k;               /* rows to return */
    int32_t n_candidates;    /* candidates supplied per query (>= pool when merging shards) */
    int32_t pool;            /* pool size to cut the candidates to before fusing */
    int32_t cand_per_rank;   /* 0: candidate arrays are [query][n_candidates]; else the arrays are
                                gathered shard payloads [rank][query][cand_per_rank] */
    int32_t bm25_f64;        /* 1: the _bm25 column is the CLI's float64 zeros (`cand["_bm25"] = 0.0`, app/test.py:252:
                                no BM25 artefact): the blend is float64 from its second term on; d_bm25 must be NULL */
    int64_t cand_rank_stride_bytes; /* distance between two ranks' payload blocks */
} rr_fuse_params;

/* Everything run_search does after the candidate pool exists
 * (app/app_product_search.py:256-312; CLI app/test.py:250-309): cut the
 * n_candidates supplied per query to the best `pool` by (dense desc, row asc)
 * [the shard merge], min-max of dense / bm25 / prior / rerank / best, Bayesian
 * prior with the pool mean, volume prior, trust, weighted blend, gate, stable
 * sort by final desc, first k.
 * Candidate inputs, n_candidates per query (device pointers): rows, dense, bm25 raw
 * (NULL = zeros), n_reviews, avg_stars, log1p_n (all three NULL = gathered from `ix`
 * by row; required when merging shards).  Pool inputs, `pool` per query, aligned
 * with the pool order this call produces (so a caller that needs them first calls
 * with k = pool and reads out_rows): rerank raw, best raw (NULL = zeros), gate
 * (NULL = ones).
 * Outputs (device): out_rows[nq x pool] global rows in pool order;
 * out_cols[nq x 8 x pool] = _dense,_bm25,_prior,_rerank,_best,_gate,_trust,_final (float64);
 * out_order[nq x k] = pool positions of the top-k, best first. */
int rr_fuse_topk_dev(rr_index* ix, const rr_fuse_params* p, int32_t n_queries,
                     const int64_t* d_rows, const float* d_dense, const float* d_bm25,
                     const double* d_n_reviews, const double* d_avg_stars, const double* d_log1p_n,
                     const float* d_rerank, const float* d_best, const float* d_gate,
                     int64_t* d_out_rows, double* d_out_cols, int32_t* d_out_order, void* stream);
/* The same call with a CANDIDATE-aligned gate column that survives the merge: d_cand_gate holds one factor per candidate,
 * addressed exactly like d_dense -- [query][n_candidates] when cand_per_rank == 0, gathered blocks
 * [rank][query][cand_per_rank], cand_rank_stride_bytes apart, otherwise -- so a row shard can gate the candidates it owns
 * BEFORE the exchange and ship the factor in its payload (sharded.py): whichever branch of the merge places a candidate
 * (the binary-search merge of ordered lists, the bitonic sort of an unordered one), its factor is read through the same
 * slot map as its dense and BM25 scores, once, where the blend applies the gate.  No first pass is needed to learn the pool
 * order.  NULL = ones.  d_gate and d_cand_gate both non-NULL is RR_E_INVALID with nothing launched.
 * rr_fuse_topk_dev is this call with d_cand_gate = NULL. */
int rr_fuse_topk_cand_dev(rr_index* ix, const rr_fuse_params* p, int32_t n_queries,
                          const int64_t* d_rows, const float* d_dense, const float* d_bm25,
                          const double* d_n_reviews, const double* d_avg_stars, const double* d_log1p_n,
                          const float* d_rerank, const float* d_best, const float* d_gate, const float* d_cand_gate,
                          int64_t* d_out_rows, double* d_out_cols, int32_t* d_out_order, void* stream);
/* Host-buffer form of rr_fuse_topk_dev. */
int rr_fuse_topk(rr_index* ix, const rr_fuse_params* p, int32_t n_queries,
                 const int64_t* h_rows, const float* h_dense, const float* h_bm25,
                 const double* h_n_reviews, const double* h_avg_stars, const double* h_log1p_n,
                 const float* h_rerank, const float* h_best, const float* h_gate,
                 int64_t* h_out_rows, double* h_out_cols, int32_t* h_out_order);
/* Gather per-row metadata for candidate rows (payload of the shard exchange). */
int rr_index_gather_meta_dev(rr_index* ix, const int64_t* d_rows, int64_t n,
                             double* d_n_reviews, double* d_avg_stars, double* d_log1p_n,
                             void* stream);

/* Kernel-driven copies: ONE launch moves up to RR_COPY_MAX_SEGS pitched segments (rows x row_bytes, each side with its
 * own pitch) on `stream`.  Either side of a segment may be PINNED HOST memory that is mapped into the device's address
 * space (hipHostMalloc, torch's pin_memory(): the host pointer is valid on the device): a batch's inputs (token ids)
 * and its answer (rows / order / final scores: what the reference returns to its caller, app/app_product_search.py:312-317)
 * then cross PCIe as the loads / stores of one kernel instead of as one copy command each.  In the same way
 * rr_dense_topk_dev accepts mapped pinned host memory as `d_queries` (its first kernel reads the queries once).
 * Not a product path of its own: the data movement in front of K1 / behind K3. */
#define RR_COPY_MAX_SEGS 4
typedef struct rr_copy_seg {
    void* dst;
    const void* src;
    int64_t row_bytes, rows, dst_pitch, src_pitch;
} rr_copy_seg;
int rr_copy_segments_dev(const rr_copy_seg* segs, int32_t n_segs, int32_t device, void* stream);

/* ------------------------------------------------------------ best review per candidate */

typedef struct rr_reviews rr_reviews;
/* Review embeddings of reviews_with_embeddings.parquet (n_reviews x dim fp32, l2-normalised on the
 * device when normalize_eps > 0 like _best_snippets does, app/app_product_search.py:347-348), grouped
 * by product: reviews of product row p are h_ids[h_indptr[p] .. h_indptr[p+1]), ascending (file order). */
int rr_reviews_create(const float* h_emb, int64_t n_reviews, int32_t dim, int64_t n_products,
                      const int64_t* h_indptr, const int32_t* h_ids, int32_t device,
                      float normalize_eps, rr_reviews** out);
/* The same with the embeddings in DEVICE memory on `device` ([n_reviews][dim] fp32, unpadded; the CSR stays host memory):
 * rows a builder left on the device become a review index without passing through the host or the file.  Waits for the device
 * before it copies (the rows may have been written on any stream). */
int rr_reviews_create_dev(const float* d_emb, int64_t n_reviews, int32_t dim, int64_t n_products,
                          const int64_t* h_indptr, const int32_t* h_ids, int32_t device,
                          float normalize_eps, rr_reviews** out);
int rr_reviews_destroy(rr_reviews* rv);
/* _best_snippets (app/app_product_search.py:320-370) for the candidates of each query: the review of
 * product rows[q][c] with the largest dot product with query q (first maximum in file order); reviews
 * with id > max_review_id are ignored (the max_rows cut of :342-345).  Outputs n_queries x pool:
 * best score (0 when the product has no review) and best review id (-1 likewise). */
int rr_reviews_best_dev(rr_reviews* rv, const float* d_queries, int32_t n_queries,
                        const int64_t* d_rows, int32_t pool, int64_t row_offset, int32_t max_review_id,
                        float* d_best_score, int32_t* d_best_id, void* stream);

/* The same for a whole batch with the reference's `iloc[:max_rows]` cut (app/app_product_search.py:342-345,
 * app/test.py:200-203) evaluated per query ON THE DEVICE: among the reviews of query q's candidates, in file
 * (= review id) order, only the first max_rows are scored; max_rows <= 0 scores none.  No host round trip. */
int rr_reviews_best_cut_dev(rr_reviews* rv, const float* d_queries, int32_t n_queries,
                            const int64_t* d_rows, int32_t pool, int64_t row_offset, int64_t max_rows,
                            float* d_best_score, int32_t* d_best_id, void* stream);

/* A review index over ONE ROW SHARD of a larger review table (sharded.py): the index holds only the reviews of its own
 * products, its review ids are LOCAL (0 .. n_reviews-1, file order), and h_global_ids[n_reviews] maps them, strictly
 * ascending, to GLOBAL review ids = positions in the whole table of n_total reviews (n_total < 2^31).  With a map every cut
 * the index compares with and every best id it writes is a GLOBAL id (rr_reviews_best_dev's max_review_id and
 * rr_reviews_best_cut_dev included; "keep all" is n_total); scores do not change: a review's score does not depend on the
 * shard it sits in.  Set once, before the first query; an index without a map behaves as before, local = global. */
int rr_reviews_set_global_ids(rr_reviews* rv, const int32_t* h_global_ids, int64_t n_total);

/* The `iloc[:max_rows]` cut when the candidates' reviews lie on several ranks: a 256-way narrowing of an interval of
 * GLOBAL review ids per query, d_state[n_queries][2] int64 = (lo, hi), one launch per round, no host read in between.
 *   begin:  (lo, hi) = (0, n_total - 1).
 *   count:  [narrows first with d_sums, the summed counts of the previous round, when d_sums != NULL;] then
 *           d_counts[q][j] (int64, j = 0..255) = the reviews with global id <= T_j = lo + ((j+1)(hi-lo+1) + 255)/256 - 1
 *           among the candidates d_rows[q][0..pool) this index owns (rows outside [row_offset, row_offset + n_products): 0).
 *           The caller sums d_counts over the ranks.
 *   narrow: with j* the first j whose summed count >= max_rows: lo <- (j* = 0 ? lo : T_{j*-1} + 1), hi <- T_{j*}.
 *           `first` != 0 marks the sums of round 1: a query with count(T_255) <= max_rows is parked at lo = hi = n_total
 *           (keep all) and later narrowings leave it alone.  d_cuts != NULL: also writes d_cuts[q] = lo (int32).
 * After R rounds, R the smallest R >= 1 with 256^R >= n_total, lo = hi = the cut: the max_rows-th smallest global id of
 * the union of the candidates' lists.  max_rows >= 1 (max_rows <= 0 is the caller's: cut -1, no round). */
int rr_reviews_cut_begin_dev(rr_reviews* rv, int32_t n_queries, int64_t* d_state, void* stream);
int rr_reviews_cut_count_dev(rr_reviews* rv, int32_t n_queries, const int64_t* d_rows, int32_t pool, int64_t row_offset,
                             int64_t max_rows, const int64_t* d_sums, int32_t first, int64_t* d_state, int64_t* d_counts,
                             void* stream);
int rr_reviews_cut_narrow_dev(rr_reviews* rv, int32_t n_queries, int64_t max_rows, const int64_t* d_sums, int32_t first,
                              int64_t* d_state, int32_t* d_cuts, void* stream);
/* rr_reviews_best_dev with one cut per query in device memory (d_cuts[n_queries], global ids when the index has a map):
 * best score and best (global) review id per (query, candidate); a row this index does not own gives (0, -1). */
int rr_reviews_best_at_dev(rr_reviews* rv, const float* d_queries, int32_t n_queries, const int64_t* d_rows, int32_t pool,
                           int64_t row_offset, const int32_t* d_cuts, float* d_best_score, int32_t* d_best_id, void* stream);

/* ------------------------------------------------------------ K5 cross-encoder / query encoder forward */

/* BERT-family encoder on the matrix cores (csrc/rr_ce.hip).  Stands in for
 *   CrossEncoder.predict(pairs, batch_size=64, show_progress_bar=False)   app/app_product_search.py:277-278, app/test.py:223-225
 *     (sentence-transformers wraps AutoModelForSequenceClassification; for cross-encoder/ms-marco-MiniLM-L-6-v2 that is
 *      BertForSequenceClassification: 6 layers, hidden 384, 12 heads, FFN 1536, 512 positions, 1 label)
 *   SentenceTransformer.encode([query], normalize_embeddings=True)        app/app_product_search.py:250-251, app/test.py:232
 *     (BAAI/bge-small-en-v1.5: BertModel of the same block shape, 12 layers, CLS pooling; the l2 normalisation is the caller's)
 * Shapes: hidden 384 / 12 heads x 32 / FFN 1536 has kernels of its own, in both precisions.  Every other shape with
 *   hidden % 128 == 0 in [128, 1024], hidden / n_heads = 32 or 64, ffn % 128 == 0 in [128, 4096]
 * (TinyBERT-L-2 128 / 2 / 512, BERT-base 768 / 12 / 3072, bge-large 1024 / 16 / 4096, ...) runs the runtime-shape kernels of
 * csrc/rr_ce_w.hip in RR_CE_PRECISION_F32 only: three bf16 terms per operand, six matrix-core products, any fp32 range.
 * rr_ce_create answers RR_E_INVALID, with nothing allocated, to RR_CE_PRECISION_BF16 at such a shape (the message names the
 * precision) and to a shape outside the family (the message names the offending number).  Layer count (<= 48), vocabulary,
 * positions (<= 512) and labels (<= 64) are free at every shape.
 * Tokenisation (WordPiece): rr_wp_encode_dev below turns documents (ASCII, or UTF-8 on a handle of rr_wp_create_utf8) into
 * the packed ids this call takes, on the device (csrc/rr_wordpiece.hip); what it flags is tokenised on the host
 * (review-recommender_amd/wordpiece.py).  Text PAIRS (the reranker): rr_pairs_measure_dev / rr_pairs_write_dev below assemble
 * them on the device from the token plane of an index and the queries' ids; without a plane they are tokenised on the host. */
typedef struct rr_ce rr_ce;
typedef struct rr_ce_config {
    int32_t hidden, n_layers, n_heads, ffn;       /* 384, L, 12, 1536 -- or another shape of the family above */
    int32_t vocab, max_pos, type_vocab;           /* embedding table sizes */
    int32_t n_labels;                             /* classifier outputs (1 for the reranker); 0 = no pooler / classifier */
    float ln_eps;                                 /* 1e-12 for BERT */
    int32_t precision;                            /* RR_CE_PRECISION_BF16 (fast path) | RR_CE_PRECISION_F32 (the reference's arithmetic) */
} rr_ce_config;
/* RR_CE_PRECISION_BF16: Linear weights rounded once to bf16, bf16 MFMA operands, fp32 accumulation / residual / LayerNorm /
 * softmax / GELU: logits within 2.5e-2 of the fp32 reference on O(1) weights.  RR_CE_PRECISION_F32: what the reference runs
 * (fp32 torch, app/app_product_search.py:250-251, 277-278): fp32 weights and activations; every product on the fp16 matrix
 * cores with both operands carried as two fp16 numbers (hi + lo / 2048, three products per fp32 product: as exact as an
 * fp32 multiply-add chain, csrc/rr_ce_h2.hip), an fp32-grade GELU, base-2 softmax: logits and embeddings within 1e-5 of
 * `transformers` (tests/test_gpu_k5.py), ~2.7x the time of the bf16 mode.  Its range: rr_ce_range_status below. */
#define RR_CE_PRECISION_BF16 0
#define RR_CE_PRECISION_F32 1
/* Weights: fp32 host arrays in the layout of a Hugging Face BERT state dict (Linear weights are [out][in]), in this order:
 *   0 word_embeddings [vocab][H]   1 position_embeddings [max_pos][H]   2 token_type_embeddings [type_vocab][H]
 *   3 embeddings.LayerNorm.weight  4 embeddings.LayerNorm.bias
 *   per layer l, 16 tensors from 5 + 16 l: query.weight, query.bias, key.weight, key.bias, value.weight, value.bias,
 *     attention.output.dense.weight, .bias, attention.output.LayerNorm.weight, .bias,
 *     intermediate.dense.weight [FFN][H], .bias, output.dense.weight [H][FFN], .bias, output.LayerNorm.weight, .bias
 *   when n_labels > 0, four more: pooler.dense.weight [H][H], pooler.dense.bias, classifier.weight [n_labels][H], classifier.bias
 * Linear weights are rounded once to bf16 (nearest even) on the device (RR_CE_PRECISION_F32 also keeps them as given, and
 * as fp16 pairs; a shape other than 384 / 12 / 1536 keeps the fp32 matrices only);
 * everything else stays fp32. */
int rr_ce_create(int32_t device, const rr_ce_config* cfg, const float* const* h_tensors, int32_t n_tensors, rr_ce** out);
int rr_ce_destroy(rr_ce* ce);
#define RR_CE_OUT_LOGITS 0   /* d_out [n_seqs][n_labels]: classifier(tanh(pooler([CLS]))), raw logits (no activation) */
#define RR_CE_OUT_CLS    1   /* d_out [n_seqs][hidden]: last_hidden_state[:, 0] (CLS pooling of the query encoder) */
#define RR_CE_OUT_HIDDEN 2   /* d_out [n_tokens][hidden]: last_hidden_state of every token (diagnostic / parity tests) */
#define RR_CE_OUT_MEAN   3   /* d_out [n_seqs][hidden]: the mean of last_hidden_state over a sequence's tokens, float32, in ONE
                              * fixed order that depends on the sequence's length only (csrc/rr_ce_pool.hip): the pooling of
                              * sentence-transformers' `pooling_mode_mean_tokens` (all-MiniLM, e5, gte).  Not normalised.  Every
                              * layer runs over all tokens: the last layer's [CLS]-only tail serves LOGITS and CLS alone. */
/* Forward over PACKED sequences (no padding is computed): sequence s owns tokens [cu_seqlens[s], cu_seqlens[s+1]);
 * token / type / position ids are per token (position = index inside its sequence); max_len = longest sequence: it must be
 * at least every sequence's length (attention sizes its LDS from it).  In RR_CE_PRECISION_F32 a longer sequence gets NaN
 * outputs and rr_ce_range_status fails with RR_E_INVALID naming max_len; the bf16 precision and the wide-range kernels do not
 * check it (the bf16 attention sizes LDS from it too: an understated max_len is undefined there).
 * RR_CE_PRECISION_F32 takes at most 2^27 tokens per call (RR_E_INVALID beyond: its GEMMs store with 32-bit offsets inside
 * a pair of 16-byte chunks of the activation scratch); its scratch is kept at the handle's largest call.
 * A shape other than 384 / 12 / 1536 does not use max_len beyond the check against the position table (its attention
 * reads every length from cu_seqlens), takes at most 8 388 480 tokens per call (RR_E_INVALID beyond: its GEMMs launch one
 * row of workgroups per 128 tokens), and keeps T x ((4 + ceil(ffn / 2048)) hidden + max(hidden, ffn)) floats of scratch.
 * No path but the fp16-pair one checks the LENGTHS in cu_seqlens on the device: a sequence of more than 512 tokens is the
 * caller's to refuse (cross_encoder.py does, before anything is launched).  At these shapes, as on the wide-range
 * kernels, the attention serves 512 queries per sequence: the context rows of a longer sequence's later tokens are left
 * unwritten (stale scratch: wrong outputs for that sequence), nothing is read or written out of bounds, no flag is raised.
 * Attention is full inside a sequence (what an all-ones attention mask over the unpadded tokens gives).
 * Asynchronous on `stream`; all pointers are device pointers. */
int rr_ce_forward_dev(rr_ce* ce, const int32_t* d_token_ids, const int32_t* d_type_ids, const int32_t* d_pos_ids,
                      const int32_t* d_cu_seqlens, int32_t n_seqs, int64_t n_tokens, int32_t max_len, int32_t mode,
                      float* d_out, void* stream);
/* HIP-event time of the last forward pass on this handle (ms). */
int rr_ce_last_forward_ms(rr_ce* ce, float* out_ms);
/* RR_CE_PRECISION_F32 multiplies on the fp16 matrix cores: every fp32 operand as hi + lo / 2048 in two fp16 numbers, three
 * products per fp32 product (csrc/rr_ce_h2.hip; as exact as an fp32 multiply-add chain).  fp16 ends at 65504: a forward pass
 * that meets a larger activation raises a flag on the device, writes NaN logits / CLS rows / mean-pooled rows for the whole call (never a wrong
 * finite number; RR_CE_OUT_HIDDEN rows are left as computed: ask here) and reports it here -- *out_of_range = 1 -- once
 * the pass has finished (this call waits for it).  A pass whose max_len was below a sequence's length (rr_ce_forward_dev)
 * makes this call return RR_E_INVALID instead: running it again on the wide-range kernels would not help.
 * rr_ce_set_wide_range(ce, 1) switches the handle to three bf16 terms per operand and six products (any fp32 range,
 * ~1.6 x the time): run the pass again after it.  cross_encoder.py does both by itself on the host path.
 * A handle of another shape than 384 / 12 / 1536 has no fp16 anywhere: rr_ce_range_status reports 0, and
 * rr_ce_set_wide_range succeeds and changes nothing (it runs the three-term arithmetic already). */
int rr_ce_range_status(rr_ce* ce, int32_t* out_of_range);
int rr_ce_set_wide_range(rr_ce* ce, int32_t on);

/* ------------------------------------------------------------ WordPiece tokenisation on the device */

/* What SentenceTransformer.encode does to its texts before the model runs (nlp/11_build_product_embeddings.py:46-47: the
 * model's BertTokenizer, lower-casing), for UTF-8 documents (csrc/rr_wordpiece.hip: rr_wp_tokenize_utf8): the host
 * tokenizer's ids, all-ASCII documents included.
 * Pieces: piece i (bytes h_piece_off[i] .. h_piece_off[i+1]) has token id i; an empty piece stands for "no such id";
 * pieces of more than max_chars_per_word (<= 255) code points after their ## can never match and are left out of the
 * device table.  unk / cls / sep are ids in [0, n_pieces).
 * The three arrays are the per-code-point table of review-recommender_amd/wp_unicode.py (unicode_tables(): built from the
 * interpreter's unicodedata so that it agrees with the host tokenizer): h_stage1 [n_stage1 = 8704] maps each block of 128
 * code points to a block of h_stage2 [n_stage2, whole blocks]; an entry = class (bits 0-2: 0 deleted, 1 blank, 2 CJK,
 * 3 other, 4 hard) | mapped code points n (bits 3-4, 0..3) | identity (bit 5) | punctuation flag of mapped code point j
 * (bit 6 + j) | first mapped code point in h_pool [n_pool] (bits 9-31).  The tables are checked here (RR_E_INVALID): nothing
 * the kernel indexes can leave them.  needs_host = 1 only for a document that, in the bytes the kernel reads (the whole
 * document, or its first 4 096 bytes cut back to a character boundary): is malformed UTF-8 (overlong forms, surrogates,
 * values above U+10FFFF, truncated sequences); holds a hard code point; has a mapped text of more than 4 096 bytes; or is
 * longer than the window without max_length - 2 pieces in it. */
typedef struct rr_wp rr_wp;
int rr_wp_create_utf8(int32_t device, const uint8_t* h_piece_bytes, const int64_t* h_piece_off, int32_t n_pieces,
                      int32_t unk_id, int32_t cls_id, int32_t sep_id, int32_t max_chars_per_word,
                      const uint16_t* h_stage1, int32_t n_stage1, const uint32_t* h_stage2, int32_t n_stage2,
                      const uint32_t* h_pool, int32_t n_pool, rr_wp** out);
int rr_wp_destroy(rr_wp* wp);
/* n_docs UTF-8 documents (document s = bytes d_text_off[s] .. d_text_off[s+1] of d_text; text_bytes = size of d_text,
 * below 2^31) -> exactly what rr_ce_forward_dev takes: sequence s = [CLS], the first max_length - 2 pieces, [SEP]; type ids
 * 0; position = index inside the sequence; d_cu_seqlens [n_docs + 1] the running sum; *d_max_len the longest sequence.
 * The ids equal the host tokenizer's, id for id.  A document the kernel hands back (the exceptions listed at
 * rr_wp_create_utf8) is not tokenised: d_needs_host[s] = 1 and its sequence is the placeholder [CLS] [SEP] (the packing
 * stays dense; the caller tokenises it on the host).  The kernel keeps the first 4 096 bytes of a document on chip: a longer
 * document is answered from them when they already hold max_length - 2 pieces in words that end inside them, else
 * needs_host = 1.
 * token_capacity (elements of the three id arrays; n_docs * max_length always suffices, 2 * n_docs is required) bounds
 * the writes: ids beyond it are dropped and d_cu_seqlens[n_docs] tells what was needed.
 * Asynchronous on `stream`, all d_ pointers device pointers; no host wait, except that the first call of a larger
 * n_docs * max_length grows the handle's scratch (hipFree + hipMalloc).  That scratch (per-document id rows and lengths,
 * laid out by THIS call's n_docs and max_length) and the bad-offset counter belong to the handle, not to the call: calls
 * on one handle must be STREAM-ORDERED (the same stream, or ordered by events); two encodes in flight on unordered streams
 * overwrite each other's scratch.  Use one handle per stream for concurrent tokenisation.  Host-checkable limits are RR_E_INVALID and nothing is
 * written; offsets live on the device and are checked THERE: a document whose offsets decrease or leave [0, text_bytes]
 * reads nothing, gets the placeholder with needs_host = 1, and rr_wp_status (which waits for the device) then returns
 * RR_E_INVALID with the count. */
int rr_wp_encode_dev(rr_wp* wp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off, int32_t n_docs,
                     int32_t max_length, int64_t token_capacity, int32_t* d_token_ids, int32_t* d_type_ids, int32_t* d_pos_ids,
                     int32_t* d_cu_seqlens, int32_t* d_needs_host, int32_t* d_max_len, void* stream);
int rr_wp_status(rr_wp* wp, int32_t* out_bad_docs);
/* The piece table rr_wp_create_utf8 puts on the device, built on the host (no device needed; tests walk it): n_slots =
 * rr_wp_table_slots(n_pieces) (a power of two, at least twice the pieces); h_slots [n_slots][4] int32 = polynomial hash
 * (base 0x01000193 mod 2^32) of the piece's bytes without its ##, first byte in h_piece_bytes, length in BYTES |
 * (## form) << 16, id (-1 = empty); open addressing, linear probing from murmur3's finaliser of hash ^ (length word *
 * 0x9E3779B1).  max_chars_per_word counts code points (the bytes that are not 10xxxxxx). */
int rr_wp_table_slots(int32_t n_pieces, int32_t* out_slots);
int rr_wp_build_table_utf8(const uint8_t* h_piece_bytes, const int64_t* h_piece_off, int32_t n_pieces, int32_t max_chars_per_word,
                           int32_t n_slots, int32_t* h_slots, int32_t* out_kept);

/* ------------------------------------------------------------ review text: clean, filter, dedup (csrc/rr_textprep.hip) */

/* nlp/11_build_product_embeddings.py:110-118 in front of rr_wp_encode_dev, which reads what these calls write.  Status word
 * of a document: 0 = it survives. */
#define RR_TP_SHORT      1   /* fewer than 10 code points after normalize_text */
#define RR_TP_SPAM       2   /* looks_spammy(normalised text) */
#define RR_TP_NEEDS_HOST 4   /* not decided here: the caller cleans this document on the host (no other bit is set, length 0) */
#define RR_TP_DUP        8   /* an earlier surviving document has the same group and the same bytes */
typedef struct rr_textprep rr_textprep;
int rr_textprep_create(int32_t device, rr_textprep** out);
int rr_textprep_destroy(rr_textprep* tp);
/* Bytes of a document the clean kernel holds on chip, bytes per step of its walk, consecutive bytes per thread. */
int rr_textprep_limits(int32_t* out_window, int32_t* out_tile, int32_t* out_per_thread);
/* normalize_text (:32-36: Unicode whitespace -> one space, strip, the first 4000 code points), the length filter (:112) and,
 * with spam != 0, looks_spammy (:38-39) for n_docs UTF-8 documents laid out as rr_wp_encode_dev reads them (document s =
 * bytes d_text_off[s] .. d_text_off[s+1] of d_text).  Document s's normalised text is written at d_out + d_text_off[s]
 * (never longer than the raw text), its length in bytes to d_out_len[s], its status word to d_status[s].  d_out may be
 * d_text when the offsets do not decrease (a workgroup reads its whole document before it writes, and then no two
 * documents overlap).  RR_TP_NEEDS_HOST: a document longer than the window, malformed UTF-8, U+0130 / U+0131 / U+017F
 * (spam only: the three code points outside ASCII that IGNORECASE folds onto a letter of the patterns), or offsets that
 * decrease or leave [0, text_bytes]; the last kind reads and writes no text and makes rr_textprep_status (which waits for
 * the device) return RR_E_INVALID with the count.  Asynchronous on `stream`; n_docs = 0 does nothing. */
int rr_textprep_clean_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                          int32_t n_docs, int32_t spam, uint8_t* d_out, int32_t* d_out_len, int32_t* d_status, void* stream);
/* The same with the cut at max_chars code points instead of 4000; 0 = no cut (nlp/10_product_prep.py:21-24 has none).
 * rr_textprep_clean_dev is this call with 4000. */
int rr_textprep_clean_chars_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                int32_t n_docs, int32_t spam, int32_t max_chars, uint8_t* d_out, int32_t* d_out_len,
                                int32_t* d_status, void* stream);
int rr_textprep_status(rr_textprep* tp, int32_t* out_bad_docs);
/* drop_duplicates(subset=["sku", "__txt"]) (:117) among the documents whose status word is 0: document s = d_len[s] bytes
 * at d_text + d_text_off[s], d_group[s] = its sku's number.  Sets RR_TP_DUP on every survivor for which an EARLIER survivor
 * has the same group and the same bytes; equality is decided by comparing bytes, hash_bits (64; tests pass 3 so that almost
 * every probe collides) only shortens the hash that picks the first slot.  The result does not depend on scheduling.
 * Calls on one handle must be stream-ordered (the table is the handle's scratch, grown on the first call of a size). */
int rr_textprep_dedup_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                          const int32_t* d_len, const int32_t* d_group, int32_t* d_status, int32_t n_docs,
                          int32_t hash_bits, void* stream);
/* The survivors (status 0), in order, as rr_wp_encode_dev reads them: texts back to back in d_out_text (capacity out_bytes),
 * d_out_off [m + 1] (capacity n_docs + 1), d_src_row [m] (capacity n_docs) the document each came from, d_count[0] = m,
 * d_count[1] = bytes.  A device prefix sum; no host wait. */
int rr_textprep_compact_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                            const int32_t* d_len, const int32_t* d_status, int32_t n_docs, uint8_t* d_out_text,
                            int64_t out_bytes, int64_t* d_out_off, int32_t* d_src_row, int64_t* d_count, void* stream);
/* The HEAD of documents of any length: the first max_chars (0 .. 2^28) code points of what a document gives, normalised
 * (normalize != 0: Unicode whitespace -> one space, strip; the space counts -- nlp/11's normalize_text read as a prefix) or
 * verbatim (str[:max_chars]).  textprep.model_head states the rules.  Output document j reads input document
 * d_doc_rows[j] (int32; NULL = j) of the n_src_docs documents d_text_off [n_src_docs + 1] describes: a row shard or the
 * survivors of a filter need no copy of their text.  d_out_len[j] = the head's bytes, d_status[j] = RR_TP_SHORT (fewer than
 * min_chars code points; min_chars 0 = no filter), RR_TP_NEEDS_HOST (malformed UTF-8 met while fewer than max_chars code
 * points were emitted: bytes behind the point where the walk stops are never examined; length 0) or 0.  Length is never a
 * reason for RR_TP_NEEDS_HOST: a workgroup streams its document in tiles (rr_textprep_limits) and stops at the cut.
 * A call with a text offset that decreases or leaves [0, text_bytes], or a d_doc_rows entry outside [0, n_src_docs), reads
 * no text, answers length 0 and RR_TP_NEEDS_HOST for every document and is reported by rr_textprep_status.  Asynchronous
 * on `stream`; the head calls of one handle must be stream-ordered. */
int rr_textprep_head_measure_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                                 int32_t n_src_docs, const int32_t* d_doc_rows, int32_t n_docs, int32_t max_chars,
                                 int32_t normalize, int32_t min_chars, int32_t* d_out_len, int32_t* d_status, void* stream);
/* d_out_off [n_docs + 1] = the exclusive scan of the lengths of the documents whose status word is 0 (a document with
 * another status takes no room); d_out_off[n_docs] = the bytes pass 2 writes.  A device prefix sum; no host wait. */
int rr_textprep_head_offsets_dev(rr_textprep* tp, const int32_t* d_out_len, const int32_t* d_status, int32_t n_docs,
                                 int64_t* d_out_off, void* stream);
/* Pass 2, over the same arguments and what pass 1 answered: the head of every document whose status word is 0 is written at
 * d_out_text + d_out_off[j] (d_out_off int64 [n_docs + 1]: an exclusive scan of the lengths, or the host's own offsets when
 * rows it cleaned itself take room between the heads; a document whose status word is not 0 writes nothing).  Refused, as
 * above and with nothing read or written: output offsets that decrease, leave [0, out_bytes] or give a surviving document
 * less room than d_out_len[j]. */
int rr_textprep_head_write_dev(rr_textprep* tp, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                               int32_t n_src_docs, const int32_t* d_doc_rows, int32_t n_docs, int32_t max_chars,
                               int32_t normalize, int32_t min_chars, const int32_t* d_out_len, const int32_t* d_status,
                               uint8_t* d_out_text, int64_t out_bytes, const int64_t* d_out_off, void* stream);

/* ------------------------------------------------------------ BM25 corpus: tokens and vocabulary ids (csrc/rr_doctok.hip) */

/* nlp/12_product_prep.py:42-49,75-83 and pd.factorize(sort=False) on the device: from the raw text column to
 * (tok int32[T], doc_off int64[n + 1], vocabulary) -- the arrays bm25.factorize_corpus(build_bm25_blob(meta)["corpus"]) makes
 * and rr_bm25_build reads.  The rules (doctok.model_tokenize states them in Python):
 *   - a byte is an alnum (0-9 a-z, A-Z lower-cased), an apostrophe or a separator; E2 84 AA (U+212A KELVIN SIGN) is the alnum
 *     'k' and C4 B0 (U+0130) the alnum 'i' followed by a separator: the only two code points outside ASCII that str.lower()
 *     maps onto ASCII.  Every other byte >= 0x80, and NUL, is a separator, so no document is left to the host;
 *   - a token is a run of alnums, and one more run behind a single apostrophe: [a-z0-9]+(?:'[a-z0-9]+)?, greedy, left to
 *     right (a'b'c -> a'b, c; ab''cd -> ab, cd); its bytes are the MAPPED bytes;
 *   - tokens of one byte and the stop words given at create are dropped, then the document keeps its first 5000 tokens.
 * The calls of one handle must be stream-ordered, in this order:
 *   rr_doctok_count_dev   pass 1: kept tokens per document and their int64 prefix sum into d_doc_off [n_docs + 1];
 *   rr_doctok_sizes       waits for the device; out_sizes[0] = T, [1] = bytes of the token arena (= text_bytes: a token's
 *                         bytes sit at the offset of its first byte in the text), [2] = n_terms, [3] = bytes of the vocabulary
 *                         (the last two once rr_doctok_vocab_dev has run, else 0).  When a document's offsets decrease or
 *                         leave [0, text_bytes] (no text is read for it), or a token has 2^31 bytes or more: RR_E_INVALID,
 *                         out_sizes[0] = the number of such documents, the count is dropped and the handle keeps what the
 *                         calls before it established.  More than 2^31 - 1 terms: RR_E_INVALID;
 *   rr_doctok_emit_dev    pass 2 over the same text and offsets: per token its arena offset, length and 64-bit hash, at the
 *                         global position d_doc_off[d] + index (buffers of the handle, sized from T);
 *   rr_doctok_vocab_dev   ids in first-appearance order into d_tok [T]: an open-addressing table of max(64, 2 T) slots of
 *                         8 bytes (it cannot fill; the probe loop is bounded by the table's size all the same and a token
 *                         without a slot makes rr_doctok_sizes fail), claimed by compare-and-swap, every hit decided by a
 *                         BYTE compare, a 64-bit atomicMin of the token's position per slot; first[p] = (minimum == p), an
 *                         exclusive int64 scan of first = the id.  hash_bits (64; tests pass 3 so that nearly every probe
 *                         collides) only shortens the hash that picks the first slot.  The result does not depend on
 *                         scheduling.  May be called again on the same token stream;
 *   rr_doctok_copy_vocab  (after rr_doctok_sizes) the vocabulary in id order to the host: h_bytes [sizes[3]], h_off
 *                         [n_terms + 1].  Waits.  d_tok = what rr_doctok_vocab_dev wrote;
 *   rr_doctok_copy_tokens the token stream before the vocabulary, for tests: h_pos [T] arena offsets, h_len [T], h_arena
 *                         [text_bytes] (may be NULL).  Waits.
 * count / emit / vocab are asynchronous on `stream` and ordered after it.  The calls that wait (rr_doctok_sizes,
 * rr_doctok_copy_vocab, rr_doctok_copy_tokens) synchronise the whole DEVICE, not only that stream, and rr_doctok_copy_vocab
 * runs its gather on the NULL stream (as rr_textprep_status waits).
 * Time: one workgroup per document, and a token is walked by the ONE thread that holds its first byte (from global memory
 * once it leaves the tile's window).  Ordinary text costs nothing for that; a document that is a single alphanumeric run
 * of many MB is walked by one lane, a byte per step, in both passes: its time grows with the run's length and nothing
 * bounds it (DESIGN.md K2-text quotes a 1 MiB run).
 * n_docs = 0 gives d_doc_off = [0]; T = 0 an empty vocabulary.
 * Every position, count and offset is int64; only ids and a token's length are int32.
 * Device memory of the handle, at its peak (rr_doctok_vocab_dev): text_bytes (arena) + 28 T (offset 8, length 4, hash 8,
 * slot 8 per token) + 16 T (table: 2 T slots of 8 bytes) + 8 T / 4096 (scan), beside the caller's text, d_doc_off and 4 T
 * of ids: 44 T + text_bytes.  rr_doctok_copy_vocab adds 16 n_terms + the vocabulary's bytes while it runs. */
typedef struct rr_doctok rr_doctok;
/* Stop words: n_stop <= 64 words of 1..8 bytes, h_stop_off [n_stop + 1] into h_stop_bytes (text.INDEX_STOP_WORDS). */
int rr_doctok_create(int32_t device, const uint8_t* h_stop_bytes, const int64_t* h_stop_off, int32_t n_stop, rr_doctok** out);
int rr_doctok_destroy(rr_doctok* dt);
/* Bytes per step of the walk, consecutive bytes per thread, tokens kept per document. */
int rr_doctok_limits(int32_t* out_tile, int32_t* out_per_thread, int32_t* out_token_cap);
int rr_doctok_count_dev(rr_doctok* dt, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off, int32_t n_docs,
                        int64_t* d_doc_off, void* stream);
int rr_doctok_sizes(rr_doctok* dt, int64_t* out_sizes);
int rr_doctok_emit_dev(rr_doctok* dt, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off, int32_t n_docs,
                       const int64_t* d_doc_off, void* stream);
int rr_doctok_vocab_dev(rr_doctok* dt, int32_t hash_bits, int32_t* d_tok, void* stream);
int rr_doctok_copy_vocab(rr_doctok* dt, const int32_t* d_tok, uint8_t* h_bytes, int64_t* h_off);
int rr_doctok_copy_tokens(rr_doctok* dt, int64_t* h_pos, int32_t* h_len, uint8_t* h_arena);

/* ------------------------------------------------------------ products.parquet: order, KPIs, agg_text (csrc/rr_products.hip) */

/* nlp/10_product_prep.py:54-78 on the device, behind rr_textprep_clean_chars_dev (max_chars 0, spam 0) and
 * rr_textprep_dedup_dev (products.model_build_products states the whole step in numpy).  The calls of one handle must be
 * stream-ordered; they use the handle's scratch. */
typedef struct rr_products rr_products;
int rr_products_create(int32_t device, rr_products** out);
int rr_products_destroy(rr_products* pb);
/* Rows s of [0, n) with d_status[s] == 0 survive; d_group[s] in [0, n_skus) = the rank of the row's sku among the sorted
 * distinct skus, d_stars[s] a double (NaN = none), d_ts[s] int64 ns (INT64_MIN = NaT).  Writes
 *   d_perm      int32 [n]: its first m = d_seg_off[n_skus] entries are the survivors, sku-major, within a sku by stars
 *               descending (NaN last, -0.0 == 0.0, the infinities as numbers), then ts descending (NaT last), then row
 *               ascending -- pandas' stable sort_values(["sku", "stars", "ts"], ascending=[True, False, False]).  The rest
 *               holds the rows that did not survive;
 *   d_seg_off   int64 [n_skus + 1]: sku k owns d_perm[d_seg_off[k] .. d_seg_off[k + 1]);
 *   per sku k:  d_n_reviews[k] (int64) = its survivors, d_star_sum[k] (double) = the sum of their non-NaN stars added one
 *               by one in d_perm order, d_star_cnt[k] (int64) = how many those are, d_last_ts[k] = the largest ts
 *               (INT64_MIN when every one is NaT).
 * A stable LSD radix sort (csrc/rr_prims.h) over order-preserving key words, least significant first: linear in n whatever
 * the segment lengths, and no atomic decides an order.  The groups of the survivors are checked on the device before
 * anything is sorted (this call waits for that): one outside [0, n_skus) returns RR_E_INVALID and writes no output. */
int rr_products_order_dev(rr_products* pb, const int32_t* d_status, const int32_t* d_group, const double* d_stars,
                          const int64_t* d_ts, int32_t n, int32_t n_skus, int32_t* d_perm, int64_t* d_seg_off,
                          int64_t* d_n_reviews, double* d_star_sum, int64_t* d_star_cnt, int64_t* d_last_ts, void* stream);
/* agg_text: for sku k the texts of its first min(length, max_per_sku) rows of d_perm (row s = d_len[s] bytes at d_text +
 * d_text_off[s]) joined by the two bytes " \n", back to back in d_out_text (capacity out_bytes; the cleaned bytes of the
 * survivors + 2 m always suffice), d_out_off int64 [n_skus + 1], d_count[0] = the bytes written: the layout
 * rr_doctok_count_dev reads.  One device scan over the skus; no host wait.  A segment offset that decreases or leaves
 * [0, n], a row outside [0, n), a text that leaves [0, text_bytes] or a capacity that is too small write NO text (d_out_off
 * and d_count are still written) and make rr_products_status return RR_E_INVALID. */
int rr_products_concat_dev(rr_products* pb, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                           const int32_t* d_len, int32_t n, const int32_t* d_perm, const int64_t* d_seg_off, int32_t n_skus,
                           int32_t max_per_sku, uint8_t* d_out_text, int64_t out_bytes, int64_t* d_out_off, int64_t* d_count,
                           void* stream);
/* Waits for the device; RR_E_INVALID when a rr_products_concat_dev since the last call refused its arguments
 * (*out_bad = how many skus or buffers it refused).  Until it is called, later rr_products_concat_dev calls on the handle
 * write no text either: ask after every concatenation whose text is used. */
int rr_products_status(rr_products* pb, int32_t* out_bad);

/* ------------------------------------------------------------ the attribute gate: plane and match (csrc/rr_gate.hip) */

/* calculate_gate_factor (utils.py:88-101; app/app_product_search.py:297-302, app/test.py:292-297) on the device: a group of
 * terms hits when any of its terms occurs as a substring of agg_text[:6000].lower(); factor = penalty ** (groups missed).
 * gate.model_gate_plane / gate.model_gate_hits state both halves in Python.  The calls of one handle must be stream-ordered.
 *
 * THE PLANE, once per index: for every document the byte image of its first max_chars code points (code points = the bytes
 * that are not 10xxxxxx), back to back with int64 offsets, such that for every string s of ASCII characters
 * s in text[:max_chars].lower() <=> s's bytes occur in the image:  A-Z -> a-z;  C4 B0 (U+0130) -> 69 B0 (lower() gives 'i' +
 * U+0307);  E2 84 AA (U+212A) -> 6B ('k', its two continuation bytes dropped);  every other byte -> itself.  Those two are
 * the only code points outside ASCII whose lower() holds an ASCII character.  The image need not be valid UTF-8, and the
 * text is not validated: it comes from a Python str (`surrogatepass` where needed), so no document is left to the host.
 *   rr_gate_measure_dev  pass 1 over the text in the layout rr_wp_encode_dev reads: the images' lengths and their exclusive
 *                        int64 sum into d_plane_off [n_docs + 1], the total also into d_total[0] (device) -- the only number
 *                        the host reads back, to size the plane: total + the slack of rr_gate_limits, 16-byte aligned;
 *   rr_gate_write_dev    pass 2 over the same text and offsets: the images into d_plane (capacity plane_bytes; too small =
 *                        nothing is written and rr_gate_status fails).
 * A workgroup per document walks it in steps and stops at the step that holds code point max_chars + 1 (a 100 KB agg_text
 * is read to its 6000th code point).  A document whose offsets decrease or leave [0, text_bytes] is not read, has an empty
 * image and is counted by rr_gate_status.  n_docs = 0 gives d_plane_off = [0].
 *
 * THE MATCH, per batch: rr_gate_factors_dev.  d_rows [n_queries x pool] int64 GLOBAL rows; candidate row r reads document
 * r - row_offset.  The batch's terms, packed (gate.pack_groups): d_term_bytes, d_term_off int32 [T + 1], d_term_group int32
 * [T] (the group 0..5 of each term), d_q_term int32 [n_queries + 1] (query q owns terms d_q_term[q] .. d_q_term[q + 1]),
 * d_q_groups int32 [n_queries] (its number of groups, 0..6), d_factor float32 [n_queries x 7]: d_factor[q][m] = the factor
 * of m missed groups, filled by the host with the reference's arithmetic (a Python float, factor *= penalty left to right,
 * one float32 cast).  Writes d_gate [n_queries x pool] float32 = d_factor[q][groups missed] -- the kernel does no floating
 * point, the value is bitwise the reference's -- and, when d_hits is not NULL, d_hits [n_queries x pool] int32 = the bit
 * mask of the groups that hit.  A query with 0 groups gives d_factor[q][0] (1.0) and reads no text.  A row outside
 * [row_offset, row_offset + n_docs) reads no text, misses every group and is counted by rr_gate_status; so is a query whose
 * packing exceeds rr_gate_limits, has a zero-length term, a byte >= 0x80 or a group outside [0, groups): it is answered
 * d_factor[q][0] (the Python side checks all of that before the call and gates such a query on the host).
 * One wave per (query, candidate), four candidates of a query per workgroup, the terms in LDS; the image is read in aligned
 * 16-byte words, and the bytes of a boundary word that belong to a neighbouring document are replaced by FF before anything
 * is compared, so a match never runs into the next or the previous document.  No result depends on scheduling.
 * Asynchronous on `stream`; no host wait, no allocation. */
typedef struct rr_gate rr_gate;
int rr_gate_create(int32_t device, rr_gate** out);
int rr_gate_destroy(rr_gate* g);
/* Bytes of a document per step of the plane kernels, bytes of an image per step of a wave of the match, consecutive bytes per
 * thread (both), the longest term in bytes, term bytes per query, terms per query, readable bytes the plane needs behind
 * its last document. */
int rr_gate_limits(int32_t* out_plane_step, int32_t* out_match_step, int32_t* out_per_thread, int32_t* out_max_term,
                   int32_t* out_term_bytes, int32_t* out_max_terms, int32_t* out_slack);
int rr_gate_measure_dev(rr_gate* g, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off, int32_t n_docs,
                        int32_t max_chars, int64_t* d_plane_off, int64_t* d_total, void* stream);
int rr_gate_write_dev(rr_gate* g, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off, int32_t n_docs,
                      int32_t max_chars, const int64_t* d_plane_off, uint8_t* d_plane, int64_t plane_bytes, void* stream);
/* plane_bytes = the images' total (d_plane_off[n_docs]); d_plane must be 16-byte aligned and readable for the slack behind
 * it.  d_plane, d_term_bytes and d_term_group must not be NULL even when they hold nothing. */
int rr_gate_factors_dev(rr_gate* g, const uint8_t* d_plane, const int64_t* d_plane_off, int64_t plane_bytes, int32_t n_docs,
                        int64_t row_offset, const int64_t* d_rows, int32_t n_queries, int32_t pool, const uint8_t* d_term_bytes,
                        const int32_t* d_term_off, const int32_t* d_term_group, const int32_t* d_q_term,
                        const int32_t* d_q_groups, const float* d_factor, float* d_gate, int32_t* d_hits, void* stream);
/* Waits for the device; RR_E_INVALID when a call since the last one refused a document, a plane buffer, a candidate row or a
 * query's packing (*out_bad = how many). */
int rr_gate_status(rr_gate* g, int32_t* out_bad);

/* ------------------------------------------------------------ the reranker's pairs: token plane and assembly (csrc/rr_pairs.hip) */

/* What CrossEncoder.predict does in front of the model as run_search calls it (app/app_product_search.py:272-278,
 * app/test.py:223-225): the pairs (query, agg_text[:2000]) as `[CLS] query [SEP] text [SEP]`, truncated `longest_first` to
 * max_length, packed as rr_ce_forward_dev takes them.  rerank.model_plane / rerank.model_pairs state both halves in numpy.
 * The calls of one handle must be stream-ordered.
 *
 * THE TOKEN PLANE, once per index (rerank.RerankText builds it with rr_wp_encode_dev): for every document the WordPiece ids
 * of its first 2000 code points, the first max_length - 3 of them (no longer text side survives the truncation), as uint16
 * back to back in d_plane_tok, with int64 offsets d_plane_off [n_docs + 1].  Document i is the product of global row
 * row_offset + i.
 *
 * THE ASSEMBLY, per batch.  d_rows [n_queries x pool] int64 GLOBAL rows, of which the first rr_k <= pool of every query are
 * reranked: pair p of the flattened list is (query b = p / rr_k, candidate j = p % rr_k) and reads d_rows[b * pool + j].  A
 * call serves the pairs [first_pair, first_pair + n_pairs), any range of the n_queries x rr_k, one that begins and ends
 * inside a query included (the caller chunks with it).  The queries' ids: d_q_tok int32, d_q_off int32 [n_queries + 1].
 *   rr_pairs_measure_dev  d_keep [n_pairs][2] int32 = the query and text tokens pair first_pair + i keeps, by the rule of
 *                         `longest_first` as wordpiece.py states it, with avail = max_length - 3: cut only when
 *                         n_a + n_b > avail; n1 = the shorter side, n2 = the longer (the text on a tie); n2 = n1 if
 *                         n1 > avail else max(n1, avail - n1); if n1 + n2 > avail still, n1 = avail / 2 and
 *                         n2 = n1 + avail % 2.  d_cu [n_pairs + 1] int32 = the exclusive sum of the sequence lengths
 *                         keep_a + keep_b + 3.  The host reads back ONE number, d_cu[n_pairs]: it sizes the three id arrays
 *                         and is the n_tokens of rr_ce_forward_dev.  n_b is what the plane holds, min(tokens, avail): the
 *                         rule answers the same for both whenever n_a <= avail, so a query of more than avail tokens is
 *                         not for this call (rerank.pack_queries hands it to the host).
 *   rr_pairs_write_dev    the sequences into d_tok / d_typ / d_pos (capacity n_tokens each): [CLS], the kept query ids,
 *                         [SEP], the kept text ids widened from uint16, [SEP]; type 0 up to and including the first [SEP],
 *                         1 behind it; position = index inside the sequence.  One wave per pair, lanes striding over the
 *                         sequence: the text reads and the three int32 stores are contiguous per wave.
 * A row outside [row_offset, row_offset + n_docs) reads no text, gives [CLS] query [SEP] [SEP] and is counted by
 * rr_pairs_status; a pair whose d_keep / d_cu do not fit the offsets or n_tokens is not written and counted too.  Limits the
 * host can check are RR_E_INVALID with nothing written: rr_k outside 1..pool, a range outside n_queries x rr_k,
 * max_length < 3, n_pairs * max_length beyond int32, n_tokens above 2^27 (rr_ce_forward_dev's fp32 call limit).
 * Asynchronous on `stream`; no host wait, except that the first measure of a larger n_pairs grows the scan's scratch. */
typedef struct rr_pairs rr_pairs;
int rr_pairs_create(int32_t device, rr_pairs** out);
int rr_pairs_destroy(rr_pairs* h);
int rr_pairs_measure_dev(rr_pairs* h, const int64_t* d_plane_off, int32_t n_docs, int64_t row_offset, const int64_t* d_rows,
                         int32_t pool, int32_t rr_k, const int32_t* d_q_off, int32_t n_queries, int32_t max_length,
                         int64_t first_pair, int32_t n_pairs, int32_t* d_keep, int32_t* d_cu, void* stream);
/* d_plane_tok and d_q_tok must not be NULL even when they hold nothing. */
int rr_pairs_write_dev(rr_pairs* h, const uint16_t* d_plane_tok, const int64_t* d_plane_off, int32_t n_docs, int64_t row_offset,
                       const int64_t* d_rows, int32_t pool, int32_t rr_k, const int32_t* d_q_tok, const int32_t* d_q_off,
                       int32_t n_queries, int32_t cls_id, int32_t sep_id, int64_t first_pair, int32_t n_pairs,
                       const int32_t* d_keep, const int32_t* d_cu, int64_t n_tokens, int32_t* d_tok, int32_t* d_typ,
                       int32_t* d_pos, void* stream);
/* Waits for the device; RR_E_INVALID when a call since the last one met a row outside the plane or refused a pair
 * (*out_bad = how many). */
int rr_pairs_status(rr_pairs* h, int32_t* out_bad);

/* ------------------------------------------------------------ the query front: ids, gate groups, reranker ids (csrc/rr_query.hip) */

/* What run_search does with the query STRING before the kernels (utils.py:57-86, app/app_product_search.py:189-227), for a
 * whole batch on the device: the BM25 term ids of text.tokenize_query, the gate groups of text.build_gate_groups packed as
 * gate.pack_groups packs them, the reranker's query ids packed as rerank.pack_queries packs them -- each in the layout its
 * consumer reads (the BM25 scores at the candidates, the gate match, the pair assembly).  querytext.model_front states in
 * plain Python what the kernels compute.  The calls of one handle must be stream-ordered.
 *
 * THE TABLES, once per index (the create call uploads them; the kernel source holds no word list):
 *   the vocabulary  bytes + int64 offsets [n_vocab + 1] in id order, hashed ON THE HOST into an open-addressing table (the
 *                   build_table call; the table_slots call gives its size: a power of two, at least 64 and at least twice
 *                   the entries): a slot = 4 int32 = hash, first byte, length, id (-1 = empty).  Entries that are not 1 .. 64
 *                   bytes of [a-z0-9'] are left out: no query token can equal them.  A lookup compares the hash, then the bytes;
 *   the stop words  bytes + int32 offsets [n_stop + 1], 1 .. 8 ASCII bytes each;
 *   the static gate groups  n_colors colour groups, then n_syn synonym groups: the terms' bytes + int32 offsets, SORTED inside
 *                   a group, h_group_off int32 [n_colors + n_syn + 1] = first term of each group; the synonym groups' keys as
 *                   bytes + int32 offsets [n_syn + 1].  Terms and keys are 1 .. 64 ASCII bytes.  max_groups (1 .. 6) groups
 *                   of the largest static group must fit the gate's 64 terms and 1024 term bytes per query, so that no query
 *                   the kernel answers can exceed a limit of the gate match.
 *
 * THE BATCH.  d_text = the UTF-8 bytes of n_queries (1 .. 65535) queries back to back, d_text_off = n_queries + 1 int64
 * offsets (the layout rr_wp_encode_dev reads, so one staged buffer serves both).  Per query:
 *   tokens      the matches of [a-z0-9]+(?:'[a-z0-9]+)? (greedy, left to right) over the bytes after A-Z -> a-z,
 *               E2 84 AA -> k, C4 B0 -> i + separator, NUL and every other byte >= 0x80 -> separator; minus the stop words;
 *   d_ids       one vocabulary id per token, in order, duplicates kept, -1 for a token the table lacks; query q owns
 *               d_ids[d_ids_off[q] .. d_ids_off[q + 1]), d_ids_off int32 [n_queries + 1];
 *   gate groups colour groups in table order, present when one of their terms is a SUBSTRING of the lower-cased query (the
 *               gate plane's byte image of it); then per token its synonym group when the token is that group's key, else
 *               {token} when it has min_keyword_len bytes or more; groups equal as sets are dropped, the first stays; the first
 *               max_groups are kept.  Written as the gate match reads them: d_term_bytes, d_term_off int32 [T + 1],
 *               d_term_group int32 [T], d_q_term int32 [n_queries + 1], d_q_groups int32 [n_queries]; the factor table
 *               stays the host's (no floating point here);
 *   d_needs_host int32 [n_queries], one bit per reason: 1 = the query has more than 1024 bytes, 2 = a token has more than 64
 *               bytes, 4 = more than max_length - 3 reranker ids, 8 = the WordPiece kernel handed it back, 16 = its offsets
 *               decrease or leave the text (also counted by the status call).  A flagged query gets no ids, no groups and
 *               no reranker ids: the caller serves it through the host functions.  (32 is not this call's: the flag call
 *               below sets it for a query the QUERY ENCODER's WordPiece kernel handed back.)
 * d_wp_cu / d_wp_needs_host (both or neither): cu_seqlens and needs_host of rr_wp_encode_dev over the SAME text and offsets
 * with the cross-encoder's vocabulary and max_length = the cross-encoder's (then a query of max_length - 2 pieces or more
 * shows as such); they decide bits 4 and 8 and the reranker counts.  d_counts int32 [n_queries x 4] (ids, terms, term bytes,
 * reranker ids per query) is scratch between the two launches and the input of the strip call.
 * Two launches, a wave per query: `measure` writes d_counts and d_needs_host, `write` sums the counts of the queries in front
 * of its own and writes.  Capacities (cap_ids ids, cap_terms terms -- d_term_off holds cap_terms + 1 --, cap_term_bytes):
 * every store is checked first; one that does not fit is not made and counted by the status call.  Upper bounds: a query
 * of b bytes has at most (b + 1) / 2 tokens, max_groups groups have at most 64 terms and 1024 term bytes.
 *
 * The strip call: d_rr_ids / d_rr_off int32 [n_queries + 1] = the pieces of every unflagged query without [CLS] and [SEP],
 * back to back (d_wp_tok of capacity wp_capacity and d_wp_cu as rr_wp_encode_dev wrote them, d_counts as the front call
 * left it).  Asynchronous on `stream`; no host wait, no allocation, nothing read back. */
typedef struct rr_query rr_query;
/* Bytes of a query, bytes of a token, groups per query, bytes of a stop word the kernels hold. */
int rr_query_limits(int32_t* out_max_query, int32_t* out_max_token, int32_t* out_max_groups, int32_t* out_max_stop);
int rr_query_table_slots(int32_t n_entries, int32_t* out_slots);
/* Host only (no device needed): h_slots [n_slots][4] int32, *out_kept = the entries kept. */
int rr_query_build_table(const uint8_t* h_bytes, const int64_t* h_off, int32_t n_entries, int32_t n_slots, int32_t* h_slots,
                         int32_t* out_kept);
int rr_query_create(int32_t device, const uint8_t* h_vocab_bytes, const int64_t* h_vocab_off, int32_t n_vocab,
                    const uint8_t* h_stop_bytes, const int32_t* h_stop_off, int32_t n_stop, const uint8_t* h_term_bytes,
                    const int32_t* h_term_off, const int32_t* h_group_off, int32_t n_colors, int32_t n_syn,
                    const uint8_t* h_key_bytes, const int32_t* h_key_off, int32_t max_groups, int32_t min_keyword_len,
                    rr_query** out);
int rr_query_destroy(rr_query* h);
int rr_query_front_dev(rr_query* h, const uint8_t* d_text, int64_t text_bytes, const int64_t* d_text_off,
                       int32_t n_queries, const int32_t* d_wp_cu, const int32_t* d_wp_needs_host, int32_t max_length,
                       int32_t* d_counts, int32_t* d_needs_host, int32_t* d_ids, int32_t* d_ids_off, int64_t cap_ids,
                       int32_t* d_term_off, int32_t* d_term_group, int32_t* d_q_term, int32_t* d_q_groups,
                       uint8_t* d_term_bytes, int64_t cap_terms, int64_t cap_term_bytes, void* stream);
int rr_query_strip_dev(rr_query* h, const int32_t* d_wp_tok, const int32_t* d_wp_cu, int64_t wp_capacity, int32_t n_queries,
                       const int32_t* d_counts, int32_t* d_rr_off, int32_t* d_rr_ids, int64_t cap_rr, void* stream);
/* Waits for the device; RR_E_INVALID when a call since the last one met offsets that decrease or leave the text or a store
 * beyond a capacity (*out_bad = how many). */
int rr_query_status(rr_query* h, int32_t* out_bad);

/* The query VECTORS of a batch: the encoder's pooled rows (rr_ce_forward_dev with RR_CE_OUT_CLS, or RR_CE_OUT_MEAN for
 * an encoder that pools the mean over the tokens, over the WordPiece ids of the same staged bytes) to the unit vectors K1 reads.  Row q of d_out = d_rows[q] / max(||d_rows[q]||, eps) in float32, every
 * rounding the one numpy makes in `e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), eps)` on a C-contiguous float32
 * array (cross_encoder.QueryEncoder.encode_ids), so the result equals the host's bit for bit (querytext.model_query_vectors
 * states the same in plain Python; tests/test_query_vectors_model.py proves it against numpy):
 *   squares      each x * x is rounded to float32 BEFORE it is summed: no FMA forms across the square and the add.  The
 *                library is built with -ffp-contract=off and the kernel is correct under it; it also carries the pragma;
 *   sum order    numpy's pairwise sum of the n = dim squares.  n < 8: sequential from 0.  8 <= n <= 128: eight accumulators
 *                r[j] = a[j]; for i = 8, 16, ... while i < n - n % 8: r[j] += a[i + j]; then
 *                ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the n % 8 tail, added sequentially.  n > 128: split at
 *                n2 = n / 2 - (n / 2) % 8, sum(left) + sum(right), recursively.  dim 384 = four pieces of 96;
 *   sqrt, divide correctly rounded (HIP's default; the library does not turn it off);
 *   max          numpy's maximum: a NaN norm stays NaN and makes the row NaN (fmaxf would drop it).  eps is the caller's
 *                float32 (the encoder's: float32(1e-12));
 *   edges        an Inf norm gives 0 (signed) for finite elements and NaN for infinite ones; a zero row stays zero;
 *                denormal squares and quotients are kept, as numpy on x86 keeps them.
 * d_needs_host (may be NULL) int32 [n_queries]: row q is written as ZEROS where d_needs_host[q] != 0, so that K1 runs on a
 * defined vector; the caller replaces that query's answer.  d_out == d_rows is allowed (a row is read in full before it is
 * written).  n_queries 0 .. 65535 (0 does nothing), dim 1 .. 8192 (what rr_index_create accepts): outside that, a NULL
 * d_rows / d_out or a NaN eps is RR_E_INVALID with nothing launched.  A wave per query, one launch, no scratch memory; the
 * pointers belong to the CURRENT device.  Asynchronous on `stream`. */
int rr_query_vectors_dev(const float* d_rows, int32_t n_queries, int32_t dim, float eps, const int32_t* d_needs_host,
                         float* d_out, void* stream);
/* d_needs_host[q] |= bit where d_src[q] != 0 (both int32 [n_queries], n_queries 0 .. 65535; bit = one bit, 1 .. 2^30).  How
 * the flags of a SECOND rr_wp_encode_dev over the batch -- the query encoder's vocabulary -- join the front call's: bit
 * 32 = the query encoder's WordPiece kernel handed the query back (its sequence is the placeholder [CLS] [SEP], its vector
 * zeros).  Queue it after the front call on the same stream.  Asynchronous on `stream`. */
int rr_query_flag_dev(const int32_t* d_src, int32_t n_queries, int32_t bit, int32_t* d_needs_host, void* stream);

/* ------------------------------------------------------------ IR metrics of a batch's answer (csrc/rr_evals.hip) */

/* What evals/performance_metrics.py:162-205 (IRMetrics.evaluate_query) computes from a ranked sku list, for a whole batch
 * from K3's outputs where they lie: retrieved row j of query b is d_out_rows[b][d_order[b][j]] (d_out_rows int64
 * [nq x pool], d_order int32 [nq x k] pool positions, best first -- what rr_fuse_topk_dev wrote; K3 returns distinct rows,
 * so the reference's set intersection is a count).  evals.model_ir_metrics states the same in numpy.
 * THE LABELS, a CSR over the queries: d_lab_off int64 [nq + 1]; d_lab_row int64 [n_labels] global rows, ascending inside a
 * query (only labelled skus the index holds have an entry); d_lab_grade float64 = the sku's relevance_scores value (1.0 for
 * binary labels); d_lab_rel uint8 = 1 when the sku is in relevant_items (the two differ when a caller passes both).
 * n_labels = d_lab_off[nq] as the host knows it: a segment is cut to [0, n_labels), so no label array is read outside it;
 * with n_labels = 0 the three label arrays may be NULL.  An empty segment is legal.
 * PER-QUERY TABLES, the labels' alone (made once per query set on the host): d_n_rel int32 [nq] = len(relevant_items),
 * skus absent from the index included (the reference's recall counts them); d_idcg float64 [nq x 2] = IDCG@5 and IDCG@10 of
 * the sorted relevance_scores values, absent skus included.  d_log2 float64 [10] = numpy's log2(arange(1, 11) + 1), uploaded
 * (the device's log2 is not numpy's bit for bit).
 * d_metrics float64 [nq x 8]: ndcg@5, ndcg@10, mrr, recall@10, recall@20, precision@5, precision@10, first_hit -- to the bit
 * what the reference computes:
 *   DCG@c       L = min(c, k) terms t_i = grade_i / d_log2[i] (unlabelled rows: grade 0.0), one IEEE division each, added in
 *               numpy's order for a contiguous float64 sum: L < 8 left to right from 0.0; 8 <= L <= 10
 *               ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)), then + t8, then + t9;
 *   nDCG@c      dcg / idcg, 0.0 when idcg == 0.0;
 *   first_hit   the 1-based rank of the first retrieved row whose d_lab_rel is 1 among ALL k, 0.0 when there is none;
 *               mrr = 1.0 / first_hit, 0.0 with no hit;
 *   recall@c    hits(min(c, k)) / n_rel, 0.0 when n_rel == 0; precision@c = hits(min(c, k)) / min(c, k); hits count
 *               d_lab_rel, not grades.
 * d_mean float64 [8] or NULL: the column means over the nq queries, from a second launch behind the first: fixed-order
 * float64 sums without floating-point atomics (two runs give the same bits), within nq * 2^-52 relative of any other order.
 * nq >= 1, 1 <= k <= pool <= RR_MAX_POOL; outside that or with a NULL argument RR_E_INVALID and nothing is launched.  A
 * d_order entry outside [0, pool) names no row (it counts as unlabelled).  A wave per query; the pointers belong to the
 * CURRENT device.  Asynchronous on `stream`; no scratch memory, nothing read back. */
int rr_ir_metrics_dev(const int64_t* d_out_rows, const int32_t* d_order, int32_t nq, int32_t pool, int32_t k,
                      const int64_t* d_lab_off, const int64_t* d_lab_row, const double* d_lab_grade, const uint8_t* d_lab_rel,
                      int64_t n_labels, const int32_t* d_n_rel, const double* d_idcg, const double* d_log2,
                      double* d_metrics, double* d_mean, void* stream);
/* The column means alone: d_mean float64 [8] of a d_metrics table of nq >= 1 rows (a query set that went through
 * rr_ir_metrics_dev in several batches, each into its rows of one table).  The launch rr_ir_metrics_dev makes for a d_mean. */
int rr_ir_mean_dev(const double* d_metrics, int32_t nq, double* d_mean, void* stream);

/* Two-phase K1 for ROW SHARDS (sharded.py: one process per GPU, this shard's rows in `ix`).  A shard's
 * own top-`top_k` threshold sits far below the corpus-wide one (rank 150 of 1.25M rows ~ rank 1 200 of 10M), so a shard
 * that selects on its own rescoring ~8x the candidates the merged answer needs.  Instead:
 *   1. rr_dense_scan_dev: the scan of rr_dense_topk_dev without its selection; d_bound[q] (device, n_queries floats) =
 *      a lower bound of the score of this shard's `kth`-best row (kth = ceil(top_k / shards)), or -inf;
 *   2. the caller takes the MINIMUM of d_bound over the shards (one all-reduce of n_queries floats): the union of the
 *      shards' kth best rows holds >= top_k rows, so that minimum is a lower bound of the corpus-wide top_k-th best score;
 *   3. rr_dense_select_dev: the selection, opening nothing that cannot reach that floor.  Its lists still hold top_k
 *      rows per query -- every row of the corpus-wide top-k that lives in this shard, filled up with other exactly
 *      scored rows of the shard (not necessarily its next best): only the MERGED top-k of all shards is the answer.
 * `*applied` (host) = 0 when the call cannot be split (fewer than 5 or more than 256 queries, 129..192, a small or
 * non-finite matrix, a pinned scan mode): nothing was launched, d_bound is untouched, use rr_dense_topk_dev.  The
 * queries, n_queries and top_k of phase 2 must be those of phase 1, with no other search on `ix` in between.
 * (Replaces nothing in the reference: utils.py:111-124 is single-process.) */
int rr_dense_scan_dev(rr_index* ix, const float* d_queries, int32_t n_queries, int32_t top_k, int32_t kth,
                      float* d_bound, int32_t* applied, void* stream);
int rr_dense_select_dev(rr_index* ix, const float* d_queries, int32_t n_queries, int32_t top_k,
                        const float* d_floor, int64_t* d_out_rows, float* d_out_scores, void* stream);

/* PIPELINED K1 ("keep K1 -> K2-gather -> allgather -> K3 on-stream ... pipeline batches"): the same two
 * phases with an explicit SCAN SLOT (0, 1 or 2).  A slot holds what one batch's scan writes and its selection reads (staged
 * queries, their bf16 planes and error bounds, tile / group maxima, the parked phase-1 state); the index has three, so batch
 * i + 1 can be scanned into one slot on one stream while batch i's selection (then K2, K3 and the answer's copy) reads the
 * other on ANOTHER stream.  The library orders scan and selection of a slot with events (a scan waits for the slot's
 * previous selection, a selection for its scan and for the previous selection's use of the shared rescoring scratch);
 * calls on one handle stay serialised on the host.  kth = 0 with d_bound = NULL: no bound is computed (single GPU);
 * d_floor may be NULL (the shard selects on its own threshold).  rr_dense_scan_dev / rr_dense_select_dev above are
 * slot 0; every other search entry point uses slot 0 and voids a scan parked there.
 * The scan kernel keeps one 512-register wave on every SIMD of a CU it runs on, so a second stream only makes progress on
 * CUs the scan does not hold: give the scans a stream masked to part of the device (rr_stream_create_cu_range), tell the
 * index how many CUs that is (rr_index_set_scan_cus: every scan's resident grid is sized for it), and run the selections
 * on a stream masked to the rest.  (Replaces nothing in the reference: utils.py:111-124 is one blocking call.) */
int rr_dense_scan_slot_dev(rr_index* ix, int32_t slot, const float* d_queries, int32_t n_queries, int32_t top_k, int32_t kth,
                           float* d_bound, int32_t* applied, void* stream);
int rr_dense_select_slot_dev(rr_index* ix, int32_t slot, int32_t n_queries, int32_t top_k, const float* d_floor,
                             int64_t* d_out_rows, float* d_out_scores, void* stream);
/* rr_dense_topk_dev in a given scan slot (rr_dense_topk_dev itself = slot 0): the whole K1 of a batch the pipeline cannot
 * split (`applied` = 0), without disturbing the scans other batches have parked in the other slots. */
int rr_dense_topk_slot_dev(rr_index* ix, int32_t slot, const float* d_queries, int32_t n_queries, int32_t top_k,
                           int64_t* d_out_rows, float* d_out_scores, void* stream);
/* The selection in its three steps, each possibly on a stream of its own (`parts` = any combination, launched in this order):
 *   RR_SELECT_LIST     per query the 8-row M-tiles whose scan bound reaches the threshold (one workgroup per query: latency-
 *                      bound, a few CUs do);
 *   RR_SELECT_RESCORE  the exact per-row scores of the listed M-tiles: a gather of ~3 MB of rows per query (HBM-bound: wants
 *                      the bandwidth of the many CUs -- e.g. the scans' stream, behind the next batch's scan);
 *   RR_SELECT_ORDER    the top_k of the rescored rows into d_out_rows / d_out_scores + the exact fallbacks of flagged queries.
 * Pass the same d_floor (or NULL) to every part of a batch (LIST reads it; the other two only act on whether there is one);
 * the outputs may be NULL unless ORDER is among the parts.  rr_dense_select_slot_dev = all three. */
#define RR_SELECT_LIST    1
#define RR_SELECT_RESCORE 2
#define RR_SELECT_ORDER   4
int rr_dense_select_part_dev(rr_index* ix, int32_t slot, int32_t parts, int32_t n_queries, int32_t top_k, const float* d_floor,
                             int64_t* d_out_rows, float* d_out_scores, void* stream);
/* A hipStream_t (as void*) whose kernels run only on CUs [first_cu, first_cu + n_cus) of `device`, counted in the driver's
 * CU-mask order (bit i sits on XCD i % 8: a contiguous range takes the same share of every XCD).  n_cus should be a multiple
 * of 32 (the dispatcher deals workgroups to the 32 shader engines in turn).  It is an ordinary BLOCKING stream: commands on
 * the NULL stream synchronise with it -- keep other work off the NULL stream while it is in use.  Destroy with
 * rr_stream_destroy before the process ends. */
int rr_stream_create_cu_range(int32_t device, int32_t first_cu, int32_t n_cus, void** out_stream);
int rr_stream_destroy(void* stream);
/* How many CUs the stream of this index's scans may use (0 or the device's CU count = all). */
int rr_index_set_scan_cus(rr_index* ix, int32_t n_cus);

/* Stream helpers for callers that chain *_dev calls. */
int rr_index_stream(rr_index* ix, void** out_stream);
int rr_index_synchronize(rr_index* ix);

#ifdef __cplusplus
}
#endif
#endif /* RR_HIP_H */
