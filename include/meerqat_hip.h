/*
 * meerqat_hip.h -- C ABI of libmeerqat_hip.so, the MI355X (gfx950) implementation of the
 * arithmetic that PaulLerner/ViQuAE's dense-retrieval path delegates to FAISS and Hugging Face.
 *
 * The reference has no FFI of its own (it is pure Python); every entry point below names the
 * reference call site whose arithmetic it replaces.  Conventions:
 *   - plain pointers and sizes only, no C++/torch types; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream);
 *   - every `*_dev` / device pointer is HBM memory owned by the CALLER (the Python host allocates
 *     through torch); nothing is allocated, freed or retained across calls;
 *   - return value: MQ_OK (0) or a negative MQ_E* code; no exceptions cross the boundary;
 *     kernels are enqueued on `stream` and NOT synchronised (results are valid after the caller
 *     synchronises the stream);
 *   - re-entrant per stream.  The library keeps no state about a caller's data; what it does keep
 *     is process-wide bookkeeping that never changes a result: the last HIP error code of the
 *     calling THREAD (thread-local, mq_last_hip_error()), the CU count of the device (read once),
 *     one "dynamic-LDS limit raised" bit per (kernel, device), and the MQ_KNN_QPX tuning knob read
 *     from the environment once.  No environment variable is ever turned into a pointer in this
 *     build (cycle-accounting builds compiled with -DMQ_TIMING are a developer tool).
 */
#ifndef MEERQAT_HIP_H
#define MEERQAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MQ_OK 0
#define MQ_EINVAL (-1)     /* bad argument (NULL pointer, non-positive size, unsupported k, ...) */
#define MQ_EWORKSPACE (-2) /* workspace too small */
#define MQ_EHIP (-3)       /* a HIP runtime call failed; see mq_last_hip_error() */
#define MQ_EUNSUPPORTED (-4)

#define MQ_METRIC_IP 0 /* faiss.METRIC_INNER_PRODUCT, "metric_type": 0 in experiments/ir/..../search/config.json */
#define MQ_METRIC_L2 1 /* faiss.METRIC_L2 (FAISS default when metric_type is None) */
/* Accepted by the mq_knn_screen_* entries, mq_knn_search_screened_f32, mq_knn_workspace_bytes_metric and mq_knn_screen_scan_kind only:
 * the inner product served by the CENTRED-QUERY screen (round 5).  With c the centre of the bf16 copy, q.x = (q - c).(x - c) +
 * c.(x - c) + q.c: the rows of a query rank by (q - c).(x - c) plus the per-row term c.(x - c), which the copy carries in two extra
 * columns like the L2 metric's -||x||^2 / 2; the rounding error -- hence the margin, hence the candidates per query -- then follows
 * the spread of the scores even when every vector shares a large common component (image features).  Results are the plain inner
 * product's, bit for bit (the screen is a lossless filter either way).  The index is built with this code (screen_bytes /
 * prepare / add_rows: a centre is required) and searched with it; xstats_dev then holds 4 + d floats: the four statistics, then
 * the centre. */
#define MQ_METRIC_IP_CENTRED 2

/* `--k` is a user option of the reference (meerqat/ir/search.py:12,135; default 100) and faiss IndexFlat takes any k.  One
 * fused scan keeps up to MQ_KNN_FUSED_K neighbours; a larger k (up to MQ_KNN_MAX_K, FAISS-GPU's own limit) is served by
 * ceil(k / 128) scans, round r + 1 admitting only candidates strictly below the last (score, id) key of round r -- the
 * rounds' results concatenate into the exact sorted top-k.  The rounds are exact fp32 scans; mq_knn_search_screened_f32 serves
 * k <= 224 through its screen and 225 <= k <= 1792 through the screen over ceil(k / 112) contiguous ROW RANGES whose top-224 lists
 * are merged -- the merge proves the union's top-k (no range delivered its whole list into it) or hands the query tile to the
 * rounds -- same results either way; it takes the rounds beyond 1792 and on shards too small for ranges (< 16,384 rows each). */
#define MQ_KNN_FUSED_K 128
#define MQ_KNN_MAX_K 2048

/* `flags` of the search entry points (the argument was `l2norm_queries`, 0 / 1, before the tie order became a parameter):
 *   MQ_KNN_FLAG_L2NORM_QUERIES  apply the index's "L2norm," transform to the queries first;
 *   MQ_KNN_FLAG_TIE_ID_DESC     among EXACTLY equal scores the HIGHER id is the better one -- for membership at the k-th
 *                               boundary and for the order of the output alike.  Default (bit clear): the LOWER id is better.
 * Which of several exactly tied rows FAISS keeps and in which order it reports them depends on its version and on k
 * (value-only heaps before 1.7.3, cmp2(val, id) heaps since, a reservoir + partition at k >= 100; oracle/knn_oracle.c
 * states what is known): both orders here are THIS LIBRARY'S documented policies, neither is a claim about FAISS.
 * mq_topk_merge_*: OR MQ_MERGE_TIE_ID_DESC into `metric` to merge shard results produced with MQ_KNN_FLAG_TIE_ID_DESC. */
#define MQ_KNN_FLAG_L2NORM_QUERIES 1
#define MQ_KNN_FLAG_TIE_ID_DESC 2
#define MQ_KNN_FLAG_L2NORM_FAISS 4 /* the query transform in FAISS's arithmetic (below); implies MQ_KNN_FLAG_L2NORM_QUERIES */
/* mq_knn_search_screened_f32 only: one search issued as two calls with the SAME arguments and workspace, so that a caller
 * searching several query chunks can put the short second half of chunk i (candidates -> exact re-scoring -> exact top-k ->
 * recomputation of flagged tiles) on another stream, under the scan of chunk i+1 (which then needs its own workspace):
 *   MQ_KNN_FLAG_PHASE_FRONT  query preparation + the screening scan only (D, I are not written yet);
 *   MQ_KNN_FLAG_PHASE_TAIL   everything after the scan, from the workspace the FRONT call filled (the caller orders the two:
 *                            the TAIL stream waits for an event recorded after the FRONT call).
 * Neither bit or both: the whole search in one call.  Searches the screen does not serve (k beyond its range, FAISS's small
 * L2 batches) run entirely in the FRONT call; their TAIL call returns MQ_OK without work.  Results are those of the
 * one-call search, bit for bit. */
#define MQ_KNN_FLAG_PHASE_FRONT 8
#define MQ_KNN_FLAG_PHASE_TAIL 16
#define MQ_MERGE_TIE_ID_DESC 0x100

/* The two arithmetics of the "L2norm," prefix -- the `l2norm` argument of mq_pack_rows_f32 / mq_knn_screen_add_rows_f32 (0 = no
 * transform), the `form` of mq_l2norm_rows_form_f32, and MQ_KNN_FLAG_L2NORM_FAISS for the queries of a search:
 *   MQ_L2NORM_NUMPY  x / sqrtf(sum x^2): the reference's L2norm() (meerqat/ir/search.py:43-46), which it also applies to the KB
 *                    column itself when `device` is given (its GPU work-around, :238-244).  A zero row becomes NaN.
 *   MQ_L2NORM_FAISS  FAISS's NormalizationTransform -> fvec_renorm_L2 (faiss/utils/distances.cpp, as published): when
 *                    nr = sum x^2 > 0, x *= (float)(1.0 / sqrtf(nr)) -- one double reciprocal per row rounded to float, one
 *                    multiplication per element; a row with nr not > 0 (zero, underflowed, NaN) stays as it is (a zero row
 *                    remains retrievable with score 0).  What "L2norm,Flat" computes with `device: null`, i.e. in every shipped
 *                    config (:230-245): for the KB rows on add and, inside the index, for the (already host-normalised) queries.
 * In both forms sum x^2 is the k-ordered fp32 fma chain (FAISS's SIMD summation order is not knowable here: parity unpinned). */
#define MQ_L2NORM_NUMPY 1
#define MQ_L2NORM_FAISS 2

/* faiss::distance_compute_blas_threshold.  A METRIC_L2 search of FEWER queries than this takes FAISS's
 * sequential path: distances are the direct sums of (q[k] - x[k])^2 (faiss fvec_L2sqr), not the BLAS form
 * ||q||^2 + ||x||^2 - 2<q,x> clamped at 0 that larger batches get (faiss/utils/distances.cpp, knn_L2sqr).
 * Both search entries below switch form on the `nq` of the CALL, so a host that cuts a large batch into
 * several calls must not leave a piece of fewer than 20 queries (viquae_amd.index.query_chunks). */
#define MQ_KNN_L2_DIRECT_BELOW 20

const char *mq_version(void);
const char *mq_strerror(int code);
int mq_last_hip_error(void);

/* ---------------------------------------------------------------------------------------------
 * KB matrix in HBM: the "panel" layout.  Replaces faiss IndexFlat's row-major storage filled by
 * FaissIndex.add_vectors (datasets/search.py:255-313, reached from meerqat/ir/search.py:245).
 * Row i, component k lives at   packed[((i / 64) * dpad + k) * 64 + (i % 64)],
 * dpad = d rounded up to 16, rows padded (zero) to a multiple of 256.
 * ------------------------------------------------------------------------------------------- */
int64_t mq_padded_rows(int64_t n_rows);
int mq_padded_dim(int d);
size_t mq_packed_bytes(int64_t n_rows, int d);

/* Pack `n` row-major fp32 rows (device) into the panel buffer at rows [row_offset, row_offset+n).
 * l2norm != 0 applies FAISS's "L2norm," NormalizationTransform (string_factory "L2norm,Flat",
 * meerqat/ir/search.py:230-233) to each row first.  sqnorm_dev[row] receives ||x||^2 of the stored
 * row (used by the L2 metric).  capacity_rows = mq_padded_rows(total rows) of the destination;
 * the caller zero-fills the panel buffer once before the first call. */
int mq_pack_rows_f32(const float *rows_dev, int64_t n, int d, int64_t row_offset, int l2norm, float *packed_dev,
                     int64_t capacity_rows, float *sqnorm_dev, void *stream);

/* Inverse of mq_pack_rows_f32 (FaissIndex.save / reconstruct, datasets/search.py:387-397). */
int mq_unpack_rows_f32(const float *packed_dev, int64_t capacity_rows, int d, int64_t row_offset, int64_t n,
                       float *rows_dev, void *stream);

/* In-place row L2 normalisation of a row-major [n,d] device matrix: L2norm(), meerqat/ir/search.py:43-46. */
int mq_l2norm_rows_f32(float *rows_dev, int64_t n, int d, void *stream);                     /* MQ_L2NORM_NUMPY */
int mq_l2norm_rows_form_f32(float *rows_dev, int64_t n, int d, int form, void *stream);      /* form: MQ_L2NORM_NUMPY | MQ_L2NORM_FAISS */

/* ---------------------------------------------------------------------------------------------
 * Exact brute-force top-k: replaces faiss IndexFlat.search behind FaissIndex.search_batch
 * (datasets/search.py:369-385), called by KnowledgeBase.search_batch (meerqat/ir/search.py:146).
 *   packed_dev/sqnorm_dev : the KB shard (N rows) as written by mq_pack_rows_f32
 *   queries_dev           : [nq, d] row-major fp32
 *   metric                : MQ_METRIC_IP or MQ_METRIC_L2
 *   flags                 : MQ_KNN_FLAG_* (above); 0 or 1 mean what `l2norm_queries` meant
 *   id_offset             : added to every returned row id (global id of the shard's row 0)
 *   D_dev [nq,k] fp32, I_dev [nq,k] int64: best first; equal scores by ascending id (descending with
 *                           MQ_KNN_FLAG_TIE_ID_DESC); unfilled slots are (-FLT_MAX | +FLT_MAX, -1): FAISS's heap
 *                           neutral values (CMin::neutral() / CMax::neutral()), what it reports when k > ntotal
 *   ws_dev/ws_bytes       : scratch of at least mq_knn_workspace_bytes_metric(N, d, nq, k, metric)
 * Scores are the k-ordered fp32 fma chain (see oracle/knn_oracle.c); selection is exact.
 * mq_knn_workspace_bytes covers either metric; the _metric variant leaves out what an inner-product search never touches
 * (the [nq][N] distance matrix of FAISS's small-batch L2 form: 114 MB per 1.5M-row shard at 19 queries).
 * ------------------------------------------------------------------------------------------- */
size_t mq_knn_workspace_bytes(int64_t N, int d, int nq, int k);
size_t mq_knn_workspace_bytes_metric(int64_t N, int d, int nq, int k, int metric);
int mq_knn_search_f32(const float *packed_dev, const float *sqnorm_dev, int64_t N, int d, const float *queries_dev,
                      int nq, int k, int metric, int flags, int64_t id_offset, float *D_dev,
                      int64_t *I_dev, void *ws_dev, size_t ws_bytes, void *stream);

/* Same call; additionally records the caller's hipEvent_t handles (may be NULL) on `stream`
 * immediately before and after the scan kernel (knn_scan_kernel), so that a benchmark can time the
 * dominant kernel on the stream it is launched on. */
int mq_knn_search_f32_ev(const float *packed_dev, const float *sqnorm_dev, int64_t N, int d, const float *queries_dev,
                         int nq, int k, int metric, int flags, int64_t id_offset, float *D_dev,
                         int64_t *I_dev, void *ws_dev, size_t ws_bytes, void *stream, void *ev_scan_begin,
                         void *ev_scan_end);

/* ---------------------------------------------------------------------------------------------
 * Screened search: SAME exact result as mq_knn_search_f32 (both metrics), computed as a bf16
 * screening scan over a bf16 copy of the shard + exact fp32 re-scoring of the few survivors
 * (csrc/knn_screen.inc states the error bound that makes the screen lossless).  For MQ_METRIC_L2 the bf16 copy carries
 * two extra columns, the bf16 pair of -||x||^2/2 (queries get 1, 1), so that the same scan ranks by q.x - ||x||^2/2.
 * The bf16 copy is metric-specific: pass the same `metric` to the three calls.  Extra shard buffers:
 *   rowmajor_dev [N, d] fp32  : the stored rows in row-major order (re-scoring operand)
 *   bf16_dev                  : mq_knn_screen_bytes(N, d, metric) bytes, bf16 copy (rows padded to 256, d (+2) to 64); an
 *                               opaque buffer owned by these three calls -- stored tile by tile ([row / 256][col / 64][256][64]:
 *                               one K step's operand is one contiguous 32-KiB block), a prefix of the rows is a prefix of it
 *   xstats_dev                : FOUR floats kept by mq_knn_screen_prepare (zero them before its first call):
 *                               max ||x||^2, max ||xc - bf16(xc)||^2, max ||xc||^2 and max |c . xc| over the shard (xc = x -
 *                               centre c), the inputs of the error bound; under MQ_METRIC_IP_CENTRED 4 + d floats: the
 *                               caller stores the centre behind the statistics, where the search reads it
 *   center_dev                : NULL, or d floats subtracted from every row before the bf16 rounding (both metrics;
 *                               ANY fixed vector is valid: q.(x - c) ranks the rows of a query like q.x, and for
 *                               embeddings with a large shared component the screen's margin then follows ||x - c||);
 *                               the same vector must be passed for every row range of a shard
 * mq_knn_screen_prepare fills rowmajor/bf16 for rows [row_offset, row_offset+n) from the panel buffer.
 * mq_knn_screen_add_rows_f32 does the same straight from incoming rows (row-major [n, d], any row_offset), applying the
 * optional "L2norm," transform and writing ||x||^2 with mq_pack_rows_f32's arithmetic -- for a shard that keeps NO panel copy
 * (1.5x the matrix in HBM instead of 2.5x): mq_knn_search_screened_f32 then takes packed_dev = NULL.
 * Query tiles whose bounded candidate buffers overflow are recomputed by the exact scan inside the
 * same call (from the panel copy, or from the row-major copy when packed_dev is NULL: same MFMA sequence, same bits, a
 * slower operand path); FAISS's small-batch L2 form (MQ_KNN_L2_DIRECT_BELOW) likewise reads whichever copy exists.
 * Workspace: mq_knn_workspace_bytes (covers all paths).  The bounded screening buffers are sized for the reference's k = 100 and hold
 * up to k = 224; 225 <= k <= 1792 runs the screen per row range and merges (above; 1.5M x 768, 4096 queries: k = 100 / 224 / 256 / 512 /
 * 1024 / 1792 = 8.6 / 10.4 / 14.3 / 17.7 / 25.6 / 32.8 ms, where ceil(k / 128) exact rounds took 147 ms at k = 256 and 294 ms at 512);
 * MQ_KNN_PARTITIONS=0 or k > 1792: the exact rounds.
 * ------------------------------------------------------------------------------------------- */
size_t mq_knn_screen_bytes(int64_t n_rows, int d, int metric);
int mq_knn_screen_prepare(const float *packed_dev, const float *sqnorm_dev, int64_t capacity_rows, int d, int metric,
                          int64_t row_offset, int64_t n, float *rowmajor_dev, uint16_t *bf16_dev, float *xstats_dev,
                          const float *center_dev, void *stream);
int mq_knn_screen_add_rows_f32(const float *rows_dev, int64_t n, int d, int64_t row_offset, int l2norm, int metric,
                               int64_t capacity_rows, float *sqnorm_dev, float *rowmajor_dev, uint16_t *bf16_dev,
                               float *xstats_dev, const float *center_dev, void *stream);
int mq_knn_search_screened_f32(const float *packed_dev, const float *sqnorm_dev, const float *rowmajor_dev,
                               const uint16_t *bf16_dev, const float *xstats_dev, int64_t N, int d,
                               const float *queries_dev, int nq, int k, int metric, int flags, int64_t id_offset,
                               float *D_dev, int64_t *I_dev, void *ws_dev, size_t ws_bytes, void *stream,
                               void *ev_scan_begin, void *ev_scan_end);
/* Telemetry of the last screened search held in ws_dev (synchronises the stream): out[0] = query
 * tiles recomputed by the exact scan, out[1] = candidates re-scored in total, out[2] = max per query,
 * out[3] / out[4] = max / total slab-pool entries, out[5] = max margin (1e-6 units), out[6] = slabs. */
int mq_knn_screen_stats(int64_t N, int d, int nq, int k, const void *ws_dev, int64_t out[8], void *stream);
/* Which screening scan mq_knn_search_screened_f32 runs for this problem on this device: the 256 x 256 tile kernel
 * (screen_scan_kernel) or, for ONE query tile (nq <= 256 -- the reference's Dataset.map batch,
 * experiments/ir/viquae/dpr/search/config.json:25 -> meerqat/ir/search.py:146) over a shard of at least 65,536 rows with at
 * most 768 bf16 columns and k <= 128, the streaming kernel that keeps the queries in registers (csrc/knn_small8.inc).
 * For 225 <= k <= 1792 the answer describes the scan of one row range.
 * MQ_SCAN_KIND_NONE: the call is not served by a screening scan at all (k > 1792 or row ranges too small: exact rounds; fewer
 * than 20 L2 queries: FAISS's direct form).  Negative: MQ_EINVAL.  MQ_KNN_OPT_SMALL_SCAN = 0 (below) switches the streaming kernel
 * off, MQ_KNN_OPT_SMALL_MIN_TILES = <n> sets its floor of 32-row tiles per workgroup (default 8). */
#define MQ_SCAN_KIND_NONE 0
#define MQ_SCAN_KIND_TILE 1
#define MQ_SCAN_KIND_STREAM 2
int mq_knn_screen_scan_kind(int64_t N, int d, int nq, int k, int metric);
/* Process-wide A/B switches of the search paths.  Their first values come from the environment, read ONCE (MQ_KNN_SMALL,
 * MQ_KNN_SMALL_MIN_TILES, MQ_KNN_PARTITIONS, MQ_KNN_SCAN_MFMA); a running process flips them with mq_knn_set_option (atomic; a search already in
 * its planning step may still see the old value), never by editing the environment.  Values are >= 0.
 *   MQ_KNN_OPT_SMALL_SCAN        1 (default): one query tile may be served by the streaming kernel; 0: always the tile kernel
 *   MQ_KNN_OPT_SMALL_MIN_TILES   the streaming kernel's floor of 32-row tiles per workgroup; 0 (default) = the built-in 8
 *   MQ_KNN_OPT_PARTITIONS        1 (default): 225 <= k <= 1792 is served over row ranges; 0: exact rounds
 *   MQ_KNN_OPT_SMALL_WAVES       retired (it chose round 4's one-wave-per-SIMD streaming kernel, since removed): still accepted
 *                                and stored, 8 at start, read by nothing -- kept so that old callers do not break
 *   MQ_KNN_OPT_SCAN_MFMA         the tile kernel's matrix instruction, for measuring one against the other in one process:
 *                                0: v_mfma_f32_32x32x16_bf16, 1 (default): v_mfma_f32_16x16x32_bf16 -- same pools, same results,
 *                                the chip holds a higher clock under the second (profiles/r07_notes.md); first value from
 *                                MQ_KNN_SCAN_MFMA, else MQ_KNN_SCAN_MFMA_DEFAULT.  The 32x32x16 instance stays for one release
 *                                as the A/B twin
 * mq_knn_set_option returns the previous value, mq_knn_get_option the current one; MQ_EINVAL for an unknown key / negative value. */
#define MQ_KNN_OPT_SMALL_SCAN 0
#define MQ_KNN_OPT_SMALL_MIN_TILES 1
#define MQ_KNN_OPT_PARTITIONS 2
#define MQ_KNN_OPT_SMALL_WAVES 3
#define MQ_KNN_OPT_SCAN_MFMA 4
#define MQ_KNN_OPT_COUNT 5
#define MQ_KNN_SCAN_MFMA_DEFAULT 1
int mq_knn_set_option(int key, int value);
int mq_knn_get_option(int key);

/* Name and launch geometry of the scan kernel for the given problem (for bench.py / profiles):
 * out[0]=workgroups, out[1]=threads per workgroup, out[2]=LDS bytes (exact scan), out[3]=query tiles,
 * out[4]=KB slabs, out[5]=KB chunks (256 rows each), out[6]/out[7]=threads / LDS bytes of the screening scan. */
int mq_knn_launch_info(int64_t N, int d, int nq, int k, int64_t out[8]);

/* Merge per-shard results after the all-gather (new step; no reference
 * counterpart): Ds/Is [nshards, nq, k] with GLOBAL ids -> the k best per query.  metric: MQ_METRIC_IP / MQ_METRIC_L2,
 * optionally OR-ed with MQ_MERGE_TIE_ID_DESC; any k <= MQ_KNN_MAX_K. */
int mq_topk_merge_f32(const float *Ds_dev, const int64_t *Is_dev, int nshards, int nq, int k, int metric,
                      float *D_dev, int64_t *I_dev, void *stream);

/* The same merge over the buffer ONE all-gather delivers ("one RCCL all-gather of
 * (score f32, id i64)[nq,k] per rank").  A rank's record is mq_shard_record_bytes(nq, k) bytes:
 *   [0, nq*k*4)                                   fp32 scores [nq,k]
 *   [mq_shard_record_ids_offset(nq,k), + nq*k*8)  int64 GLOBAL ids [nq,k]
 * (offsets rounded so that ids are 8-byte and records 16-byte aligned).  A shard's search writes D / I
 * straight into its record (D_dev = record, I_dev = record + ids offset), the collective concatenates the
 * records rank-major, and records_dev = that [nshards * record_bytes] buffer (8-byte aligned). */
size_t mq_shard_record_bytes(int nq, int k);
size_t mq_shard_record_ids_offset(int nq, int k);
int mq_topk_merge_records_f32(const void *records_dev, int nshards, int nq, int k, int metric, float *D_dev,
                              int64_t *I_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder building blocks (fp32): the arithmetic of Hugging Face DPRContextEncoder /
 * DPRQuestionEncoder (reached from meerqat/ir/embedding.py:226; op order stated in-tree by
 * meerqat/models/bert.py:12-380) and CLIPModel.get_image_features (meerqat/image/embedding.py:156-161).
 * Activations are row-major fp32 [tokens, features]; weights keep nn.Linear's [out, in] layout.
 * ------------------------------------------------------------------------------------------- */
#define MQ_EPI_NONE 0           /* C = A.W^T                       (CLIP patch embedding, visual projection) */
#define MQ_EPI_BIAS 1           /* C = A.W^T + b                   (Q/K/V projections)                        */
#define MQ_EPI_BIAS_GELU 2      /* C = gelu_erf(A.W^T + b)         (BertIntermediate, bert.py:217-229)         */
#define MQ_EPI_BIAS_QUICKGELU 3 /* C = x*sigmoid(1.702x), x=A.W^T+b (CLIP MLP fc1)                            */
#define MQ_EPI_BIAS_RESIDUAL 4  /* C = A.W^T + b + R               (BertSelfOutput/BertOutput dense + input)  */

/* A/B switch of the split-bf16 GEMM kernels (both give bit-identical outputs).  First value from the environment, read ONCE
 * (MQ_GEMM_WIDE); a running process flips it with mq_gemm_set_option (atomic), which returns the previous value (MQ_EINVAL for an
 * unknown key).
 *   MQ_GEMM_OPT_WIDE   1 (default): eight waves of 128 x 64 outputs, two per SIMD, fragments prefetched across the mid-step
 *                      barrier, a two-step LDS-DMA lookahead that runs across tile boundaries (csrc/gemm_x3w.inc, round 6);
 *                      0: sixteen waves of 64 x 64 (gemm_nt_x3s_kernel, rounds 2-5).
 *   MQ_GEMM_OPT_STAGGER  (eight-wave kernel) start offset between the four phases of workgroups, in units of 1024 shader
 *                      clocks; 0 = all workgroups start together.  Environment: MQ_GEMM_STAGGER */
#define MQ_GEMM_OPT_WIDE 0
#define MQ_GEMM_OPT_STAGGER 1
#define MQ_GEMM_OPT_COUNT 2
int mq_gemm_set_option(int key, int value);

/* nn.Linear with a fused epilogue: A [M,K], W [N,K], bias [N] or NULL, R [M,N] or NULL, C [M,N].
 * K must be a multiple of 16; A and W 16-byte aligned. */
int mq_gemm_nt_f32(const float *A_dev, const float *W_dev, const float *bias_dev, const float *residual_dev,
                   float *C_dev, int M, int N, int K, int epilogue, void *stream);

/* Split-bf16 variant of mq_gemm_nt_f32: W is given as two bf16 matrices Wh + Wl (mq_split_bf16_f32, once per
 * weight), A stays fp32 and is split in registers; C ~= Ah.Wh + Al.Wh + Ah.Wl with fp32 accumulation --
 * relative error ~1e-5 (fp32-class) at 3/16 of the fp32-MFMA cycles.  K must be a multiple of 32. */
int mq_split_bf16_f32(const float *src_dev, int64_t n, uint16_t *hi_dev, uint16_t *lo_dev, void *stream);
/* The same split of a weight matrix W [N, K] (K a multiple of 32), stored in TILE layout [ceil(N / 256)][K / 32][256][32]
 * (rows beyond N are zeros): the operand of one K step of a GEMM tile is then one contiguous 16-KiB block.  hi / lo hold
 * mq_split_bf16_tiled_elems(N, K) elements each.  Pass such a pair to mq_gemm_nt_bf16x3_f32 / mq_gemm_nt_bf16x3s_f32 with
 * MQ_GEMM_W_TILED or-ed into `epilogue`: same products in the same order, bit-identical results, 3.5-6 % faster GEMMs. */
#define MQ_GEMM_W_TILED 0x100
int64_t mq_split_bf16_tiled_elems(int N, int K);
int mq_split_bf16_tiled_f32(const float *W_dev, int N, int K, uint16_t *hi_dev, uint16_t *lo_dev, void *stream);
int mq_gemm_nt_bf16x3_f32(const float *A_dev, const uint16_t *Wh_dev, const uint16_t *Wl_dev, const float *bias_dev,
                          const float *residual_dev, float *C_dev, int M, int N, int K, int epilogue, void *stream);

/* nn.LayerNorm over the last dimension (C <= 1024); X and Y may alias. */
int mq_layernorm_f32(const float *X_dev, const float *gamma_dev, const float *beta_dev, float *Y_dev, int M, int C,
                     float eps, void *stream);

/* BertEmbeddings (meerqat/models/bert.py:153-214): LayerNorm(word[ids] + type[token_type_ids] + pos[0..L)).
 * ids / token_type_ids are int64 [B,L] (token_type_ids may be NULL = zeros); out [B*L, H]. */
int mq_bert_embed_ln_f32(const int64_t *input_ids_dev, const int64_t *token_type_ids_dev, const float *word_dev,
                         const float *pos_dev, const float *type_dev, const float *gamma_dev, const float *beta_dev,
                         float *out_dev, int B, int L, int H, float eps, void *stream);

/* Multi-head self-attention core (BertSelfAttention.forward, meerqat/models/bert.py:44-136):
 * qkv [B*L, 3*heads*head_dim] = [q | k | v] projections; attention_mask int64 [B,L] (1 = attend, as the
 * tokenizer emits it; NULL = attend everywhere); out [B*L, heads*head_dim] = softmax(q k^T * scale + mask) v.
 * head_dim must be 64; any L (sequences beyond 256 keys are processed in 256-key blocks with the online softmax). */
int mq_attention_f32(const float *qkv_dev, const int64_t *attention_mask_dev, float *out_dev, int B, int L, int heads,
                     int head_dim, float scale, void *stream);

/* CLIPVisionEmbeddings.patch_embedding as a GEMM operand: pixels [B,C,S,S] -> [B*(S/P)^2, C*P*P]. */
int mq_clip_patchify_f32(const float *pixels_dev, float *patches_dev, int B, int channels, int image_size,
                         int patch_size, void *stream);

/* CLIPVisionEmbeddings + pre_layrnorm: out [B*tokens, H] = LayerNorm([class | patch_emb] + position). */
int mq_clip_assemble_ln_f32(const float *patch_emb_dev, const float *class_emb_dev, const float *pos_emb_dev,
                            const float *gamma_dev, const float *beta_dev, float *out_dev, int B, int tokens, int H,
                            float eps, void *stream);

/* CLIPModel.get_text_features (the `call` of experiments/ir/viquae/clip/config.json:15):
 * mq_attention_causal_f32 = mq_attention_f32 with the text tower's causal mask (key <= query) on top of the
 * optional padding mask; mq_clip_text_embed_f32 = token + position embeddings -> out [B*L, H];
 * mq_clip_eos_pool_ln_f32 = final LayerNorm of the hidden state at the end-of-text token of each sequence
 * (eos_token_id == 2, the published checkpoints' legacy config: position of the largest id; otherwise the first
 * position equal to eos_token_id) -> out [B, H]. */
int mq_attention_causal_f32(const float *qkv_dev, const int64_t *attention_mask_dev, float *out_dev, int B, int L, int heads,
                            int head_dim, float scale, int causal, void *stream);
int mq_clip_text_embed_f32(const int64_t *input_ids_dev, const float *token_emb_dev, const float *pos_emb_dev, float *out_dev,
                           int B, int L, int H, void *stream);
int mq_clip_eos_pool_ln_f32(const float *hidden_dev, const int64_t *input_ids_dev, int64_t eos_token_id, const float *gamma_dev,
                            const float *beta_dev, float *out_dev, int B, int L, int H, float eps, void *stream);
/* mq_clip_text_embed_f32 over a PACKED token matrix (the real tokens of right-padded titles, see mq_attention_packed_f32):
 * out[t] = token_emb[input_ids[t]] + pos_emb[position_ids[t]], t < T. */
int mq_clip_text_embed_packed_f32(const int64_t *input_ids_dev, const int32_t *position_ids_dev, const float *token_emb_dev,
                                  const float *pos_emb_dev, float *out_dev, int T, int H, void *stream);

/* Split activations: a tensor that only feeds GEMMs is kept as its (hi, lo) bf16 pair (hi = bf16(x), lo = bf16(x - hi),
 * two uint16 arrays of the tensor's shape), written by the kernel that produces it, so that the consuming GEMM streams
 * bf16 operands and converts nothing in its MFMA loop.  Results are bit-identical to the fp32-activation entry points.
 *   mq_gemm_nt_bf16x3s_f32     mq_gemm_nt_bf16x3_f32 with A given as (Ah, Al); output EITHER fp32 C OR the pair (Ch, Cl)
 *   mq_layernorm_split_f32     mq_layernorm_f32 writing Y (fp32, may be NULL) and/or the pair (Yh, Yl)
 *   mq_bert_embed_ln_split_f32 mq_bert_embed_ln_f32 writing fp32 and, optionally, the pair
 *   mq_attention_split_f32     mq_attention_causal_f32 writing fp32 (may be NULL) and/or the pair; bf16x3 != 0 computes
 *                              q.k and p.v as three-term split-bf16 products on the bf16 matrix pipe (fp32-class accuracy)
 *                              A sequence whose attention_mask row has no live key (all zeros) attends UNIFORMLY to all its
 *                              L keys -- every context row is the mean of its L value rows -- as Hugging Face BERT does by
 *                              adding finfo.min to the logits; every other sequence keeps its bits.  causal != 0 together with
 *                              such a row is undefined.  (The same holds for mq_attention_f32 / mq_attention_causal_f32.)
 * PAIR LAYOUT: the two arrays of a pair [M, K] are stored tile by tile -- element (row, col) at
 * [row / 256][col / 32][row % 256][col % 32] -- so that the operand of one K step of a GEMM tile is one contiguous 16-KiB
 * block (the layout of mq_split_bf16_tiled_f32, which can mint such a pair from an fp32 matrix).  Each array holds
 * mq_split_bf16_tiled_elems(M, K) = ceil(M / 256) * 256 * K elements (rows beyond M are neither written nor read) and K must
 * be a multiple of 32 (MQ_EUNSUPPORTED otherwise).  Every producer below writes it, mq_gemm_nt_bf16x3s_f32 reads it; the
 * fp32 outputs stay row-major. */
int mq_gemm_nt_bf16x3s_f32(const uint16_t *Ah_dev, const uint16_t *Al_dev, const uint16_t *Wh_dev, const uint16_t *Wl_dev,
                           const float *bias_dev, const float *residual_dev, float *C_dev, uint16_t *Ch_dev, uint16_t *Cl_dev,
                           int M, int N, int K, int epilogue, void *stream);
/* mq_gemm_nt_bf16x3s_f32 with epilogue MQ_EPI_BIAS_RESIDUAL whose residual [M, N] is given as a split pair in PAIR LAYOUT (value
 * hi + lo, exact in fp32; N a multiple of 32): a LayerNorm output that only feeds GEMMs and shortcuts then needs no fp32 copy. */
int mq_gemm_nt_bf16x3s_respair_f32(const uint16_t *Ah_dev, const uint16_t *Al_dev, const uint16_t *Wh_dev,
                                   const uint16_t *Wl_dev, const float *bias_dev, const uint16_t *Rh_dev, const uint16_t *Rl_dev,
                                   float *C_dev, uint16_t *Ch_dev, uint16_t *Cl_dev, int M, int N, int K, int epilogue,
                                   void *stream);
/* Split-K form of mq_gemm_nt_bf16x3s_f32 for a long K over a small output (ArcFace's head: [faces, 512] over K = 25,088):
 * `nsplit` workgroup rows each accumulate a contiguous range of K steps into fp32 partials (partials_dev: nsplit * M * N floats),
 * then C = bias + the partials summed in split order (bias_dev may be NULL).  fp32 output only; w_tiled != 0: Wh / Wl in tile
 * layout.  The sum order differs from the one-pass GEMM's: equal within fp32 rounding, not bit for bit. */
int mq_gemm_nt_bf16x3s_splitk_f32(const uint16_t *Ah_dev, const uint16_t *Al_dev, const uint16_t *Wh_dev,
                                  const uint16_t *Wl_dev, const float *bias_dev, float *C_dev, int M, int N, int K,
                                  int w_tiled, int nsplit, float *partials_dev, void *stream);
int mq_layernorm_split_f32(const float *X_dev, const float *gamma_dev, const float *beta_dev, float *Y_dev, uint16_t *Yh_dev,
                           uint16_t *Yl_dev, int M, int C, float eps, void *stream);
int mq_bert_embed_ln_split_f32(const int64_t *input_ids_dev, const int64_t *token_type_ids_dev, const float *word_dev,
                               const float *pos_dev, const float *type_dev, const float *gamma_dev, const float *beta_dev,
                               float *out_dev, uint16_t *out_h_dev, uint16_t *out_l_dev, int B, int L, int H, float eps,
                               void *stream);
int mq_attention_split_f32(const float *qkv_dev, const int64_t *attention_mask_dev, float *out_dev, uint16_t *out_h_dev,
                           uint16_t *out_l_dev, int B, int L, int heads, int head_dim, float scale, int causal, int bf16x3,
                           void *stream);

/* Packed (variable-length) batch: the REAL tokens of all sequences, concatenated -- row r of every activation
 * matrix is one token, sequence b = rows [cu_seqlens[b], cu_seqlens[b+1]).  The reference pads every passage to
 * max_length 256 (experiments/ir/viquae/dpr/passages/config.json:11-14) although a passage has ~130 tokens; GEMMs and
 * LayerNorm are row-wise, so on the packed matrix they simply skip the padding, and these two entries supply the only
 * sequence-aware operations:
 *   mq_bert_embed_ln_packed_f32: BertEmbeddings + LayerNorm with an explicit position id per row;
 *   mq_attention_packed_f32: attention of the n_seqs sequences listed in seq_ids_dev (one launch per length class:
 *     max_len = the longest of them, it selects the key-tile count), each over exactly its own keys.  A padded key
 *     of the dense forward contributes exactly 0 to every sum, so the outputs equal the dense forward's bit for bit. */
int mq_bert_embed_ln_packed_f32(const int64_t *input_ids_dev, const int64_t *token_type_ids_dev, const int32_t *position_ids_dev,
                                const float *word_dev, const float *pos_dev, const float *type_dev, const float *gamma_dev,
                                const float *beta_dev, float *out_dev, uint16_t *out_h_dev, uint16_t *out_l_dev, int T, int H,
                                float eps, void *stream);
int mq_attention_packed_f32(const float *qkv_dev, const int32_t *cu_seqlens_dev, const int32_t *seq_ids_dev, int n_seqs,
                            int max_len, float *out_dev, uint16_t *out_h_dev, uint16_t *out_l_dev, int heads, int head_dim,
                            float scale, int causal, int bf16x3, void *stream);

/* Multimodal encoders of the reference (meerqat/models/mm.py: ECAEncoder :557-754, IntermediateLinearFusion :773-861) reuse
 * the entry points above; the only extra arithmetic is the sum of an example's face embeddings into its text vector
 * (mm.py:838-843): out[g, :] = init[g, :] + sum_j x[g, j, :], x [G, n, H], init (may be NULL) and out [G, H]. */
int mq_sum_groups_f32(const float *x_dev, const float *init_dev, float *out_dev, int G, int n, int H, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Late fusion of several runs on the device: replaces, for integer document
 * ids, `default_minimum` (meerqat/ir/fuse.py:129-146), `gzmuv_norm` (:86-126) and ranx's
 * `fuse(runs, norm, method="wsum", params={"weights": ...})` as called by `Fusion.test` (:215-236) from
 * `dataset_search` (meerqat/ir/search.py:514-524).
 *   ids_dev    [n_runs, nq, K] int64   document ids, -1 = empty slot; unique within one (run, query);
 *                                      0 <= id < 2^58; every run lists the same nq queries
 *   scores_dev [n_runs, nq, K] f64
 *   weights_host [n_runs] f64 (HOST memory), n_runs <= MQ_FUSE_MAX_RUNS, n_runs*K <= 4096
 *   norm       MQ_FUSE_NORM_NONE | _GZMUV (one mean/std per run over all its queries, population std,
 *              denominator max(std, 1e-9)) | _ZMUV (ranx "zmuv": the same per query)
 *   defmin     != 0: before normalising, every run that has results for a query receives the documents
 *              only other runs retrieved, at its own minimum score for that query
 *   out_ids_dev [nq, n_runs*K] int64 / out_scores_dev [nq, n_runs*K] f64: the fused run, best first,
 *              equal scores by ascending id, (-1, 0.0) after out_count_dev[q] entries
 * Fused score of a document = ((0.0 + w0*s0) + w1*s1) + ... over the runs that hold it, in run order,
 * f64 without contraction (what ranx's comb_sum computes).  ws_dev: mq_fuse_workspace_bytes().
 * ------------------------------------------------------------------------------------------- */
#define MQ_FUSE_MAX_RUNS 32
#define MQ_FUSE_NORM_NONE 0
#define MQ_FUSE_NORM_GZMUV 1
#define MQ_FUSE_NORM_ZMUV 2
size_t mq_fuse_workspace_bytes(int n_runs, int nq, int K);
int mq_fuse_wsum_f64(const int64_t *ids_dev, const double *scores_dev, int n_runs, int nq, int K,
                     const double *weights_host, int norm, int defmin, int64_t *out_ids_dev, double *out_scores_dev,
                     int32_t *out_count_dev, void *ws_dev, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Rank metrics of a run against relevance judgements -- what `ranx.compare(qrels, runs, metrics=[...])` reports at
 * the end of a search job (meerqat/ir/search.py:397,500-512; ranx is un-vendored, `ranx>=0.3.2`: the published
 * definitions are restated, parity unpinned):
 *   ids_dev [nq, K] int64    one run, best first; a row ends at its first negative id
 *   rel_ptr_dev [nq + 1] / rel_ids_dev    CSR of the RELEVANT documents (judgement >= 1) of every query, ascending
 *                                         inside a query
 *   codes_host / ks_host [n_metrics]      MQ_RANK_METRIC_* and the cut k (0 = the whole run); n_metrics <= MQ_RANK_MAX_METRICS
 *     MRR        1 / (1 + rank of the first relevant document inside the cut), else 0
 *     PRECISION  (relevant inside the cut) / k     (k = 0: / the length of the query's run; an empty run scores 0)
 *     HIT_RATE   1 when a relevant document is inside the cut
 *     RECALL     (relevant inside the cut) / (relevant documents of the query), 0 when it has none
 *   per_query_dev [n_metrics, nq] f64, mean_dev [n_metrics] f64 = numpy's mean of each row (np.mean's pairwise
 *   summation restated: the number ranx.evaluate returns)
 * ------------------------------------------------------------------------------------------- */
#define MQ_RANK_METRIC_MRR 0
#define MQ_RANK_METRIC_PRECISION 1
#define MQ_RANK_METRIC_HIT_RATE 2
#define MQ_RANK_METRIC_RECALL 3
#define MQ_RANK_MAX_METRICS 16
int mq_run_metrics_f64(const int64_t *ids_dev, int nq, int K, const int64_t *rel_ptr_dev, const int64_t *rel_ids_dev,
                       int n_metrics, const int *codes_host, const int *ks_host, double *per_query_dev,
                       double *mean_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The weight search of `Fusion.fit` (meerqat/ir/fuse.py:193-217 -> `ranx.optimize_fusion(method="wsum")`): every
 * trial weight vector fuses the runs like mq_fuse_wsum_f64 and is scored by ONE rank metric, all trials in one
 * launch (a workgroup sorts and normalises a query's entries once, then walks the trials).
 *   ids_dev / scores_dev / n_runs / nq / K / norm / defmin: as mq_fuse_wsum_f64
 *   trials_dev [n_trials, n_runs] f64 (DEVICE memory)
 *   rel_ptr_dev / rel_ids_dev: as mq_run_metrics_f64;  metric / metric_k: one MQ_RANK_METRIC_* and its cut
 *   per_query_dev [n_trials, nq] f64: the metric of query q under trial t (rank = fused score descending, equal
 *   scores by ascending id -- the order mq_fuse_wsum_f64 writes); mean_dev [n_trials] f64: np.mean of each row.
 *   ws_dev: mq_fuse_workspace_bytes(n_runs, nq, K).
 * ------------------------------------------------------------------------------------------- */
int mq_fuse_fit_wsum_f64(const int64_t *ids_dev, const double *scores_dev, int n_runs, int nq, int K,
                         const double *trials_dev, int n_trials, int norm, int defmin, const int64_t *rel_ptr_dev,
                         const int64_t *rel_ids_dev, int metric, int metric_k, double *per_query_dev, double *mean_dev,
                         void *ws_dev, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Run files -- HOST function, no device work: replaces the per-hit Python objects behind
 * `run.save(metric_save_path / f"{index_name}.json")` (meerqat/ir/search.py:485-498) over the dicts of :413-440.  Formats the
 * rows of a result block kept as arrays into the text `json.dump({q_id: {str(doc): float(score)}})` writes, byte for byte
 * (", " and ": " separators, CPython's float repr of the score widened to double, NaN / Infinity spelled as json does),
 * WITHOUT the enclosing braces:   "<q0>": {"<id>": <score>, ...}, "<q1>": {...}
 *   qid_json / qid_off [nq + 1]: the already JSON-encoded question ids (quotes included), concatenated, and their offsets;
 *   ids [nq, stride] int64, scores [nq, stride] fp32 (scores_f64 = 0) or f64 (= 1), host memory; a row ends at counts[q]
 *   entries (counts NULL: stride) or at its first negative id (FAISS's -1 padding);
 *   out / out_cap: destination, at least nq * (8 + 52 * stride) + the length of qid_json bytes (the worst case);
 *   n_threads: 0 = all host cores (at most MQ_RUN_JSON_MAX_PARTS); parts [2 * MQ_RUN_JSON_MAX_PARTS] int64 (host).
 * The rows are cut into P contiguous parts formatted concurrently, each into its own region of `out`; returns P and sets
 * parts[2 * p] / parts[2 * p + 1] to the offset / length of part p: the run text is the parts in order, joined by ", " (written
 * one after the other by the caller: no second copy of a 50 MB run is made).  0 for nq = 0.  If out_cap is too small nothing
 * is written and the return value r < -16 encodes the size needed as -(r + 16); MQ_EINVAL for bad arguments. */
#define MQ_RUN_JSON_MAX_PARTS 32
int64_t mq_format_run_json(const char *qid_json, const int64_t *qid_off, int64_t nq, const int64_t *ids, const void *scores,
                           int scores_f64, int64_t stride, const int32_t *counts, char *out, int64_t out_cap, int n_threads,
                           int64_t *parts);

/* ---------------------------------------------------------------------------------------------
 * Image preprocessing in front of the CLIP tower: replaces
 * `transform(images, return_tensors="pt")` in `embed` (meerqat/image/embedding.py:141-152), the transform being the
 * `CLIPFeatureExtractor` of experiments/image_embedding/clip/vit_config.json:13-17 -- Pillow's 8-bit
 * `Image.resize(..., BICUBIC | BILINEAR)`, centre crop, `float32(float64(u8) * rescale_factor)`, `(x - mean) / std`.
 * Bit-identical to Pillow 12 + transformers 5 (`CLIPImageProcessorPil`).
 *
 * mq_image_plan (HOST arithmetic, needs no GPU): sizes_host [n_images][2] = (height, width) of the decoded RGB
 * images -> geom_host [n_images][MQ_IMAGE_GEOM] int64 (source byte offset of the image in the packed buffer, sizes,
 * resized sizes, crop origin, workspace offsets, tap counts) and totals_host[MQ_IMAGE_TOTALS] = {bytes of the packed uint8
 * source buffer (each image HWC at a 16-byte aligned offset, the buffer itself 16-byte aligned), workspace bytes, largest
 * image height, coefficient ints, largest image width}.
 *   resize_mode  MQ_IMAGE_RESIZE_NONE | _SHORTEST (shortest edge -> size_h, long edge int(size_h * long / short), the
 *                `get_resize_output_image_size(default_to_square=False)` rule) | _EXACT (size_h x size_w)
 *                OR MQ_IMAGE_CROP_TORCHVISION into it for torchvision's CenterCrop origin, int(round((size - crop) / 2.0)) with
 *                Python's round-half-to-even, instead of the default (size - crop) / 2 rounded down (transformers' center_crop):
 *                the two differ when size - crop = 3 (mod 4)
 *   MQ_EUNSUPPORTED when a resized image is smaller than the crop window (HF zero-pads; not provided) or for filters
 *   other than bilinear / bicubic.
 * mq_image_preprocess_u8: src_dev = the packed source buffer, geom_dev = geom_host copied to the device,
 *   totals_host = what the plan returned, flags = MQ_IMAGE_RESCALE | MQ_IMAGE_NORMALIZE, mean3_host / std3_host = 3
 *   floats in HOST memory; out_dev float32 [n_images][3][crop_h][crop_w].  Images wider than 21 k pixels: MQ_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
#define MQ_IMAGE_GEOM 12
#define MQ_IMAGE_TOTALS 5
#define MQ_IMAGE_BILINEAR 2 /* PIL.Image.Resampling values */
#define MQ_IMAGE_BICUBIC 3
#define MQ_IMAGE_RESIZE_NONE 0
#define MQ_IMAGE_RESIZE_SHORTEST 1
#define MQ_IMAGE_RESIZE_EXACT 2
#define MQ_IMAGE_CROP_TORCHVISION 0x100
#define MQ_IMAGE_RESCALE 1
#define MQ_IMAGE_NORMALIZE 2
int mq_image_plan(const int64_t *sizes_host, int n_images, int resize_mode, int size_h, int size_w, int crop_h, int crop_w,
                  int filter, int64_t *geom_host, int64_t *totals_host);
int mq_image_preprocess_u8(const uint8_t *src_dev, const int64_t *geom_dev, int n_images, const int64_t *totals_host, int crop_h,
                           int crop_w, int filter, int flags, double rescale_factor, const float *mean3_host,
                           const float *std3_host, float *out_dev, void *ws_dev, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Baseline-JPEG decoding split between host and GPU (csrc/jpeg.hip): replaces, per image,
 * `Image.open(path).convert('RGB')` of `load_image` (meerqat/data/loading.py:108-124, called by meerqat/image/embedding.py:127)
 * for the files it covers -- 8-bit Huffman-coded JPEGs, sequential (SOF0 / SOF1) with ONE interleaved scan or progressive (SOF2)
 * with a complete, regular progression, grey or YCbCr with luma sampling 1x1 / 2x1 / 1x2 / 2x2 and chroma 1x1 -- with the same RGB bytes as Pillow 12 / libjpeg-turbo (ISLOW inverse DCT,
 * fancy upsampling, fixed-point colour tables; oracle/jpeg.py, pinned against Pillow).  Everything else, and any irregularity of
 * the entropy-coded data, is declined and stays Pillow's: the caller keeps the reference's errors and warnings.
 *
 * mq_jpeg_probe (HOST, needs no GPU): file bytes -> info_host[MQ_JPEG_INFO] = {height, width, components, 8 x 8 blocks,
 *   staging bytes (header + the larger of the coefficient blocks and the RGB image, a multiple of 16), luma sampling h * 16 + v
 *   (0 for grey)}.  MQ_OK | MQ_EUNSUPPORTED (a JPEG of another kind) | MQ_EINVAL (not a JPEG / damaged headers).
 * mq_jpeg_read_coefficients (HOST): Huffman-decodes the scan into staging_host (4-byte aligned, >= the probe's staging bytes):
 *   a MQ_JPEG_HEADER_BYTES header (int32 words: magic, height, width, components, hmax, vmax, MCUs across / down, then per
 *   component h, v, blocks across / down, first block, [total blocks], real samples across / down; uint16 quantisation tables
 *   [3][64] in natural order at byte 128) followed by the quantised coefficients, int16 [block][64] in natural order,
 *   component after component.  MQ_EINVAL when the scan is irregular in any way (the staging area is then undefined).
 *   A caller that decodes such a file by other means stores its H x W x 3 RGB bytes behind a header whose words 0-2 are
 *   MQ_JPEG_MAGIC_RGB, height, width.
 * mq_jpeg_decode_rgb_u8 (GPU): items_dev int64 [n_images][2] = (byte offset of an image's header, byte offset of its RGB
 *   output) inside buf_dev (16-byte aligned offsets and buffer); max_blocks / max_strips = the largest block count and the
 *   largest ceil(height / 2) * ceil(width / 16) of the batch (the colour kernel runs one thread per 16 x 2 pixels).  The inverse DCT runs in place (the coefficient area is consumed); the H x W x 3 bytes are what
 *   mq_image_preprocess_u8 / mq_warp_affine_faces_f32 read.
 * ------------------------------------------------------------------------------------------- */
#define MQ_JPEG_INFO 6
#define MQ_JPEG_HEADER_BYTES 512
#define MQ_JPEG_MAGIC_COEFFICIENTS 0x4745504A /* "JPEG" */
#define MQ_JPEG_MAGIC_RGB 0x20424752          /* "RGB " */
#define MQ_JPEG_MAX_PIXELS (1 << 26)
int mq_jpeg_probe(const uint8_t *file_host, size_t nbytes, int64_t *info_host);
int mq_jpeg_read_coefficients(const uint8_t *file_host, size_t nbytes, void *staging_host, size_t staging_cap);
int mq_jpeg_decode_rgb_u8(uint8_t *buf_dev, const int64_t *items_dev, int n_images, int max_blocks, int64_t max_strips,
                          void *stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement aid (csrc/diag.hip; no reference counterpart, not on the product path): `workgroups` x 16 waves loop over
 * `iters` x 16 v_mfma_f32_32x32x16_bf16 on register operands (zero, or N(0,1)-like random when random_operands != 0), no
 * memory traffic: 2*32*32*16 * 16 * iters * 16 * workgroups FLOP per launch.  bench.py times it for the matrix-pipe rate
 * this chip SUSTAINS on such operands (its power management lowers the clock on random data).  out_dev: workgroups * 1024
 * floats (keeps the accumulators observable).
 * ------------------------------------------------------------------------------------------- */
int mq_diag_mfma_bf16_loop(int iters, int random_operands, int workgroups, float *out_dev, void *stream);

/* What the matrix instruction RETURNS: out_dev[32][32] fp32 = A . B^T for A_dev, B_dev = 32 rows x dp bf16 (row-major, dp a
 * multiple of 16), one v_mfma_f32_32x32x16_bf16 per 16 columns in column order, each chained on the previous result -- the
 * accumulation of csrc/knn_screen.inc's screening scan.  tests/test_screened_gpu.py bounds its distance to the float64 sum of
 * the same bf16 operands by the accumulation term of the screening margin (the one term of the bound that rests on the
 * instruction's undocumented internal summation). */
int mq_diag_mfma_bf16_dot(const uint16_t *A_dev, const uint16_t *B_dev, int dp, float *out_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * ArcFace r50 face encoder (meerqat/image/face_recognition.py:44-102; insightface arcface_torch IResNet-50 and OpenCV /
 * scikit-image are un-vendored and not installable here: parity unpinned, oracle/arcface.py restates the published algorithms).
 * A convolution = mq_im2col_split_f32 (patch gather + the layer's elementwise pre-operations -> the GEMM's split pair) followed
 * by mq_gemm_nt_bf16x3s_f32 (BatchNorms behind the convolution folded into W / bias, residual in the epilogue); NHWC.
 *   x_dev   fp32 activation, NHWC [B, H, W, C] (nchw != 0: NCHW [B, C, H, W], the network's input)
 *   A       rows = B * Ho * Wo output pixels (Ho = (H + 2 pad - KH) / stride + 1), column (kh * KW + kw) * C + c, zero beyond
 *           KH * KW * C up to Kpad (a multiple of 32); PAIR LAYOUT, mq_split_bf16_tiled_elems(rows, Kpad) elements per array
 *   pre-operations on every in-bounds element, in this order: PReLU (prelu_slope_dev [C] or NULL), then x * scale + shift
 *           (scale_dev / shift_dev [C], both or neither: an eval-mode BatchNorm in front of the convolution); padding is zero.
 * mq_warp_affine_faces_f32: cv2.warpAffine(image, M, (size, size), borderValue = 0) in OpenCV's fixed-point bilinear
 * arithmetic + ToTensor + Normalize(0.5, 0.5) for `nfaces` faces.  images_dev: the decoded RGB images of a batch packed in one
 * uint8 buffer (image i = H_i x W_i x 3 at byte offsets_dev[i], hw_dev[2 i] = H_i, hw_dev[2 i + 1] = W_i); face f is cut from image
 * face_image_dev[f] with the INVERTED 2 x 3 matrix minv_dev[6 f ..] (doubles); out_dev fp32 [nfaces, 3, size, size].
 * ------------------------------------------------------------------------------------------- */
int mq_im2col_split_f32(const float *x_dev, int B, int H, int W, int C, int nchw, int KH, int KW, int stride, int pad,
                        const float *prelu_slope_dev, const float *scale_dev, const float *shift_dev, uint16_t *Ah_dev,
                        uint16_t *Al_dev, int Kpad, void *stream);
/* A 3 x 3 convolution (padding 1, stride 1 or 2) as an IMPLICIT GEMM: the patch matrix is never written -- the GEMM's LDS-DMA
 * gathers its A stage from the input pair (zeros at the border) -- and the layer's elementwise operations ride on the epilogue of
 * the convolution that PRODUCES a tensor instead of on the im2col that consumes it.  Same products in the same order as
 * mq_im2col_split_f32 + mq_gemm_nt_bf16x3s_f32: the same bits.
 *   Xh / Xl       the convolution's input AFTER its pre-operations, as a split pair in PAIR LAYOUT over [B * H * W, C] (NHWC; C a
 *                 multiple of 32): what mq_im2col_split_f32 with KH = KW = 1 or a previous call of this function wrote
 *   Wh / Wl       mq_split_bf16_tiled_f32 of W [N, 9 C], column (kh * 3 + kw) * C + c (N a multiple of 64); bias_dev [N]
 *   prelu_slope_dev != NULL:  P = split(prelu(conv + bias))                       (Y, residual, scale, shift must be NULL)
 *   prelu_slope_dev == NULL:  Y = conv + bias + residual (fp32 [M, N], M = B * Ho * Wo, Ho = (H - 1) / stride + 1), and, when
 *                 scale_dev / shift_dev [N] are given, P = split(Y * scale + shift) (the BatchNorm in front of the NEXT convolution)
 *   Ph / Pl       pair output, PAIR LAYOUT over [M, N], mq_split_bf16_tiled_elems(M, N) elements each
 *   zeros_dev     at least 16 bytes of zeros on the device (the padded border's source)
 *   tile          MQ_CONV_TILE_AUTO, or one of the workgroup tiles (rows x columns; the column count must divide N).  AUTO takes
 *                 MQ_CONV_TILE_PATCH_256x64 for N = 64 at stride 1 with MQ_CONV_K_CHANNEL_MAJOR and W <= 127, otherwise the
 *                 widest tile the channel count fills while it still gives every CU a workgroup */
#define MQ_CONV_TILE_AUTO 0
#define MQ_CONV_TILE_256x256 1
#define MQ_CONV_TILE_512x128 2
#define MQ_CONV_TILE_256x128 3
#define MQ_CONV_TILE_512x64 4
#define MQ_CONV_TILE_PATCH_256x64 5 /* stride 1, W <= 127, with MQ_CONV_K_CHANNEL_MAJOR: the nine taps of a channel block read one
                                     * LDS-resident input patch (256 + 2 W + 2 pixels) instead of nine gathers; same bits */
/* OR into `tile`: walk K as (32-channel block, tap) instead of (tap, block) -- the nine taps of a block re-read the same input
 * lines back to back, so a workgroup's live footprint in L2 is one block's rows instead of all C channels'.  The sum order then
 * differs from the explicit path's (equal within fp32 rounding, not bit for bit). */
#define MQ_CONV_K_CHANNEL_MAJOR 0x100
int mq_conv3x3_pair_f32(const uint16_t *Xh_dev, const uint16_t *Xl_dev, int B, int H, int W, int C, int stride,
                        const uint16_t *Wh_dev, const uint16_t *Wl_dev, int N, const float *bias_dev,
                        const float *prelu_slope_dev, const float *residual_dev, const float *scale_dev,
                        const float *shift_dev, float *Y_dev, uint16_t *Ph_dev, uint16_t *Pl_dev, const void *zeros_dev,
                        int tile, void *stream);
/* The stem of IResNet: 3 -> 64 channels, 3 x 3, stride 1, padding 1, as a direct fp32 convolution (K = 27 has no matrix-pipe shape),
 * fused with what follows it: v = prelu(conv(x) + bias);
 *   P = split(v * scale + shift)  PAIR LAYOUT over [B * H * W, 64]: the first block's conv1 input (its bn1 applied)
 *   D = split(v) at even (h, w)   PAIR LAYOUT over [B * H/2 * W/2, 64]: the A operand of the first block's strided 1 x 1 downsample
 *                                 (Dh / Dl may both be NULL)
 * x_dev fp32 NCHW [B, 3, H, W] (W a multiple of 4, H even when D is asked for); wt_dev fp32 [27, 64]: row (kh * 3 + kw) * 3 + c,
 * the BatchNorm behind the convolution folded in; bias / prelu_slope / scale / shift fp32 [64]. */
int mq_stem_conv3x3_f32(const float *x_dev, int B, int H, int W, const float *wt_dev, const float *bias_dev,
                        const float *prelu_slope_dev, const float *scale_dev, const float *shift_dev, uint16_t *Ph_dev,
                        uint16_t *Pl_dev, uint16_t *Dh_dev, uint16_t *Dl_dev, void *stream);
/* ---- fp16 mode of the face encoder: the reference's autocast precision (arcface_torch `get_model('r50', fp16=True)`) ----
 * Every tensor of the trunk is fp16, NHWC, in PAIR LAYOUT over [pixels, channels] (ONE array: 64-byte rows of 32 channels, rows padded
 * to 256; mq_split_bf16_tiled_elems(rows, C) elements).  r(v) = round to fp16, nearest even, overflow to +-inf (Tensor.half()).  The
 * BatchNorm behind a convolution is NOT folded: post_scale / post_shift [N] fp32 apply to r(acc), as autocast rounds the conv output
 * before the BatchNorm.  PReLU slopes must hold fp16 values (r(slope)); BatchNorm scale / shift are fp32.
 * mq_conv3x3_f16: 3 x 3, padding 1, stride 1 or 2, fp16 operands, one v_mfma_f32_32x32x16_f16 per 16 k, fp32 accumulation.
 *   X_dev         fp16 input [B * H * W, C] (C a multiple of 32); Wt_dev fp16 weights [N, 9 C] (column (kh * 3 + kw) * C + c) in the
 *                 tile layout of mq_split_bf16_tiled_f32 ([ceil(N / 256)][9 C / 32][256][32], zero rows beyond N; N a multiple of 64)
 *   t = r(r(acc) * post_scale + post_shift)
 *   prelu_slope_dev != NULL:  P = r(prelu(t))                                        (residual, Y, scale, shift must be NULL)
 *   prelu_slope_dev == NULL:  Y = r(t + residual) (fp16 [M, N]: the next shortcut), and, when scale_dev / shift_dev [N] are given,
 *                 P = r(Y * scale + shift) (the next block's bn1)
 *   tile          as for mq_conv3x3_pair_f32 (MQ_CONV_TILE_PATCH_256x64 needs MQ_CONV_K_CHANNEL_MAJOR)
 * mq_stem_conv3x3_f16: the stem (3 -> 64, 3 x 3, stride 1, padding 1) on the vector ALU: r(x) * wt (wt fp32 [27, 64] holding the
 *   fp16 weights, row (kh * 3 + kw) * 3 + c), fp32 accumulation; v = r(prelu(r(r(acc) * post_scale + post_shift)));
 *   P = r(v * scale + shift) [B * H * W, 64] (the first block's bn1);  D = v at even (h, w) [B * H/2 * W/2, 64] (D may be NULL).
 *   W a multiple of 4, H even when D is asked for.
 * mq_conv1x1_f16: 1 x 1, stride 1 or 2, no padding: Y = r(r(conv) * post_scale + post_shift) [B * Ho * Wo, N];  Wt_dev fp16
 *   ROW-MAJOR [N, C]; C a multiple of 32, N a multiple of 64.
 * mq_head_prep_f16: A[b, (h W + w) C + c] = split(r(X[b, h, w, c] * scale + shift)) -- bn2 - flatten (NHWC order) - .float() -- as
 *   the bf16 (hi, lo) pair of mq_gemm_nt_bf16x3s_splitk_f32 (PAIR LAYOUT over [B, HW * C]); exact: an fp16 value is hi + lo. */
int mq_conv3x3_f16(const uint16_t *X_dev, int B, int H, int W, int C, int stride, const uint16_t *Wt_dev, int N,
                   const float *post_scale_dev, const float *post_shift_dev, const float *prelu_slope_dev,
                   const uint16_t *residual_dev, const float *scale_dev, const float *shift_dev, uint16_t *Y_dev,
                   uint16_t *P_dev, const void *zeros_dev, int tile, void *stream);
int mq_stem_conv3x3_f16(const float *x_dev, int B, int H, int W, const float *wt_dev, const float *post_scale_dev,
                        const float *post_shift_dev, const float *prelu_slope_dev, const float *scale_dev,
                        const float *shift_dev, uint16_t *P_dev, uint16_t *D_dev, void *stream);
int mq_conv1x1_f16(const uint16_t *X_dev, int B, int H, int W, int C, int stride, const uint16_t *Wt_dev, int N,
                   const float *post_scale_dev, const float *post_shift_dev, uint16_t *Y_dev, void *stream);
int mq_head_prep_f16(const uint16_t *X_dev, int B, int HW, int C, const float *scale_dev, const float *shift_dev,
                     uint16_t *Ah_dev, uint16_t *Al_dev, void *stream);
int mq_warp_affine_faces_f32(const uint8_t *images_dev, const int64_t *offsets_dev, const int32_t *hw_dev,
                             const int32_t *face_image_dev, const double *minv_dev, int nfaces, int size, float *out_dev,
                             void *stream);

/* ---- torchvision bottleneck ResNet (csrc/resnet.hip; meerqat/image/embedding.py: resnet50 cut before avgpool + AdaptiveMaxPool2d(1), the
 * `imagenet-RN50` column).  NHWC; activations that only feed convolutions are split pairs in PAIR LAYOUT; the BatchNorm behind each
 * convolution is folded into W / bias by the caller.  The 3 x 3 convolutions are mq_conv3x3_pair_f32 with a zero PReLU slope (= ReLU).
 * mq_conv1x1_pair_f32: a 1 x 1 convolution, stride 1 or 2, no padding, as an implicit GEMM on the input pair (the strided form reads
 *   the pixels at even coordinates; nothing is copied), three bf16 MFMA products per fp32 product in the order of mq_gemm_nt_bf16x3s_f32.
 *   Xh / Xl       input pair, PAIR LAYOUT over [B * H * W, C] (C a multiple of 32)
 *   Wh / Wl       mq_split_bf16_tiled_f32 of W [N, C] (N a multiple of 64); bias_dev [N]
 *   per element   v = acc + bias;  v += residual (fp32 [M, N], M = B * Ho * Wo, Ho = (H - 1) / stride + 1; may be NULL);
 *                 v = max(v, 0) when relu != 0;  Y = v (fp32 [M, N]) and P = split(v) (PAIR LAYOUT over [M, N]): either may be NULL, not both
 *   zeros_dev     at least 16 bytes of zeros on the device (the source of the tile rows beyond M)
 *   tile          MQ_CONV_TILE_AUTO | _256x256 | _256x128 | _512x64 (the column count must divide N)
 * mq_stem_conv7x7_pool_f32: the stem -- convolution 7 x 7, stride 2, padding 3, 3 -> 64 channels, + bias, ReLU, max-pool 3 x 3 stride 2
 *   padding 1 -- in one kernel on the vector ALU; the un-pooled tensor is never stored.  x_dev fp32 NCHW [B, 3, H, W] (H a multiple of
 *   4, W of 8: MQ_EUNSUPPORTED otherwise); wt_dev fp32 [147, 64], row (kh * 7 + kw) * 3 + c, bn1 folded in; bias_dev [64]; fp32 fused
 *   multiply-adds in (kh, c, kw) order starting from the bias.  Ph / Pl: PAIR LAYOUT over [B * H/4 * W/4, 64].
 * mq_pool_hw_f32: out[b, c] = max (MQ_POOL_MAX) or mean (MQ_POOL_MEAN) over p of X[b * HW + p, c], X fp32 [B * HW, C], B <= 65535.  The
 *   mean is the fp32 sum in the order p = 0 ... HW - 1 (one rounding per pixel), divided once by HW. */
#define MQ_POOL_MAX 0
#define MQ_POOL_MEAN 1
int mq_conv1x1_pair_f32(const uint16_t *Xh_dev, const uint16_t *Xl_dev, int B, int H, int W, int C, int stride,
                        const uint16_t *Wh_dev, const uint16_t *Wl_dev, int N, const float *bias_dev, const float *residual_dev,
                        int relu, float *Y_dev, uint16_t *Ph_dev, uint16_t *Pl_dev, const void *zeros_dev, int tile, void *stream);
int mq_stem_conv7x7_pool_f32(const float *x_dev, int B, int H, int W, const float *wt_dev, const float *bias_dev, uint16_t *Ph_dev,
                             uint16_t *Pl_dev, void *stream);
int mq_pool_hw_f32(const float *X_dev, int B, int HW, int C, int mode, float *out_dev, void *stream);

/* ---- openai-clip's ModifiedResNet (csrc/clip_resnet.hip; `clip.load("RN50")`'s visual tower, the `clip-RN50` column).  The bottlenecks
 * are mq_conv1x1_pair_f32 / mq_conv3x3_pair_f32 at stride 1 with these around them; all four run on the vector ALU.
 * mq_clip_stem_conv3x3s2_f32: the stem's first convolution -- 3 x 3, stride 2, padding 1, 3 -> N channels (N = 32: MQ_EUNSUPPORTED
 *   otherwise), + bias, ReLU.  x_dev fp32 NCHW [B, 3, H, W] (H, W even: MQ_EUNSUPPORTED otherwise); wt_dev fp32 [27, N], row
 *   (kh * 3 + kw) * 3 + c, bn1 folded in; bias_dev [N]; fp32 fused multiply-adds in (kh, c, kw) order starting from the bias.
 *   Ph / Pl: PAIR LAYOUT over [B * H/2 * W/2, N].
 * mq_avgpool2x2_pair_f32: nn.AvgPool2d(2) on a pair.  Xh / Xl: PAIR LAYOUT over [B * H * W, C] (NHWC; H, W even, C a multiple of 32:
 *   MQ_EINVAL otherwise); Ph / Pl: PAIR LAYOUT over [B * H/2 * W/2, C].  With x_ij = hi + lo (exact in fp32) of input pixel
 *   (2 ho + i, 2 wo + j): out = split((((x00 + x01) + x10) + x11) * 0.25f), every operation one fp32 rounding.
 * mq_attnpool_tokens_f32: AttentionPool2d's token matrix from the last block's fp32 output Y [B * HW, C] and the positional embedding
 *   pos_dev fp32 [HW + 1, C] (C a multiple of 32; Y and pos 16-byte aligned).  T / Th, Tl: PAIR LAYOUT over [B * (HW + 1), C];
 *   row b * (HW + 1) = mean_b + pos[0] with mean_b mq_pool_hw_f32's MQ_POOL_MEAN (the fp32 sum in the order p = 0 ... HW - 1, divided
 *   once by HW), rows b * (HW + 1) + 1 + p = Y[b * HW + p] + pos[1 + p].  Qh / Ql: PAIR LAYOUT over [B, C], row b = the mean token of
 *   image b once more (the operand of q_proj).
 * mq_attention_single_query_f32: multi-head attention with ONE query per image: q_dev fp32 [B, heads * 64], kv_dev fp32
 *   [B * T, 2 * heads * 64] = [k | v] projections of the T tokens of every image.  Per (image, head), in fp32:
 *   s_t = (q . k_t) * scale, the 64 products summed by a butterfly over the lanes (xor 32, 16, ..., 1);  p_t = expf(s_t - max s);
 *   o = (sum over t = 0 ... T - 1 in that order of p_t v_t) / (sum of p_t).  Oh / Ol: PAIR LAYOUT over [B, heads * 64].
 *   head_dim must be 64 and T <= 8192 (MQ_EUNSUPPORTED otherwise); T is a runtime value. */
int mq_clip_stem_conv3x3s2_f32(const float *x_dev, int B, int H, int W, const float *wt_dev, const float *bias_dev, int N,
                               uint16_t *Ph_dev, uint16_t *Pl_dev, void *stream);
int mq_avgpool2x2_pair_f32(const uint16_t *Xh_dev, const uint16_t *Xl_dev, int B, int H, int W, int C, uint16_t *Ph_dev,
                           uint16_t *Pl_dev, void *stream);
int mq_attnpool_tokens_f32(const float *Y_dev, int B, int HW, int C, const float *pos_dev, uint16_t *Th_dev, uint16_t *Tl_dev,
                           uint16_t *Qh_dev, uint16_t *Ql_dev, void *stream);
int mq_attention_single_query_f32(const float *q_dev, const float *kv_dev, int B, int T, int heads, int head_dim, float scale,
                                  uint16_t *Oh_dev, uint16_t *Ol_dev, void *stream);

/* ---- reader: MultiPassageBERT answer extraction (csrc/reader.hip; the evaluation path of meerqat/train/trainee.py:742-824) ----
 * N questions, M passages each, L tokens per (question, passage) pair; every array is dense fp32 / int64, row-major.
 * mq_reader_qa_head_f32: BertForQuestionAnswering.qa_outputs on the last hidden states h [rows, H] (H a multiple of 4; h and w
 *   16-byte aligned): start[r] = h[r] . w[0] + b[0], end[r] = h[r] . w[1] + b[1] for w [2, H], b [2] (NULL = no bias), fp32
 *   fused multiply-adds.  One wave per row, the rows spread over the whole GPU.
 * mq_reader_log_softmax_f32: nn.LogSoftmax over each question's M * L positions (meerqat/train/optim.py:42-87), for the start
 *   and the end logits [N, M, L]: logp = fl(fl(x - max) - logf(S)) with S = sum expf(x - max) summed in fp32 as per-thread
 *   partials and a tree; p = expf(logp).  Writes the four [N, M, L] arrays.
 * mq_reader_best_spans_f32: get_best_spans (meerqat/models/qa.py:18-77) on probabilities [N, M, L]: candidate P[m, i, j] =
 *   fl(s_i e_j) for i <= j, else 0; row i = 0 zeroed when cannot_be_first_token; times weights[q, m] when weights_dev [N, M] is
 *   given (shifted to >= 1 by the caller, as the reference does in place).  Per question: the lowest passage holding the
 *   largest candidate, then the lowest flat index i * L + j reaching it -> passage, start = i, end = j + 1 (exclusive), int64 [N].
 *   Bit-exact for finite non-negative inputs (no denormal flushing).  M * L * L must stay below 2^32 (MQ_EINVAL). */
int mq_reader_qa_head_f32(const float *h_dev, const float *w_dev, const float *b_dev, float *start_dev, float *end_dev,
                          int64_t rows, int H, void *stream);
int mq_reader_log_softmax_f32(const float *start_logits_dev, const float *end_logits_dev, int N, int M, int L,
                              float *start_logp_dev, float *end_logp_dev, float *start_p_dev, float *end_p_dev, void *stream);
int mq_reader_best_spans_f32(const float *start_p_dev, const float *end_p_dev, const float *weights_dev, int N, int M, int L,
                             int cannot_be_first_token, int64_t *passage_dev, int64_t *start_dev, int64_t *end_dev,
                             void *stream);

/* ---- sparse retrieval: exhaustive BM25 over a CSR inverted index (csrc/bm25.hip) -- what the reference delegates to Elasticsearch
 * for its `"es": true` / `kind: "ES"` indexes (meerqat/ir/search.py:81-205).  The arithmetic restates Lucene 8's BM25Similarity as
 * published (parity with a live Elasticsearch is UNPINNED: none exists in this image):
 *   code[d]   one byte per document, Lucene's SmallFloat.intToByte4 of its token count; cache[256] fp32 =
 *             k1 * ((1 - b) + b * byte4ToInt(code) / avgdl), computed by the caller
 *   impact    fp32 per posting = float(tf / (tf + cache[code[doc]])), the addition and the division in double
 *   score     of a document for a query = the sequential fp32 sum, in clause order, of weight * impact (multiply, then add: never
 *             fused) over the clauses (term, weight = float(multiplicity) * idf) whose term the document holds
 * Index layout (device): ptr [n_terms + 1] int64, doc [nnz] int32 ascending inside a term, tf [nnz] int32, impact [nnz] fp32.
 * Queries (device): qptr [nq + 1] int32 into cterm [n_clauses] int32 / cweight [n_clauses] fp32, clauses in clause order.  A
 *   clause whose term id lies outside [0, n_terms) contributes nothing and nothing is read through it (ptr is not indexed with it);
 *   the same term may recur among a query's clauses, each occurrence is added in its place.
 * mq_bm25_block_rows: documents per scoring workgroup, whose fp32 accumulators live in LDS (MQ_BM25_BLOCK_ROWS).
 * mq_bm25_clause_batch: clauses of a query whose posting ranges a scoring workgroup searches at once (both scoring kernels); a longer
 *   query takes several batches, its sum stays the sequential one in clause order.
 * mq_bm25_impacts_f32: fills impact for all nnz postings (again after a change of k1 / b: the index itself stays).
 * mq_topk_rows_f32: exact top-k of every row of a dense fp32 matrix scores [rows, N] of NON-NEGATIVE values (N < 2^31, rows <=
 *   65535): D [rows, k] fp32 / I [rows, k] int64 best first, equal scores by ascending id (descending with MQ_KNN_FLAG_TIE_ID_DESC,
 *   the only flag accepted); an element equal to +0 is not a hit; slots beyond a row's hits are (-inf, -1); id_offset is added to
 *   every id.  Radix select on the key (score bits << 32) | id, integer atomics only: results are bit for bit reproducible.
 *   k <= MQ_KNN_MAX_K (MQ_EUNSUPPORTED beyond); ws: mq_topk_rows_workspace_bytes(rows, k).
 * mq_topk_rows_launch_info: the geometry of that selection for `rows` rows of N elements (host only, no HIP call; for tests and
 *   profiles): out[0] = workgroups that share one row, out[1] = histogram passes, out[2 + p] = the key shift of pass p.  MQ_EINVAL
 *   for the rows / N that mq_topk_rows_f32 refuses, and for out == NULL.
 * mq_bm25_search_f32: scores the nq queries in chunks of mq_bm25_chunk_queries(N, nq, budget_bytes) -- as many as keep the dense
 *   [chunk, N] fp32 score matrix within budget_bytes, at least one -- and selects each chunk's top-k; results do not depend on the
 *   chunking.  ws: mq_bm25_workspace_bytes(N, nq, k, budget_bytes).  Arguments are validated before any HIP call. */
#define MQ_BM25_BLOCK_ROWS 16384
int mq_bm25_block_rows(void);
int mq_bm25_clause_batch(void);
int mq_bm25_impacts_f32(const int32_t *doc_dev, const int32_t *tf_dev, const uint8_t *code_dev, const float *cache_dev, int64_t nnz,
                        float *impact_dev, void *stream);
size_t mq_topk_rows_workspace_bytes(int rows, int k);
int mq_topk_rows_launch_info(int rows, int64_t N, int64_t out[8]);
int mq_topk_rows_f32(const float *scores_dev, int rows, int64_t N, int k, int flags, int64_t id_offset, float *D_dev,
                     int64_t *I_dev, void *ws_dev, size_t ws_bytes, void *stream);
int mq_bm25_chunk_queries(int64_t N, int nq, size_t budget_bytes);
size_t mq_bm25_workspace_bytes(int64_t N, int nq, int k, size_t budget_bytes);
int mq_bm25_search_f32(const int64_t *ptr_dev, const int32_t *doc_dev, const float *impact_dev, int64_t N, int64_t n_terms,
                       const int32_t *qptr_dev, const int32_t *cterm_dev, const float *cweight_dev, int nq, int k, int flags,
                       int64_t id_offset, float *D_dev, int64_t *I_dev, void *ws_dev, size_t ws_bytes, size_t budget_bytes,
                       void *stream);
/* Parameter grid (the reference's `hp bm25` job): G settings of (k1, b), each given as its norm cache (caches [G][256] fp32, device),
 * searched over the SAME index without touching its impact array.  One sweep of the postings scores a tile of settings: a posting's
 * impact under setting g is float(tf / (tf + caches[g][code[doc]])) (the division in double), then weight * impact and the sum as in
 * mq_bm25_search_f32 -- D / I [G, nq, k] hold, slice by slice, bit for bit what mq_bm25_impacts_f32 with caches[g] followed by
 * mq_bm25_search_f32 gives.
 * mq_bm25_grid_tile: the most settings one sweep scores.  mq_bm25_grid_block_rows(g): documents per scoring workgroup when a tile
 *   holds g settings -- MQ_BM25_BLOCK_ROWS over the next power of two >= g (g = 1: mq_bm25_block_rows()); 0 outside 1 ... tile.
 * mq_bm25_grid_chunk_queries(N, nq, g, budget_bytes): queries per launch for a tile of g settings -- the most that keep the dense
 *   [g, chunk, N] fp32 score matrix within budget_bytes, g * chunk within the 65535 rows of a selection launch and the scoring launch
 *   below 2^31 threads; at least one.  ws: mq_bm25_grid_workspace_bytes(N, nq, min(G, tile), k, budget_bytes).
 * mq_bm25_search_grid_f32 walks the G settings in tiles (a last one may be partial) and the queries in chunks; results depend on
 *   neither.  Validation (before any HIP call) and the NULL conventions are mq_bm25_search_f32's; G < 1 is MQ_EINVAL. */
int mq_bm25_grid_tile(void);
int mq_bm25_grid_block_rows(int g);
int mq_bm25_grid_chunk_queries(int64_t N, int nq, int g, size_t budget_bytes);
size_t mq_bm25_grid_workspace_bytes(int64_t N, int nq, int g, int k, size_t budget_bytes);
int mq_bm25_search_grid_f32(const int64_t *ptr_dev, const int32_t *doc_dev, const int32_t *tf_dev, const uint8_t *code_dev,
                            const float *caches_dev, int G, int64_t N, int64_t n_terms, const int32_t *qptr_dev,
                            const int32_t *cterm_dev, const float *cweight_dev, int nq, int k, int flags, int64_t id_offset,
                            float *D_dev, int64_t *I_dev, void *ws_dev, size_t ws_bytes, size_t budget_bytes, void *stream);

/* ---- face detection: MTCNN (csrc/mtcnn.hip) -- what the reference runs through facenet_pytorch on a CUDA machine
 * (meerqat/image/face_detection.py).  The arithmetic restates the published detect_face (tests/mtcnn_restatement.py lists every
 * restated point; parity with facenet_pytorch on the published checkpoints is UNPINNED: the package is not in this image).  Networks:
 * fp32 FMA, fp32 accumulation.  Box geometry: separate fp32 multiplies and adds, as the elementwise tensor operations it restates.
 * Images: the packed layout of mq_warp_affine_faces_f32 (uint8 RGB, per-image byte offset, (h, w) pairs).
 *
 * A box record is MQ_MTCNN_REC floats: x1, y1, x2, y2, score, reg 0..3.
 * Packed weights (mq_mtcnn_weight_floats(net) floats): per layer, in network order, weight, bias and (where the layer has one) PReLU
 *   slope; convolutions and heads in the published [out][in][kh][kw] / [out][in] layout, the dense layers dense4 (R-Net) and dense5
 *   (O-Net) as [in][out] with `in` running over (c, y, x) of the map in front of them -- the published flatten order (x, y, c) is
 *   folded into that row order by the caller.
 * mq_mtcnn_resample_u8_f32: jobs [n_jobs][MQ_MTCNN_JOB] int64 = image, x0, y0, width, height of the rectangle (0-based; pixels outside
 *   the image read as 0), out_w, out_h, offset (floats) of the planar [3][out_h][out_w] result in out.  Adaptive average pooling
 *   ("area"), then (x - 127.5) * 0.0078125; a rectangle without pixels gives zeros.  A job whose result does not fit in out_floats
 *   writes nothing and raises *overflow.  max_out_pixels: the largest out_w * out_h (sizes the launch).
 * mq_mtcnn_pnet_f32: levels [n_levels][MQ_MTCNN_LEVEL] int64 = offset (floats) of the level's planar input, h, w, image, sub-group
 *   (scale number), index of the level's first cell inside its image (scale-major), offset (floats) into maps, 0; level_scale
 *   [n_levels] fp32.  Cells with prob >= threshold are appended to the image's list at [image * cap + position): rec, idx (candidate
 *   index: first cell + row-major cell), sub.  count [n_images] receives the number of passing cells even where it exceeds cap; then
 *   *overflow is raised and nothing is written past the list's end: grow cap and repeat.  The order of a list is unspecified
 *   (mq_mtcnn_nms_f32 sorts).  maps (tests; may be NULL): per level [5][ho][wo] = prob, reg 0..3.  max_tiles: the largest number of
 *   16 x 16 output tiles of a level.  n_levels <= 65535.  in_floats / maps_floats: the sizes of in and maps; a level whose input or
 *   maps would lie outside them is not run and raises *overflow.
 * mq_mtcnn_nms_f32: greedy NMS of n_seg segments [seg_start, seg_start + seg_count) of rec [n_total]; boxes whose score is not
 *   > score_gt take no part; by descending score, equal scores by ascending key (NULL: position in the segment); a box is dropped
 *   when its overlap with a kept box of the same sub (NULL: all the same) is > threshold; areas and intersections with +1.  The kept
 *   records, keys, subs and source positions are written from seg_start on in kept order, their number to out_count.  A seg_count
 *   that reaches past n_total, or above seg_cap (the capacity of every segment; 0: none given), is clipped, so a counter that ran
 *   past its list never reads the next image's.  ws: mq_mtcnn_nms_workspace_bytes(n_total).
 * mq_mtcnn_refine_f32: gathers segment g's first dst_start[g + 1] - dst_start[g] records to [dst_start[g], ...), applies the box
 *   regression (widths with +1 under MQ_MTCNN_REFINE_PLUS_ONE), rerec under MQ_MTCNN_REFINE_REREC, then trunc + pad against image g:
 *   out_pad [total][4] = y, ey, x, ex (1-based), valid = (ey > y - 1 && ex > x - 1), and the resampling job of the crop
 *   (crop_size x crop_size at offset k * 3 * crop_size^2; an invalid box gets an empty rectangle).  total = dst_start[n_seg]; records
 *   at or past out_cap are not written and raise *overflow.
 * mq_mtcnn_rnet_f32 / mq_mtcnn_onet_f32: crops [n][3][24][24] / [n][3][48][48] -> rec[k][4] = score, rec[k][5..8] = regression
 *   (an entry with valid[k] == 0 gets score -inf); O-Net also points [n][10] (x 0..4, y 0..4), and with MQ_MTCNN_ONET_POST maps them
 *   to pixels (w * p + x1 - 1) and applies the regression (+1) to rec in place. */
#define MQ_MTCNN_REC 9
#define MQ_MTCNN_JOB 8
#define MQ_MTCNN_LEVEL 8
#define MQ_MTCNN_PNET 0
#define MQ_MTCNN_RNET 1
#define MQ_MTCNN_ONET 2
#define MQ_MTCNN_NMS_UNION 0
#define MQ_MTCNN_NMS_MIN 1
#define MQ_MTCNN_REFINE_PLUS_ONE 1
#define MQ_MTCNN_REFINE_REREC 2
#define MQ_MTCNN_ONET_POST 1
int mq_mtcnn_weight_floats(int net);
int mq_mtcnn_resample_u8_f32(const uint8_t *images_dev, const int64_t *offsets_dev, const int32_t *hw_dev, int n_images,
                             const int64_t *jobs_dev, int64_t n_jobs, int64_t max_out_pixels, float *out_dev, int64_t out_floats,
                             int32_t *overflow_dev, void *stream);
int mq_mtcnn_pnet_f32(const float *in_dev, int64_t in_floats, const int64_t *levels_dev, const float *level_scale_dev, int n_levels,
                      int max_tiles, const float *weights_dev, float threshold, int n_images, int cap, float *rec_dev, int32_t *idx_dev,
                      int32_t *sub_dev, int32_t *count_dev, int32_t *overflow_dev, float *maps_dev, int64_t maps_floats, void *stream);
size_t mq_mtcnn_nms_workspace_bytes(int64_t n_total);
int mq_mtcnn_nms_f32(const float *rec_dev, int64_t n_total, const int64_t *seg_start_dev, const int32_t *seg_count_dev, int n_seg,
                     int64_t seg_cap,
                     const int32_t *key_dev, const int32_t *sub_dev, float score_gt, float threshold, int mode, float *out_rec_dev,
                     int32_t *out_key_dev, int32_t *out_sub_dev, int32_t *out_src_dev, int32_t *out_count_dev, void *ws_dev,
                     size_t ws_bytes, void *stream);
int mq_mtcnn_refine_f32(const float *in_rec_dev, const int64_t *seg_start_dev, const int64_t *dst_start_dev, int n_seg, int64_t total,
                        const int32_t *hw_dev, int flags, int crop_size, int64_t out_cap, float *out_rec_dev, int32_t *out_img_dev,
                        int32_t *out_pad_dev, int64_t *jobs_dev, int32_t *valid_dev, int32_t *overflow_dev, void *stream);
int mq_mtcnn_rnet_f32(const float *crops_dev, int64_t n, const float *weights_dev, const int32_t *valid_dev, float *rec_dev,
                      void *stream);
int mq_mtcnn_onet_f32(const float *crops_dev, int64_t n, const float *weights_dev, const int32_t *valid_dev, float *rec_dev,
                      float *points_dev, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MEERQAT_HIP_H */
