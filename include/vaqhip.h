/*
 * vaqhip.h -- C ABI of the MI355X (gfx950) implementation of VAQ's
 * quantized-distance search path.
 *
 * The reference has no FFI layer: the path sits behind C++ member functions
 * called directly by its drivers.  Each entry point below names the reference
 * interface it replaces (file:line under the reference checkout).  A C++
 * adapter with the reference's own names (class VaqHip: search(),
 * parseMethodString(), public mCodebook-style members) is in
 * include/vaqhip.hpp; INTEGRATION.md shows the binding a reference
 * maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types cross this boundary
 *  - every function returns 0 on success or a negative VAQHIP_E* code; the
 *    process is never exit()ed or assert()ed (the reference prints and
 *    exits: VAQ.cpp:64-78, 1263-1266); vaqhip_last_error() gives the text
 *  - "host" entry points take host pointers and are synchronous;
 *    "_device" entry points take device pointers on the index's GPU plus a
 *    hipStream_t (passed as void*), enqueue only, and never synchronise
 *  - the library has no CPU fallback: without a usable HIP device every call
 *    fails with VAQHIP_ENODEVICE
 *  - one index may be used from several host threads and several streams: calls on the same
 *    index are serialised internally on the host, and since every call shares the index's
 *    workspaces (lookup tables, partial lists, thresholds), a "_device" call on a stream other
 *    than the one the previous call used makes its stream wait (hipStreamWaitEvent) for that
 *    call's work first -- searches on one index never overlap on the GPU; use one index per
 *    stream (or vaqhip_multi) for concurrency
 */
#ifndef VAQHIP_H_
#define VAQHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAQHIP_VERSION 122

/* error codes */
#define VAQHIP_OK            0
#define VAQHIP_EINVAL       -1   /* bad argument (null, negative size, ...)                    */
#define VAQHIP_EUNSUPPORTED -2   /* valid for the reference but outside this build's limits     */
#define VAQHIP_ENODEVICE    -3   /* no usable HIP device / HIP runtime error at init            */
#define VAQHIP_ENOMEM       -4   /* device or host allocation failed                            */
#define VAQHIP_EHIP         -5   /* HIP runtime error during a call                             */
#define VAQHIP_ERANGE       -6   /* label would not fit the reference's 32-bit int labels       */
#define VAQHIP_ESTATE       -7   /* call order (e.g. search before codes were added)            */
#define VAQHIP_ENOCONV      -8   /* an iteration reached its limit (vaqhip_sym_eigen_*: 60 sweeps) */

/* search method bits, numerically equal to VAQ::NNMethod (VAQ.hpp:38-49).
 * HEAP and EA run the same kernels because the reference's early abandon
 * returns results identical to HEAP (VAQ.cpp:1694-1727 vs 1729-1758).  TI is
 * the triangle-inequality cluster pruning (VAQ.cpp:799-826, 1540-1692); see
 * vaqhip_index_set_ti_clusters. */
#define VAQHIP_METHOD_EA   0x02u
#define VAQHIP_METHOD_TI   0x04u
#define VAQHIP_METHOD_HEAP 0x80u
/* VAQ::searchFast (VAQ.cpp:1778-1834): uint8 tables over codes of at most 4 bits, integer row sums,
 * KNNFromDists' top-k; see vaqhip_index_set_lut_quantization */
#define VAQHIP_METHOD_FAST 0x08u

/* limits of this build */
#define VAQHIP_MAX_SUBSPACES 128
#define VAQHIP_MAX_BITS      15    /* VAQ.cpp:787-798 dispatches CreateLUT<9..15> */
#define VAQHIP_MAX_K         1024
#define VAQHIP_MAX_TI_CLUSTERS 4096 /* mTIClusterNum; the paper's runs use 100..2000 */

typedef struct vaqhip_index vaqhip_index;

/* ---------------------------------------------------------------------------
 * Index state = the public members VAQ::search reads (VAQ.hpp:51-75):
 *   D                 mTotalDim (= M * mSubsLen)
 *   M                 mHighestSubs; must be a multiple of 4 (VAQ.cpp:1741-1746
 *                     reads four codes per step)
 *   bits[M]           mBitsAlloc; mCentroidsNum[s] = 1 << bits[s]
 *   centroids[s]      mCentroidsPerSubs[s], row-major (1<<bits[s]) x (D/M)
 *   eigvec_real       real part of mEigenVectors, row-major D x D, or NULL for
 *                     identity (queries already in PCA space)
 *   device_id         HIP device ordinal the index lives on
 * Replaces: the state half of `class VAQ` consumed by search(), VAQ.hpp:51-75.
 * ------------------------------------------------------------------------- */
int vaqhip_index_create(vaqhip_index **out, int D, int M, const int *bits,
                        const float *const *centroids_rowmajor,
                        const float *eigvec_real_rowmajor, int device_id);

/* Same with flags.  VAQHIP_SUM_SEQUENTIAL selects the row sum of the reference's other
 * entry on this path, BitVecEngine::queryLUT (BitVecEngine.hpp:1222-1343): one scalar
 * quantiser per PCA dimension (D == M, sub-vector length 1), LUT column stride 256, and
 * dist = ((l_0 + l_1) + l_2) + ... summed column by column (:1296-1300) instead of in
 * groups of four; M need not be a multiple of 4.  centroids[s] is then column s of the
 * engine's centroidsMat (1 << bits[s] values).  Queries are projected WITH CHECKING, as queryLUT
 * does (:1226 -> :53-71): a PCA coordinate that comes out NaN or infinite becomes 0 (one non-finite
 * component makes every coordinate of z * V non-finite, so such a query is answered as the zero
 * vector); VAQ::search's projection (VAQ.hpp:198-201) does not check and is left as it is.
 * Option "exact_ties" reproduces queryLUT's own order among equal distances (below). */
#define VAQHIP_SUM_SEQUENTIAL 0x1u
int vaqhip_index_create_ex(vaqhip_index **out, int D, int M, const int *bits,
                           const float *const *centroids_rowmajor,
                           const float *eigvec_real_rowmajor, int device_id, unsigned flags);

void vaqhip_index_destroy(vaqhip_index *ix);

/* mCodebook (CodebookType = RowMatrix<uint16_t>, utils/Types.hpp:31), N x M
 * row-major.  The codes are repacked on the GPU into the bit-packed device
 * layout (DESIGN.md "Data layout"); the caller keeps ownership of the input.
 * Replaces the `mCodebook` member filled by VAQ::encode (VAQ.cpp:663-726) or
 * loadCodebook (utils/IO.hpp:551-571).  Calling it again replaces the codes.
 * id_base: global row index of local row 0 (shard offset); labels
 * returned by search are id_base + local row and must stay < 2^31.
 * Both forms sort the rows by their first code on the GPU (bucketed order,
 * DESIGN.md section 3) and therefore synchronise; the _device form does so on `stream`. */
int vaqhip_index_set_codes_u16(vaqhip_index *ix, const uint16_t *codes_rowmajor,
                               int64_t N, int64_t id_base);
int vaqhip_index_set_codes_u16_device(vaqhip_index *ix, const uint16_t *d_codes_rowmajor,
                                      int64_t N, int64_t id_base, void *stream);

/* Append n_new rows (same layout) behind the rows already in the index; their labels
 * continue at id_base + N.  Stands for growing `mCodebook` and calling the setter again
 * (SURVEY.md section 8b lists the entry point as `add_codes`).  A bucketed index sorts and packs
 * the NEW rows only and merges them into the existing order bucket by bucket: the packed rows and
 * their labels are copied once, nothing is unpacked or re-sorted, temporaries are O(n_new) plus
 * the new packed buffer; the bucket key width stays the one chosen when the codes were set.  A
 * TI-grouped index (rows ordered by cluster and centre distance) is rebuilt as a whole.
 * Synchronises. */
int vaqhip_index_add_codes_u16(vaqhip_index *ix, const uint16_t *codes_rowmajor, int64_t n_new);
int vaqhip_index_add_codes_u16_device(vaqhip_index *ix, const uint16_t *d_codes_rowmajor,
                                      int64_t n_new, void *stream);

/* VAQ::clusterTI (VAQ.hpp:106, VAQ.cpp:878-999) from the point where mTIClusters
 * exists: `clusters` is mTIClusters, T x (seg_num * D/M) row-major, i.e. T
 * centres over the first seg_num subspaces (mTIClusterNum, mTISegmentNum); how
 * they were made is the caller's business, like the codebooks (the reference's own
 * way, k-means over decoded codes, VAQ.cpp:897-900: vaqhip_index_cluster_ti_kmeans below).  Every code row joins its nearest
 * centre (VAQ.cpp:926-950), clusters are ordered farthest member first
 * (:972-979) and the packed codes are regrouped on the GPU (:984-996).  May be
 * called before or after the codes are set (the reference calls it after
 * encode); T = 0 returns the index to the exhaustive HEAP/EA form.  Sets /
 * clears VAQHIP_METHOD_TI in the index's method.  Synchronises.
 * Labels stay ORIGINAL row indices + id_base, as mTIClustersMember holds them. */
int vaqhip_index_set_ti_clusters(vaqhip_index *ix, const float *clusters_rowmajor, int T,
                                 int seg_num);

/* VAQ::clusterTI(true) (VAQ.cpp:896-900): the centres themselves, made on the GPU as the reference makes
 * them -- KMeans::staticFitCodebook (KMeans.hpp:618-652) -> staticFitSampling (:487-616) over the decoded
 * first seg_num codes of the index's rows in original row order:
 *   sample   N > 256 * T: rows randomPermutation(N)[0 .. 256 * T) (utils/Random.hpp:18-28, mt19937(13517106)),
 *            in that order; else all rows
 *   seeds    means[i] = row randomPermutation(rows)[i] of the sample
 *   Lloyd    until no centre changes or max_iter (the reference passes 50): nearest centre by
 *            sqrt(squaredNorm) with Eigen's summation order, strict `<`; sums in the order of the reference's
 *            two OpenMP threads; new = (p0 + p1) / float(count)
 * The result equals the reference's bit for bit where finite (compiled without -ffast-math and with
 * -ffp-contract=off, as everything this library is compared with).  An empty cluster is 0 / 0: its centre
 * becomes NaN, stays NaN, and the loop then runs to max_iter -- the reference's behaviour, reproduced, not
 * repaired (equal decoded rows among the seeds are enough for it).
 * Then exactly what vaqhip_index_set_ti_clusters(ix, means, T, seg_num) does.  clusters_out (T x seg_num * D/M),
 * iters_out (iterations run) and nan_rows_out (centres holding a NaN) may be NULL.
 * VAQHIP_ESTATE before the codes are set or while a staged search is open; VAQHIP_EINVAL for T < 1, T > N (the
 * reference reads out of bounds), seg_num outside 1..M, max_iter < 1; the limits of set_ti_clusters apply.
 * Calling it again, or after add_codes, clusters the codes then present.  Synchronises. */
int vaqhip_index_cluster_ti_kmeans(vaqhip_index *ix, int T, int seg_num, int max_iter, float *clusters_out,
                                   int *iters_out, int *nan_rows_out);
typedef struct {
  float total_ms;                             /* host time of the k-means: sample, gather, decode, iterations */
  float assign_ms, accumulate_ms, update_ms;  /* per phase over all iterations; only with option "timing" = 1
                                                 (each phase then ends with a stream synchronisation), else 0 */
  int iterations, rows, dims, clusters;       /* rows = the sample's */
} vaqhip_kmeans_timing;
/* figures of the last vaqhip_index_cluster_ti_kmeans on this index */
int vaqhip_last_kmeans_timing(vaqhip_index *ix, vaqhip_kmeans_timing *out);

/* mMethods (VAQ::parseMethodString, VAQ.cpp:1205-1262) and mVisit (VAQ.hpp:84,
 * demo_vaq --visit-cluster).  With TI:
 *   - the clusters visited are the first  max(int(T * visit), shortest prefix
 *     holding k rows)  in ascending query-to-centre distance (VAQ.cpp:1548-1555,
 *     :1611); visit >= 1 visits all;
 *   - TI | EA returns the k best of the visited rows; distances are sqrt'ed
 *     (VAQ.cpp:1583);
 *   - TI without EA returns the first k rows of the visiting order, as the
 *     reference does (its bsfKSquared stays 0, VAQ.cpp:1617-1686).
 * HEAP / EA without TI: the exhaustive scan; `visit` is ignored.
 * FAST (max bits <= 4, else VAQHIP_EUNSUPPORTED; not on VAQHIP_SUM_SEQUENTIAL indexes) runs only when
 * none of TI, EA, HEAP is set: the reference's precedence is TI > EA > HEAP > FAST (VAQ.cpp:799-834).
 * SORT, FAST2, FAST3 are refused (VAQHIP_EUNSUPPORTED). */
int vaqhip_index_set_method(vaqhip_index *ix, unsigned methods, float visit);

/* FAST: mOffsets[M] and mScale[M] (VAQ.hpp), the affine map smallQuantize applies to every table:
 *   q[s][c] = (uint8) min(floor(max(lut[s][c] - offsets[s], 0) * scale[s]), 255)   (Math.hpp:215-224)
 * Non-finite values or scale <= 0: VAQHIP_EINVAL.  Setting or appending codes keeps them.
 * With FAST in force, vaqhip_search* then answer as VAQ::searchFast does, slot for slot:
 *   distances  float(sum_s q[s][code[s]]) -- integers, no sqrt;
 *   labels     the k smallest rows by (dist, seq), seq = the row's position in KNNFromDists' std::sort
 *              of rows 0..k-1 (utils/Experiment.hpp:40-56), the row itself for rows >= k; id_base + row;
 *   N < k      unfilled slots -1 / FLT_MAX (the reference reads past its array there).
 * Without a quantisation: VAQHIP_ESTATE.  exact_ties has no effect (FAST is slot-exact by itself);
 * the staged search is VAQHIP_EUNSUPPORTED with FAST.  A vaqhip_multi answers FAST over its shards with the
 * same slots (vaqhip_multi_set_lut_quantization below).
 * Memory: while FAST is the method in force the index keeps a second copy of its codes in original row order
 * (16 * ceil(M / 32) bytes per row, built at the first FAST search) and up to 1 GiB of per-search workspace;
 * both are released when another method is set.  Indexes that never run FAST carry neither. */
int vaqhip_index_set_lut_quantization(vaqhip_index *ix, const float *offsets, const float *scale);

/* VAQ::learnQuantization(XTrain, ratio) (VAQ.cpp:1118-1187): sampleSize = int(ratio * float(n)) rows
 * (< 1: VAQHIP_EINVAL) in randomPermutation order (utils/Random.hpp:18-28, mt19937(13517106)), their
 * zero-padded tables, and per alpha in {.001, .002, .005, .01, .02, .05, .1} offsets = percentile(alpha),
 * scale = 255 / percentile(1 - alpha) of the offset tables; the alpha of least quantisation loss wins
 * (a later one on ties; the loss is summed in double, DESIGN.md "FAST").  X is n x D row-major,
 * projected != 0: already in PCA space.  The result is set on the index and, where the pointers are
 * not NULL, written to offsets_out[M] / scale_out[M]. */
int vaqhip_learn_quantization(vaqhip_index *ix, const float *X_rowmajor, int64_t n, int projected,
                              float sample_ratio, float *offsets_out, float *scale_out);

/* Learning on the device: vaqhip_learn_quantization over rows where they live and in the type they have -- host
 * bytes (_u8), device floats (_device), device bytes (_u8_device), or the rows resident in a refiner, float or
 * byte, read in place as raw rows (projected = 0).  offsets, scale and the chosen alpha are those of
 * vaqhip_learn_quantization on the same rows (a byte widened, (float)uint8 is exact), bit for bit.
 *   how         only the sampled rows are gathered (the first sampleSize entries of randomPermutation, found
 *               without building the permutation), their tables are built by the launches the host form makes
 *               and stay on the device; per column a radix sort, the few order statistics the fourteen
 *               percentiles read are fetched, floors and scales are computed on the host by the host form's
 *               code, and the loss is summed on the device in the host form's order: per (alpha, column) one
 *               chain of double additions over the table in sample-major, centroid-minor order.
 *   memory      the tables of at most Mc subspaces are held at a time ([sampleSize][Mc][16] floats) beside one
 *               column's sort buffers; Mc is the largest that fits the workspace of vaqhip_learn_set_workspace.
 *               The results do not depend on Mc.
 *   refusals    as the host form's, all before a device is touched: null index or rows, n <= 0 VAQHIP_EINVAL;
 *               n > INT_MAX VAQHIP_ERANGE; int(ratio * float(n)) < 1 VAQHIP_EINVAL; no FAST form
 *               VAQHIP_EUNSUPPORTED; a refiner without rows VAQHIP_ESTATE, of another D or device VAQHIP_EINVAL.
 *               Also sampleSize > n (a ratio above 1): VAQHIP_EINVAL -- the host form reads past its
 *               permutation there.  A table value that is NaN or infinite (a NaN in a sampled row), or no alpha
 *               of finite loss: VAQHIP_EINVAL, the outputs and the index's quantisation untouched.
 *   streams     the device forms run on the index's own stream and return when the result is set: the rows
 *               must be complete when the call is made. */
int vaqhip_learn_quantization_u8(vaqhip_index *ix, const uint8_t *X_rowmajor, int64_t n, int projected,
                                 float sample_ratio, float *offsets_out, float *scale_out);
int vaqhip_learn_quantization_device(vaqhip_index *ix, const float *d_X, int64_t n, int projected,
                                     float sample_ratio, float *offsets_out, float *scale_out);
int vaqhip_learn_quantization_u8_device(vaqhip_index *ix, const uint8_t *d_X, int64_t n, int projected,
                                        float sample_ratio, float *offsets_out, float *scale_out);
/* (vaqhip_learn_quantization_from_refiner is declared with the refiner, below) */
/* bytes the device forms called from this thread may hold for tables and sort buffers; 0 = the default (1 GiB).
 * A group of one subspace is taken even where it does not fit.  Negative: VAQHIP_EINVAL. */
int vaqhip_learn_set_workspace(int64_t bytes);
typedef struct vaqhip_learn_timing {
  int sample_rows, column_groups, chosen_alpha; /* chosen_alpha: index into the seven alphas, -1 = none was finite */
  float gather_ms, tables_ms, sort_ms, order_stats_ms, loss_ms, total_ms; /* host clock around each phase */
  double loss[7]; /* per alpha, the columns' losses added for s = 0 .. M - 1 */
} vaqhip_learn_timing;
/* the last device-form learn on this index (a multi index: on vaqhip_multi_shard(mx, 0)) */
int vaqhip_last_learn_timing(vaqhip_index *ix, vaqhip_learn_timing *out);

/* Test hook for FAST's smallQuantize(CreateLUT(query)): out[q*M*16 + s*16 + c], uint8; entries
 * c >= 1 << max(bits) (the reference's table has no such rows) are 0.  Needs max bits <= 4 and a
 * quantisation (VAQHIP_EUNSUPPORTED / VAQHIP_ESTATE). */
int vaqhip_build_small_lut(vaqhip_index *ix, const float *queries_rowmajor, int nq, int projected,
                           uint8_t *out);

/* VAQ::search (VAQ.hpp:102, VAQ.cpp:776-847), HEAP / EA semantics:
 *   queries   nq x D row-major, unprojected (projected by eigvec on the GPU)
 *   labels    nq x k, ascending by (distance, label); unfilled slots -1
 *   distances nq x k squared L2 in PCA space (no sqrt, VAQ.cpp:1737-1753);
 *             unfilled slots FLT_MAX (utils/Heap.hpp:322-349)
 * Among rows of exactly equal distance the smaller label wins (the
 * reference's choice there depends on heap internals; DESIGN.md "Ties"). */
int vaqhip_search(vaqhip_index *ix, const float *queries_rowmajor, int nq, int k,
                  int32_t *labels, float *distances);
/* queries already in PCA space (skips ProjectOnEigenVectors, VAQ.hpp:198-201) */
int vaqhip_search_projected(vaqhip_index *ix, const float *qproj_rowmajor, int nq, int k,
                            int32_t *labels, float *distances);
/* device pointers, enqueue on `stream` */
int vaqhip_search_device(vaqhip_index *ix, const float *d_queries, int nq, int k,
                         int projected, int32_t *d_labels, float *d_distances,
                         void *stream);

/* Staged search for hosts that shard the rows over several GPUs, one process (or index) per GPU: every
 * shard finds ITS k best, so on its own its admission thresholds are looser than the global k-th
 * distance allows.  `begin` runs the first rounds of the search (each query's nearest buckets) and
 * writes the thresholds they leave -- nq distance bit patterns, int32, ordered like the distances --
 * to d_thresholds_out; the caller takes the element-wise MINIMUM over all shards (one all-reduce of
 * 4 * nq bytes: a threshold is an upper bound of the query's final k-th distance, and any shard's
 * bound holds everywhere, the k rows behind it exist) and hands it to `finish`, which scans what is
 * still in reach under it.  A shard may then return fewer than k rows for a query (slots -1 / FLT_MAX):
 * the merge of the shards' lists (vaqhip_merge_topk_*) is the global result, bit for bit what one
 * index over all rows returns.  d_labels / d_distances of `begin` hold intermediate lists until `finish`
 * returns; no other call on the index in between (VAQHIP_ESTATE).  VAQHIP_EUNSUPPORTED when the search
 * would not run the bucket-major rounds (few queries, cache-resident or bit-packed rows, TI): use
 * vaqhip_search_device then -- vaqhip_search_staged_supported tells beforehand, so that all shards can
 * agree.  d_thresholds_in may be NULL (no exchange).  Replaces nothing in the reference (its search is
 * one process on one host, VAQ.cpp:776); it is the exchange step SURVEY 8(e) allows for. */
int vaqhip_search_staged_supported(vaqhip_index *ix, int nq, int k);
int vaqhip_search_begin_device(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                               int32_t *d_labels, float *d_distances, int32_t *d_thresholds_out, void *stream);
int vaqhip_search_finish_device(vaqhip_index *ix, const int32_t *d_thresholds_in, void *stream);

/* Test hook for VAQ::CreateLUT<maxbit> (VAQ.hpp:128-167): writes, per query,
 * the reference LUTType (column-major ksub x M, ksub = 1 << max(bits), rows
 * >= 1<<bits[s] zero): lut_out[q*M*ksub + s*ksub + c]. */
int vaqhip_build_lut(vaqhip_index *ix, const float *queries_rowmajor, int nq,
                     int projected, float *lut_out);

/* VAQ::ProjectOnEigenVectors (VAQ.hpp:198-201): out = X * real(eigvec). */
int vaqhip_project(vaqhip_index *ix, const float *X_rowmajor, int64_t n, float *out);

/* VAQ::encode / encodeImpl (VAQ.cpp:663-748): per subspace, argmin over centroids of the
 * squared L2 to the row's sub-vector (strict <, first minimum wins).  codes_out is the
 * reference's CodebookType, n x M uint16 row-major.  projected != 0: X is already in
 * PCA space, which is what the reference's encode() expects (train() projects the
 * dataset in place, VAQ.cpp:294); projected == 0 applies eigvec first. */
int vaqhip_encode(vaqhip_index *ix, const float *X_rowmajor, int64_t n, int projected,
                  uint16_t *codes_out);
int vaqhip_encode_device(vaqhip_index *ix, const float *d_X, int64_t n, int projected,
                         uint16_t *d_codes_out, void *stream);
/* Byte rows: the same calls over uint8 rows, n x D row-major, as a bvecs file stores them.  (float)uint8 is exact and
 * a byte is widened where the projection loads it, so the codes are those of the float call on the widened matrix,
 * code for code: the same refusals, codes and chunks; the host form uploads a quarter of the bytes.  Where no
 * projection runs (projected != 0, or no eigvec on an index that is not VAQHIP_SUM_SEQUENTIAL) a chunk is widened on the
 * device first.  The _device forms take ANY byte address (a view that starts at an odd offset): packed 4-byte loads
 * are used only where d_X is 4-byte aligned, and the result is that of an aligned copy.  This holds for every *_u8
 * call that builds an index below (vaqhip_encode_lut_u8*, vaqhip_lut_fit_quantiles_u8*, vaqhip_multi_*_u8). */
int vaqhip_encode_u8(vaqhip_index *ix, const uint8_t *X_rowmajor, int64_t n, int projected, uint16_t *codes_out);
int vaqhip_encode_u8_device(vaqhip_index *ix, const uint8_t *d_X, int64_t n, int projected,
                            uint16_t *d_codes_out, void *stream);

/* ---------------------------------------------------------------------------
 * Building a queryLUT index: BitVecEngine::binaryEncodingLUT (BitVecEngine.hpp:594-935) from the bit allocation
 * on.  The PCA (:596-617) and the glpk bit allocation (:622-809) stay the caller's: eigenvectors and bits per
 * dimension come in, as the reference's own parseAndLoadHardcoded / hardcodedSolutionX (:127-149) takes the bits.
 *
 * vaqhip_lut_fit_quantiles = centroidsQuantile (:811-840) for every dimension d, N = 1 << bits[d], over the
 * column sorted ascending (Z):
 *   Q[0] = Z.front(), Q[N] = Z.back(), Q[i+1] = (1 - (poi - left)) * Z[left] + (poi - left) * Z[right] with
 *   p = (float)(i+1)/N, poi = float((1 - p) * (-0.5) + p * ((float)n - 0.5)) -- the products and the sum in
 *   double --, left = max(floor(poi), 0), right = min(ceil(poi), n - 1);
 *   bucket i = the values from where bucket i-1 ended up to the first Z > Q[i+1]; its centre is the float sum of
 *   its values, ONE ADD AFTER ANOTHER in ascending order from +0, divided by the count; an empty bucket gets
 *   (Q[i] + Q[i+1]) / 2.
 *   X              n x D row-major (the reference's matrix is column-major); in PCA space when eigvec is NULL,
 *                  else out = X * eigvec is taken first WITHOUT checking, as :620 does
 *   bits[D]        solutionX, 1..8 each
 *   centroids_out  256 x D column-major, the layout of centroidsMat (column d at centroids_out + 256 * d, rows
 *                  >= N zero)
 *   quantiles_out  D x 257 (row d = Q[d][0 .. N], the rest zero)
 * Refused with VAQHIP_EINVAL: bits outside 1..8, n < 1, n >= 2^31, a NaN or infinite (projected) training value
 * (std::sort has no defined result on NaN) -- the outputs are then left untouched.  A column holding both -0 and
 * +0 is sorted with -0 first where std::sort's order among them is unspecified: only the sign of a zero in Q can
 * differ.  Workspace: two key buffers of n words (one column at a time), plus the projected rows when eigvec is
 * given.  The result equals a build of the reference without -ffast-math and with -ffp-contract=off bit for bit
 * by construction; it is not pinned against a compiled reference (BitVecEngine.hpp needs glpk.h).
 * The _device form takes device pointers (bits stays a host array) and works on `stream`, which it
 * synchronises before it returns (the refusal above is known only then). */
int vaqhip_lut_fit_quantiles(int device_id, const float *X_rowmajor, int64_t n, int D, const int *bits,
                             const float *eigvec_real_rowmajor, float *centroids_out, float *quantiles_out);
int vaqhip_lut_fit_quantiles_device(int device_id, const float *d_X, int64_t n, int D, const int *bits,
                                    const float *d_eigvec, float *d_centroids_out, float *d_quantiles_out,
                                    void *stream);
/* the same over uint8 rows (see vaqhip_encode_u8): the float call's result on the widened matrix, bit for bit; with
 * eigvec the projection widens the bytes, without it the column extract does, and no float copy of the rows is made */
int vaqhip_lut_fit_quantiles_u8(int device_id, const uint8_t *X_rowmajor, int64_t n, int D, const int *bits,
                                const float *eigvec_real_rowmajor, float *centroids_out, float *quantiles_out);
int vaqhip_lut_fit_quantiles_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, const int *bits,
                                       const float *d_eigvec, float *d_centroids_out, float *d_quantiles_out,
                                       void *stream);
typedef struct {
  float total_ms;                                    /* host time of the last fit on this thread, copies excluded */
  float project_ms;                                  /* only with vaqhip_lut_fit_set_timing(1), else 0: */
  float extract_ms, sort_ms, quantile_ms, means_ms;  /*   device time per phase, summed over the columns */
  int64_t rows;
  int dims;
} vaqhip_lut_fit_timing;
int vaqhip_lut_fit_set_timing(int on);                       /* per calling thread */
int vaqhip_last_lut_fit_timing(vaqhip_lut_fit_timing *out);  /* the calling thread's last fit */

/* Keeps Q (D x 257, as vaqhip_lut_fit_quantiles writes it) on a VAQHIP_SUM_SEQUENTIAL index, whose centroids are
 * the matching centres; VAQHIP_EINVAL on any other index, for bits above 8 and for a NaN in Q. */
int vaqhip_index_set_lut_quantiles(vaqhip_index *ix, const float *quantiles);

/* encodeToLUTCode (:889-932): per row x and dimension j, the first q in 0..N with x <= Q[j][q]; none (x above
 * the range, NaN): code N - 1; q == 0: 0; q == 1: |x - c[0]| <= |x - c[1]| ? 0 : 1; q == N: m = |x - c[N-1]|,
 * l = |x - c[N-2]|, m <= l ? N - 1 : N - 2; else m = |x - c[q-1]|, l = |x - c[q-2]|, r = |x - c[q]|:
 * m <= l && m <= r gives q - 1, else l <= m && l <= r gives q - 2, else q.  (With bits == 1, q == 1 is tested
 * first.)  NOT vaqhip_encode's first global argmin under strict <: the two differ where distances tie and
 * outside the training range.  codes_out is n x D uint16 row-major, what vaqhip_index_set_codes_u16* takes.
 * projected == 0 applies eigvec first, unchecked (:620).  VAQHIP_ESTATE before the quantiles are set. */
int vaqhip_encode_lut(vaqhip_index *ix, const float *X_rowmajor, int64_t n, int projected, uint16_t *codes_out);
int vaqhip_encode_lut_device(vaqhip_index *ix, const float *d_X, int64_t n, int projected, uint16_t *d_codes_out,
                             void *stream);
/* the same over uint8 rows (see vaqhip_encode_u8) */
int vaqhip_encode_lut_u8(vaqhip_index *ix, const uint8_t *X_rowmajor, int64_t n, int projected, uint16_t *codes_out);
int vaqhip_encode_lut_u8_device(vaqhip_index *ix, const uint8_t *d_X, int64_t n, int projected, uint16_t *d_codes_out,
                                void *stream);

/* ---------------------------------------------------------------------------
 * Fitting the subspace codebooks mCentroidsPerSubs: KMeans::staticFitSampling (KMeans.hpp:487-616), the call of
 * VAQ.cpp:644-649 -- KMeans::staticFitSampling(XTrain.block(0, s * L, n, L), 1 << bits[s], 25) for every subspace s.
 * It is NOT the arma::kmeans call VAQ::train runs today beside it (armadillo: not reproduced).  eigvec and bits come
 * in: the caller's, or vaqhip_train_rotation's below.  With this an index is built on the device from raw rows:
 * fit, vaqhip_index_create with the centres, vaqhip_encode.
 *   X              n x D row-major; in PCA space when eigvec is NULL, else X * eigvec by vaqhip_project's chain, unchecked
 *   M, bits[M]     M subspaces of L = D / M columns, k_s = 1 << bits[s] centres, 1 <= bits[s] <= VAQHIP_MAX_BITS
 *   sample         decided PER SUBSPACE, as every call of the reference decides for itself (KMeans.hpp:489-503): with
 *                  size_s = max(256 * k_s, 65536), subspace s works on all n rows in their own order when n <= size_s,
 *                  else on rows randomPermutation(n)[0 .. size_s) (mt19937(13517106)) in that order; rows_s =
 *                  min(n, size_s).  One batch may hold both kinds (65536 < n <= 256 * k_max with a smaller k_s beside
 *                  it): a subspace that samples never works on rows 0 .. rows_s-1 in order.  The head of the permutation
 *                  for a smaller sample is a prefix of the head for a larger one, so one sample -- the largest among the
 *                  subspaces that sample -- is gathered and each of them works on its prefix; the subspaces that do
 *                  not sample read the full matrix, projected or widened whole where eigvec or byte rows require it
 *                  (the sample is then gathered from the projected matrix: a row's projection is its own).
 *   seeds          means[i] = row randomPermutation(rows_s)[i] of the subspace's rows_s rows
 *   Lloyd          until no centre of the subspace changes or max_iter (the reference passes 25): assign by
 *                  sqrt((x - mean).squaredNorm()) in Eigen's summation order over the L floats (plain sequential for
 *                  L < 8), centres ascending, strict <; sums in the order of the reference's two OpenMP threads (rows
 *                  [0, ceil(rows_s / 2)) and the rest, each ascending from +0); new = ((0 + p0) + p1) / float(count).
 *                  An empty cluster becomes NaN and stays NaN, and that subspace runs to max_iter, as the reference's.
 *   centroids_out  the M matrices back to back in subspace order, k_s x L row-major each (sum of k_s * L floats): what
 *                  vaqhip_index_create takes
 *   iters_out[M]   the reference's iter_count per subspace (the iteration that changes nothing is counted); may be NULL
 *   nan_rows_out[M]  centres of the subspace that hold a NaN; may be NULL.  Both are host arrays in every form.
 * Every centre equals the reference's bit for bit (a NaN by position), pinned by tests/golden/codebooks.  All
 * subspaces are fitted together, one launch per phase and iteration; no value of a subspace depends on another.
 * Refused before any device work, the outputs left untouched: VAQHIP_EINVAL for a null X, bits or centroids_out,
 * n < 1, n >= 2^31, M < 1, D % M != 0, max_iter < 1, bits outside 1..VAQHIP_MAX_BITS, and 1 << bits[s] above that
 * subspace's rows_s (the reference seeds from rows out of bounds); VAQHIP_EUNSUPPORTED for M > VAQHIP_MAX_SUBSPACES
 * and D > 4096.  Known only after the run: VAQHIP_EINVAL when a row is
 * at a distance >= FLT_MAX or NaN from every centre (the reference indexes row -1); VAQHIP_ENOMEM from a failed
 * allocation (nothing is kept).  Workspace: the projected sample (sample x D floats, twice with a gathered sample and
 * eigvec), n x D floats more when a subspace reads all rows and they are bytes or rotated, and 16 bytes per
 * (subspace, row it works on).  The host forms upload only the sample when every subspace samples, else all rows; the
 * _device forms take
 * device pointers for X, eigvec and centroids_out (bits and the two small outputs stay host arrays), work on
 * `stream` and synchronise it before they return.  The _u8 forms: the float call's result on the widened matrix, bit
 * for bit (see vaqhip_encode_u8; any byte address in the _device form). */
int vaqhip_fit_codebooks(int device_id, const float *X_rowmajor, int64_t n, int D, int M, const int *bits,
                         const float *eigvec_real_rowmajor, int max_iter, float *centroids_out, int *iters_out,
                         int *nan_rows_out);
int vaqhip_fit_codebooks_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                int *nan_rows_out, void *stream);
int vaqhip_fit_codebooks_u8(int device_id, const uint8_t *X_rowmajor, int64_t n, int D, int M, const int *bits,
                            const float *eigvec_real_rowmajor, int max_iter, float *centroids_out, int *iters_out,
                            int *nan_rows_out);
int vaqhip_fit_codebooks_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                   const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                   int *nan_rows_out, void *stream);
typedef struct {
  float total_ms;                          /* host time of the last fit on this thread, the copies of the host forms excluded */
  float gather_ms;                         /* only with vaqhip_fit_codebooks_set_timing(1), else 0: gather, project, seeds */
  float assign_ms, accumulate_ms, update_ms;  /*   summed over the iterations; accumulate = sort + run bounds + sums */
  int iterations;                          /* the largest iteration count of a subspace */
  int subspaces, dims;
  int64_t sample_rows;                     /* the most rows a subspace worked on: max rows_s (n when one read all rows) */
  int64_t rows;
} vaqhip_fit_codebooks_timing;
int vaqhip_fit_codebooks_set_timing(int on);                             /* per calling thread */
int vaqhip_last_fit_codebooks_timing(vaqhip_fit_codebooks_timing *out);  /* the calling thread's last fit */

/* ---------------------------------------------------------------------------
 * The hierarchical form of the fit above: VAQ::train with mHierarchicalKmeans (demo_vaq --kmeans-ver 1; VAQ.cpp:535-594).
 * Inputs and outputs are vaqhip_fit_codebooks's.  B = sum(bits), L = D / M, k_s = 1 << bits[s].
 *   flat subspaces   bits[s] <= 8: fitted exactly as vaqhip_fit_codebooks fits them -- the same rows, seeds, Lloyd loop
 *                    and NaN centres.  A call in which no subspace exceeds 8 bits IS vaqhip_fit_codebooks, bit for bit.
 *   hierarchical     bits[s] > 8: two stages, K1 = 128 and K2 = 1 << (bits[s] - 7) centres.
 *   rows R_s         rows_s = min(n, max(256 * k_s, 256 << (B / M))) (VAQ.cpp:535-536, integer division).  Row i of R_s
 *                    is row randomPermutation(n)[i] of the projected matrix, for every rows_s, also when rows_s == n
 *                    (VAQ.cpp:539-543).  The reference leaves the slice unfilled when rows_s < n: a defect, not a rule;
 *                    here it is always filled.  Heads of one permutation are prefixes of each other: one gather of the
 *                    largest serves every hierarchical subspace (and every flat one that samples).
 *   stage 1          C1 = KMeans::staticFitSampling(R_s[:, s*L .. (s+1)*L), 128, max_iter) as that function behaves
 *                    when handed those rows: with rows_s > 65536 it works on rows randomPermutation(rows_s)[0 .. 65536)
 *                    of R_s; its seeds are the head of randomPermutation(rows it works on); its two OpenMP halves are
 *                    the flat fit's.  This stands for the reference's arma::kmeans call there (armadillo: not
 *                    reproduced) -- the substitution this library makes everywhere (see vaqhip_fit_codebooks).
 *   membership       of ALL rows_s rows of R_s (getBelongsToCluster, VAQ.cpp:1272-1292): the nearest of the 128 centres
 *                    by (x - c).squaredNorm() in Eigen's summation order (plain sequential for L < 8), centres
 *                    ascending, strict <.  NO sqrt, unlike the Lloyd assign: two distinct squares whose roots round to
 *                    one float choose different centres under the two rules.  Group i keeps its rows in ascending
 *                    position within R_s.
 *   stage 2          for i = 0..127: staticFitSampling(rows of group i, K2, max_iter) with its own seeds (the head of
 *                    randomPermutation(m_i), m_i the group's rows), its own halves [0, ceil(m_i / 2)) and the rest, its
 *                    own stopping and its own NaN centres.  Its centres are rows i * K2 .. (i + 1) * K2 - 1 of the
 *                    subspace's block of centroids_out (VAQ.cpp:593).
 *   iters_out[s]     the largest iteration count among the subspace's 129 fits; nan_rows_out[s] the NaN centres among
 *                    its final k_s.
 * The flat subspaces and every 128-centre fit run as ONE batch of the flat fit's phases; stage 2 of all groups of all
 * hierarchical subspaces as one more, over a compact matrix regrouped by a stable sort.  A row meets 128 + K2 centres
 * per iteration in place of k_s.
 * Parity: VAQ.cpp does not compile, so the composition is not pinned against the compiled reference; each component is
 * (staticFitSampling: tests/golden/codebooks; randomPermutation; Eigen's squaredNorm), and the oracle is the
 * composition of their numpy restatements (tests/codebooks_hier_ref.py).
 * Refused before any device work, the outputs untouched: everything vaqhip_fit_codebooks refuses, and rows_s < k_s for
 * a hierarchical subspace.  Refused after stage 1, outputs untouched, the message naming subspace and group:
 * VAQHIP_EINVAL when a stage-1 centre is NaN or a group is empty (the reference asserts "hierarchical kmeans failed"),
 * when m_i < K2 (the reference seeds from rows out of bounds), when a row has no centre (squared distance NaN or
 * >= FLT_MAX from all 128); VAQHIP_EUNSUPPORTED when m_i > max(256 * K2, 65536): there the reference's stage 2 would
 * sample the group.  That happens under extreme skew, and regularly at 15 bits, where the average group already holds
 * 256 * K2 = 65536 rows; it is left out on purpose (vaqhip_fit_codebooks_bin below never refuses on group sizes).
 * Not built either: a multi-device form.
 * The host forms upload all rows when a subspace is hierarchical.  _device and _u8 forms: as vaqhip_fit_codebooks's. */
int vaqhip_fit_codebooks_hier(int device_id, const float *X_rowmajor, int64_t n, int D, int M, const int *bits,
                              const float *eigvec_real_rowmajor, int max_iter, float *centroids_out, int *iters_out,
                              int *nan_rows_out);
int vaqhip_fit_codebooks_hier_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                     const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                     int *nan_rows_out, void *stream);
int vaqhip_fit_codebooks_hier_u8(int device_id, const uint8_t *X_rowmajor, int64_t n, int D, int M, const int *bits,
                                 const float *eigvec_real_rowmajor, int max_iter, float *centroids_out, int *iters_out,
                                 int *nan_rows_out);
int vaqhip_fit_codebooks_hier_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                        const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                        int *nan_rows_out, void *stream);
typedef struct {
  float total_ms;                       /* host time of the last hierarchical fit on this thread, host copies excluded */
  float stage1_ms;                      /* sources, seeds and the batch of flat subspaces and 128-centre fits */
  float regroup_ms;                     /* membership, stable sort, group bounds, gather into the compact matrices */
  float stage2_ms;                      /* the batch of all groups' K2-centre fits */
  int groups;                           /* 128 per hierarchical subspace */
  int min_group_rows, max_group_rows;   /* the smallest and the largest group */
  int stage1_iterations, stage2_iterations;  /* the largest iteration count of a fit of the stage */
  int hier_subspaces;                   /* 0: the call was the flat fit (stage1_ms = total_ms) */
  int subspaces, dims;
  int64_t rows;
} vaqhip_fit_codebooks_hier_timing;
int vaqhip_last_fit_codebooks_hier_timing(vaqhip_fit_codebooks_hier_timing *out);  /* the calling thread's last one */

/* ---------------------------------------------------------------------------
 * The binary-tree form of the fit: VAQ::train with mBinaryKmeans (hierarchicalBinKmeans, VAQ.cpp:1293-1371; demo_vaq
 * --kmeans-ver 2).  Inputs and outputs are vaqhip_fit_codebooks's.  B = sum(bits), L = D / M, k_s = 1 << bits[s].
 *   flat subspaces   bits[s] <= 8: the flat fit's, exactly, as in the hierarchical form.  A call in which no subspace
 *                    exceeds 8 bits IS vaqhip_fit_codebooks, bit for bit.
 *   rows R_s         of a subspace with bits[s] > 8: exactly the hierarchical form's -- rows_s = min(n, max(256 * k_s,
 *                    256 << (B / M))), row i = row randomPermutation(n)[i] of the projected matrix, always filled; one
 *                    gathered head serves every reader.
 *   node (d, j)      depth d = 1 .. maxdepth = bits[s], tempK = 1 << (maxdepth - d + 1).  The root (1, 0) holds R_s.
 *                    Node (d, j) owns rows [j * tempK, (j + 1) * tempK) of the subspace's block of centroids_out
 *                    (VAQ.cpp:1361-1367: the left block first).
 *   2-centre fit     C = KMeans::staticFitSampling(node rows, 2, max_iter) as that function behaves on those rows: above
 *                    65536 rows it works on rows randomPermutation(m)[0 .. 65536) of the node; its seeds are the head of
 *                    randomPermutation(rows it works on); its halves [0, ceil(m / 2)) and the rest; its NaN centres and
 *                    its stopping are its own.  It stands for the reference's arma::kmeans, as everywhere in this library.
 *   leaf             d == maxdepth: the two centres are the node's output.
 *   split            getBelongsToBinaryCluster (VAQ.cpp:1293-1310) over ALL m rows of the node: left = (x - C0)
 *                    .squaredNorm(), right = (x - C1).squaredNorm(), each in Eigen's summation order (sequential for
 *                    L < 8), NO sqrt; the row goes left iff left < right (strict).  A tie and a NaN on either side go
 *                    right; there is no "row without a centre": a NaN centre 0 sends every row right.
 *   cut              sizeleft < tempK / 2 or sizeright < tempK / 2: the node's output is staticFitSampling(node rows,
 *                    tempK, max_iter) -- sampling for itself above max(256 * tempK, 65536) rows, with its own seeds --
 *                    and the recursion stops there.  Every node holds at least tempK rows once rows_s >= k_s.
 *   children         else (d + 1, 2j) takes the left rows and (d + 1, 2j + 1) the right ones, each in ascending
 *                    position within the node (VAQ.cpp:1345-1351): that order makes the children's sums the reference's.
 *   iters_out[s]     the largest iteration count among the subspace's fits; nan_rows_out[s] the NaN centres among its
 *                    final k_s.
 * The tree is walked level by level: the 2-centre fits of all live nodes of all binary subspaces are ONE batch of the
 * flat fit's phases (the first level's carries the flat subspaces), then one split pass, a stable sort, the sizes back
 * to the host, the cut fits as one more batch, and a gather into the next level's compact matrix.  The batches' ordered
 * sums run through a kernel in which a wavefront owns a run and stages its rows through LDS: the additions per (run,
 * column) are the flat fit's, from +0 in ascending row order.
 * Parity: as for the hierarchical form -- VAQ.cpp does not compile, every component is pinned, the oracle is the
 * composition of the numpy restatements (tests/codebooks_bin_ref.py).
 * Refused before any device work, the outputs untouched: everything vaqhip_fit_codebooks refuses, and rows_s < k_s for
 * a binary subspace.  After the run: VAQHIP_EINVAL when a Lloyd assign meets a row at NaN or >= FLT_MAX from every
 * centre (the flat rule).  Group sizes never refuse: this is the form for inputs the hierarchical one refuses.
 * Not built: a multi-device form.  The host forms upload all rows when a subspace is binary. */
int vaqhip_fit_codebooks_bin(int device_id, const float *X_rowmajor, int64_t n, int D, int M, const int *bits,
                             const float *eigvec_real_rowmajor, int max_iter, float *centroids_out, int *iters_out,
                             int *nan_rows_out);
int vaqhip_fit_codebooks_bin_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                    const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                    int *nan_rows_out, void *stream);
int vaqhip_fit_codebooks_bin_u8(int device_id, const uint8_t *X_rowmajor, int64_t n, int D, int M, const int *bits,
                                const float *eigvec_real_rowmajor, int max_iter, float *centroids_out, int *iters_out,
                                int *nan_rows_out);
int vaqhip_fit_codebooks_bin_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                       const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                       int *nan_rows_out, void *stream);
typedef struct {
  float total_ms;                       /* host time of the last binary fit on this thread, host copies excluded */
  float fit_ms;                         /* sources, seeds and the levels' batches of 2-centre fits (and the flat subspaces) */
  float split_ms;                       /* split pass, stable sort, bounds, counts to the host, regroup */
  float cut_ms;                         /* the batches of the cut nodes' flat fits */
  int levels;                           /* levels walked: the deepest node's depth */
  int nodes;                            /* 2-centre fits run */
  int cut_nodes;                        /* nodes that ended in a flat fit of tempK centres */
  int resampled_fits;                   /* fits, 2-centre or cut, that sampled their node's rows */
  int leaf_nodes;                       /* nodes at depth bits[s] */
  int min_leaf_rows, max_leaf_rows;     /* the smallest and the largest of them (0: no path reached leaf depth) */
  int max_iterations;                   /* the largest iteration count of a fit */
  int bin_subspaces;                    /* 0: the call was the flat fit (fit_ms = total_ms) */
  int subspaces, dims;
  int64_t rows;
} vaqhip_fit_codebooks_bin_timing;
int vaqhip_last_fit_codebooks_bin_timing(vaqhip_fit_codebooks_bin_timing *out);  /* the calling thread's last one */
/* per calling thread, for tests and measurements: 0 (default) the staged ordered sums, 1 the flat fit's one-thread-per-run
 * kernel; the centres are the same bit for bit.  VAQHIP_EINVAL for another value. */
int vaqhip_fit_codebooks_bin_set_sums(int mode);

/* ---------------------------------------------------------------------------
 * Training from raw rows: the front half of VAQ::train (VAQ.cpp:11-524) -- the second moment of the sampled rows, its
 * eigen-decomposition, the partial balance of the leading dimensions and the ILP that hands each subspace its bits.
 * With vaqhip_fit_codebooks above an index is built from raw rows and a bit budget alone.  The parity contract:
 *   covmat       The reference builds XtX in float through Eigen's blocked GEMM (no mean is subtracted: a second moment);
 *                its summation order is NOT reproduced.  Here the sum is taken in double -- the product of two floats is
 *                exact, only the additions round -- in a fixed order: the rows are those of VAQ.cpp:17-24 (with
 *                s = 1000 * D < n the rows randomPermutation(n)[0 .. s) in that order, mt19937(13517106); else all rows
 *                in order), gathered where they are loaded; sample positions are cut into tiles of 1024; within a tile
 *                the products are added in ascending position from +0; the tile partials are added in ascending tile
 *                order from +0; no floating-point atomics, no MFMA.  Every entry (i, j) follows the same order: the
 *                matrix is exactly symmetric.  It lies within gamma_n * sum_r |x_ri x_rj| of the reference's entry by
 *                entry (gamma_n = n u / (1 - n u), u = 2^-24, n the rows summed); integer-valued rows (bvecs) with
 *                n * 255^2 < 2^53 give the exact integer in any order.  A non-finite input propagates; nothing is
 *                filtered.  cov_f_out (may be NULL): the same matrix rounded to float.
 *   eigen        Eigen::EigenSolver (real Schur in float, signs arbitrary) cannot be matched bit for bit.  Here: a cyclic
 *                two-sided Jacobi in double with round-robin ordering, two ordinary launches per step (no cooperative
 *                launch, no grid barrier, no spinning), one read-back per sweep.  A pair is rotated when
 *                |a_pq| > 2^-52 sqrt(|a_pp a_qq|) (zero product: a_pq != 0) by theta = (a_qq - a_pp) / (2 a_pq),
 *                t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c; a_pq = a_qp = 0 after it.
 *                Stops after the first sweep that rotates nothing (sweeps_out counts the sweeps that rotated: 0 for a
 *                diagonal matrix or D = 1) or with VAQHIP_ENOCONV when sweep 60 still rotated.  A NaN or Inf in A:
 *                VAQHIP_EINVAL before the first sweep.  A (D x D double, row-major) is destroyed.  After the sweeps
 *                every vector is divided by its norm (a product of hundreds of rotations drifts from length 1) and its
 *                eigenvalue is its Rayleigh quotient v^T (A v) on the matrix as it came, all sums in ascending index
 *                from +0, on the host in both forms (2 D^3 host operations).  Eigenvalues
 *                descending, equal ones by ascending original column; each vector (a COLUMN of the row-major D x D
 *                matrix, like eigvec everywhere) has its component of largest magnitude positive, the first such on
 *                ties.  vaqhip_sym_eigen_host is the same algorithm on the host from the same header
 *                (vaq_train_rot.h).  What is pinned: the invariants (residual, orthogonality, eigenvalues against
 *                LAPACK) and the DECISIONS the reference takes from its eigenvalues, not the solver's bits.
 *   plan         VAQ.cpp:80-96, 243-280, 301-336, 374-412 restated in float BIT FOR BIT from a vector of eigenvalues (in
 *                the solver's order): sorted_out[D] the columns by descending value (may be NULL), order_out[D] the same
 *                after the partial balance (with its break at the first swap that leaves the per-subspace sums
 *                unsorted; swaps_kept_out, may be NULL), var_out[M] varExplainedPerSubs in Eigen's sum() /
 *                segment().sum() order after the division by the sum and the clamp to 1e-12, cum_out[M] the sequential
 *                cumSum, highest_subs, lb_out[highest_subs] (min_bits where cum <= percent_var, else 0),
 *                k_out[highest_subs - 1] = nextPow2 of the float ratio widened to double, clamped to [0, 2^30] (the
 *                reference's (int) cast of a larger power is undefined; any k >= max_bits constrains nothing).
 *                lb_out and k_out have room for M and M - 1 entries.  VAQHIP_EINVAL: D % M != 0 (the reference rounds
 *                the subspace length up and reads past the end), min_bits > max_bits, max_bits > VAQHIP_MAX_BITS,
 *                M > VAQHIP_MAX_SUBSPACES, a non-finite eigenvalue, a non-positive eigenvalue sum.
 *   allocation   maximise sum c_i x_i subject to sum x_i = budget, lb_i <= x_i <= max_bits, x_i - x_(i+1) <= k_i, solved
 *                EXACTLY by dynamic programming over (subspace, its bits, bits spent); c_i the float coefficients widened
 *                to double as glpk receives them, objective sums in double in ascending i.  Where several allocations
 *                reach the optimum the lexicographically greatest is taken (most bits to subspace 0, then 1, ...):
 *                glpk's choice among ties is unknown and not reproduced.  The reference's repair loop for totalBit <
 *                mBitBudget (VAQ.cpp:473-498) cannot trigger under the equality constraint and is not restated.
 *                VAQHIP_EINVAL when no allocation satisfies the constraints (the reference asserts).
 *   composite    vaqhip_train_rotation*: moment -> eigen -> plan -> allocation.  eigvec_out: float D x D, columns in
 *                balanced order -- what vaqhip_project, vaqhip_fit_codebooks and vaqhip_index_create take;
 *                eigenvalues_out[D] in that order (may be NULL); bits_out[M] (entries from highest_subs on are 0);
 *                highest_subs_out.  LIMIT: when percent_var < 1 leaves a subspace with 0 bits or highest_subs < M the
 *                outputs are returned as they are, and the caller must not pass them to vaqhip_fit_codebooks, which
 *                takes 1..VAQHIP_MAX_BITS over all M subspaces (the chained forms of the adapters return
 *                VAQHIP_EUNSUPPORTED there rather than guessing).
 * Refused before any device work: null pointers, n < 1, n >= 2^31, D < 1, D > 4096 (VAQHIP_EINVAL), and the plan's
 * refusals.  The host forms upload only the sample; the _device forms take device pointers for the rows and the
 * matrices (eigenvalues, bits and highest_subs stay host values), work on `stream` and synchronise it.  The _u8 forms
 * widen a byte where it is loaded: the float call's result on the widened rows, bit for bit.  The refiner forms read a
 * single-device refiner's resident rows of either type in place; VAQHIP_ESTATE without rows.  Not provided: the
 * multi-device forms.
 * ------------------------------------------------------------------------- */
int vaqhip_train_moment(int device_id, const float *X_rowmajor, int64_t n, int D, double *cov_out, float *cov_f_out);
int vaqhip_train_moment_device(int device_id, const float *d_X, int64_t n, int D, double *d_cov_out, float *d_cov_f_out,
                               void *stream);
int vaqhip_train_moment_u8(int device_id, const uint8_t *X_rowmajor, int64_t n, int D, double *cov_out, float *cov_f_out);
int vaqhip_train_moment_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, double *d_cov_out,
                                  float *d_cov_f_out, void *stream);
int vaqhip_sym_eigen_device(int device_id, double *d_A, int D, double *d_values, double *d_vectors, int *sweeps_out,
                            void *stream);
int vaqhip_sym_eigen_host(double *A, int D, double *values, double *vectors, int *sweeps_out);
int vaqhip_train_plan(const float *eigenvalues, int D, int M, float percent_var, int min_bits, int max_bits,
                      int *sorted_out, int *order_out, float *var_out, float *cum_out, int *highest_subs_out, int *lb_out,
                      int *k_out, int *swaps_kept_out);
int vaqhip_allocate_bits(const float *c, int H, const int *lb, int max_bits, const int *k, int budget, int *bits_out,
                         double *objective_out);
int vaqhip_train_rotation(int device_id, const float *X_rowmajor, int64_t n, int D, int M, int bit_budget, int min_bits,
                          int max_bits, float percent_var, float *eigvec_out, float *eigenvalues_out, int *bits_out,
                          int *highest_subs_out);
int vaqhip_train_rotation_device(int device_id, const float *d_X, int64_t n, int D, int M, int bit_budget, int min_bits,
                                 int max_bits, float percent_var, float *d_eigvec_out, float *eigenvalues_out,
                                 int *bits_out, int *highest_subs_out, void *stream);
int vaqhip_train_rotation_u8(int device_id, const uint8_t *X_rowmajor, int64_t n, int D, int M, int bit_budget,
                             int min_bits, int max_bits, float percent_var, float *eigvec_out, float *eigenvalues_out,
                             int *bits_out, int *highest_subs_out);
int vaqhip_train_rotation_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, int bit_budget,
                                    int min_bits, int max_bits, float percent_var, float *d_eigvec_out,
                                    float *eigenvalues_out, int *bits_out, int *highest_subs_out, void *stream);
typedef struct {
  float total_ms;               /* host time of the last vaqhip_*train_rotation* on this thread, uploads excluded */
  float moment_ms, eigen_ms;    /* the second moment; the solver: sweeps, read-backs and the host finish */
  float finish_ms;              /*   of eigen_ms: the host finish (norms, Rayleigh quotients, order, signs) */
  float plan_ms;                /* the plan, the allocation and the outputs */
  int sweeps;                   /* Jacobi sweeps that rotated */
  int subspaces, dims;
  int64_t sample_rows, rows;    /* rows summed; rows given */
} vaqhip_train_timing;
int vaqhip_last_train_timing(vaqhip_train_timing *out);  /* the calling thread's last composite */

/* VAQ::refine (VAQ.cpp:849-876): exact squared L2 in the ORIGINAL space between each
 * query and its R candidate rows of the raw dataset, k best by the same k-min rule.  The sum is
 * sequential (dist += t * t), ties go to the smaller label: see the resident refiner below for the
 * reference's own summation order and heap.
 * labels_in: nq x R (negative labels are skipped); R <= 2048.  The host form gathers
 * the candidate rows from `dataset_rowmajor` (N x D, raw, unprojected) itself. */
int vaqhip_refine(int device_id, const float *queries_rowmajor, int nq, int D,
                  const float *dataset_rowmajor, int64_t N, const int32_t *labels_in, int R,
                  int k, int32_t *labels_out, float *distances_out);
int vaqhip_refine_device(int device_id, const float *d_queries, int nq, int D,
                         const float *d_dataset, const int32_t *d_labels_in, int R, int k,
                         int32_t *d_labels_out, float *d_distances_out, void *stream);

/* ---------------------------------------------------------------------------
 * Resident refiner: VAQ::refine (VAQ.cpp:849-876) with the reference's own numbers, over raw rows that stay on
 * the device -- what `demo_vaq --refine R1,R2` runs after every search (demo_vaq.cpp:336-345).
 *   distances  (XTest.row(q) - XTrain.row(l)).squaredNorm() in Eigen's summation order (8-float packets, two
 *              accumulators, predux, scalar tail; plain sequential below 8 columns): bit for bit the reference's on
 *              any float data.  vaqhip_refine* above sum sequentially, which equals this only for D < 8 or where
 *              every partial sum is exact (integer-valued data such as SIFT).
 *   rows       N x D raw, unprojected float32, row-major; row i has label id_base + i (set_rows_device copies;
 *              add_rows appends, labels continue at id_base + N).  VAQHIP_ERANGE where labels would pass int32.
 *   labels_in  nq x R in the order the search returned them, 1 <= k <= R <= 2048.  A label that is negative or
 *              outside [id_base, id_base + N) is SKIPPED and its row never read (the reference reads out of bounds),
 *              also in the _device form: the kernel checks every label itself.  Duplicates are kept, as the
 *              reference keeps them.
 *   result     nq x k; admission is the reference's heap_top > dist from a heap of FLT_MAX: an infinite or NaN
 *              distance never enters; unfilled slots -1 / FLT_MAX.
 *   option "exact_ties"  0 (default): the k smallest by (distance, label).  1: which of several candidates tying at
 *              the k-th distance survive, and the order equal distances come in, are the reference's -- its loop
 *              (heap_heapify, heap_pop + heap_push when heap_top > dist, heap_reorder; utils/Heap.hpp) is replayed
 *              over the R distances in candidate order: labels and distances equal VAQ::refine's slot for slot.
 * vaqhip_search_refine = the index's search with k = R (its own method and options, "exact_ties" included) followed
 * by the refine of that result in the order the search returned it; the candidates never leave the device.  Equals
 * vaqhip_search followed by vaqhip_refiner_refine on the same inputs.  R <= VAQHIP_MAX_K.  VAQHIP_ESTATE when the
 * refiner's N or id_base differ from the index's, VAQHIP_EINVAL when the two live on different devices or differ in D.
 * The host forms are synchronous; the _device forms take device pointers on the refiner's GPU, enqueue on `stream`
 * and never synchronise (the fused one grows its candidate buffer on first use).  Calls on one refiner are serialised
 * on the host; set_rows / add_rows wait for the device to go idle before rows are moved or replaced.
 *   byte rows  the *_u8 calls keep the rows as uint8, N x D row-major, as a bvecs file (SIFT1B / BIGANN; the reference's
 *              --file-format-ori bvecs) stores them: a quarter of the memory and of the bytes a refine fetches.  The
 *              reference widens every byte to a float when it reads the file (utils/IO.hpp, readBVecsFromExternal);
 *              here the kernels widen a byte where they load it.  (float)uint8 is exact, so every distance is the same
 *              float operations on the same operands as over the widened rows: all of the above holds bit for bit,
 *              for any float query, in every call that reads the rows (refine, the fused call, the exhaustive form).
 *              The element type belongs to the rows: set_rows* of either type replaces the rows and their type;
 *              add_rows on byte rows and add_rows_u8 on float rows are VAQHIP_ESTATE (nothing is converted), a refiner
 *              with N == 0 takes either.  Null, range and id_base checks are those of the float calls.
 *              vaqhip_refiner_elem_size: 4 (float32, also before any rows) or 1 (uint8); negative for a null handle.
 * ------------------------------------------------------------------------- */
typedef struct vaqhip_refiner vaqhip_refiner;
int vaqhip_refiner_create(vaqhip_refiner **out, int device_id, int D);
void vaqhip_refiner_destroy(vaqhip_refiner *r);
int vaqhip_refiner_set_rows(vaqhip_refiner *r, const float *X_rowmajor, int64_t N, int64_t id_base);
int vaqhip_refiner_set_rows_device(vaqhip_refiner *r, const float *d_X, int64_t N, int64_t id_base, void *stream);
int vaqhip_refiner_add_rows(vaqhip_refiner *r, const float *X_rowmajor, int64_t n_new);
int vaqhip_refiner_set_rows_u8(vaqhip_refiner *r, const uint8_t *X_rowmajor, int64_t N, int64_t id_base);
int vaqhip_refiner_set_rows_u8_device(vaqhip_refiner *r, const uint8_t *d_X, int64_t N, int64_t id_base, void *stream);
int vaqhip_refiner_add_rows_u8(vaqhip_refiner *r, const uint8_t *X_rowmajor, int64_t n_new);
int vaqhip_refiner_elem_size(vaqhip_refiner *r);
int vaqhip_refiner_set_option(vaqhip_refiner *r, const char *key, int64_t value);
int vaqhip_refiner_refine(vaqhip_refiner *r, const float *queries_rowmajor, int nq, const int32_t *labels_in, int R,
                          int k, int32_t *labels_out, float *distances_out);
int vaqhip_refiner_refine_device(vaqhip_refiner *r, const float *d_queries, int nq, const int32_t *d_labels_in, int R,
                                 int k, int32_t *d_labels_out, float *d_distances_out, void *stream);
int vaqhip_search_refine(vaqhip_index *ix, vaqhip_refiner *r, const float *queries_raw_rowmajor, int nq, int R, int k,
                         int32_t *labels_out, float *distances_out);
int vaqhip_search_refine_device(vaqhip_index *ix, vaqhip_refiner *r, const float *d_queries_raw, int nq, int R, int k,
                                int32_t *d_labels_out, float *d_distances_out, void *stream);
/* "Learning on the device" above, over the refiner's resident rows (raw rows: projected = 0) */
int vaqhip_learn_quantization_from_refiner(vaqhip_index *ix, vaqhip_refiner *r, float sample_ratio,
                                           float *offsets_out, float *scale_out);
/* vaqhip_fit_codebooks above over the refiner's resident rows, float or byte, read in place (eigvec and the outputs are
 * host arrays); VAQHIP_ESTATE on a refiner without rows */
int vaqhip_refiner_fit_codebooks(vaqhip_refiner *r, int M, const int *bits, const float *eigvec_real_rowmajor,
                                 int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out);
/* vaqhip_fit_codebooks_hier above over the refiner's resident rows, float or byte, read in place */
int vaqhip_refiner_fit_codebooks_hier(vaqhip_refiner *r, int M, const int *bits, const float *eigvec_real_rowmajor,
                                      int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out);
/* vaqhip_fit_codebooks_bin above over the refiner's resident rows, float or byte, read in place */
int vaqhip_refiner_fit_codebooks_bin(vaqhip_refiner *r, int M, const int *bits, const float *eigvec_real_rowmajor,
                                     int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out);
/* "Training from raw rows" above over the refiner's resident rows, float or byte, read in place (outputs: host arrays) */
int vaqhip_refiner_train_moment(vaqhip_refiner *r, double *cov_out, float *cov_f_out);
int vaqhip_refiner_train_rotation(vaqhip_refiner *r, int M, int bit_budget, int min_bits, int max_bits, float percent_var,
                                  float *eigvec_out, float *eigenvalues_out, int *bits_out, int *highest_subs_out);

/* Exhaustive form of the resident refiner: the true k nearest rows of every query, i.e. what vaqhip_refiner_refine
 * would return for the candidate list id_base, id_base + 1, ..., id_base + N - 1 in that order if R were allowed to be
 * N -- VAQ::refine (VAQ.cpp:849-876) with answersIn naming every row once in row order; ground truth with the
 * reference's own distances, no file needed.  Rows appended with add_rows are searched.
 *   distances   the refiner's: Eigen's summation order, bit for bit, for every D the refiner accepts (rows of up to 128
 *               columns are held in registers, one thread per row, and meet many queries; wider rows take a general
 *               path with the same answers).
 *   selection   "exact_ties" = 0: the k smallest by (distance, label) among rows with distance < FLT_MAX; unfilled
 *               slots -1 / FLT_MAX (N < k, rows whose distance is inf or NaN).  "exact_ties" = 1: the reference heap's
 *               labels and distances slot for slot (heap_heapify, then over rows 0..N-1 heap_pop + heap_push when
 *               heap_top > dist, heap_reorder): queries whose k + 1 best hold two equal distances are replayed through
 *               the heap on the device, one streamed pass over the rows each.  Both modes at every k <= VAQHIP_MAX_K.
 *   options     "exhaustive_splits": the rows are cut into S splits searched side by side and merged; 0 = automatic,
 *               1..64 forces S (any other value VAQHIP_EINVAL; a split may be empty).  The answer does not depend on it.
 *               "timing" = 1: device events around the phases of every following search, which then synchronises
 *               after each launch set; vaqhip_refiner_last_search_timing reads the last call's figures.
 *   limits      1 <= k <= VAQHIP_MAX_K (larger: VAQHIP_EUNSUPPORTED); nq == 0 succeeds and writes nothing; null
 *               pointers or k < 1 VAQHIP_EINVAL -- all checked before any device work; VAQHIP_ESTATE before rows are set.
 * The host form is synchronous; the _device form takes pointers on the refiner's GPU, enqueues on `stream` and never
 * synchronises (it grows its workspace on first use).  Serialised with the refiner's other calls. */
int vaqhip_refiner_search(vaqhip_refiner *r, const float *queries_rowmajor, int nq, int k, int32_t *labels_out,
                          float *distances_out);
int vaqhip_refiner_search_device(vaqhip_refiner *r, const float *d_queries, int nq, int k, int32_t *d_labels_out,
                                 float *d_distances_out, void *stream);
typedef struct {
  float select_ms;        /* distances + streaming selection, all splits */
  float merge_ms;         /* the splits' lists merged */
  float flag_ms;          /* "exact_ties": queries with equal distances listed, the others copied out */
  float replay_ms;        /* "exact_ties": the listed queries through the reference's heap */
  int listed_queries;     /* queries replayed */
  int splits;             /* S */
  int workgroups;         /* of one select launch: S x query groups */
  int queries_per_group;  /* queries one workgroup's rows meet */
  int register_form;      /* 1: one thread per row (D <= 128), 0: the general path */
} vaqhip_refiner_search_timing;
/* figures of the last vaqhip_refiner_search[_device] on this refiner (zero times unless "timing" was set) */
int vaqhip_refiner_last_search_timing(vaqhip_refiner *r, vaqhip_refiner_search_timing *out);

/* Multi-GPU exchange step: after an all-gather of per-shard
 * results laid out [n_lists][nq][k] (labels already global), keep per query
 * the k smallest by (distance, label).  Device pointers.  The reference's
 * precedent for shard-and-merge: BitVecEngine.cpp:1034-1132 (:1114-1126). */
int vaqhip_merge_topk_device(int device_id, const float *d_dist_lists,
                             const int32_t *d_label_lists, int n_lists, int nq, int k,
                             int32_t *d_labels_out, float *d_dist_out, void *stream);

/* Same with explicit element strides: candidate i of list l of query q is read at
 * d_dist_lists[l*list_stride + q*query_stride + i] (labels likewise), so the lists may
 * sit inside one packed all-gather buffer (labels and distances gathered by a single
 * collective: vaq_amd/sharding.py). */
int vaqhip_merge_topk_strided_device(int device_id, const float *d_dist_lists,
                                     const int32_t *d_label_lists, int n_lists,
                                     int64_t list_stride, int64_t query_stride, int nq, int k,
                                     int32_t *d_labels_out, float *d_dist_out, void *stream);

/* FAST's exchange step.  A FAST answer is not ordered by (distance, label): it is the first k of a stable sort
 * by distance of "the head -- the first n_head = min(k, N) rows of the whole database -- in the order
 * KNNFromDists' std::sort leaves them, then every other row in row order" ("FAST across
 * shards").  So a shard contributes the distances of the head rows it holds, untruncated, and the top-k of its
 * OTHER rows by (distance, row); this call sorts the gathered head as the single index does and merges:
 *   d_head_dist   uint16 distance of head row p of query q at [q * head_stride + p], p < n_head <= k
 *   lists         as for vaqhip_merge_topk_strided_device (candidate i of list l of query q at
 *                 [l * list_stride + q * query_stride + i]), each ascending by distance, lists in row order,
 *                 k slots each, empty slots label < 0; distances are integers below 65535 held as float
 *   result        k per query; head rows get label head_label_base + p; ties go to the head, then to the
 *                 earlier list, then to the earlier slot; slots past the number of entries are -1 / FLT_MAX
 * At most 16 lists, k <= VAQHIP_MAX_K (VAQHIP_EUNSUPPORTED).  The outputs are used as scratch while the call
 * runs on the device and must not overlap the inputs.  Enqueue only. */
int vaqhip_merge_fast_device(int device_id, const uint16_t *d_head_dist, int64_t head_stride, int n_head,
                             int64_t head_label_base, const float *d_dist_lists, const int32_t *d_label_lists,
                             int n_lists, int64_t list_stride, int64_t query_stride, int nq, int k,
                             int32_t *d_labels_out, float *d_dist_out, void *stream);

/* ---------------------------------------------------------------------------
 * Multi-device index (north_star: "the code database shards
 * naturally across the 8 GPUs of one node with a final RCCL all-gather of per-shard top-k").
 * One process, one host thread per GPU.  set_codes cuts the rows into contiguous shards (shard g =
 * rows [g * ceil(N/G), (g+1) * ceil(N/G)), labels stay global row numbers); every device answers
 * all queries on its shard; the exchange step is ONE ncclAllGather (RCCL over xGMI) of the packed
 * per-shard results followed by the k-min merge by (distance, label): the result equals a single
 * index over all rows bit for bit.  The reference's precedent for shard-and-merge is
 * BitVecEngine.cpp:1034-1132 (merge at :1114-1126); its own search is single-threaded on one host
 * (VAQ.cpp:776-847), so this is the form `class VAQ` takes on a multi-GPU node.
 *   device_ids   HIP ordinals, one per shard.  Naming one GPU several times gives LOGICAL shards
 *                on that GPU (RCCL refuses duplicate devices, so the gather is then done with
 *                device-to-device copies; same buffers, same merge) -- how a one-GPU box tests
 *                the sharded path.
 * Options ("exchange": 0 auto, 1 RCCL, 2 copies; "exact_batch" below; "encode_chunk_rows": "Encode across the
 * shards" below; anything else is forwarded to every shard).
 *   "exact_ties" = 1 holds ACROSS the shards: labels and distances are VAQ::search's over all rows,
 *                slot for slot.  Shards are contiguous label ranges in label order (appends extend the
 *                last one), so the reference's heap after the rows of shards 0..g is shard g's replay
 *                started from the heap shards 0..g-1 left.  Shape of the cost: every shard scans with
 *                k + 1 by the smallest-label rule, the exchange and merge give the global k + 1 list,
 *                queries without equal neighbours in it are done; the tied ones take a second pass, a
 *                chain of replays shard after shard with ONE hand-over of k * 8 bytes per tied query
 *                per shard boundary (peer copies ordered by events, in batches of the list so that
 *                distinct GPUs work on different batches at the same time; a shard that inherits an
 *                already tight heap top skips most of its rows).  Calls of more than 16384 queries are
 *                served in sets of that size.  last_merge_ms then includes the second pass.
 *                No effect -- the result is then what each shard's own option gives, merged by
 *                (distance, label), as on a single index where the option has no effect either --
 *                with TI, with FAST (whose sharded answer is the single index's slot for slot already)
 *                (a cluster's member order is one std::sort over rows of all shards: no chain reproduces it)
 *                and for k == VAQHIP_MAX_K.  One shard: that shard's own replay.
 *                On VAQHIP_SUM_SEQUENTIAL shards the answer is BitVecEngine::queryLUT's over all rows: the
 *                state handed on is its raw std heap (k + 1 pairs), the heap's length and bsfK
 *                ((k + 2) * 8 bytes), and `dataIndex >= k` counts from the shard's first global row.
 *   "exact_batch" list entries per batch of that second pass; 0 (default) = max(64, a 16th of the
 *                set's queries); never fewer than a 256th of them.  Results do not depend on it.
 * ------------------------------------------------------------------------- */
#define VAQHIP_MAX_DEVICES 16
typedef struct vaqhip_multi vaqhip_multi;
typedef struct vaqhip_multi_refiner vaqhip_multi_refiner;  /* "Multi-device refiner" below */
int vaqhip_multi_create(vaqhip_multi **out, int D, int M, const int *bits,
                        const float *const *centroids_rowmajor, const float *eigvec_real_rowmajor,
                        int n_devices, const int *device_ids, unsigned flags);
void vaqhip_multi_destroy(vaqhip_multi *mx);
/* mCodebook for the whole database (host pointer); sharded contiguously across the devices, every
 * shard uploaded, sorted and packed by its own host thread at the same time */
int vaqhip_multi_set_codes_u16(vaqhip_multi *mx, const uint16_t *codes_rowmajor, int64_t N, int64_t id_base);
/* append: the new rows continue the numbering, so they extend the LAST shard -- repeated appends pile
 * rows (memory and scan time) on one device; vaqhip_multi_get_info's shard_rows shows the skew, and
 * vaqhip_multi_set_codes_u16 with the whole matrix re-balances */
int vaqhip_multi_add_codes_u16(vaqhip_multi *mx, const uint16_t *codes_rowmajor, int64_t n_new);
/* VAQ::search on every shard + exchange + merge; host pointers, synchronous */
int vaqhip_multi_search(vaqhip_multi *mx, const float *queries_rowmajor, int nq, int k, int projected,
                        int32_t *labels, float *distances);
/* The same with device pointers, enqueue only: d_queries (nq x D) and the outputs live on device_ids[0];
 * the call returns once every shard's work is enqueued -- each shard copies the queries over the fabric
 * (hipMemcpyPeerAsync, no host staging), `stream` (a stream of device_ids[0]) is made to wait for the
 * merged result, the host is not.  Like the single-index "_device" entry points it never synchronises. */
int vaqhip_multi_search_device(vaqhip_multi *mx, const float *d_queries, int nq, int k, int projected,
                               int32_t *d_labels, float *d_distances, void *stream);
/* forwarded to every shard (each shard regroups its own rows under the same TI centres) */
int vaqhip_multi_set_ti_clusters(vaqhip_multi *mx, const float *clusters_rowmajor, int T, int seg_num);
int vaqhip_multi_set_method(vaqhip_multi *mx, unsigned methods, float visit);
/* vaqhip_index_cluster_ti_kmeans over ALL rows of the multi index, in global row order: the same sample
 * (randomPermutation(N)[0 .. 256 * T) when N > 256 * T, else every row; id_base plays no part), the same seeds, and
 * therefore the same centres, iteration count and NaN-centre count as a single index over the same rows, bit for
 * bit, for any number of shards -- shards grown by add_codes and empty shards included.  Every shard reads its
 * part of the sample from its packed rows on its own device; the assign step of every iteration is cut over the
 * shards' devices (contiguous slices of ceil(rows / G) sample rows; keys, values and centres travel by peer copy),
 * the sums and the update run on the first device, which alone decides the summation order.  Then what
 * vaqhip_multi_set_ti_clusters does with the centres.  Refusals are the single index's (VAQHIP_EINVAL: T < 1,
 * max_iter < 1, seg_num outside 1..M, T > N, a sequential-sum index; VAQHIP_ESTATE: no codes yet;
 * VAQHIP_EUNSUPPORTED: T > 4096, centres of more than 1024 dims); a call that fails or is refused leaves every
 * shard's grouping and method as they were.  The out-pointers may be NULL.  Synchronises. */
int vaqhip_multi_cluster_ti_kmeans(vaqhip_multi *mx, int T, int seg_num, int max_iter, float *clusters_out,
                                   int *iters_out, int *nan_rows_out);
/* figures of the last vaqhip_multi_cluster_ti_kmeans: total_ms covers the gather on the shards, the fit and the
 * copies; with option "timing" = 1 assign_ms is the wall time of the assign step over all shards, copies included */
int vaqhip_multi_last_kmeans_timing(vaqhip_multi *mx, vaqhip_kmeans_timing *out);
int vaqhip_multi_set_option(vaqhip_multi *mx, const char *key, int64_t value);
/* Method FAST on a multi index: labels and distances are the single index's over all rows, slot for slot.
 * Every shard sends the distances of the head rows it holds (the first min(k, N) rows of the database, which
 * span several shards when N / n_devices < k) and the top-k of its other rows by (distance, row) in the ONE
 * all-gather; shard 0 sorts the head and merges (vaqhip_merge_fast_device).  The rows being sharded, the
 * [queries][rows] distance matrix of a chunk is a shard's, not the database's.  One shard: the single-index
 * search itself.  set_lut_quantization gives every shard the same mOffsets / mScale; learn_quantization is
 * vaqhip_learn_quantization once, on shard 0 (the rows play no part in it), replicated to the others -- the
 * same values as on a single index, bit for bit.  Both leave the caller's current device as it was.
 * Call order: the quantisation first.  vaqhip_multi_set_method with FAST alone stays VAQHIP_EUNSUPPORTED until one
 * of these two calls has given every shard the same quantisation (a multi index without one cannot run FAST on
 * any shard; it is refused where the method is chosen, not at the first search). */
int vaqhip_multi_set_lut_quantization(vaqhip_multi *mx, const float *offsets, const float *scale);
int vaqhip_multi_learn_quantization(vaqhip_multi *mx, const float *X_rowmajor, int64_t n, int projected,
                                    float sample_ratio, float *offsets_out, float *scale_out);
/* The device forms on a multi index.  _u8: vaqhip_learn_quantization_u8 on shard 0, replicated.  _from_refiner: the
 * sample is cut by the shard that holds each row; every shard gathers its rows on its own device (a byte widened)
 * and they are copied to the first device at their sample positions; the first device learns and every shard is
 * given the result.  The index and the refiner must name the same device list and D (VAQHIP_EINVAL); a refiner
 * without rows is VAQHIP_ESTATE. */
int vaqhip_multi_learn_quantization_u8(vaqhip_multi *mx, const uint8_t *X_rowmajor, int64_t n, int projected,
                                       float sample_ratio, float *offsets_out, float *scale_out);
int vaqhip_multi_learn_quantization_from_refiner(vaqhip_multi *mx, vaqhip_multi_refiner *r, float sample_ratio,
                                                 float *offsets_out, float *scale_out);
/* Encode across the shards: VAQ::encode (vaqhip_encode's rule: strict `<`, first minimum, the checked projection on
 * VAQHIP_SUM_SEQUENTIAL shards) with every shard encoding the rows it will hold, on its own device.
 *   contract    vaqhip_multi_encode_set_codes leaves the index in exactly the state of vaqhip_encode on one index with
 *               the same codebooks over all N rows followed by vaqhip_multi_set_codes_u16(mx, codes, N, id_base): the
 *               same cut, shard_rows, labels and packed order, hence the same answer bit for bit from every later call.
 *               codes_out (N x M, may be NULL) is vaqhip_encode's matrix.  vaqhip_multi_encode_add_codes is the same
 *               against vaqhip_encode + vaqhip_multi_add_codes_u16: the rows extend the last shard and are encoded on
 *               its device.  A row's code depends on that row and the codebooks only, and every shard holds the
 *               codebooks and the rotation: nothing is exchanged.
 *   host form   every shard's host thread uploads ITS slice of X in chunks, encodes them into a device buffer of
 *               rows_g x M uint16 and hands that buffer to its index on the device.  No code reaches the host unless
 *               codes_out asks for it, no row reaches a device other than the one that will hold its code.  Per shard:
 *               rows_g * M * 2 bytes of codes and one chunk of D * 4 bytes per row (twice with projected = 0).
 *   refiner     vaqhip_multi_encode_from_refiner reads the RAW rows resident in a multi refiner in place (projected = 0):
 *               N, id_base and the cut are the refiner's, shard g of the index receives the rows of shard g of the
 *               refiner -- a last shard grown by add_rows and empty shards included -- so vaqhip_multi_search_refine
 *               sees equal N and id_base afterwards.  Nothing is uploaded.
 *   refusals    before any device is touched: VAQHIP_EINVAL for a null index, matrix or refiner, negative sizes, D or
 *               device lists that differ between index and refiner; labels that would pass int32 and N == 0 as
 *               vaqhip_multi_set_codes_u16 treats them; VAQHIP_ESTATE for a refiner without rows and for _add_codes on
 *               an index that never received codes.
 *   failure     phase one, every shard encodes into scratch: a failure leaves every shard as it was.  Phase two, the
 *               shards take their codes: a failure there is vaqhip_multi_set_codes_u16's.
 *   option      "encode_chunk_rows" (vaqhip_multi_set_option): rows per upload / project chunk, 0 = 1 << 20, negative
 *               VAQHIP_EINVAL.  Results do not depend on it.
 *   byte rows   the *_u8 forms take uint8 rows (vaqhip_encode_u8's contract): every shard uploads ITS slice as bytes,
 *               chunks of D bytes per row, and encodes it with vaqhip_encode_u8_device; the index ends in the state the
 *               float form leaves from the widened matrix.  The refiner form over a byte refiner reads the bytes in
 *               place the same way: no widened chunk is written where a projection runs.
 * Synchronous; the caller's current device is left as it was; serialised with the other calls on the index. */
int vaqhip_multi_encode_set_codes(vaqhip_multi *mx, const float *X_rowmajor, int64_t N, int projected,
                                  int64_t id_base, uint16_t *codes_out /* N x M, may be NULL */);
int vaqhip_multi_encode_add_codes(vaqhip_multi *mx, const float *X_rowmajor, int64_t n_new, int projected,
                                  uint16_t *codes_out /* n_new x M, may be NULL */);
int vaqhip_multi_encode_from_refiner(vaqhip_multi *mx, vaqhip_multi_refiner *r,
                                     uint16_t *codes_out /* N x M, may be NULL */);
int vaqhip_multi_encode_set_codes_u8(vaqhip_multi *mx, const uint8_t *X_rowmajor, int64_t N, int projected,
                                     int64_t id_base, uint16_t *codes_out /* N x M, may be NULL */);
int vaqhip_multi_encode_add_codes_u8(vaqhip_multi *mx, const uint8_t *X_rowmajor, int64_t n_new, int projected,
                                     uint16_t *codes_out /* n_new x M, may be NULL */);
typedef struct {
  float total_ms;      /* wall time of the call                                                   */
  float encode_ms;     /* the slowest shard, device events: upload (host form), project, encode   */
  float set_codes_ms;  /* the slowest shard, device events: sort and pack (append: merge)         */
  int64_t rows;        /* rows encoded                                                            */
  int n_devices;
} vaqhip_multi_encode_timing;
/* figures of the last of the three calls above, or of their _lut forms below, that ran (zeros before the first) */
int vaqhip_multi_last_encode_timing(vaqhip_multi *mx, vaqhip_multi_encode_timing *out);
/* Build a queryLUT index across the shards (BitVecEngine::binaryEncodingLUT on a VAQHIP_SUM_SEQUENTIAL multi index).
 * Call order: the fit (below) -> vaqhip_multi_create with its centres -> vaqhip_multi_set_lut_quantiles -> one of the
 * vaqhip_multi_encode_lut_* calls.
 *   Q           vaqhip_multi_set_lut_quantiles is vaqhip_index_set_lut_quantiles on every shard.  It validates once on
 *               the host with that call's checks (VAQHIP_EINVAL: shards that are not sequential-sum, D != M, bits > 8,
 *               a NaN in Q) and then gives Q to shard after shard.  If a shard fails, the shards that already took Q
 *               keep it and the error is returned: Q is idempotent state, a repeated call heals it.
 *   encoders    the contract of "Encode across the shards" above with vaqhip_encode_lut (encodeToLUTCode: the boundary
 *               scan, `<=` ties to the middle, then left; the unchecked projection) in the place of vaqhip_encode: the
 *               index ends in exactly the state of vaqhip_encode_lut on one index over all rows followed by
 *               vaqhip_multi_set_codes_u16 / _add_codes_u16, codes_out is that call's matrix; the same two phases, failure
 *               semantics, option "encode_chunk_rows" and vaqhip_multi_last_encode_timing.  VAQHIP_ESTATE before
 *               vaqhip_multi_set_lut_quantiles, and from _add_codes before any codes. */
int vaqhip_multi_set_lut_quantiles(vaqhip_multi *mx, const float *quantiles /* [D][257] */);
int vaqhip_multi_encode_lut_set_codes(vaqhip_multi *mx, const float *X_rowmajor, int64_t N, int projected,
                                      int64_t id_base, uint16_t *codes_out /* N x M, may be NULL */);
int vaqhip_multi_encode_lut_add_codes(vaqhip_multi *mx, const float *X_rowmajor, int64_t n_new, int projected,
                                      uint16_t *codes_out /* n_new x M, may be NULL */);
int vaqhip_multi_encode_lut_from_refiner(vaqhip_multi *mx, vaqhip_multi_refiner *r,
                                         uint16_t *codes_out /* N x M, may be NULL */);
int vaqhip_multi_encode_lut_set_codes_u8(vaqhip_multi *mx, const uint8_t *X_rowmajor, int64_t N, int projected,
                                         int64_t id_base, uint16_t *codes_out /* N x M, may be NULL */);
int vaqhip_multi_encode_lut_add_codes_u8(vaqhip_multi *mx, const uint8_t *X_rowmajor, int64_t n_new, int projected,
                                         uint16_t *codes_out /* n_new x M, may be NULL */);
/* The sharded quantile fit: vaqhip_lut_fit_quantiles's result, bit for bit, for ANY device list, with no device ever
 * holding the n x D rows (nor a projected copy of its own slice).
 *   scheme      dimension d is owned by device d % G.  In rounds of G consecutive dimensions every shard turns its
 *               resident rows into the round's column slices of sortable keys (one kernel, the projection fused: one
 *               fmaf chain per value, vaqhip_project's), sends slice j to owner j at the word offset of its first row
 *               (peer copies; device-to-device where two shards name one GPU), and every owner runs the single fit's
 *               column pipeline on its assembled n keys: radix sort, quantiles, ordered bucket sums.  A sorted column
 *               does not depend on the order its values arrived in and everything behind the sort runs unchanged on
 *               one device, so no chain and no tie question arises.  The last round may be partial; D < G leaves
 *               owners idle.  The rows are re-read once per round, ceil(D / G) times in all.
 *   host form   X is cut over the devices as vaqhip_multi_set_codes_u16 cuts rows; every shard uploads its slice once.
 *   refiner     the RAW rows a multi refiner holds are read in place; n, D and the cut are the refiner's (a last shard
 *               grown by add_rows and empty shards included); nothing is uploaded but eigvec.
 *   workspace   per owner two key buffers of n words and rocprim's scratch; per shard G x n_g words and, in the host
 *               form, its slice of n_g x D floats.
 *   refusals    decided before any device is touched, with the single fit's codes: null pointers, n < 1, n >= 2^31,
 *               D < 1 (VAQHIP_EINVAL), D > 4096 (VAQHIP_EUNSUPPORTED), bits outside 1..8; n_devices outside
 *               1..VAQHIP_MAX_DEVICES, a null refiner (VAQHIP_EINVAL), a refiner without rows (VAQHIP_ESTATE).  A NaN or
 *               infinite (projected) value on ANY shard: VAQHIP_EINVAL, both outputs untouched.
 *   byte rows   vaqhip_multi_lut_fit_quantiles_u8 uploads every shard's slice as n_g x D bytes, and a refiner that holds
 *               uint8 rows (vaqhip_multi_refiner_set_rows_u8) is read in place like one that holds floats: the column
 *               kernel widens a byte where it loads it, every round, and no n_g x D float copy exists at any time.
 *               Per shard the call owns what it owns over float rows: G x n_g key words, eigvec and the flag.  The
 *               result is vaqhip_lut_fit_quantiles's on the widened rows, bit for bit.
 * Synchronous; a failing shard ends the call; the caller's current device is left as it was. */
int vaqhip_multi_lut_fit_quantiles(int n_devices, const int *device_ids, const float *X_rowmajor, int64_t n, int D,
                                   const int *bits, const float *eigvec_real_rowmajor /* D x D or NULL */,
                                   float *centroids_out /* [D][256] */, float *quantiles_out /* [D][257] */);
int vaqhip_multi_lut_fit_quantiles_u8(int n_devices, const int *device_ids, const uint8_t *X_rowmajor, int64_t n, int D,
                                      const int *bits, const float *eigvec_real_rowmajor /* D x D or NULL */,
                                      float *centroids_out /* [D][256] */, float *quantiles_out /* [D][257] */);
int vaqhip_multi_refiner_lut_fit_quantiles(vaqhip_multi_refiner *r, const int *bits,
                                           const float *eigvec_real_rowmajor /* D x D or NULL */,
                                           float *centroids_out /* [D][256] */, float *quantiles_out /* [D][257] */);
typedef struct {
  float total_ms;     /* wall time of the call                                                       */
  float columns_ms;   /* per phase: the slowest device, device events, summed over the rounds --     */
  float copy_ms;      /*   rows -> column keys; slices to their owners;                              */
  float sort_ms;      /*   radix sort; quantiles and bucket ends; ordered bucket sums                */
  float quantile_ms;
  float means_ms;
  int64_t rows;
  int dims;
  int n_devices;
} vaqhip_multi_lut_fit_timing;
int vaqhip_multi_last_lut_fit_timing(vaqhip_multi_lut_fit_timing *out);  /* the calling thread's last sharded fit */
/* The sharded codebook fit: vaqhip_fit_codebooks's result, bit for bit -- centres (a NaN by position), iterations and
 * NaN counts --, for ANY device list, with the training rows cut over the devices and no device ever holding the
 * n x D rows, nor a projected copy of them.  Outputs and semantics are vaqhip_fit_codebooks's: sampling decided per
 * subspace, all subspaces drawing from one permutation head, its seeds, Lloyd loop and NaN centres.
 *   scheme      subspace s is owned by device s % G (M < G leaves owners idle; the result does not depend on the rule:
 *               no value of a subspace is computed from another's).  Every shard writes, per owner, the packed block
 *               [rows it contributes][D_w] of that owner's columns, D_w = subspaces owned x L (one kernel: a byte is
 *               widened where it is loaded and, with eigvec, every value is one fmaf chain over the row's D inputs in
 *               vaqhip_project's order; only the columns an owner needs are computed for it, so across owners the
 *               contributed rows are projected once).  The rows contributed are the shard's rows of the sample
 *               permutation_head(n, sample), or ALL of its rows for an owner of a subspace that does not sample.
 *               Copies only carry the blocks to the owners (peer copies; device-to-device where two shards name one
 *               GPU): a block of all rows lands at row lo_g of the owner's n x D_w matrix, a sample block in a staging
 *               area from where a placement kernel writes each row to its position in the owner's sample x D_w matrix.
 *               Every owner then runs the single fit's phases unchanged over its two matrices with D = D_w and no
 *               eigvec: seeds, assign, one stable radix sort, run bounds, ordered sums, update.
 *   G == 1      is the single fit itself (vaqhip_fit_codebooks / vaqhip_refiner_fit_codebooks): no exchange.
 *   host form   X is cut over the devices as vaqhip_multi_set_codes_u16 cuts rows.  Where every subspace samples, each
 *               shard uploads only the sample rows that fall in its slice, picked on the host; otherwise its slice,
 *               once.  Float or byte rows go up as they are.
 *   refiner     the RAW rows a multi refiner holds, float or byte, are read in place; n, D and the cut are the
 *               refiner's (a last shard grown by add_rows and empty shards included); nothing is uploaded but eigvec
 *               and the row lists.  The refiner's lock is held; its rows are only read.
 *   memory      per owner sample x D_w floats (twice while the staging area lives); per owner of a subspace that does
 *               not sample n x D_w floats more (there n <= 256 k_max); per owner 16 bytes per (owned subspace, row it
 *               works on); per shard its packed blocks (rows contributed x D floats at most per kind) and, in the host
 *               form, its uploaded rows.
 *   refusals    decided before any device is touched, the three outputs untouched: vaqhip_fit_codebooks's, with its
 *               codes; n_devices outside 1..VAQHIP_MAX_DEVICES and a null device list or refiner (VAQHIP_EINVAL); a
 *               refiner without rows (VAQHIP_ESTATE); D % M != 0 against the refiner's D (VAQHIP_EINVAL).  Known only
 *               after the run: VAQHIP_EINVAL when a row has no centre on ANY owner, the outputs untouched as on every
 *               failure.
 * iters_out and nan_rows_out may be NULL.  Synchronous; a failing shard ends the call; the caller's current device is
 * left as it was; errors are read through vaqhip_multi_last_error(). */
int vaqhip_multi_fit_codebooks(int n_devices, const int *device_ids, const float *X_rowmajor, int64_t n, int D, int M,
                               const int *bits, const float *eigvec_real_rowmajor /* D x D or NULL */, int max_iter,
                               float *centroids_out, int *iters_out, int *nan_rows_out);
int vaqhip_multi_fit_codebooks_u8(int n_devices, const int *device_ids, const uint8_t *X_rowmajor, int64_t n, int D, int M,
                                  const int *bits, const float *eigvec_real_rowmajor /* D x D or NULL */, int max_iter,
                                  float *centroids_out, int *iters_out, int *nan_rows_out);
int vaqhip_multi_refiner_fit_codebooks(vaqhip_multi_refiner *r, int M, const int *bits,
                                       const float *eigvec_real_rowmajor /* D x D or NULL */, int max_iter,
                                       float *centroids_out, int *iters_out, int *nan_rows_out);
typedef struct {
  float total_ms;       /* wall time of the call, its planning and the release of its workers, streams and
                           buffers included (G == 1: the single fit's total_ms)                               */
  float columns_ms;     /* per phase the slowest device, device events: rows -> the owners' packed blocks;     */
  float copy_ms;        /*   the blocks to their owners;                                                       */
  float place_ms;       /*   staging -> sample matrix (or the owner's own gather from its full matrix)         */
  float assign_ms, accumulate_ms, update_ms;  /* the slowest owner's, as vaqhip_fit_codebooks_timing has them: only
                                                 with vaqhip_fit_codebooks_set_timing(1) on the calling thread, else 0 */
  int iterations;       /* the largest iteration count of a subspace */
  int subspaces, dims;
  int64_t rows;
  int64_t sample_rows;  /* the most rows a subspace worked on */
  int n_devices;
  int owner_subspaces[VAQHIP_MAX_DEVICES];  /* subspaces fitted per device of the list; they sum to M */
} vaqhip_multi_fit_codebooks_timing;
int vaqhip_multi_last_fit_codebooks_timing(vaqhip_multi_fit_codebooks_timing *out);  /* calling thread's last sharded fit */
typedef struct {
  int n_devices;
  int exchange;              /* what the last search used: 0 none (one shard), 1 RCCL all-gather, 2 copies */
  int64_t N, id_base;
  int device_ids[VAQHIP_MAX_DEVICES];
  int64_t shard_rows[VAQHIP_MAX_DEVICES];
  float last_search_ms;      /* device time on shard 0: upload + project + LUT + scan (+ merge of its slices) */
  float last_exchange_ms;    /*   the all-gather (or the copies), incl. waiting for the slowest shard       */
  float last_merge_ms;       /*   the G-way merge kernel                                                     */
} vaqhip_multi_info;
int vaqhip_multi_get_info(const vaqhip_multi *mx, vaqhip_multi_info *out);
/* shard g's single-device index (options, timing, info); owned by the multi index */
vaqhip_index *vaqhip_multi_shard(vaqhip_multi *mx, int g);
const char *vaqhip_multi_last_error(void);

/* ---------------------------------------------------------------------------
 * Multi-device refiner: the resident refiner above with the raw rows cut over several GPUs -- at 1B x 128 floats
 * the rows (512 GB) fit no single device, the 8 GPUs of a node hold them together; kept as the bytes a bvecs file
 * holds (the *_u8 calls below) they are 128 GB, within the 288 GB of one MI355X.  The answer is the single
 * refiner's slot for slot, with "exact_ties" on or off and for any number of shards: a candidate's distance depends
 * on the query and its own row only, the selection on the R (distance, label) pairs in candidate order only.  So
 * every shard computes the distances of the candidates it holds (the same reduction, Eigen's summation order), and
 * ONE selection runs on device_ids[0] over the R gathered distances in the original candidate order.  No chain of
 * replays is needed, unlike the search's "exact_ties".
 *   cut         the multi index's: shard g holds rows [g * ceil(N/G), (g+1) * ceil(N/G)), row i has label
 *               id_base + i; add_rows extends the LAST shard (set_rows with the whole matrix re-balances).  Every
 *               shard's rows are uploaded by its own host thread.
 *   device_ids  as for vaqhip_multi_create; a device named several times gives logical shards on that GPU.
 *   a refine    per set of queries: (1) queries (nq * D * 4 bytes) and candidate labels (nq * R * 4) go from
 *               device_ids[0] to every other shard that holds rows (hipMemcpyPeerAsync behind an event of the caller's
 *               stream; the first shard reads them in place); (2) every shard runs the distance kernel on its own
 *               stream; (3) their [nq][R] float planes (nq * R * 4 bytes per shard) are copied to device_ids[0];
 *               (4) the select kernel runs there and writes the caller's buffers.  Copies only, no RCCL.  Calls of
 *               more than VAQHIP_MULTI_REFINER_SET queries are served in sets of that size (the gathered planes take
 *               G * set * R * 4 bytes); results do not depend on it.  One shard: the single refiner's kernel itself, on
 *               the caller's stream.
 *   limits      the single refiner's: 1 <= k <= R <= 2048 (VAQHIP_EUNSUPPORTED), sizes that are not positive
 *               VAQHIP_EINVAL, labels that would pass int32 VAQHIP_ERANGE, D beyond the workgroup's LDS
 *               VAQHIP_EUNSUPPORTED; labels outside [id_base, id_base + N) are skipped, never read.
 *   options     "exact_ties" as above; "timing" = 1: device events around the four phases of every following call;
 *               "exhaustive_splits" (0 = automatic, 1..64 per shard, any other value VAQHIP_EINVAL): the search below.
 * vaqhip_multi_search_refine = vaqhip_multi_search_device with k = R (the multi index's own method and options as they
 * are, "exact_ties" and its stated exceptions included) into a buffer on device_ids[0], followed by the refine of that
 * buffer in the order the search returned it; the candidates never reach the host.  R <= VAQHIP_MAX_K.  VAQHIP_ESTATE
 * when N or id_base differ between the index and the refiner, VAQHIP_EINVAL when D or the device lists differ.
 * The host forms are synchronous; the _device forms take pointers on device_ids[0], enqueue only and never
 * synchronise once their buffers have their size (`stream`, a stream of device_ids[0], is made to wait for the
 * result).  Errors: vaqhip_multi_last_error().  Calls on one refiner are serialised on the host.
 *   byte rows   vaqhip_multi_refiner_set_rows_u8 / _add_rows_u8 / _elem_size: the single refiner's byte rows with its
 *               rules (one element type for all shards; VAQHIP_ESTATE for an append of the other type), cut as set_rows
 *               cuts, add_rows_u8 extending the last shard.  Refine, the fused call, the exhaustive form and
 *               vaqhip_multi_encode[_lut]_from_refiner (chunks of "encode_chunk_rows" rows, a byte widened where the
 *               projection loads it, codes equal to those from the widened host matrix) and
 *               vaqhip_multi_refiner_lut_fit_quantiles read them in place.
 * ------------------------------------------------------------------------- */
#define VAQHIP_MULTI_REFINER_SET 16384
int vaqhip_multi_refiner_create(vaqhip_multi_refiner **out, int D, int n_devices, const int *device_ids);
void vaqhip_multi_refiner_destroy(vaqhip_multi_refiner *r);
int vaqhip_multi_refiner_set_rows(vaqhip_multi_refiner *r, const float *X_rowmajor, int64_t N, int64_t id_base);
int vaqhip_multi_refiner_add_rows(vaqhip_multi_refiner *r, const float *X_rowmajor, int64_t n_new);
int vaqhip_multi_refiner_set_rows_u8(vaqhip_multi_refiner *r, const uint8_t *X_rowmajor, int64_t N, int64_t id_base);
int vaqhip_multi_refiner_add_rows_u8(vaqhip_multi_refiner *r, const uint8_t *X_rowmajor, int64_t n_new);
int vaqhip_multi_refiner_elem_size(vaqhip_multi_refiner *r);
int vaqhip_multi_refiner_set_option(vaqhip_multi_refiner *r, const char *key, int64_t value);
int vaqhip_multi_refiner_refine(vaqhip_multi_refiner *r, const float *queries_rowmajor, int nq, const int32_t *labels_in,
                                int R, int k, int32_t *labels_out, float *distances_out);
int vaqhip_multi_refiner_refine_device(vaqhip_multi_refiner *r, const float *d_queries, int nq,
                                       const int32_t *d_labels_in, int R, int k, int32_t *d_labels_out,
                                       float *d_distances_out, void *stream);
int vaqhip_multi_search_refine(vaqhip_multi *mx, vaqhip_multi_refiner *r, const float *queries_raw_rowmajor, int nq,
                               int R, int k, int32_t *labels_out, float *distances_out);
int vaqhip_multi_search_refine_device(vaqhip_multi *mx, vaqhip_multi_refiner *r, const float *d_queries_raw, int nq,
                                      int R, int k, int32_t *d_labels_out, float *d_distances_out, void *stream);
typedef struct {
  int n_devices, D;
  int64_t N, id_base;
  int device_ids[VAQHIP_MAX_DEVICES];
  int64_t shard_rows[VAQHIP_MAX_DEVICES];  /* rows resident per shard */
  int exact_ties;
  int set_queries;           /* VAQHIP_MULTI_REFINER_SET */
  /* the last refine made under "timing" = 1, summed over its sets (get_info waits for it); 0 without the option */
  int last_sets;
  float last_broadcast_ms;   /* queries and labels to the shards: the slowest shard                         */
  float last_distances_ms;   /* the distance kernel: the slowest shard (one shard: the whole refine kernel) */
  float last_gather_ms;      /* the planes to device_ids[0]                                                 */
  float last_select_ms;      /* the select kernel                                                           */
} vaqhip_multi_refiner_info;
int vaqhip_multi_refiner_get_info(vaqhip_multi_refiner *r, vaqhip_multi_refiner_info *out);

/* Exhaustive form across the shards: what vaqhip_refiner_search[_device] returns for the same rows, queries, k and
 * options -- labels and distance bit patterns slot for slot -- for any number of shards, logical and empty ones and
 * rows that arrived by add_rows included.  Per set of queries:
 *   select      every shard that holds rows runs the single form's select over its own rows (labels from the shard's
 *               first label, "exhaustive_splits" splits per shard, merged on the shard) into a [nq][k1] list, k1 = k,
 *               or k + 1 under "exact_ties"; the queries reach shards 1.. by peer copy behind the caller's stream's event.
 *   gather      the lists are copied next to the first device's (nq * k1 * 8 bytes per shard) and merged there by
 *               (distance, label).  Labels are global and distinct, so the k smallest keys of the union are among the
 *               shards' k smallest: without "exact_ties" this is the answer.
 *   exact_ties  the flag step runs on the MERGED k + 1 list (a run of equal distances may span a cut).  The listed
 *               queries are replayed as a chain: shard g walks its rows in row order through the reference's heap,
 *               starting from the raw heap arrays shard g - 1 left (k * 8 bytes per query of the set and hop, by peer
 *               copy behind events); only the last shard that holds rows applies heap_reorder.  The heap's statements
 *               meet rows 0..N-1 in order with nothing in between: the reference's answer by construction.
 * Calls are cut into equal sets of queries such that the gathered lists stay within 256 MB on the first device and
 * every shard's candidate lists within the single form's 256 MB (never more than VAQHIP_MULTI_REFINER_SET queries);
 * the answer does not depend on the set size.  Copies only, no RCCL.  One shard: the single form's launches on the
 * caller's stream.  Limits and refusals are the single form's, all checked before any device work: 1 <= k <=
 * VAQHIP_MAX_K (VAQHIP_EUNSUPPORTED), nq == 0 succeeds, null pointers or k < 1 VAQHIP_EINVAL, VAQHIP_ESTATE before
 * rows are set.  The host form is synchronous; the _device form takes pointers on device_ids[0], enqueues only and
 * never synchronises once its buffers have their size.  "timing" = 1 synchronises after every set. */
int vaqhip_multi_refiner_search(vaqhip_multi_refiner *r, const float *queries_rowmajor, int nq, int k,
                                int32_t *labels_out, float *distances_out);
int vaqhip_multi_refiner_search_device(vaqhip_multi_refiner *r, const float *d_queries, int nq, int k,
                                       int32_t *d_labels_out, float *d_distances_out, void *stream);
typedef struct {
  /* the fields of vaqhip_refiner_search_timing: times of the SLOWEST shard, geometry of the first shard with rows */
  float select_ms;        /* distances + streaming selection on a shard */
  float merge_ms;         /* a shard's splits merged */
  float flag_ms;          /* "exact_ties": the flag step on the merged lists (first device) */
  float replay_ms;        /* "exact_ties": one shard's link of the chain (one shard: the whole replay) */
  int listed_queries;
  int splits;
  int workgroups;
  int queries_per_group;
  int register_form;
  /* across the shards, summed over the sets (0 with one shard) */
  float gather_ms;        /* the shards' lists to the first device, incl. waiting for the slowest shard's copy */
  float cross_merge_ms;   /* the merge of the gathered lists */
  float chain_ms;         /* "exact_ties": from the flag step's end to the last slot placed on the first device */
  int chain_shards;       /* shards that hold rows: links of the chain, lists of the cross-shard merge */
  int sets;               /* sets of queries the call was cut into */
} vaqhip_multi_refiner_search_timing;
/* figures of the last vaqhip_multi_refiner_search[_device] (zero times unless "timing" was set) */
int vaqhip_multi_refiner_last_search_timing(vaqhip_multi_refiner *r, vaqhip_multi_refiner_search_timing *out);

/* ----- introspection / tuning -------------------------------------------- */
typedef struct {
  int D, M, L;
  int max_bits;        /* mMaxBitsPerSubs                                   */
  int total_bits;      /* sum of bits                                       */
  int code_bytes;      /* packed bytes per row on the device                */
  int algo_code_bytes; /* ceil(total_bits / 8): the roofline's byte figure  */
  int lut_floats;      /* sum of 1<<bits[s]: packed LUT entries per query   */
  int64_t N;
  int64_t id_base;
  int device_id;
  int layout;          /* 0 = one byte per subspace (all bits == 8), 1 = bit-packed */
  int ti_clusters;     /* mTIClusterNum, 0 = rows in the exhaustive (bucketed) order */
  int ti_segments;     /* mTISegmentNum                                     */
  unsigned methods;    /* VAQHIP_METHOD_* bits in force                     */
  float visit;         /* mVisit                                            */
} vaqhip_info;
int vaqhip_index_info(const vaqhip_index *ix, vaqhip_info *out);

/* Options (all optional; defaults chosen per launch):
 *   "queries_per_pass"  Qb in {0 = auto, 1, 2, 4}: queries served by one
 *                       streaming pass of a workgroup over its code slice
 *   "slices"            0 = auto, else number of row slices per query batch
 *   "timing"            1: record hipEvents (on the search's own stream) around
 *                       each kernel of every following search, up to 256
 *                       searches between two vaqhip_last_timing reads
 *   "hot_buckets"       0..32 (default 16): buckets (rows sharing their first code) each
 *                       workgroup scans best-first, closest first term first, before
 *                       the rest of its slice; 0 = natural order only
 *   "waves_per_workgroup" 0 = auto (most wavefronts per CU), else 4, 8 or 16
 *   "ordered_slices"    0 (default): slices in row order.  1: when a query's rows are
 *                       split over 2..4096 workgroups, dispatch the slices
 *                       best-first per query batch instead of running the sampling
 *                       pre-pass (experimental; measured slower)
 *   "seed_thresholds"   1 (default): when a query's rows are split over several
 *                       workgroups, a pre-pass over 1/64 of the rows seeds their
 *                       admission thresholds; 0: every workgroup warms up alone
 *   "early_abandon"     how a row is dropped once a partial sum exceeds the query's
 *                       current k-th best (the GPU forms of VAQ::searchEarlyAbandon,
 *                       VAQ.cpp:1694-1727); results are identical for every value:
 *                       0 never (VAQ::searchHeap as written), 1 survivors are
 *                       compacted through an LDS queue, 2 survivors finish in
 *                       place, 3 (default) 1 or 2 chosen per search            */
/*   "group_queries"     1 (default): on a streamed database (> 256 MB of codes) with several
 *                       multi-query passes, the queries are ordered by their nearest first and
 *                       second codes before they are cut into passes -- a pass can only skip a
 *                       bucket all of its queries can skip, and similar queries skip the same ones;
 *                       2: always; 0: never.  Results are written to the queries' own slots.
 *   "best_first"        1 (default): a one-query workgroup whose row slice spans many buckets (the
 *                       cache-resident databases) visits ALL of them in ascending order of their
 *                       bound, work units handed to its waves by ticket, and stops at the first
 *                       bucket out of reach ("best-first form"); 0: the
 *                       16-hot-buckets-then-natural-order form.  Results are identical.
 *   "cost_order"        1 (default): with one best-first workgroup per query and at least 1024
 *                       queries in the call, the queries are ranked by a cost key (how flat the
 *                       first lookup table is near its minimum: sum of its 16 smallest bucket
 *                       minima - 16 x the smallest) and the expensive ones are
 *                       dispatched first -- a query's cost spans 6x and a launch otherwise ends
 *                       with its few most expensive workgroups; 0: block b serves query b.
 *                       Results are written to the queries' own rows and are identical.
 *   "defer_units"       0 (default) = off; n > 0: with one best-first workgroup per query, a
 *                       query's first round takes at most n work units (64 wave steps each); the
 *                       buckets still in reach after it are scanned by a second launch, two
 *                       workgroups per query, and merged in (-1: n = 96 from 4096 queries per call
 *                       on).  Results are identical.  Measured slower than scanning on in place
 *                       (DESIGN.md section 4): the second launch has a tail of its own.
 *   "bucket_bits"       0 (default) = auto, else 1..12: width of the key the rows are bucketed by
 *                       (top bits of the first code, continued into the second); takes
 *                       effect when the codes are (re)set
 *   "bucket_skip"       1 (default); 0 visits every bucket -- for measuring the streaming
 *                       rate of the scan, results are the same                             */
/*   "exact_ties"        0 (default): among rows of exactly equal distance the smaller label wins (above).
 *                       1: the reference's own choice -- which of several rows tying at the k-th
 *                       distance survive, and the order equal distances are returned in, come from
 *                       its heap (VAQ.cpp:1750-1757, utils/Heap.hpp:115-169, 322-349).  The scan runs
 *                       with k + 1; a query whose k + 1 smallest distances are distinct is unaffected,
 *                       every other query is replayed through that heap over ALL rows in original
 *                       order (one workgroup per such query: 1M rows x 10 k queries, nine in ten of
 *                       them with ties: 0.65 -> 43 ms; about a second per tied query at 1B rows).
 *                       HEAP / EA: k < 1024; labels and distances are then identical to
 *                       VAQ::search's, slot for slot.
 *                       On a TI index (vaqhip_index_set_ti_clusters, vaqhip_index_cluster_ti_kmeans; methods
 *                       TI and TI | EA; any visit; every k up to VAQHIP_MAX_K) the reference's answer is a
 *                       function of its sequential walk, and EVERY query is answered by a replay of it: the
 *                       members of a cluster in the order std::sort leaves them (VAQ.cpp:973-979: ascending
 *                       rows under mCodeToCCDist[i] > mCodeToCCDist[j]; libstdc++'s introsort, not stable),
 *                       the clusters in the order std::sort of 0..T-1 under qToCCDist[i] < qToCCDist[j]
 *                       leaves (:815-820; NaN centres compare false, keep places in the order and count
 *                       towards maxClusterVisit), then VAQ::searchTriangleInequality (:1540-1692) statement
 *                       for statement: the first k rows enter unconditionally, break at
 *                       bsfK <= qcc - xcc (no slack), admission on dist < bsfKSquared with
 *                       bsfKSquared = bsfK * bsfK, heap_reorder; without EA the answer is the first k rows
 *                       of the walk.  The member order is built at the first such search after the rows
 *                       were (re)grouped (one thread per cluster sorts its members: one-time cost) and
 *                       kept on the index; one workgroup per query walks its visited rows (1M rows x 8 B,
 *                       1000 centres, 10 k queries, k = 100, TI | EA: visit 0.1 2.9 -> 25.5 ms, visit 1
 *                       27.5 -> 110 ms; the member order 16 ms, once).  With option
 *                       "timing" the plan is reported as seed_ms and the replay as scan_ms.  On a
 *                       vaqhip_multi with TI the option has NO effect: a cluster's member list is one
 *                       std::sort over rows of all shards and does not decompose into a chain.
 *                       Set on a vaqhip_multi (HEAP / EA) it holds across the shards
 *                       (the replay runs as a chain from shard to shard, see "multi-device" above); the
 *                       staged search of one-process-per-GPU sharding (vaqhip_search_begin_device)
 *                       stays VAQHIP_EUNSUPPORTED with the option set.
 *                       On a VAQHIP_SUM_SEQUENTIAL index the choice reproduced is BitVecEngine::queryLUT's
 *                       (BitVecEngine.hpp:1282-1317), which keeps its k best in a std::vector under
 *                       libstdc++'s std::push_heap / std::pop_heap / std::sort_heap with the comparator
 *                       a.dist < b.dist: rows in original order, bsfK = FLT_MAX; a row with
 *                       dist < bsfK (strict; :1301) is appended and pushed (:1302-1303); from row k on
 *                       (the row's POSITION in the database, :1304) the maximum of the k + 1 pairs is
 *                       popped and bsfK becomes the new front's distance (:1305-1307); std::sort_heap at
 *                       the end (:1316).  So the first k rows enter unconditionally, and N <= k never
 *                       pops.  Same pipeline and limits as above (vaqhip_search, _projected, _device;
 *                       k < 1024 -- no effect at k == VAQHIP_MAX_K; the staged search stays
 *                       VAQHIP_EUNSUPPORTED); labels are id_base + row, unfilled slots -1 / FLT_MAX.
 *                       Assumes finite lookup tables (the reference reads front() of an empty vector
 *                       when a row sum is not finite); queryLUT's checked projection makes every query
 *                       finite, so finite centroids suffice.
 *   "bucket_major"      1 (default): on a streamed database (> 128 MB of byte codes) with at least 8
 *                       queries in the call, the best-first pass is cut after each query's nearest
 *                       buckets and what is left in reach is scanned bucket by bucket: a bucket's
 *                       rows are streamed once for ALL the queries that still want it, four
 *                       queries' lookup tables at a time in LDS, instead of once per query
 *                       ("Bucket-major second pass"); 0: off; 2: whenever a
 *                       kernel exists (tests).  Results are identical.
 *   "bm_candidates"     slots of a query's candidate buffer in that pass (default 4096); a query that
 *                       overflows it tries the same buckets again under the threshold the stored rows
 *                       give, and is finished by the best-first form if that overflows too
 *   "bm_units"          work units (64 wave steps) of the first pass per query; 0 = about one
 *                       average bucket
 *   "bm_boot"           2: no best-first pass at all -- every query gets a threshold from a
 *                       sample of its nearest rows, and its nearest bucket is the first bucket-major
 *                       round; 0: a capped best-first pass ("bm_units") comes first; 1 (default):
 *                       the former when buckets are large (>= 24 work units on average)
 *   "bm_round"          buckets per query of the middle round (default 6, 0 = no middle round): after
 *                       it the thresholds are near their final values, and the last round -- every
 *                       bucket still in reach -- meets far fewer rows
 *   "bm_runs"           1 (default): runs of rows sharing their first two codes are skipped when out of
 *                       every query's reach ("sub_order": the rows of a bucket are kept ordered by the
 *                       second code; set before the codes)
 *   "bm_queries_per_group", "bm_waves"   launch shape of the second pass (0 = default 4 / 16)    */
int vaqhip_set_option(vaqhip_index *ix, const char *key, int64_t value);

typedef struct {
  float project_ms, lut_ms, seed_ms, scan_ms, merge_ms; /* mean device time per search over
                                                  the searches recorded since the last read;
                                                  seed = threshold pre-pass, scan = the
                                                  full code scan kernel alone             */
  int n_searches;                              /* how many searches that mean covers   */
  int queries_per_pass;                        /* Qb actually used              */
  int slices;                                  /* row slices per query batch    */
  int workgroups;                              /* scan kernel grid size         */
  int passes;                                  /* ceil(nq / Qb)                 */
  int lds_bytes;                               /* LDS per scan workgroup        */
  int seed_slices;                             /* row slices of the pre-pass (0 = none) */
  int early_abandon;                           /* form the scan ran in: 0 none, 1 queue, 2 in place */
  int best_first;                              /* 1: the best-first form ("best_first" option) ran */
  int deferred_queries;                        /* queries of the last search cut in two ("defer_units"): handed
                                                  to the second launch; -1 = the search did not defer */
  int bucket_major;                            /* 1: the bucket-major second pass ran ("bucket_major") */
} vaqhip_timing;
int vaqhip_last_timing(vaqhip_index *ix, vaqhip_timing *out);

/* ---- Hamming engine: BitVecEngine::query and BitVecEngine::queryRerank over packed bit rows -------------------------
 * The rows of BitVecEngine's `data` (bitvectors: W = (n_bits + 63) / 64 uint64 words a row, actBitVLen) resident on the
 * device.  hammingDist (utils/DistanceFunctions.hpp:164-172) counts every bit of every word: nothing is masked, and
 * whatever bits the caller left in the tail of the last word count, in rows and in queries alike.
 *   create      1 <= n_bits, W <= 16 (more: VAQHIP_EUNSUPPORTED -- a distance must fit 16 bits); both are checked
 *               before a device is looked for.
 *   rows        set_rows replaces them (row i has label id_base + i), add_rows appends (labels continue); both copy
 *               synchronously.  set_rows_device takes a pointer on the engine's GPU and copies on `stream`, waiting for
 *               it.  Labels are 32-bit ints: VAQHIP_ERANGE past 2^31 - 1.
 *   query       BitVecEngine::query(queries, k, QueryMethod::Sort) (BitVecEngine.cpp:60-76): every row's distance, then
 *               KNNFromDists (utils/Experiment.hpp:40-56) -- std::sort (libstdc++) of rows 0..k-1 by distance alone,
 *               every later row inserted behind its equals: the reference's labels slot for slot, ties included.
 *               labels_out int32 [nq][k] = id_base + row, distances_out float [nq][k] = the exact integers; slots past
 *               min(k, n) are -1 / FLT_MAX (the reference reads past its array there).
 *   method      the reference's QueryMethod values.  Only VAQHIP_BITVEC_SORT is provided: Heap, HeapEarlyAbandon and
 *               SortEarlyAbandon return the same distances but keep OTHER rows among equal ones (their answer follows
 *               from a sequential walk of all rows per query, and with integer distances every query has ties):
 *               VAQHIP_EUNSUPPORTED.  Any other value VAQHIP_EINVAL.
 *   rerank      BitVecEngine::queryRerank(queries, oriQueries, k, factor, Sort, earlyAbandonRank = false)
 *               (BitVecEngine.cpp:454-466, :521-535): kTemp = min(factor * k, n); the Hamming kTemp best as above, kept
 *               on the device; euclideanDistNoSQRT of each against ori_queries [nq][D] over the refiner's resident rows,
 *               float or byte (distance += (a - b) * (a - b) in dimension order, nothing fused: squared distances, as
 *               the reference returns them); then KNNFromDistsIndicesSupplied (BitVecEngine.hpp:171-187): std::sort of
 *               the first k (dist, idx) pairs by distance alone, every later candidate behind its equals.  Slots past
 *               min(k, kTemp) are -1 / FLT_MAX.  factor >= 1 (VAQHIP_EINVAL); factor * k <= VAQHIP_MAX_K before the
 *               clamp to n (VAQHIP_EUNSUPPORTED).  The refiner must be on the engine's device (VAQHIP_EINVAL) and hold
 *               the engine's number of rows from the engine's id_base (VAQHIP_ESTATE).  Rows or queries that are not
 *               finite are outside the contract: the reference's comparator is no strict weak order on them and its
 *               std::sort is undefined (here the call stays inside its arrays and returns some order).
 *   option      "dist_chunk_bytes" (default 2^30): the queries are cut into chunks whose [chunk][n padded to 32] uint16
 *               distance matrix stays within it (one query at least).  The answer does not depend on it.
 *   limits      1 <= k <= VAQHIP_MAX_K (larger: VAQHIP_EUNSUPPORTED); nq == 0 succeeds and writes nothing; null pointers,
 *               nq < 0 or k < 1 VAQHIP_EINVAL.  Every refusal is made before any device work.
 * The host forms are synchronous; the _device forms take pointers on the engine's GPU, enqueue on `stream` and do not
 * synchronise once the workspaces have their size.  Calls on one engine are serialised.  Errors leave their text in
 * vaqhip_last_error(), as the index's and the refiner's do.  Not provided: the other three methods, earlyAbandonRank,
 * the cluster-info, filtering and naive variants, the encoders (binaryEncoding*), a multi-device form. */
typedef struct vaqhip_bitvec vaqhip_bitvec;
#define VAQHIP_BITVEC_HEAP                0  /* BitVecEngine::QueryMethod (BitVecEngine.hpp:82-84) */
#define VAQHIP_BITVEC_SORT                1
#define VAQHIP_BITVEC_HEAP_EARLY_ABANDON  2
#define VAQHIP_BITVEC_SORT_EARLY_ABANDON  3
int vaqhip_bitvec_create(vaqhip_bitvec **out, int device_id, int n_bits);
void vaqhip_bitvec_destroy(vaqhip_bitvec *bv);
int vaqhip_bitvec_set_rows(vaqhip_bitvec *bv, const uint64_t *rows, int64_t n, int64_t id_base);
int vaqhip_bitvec_set_rows_device(vaqhip_bitvec *bv, const uint64_t *d_rows, int64_t n, int64_t id_base, void *stream);
int vaqhip_bitvec_add_rows(vaqhip_bitvec *bv, const uint64_t *rows, int64_t n_new);
/* rows held, or a negative error code */
int64_t vaqhip_bitvec_size(vaqhip_bitvec *bv);
int vaqhip_bitvec_set_option(vaqhip_bitvec *bv, const char *key, int64_t value);
int vaqhip_bitvec_query(vaqhip_bitvec *bv, const uint64_t *queries, int nq, int k, int method, int32_t *labels_out,
                        float *distances_out);
int vaqhip_bitvec_query_device(vaqhip_bitvec *bv, const uint64_t *d_queries, int nq, int k, int method,
                               int32_t *d_labels_out, float *d_distances_out, void *stream);
int vaqhip_bitvec_query_rerank(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *bit_queries, const float *ori_queries,
                               int nq, int k, int factor, int32_t *labels_out, float *distances_out);
int vaqhip_bitvec_query_rerank_device(vaqhip_bitvec *bv, vaqhip_refiner *r, const uint64_t *d_bit_queries,
                                      const float *d_ori_queries, int nq, int k, int factor, int32_t *d_labels_out,
                                      float *d_distances_out, void *stream);

const char *vaqhip_last_error(void);
int vaqhip_version(void);
/* number of HIP devices visible, or a negative error code */
int vaqhip_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* VAQHIP_H_ */
