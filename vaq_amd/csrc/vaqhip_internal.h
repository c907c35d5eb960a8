// vaqhip_internal.h -- entries of the single-device index that only the multi-device host
// (vaqhip_multi*.cpp) calls: the pieces of option "exact_ties" as a chain over shards (vaq_exact.hip), and
// one shard's part of a FAST search (vaq_fast.hip), and one shard's part of the k-means of clusterTI (vaq_kmeans.hip).
// Not part of the public interface (include/vaqhip.h).
#ifndef VAQHIP_INTERNAL_H
#define VAQHIP_INTERNAL_H
#include "vaqhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* queries per internal launch set: the lookup tables of at most this many queries are kept per search */
int vaqhip_internal_query_chunk(void);
/* 1 when "exact_ties" is set on this index and the chain over shards reproduces it for this k (not TI, not
 * FAST, k < VAQHIP_MAX_K).  TI: on one index the option replays the reference's walk, but its member list of a
 * cluster is ONE std::sort over rows of all shards, whose order among equal keys does not decompose into a
 * chain -- so this answers 0 and a multi-device index with TI keeps the default tie contract. */
int vaqhip_internal_exact_applies(vaqhip_index *ix, int k);
/* marks the index as one shard of several: "exact_ties" then leaves its TI searches alone (above) */
void vaqhip_internal_set_sharded(vaqhip_index *ix, int sharded);
/* int32 words of one list entry's heap state in the chain: 2 * k (k distance bits, k ids), or on a
 * sequential-sum index 2 * (k + 1) + 2 (queryLUT's k + 1 pairs, their number, bsfK) */
int vaqhip_internal_exact_state_words(vaqhip_index *ix, int k);
/* vaqhip_search_device by the smallest-label rule whatever "exact_ties" says; nq at most the query
 * chunk.  The index keeps the lookup tables of these queries until its next search. */
int vaqhip_internal_search_plain_device(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                                        int32_t *d_labels, float *d_distances, void *stream);
/* on `device`: queries whose k + 1 merged distances are distinct are copied to d_labels / d_distances
 * [nq][k], the others are appended to d_list; d_count (one word) is zeroed first */
int vaqhip_internal_exact_flag_device(int device, int nq, int k, const int32_t *d_in_labels, const float *d_in_dist,
                                      int32_t *d_labels, float *d_distances, int *d_list, unsigned *d_count,
                                      void *stream);
/* one link of the chain on this index: entries [e0, e0 + n_entries) of d_list (queries of the last
 * vaqhip_internal_search_plain_device) from d_state_in (NULL: neutral) to d_state_out;
 * vaqhip_internal_exact_state_words words per list entry.  row0: the position of this index's first row in
 * the whole database (a sequential-sum index admits unconditionally below position k) */
int vaqhip_internal_exact_link_device(vaqhip_index *ix, int k, int64_t row0, const int *d_list, const unsigned *d_count,
                                      int e0, int n_entries, const int32_t *d_state_in, int32_t *d_state_out,
                                      void *stream);
/* on `device`: the reference's heap_reorder (seq != 0: queryLUT's std::sort_heap) on the last state, into the
 * listed queries' k slots */
int vaqhip_internal_exact_finish_device(int device, const int32_t *d_state, const int *d_list, const unsigned *d_count,
                                        int n_entries, int seq, int k, int32_t *d_labels, float *d_distances,
                                        void *stream);


/* 1 when FAST is the method in force on this index (none of TI, EA, HEAP set) */
int vaqhip_internal_fast_in_force(vaqhip_index *ix);
/* One shard's part of a FAST search over a sharded index ("FAST across shards"), for all
 * nq queries, chunked by this shard's own row count.  row_offset: the shard's first row within the whole index;
 * kk = min(k, rows of the whole index), the head.  The shard's rows at index positions < kk are head rows: their
 * distances are written to d_head[q * kk + position] (uint16; positions other shards own are left alone) and they
 * are left out of the list.  d_labels / d_distances [nq][k]: the other rows' top min(k, their count) by
 * (dist, row), labels id_base + row, the rest -1 / FLT_MAX.  VAQHIP_ESTATE while a staged search is open, without
 * a quantisation, or when FAST is not in force. */
int vaqhip_internal_search_fast_shard_device(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                                             int64_t row_offset, int kk, int32_t *d_labels, float *d_distances,
                                             uint16_t *d_head, void *stream);
/* on `device`: d_head[q * kk + p] for p < kk from the gathered planes; part g (n_parts <= 16) owns positions
 * [start[g], start[g + 1]) and holds them at d_planes[g * plane_stride + q * kk + p]; start[n_parts] = kk */
int vaqhip_internal_fast_head_gather_device(int device, const uint16_t *d_planes, int64_t plane_stride, int n_parts,
                                            const int *start, int nq, int kk, uint16_t *d_head, void *stream);


/* The k-means of clusterTI over the shards of a multi index (vaq_kmeans.hip).
 * What vaqhip_index_cluster_ti_kmeans refuses for reasons the index alone knows (T >= 1 assumed): the limits of
 * set_ti_clusters, no codes yet, a staged search open. */
int vaqhip_internal_kmeans_check(vaqhip_index *ix, int T, int seg_num);
/* scodes_out (host) [n_sample][seg_num] = the first seg_num codes of this index's rows sample_rows[0 .. n_sample)
 * (local rows, all different), read from the packed rows in place; sample_rows NULL (n_sample = the index's rows):
 * every row in original order.  Synchronises. */
int vaqhip_internal_kmeans_gather(vaqhip_index *ix, const int *sample_rows, int n_sample, int seg_num,
                                  uint16_t *scodes_out);
/* the index's subspace table (vaq::SubDesc [M]) and centroids on its device, and D / M */
int vaqhip_internal_kmeans_tables(vaqhip_index *ix, const void **d_sub, const float **d_cent, int *L);


/* learnQuantization's device forms on a multi index (vaqhip_learn.cpp).  1 when the index can hold FAST codes. */
int vaqhip_internal_fast_ok(vaqhip_index *ix);
/* vaqhip_learn_quantization_device without the sampling: d_rows [sample][D] floats on the index's device, complete,
 * ARE the sample in sample order.  gather_ms: what the caller spent bringing them there, for the timing. */
int vaqhip_internal_learn_sample_device(vaqhip_index *ix, const float *d_rows, int sample, int projected,
                                        float gather_ms, float *offsets_out, float *scale_out);


/* The sharded quantile fit (vaqhip_multi_lutfit.cpp): every refusal of vaqhip_lut_fit_quantiles that needs no device,
 * with its code and text (vaqhip_last_error).  X: the rows, or any non-null pointer that stands for resident ones. */
int vaqhip_internal_lut_fit_check(const void *X, int64_t n, int D, const int *bits, const void *centroids_out,
                                  const void *quantiles_out);


/* The sharded codebook fit (vaqhip_multi_codebooks.cpp) over the single fit's host side (vaqhip_codebooks.cpp).
 * Every refusal of vaqhip_fit_codebooks that needs no device, with its code and text (vaqhip_last_error). */
int vaqhip_internal_fit_codebooks_check(const void *X, int64_t n, int D, int M, const int *bits, int max_iter,
                                        const void *centroids_out);
/* vaqhip_fit_codebooks[_u8] from the upload on, over n x D rows resident on `device` (elem: 4 float, 1 byte); eigvec
 * and the outputs are the host's.  What vaqhip_refiner_fit_codebooks runs: a multi refiner of one shard is that. */
int vaqhip_internal_fit_codebooks_rows_device(int device, const void *d_X, int elem, int64_t n, int D, int M,
                                              const int *bits, const float *eigvec, int max_iter, float *centroids_out,
                                              int *iters_out, int *nan_rows_out);
/* 1 when vaqhip_fit_codebooks_set_timing(1) holds for the calling thread */
int vaqhip_internal_fit_codebooks_timing_on(void);

#ifdef __cplusplus
}
#endif
#endif
