// vaqhip_internal.h -- entries of the single-device index that only the multi-device host
// (vaqhip_multi.cpp) calls: the pieces of option "exact_ties" as a chain over shards (vaq_exact.hip).
// Not part of the public interface (include/vaqhip.h).
#ifndef VAQHIP_INTERNAL_H
#define VAQHIP_INTERNAL_H
#include "vaqhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* queries per internal launch set: the lookup tables of at most this many queries are kept per search */
int vaqhip_internal_query_chunk(void);
/* 1 when "exact_ties" is set on this index and has an effect for this k (not TI, not the sequential
 * sum, not FAST, k < VAQHIP_MAX_K) */
int vaqhip_internal_exact_applies(vaqhip_index *ix, int k);
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
 * vaqhip_internal_search_plain_device) from d_state_in (NULL: neutral) to d_state_out; 2 * k words per
 * list entry */
int vaqhip_internal_exact_link_device(vaqhip_index *ix, int k, const int *d_list, const unsigned *d_count, int e0,
                                      int n_entries, const int32_t *d_state_in, int32_t *d_state_out, void *stream);
/* on `device`: the reference's heap_reorder on the last state, into the listed queries' k slots */
int vaqhip_internal_exact_finish_device(int device, const int32_t *d_state, const int *d_list, const unsigned *d_count,
                                        int n_entries, int k, int32_t *d_labels, float *d_distances, void *stream);

#ifdef __cplusplus
}
#endif
#endif
