// vaq_merge.h -- the final k-min over a query's partial lists, and the first-generation refine that shares its fold
// (vaq_merge.hip).
#ifndef VAQ_MERGE_H_
#define VAQ_MERGE_H_

#include "vaq_scan_params.h"  // DeferRec

namespace vaq {

// in_final != 0: inputs use the API's -1 / FLT_MAX convention for empty slots
// candidate i of list l of query q sits at l*list_stride + q*query_stride + i
// labels == nullptr: no result is written (only thr_out is wanted).
// thr_out (optional): [nq] float bits, lowered to each query's k-th distance.
// More than 64 lists are folded in levels through scratch_d/scratch_id
// (merge_scratch_elems() elements each).
size_t merge_scratch_elems(int n_lists, int nq, int k);
// part_cnt (optional, scan partials only): real entries per list, [nq][n_lists]
hipError_t launch_merge(const float *part_d, const int *part_id, const int *part_cnt, int n_lists,
                        int64_t list_stride, int64_t query_stride, int nq, int k,
                        int64_t id_base, int in_final, int32_t *labels, float *dist,
                        unsigned *thr_out, float *scratch_d, int *scratch_id, hipStream_t st);
// queries cut in two by the best-first form (ScanParams::defer_*): the first launch's result (already in
// labels/dist, the API's format) and the n_lists lists of the second -> the k best, in place
hipError_t launch_defer_merge(const unsigned *defer_count, int defer_cap, const DeferRec *defer_list, int n_lists, int k,
                              const float *part_d, const int *part_id, const int *part_cnt, int64_t id_base,
                              int32_t *labels, float *dist, hipStream_t st);
// VAQ::refine: exact re-rank of R (<= 2048) candidates per query
hipError_t launch_refine(const float *Q, int nq, int D, const float *dataset, const float *rows,
                         const int32_t *labels_in, int R, int k, int32_t *labels, float *dist,
                         hipStream_t st);

} // namespace vaq
#endif
