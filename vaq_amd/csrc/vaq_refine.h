// vaq_refine.h -- VAQ::refine over resident raw rows (vaq_refine.hip): rows is N x D, row i carries label id_base + i;
// distances in Eigen's summation order; a label outside [id_base, id_base + N) is skipped and its row never read.
// exact != 0: the k best are the reference heap's (VAQ.cpp:863-872), else the k smallest by (distance, label).
// 1 <= k <= R <= 2048, D <= refine_rows_max_dim().  Rows of either type: RowsRef (vaq_common.h).
#ifndef VAQ_REFINE_H_
#define VAQ_REFINE_H_

#include "refine_owner.h"
#include "vaq_common.h"

namespace vaq {

size_t refine_rows_max_dim();
hipError_t launch_refine_rows(const float *Q, int nq, int D, RowsRef rows, int64_t N, int64_t id_base,
                              const int32_t *labels_in, int R, int k, int exact, int32_t *labels, float *dist,
                              hipStream_t st);
// The same in two halves, for rows sharded over devices (refine_owner.h has the cut).  launch_refine_dist: one shard's
// rows (n x D, row i carries label lo_label + i) -> plane[q * R + c] for the candidates it holds, other slots left
// alone; n == 0 launches nothing.  launch_refine_select: slot c of query q is read from the plane of the shard that owns
// its label (planes + owner * plane_stride), labels nobody owns are skipped, then launch_refine_rows' selection.
hipError_t launch_refine_dist(const float *Q, int nq, int D, RowsRef rows, int64_t n, int64_t lo_label,
                              const int32_t *labels_in, int R, float *plane, hipStream_t st);
hipError_t launch_refine_select(const int32_t *labels_in, int nq, const float *planes, size_t plane_stride,
                                const RefineBounds &bounds, int R, int k, int exact, int32_t *labels, float *dist,
                                hipStream_t st);
// n x D byte rows widened to float (dst[i] = (float)src[i]): the encoders read float rows, so a chunk of byte rows
// that no projection turns into floats goes through here first
hipError_t launch_widen_rows_u8(const uint8_t *src, int64_t elems, float *dst, hipStream_t st);

} // namespace vaq
#endif
