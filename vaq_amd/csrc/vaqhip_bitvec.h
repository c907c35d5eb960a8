// vaqhip_bitvec.h -- the Hamming engine's handle, shared by its two hosts: vaqhip_bitvec.cpp (rows and queries) and
// vaqhip_bitvec_encode.cpp (the encoders that make the rows on the device).
#ifndef VAQHIP_BITVEC_H
#define VAQHIP_BITVEC_H
#include "vaqhip_index.h"

#include "vaq_bitvec_clusters.h"
#include "vaq_bitvec_encode.h"
#include "vaq_bitvec_ti.h"
#include "vaqhip_refine_common.h"

// What vaqhip_bitvec_set_encoder leaves on the device: the rotation, and for the quantile form the allocated
// dimensions and their running-maximum thresholds, ragged.  Read by encodes enqueued on any stream: a set waits for the
// device before it replaces them.
struct BitvecEncoder {
  bool set = false;
  int D = 0, n_live = 0, pm_floats = 0;
  bool quantile = false, has_eig = false;
  vaqhost::DevBuf eig, live, pm;
  vaq::BitvecEncodePlan plan(int W) const {
    return vaq::BitvecEncodePlan{D, W, has_eig ? eig.as<float>() : nullptr, n_live,
                                 quantile ? live.as<vaq::BitvecLive>() : nullptr, pm.as<float>(), pm_floats};
  }
};

// What vaqhip_bitvec_set_clusters leaves on the device: the centres dimension-major, the clusters' first image rows
// (start[T + 1]), the original row of every image row, and the bit rows once more, cluster after cluster.  Whatever
// replaces or appends rows drops it (`set`); a set waits for the device before it replaces the buffers.
struct BitvecClusters {
  bool set = false;
  int T = 0, D = 0;
  vaqhost::DevBuf centres_t, start, member, image;
};

// What vaqhip_bitvec_set_ti_clusters_from_refiner leaves on the device: the centres dimension-major, and the refiner's
// rows grouped cluster after cluster, inside one the farthest from its centre first -- start[T + 1], member[n] (the raw
// row of every grouped position) and xcc[n] (its distance to its centre).  The raw rows stay where the refiner has them.
// Separate from BitvecClusters (whose members ascend by row); dropped with it.
struct BitvecTiClusters {
  bool set = false;
  int T = 0, D = 0;
  vaqhost::DevBuf centres_t, start, member, xcc;
};

struct vaqhip_bitvec : vaqhost::HandleCore {
  int n_bits = 0, W = 0;
  int64_t N = 0, id_base = 0;
  int64_t dist_chunk_bytes = (int64_t)1 << 30;  // option "dist_chunk_bytes": the distance matrix of a chunk of queries
  int ti_refresh = vaq::BITVEC_TI_REFRESH;      // option "ti_refresh": admissions that make the TI walk compact its pool
  vaqhost::RowStore rows;  // uint64 words (elem 8, W a row), room for the rows padded to FAST_ROW_PAD
  // workspaces (grow-only), shared by the callers' streams (WS_SCOPE): the distance matrix, FAST's head order and its
  // scratch; the cluster form's visit lists and plans; the TI form's centre distances and, for its host form, the counts
  vaqhost::DevBuf w_dist, w_order, w_scratch, w_visit, w_plan, w_qcc, w_eval;
  vaqhost::StagingBufs w;  // the rerank's candidates and the staging of the host forms
  BitvecEncoder enc;
  BitvecClusters cl;
  BitvecTiClusters ti;
  // the rows change: both cluster states describe them as they were
  void drop_clusters() { cl.set = ti.set = false; }
};

// What vaqhip_cluster_index.cpp shares with vaqhip_bitvec.cpp, which defines both.  The caller holds bv->mu with the
// engine's device current (ENTRY).
namespace vaqhost __attribute__((visibility("hidden"))) {
// set_clusters' own limits, before any device work
inline int bitvec_check_centres(const float *centroids, int T, int D) {
  if (!centroids) return fail(VAQHIP_EINVAL, "null pointer");
  if (T < 1 || T > vaq::BITVEC_CLUSTERS_MAX) return fail(VAQHIP_EINVAL, "T=%d centres outside 1..%d", T, vaq::BITVEC_CLUSTERS_MAX);
  if (D < 1 || D > vaq::BITVEC_CLUSTERS_MAX_DIM)
    return fail(VAQHIP_EINVAL, "D=%d outside 1..%d (the refiner's row limit)", D, vaq::BITVEC_CLUSTERS_MAX_DIM);
  return VAQHIP_OK;
}
// the refiner describes the engine's rows, on the engine's device; rv is read under the refiner's lock
int check_refiner_rows(const vaqhip_bitvec *bv, const RefinerView &rv);
// vaqhip_bitvec_set_clusters behind its refusals of T and D: the counting sort, the centres, the cluster-major image
int bitvec_set_clusters_locked(vaqhip_bitvec *bv, const float *centroids, int T, int D, const int32_t *clust_idx);
}  // namespace vaqhost
#endif
