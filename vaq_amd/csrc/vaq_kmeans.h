// vaq_kmeans.h -- the k-means of VAQ::clusterTI(true) (vaq_kmeans.hip).
#ifndef VAQ_KMEANS_H_
#define VAQ_KMEANS_H_

#include "vaq_common.h"

namespace vaq {

// d_scodes[slot][seg] = the first seg codes of the sampled rows, read from the packed rows in place (either layout,
// bucketed or TI-grouped order; d_perm: packed position -> original row).  sample_rows (host, n_sample original
// rows, all different): slot = the row's position in it; nullptr (then n_sample == n): every row, slot = the row.
// Scratch: 16 bytes per sampled row, nothing per row of the index.  Synchronises the stream.
hipError_t kmeans_gather_packed(const uint32_t *d_packed, int64_t n, int M, int layout, int W, const SubDesc *sub,
                                const uint32_t *d_perm, const int *sample_rows, int n_sample, int seg,
                                uint16_t *d_scodes, hipStream_t st);
// host time per phase over all iterations, each phase ended by a stream synchronisation
struct KmeansPhases {
  double assign_ms = 0, accumulate_ms = 0, update_ms = 0;
};
// a device that takes a share of the assign step: its stream, and the index's tables as that device holds them
struct KmeansDev {
  int device;
  hipStream_t st;
  const SubDesc *sub;
  const float *cent;
};
constexpr int KMEANS_MAX_DEVS = 16;
// KMeans::staticFitSampling on the rows whose first seg codes are d_scodes[rows][seg] (on devs[0], complete on
// its stream, in the reference's row order): d_means[T][seg * L] (devs[0]) seeded from rows seed_rows[0..T) (host),
// then Lloyd iterations until no centre changes or max_iter.  The assign step is cut over the G devices (device g
// takes the slice kmeans_assign_slice gives it: keys and values come back to devs[0] by peer copy, the new centres
// go out the same way); everything else runs on devs[0], which holds all decoded rows, so the result does not
// depend on G.  G == 1 sets no device: devs[0].device is current.  G > 1 leaves devs[0].device current.
// *no_centre_out != 0: some row had no centre at a distance below FLT_MAX (the reference indexes row -1 there);
// the centres are then not to be used.  phases (optional) adds one synchronisation per phase; assign_ms then
// holds the copies too.  *failed_dev (optional): the index in devs of the device a failing call belonged to.
// Synchronises the streams.
hipError_t kmeans_fit(const KmeansDev *devs, int G, const uint16_t *d_scodes, int rows, int seg, int L,
                      const int *seed_rows, int T, int max_iter, float *d_means, int *iters_out, int *no_centre_out,
                      KmeansPhases *phases, int *failed_dev);

} // namespace vaq
#endif
