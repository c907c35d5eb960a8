// vaqhip_kmeans_fit.cpp -- vaqhip_refiner_fit_centres*: KMeans::fit (KMeans.hpp:42-107) with the caller's seeds over a
// refiner's resident rows.  Kernels and the iteration loop in vaq_kmeans_fit.hip, statement in vaq_kmeans_fit.h.
#include "vaqhip_bitvec.h"

#include "vaq_kmeans_fit.h"

using namespace vaqhost;

namespace {

thread_local vaqhip_fit_centres_timing g_last = {};

// both entries: seeds, centres and assignment are the device's and the work goes on st, or the host's
int fit_entry(vaqhip_refiner *r, int T, const int32_t *seed_rows, int max_iter, float *centres_out, int32_t *belongs_to_out,
              int *iterations_out, bool on_device, hipStream_t st) {
  if (T < 1) return fail(VAQHIP_EINVAL, "T=%d centres", T);
  if (T > vaq::BITVEC_CLUSTERS_MAX) return fail(VAQHIP_EUNSUPPORTED, "T=%d > %d (the cluster state's limit)", T, vaq::BITVEC_CLUSTERS_MAX);
  if (max_iter < 1) return fail(VAQHIP_EINVAL, "max_iter=%d", max_iter);
  if (!r) return fail(VAQHIP_EINVAL, "refiner is null");
  if (!seed_rows || !centres_out || !belongs_to_out || !iterations_out) return fail(VAQHIP_EINVAL, "null pointer");
  HandleCore *h = refiner_core(r);
  ENTRY(h);
  const RefinerView rv = refiner_view(r);
  if (rv.N < 1) return fail(VAQHIP_ESTATE, "the refiner holds no rows");
  if (!on_device) {
    st = h->stream;
    for (int c = 0; c < T; c++)
      if (seed_rows[c] < 0 || seed_rows[c] >= rv.N)
        return fail(VAQHIP_EINVAL, "seed_rows[%d]=%d outside [0, %lld)", c, seed_rows[c], (long long)rv.N);
  }
  vaq::KmeansFitWork w;  // (freed when the call ends, behind the synchronisation below)
  DevBuf d_seeds;
  if (!on_device) {
    HIP_TRY(d_seeds.ensure((size_t)T * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(d_seeds.p, seed_rows, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  vaq::KmeansFitResult res;
  HIP_TRY(vaq::kmeans_fit(rv.rows, rv.N, rv.D, T, on_device ? seed_rows : d_seeds.as<int32_t>(), max_iter, w, &res, st));
  g_last = vaqhip_fit_centres_timing{res.assign_ms, res.group_ms, res.update_ms, res.iterations, rv.N, T, rv.D};
  if (res.flags.bad_seed != INT32_MAX)
    return fail(VAQHIP_EINVAL, "seed_rows[%d] outside [0, %lld)", res.flags.bad_seed, (long long)rv.N);
  if (res.flags.no_centre_row != INT32_MAX)
    return fail(VAQHIP_EINVAL, "row %d has no centre at a distance below FLT_MAX in iteration %d (a NaN or an overflow in every "
                "sum): the reference would index new_centroids[-1]; nothing is written", res.flags.no_centre_row, res.iterations);
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(hipMemcpyAsync(centres_out, w.means.p, (size_t)T * rv.D * sizeof(float), kind, st));
  HIP_TRY(hipMemcpyAsync(belongs_to_out, w.belongs.p, (size_t)rv.N * sizeof(int32_t), kind, st));
  HIP_TRY(hipStreamSynchronize(st));
  *iterations_out = res.iterations;
  return VAQHIP_OK;
}

}  // namespace

extern "C" {

int vaqhip_refiner_fit_centres(vaqhip_refiner *r, int T, const int32_t *seed_rows, int max_iter, float *centres_out,
                               int32_t *belongs_to_out, int *iterations_out) {
  return fit_entry(r, T, seed_rows, max_iter, centres_out, belongs_to_out, iterations_out, false, nullptr);
}
int vaqhip_refiner_fit_centres_device(vaqhip_refiner *r, int T, const int32_t *d_seed_rows, int max_iter, float *d_centres_out,
                                      int32_t *d_belongs_to_out, int *iterations_out, void *stream) {
  return fit_entry(r, T, d_seed_rows, max_iter, d_centres_out, d_belongs_to_out, iterations_out, true,
                   static_cast<hipStream_t>(stream));
}

int vaqhip_last_fit_centres_timing(vaqhip_fit_centres_timing *out) {
  if (!out) return fail(VAQHIP_EINVAL, "null pointer");
  *out = g_last;
  return VAQHIP_OK;
}

}  // extern "C"
