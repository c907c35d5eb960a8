// vaqhip_learn.cpp -- VAQ::learnQuantization (VAQ.cpp:1118-1187) over rows where they live: the device forms of
// vaqhip_learn_quantization (include/vaqhip.h, "Learning on the device").  Kernels in vaq_learn.hip, the arithmetic
// shared with the host form (vaqhip_fast.cpp) in learn_plan.h.
//
//   sample   permutation_head(n, sample): the first entries of randomPermutation without the other n - sample
//   gather   the sampled rows as dense floats [sample][D] (device rows: one kernel; host bytes: gathered on the host,
//            uploaded as bytes, widened on the device)
//   per group of Mc subspaces (learn_plan.h: group_columns):
//     tables   launch_project, launch_lut_build, launch_lut_expand in the host form's chunks -- the same launches, so
//              the same bits -- and the group's columns sliced into [sample][Mc][ksub]
//     sort     per column: keys in table order, rocprim's radix sort, the 28 order statistics fetched
//     stats    floors and scales of the 7 alphas on the host, by the host form's code
//     loss     vaq_learn.hip's chains
//   the argmin over alphas on the host, then set_quantization_locked: the state of vaqhip_index_set_lut_quantization
#include "vaqhip_index.h"

#include <chrono>
#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>

#include "kmeans_sample.h"
#include "learn_plan.h"
#include "vaq_front.h"
#include "vaq_learn.h"
#include "vaq_refine.h"

using namespace vaqhost;
namespace ln = vaq::learn;

namespace {

thread_local int64_t g_workspace = 0;  // vaqhip_learn_set_workspace, 0 = the default

struct Clock {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  float lap() {
    const auto now = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(now - t).count();
    t = now;
    return ms;
  }
};

// Declared after the buffers (and host vectors) that work enqueued on `s` reads: the stream is idle before they go,
// whichever way the scope ends.
struct Drain {
  hipStream_t s;
  ~Drain() { (void)hipStreamSynchronize(s); }
};

// what every form refuses before a device is touched; *sample_out: int(ratio * float(n)), VAQ.cpp:1120
int check_learn_args(const vaqhip_index *ix, const void *X, int64_t n, float ratio, int *sample_out) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (n <= 0 || !X) return fail(VAQHIP_EINVAL, "bad X / n");
  if (!ix->fast_ok) return fail(VAQHIP_EUNSUPPORTED, "FAST needs max bits per subspace <= 4 and the grouped row sum");
  if (n > 0x7fffffffLL) return fail(VAQHIP_ERANGE, "the reference's rows are int: n = %lld", (long long)n);
  const int sample = static_cast<int>(ratio * (float)n);
  if (!(sample >= 1)) return fail(VAQHIP_EINVAL, "sampleSize = int(%g * %lld) < 1", ratio, (long long)n);
  if (sample > n) return fail(VAQHIP_EINVAL, "sampleSize = int(%g * %lld) > n: the permutation has n entries", ratio, (long long)n);
  *sample_out = sample;
  return VAQHIP_OK;
}

// The sampled rows are d_rows [sample][D] floats on the index's device, complete on `st`.  The index is locked, its
// device current.  The index's timing is filled; its quantisation and the outputs change only on success.
int learn_core(vaqhip_index *ix, const float *d_rows, int sample, int projected, float *offsets_out, float *scale_out,
               hipStream_t st, float gather_ms, Clock total) {
  const int M = ix->M, D = ix->D, ksub = 1 << ix->max_bits;
  const int64_t rows = (int64_t)sample * ksub;  // rows of the reference's `luts`
  const int Mc = ln::group_columns(g_workspace, sample, M, ksub), groups = ln::group_count(M, Mc);
  vaqhip_learn_timing tm = {};
  tm.sample_rows = sample;
  tm.column_groups = groups;
  tm.chosen_alpha = -1;
  tm.gather_ms = gather_ms;
  ix->learn_last = tm;

  int64_t h_idx[ln::STATS_PER_COLUMN];
  ln::stat_indices(rows, h_idx);
  for (int64_t i : h_idx)
    if (i < 0 || i >= rows) return fail(VAQHIP_EINVAL, "a percentile of %lld values reads element %lld", (long long)rows, (long long)i);

  const int chunk = std::min(sample, 16384);
  const bool do_project = !projected && ix->has_eig;
  if (do_project) HIP_TRY(ix->w_qproj.ensure((size_t)chunk * D * sizeof(float)));
  HIP_TRY(ix->w_lut.ensure((size_t)chunk * ix->lut_floats * sizeof(float)));
  HIP_TRY(ix->w_lutref.ensure((size_t)chunk * M * ksub * sizeof(float)));
  DevBuf b_group, b_keys, b_sorted, b_temp, b_idx, b_stats, b_fs, b_loss, b_bad;
  HIP_TRY(b_group.ensure((size_t)rows * Mc * sizeof(float)));
  HIP_TRY(b_keys.ensure((size_t)rows * sizeof(uint32_t)));
  HIP_TRY(b_sorted.ensure((size_t)rows * sizeof(uint32_t)));
  size_t temp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_keys(nullptr, temp_bytes, b_keys.as<uint32_t>(), b_sorted.as<uint32_t>(), (size_t)rows, 0u,
                                   32u, st));
  HIP_TRY(b_temp.ensure(temp_bytes ? temp_bytes : 16));
  HIP_TRY(b_idx.ensure(sizeof h_idx));
  HIP_TRY(b_stats.ensure((size_t)Mc * ln::STATS_PER_COLUMN * sizeof(float)));
  HIP_TRY(b_fs.ensure((size_t)2 * ln::N_ALPHA * Mc * sizeof(float)));
  HIP_TRY(b_loss.ensure((size_t)ln::N_ALPHA * Mc * sizeof(double)));
  HIP_TRY(b_bad.ensure(sizeof(int)));
  std::vector<float> floors((size_t)ln::N_ALPHA * M), scales((size_t)ln::N_ALPHA * M);
  std::vector<double> loss((size_t)ln::N_ALPHA * M);
  std::vector<float> stats((size_t)Mc * ln::STATS_PER_COLUMN), fs((size_t)2 * ln::N_ALPHA * Mc);
  std::vector<double> gloss((size_t)ln::N_ALPHA * Mc);
  int bad = 0;
  Drain drain{st};  // (everything above is this call's, device and host side, and goes on return)

  WS_SCOPE(ws, ix, st);
  HIP_TRY(hipMemcpyAsync(b_idx.p, h_idx, sizeof h_idx, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(b_bad.p, 0, sizeof(int), st));
  Clock ck;
  for (int g = 0; g < groups; g++) {
    int s0 = 0, m_cols = 0;
    ln::group_range(M, Mc, g, &s0, &m_cols);
    // the group's tables, rebuilt from the resident rows in the host form's chunks
    for (int i0 = 0; i0 < sample; i0 += chunk) {
      const int m = std::min(chunk, sample - i0);
      const float *qp = d_rows + (size_t)i0 * D;
      if (do_project) {
        HIP_TRY(vaq::launch_project(qp, m, D, ix->d_eig.as<float>(), ix->w_qproj.as<float>(), st));
        qp = ix->w_qproj.as<float>();
      }
      HIP_TRY(vaq::launch_lut_build(qp, m, D, M, ix->L, ix->d_sub.as<vaq::SubDesc>(), ix->d_cent_t.as<float>(),
                                    ix->lut_floats, ksub, ix->w_lut.as<float>(), st, 1 << ix->min_bits));
      HIP_TRY(vaq::launch_lut_expand(ix->w_lut.as<float>(), m, M, ix->d_sub.as<vaq::SubDesc>(), ix->lut_floats, ksub,
                                     ix->w_lutref.as<float>(), st));
      HIP_TRY(vaq::launch_learn_slice(ix->w_lutref.as<float>(), m, M, ksub, s0, m_cols, i0, b_group.as<float>(), st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    tm.tables_ms += ck.lap();
    for (int sl = 0; sl < m_cols; sl++) {
      HIP_TRY(vaq::launch_learn_keys(b_group.as<float>(), sample, m_cols, ksub, sl, b_keys.as<uint32_t>(), b_bad.as<int>(), st));
      HIP_TRY(rocprim::radix_sort_keys(b_temp.p, temp_bytes, b_keys.as<uint32_t>(), b_sorted.as<uint32_t>(), (size_t)rows,
                                       0u, 32u, st));
      HIP_TRY(vaq::launch_learn_fetch(b_sorted.as<uint32_t>(), b_idx.as<int64_t>(), ln::STATS_PER_COLUMN,
                                      b_stats.as<float>() + (size_t)sl * ln::STATS_PER_COLUMN, st));
    }
    HIP_TRY(hipMemcpyAsync(&bad, b_bad.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stats.data(), b_stats.p, (size_t)m_cols * ln::STATS_PER_COLUMN * sizeof(float),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tm.sort_ms += ck.lap();
    if (bad) {
      ix->learn_last = tm;
      return fail(VAQHIP_EINVAL, "a table value of a sampled row is NaN or infinite: std::sort has no defined result on it");
    }
    // floors[7][m_cols], then scales[7][m_cols], as the loss kernel reads them
    for (int a = 0; a < ln::N_ALPHA; a++)
      for (int sl = 0; sl < m_cols; sl++) {
        float fl, sc;
        ln::floor_scale_from_stats(&stats[(size_t)sl * ln::STATS_PER_COLUMN], rows, a, &fl, &sc);
        floors[(size_t)a * M + s0 + sl] = fs[(size_t)a * m_cols + sl] = fl;
        scales[(size_t)a * M + s0 + sl] = fs[(size_t)(ln::N_ALPHA + a) * m_cols + sl] = sc;
      }
    HIP_TRY(hipMemcpyAsync(b_fs.p, fs.data(), (size_t)2 * ln::N_ALPHA * m_cols * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    tm.order_stats_ms += ck.lap();
    HIP_TRY(vaq::launch_learn_loss(b_group.as<float>(), sample, m_cols, ksub, b_fs.as<float>(),
                                   b_fs.as<float>() + (size_t)ln::N_ALPHA * m_cols, b_loss.as<double>(), st));
    HIP_TRY(hipMemcpyAsync(gloss.data(), b_loss.p, (size_t)ln::N_ALPHA * m_cols * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int a = 0; a < ln::N_ALPHA; a++)
      for (int sl = 0; sl < m_cols; sl++) loss[(size_t)a * M + s0 + sl] = gloss[(size_t)a * m_cols + sl];
    tm.loss_ms += ck.lap();
  }
  if (int rc = ws.finish()) return rc;
  const int best_a = ln::best_alpha(loss.data(), M, tm.loss);
  tm.chosen_alpha = best_a;
  tm.total_ms = total.lap();
  ix->learn_last = tm;
  if (best_a < 0) return fail(VAQHIP_EINVAL, "no alpha gives a finite quantisation loss");
  const float *off = &floors[(size_t)best_a * M], *sc = &scales[(size_t)best_a * M];
  if (int rc = set_quantization_locked(ix, off, sc)) return rc;
  if (offsets_out) std::memcpy(offsets_out, off, (size_t)M * sizeof(float));
  if (scale_out) std::memcpy(scale_out, sc, (size_t)M * sizeof(float));
  ix->learn_last.total_ms += total.lap();
  return VAQHIP_OK;
}

// host byte rows: the sample's bytes gathered on the host, uploaded as bytes, widened on the device
int learn_host_u8(vaqhip_index *ix, const uint8_t *X, int64_t n, int projected, float ratio, float *offsets_out,
                  float *scale_out) {
  int sample = 0;
  if (int rc = check_learn_args(ix, X, n, ratio, &sample)) return rc;
  ENTRY(ix);
  Clock total, ck;
  const size_t D = (size_t)ix->D;
  const std::vector<int> perm = vaq::permutation_head(n, sample);
  std::vector<uint8_t> xs((size_t)sample * D);
  for (int i = 0; i < sample; i++) std::memcpy(&xs[(size_t)i * D], X + (size_t)perm[(size_t)i] * D, D);
  DevBuf b_bytes, b_rows;
  HIP_TRY(b_bytes.ensure(xs.size()));
  HIP_TRY(b_rows.ensure(xs.size() * sizeof(float)));
  hipStream_t st = ix->stream;
  Drain drain{st};
  HIP_TRY(hipMemcpyAsync(b_bytes.p, xs.data(), xs.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(vaq::launch_widen_rows_u8(b_bytes.as<uint8_t>(), (int64_t)xs.size(), b_rows.as<float>(), st));
  HIP_TRY(hipStreamSynchronize(st));
  return learn_core(ix, b_rows.as<float>(), sample, projected, offsets_out, scale_out, st, ck.lap(), total);
}

}  // namespace

// device rows of either type, n x D on the index's device and complete: the sampled ones are gathered by one kernel
int vaqhost::learn_rows_device(vaqhip_index *ix, vaq::RowsRef d_X, int64_t n, int projected, float ratio,
                               float *offsets_out, float *scale_out) {
  int sample = 0;
  if (int rc = check_learn_args(ix, d_X.p, n, ratio, &sample)) return rc;
  ENTRY(ix);
  Clock total, ck;
  const std::vector<int> perm = vaq::permutation_head(n, sample);
  DevBuf b_perm, b_rows;
  HIP_TRY(b_perm.ensure((size_t)sample * sizeof(int)));
  HIP_TRY(b_rows.ensure((size_t)sample * ix->D * sizeof(float)));
  hipStream_t st = ix->stream;
  Drain drain{st};
  HIP_TRY(hipMemcpyAsync(b_perm.p, perm.data(), (size_t)sample * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(vaq::launch_learn_gather(d_X, b_perm.as<int>(), sample, ix->D, b_rows.as<float>(), st));
  HIP_TRY(hipStreamSynchronize(st));
  return learn_core(ix, b_rows.as<float>(), sample, projected, offsets_out, scale_out, st, ck.lap(), total);
}

extern "C" {

int vaqhip_learn_quantization_u8(vaqhip_index *ix, const uint8_t *X, int64_t n, int projected, float sample_ratio,
                                 float *offsets_out, float *scale_out) {
  return learn_host_u8(ix, X, n, projected, sample_ratio, offsets_out, scale_out);
}
int vaqhip_learn_quantization_device(vaqhip_index *ix, const float *d_X, int64_t n, int projected, float sample_ratio,
                                     float *offsets_out, float *scale_out) {
  return learn_rows_device(ix, vaq::RowsRef{d_X, 4}, n, projected, sample_ratio, offsets_out, scale_out);
}
int vaqhip_learn_quantization_u8_device(vaqhip_index *ix, const uint8_t *d_X, int64_t n, int projected,
                                        float sample_ratio, float *offsets_out, float *scale_out) {
  return learn_rows_device(ix, vaq::RowsRef{d_X, 1}, n, projected, sample_ratio, offsets_out, scale_out);
}

int vaqhip_learn_set_workspace(int64_t bytes) {
  if (bytes < 0) return fail(VAQHIP_EINVAL, "workspace = %lld bytes: 0 (the default) or a number of bytes", (long long)bytes);
  g_workspace = bytes;
  return VAQHIP_OK;
}

int vaqhip_last_learn_timing(vaqhip_index *ix, vaqhip_learn_timing *out) {
  if (!ix || !out) return fail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(ix->mu);
  *out = ix->learn_last;
  return VAQHIP_OK;
}

// (vaqhip_internal.h) the sample itself, d_rows [sample][D] floats on the index's device and complete: the multi
// refiner form gathers it across the shards and learns here
int vaqhip_internal_learn_sample_device(vaqhip_index *ix, const float *d_rows, int sample, int projected,
                                        float gather_ms, float *offsets_out, float *scale_out) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (!d_rows || sample < 1) return fail(VAQHIP_EINVAL, "bad sample");
  if (!ix->fast_ok) return fail(VAQHIP_EUNSUPPORTED, "FAST needs max bits per subspace <= 4 and the grouped row sum");
  ENTRY(ix);
  Clock total;
  return learn_core(ix, d_rows, sample, projected, offsets_out, scale_out, ix->stream, gather_ms, total);
}

int vaqhip_internal_fast_ok(vaqhip_index *ix) {
  if (!ix) return 0;
  return ix->fast_ok ? 1 : 0;
}

}  // extern "C"
