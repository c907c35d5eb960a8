// vaqhip_fast.cpp -- the FAST search method on the single-device index (vaq_fast.hip): the code image,
// the LUT quantisation and how it is learnt, the search, and one shard's part of a sharded search.
#include "vaqhip_index.h"

#include <cmath>
#include <limits>
#include <random>
#include <thread>

#include "learn_plan.h"
#include "vaq_fast.h"
#include "vaq_front.h"
#include "vaq_ti.h"

using namespace vaqhost;

namespace vaqhost {
// FAST is the method in force: the reference's precedence is TI > EA > HEAP > FAST (VAQ.cpp:799-834)
bool fast_only(const vaqhip_index *ix) {
  return (ix->methods & VAQHIP_METHOD_FAST) &&
         !(ix->methods & (VAQHIP_METHOD_TI | VAQHIP_METHOD_EA | VAQHIP_METHOD_HEAP));
}

void fast_release(vaqhip_index *ix) {
  for (DevBuf *b : {&ix->d_fast_codes, &ix->w_fast_small, &ix->w_fast_dist, &ix->w_fast_order, &ix->w_fast_scratch})
    b->release();
  ix->fast_rows = -1;
  ix->fast_cap = 0;
}

// FAST code image, original row order: rows [row_begin, row_end) are packed from d_u16 (whose first row
// is row_begin), the rows before row_begin are kept (an append), padding rows hold code 0.  Only while
// FAST is in force and the image is current up to row_begin; otherwise the image is dropped and the next
// FAST search rebuilds it (fast_codes_ensure).  Appends grow the allocation geometrically.  Synchronises.
int fast_codes_update(vaqhip_index *ix, const uint16_t *d_u16, int64_t row_begin, int64_t row_end,
                             hipStream_t st) {
  if (!ix->fast_ok || !fast_only(ix) || (row_begin > 0 && ix->fast_rows != row_begin)) {
    fast_release(ix);
    return VAQHIP_OK;
  }
  const size_t row_bytes = (size_t)16 * vaq::fast_code_words(ix->M);
  const int64_t n_pad = std::max<int64_t>(1, (row_end + vaq::FAST_ROW_PAD - 1) / vaq::FAST_ROW_PAD) * vaq::FAST_ROW_PAD;
  if (n_pad > ix->fast_cap || row_begin == 0) {
    const int64_t cap = row_begin == 0 ? n_pad
                                       : std::max<int64_t>(n_pad, (2 * ix->fast_cap) / vaq::FAST_ROW_PAD * vaq::FAST_ROW_PAD);
    DevBuf nb;
    HIP_TRY(nb.ensure((size_t)cap * row_bytes));
    HIP_TRY(hipMemsetAsync(nb.p, 0, (size_t)cap * row_bytes, st));
    if (row_begin > 0)
      HIP_TRY(hipMemcpyAsync(nb.p, ix->d_fast_codes.p, (size_t)row_begin * row_bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the old buffer is freed below)
    std::swap(ix->d_fast_codes.p, nb.p);
    std::swap(ix->d_fast_codes.cap, nb.cap);
    ix->fast_cap = cap;
  }
  HIP_TRY(vaq::launch_fast_pack_codes(d_u16, row_begin, row_end, ix->M, ix->d_fast_codes.as<uint32_t>(), st));
  HIP_TRY(hipStreamSynchronize(st));
  ix->fast_rows = row_end;
  return VAQHIP_OK;
}
// vaqhip_index_set_lut_quantization with the index locked and its device current (the learnt forms end with it)
int set_quantization_locked(vaqhip_index *ix, const float *off, const float *scale) {
  for (int s = 0; s < ix->M; s++)
    if (!std::isfinite(off[s]) || !std::isfinite(scale[s]) || !(scale[s] > 0.0f))
      return fail(VAQHIP_EINVAL, "subspace %d: offset %g, scale %g (finite, scale > 0)", s, off[s], scale[s]);
  HIP_TRY(ix->d_fast_off.ensure((size_t)ix->M * sizeof(float)));
  HIP_TRY(ix->d_fast_scale.ensure((size_t)ix->M * sizeof(float)));
  WS_SCOPE(ws, ix, ix->stream);  // (a search on another stream may still read them)
  HIP_TRY(hipMemcpyAsync(ix->d_fast_off.p, off, (size_t)ix->M * sizeof(float), hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipMemcpyAsync(ix->d_fast_scale.p, scale, (size_t)ix->M * sizeof(float), hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->fast_off.assign(off, off + ix->M);
  ix->fast_scale.assign(scale, scale + ix->M);
  ix->fast_q = true;
  return ws.finish();
}
} // namespace vaqhost

namespace {
// the tables of n (projected) queries as smallQuantize leaves them: w_fast_small [n][M][16]
int fast_small_luts(vaqhip_index *ix, const float *qp, int n, hipStream_t st) {
  const int ksub = 1 << ix->max_bits;
  HIP_TRY(vaq::launch_lut_build(qp, n, ix->D, ix->M, ix->L, ix->d_sub.as<vaq::SubDesc>(), ix->d_cent_t.as<float>(),
                                ix->lut_floats, ksub, ix->w_lut.as<float>(), st, 1 << ix->min_bits));
  HIP_TRY(vaq::launch_lut_expand(ix->w_lut.as<float>(), n, ix->M, ix->d_sub.as<vaq::SubDesc>(), ix->lut_floats, ksub,
                                 ix->w_lutref.as<float>(), st));
  HIP_TRY(vaq::launch_fast_quantize(ix->w_lutref.as<float>(), n, ix->M, ksub, ix->d_fast_off.as<float>(),
                                    ix->d_fast_scale.as<float>(), ix->w_fast_small.as<uint8_t>(), st));
  return VAQHIP_OK;
}

// the image for the first FAST search after the codes or the method changed: the rows in original order
// are recovered from the packed codes (the append path's unpack) and packed once
int fast_codes_ensure(vaqhip_index *ix, hipStream_t st) {
  if (ix->fast_rows == ix->N) return VAQHIP_OK;
  DevBuf rows;
  HIP_TRY(rows.ensure(std::max<size_t>((size_t)ix->N * ix->M * sizeof(uint16_t), 16)));
  if (ix->N > 0)
    HIP_TRY(vaq::launch_unpack_codes(ix->d_codes.as<uint32_t>(), ix->N, ix->M, ix->layout, ix->W,
                                     ix->d_sub.as<vaq::SubDesc>(), ix->d_perm.as<uint32_t>(), rows.as<uint16_t>(), st));
  return fast_codes_update(ix, rows.as<uint16_t>(), 0, ix->N, st);  // synchronises: `rows` is freed on return
}

// utils/Math.hpp:190-213 on an ascending column (learn_plan.h has the body, shared with the device forms)
float percentile_sorted(const float *v, int64_t rows, float percent) {
  return vaq::learn::percentile_at([v](int64_t i) { return v[i]; }, rows, percent);
}
} // namespace

// One shard's part of a sharded FAST search (vaqhip_internal_search_fast_shard_device): the shard's first
// head_rows rows belong to the head of the whole index (positions head_at.. of its kk_all); their distances go
// to d_head [nq][kk_all], the other rows are ranked by (dist, row)
struct vaqhost::FastShardPart {
  int head_rows, head_at, kk_all;
  uint16_t *d_head;
};

// VAQ::searchFast for nq queries (device pointers): per chunk of queries, tables -> uint8 tables -> every
// row's distance (matrix cores) -> std::sort of rows < k -> the k best by (dist, seq)
int vaqhost::search_fast(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected, int32_t *d_labels,
                float *d_dist, hipStream_t st, const FastShardPart *part) {
  const char *method_err = nullptr;
  if (ix->ti_T > 0) method_err = "the rows are grouped by TI cluster: the method must include TI";
  else if (!ix->fast_q) method_err = "method FAST needs vaqhip_index_set_lut_quantization or vaqhip_learn_quantization first";
  if (int rc = check_search_args(ix, d_queries, nq, k, d_labels, d_dist, method_err)) return rc;
  if (nq == 0) return VAQHIP_OK;
  WS_SCOPE(ws, ix, st);
  if (int rc = fast_codes_ensure(ix, st)) return rc;
  const int64_t N = ix->N;
  const int64_t n_pad = std::max<int64_t>(1, (N + vaq::FAST_ROW_PAD - 1) / vaq::FAST_ROW_PAD) * vaq::FAST_ROW_PAD;
  const int kk = (int)std::min<int64_t>(k, N);
  // the distance matrix of a chunk stays within 1 GiB
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nq, (int64_t)QUERY_CHUNK, ((int64_t)1 << 29) / n_pad}));
  const bool do_project = !projected && ix->has_eig;
  if (do_project) HIP_TRY(ix->w_qproj.ensure((size_t)chunk * ix->D * sizeof(float)));
  HIP_TRY(ix->w_lut.ensure((size_t)chunk * ix->lut_floats * sizeof(float)));
  HIP_TRY(ix->w_lutref.ensure((size_t)chunk * ix->M * (1 << ix->max_bits) * sizeof(float)));
  HIP_TRY(ix->w_fast_small.ensure((size_t)chunk * ix->M * 16));
  HIP_TRY(ix->w_fast_dist.ensure((size_t)chunk * n_pad * sizeof(uint16_t)));
  if (!part) {
    HIP_TRY(ix->w_fast_order.ensure((size_t)chunk * std::max(kk, 1) * sizeof(uint16_t)));
    HIP_TRY(ix->w_fast_scratch.ensure((size_t)chunk * std::max(kk, 1) * sizeof(uint32_t)));
  }
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    const float *qp = d_queries + (size_t)q0 * ix->D;
    if (do_project) {
      HIP_TRY(vaq::launch_project(qp, n, ix->D, ix->d_eig.as<float>(), ix->w_qproj.as<float>(), st));
      qp = ix->w_qproj.as<float>();
    }
    if (int rc = fast_small_luts(ix, qp, n, st)) return rc;
    if (N > 0)
      HIP_TRY(vaq::launch_fast_scan(ix->d_fast_codes.as<uint32_t>(), n_pad, ix->M, ix->w_fast_small.as<uint8_t>(), n,
                                    ix->w_fast_dist.as<uint16_t>(), ix->n_cu, st));
    if (part) {
      // the head is sorted where all of it is known (shard 0, after the exchange), not here
      HIP_TRY(vaq::launch_fast_head_copy(ix->w_fast_dist.as<uint16_t>(), n_pad, n, part->head_rows,
                                         part->d_head + (size_t)q0 * part->kk_all + part->head_at, part->kk_all, st));
      HIP_TRY(vaq::launch_fast_select_tail(ix->w_fast_dist.as<uint16_t>(), n_pad, N, part->head_rows, n, k, ix->M,
                                           ix->id_base, d_labels + (size_t)q0 * k, d_dist + (size_t)q0 * k, st));
      continue;
    }
    if (N > 0)
      HIP_TRY(vaq::launch_fast_head_sort(ix->w_fast_dist.as<uint16_t>(), n_pad, n, kk, ix->w_fast_scratch.as<uint32_t>(),
                                         ix->w_fast_order.as<uint16_t>(), st));
    HIP_TRY(vaq::launch_fast_select(ix->w_fast_dist.as<uint16_t>(), n_pad, N, n, k, ix->M, ix->w_fast_order.as<uint16_t>(),
                                    ix->id_base, d_labels + (size_t)q0 * k, d_dist + (size_t)q0 * k, st));
  }
  return ws.finish();
}

extern "C" {
int vaqhip_index_set_lut_quantization(vaqhip_index *ix, const float *offsets, const float *scale) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (!offsets || !scale) return fail(VAQHIP_EINVAL, "null pointer");
  if (!ix->fast_ok) return fail(VAQHIP_EUNSUPPORTED, "FAST needs max bits per subspace <= 4 and the grouped row sum");
  ENTRY(ix);
  return set_quantization_locked(ix, offsets, scale);
}

int vaqhip_learn_quantization(vaqhip_index *ix, const float *X, int64_t n, int projected, float sample_ratio,
                              float *offsets_out, float *scale_out) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (n <= 0 || !X) return fail(VAQHIP_EINVAL, "bad X / n");
  if (!ix->fast_ok) return fail(VAQHIP_EUNSUPPORTED, "FAST needs max bits per subspace <= 4 and the grouped row sum");
  if (n > 0x7fffffffLL) return fail(VAQHIP_ERANGE, "the reference's rows are int: n = %lld", (long long)n);
  const int sample = static_cast<int>(sample_ratio * (float)n);  // VAQ.cpp:1120
  if (!(sample >= 1)) return fail(VAQHIP_EINVAL, "sampleSize = int(%g * %lld) < 1", sample_ratio, (long long)n);
  ENTRY(ix);
  // randomPermutation (utils/Random.hpp:18-28): i2 = i + mt() % (n - i)
  std::vector<int> perm((size_t)n);
  for (int64_t i = 0; i < n; i++) perm[i] = (int)i;
  {
    std::mt19937 mt(13517106u);
    for (int64_t i = 0; i + 1 < n; i++) {
      const int i2 = (int)i + (int)(mt() % (unsigned)(int)(n - i));
      std::swap(perm[i], perm[i2]);
    }
  }
  // the sampled rows' zero-padded tables (CreateLUT), sample x [M][ksub]: projecting only them is the
  // same as projecting XTrain (row-wise)
  const int M = ix->M, D = ix->D, ksub = 1 << ix->max_bits;
  const int64_t rows = (int64_t)sample * ksub;  // rows of the reference's `luts`
  std::vector<float> luts((size_t)sample * M * ksub);
  {
    const int chunk = std::min(sample, 16384);
    std::vector<float> xs((size_t)chunk * D);
    HIP_TRY(ix->w_q.ensure((size_t)chunk * D * sizeof(float)));
    HIP_TRY(ix->w_qproj.ensure((size_t)chunk * D * sizeof(float)));
    HIP_TRY(ix->w_lut.ensure((size_t)chunk * ix->lut_floats * sizeof(float)));
    HIP_TRY(ix->w_lutref.ensure((size_t)chunk * M * ksub * sizeof(float)));
    hipStream_t st = ix->stream;
    WS_SCOPE(ws, ix, st);
    for (int i0 = 0; i0 < sample; i0 += chunk) {
      const int m = std::min(chunk, sample - i0);
      for (int i = 0; i < m; i++) std::memcpy(&xs[(size_t)i * D], X + (size_t)perm[i0 + i] * D, (size_t)D * sizeof(float));
      HIP_TRY(hipMemcpyAsync(ix->w_q.p, xs.data(), (size_t)m * D * sizeof(float), hipMemcpyHostToDevice, st));
      const float *qp = ix->w_q.as<float>();
      if (!projected && ix->has_eig) {
        HIP_TRY(vaq::launch_project(qp, m, D, ix->d_eig.as<float>(), ix->w_qproj.as<float>(), st));
        qp = ix->w_qproj.as<float>();
      }
      HIP_TRY(vaq::launch_lut_build(qp, m, D, M, ix->L, ix->d_sub.as<vaq::SubDesc>(), ix->d_cent_t.as<float>(),
                                    ix->lut_floats, ksub, ix->w_lut.as<float>(), st, 1 << ix->min_bits));
      HIP_TRY(vaq::launch_lut_expand(ix->w_lut.as<float>(), m, M, ix->d_sub.as<vaq::SubDesc>(), ix->lut_floats, ksub,
                                     ix->w_lutref.as<float>(), st));
      HIP_TRY(hipMemcpyAsync(&luts[(size_t)i0 * M * ksub], ix->w_lutref.p, (size_t)m * M * ksub * sizeof(float),
                             hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    if (int rc = ws.finish()) return rc;
  }
  // per column s: its values sorted once; max(x - f, 0) is monotone, so the offset column's order
  // statistics are those of the sorted column shifted.  Loss per (alpha, column) in double.
  static const float alphas[7] = {.001f, .002f, .005f, .01f, .02f, .05f, .1f};
  std::vector<float> floors(7 * (size_t)M), scales(7 * (size_t)M);
  std::vector<double> loss(7 * (size_t)M);
  auto column = [&](int s) {
    std::vector<float> col((size_t)rows), sorted((size_t)rows), offc((size_t)rows);
    for (int64_t i = 0; i < sample; i++)
      for (int c = 0; c < ksub; c++) col[(size_t)(i * ksub + c)] = luts[((size_t)i * M + s) * ksub + c];
    sorted = col;
    std::sort(sorted.begin(), sorted.end());
    for (int a = 0; a < 7; a++) {
      const float fl = percentile_sorted(sorted.data(), rows, alphas[a]);
      for (int64_t i = 0; i < rows; i++) offc[(size_t)i] = std::max(sorted[(size_t)i] - fl, 0.0f);
      const float ceil = percentile_sorted(offc.data(), rows, 1.0f - alphas[a]);
      const float sc = 255.0f / ceil;
      double l = 0.0;
      for (int64_t i = 0; i < rows; i++) {
        const float x = col[(size_t)i];
        const float off = std::max(x - fl, 0.0f);
        const float qv = std::min(std::floor(off * sc), 255.0f);
        const float quant = (float)(uint8_t)qv;
        const float ideal = ((x - off) * sc) - quant;  // VAQ.cpp:1171-1176, as written
        l += (double)(ideal * ideal);
      }
      floors[(size_t)a * M + s] = fl;
      scales[(size_t)a * M + s] = sc;
      loss[(size_t)a * M + s] = l;
    }
  };
  {
    const int nth = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (int t = 0; t < nth; t++)
      pool.emplace_back([&, t] { for (int s = t; s < M; s += nth) column(s); });
    for (auto &th : pool) th.join();
  }
  double best = (double)std::numeric_limits<float>::max();
  int best_a = -1;
  for (int a = 0; a < 7; a++) {
    double l = 0.0;
    for (int s = 0; s < M; s++) l += loss[(size_t)a * M + s];
    if (l <= best) {
      best = l;
      best_a = a;
    }
  }
  if (best_a < 0) return fail(VAQHIP_EINVAL, "no alpha gives a finite quantisation loss");
  const float *off = &floors[(size_t)best_a * M], *sc = &scales[(size_t)best_a * M];
  if (int rc = set_quantization_locked(ix, off, sc)) return rc;
  if (offsets_out) std::memcpy(offsets_out, off, (size_t)M * sizeof(float));
  if (scale_out) std::memcpy(scale_out, sc, (size_t)M * sizeof(float));
  return VAQHIP_OK;
}

int vaqhip_build_small_lut(vaqhip_index *ix, const float *queries, int nq, int projected, uint8_t *out) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (nq < 0 || (nq > 0 && (!queries || !out))) return fail(VAQHIP_EINVAL, "bad arguments");
  if (!ix->fast_ok) return fail(VAQHIP_EUNSUPPORTED, "FAST needs max bits per subspace <= 4 and the grouped row sum");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->fast_q) return fail(VAQHIP_ESTATE, "no LUT quantisation set");
  if (nq == 0) return VAQHIP_OK;
  DeviceGuard g(ix->device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", ix->device);
  const int chunk = std::min(nq, 16384);
  HIP_TRY(ix->w_q.ensure((size_t)chunk * ix->D * sizeof(float)));
  HIP_TRY(ix->w_qproj.ensure((size_t)chunk * ix->D * sizeof(float)));
  HIP_TRY(ix->w_lut.ensure((size_t)chunk * ix->lut_floats * sizeof(float)));
  HIP_TRY(ix->w_lutref.ensure((size_t)chunk * ix->M * (1 << ix->max_bits) * sizeof(float)));
  HIP_TRY(ix->w_fast_small.ensure((size_t)chunk * ix->M * 16));
  hipStream_t st = ix->stream;
  WS_SCOPE(ws, ix, st);
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    HIP_TRY(hipMemcpyAsync(ix->w_q.p, queries + (size_t)q0 * ix->D, (size_t)n * ix->D * sizeof(float),
                           hipMemcpyHostToDevice, st));
    const float *qp = ix->w_q.as<float>();
    if (!projected && ix->has_eig) {
      HIP_TRY(vaq::launch_project(qp, n, ix->D, ix->d_eig.as<float>(), ix->w_qproj.as<float>(), st));
      qp = ix->w_qproj.as<float>();
    }
    if (int rc = fast_small_luts(ix, qp, n, st)) return rc;
    HIP_TRY(hipMemcpyAsync(out + (size_t)q0 * ix->M * 16, ix->w_fast_small.p, (size_t)n * ix->M * 16,
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return ws.finish();
}

int vaqhip_merge_fast_device(int device_id, const uint16_t *d_head_dist, int64_t head_stride, int n_head,
                             int64_t head_label_base, const float *d_dist_lists, const int32_t *d_label_lists,
                             int n_lists, int64_t list_stride, int64_t query_stride, int nq, int k,
                             int32_t *d_labels_out, float *d_dist_out, void *stream) {
  if (n_lists < 0 || nq < 0 || k <= 0 || n_head < 0) return fail(VAQHIP_EINVAL, "bad sizes");
  if (k > VAQHIP_MAX_K) return fail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  if (n_lists > vaq::FAST_MAX_LISTS) return fail(VAQHIP_EUNSUPPORTED, "at most %d lists per merge", vaq::FAST_MAX_LISTS);
  if (n_head > k) return fail(VAQHIP_EINVAL, "n_head=%d > k=%d: the head is the first min(k, N) rows", n_head, k);
  if (list_stride < 0 || query_stride < 0 || head_stride < 0 || (n_head > 0 && head_stride < n_head))
    return fail(VAQHIP_EINVAL, "bad stride");
  if (head_label_base < 0 || head_label_base + n_head > 0x7fffffffLL) return fail(VAQHIP_ERANGE, "head labels past 2^31");
  if ((n_lists > 0 && (!d_dist_lists || !d_label_lists)) || (n_head > 0 && !d_head_dist) || !d_labels_out || !d_dist_out)
    return fail(VAQHIP_EINVAL, "null pointer");
  if (nq == 0) return VAQHIP_OK;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", device_id);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // every query's output rows serve its head sort first: the items in the label row (n_head <= k words), the
  // order in the distance row; the merge reads the items whole before it writes
  uint32_t *items = reinterpret_cast<uint32_t *>(d_labels_out);
  HIP_TRY(vaq::launch_fast_head_sort_strided(d_head_dist, head_stride, nq, n_head, items, k,
                                             reinterpret_cast<uint16_t *>(d_dist_out), 2 * (int64_t)k, st));
  HIP_TRY(vaq::launch_fast_merge(items, k, n_head, head_label_base, d_dist_lists, d_label_lists, n_lists, list_stride,
                                 query_stride, nq, k, d_labels_out, d_dist_out, st));
  return VAQHIP_OK;
}

// ---- FAST across the shards of a multi-device index (vaqhip_internal.h) ----
int vaqhip_internal_fast_in_force(vaqhip_index *ix) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lk(ix->mu);
  return fast_only(ix) ? 1 : 0;
}

int vaqhip_internal_search_fast_shard_device(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                                             int64_t row_offset, int kk, int32_t *d_labels, float *d_dist,
                                             uint16_t *d_head, void *stream) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (row_offset < 0 || kk < 0 || kk > k || (kk > 0 && !d_head)) return fail(VAQHIP_EINVAL, "bad head description");
  ENTRY(ix);
  if (!fast_only(ix)) return fail(VAQHIP_ESTATE, "method FAST is not in force on this shard");
  FastShardPart part;
  part.kk_all = kk;
  part.head_at = (int)std::min<int64_t>(row_offset, kk);
  part.head_rows = (int)std::max<int64_t>(0, std::min<int64_t>(kk - part.head_at, std::max<int64_t>(ix->N, 0)));
  part.d_head = d_head;
  return search_fast(ix, d_queries, nq, k, projected, d_labels, d_dist, static_cast<hipStream_t>(stream), &part);
}

int vaqhip_internal_fast_head_gather_device(int device, const uint16_t *d_planes, int64_t plane_stride, int n_parts,
                                            const int *start, int nq, int kk, uint16_t *d_head, void *stream) {
  if (n_parts < 1 || n_parts > vaq::FAST_MAX_LISTS || !start || nq < 0 || kk < 0 || plane_stride < 0)
    return fail(VAQHIP_EINVAL, "bad arguments");
  if (nq == 0 || kk == 0) return VAQHIP_OK;
  if (!d_planes || !d_head) return fail(VAQHIP_EINVAL, "null pointer");
  vaq::FastHeadParts parts;
  parts.n_parts = n_parts;
  for (int g = 0; g <= vaq::FAST_MAX_LISTS; g++) parts.start[g] = start[std::min(g, n_parts)];
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", device);
  HIP_TRY(vaq::launch_fast_head_gather(d_planes, plane_stride, parts, nq, kk, d_head, static_cast<hipStream_t>(stream)));
  return VAQHIP_OK;
}
} // extern "C"
