// vaqhip_codes.cpp -- the rows of the single-device index: upload, bucketed (or TI-grouped) order,
// packing, append, TI clustering (the regrouping, and the k-means that makes the centres).
#include "vaqhip_index.h"

#include "kmeans_sample.h"
#include "vaq_codes.h"
#include "vaq_kmeans.h"
#include "vaq_ti.h"

#include <chrono>
#include <cmath>

using namespace vaqhost;

namespace {
constexpr int64_t BUCKET_MIN_ROWS = 900;       // average rows per bucket the bucketed order aims for
constexpr int64_t BUCKET_MIN_ROWS_10 = 1900;   // ... before it takes a tenth key bit
constexpr int64_t UPLOAD_CHUNK_ROWS = 1 << 22; // rows per host->device staging chunk

// Order the N rows of the device matrix d_u16 (CodebookType layout) -- by first code, or by TI
// cluster when clusters are set -- and pack them.  Synchronises the stream.
int build_rows(vaqhip_index *ix, const uint16_t *d_u16, int64_t N, hipStream_t st) {
  const int step = vaq::scan_wg_step_rows(ix->layout, ix->M);
  const int64_t padded = std::max<int64_t>(step, ((N + step - 1) / step) * step);
  const int64_t words = vaq::packed_words(padded, ix->M, ix->layout, ix->W);
  // (behind the padded rows: what the best-first form's last wave step may read, never use -- not written)
  HIP_TRY(ix->d_codes.ensure((size_t)(words + vaq::scan_bf_slack_words(ix->layout, ix->M)) * sizeof(uint32_t)));
  const vaq::SubDesc *dsub = ix->d_sub.as<vaq::SubDesc>();
  int shift = 0, bt = 0, K0 = 1, fine = 0;
  if (ix->ti_T > 0) {
    K0 = ix->ti_T;
  } else {
    // bucket key = the top bits of the first code, continued -- when the whole first code is
    // used up -- by up to 4 top bits of the second: as many key bits as keep ~900 rows per
    // bucket on average, at most 10 (measured on 250M rows x 16 B: 10 bits beat 8, 11 and 12
    // for 2, 32 and 256 queries; the option accepts up to 12); a tenth bit from the second code
    // wants ~1900 rows per bucket (8 B rows, 10 k queries, best-first form: 1M rows 0.86 / 0.75 /
    // 0.83 ms with 8 / 9 / 10 bits, 2M 1.41 / 1.11 / 1.09, 8M 4.98 / 3.36 / 2.96), one from the
    // first code does not (12-bit first code, 1M rows: 1.54 ms with 10 bits, 1.83 with 9)
    int want = 4;
    while (want < 10 && ((int64_t)2 << want) * BUCKET_MIN_ROWS <= std::max<int64_t>(N, 1)) want++;
    if (ix->opt_bucket_bits > 0) want = ix->opt_bucket_bits;
    const int kb = std::min(want, ix->bits[0]);
    shift = ix->bits[0] - kb;
    // Continuing into the second code: always where the best-first form will scan the rows (its
    // per-bucket bookkeeping is a key in LDS), else only on large databases -- 250M rows, 32
    // queries: 4.0 vs 5.3 ms, but 1M rows, 10 bits, shared-stream form: 2.0 vs 1.45 ms; an
    // explicit "bucket_bits" option is obeyed as given
    if (shift == 0 && ix->M > 1) {
      int want_c = want;  // (a tenth bit taken from the SECOND code wants more rows per bucket)
      if (want_c == 10 && kb < 10 && ix->opt_bucket_bits <= 0 && N < (int64_t)1024 * BUCKET_MIN_ROWS_10) want_c = 9;
      const int cont = std::min(std::min(want_c - kb, 4), ix->bits[1]);
      const bool bf_form = ix->opt_bf && cont > 0 &&
                           vaq::scan_bf_supported(ix->layout, ix->M, 1, vaq::EA_QUEUE, 1 << (kb + cont), ix->seq);
      if (N >= ((int64_t)1 << 24) || ix->opt_bucket_bits > 0 || bf_form) bt = std::max(cont, 0);
    }
    K0 = 1 << (kb + bt);
  }
  HIP_TRY(ix->d_bstart.ensure((size_t)(K0 + 1) * sizeof(int)));
  HIP_TRY(ix->d_perm.ensure(std::max<size_t>((size_t)N, 1) * sizeof(uint32_t)));
  if (ix->ti_T > 0) HIP_TRY(ix->d_ti_xcc.ensure(std::max<size_t>((size_t)padded, 1) * sizeof(float)));
  std::vector<int> bstart((size_t)K0 + 1, (int)N);
  if (N == 0) {
    HIP_TRY(hipMemsetAsync(ix->d_codes.p, 0, (size_t)words * sizeof(uint32_t), st));
  } else {
    if (ix->ti_T > 0)
      HIP_TRY(vaq::ti_group_rows(d_u16, N, ix->M, ix->L, ix->ti_seg, dsub, ix->d_cent.as<float>(),
                                 ix->d_ti_clusters.as<float>(), ix->ti_T, ix->d_perm.as<uint32_t>(),
                                 ix->d_bstart.as<int>(), ix->d_ti_xcc.as<float>(), st));
    else {
      // (byte codes keyed by the whole first code: order each bucket by the rest of the second code)
      fine = (ix->layout == vaq::LAYOUT_BYTES && shift == 0 && ix->M > 1 && ix->opt_sub_order) ? ix->bits[1] - bt : 0;
      if (fine > 0) HIP_TRY(ix->d_substart.ensure((((size_t)K0 << fine) + 1) * sizeof(int)));
      HIP_TRY(vaq::sort_by_first_code(d_u16, N, ix->M, ix->bits[0], shift, ix->M > 1 ? ix->bits[1] : 0, bt,
                                      ix->d_perm.as<uint32_t>(), ix->d_bstart.as<int>(), st, fine,
                                      fine > 0 ? ix->d_substart.as<int>() : nullptr));
      if (fine > 0) {
        std::vector<int> ss(((size_t)K0 << fine) + 1);
        HIP_TRY(hipMemcpy(ss.data(), ix->d_substart.p, ss.size() * sizeof(int), hipMemcpyDeviceToHost));
        ss[ss.size() - 1] = (int)N;
        for (int64_t f = (int64_t)ss.size() - 2; f >= 0; f--)
          if (ss[f] < 0) ss[f] = ss[f + 1];  // runs that do not occur: empty
        HIP_TRY(hipMemcpy(ix->d_substart.p, ss.data(), ss.size() * sizeof(int), hipMemcpyHostToDevice));
      }
    }
    HIP_TRY(hipMemcpy(bstart.data(), ix->d_bstart.p, (size_t)(K0 + 1) * sizeof(int), hipMemcpyDeviceToHost));
    bstart[K0] = (int)N;
    for (int b = K0 - 1; b >= 0; b--)
      if (bstart[b] < 0) bstart[b] = bstart[b + 1];  // codes / clusters that do not occur: empty
    HIP_TRY(vaq::launch_pack_codes(d_u16, 0, N, padded, ix->M, ix->layout, ix->W, dsub,
                                   ix->d_perm.as<uint32_t>(), ix->d_codes.as<uint32_t>(), st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  HIP_TRY(hipMemcpy(ix->d_bstart.p, bstart.data(), (size_t)(K0 + 1) * sizeof(int), hipMemcpyHostToDevice));
  ix->N = N;
  ix->N_keyed = N;
  ix->bucket_shift = shift;
  ix->bucket_t = bt;
  ix->n_buckets = K0;
  ix->sub_fine = N > 0 ? fine : 0;
  ix->inv_valid = false;
  ix->ti_walk_valid = false;  // (set / add codes, set_ti_clusters and cluster_ti_kmeans all regroup here)
  return VAQHIP_OK;
}

int set_codes_common(vaqhip_index *ix, const uint16_t *codes, bool on_device, int64_t N,
                            int64_t id_base, hipStream_t st) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (N < 0 || (N > 0 && !codes)) return fail(VAQHIP_EINVAL, "bad codes/N");
  if (id_base < 0) return fail(VAQHIP_EINVAL, "id_base < 0");
  if (N > 0x7fffffffLL - 1 || id_base + N > 0x7fffffffLL)
    return fail(VAQHIP_ERANGE, "labels are 32-bit ints (utils/Types.hpp:100): id_base+N = %lld",
                (long long)(id_base + N));
  ENTRY(ix);
  // all rows must be resident to sort them: stage a host matrix on the device first
  DevBuf staged;
  const uint16_t *d_u16 = codes;
  if (!on_device && N > 0) {
    HIP_TRY(staged.ensure((size_t)N * ix->M * sizeof(uint16_t)));
    for (int64_t r = 0; r < N; r += UPLOAD_CHUNK_ROWS) {
      const int64_t e = std::min(N, r + UPLOAD_CHUNK_ROWS);
      HIP_TRY(hipMemcpyAsync(staged.as<uint16_t>() + r * ix->M, codes + r * ix->M,
                             (size_t)(e - r) * ix->M * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    }
    d_u16 = staged.as<uint16_t>();
  }
  // (a search enqueued on another stream may still be scanning the rows this call rewrites)
  WS_SCOPE(ws, ix, st);
  if (int rc = fast_codes_update(ix, d_u16, 0, N, st)) return rc;
  if (int rc = build_rows(ix, d_u16, N, st)) return rc;  // synchronises: `staged` is freed on return
  ix->id_base = id_base;
  return ws.finish();
}

// append to a bucketed (non-TI) index: sort and pack the NEW rows only, then merge them into the
// existing order bucket by bucket (launch_merge_rows).  O(N) bytes are copied once -- the packed
// rows and their labels -- but nothing is unpacked and nothing is re-sorted; temporaries are
// O(n_new) plus the new packed buffer.
int append_rows_bucketed(vaqhip_index *ix, const uint16_t *d_new, int64_t n_new, hipStream_t st) {
  const int64_t n_old = ix->N, N = n_old + n_new;
  // (rows ordered inside the buckets too: merge run by run, so that the order survives -- the runs
  //  are the buckets of a finer key, ix->d_substart their starts)
  const int fine = ix->sub_fine;
  const int KB = ix->n_buckets;
  const int K0 = KB << fine;
  const int step = vaq::scan_wg_step_rows(ix->layout, ix->M);
  const vaq::SubDesc *dsub = ix->d_sub.as<vaq::SubDesc>();
  // the new rows in bucketed order among themselves
  DevBuf new_perm, new_start, new_bstart, new_codes, out_codes, out_perm;
  HIP_TRY(new_perm.ensure((size_t)n_new * sizeof(uint32_t)));
  HIP_TRY(new_start.ensure((size_t)(K0 + 1) * sizeof(int)));
  HIP_TRY(new_bstart.ensure((size_t)(KB + 1) * sizeof(int)));
  HIP_TRY(vaq::sort_by_first_code(d_new, n_new, ix->M, ix->bits[0], ix->bucket_shift, ix->M > 1 ? ix->bits[1] : 0,
                                  ix->bucket_t, new_perm.as<uint32_t>(), fine > 0 ? new_bstart.as<int>() : new_start.as<int>(), st,
                                  fine, fine > 0 ? new_start.as<int>() : nullptr));
  std::vector<int> ns((size_t)K0 + 1), os((size_t)K0 + 1), ts((size_t)K0 + 1);
  HIP_TRY(hipMemcpy(ns.data(), new_start.p, (size_t)(K0 + 1) * sizeof(int), hipMemcpyDeviceToHost));
  ns[K0] = (int)n_new;
  for (int b = K0 - 1; b >= 0; b--)
    if (ns[b] < 0) ns[b] = ns[b + 1];
  HIP_TRY(hipMemcpy(new_start.p, ns.data(), (size_t)(K0 + 1) * sizeof(int), hipMemcpyHostToDevice));
  const int *d_old_start = fine > 0 ? ix->d_substart.as<int>() : ix->d_bstart.as<int>();
  HIP_TRY(hipMemcpy(os.data(), d_old_start, (size_t)(K0 + 1) * sizeof(int), hipMemcpyDeviceToHost));
  const int64_t new_padded = std::max<int64_t>(step, ((n_new + step - 1) / step) * step);
  HIP_TRY(new_codes.ensure((size_t)vaq::packed_words(new_padded, ix->M, ix->layout, ix->W) * sizeof(uint32_t)));
  HIP_TRY(vaq::launch_pack_codes(d_new, 0, n_new, new_padded, ix->M, ix->layout, ix->W, dsub, new_perm.as<uint32_t>(),
                                 new_codes.as<uint32_t>(), st));
  // the merged buffers
  const int64_t padded = std::max<int64_t>(step, ((N + step - 1) / step) * step);
  const int64_t words = vaq::packed_words(padded, ix->M, ix->layout, ix->W);
  HIP_TRY(out_codes.ensure((size_t)(words + vaq::scan_bf_slack_words(ix->layout, ix->M)) * sizeof(uint32_t)));
  HIP_TRY(out_perm.ensure((size_t)N * sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(out_codes.p, 0, (size_t)words * sizeof(uint32_t), st));  // (the padding rows must be zero)
  HIP_TRY(vaq::launch_merge_rows(ix->d_codes.as<uint32_t>(), ix->d_perm.as<uint32_t>(), d_old_start,
                                 new_codes.as<uint32_t>(), new_perm.as<uint32_t>(), new_start.as<int>(), K0, n_old, N,
                                 ix->M, ix->layout, ix->W, out_codes.as<uint32_t>(), out_perm.as<uint32_t>(), st));
  for (int b = 0; b <= K0; b++) ts[b] = os[b] + ns[b];
  HIP_TRY(hipStreamSynchronize(st));
  std::swap(ix->d_codes.p, out_codes.p);
  std::swap(ix->d_codes.cap, out_codes.cap);
  std::swap(ix->d_perm.p, out_perm.p);
  std::swap(ix->d_perm.cap, out_perm.cap);
  if (fine > 0) {
    HIP_TRY(hipMemcpy(ix->d_substart.p, ts.data(), (size_t)(K0 + 1) * sizeof(int), hipMemcpyHostToDevice));
    std::vector<int> tb((size_t)KB + 1);
    for (int b = 0; b <= KB; b++) tb[b] = ts[(size_t)b << fine];
    HIP_TRY(hipMemcpy(ix->d_bstart.p, tb.data(), (size_t)(KB + 1) * sizeof(int), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(ix->d_bstart.p, ts.data(), (size_t)(K0 + 1) * sizeof(int), hipMemcpyHostToDevice));
  }
  ix->N = N;
  ix->inv_valid = false;
  return VAQHIP_OK;
}

// append: a bucketed index merges the new rows in (above); a TI-grouped index (rows ordered by
// cluster and distance to the centre) and an empty index are rebuilt: recover the rows already
// packed (original order), put the new ones behind them, regroup everything
int add_codes_common(vaqhip_index *ix, const uint16_t *codes, bool on_device, int64_t n_new,
                            hipStream_t st) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (n_new < 0 || (n_new > 0 && !codes)) return fail(VAQHIP_EINVAL, "bad codes/N");
  std::lock_guard<std::mutex> lk(ix->mu);
  const int64_t n_old = ix->N < 0 ? 0 : ix->N;
  const int64_t N = n_old + n_new;
  if (N > 0x7fffffffLL - 1 || ix->id_base + N > 0x7fffffffLL)
    return fail(VAQHIP_ERANGE, "labels are 32-bit ints (utils/Types.hpp:100): id_base+N = %lld",
                (long long)(ix->id_base + N));
  DeviceGuard g(ix->device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", ix->device);
  if (n_new == 0 && ix->N >= 0) return VAQHIP_OK;
  WS_SCOPE(ws, ix, st);  // (a search on another stream may still be reading the codes)
  if (ix->ti_T == 0 && n_old > 0 && n_new > 0 && N < 4 * std::max<int64_t>(ix->N_keyed, 4096)) {
    DevBuf staged;
    const uint16_t *d_new = codes;
    if (!on_device) {
      HIP_TRY(staged.ensure((size_t)n_new * ix->M * sizeof(uint16_t)));
      HIP_TRY(hipMemcpyAsync(staged.p, codes, (size_t)n_new * ix->M * sizeof(uint16_t), hipMemcpyHostToDevice, st));
      d_new = staged.as<uint16_t>();
    }
    if (int rc = fast_codes_update(ix, d_new, n_old, N, st)) return rc;
    if (int rc = append_rows_bucketed(ix, d_new, n_new, st)) return rc;  // synchronises
    return ws.finish();
  }
  DevBuf rows;
  HIP_TRY(rows.ensure(std::max<size_t>((size_t)N * ix->M * sizeof(uint16_t), 16)));
  if (n_old > 0)
    HIP_TRY(vaq::launch_unpack_codes(ix->d_codes.as<uint32_t>(), n_old, ix->M, ix->layout, ix->W,
                                     ix->d_sub.as<vaq::SubDesc>(), ix->d_perm.as<uint32_t>(),
                                     rows.as<uint16_t>(), st));
  if (n_new > 0)
    HIP_TRY(hipMemcpyAsync(rows.as<uint16_t>() + n_old * ix->M, codes, (size_t)n_new * ix->M * sizeof(uint16_t),
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (int rc = fast_codes_update(ix, rows.as<uint16_t>() + n_old * ix->M, n_old, N, st)) return rc;
  if (int rc = build_rows(ix, rows.as<uint16_t>(), N, st)) return rc;  // synchronises
  return ws.finish();
}
// what set_ti_clusters and cluster_ti_kmeans refuse alike (T > 0)
int check_ti_shape(const vaqhip_index *ix, int T, int seg_num) {
  if (T > VAQHIP_MAX_TI_CLUSTERS)
    return fail(VAQHIP_EUNSUPPORTED, "T=%d > %d clusters", T, VAQHIP_MAX_TI_CLUSTERS);
  if (T > 0 && (seg_num < 1 || seg_num > ix->M))
    return fail(VAQHIP_EINVAL, "seg_num=%d outside 1..%d", seg_num, ix->M);
  if (T > 0 && (int64_t)seg_num * ix->L > 1024)
    return fail(VAQHIP_EUNSUPPORTED, "TI centres of %d dims (> 1024)", seg_num * ix->L);
  if (T > 0 && ix->seq) return fail(VAQHIP_EINVAL, "TI is a VAQ::search method, not a queryLUT one");
  return VAQHIP_OK;
}

// vaqhip_index_set_ti_clusters under the index's lock, arguments checked
int set_ti_clusters_locked(vaqhip_index *ix, const float *clusters, int T, int seg_num) {
  if (T == 0 && ix->ti_T == 0) return VAQHIP_OK;
  hipStream_t st = ix->stream;
  // (a search enqueued on another stream may still be scanning the rows this call regroups)
  WS_SCOPE(ws, ix, st);
  // rows already handed over: recover them in original order, then regroup
  DevBuf rows;
  if (ix->N > 0) {
    HIP_TRY(rows.ensure((size_t)ix->N * ix->M * sizeof(uint16_t)));
    HIP_TRY(vaq::launch_unpack_codes(ix->d_codes.as<uint32_t>(), ix->N, ix->M, ix->layout, ix->W,
                                     ix->d_sub.as<vaq::SubDesc>(), ix->d_perm.as<uint32_t>(),
                                     rows.as<uint16_t>(), st));
  }
  if (T > 0) {
    const size_t bytes = (size_t)T * seg_num * ix->L * sizeof(float);
    HIP_TRY(ix->d_ti_clusters.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(ix->d_ti_clusters.p, clusters, bytes, hipMemcpyHostToDevice, st));
    // dimension-major copy for the per-query plan (one centre per lane, coalesced)
    const int dd = seg_num * ix->L;
    std::vector<float> t((size_t)T * dd);
    for (int c = 0; c < T; c++)
      for (int j = 0; j < dd; j++) t[(size_t)j * T + c] = clusters[(size_t)c * dd + j];
    HIP_TRY(ix->d_ti_clusters_t.ensure(bytes));
    HIP_TRY(hipMemcpy(ix->d_ti_clusters_t.p, t.data(), bytes, hipMemcpyHostToDevice));
  }
  ix->ti_T = T;
  ix->ti_seg = T > 0 ? seg_num : 0;
  if (T > 0) ix->methods |= VAQHIP_METHOD_TI;
  else {
    ix->methods &= ~VAQHIP_METHOD_TI;
    if (!ix->methods) ix->methods = VAQHIP_METHOD_HEAP;
  }
  if (ix->N >= 0) {
    if (int rc = build_rows(ix, rows.as<uint16_t>(), ix->N, st)) return rc;
  }
  HIP_TRY(hipStreamSynchronize(st));
  return ws.finish();
}

// what vaqhip_index_cluster_ti_kmeans refuses beyond its plain arguments (T >= 1); under the index's lock
int check_kmeans_state(const vaqhip_index *ix, int T, int seg_num) {
  if (int rc = check_ti_shape(ix, T, seg_num)) return rc;
  if (ix->N < 0) return fail(VAQHIP_ESTATE, "the k-means of clusterTI runs over the codes: set them first");
  if (ix->staged.open)
    return fail(VAQHIP_ESTATE, "a staged search is open on this index: call vaqhip_search_finish_device first");
  return VAQHIP_OK;
}

// the first seg_num codes of the sampled rows (vaq::kmeans_gather_packed), read from the packed rows as they lie
int gather_sample(vaqhip_index *ix, const int *sample_rows, int n_sample, int seg_num, uint16_t *d_scodes,
                  hipStream_t st) {
  HIP_TRY(vaq::kmeans_gather_packed(ix->d_codes.as<uint32_t>(), ix->N, ix->M, ix->layout, ix->W,
                                    ix->d_sub.as<vaq::SubDesc>(), ix->d_perm.as<uint32_t>(), sample_rows, n_sample,
                                    seg_num, d_scodes, st));
  return VAQHIP_OK;
}
} // namespace

extern "C" {
int vaqhip_index_add_codes_u16(vaqhip_index *ix, const uint16_t *codes, int64_t n_new) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  return add_codes_common(ix, codes, false, n_new, ix->stream);
}

int vaqhip_index_add_codes_u16_device(vaqhip_index *ix, const uint16_t *d_codes, int64_t n_new, void *stream) {
  return add_codes_common(ix, d_codes, true, n_new, static_cast<hipStream_t>(stream));
}

int vaqhip_index_set_codes_u16(vaqhip_index *ix, const uint16_t *codes, int64_t N, int64_t id_base) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (int rc = set_codes_common(ix, codes, false, N, id_base, ix->stream)) return rc;
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return VAQHIP_OK;
}

int vaqhip_index_set_codes_u16_device(vaqhip_index *ix, const uint16_t *d_codes, int64_t N,
                                      int64_t id_base, void *stream) {
  return set_codes_common(ix, d_codes, true, N, id_base, static_cast<hipStream_t>(stream));
}

int vaqhip_index_set_ti_clusters(vaqhip_index *ix, const float *clusters, int T, int seg_num) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (T < 0 || (T > 0 && !clusters)) return fail(VAQHIP_EINVAL, "bad clusters/T");
  if (int rc = check_ti_shape(ix, T, seg_num)) return rc;
  ENTRY(ix);
  return set_ti_clusters_locked(ix, clusters, T, seg_num);
}

int vaqhip_index_cluster_ti_kmeans(vaqhip_index *ix, int T, int seg_num, int max_iter, float *clusters_out,
                                   int *iters_out, int *nan_rows_out) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (T < 1 || max_iter < 1) return fail(VAQHIP_EINVAL, "T=%d max_iter=%d", T, max_iter);
  ENTRY(ix);
  if (int rc = check_kmeans_state(ix, T, seg_num)) return rc;
  if (T > ix->N)  // (the sample is min(N, 256 * T) rows: never fewer than T unless N is)
    return fail(VAQHIP_EINVAL, "T=%d centres from %lld rows (the reference reads out of bounds)", T, (long long)ix->N);
  const int64_t N = ix->N;
  const int rows = vaq::kmeans_sample_rows(N, T), dd = seg_num * ix->L;
  std::vector<float> means((size_t)T * dd);
  int iters = 0, no_centre = 0;
  {
    hipStream_t st = ix->stream;
    WS_SCOPE(ws, ix, st);  // (a search enqueued on another stream may still be using the index)
    const auto t0 = std::chrono::steady_clock::now();
    // the sample's first seg_num codes as [rows][seg_num], from the packed rows
    DevBuf scodes, d_means;
    std::vector<int> sample;
    if (N > rows) sample = vaq::permutation_head(N, rows);
    HIP_TRY(scodes.ensure((size_t)rows * seg_num * sizeof(uint16_t)));
    if (int rc = gather_sample(ix, N > rows ? sample.data() : nullptr, rows, seg_num, scodes.as<uint16_t>(), st))
      return rc;
    const std::vector<int> seeds = vaq::permutation_head(rows, T);
    HIP_TRY(d_means.ensure(means.size() * sizeof(float)));
    vaq::KmeansPhases ph;
    const vaq::KmeansDev dev = {ix->device, st, ix->d_sub.as<vaq::SubDesc>(), ix->d_cent.as<float>()};
    HIP_TRY(vaq::kmeans_fit(&dev, 1, scodes.as<uint16_t>(), rows, seg_num, ix->L, seeds.data(), T, max_iter,
                            d_means.as<float>(), &iters, &no_centre, ix->opt_timing ? &ph : nullptr,
                            nullptr));  // synchronises
    HIP_TRY(hipMemcpy(means.data(), d_means.p, means.size() * sizeof(float), hipMemcpyDeviceToHost));
    ix->km_last = vaqhip_kmeans_timing{};
    ix->km_last.total_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ix->km_last.assign_ms = (float)ph.assign_ms;
    ix->km_last.accumulate_ms = (float)ph.accumulate_ms;
    ix->km_last.update_ms = (float)ph.update_ms;
    ix->km_last.iterations = iters;
    ix->km_last.rows = rows;
    ix->km_last.dims = dd;
    ix->km_last.clusters = T;
    if (int rc = ws.finish()) return rc;
  }
  if (no_centre)
    return fail(VAQHIP_EINVAL, "a row is at a distance >= FLT_MAX (or NaN) from every centre: the reference indexes row -1");
  if (clusters_out) std::memcpy(clusters_out, means.data(), means.size() * sizeof(float));
  if (iters_out) *iters_out = iters;
  if (nan_rows_out) *nan_rows_out = vaq::nan_rows(means.data(), T, dd);
  return set_ti_clusters_locked(ix, means.data(), T, seg_num);
}

int vaqhip_internal_kmeans_check(vaqhip_index *ix, int T, int seg_num) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  return check_kmeans_state(ix, T, seg_num);
}

int vaqhip_internal_kmeans_gather(vaqhip_index *ix, const int *sample_rows, int n_sample, int seg_num,
                                  uint16_t *scodes_out) {
  if (!ix || !scodes_out || n_sample < 0) return fail(VAQHIP_EINVAL, "null pointer");
  ENTRY(ix);
  if (int rc = check_kmeans_state(ix, 1, seg_num)) return rc;
  if (sample_rows ? n_sample > ix->N : n_sample != ix->N)
    return fail(VAQHIP_EINVAL, "%d sampled rows of %lld", n_sample, (long long)ix->N);
  for (int i = 0; sample_rows && i < n_sample; i++)
    if (sample_rows[i] < 0 || sample_rows[i] >= ix->N)
      return fail(VAQHIP_EINVAL, "sampled row %d outside the index's %lld rows", sample_rows[i], (long long)ix->N);
  if (n_sample == 0) return VAQHIP_OK;
  hipStream_t st = ix->stream;
  WS_SCOPE(ws, ix, st);  // (a search enqueued on another stream may still be using the index)
  DevBuf scodes;
  const size_t bytes = (size_t)n_sample * seg_num * sizeof(uint16_t);
  HIP_TRY(scodes.ensure(bytes));
  if (int rc = gather_sample(ix, sample_rows, n_sample, seg_num, scodes.as<uint16_t>(), st)) return rc;
  HIP_TRY(hipMemcpyAsync(scodes_out, scodes.p, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ws.finish();
}

int vaqhip_internal_kmeans_tables(vaqhip_index *ix, const void **d_sub, const float **d_cent, int *L) {
  if (!ix || !d_sub || !d_cent || !L) return fail(VAQHIP_EINVAL, "null pointer");
  *d_sub = ix->d_sub.p;
  *d_cent = ix->d_cent.as<float>();
  *L = ix->L;
  return VAQHIP_OK;
}

int vaqhip_last_kmeans_timing(vaqhip_index *ix, vaqhip_kmeans_timing *out) {
  if (!ix || !out) return fail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(ix->mu);
  *out = ix->km_last;
  return VAQHIP_OK;
}
} // extern "C"
