// vaqhip_codebooks.cpp -- host side of the subspace codebook fit of include/vaqhip.h (vaqhip_fit_codebooks*): the
// argument checks, the copies around vaq::codebooks_fit (vaq_codebooks.hip) and the calling thread's timing.  No
// index handle: the centres are what vaqhip_index_create takes.  The plan is fit_codebooks_plan.h's.
#include "vaqhip_index.h"

#include <chrono>
#include <cstring>
#include <vector>

#include "fit_codebooks_bin_plan.h"
#include "fit_codebooks_hier_plan.h"
#include "kmeans_sample.h"
#include "vaq_codebooks.h"

using namespace vaqhost;
namespace cb = vaq::cbfit;
namespace ch = vaq::cbhier;
namespace cn = vaq::cbbin;

namespace {
thread_local int g_cb_timing = 0;
thread_local vaqhip_fit_codebooks_timing g_cb_last = {};
thread_local vaqhip_fit_codebooks_hier_timing g_cbh_last = {};
thread_local vaqhip_fit_codebooks_bin_timing g_cbn_last = {};
thread_local int g_cbn_sums = 0;  // vaqhip_fit_codebooks_bin_set_sums

using Form = vaqhost::CodebookForm;  // which of the three forms an entry point is

// every refusal that needs no device, in the order the header lists them; fills the plan when there is none
int check_args(const void *X, int64_t n, int D, int M, const int *bits, int max_iter, const void *cent, cb::Plan *plan) {
  if (!X || !bits || !cent) return fail(VAQHIP_EINVAL, "null pointer");
  if (n < 1) return fail(VAQHIP_EINVAL, "n=%lld: no row to seed a centre from", (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(VAQHIP_EINVAL, "n=%lld: randomPermutation counts rows in an int", (long long)n);
  if (D < 1 || M < 1 || D % M != 0) return fail(VAQHIP_EINVAL, "D=%d is not M=%d subspaces of equal length", D, M);
  if (max_iter < 1) return fail(VAQHIP_EINVAL, "max_iter=%d", max_iter);
  if (M > VAQHIP_MAX_SUBSPACES) return fail(VAQHIP_EUNSUPPORTED, "M=%d > %d", M, VAQHIP_MAX_SUBSPACES);
  if (D > 4096) return fail(VAQHIP_EUNSUPPORTED, "D=%d > 4096", D);
  for (int s = 0; s < M; s++) {
    if (bits[s] < 1 || bits[s] > VAQHIP_MAX_BITS)
      return fail(VAQHIP_EINVAL, "bits[%d]=%d outside 1..%d", s, bits[s], VAQHIP_MAX_BITS);
    if (((int64_t)1 << bits[s]) > cb::sample_rows(n, 1 << bits[s]))
      return fail(VAQHIP_EINVAL, "bits[%d]=%d: %d centres from %lld rows (the reference seeds from rows out of bounds)", s,
                  bits[s], 1 << bits[s], (long long)n);
  }
  // (at most VAQHIP_MAX_SUBSPACES * 256 << VAQHIP_MAX_BITS = 2^30 sampled rows over all subspaces: the runs fit an int)
  *plan = cb::make_plan(n, M, bits);
  return VAQHIP_OK;
}

// the plans of a call: the flat one always, and the form's own (fit_codebooks_hier_plan.h, fit_codebooks_bin_plan.h)
// where a subspace is above 8 bits -- else the call is the flat fit, bit for bit
struct Plans {
  Form form = Form::FLAT;
  cb::Plan flat;
  ch::Plan hier;
  cn::Plan bin;
  // the wide form's plan head; null when the call is the flat fit
  const cb::WideHead *wide() const { return !hier.hsub.empty() ? &hier : !bin.bsub.empty() ? &bin : (const cb::WideHead *)nullptr; }
};

// every refusal that needs no device, for any form; fills the plans
int plan_call(Form form, const void *X, int64_t n, int D, int M, const int *bits, int max_iter, const void *cent, Plans *p) {
  p->form = form;
  if (int rc = check_args(X, n, D, M, bits, max_iter, cent, &p->flat)) return rc;
  if (form == Form::FLAT) return VAQHIP_OK;
  const int s = cb::first_short_subspace(n, M, bits);  // (both wide forms: the same subspaces, the same rows)
  if (s >= 0)
    return fail(VAQHIP_EINVAL, "bits[%d]=%d: %d centres from %lld rows (the reference seeds from rows out of bounds)", s,
                bits[s], 1 << bits[s], (long long)n);
  bool any = false;
  for (int i = 0; i < M; i++) any |= cb::wide(bits[i]);
  if (any && form == Form::HIER) p->hier = ch::make_plan(n, D, M, bits);
  if (any && form == Form::BIN) p->bin = cn::make_plan(n, M, bits);
  return VAQHIP_OK;
}

int refuse_hier(const ch::Refusal &r) {
  switch (r.kind) {
  case ch::NAN_CENTRE:
    return fail(VAQHIP_EINVAL, "subspace %d, group %d: the stage-1 centre is NaN (the reference asserts \"hierarchical kmeans failed\")",
                r.s, r.group);
  case ch::EMPTY_GROUP:
    return fail(VAQHIP_EINVAL, "subspace %d, group %d: no row is nearest to this stage-1 centre (the reference asserts "
                               "\"hierarchical kmeans failed\")", r.s, r.group);
  case ch::SHORT_GROUP:
    return fail(VAQHIP_EINVAL, "subspace %d, group %d: %d centres from %lld rows (the reference seeds from rows out of bounds)",
                r.s, r.group, r.K2, (long long)r.rows);
  case ch::NO_CENTRE:
    return fail(VAQHIP_EINVAL, "subspace %d: a row is at a squared distance >= FLT_MAX (or NaN) from all 128 stage-1 centres", r.s);
  case ch::SAMPLED_GROUP:
    return fail(VAQHIP_EUNSUPPORTED, "subspace %d, group %d: %lld rows > %lld: the reference's stage 2 would sample the group "
                                     "(not built)", r.s, r.group, (long long)r.rows, (long long)ch::group_limit(r.K2));
  default:
    return VAQHIP_OK;
  }
}

// what every form reports of its last call
void note_last(float total_ms, const vaq::CodebookPhases &ph, int iterations, int64_t sample_rows, int64_t n, int D, int M) {
  g_cb_last = vaqhip_fit_codebooks_timing{};
  g_cb_last.total_ms = total_ms;
  g_cb_last.gather_ms = (float)ph.gather_ms;
  g_cb_last.assign_ms = (float)ph.assign_ms;
  g_cb_last.accumulate_ms = (float)ph.accumulate_ms;
  g_cb_last.update_ms = (float)ph.update_ms;
  g_cb_last.iterations = iterations;
  g_cb_last.sample_rows = sample_rows;
  g_cb_last.rows = n;
  g_cb_last.dims = D;
  g_cb_last.subspaces = M;
}

// a wide form's figures emptied but for what they share with g_cb_last; a call that was the flat fit (no subspace above
// 8 bits) is one stage `ms` of `iterations`
template <typename T>
void note_wide(T &last, float T::*ms = nullptr, int T::*iterations = nullptr) {
  last = T{};
  last.total_ms = g_cb_last.total_ms;
  if (ms) last.*ms = g_cb_last.total_ms;
  if (iterations) last.*iterations = g_cb_last.iterations;
  last.subspaces = g_cb_last.subspaces;
  last.dims = g_cb_last.dims;
  last.rows = g_cb_last.rows;
}
void note_flat_as(Form form) {
  if (form == Form::HIER)
    note_wide(g_cbh_last, &vaqhip_fit_codebooks_hier_timing::stage1_ms, &vaqhip_fit_codebooks_hier_timing::stage1_iterations);
  if (form == Form::BIN)
    note_wide(g_cbn_last, &vaqhip_fit_codebooks_bin_timing::fit_ms, &vaqhip_fit_codebooks_bin_timing::max_iterations);
}

// The fit of any form: the form's own device fit where a subspace is above 8 bits, else the flat one.  Device pointers
// throughout (bits, iters_out, nan_rows_out: host), the device current; the outputs are written only when the fit
// succeeds.
int fit_core(vaq::RowsRef d_X, int64_t n, int D, const Plans &p, const float *d_eig, int max_iter, float *d_cent_out,
             int *iters_out, int *nan_rows_out, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  const int M = (int)p.flat.sub.size(), L = D / M, H = (int)p.hier.hsub.size();
  const bool bin = !p.bin.bsub.empty();
  const size_t cent_floats = (size_t)p.flat.n_cent * L;
  DevBuf b_means;  // the final centres, the hierarchical form's stage-1 centres behind them
  HIP_TRY(b_means.ensure((cent_floats + (size_t)H * ch::K1 * L) * sizeof(float)));
  std::vector<int> iters((size_t)M, 0);
  int no_centre = 0;
  ch::Refusal refusal;
  vaq::CodebookHierStats hs;
  vaq::CodebookBinStats bs;
  vaq::CodebookPhases ph, *php = g_cb_timing ? &ph : nullptr;
  if (H)  // (all three synchronise)
    HIP_TRY(vaq::codebooks_fit_hier(d_X, n, D, L, p.hier, d_eig, max_iter, b_means.as<float>(), iters.data(), &no_centre, &refusal,
                                    &hs, php, st));
  else if (bin)
    HIP_TRY(vaq::codebooks_fit_bin(d_X, n, D, L, p.bin, d_eig, max_iter, g_cbn_sums == 0, b_means.as<float>(), iters.data(),
                                   &no_centre, &bs, php, st));
  else
    HIP_TRY(vaq::codebooks_fit(d_X, n, D, L, p.flat, d_eig, max_iter, b_means.as<float>(), iters.data(), &no_centre, php, st));
  if (refusal.kind != ch::OK) return refuse_hier(refusal);
  if (no_centre)
    return fail(VAQHIP_EINVAL, "a row is at a distance >= FLT_MAX (or NaN) from every centre: the reference indexes row -1");
  std::vector<float> means(cent_floats);
  HIP_TRY(hipMemcpyAsync(means.data(), b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(d_cent_out, b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  int max_iters = 0;
  for (int s = 0; s < M; s++) {
    const cb::Sub &sd = p.flat.sub[(size_t)s];
    if (iters_out) iters_out[s] = iters[(size_t)s];
    if (nan_rows_out) nan_rows_out[s] = vaq::nan_rows(means.data() + (size_t)sd.cent_off * L, sd.k, L);
    max_iters = std::max(max_iters, iters[(size_t)s]);
  }
  const cb::WideHead *w = p.wide();
  note_last(bin ? (float)bs.total_ms : std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(), ph,
            bin ? bs.max_iters : max_iters, w ? std::max(w->gathered, w->n_full ? n : (int64_t)0) : p.flat.sample, n, D, M);
  if (H) {
    note_wide(g_cbh_last);
    g_cbh_last.stage1_ms = (float)hs.stage1_ms;
    g_cbh_last.regroup_ms = (float)hs.regroup_ms;
    g_cbh_last.stage2_ms = (float)hs.stage2_ms;
    g_cbh_last.groups = hs.groups;
    g_cbh_last.min_group_rows = hs.min_group;
    g_cbh_last.max_group_rows = hs.max_group;
    g_cbh_last.stage1_iterations = hs.stage1_iters;
    g_cbh_last.stage2_iterations = hs.stage2_iters;
    g_cbh_last.hier_subspaces = H;
  } else if (bin) {
    note_wide(g_cbn_last);
    g_cbn_last.fit_ms = (float)bs.fit_ms;
    g_cbn_last.split_ms = (float)bs.split_ms;
    g_cbn_last.cut_ms = (float)bs.cut_ms;
    g_cbn_last.levels = bs.levels;
    g_cbn_last.nodes = bs.nodes;
    g_cbn_last.cut_nodes = bs.cut_nodes;
    g_cbn_last.resampled_fits = bs.resampled_fits;
    g_cbn_last.leaf_nodes = bs.leaf_nodes;
    g_cbn_last.min_leaf_rows = bs.min_leaf_rows;
    g_cbn_last.max_leaf_rows = bs.max_leaf_rows;
    g_cbn_last.max_iterations = bs.max_iters;
    g_cbn_last.bin_subspaces = (int)p.bin.bsub.size();
  } else {
    note_flat_as(p.form);
  }
  return VAQHIP_OK;
}

int fit_device_entry(Form form, int device_id, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits, const float *d_eigvec,
                     int max_iter, float *d_centroids_out, int *iters_out, int *nan_rows_out, void *stream) {
  Plans p;
  if (int rc = plan_call(form, d_X.p, n, D, M, bits, max_iter, d_centroids_out, &p)) return rc;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  return fit_core(d_X, n, D, p, d_eigvec, max_iter, d_centroids_out, iters_out, nan_rows_out, static_cast<hipStream_t>(stream));
}

// the rest of a host-output call once the rows are on the device (current): eigvec up, fit, centres down
int fit_to_host(vaq::RowsRef d_X, int64_t n, int D, const Plans &p, const float *eigvec, int max_iter,
                float *centroids_out, int *iters_out, int *nan_rows_out) {
  const cb::Plan &plan = p.flat;
  DevBuf d_eig, d_cent;
  const size_t cent_bytes = (size_t)plan.n_cent * (D / (int)plan.sub.size()) * sizeof(float);
  HIP_TRY(d_cent.ensure(cent_bytes));
  if (eigvec) {
    HIP_TRY(d_eig.ensure((size_t)D * D * sizeof(float)));
    HIP_TRY(hipMemcpy(d_eig.p, eigvec, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice));
  }
  CallStream st;
  HIP_TRY(st.open());
  if (int rc = fit_core(d_X, n, D, p, eigvec ? d_eig.as<float>() : nullptr, max_iter, d_cent.as<float>(), iters_out,
                        nan_rows_out, st.s))
    return rc;
  HIP_TRY(hipMemcpy(centroids_out, d_cent.p, cent_bytes, hipMemcpyDeviceToHost));
  return VAQHIP_OK;
}

// X: host rows of X.elem bytes per element, uploaded as they are.  Where every subspace samples, only the sample goes
// up: its rows are copied out in the sample's order here, and the device is handed the sample itself.  Where one
// subspace reads all rows, all rows go up, and the device gathers the sample of the others.
// The hierarchical and the binary form with a subspace above 8 bits upload all rows: their one gather serves both kinds
// of subspace.
int fit_host_entry(Form form, int device_id, vaq::RowsRef X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                   int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  Plans p;
  if (int rc = plan_call(form, X.p, n, D, M, bits, max_iter, centroids_out, &p)) return rc;
  cb::Plan &plan = p.flat;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  DevBuf d_x;
  const bool sample_only = plan.sampled && !p.wide();
  const size_t row_bytes = (size_t)D * (size_t)X.elem, x_bytes = (size_t)(sample_only ? plan.sample : n) * row_bytes;
  HIP_TRY(d_x.ensure(x_bytes));
  if (sample_only) {
    const std::vector<int> rows = vaq::permutation_head(n, plan.sample);
    std::vector<char> picked(x_bytes);
    for (int64_t i = 0; i < plan.sample; i++)
      std::memcpy(picked.data() + (size_t)i * row_bytes, static_cast<const char *>(X.p) + (size_t)rows[(size_t)i] * row_bytes, row_bytes);
    HIP_TRY(hipMemcpy(d_x.p, picked.data(), x_bytes, hipMemcpyHostToDevice));
    plan.gather = false;
  } else {
    HIP_TRY(hipMemcpy(d_x.p, X.p, x_bytes, hipMemcpyHostToDevice));
  }
  return fit_to_host(vaq::RowsRef{d_x.p, X.elem}, n, D, p, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
}  // namespace

// vaqhip_refiner.cpp calls this over its resident rows (n x D on `device`, complete), its lock held: a form over rows
// resident on `device`, the outputs the host's
int vaqhost::fit_codebooks_rows_device(CodebookForm form, int device, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits,
                                       const float *eigvec, int max_iter, float *centroids_out, int *iters_out,
                                       int *nan_rows_out) {
  Plans p;
  if (int rc = plan_call(form, d_X.p, n, D, M, bits, max_iter, centroids_out, &p)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  return fit_to_host(d_X, n, D, p, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}

extern "C" {

int vaqhip_fit_codebooks_hier(int device_id, const float *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                              int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(Form::HIER, device_id, vaq::RowsRef{X, 4}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_hier_u8(int device_id, const uint8_t *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                                 int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(Form::HIER, device_id, vaq::RowsRef{X, 1}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_hier_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                     const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                     int *nan_rows_out, void *stream) {
  return fit_device_entry(Form::HIER, device_id, vaq::RowsRef{d_X, 4}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}
int vaqhip_fit_codebooks_hier_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                        const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                        int *nan_rows_out, void *stream) {
  return fit_device_entry(Form::HIER, device_id, vaq::RowsRef{d_X, 1}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}
int vaqhip_last_fit_codebooks_hier_timing(vaqhip_fit_codebooks_hier_timing *out) {
  if (!out) return fail(VAQHIP_EINVAL, "null pointer");
  *out = g_cbh_last;
  return VAQHIP_OK;
}

int vaqhip_fit_codebooks_bin(int device_id, const float *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                             int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(Form::BIN, device_id, vaq::RowsRef{X, 4}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_bin_u8(int device_id, const uint8_t *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                                int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(Form::BIN, device_id, vaq::RowsRef{X, 1}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_bin_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                    const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                    int *nan_rows_out, void *stream) {
  return fit_device_entry(Form::BIN, device_id, vaq::RowsRef{d_X, 4}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}
int vaqhip_fit_codebooks_bin_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                       const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                       int *nan_rows_out, void *stream) {
  return fit_device_entry(Form::BIN, device_id, vaq::RowsRef{d_X, 1}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}
int vaqhip_last_fit_codebooks_bin_timing(vaqhip_fit_codebooks_bin_timing *out) {
  if (!out) return fail(VAQHIP_EINVAL, "null pointer");
  *out = g_cbn_last;
  return VAQHIP_OK;
}
int vaqhip_fit_codebooks_bin_set_sums(int mode) {
  if (mode != 0 && mode != 1) return fail(VAQHIP_EINVAL, "mode=%d: 0 (staged sums) or 1 (one thread per run)", mode);
  g_cbn_sums = mode;
  return VAQHIP_OK;
}

int vaqhip_fit_codebooks(int device_id, const float *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                         int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(Form::FLAT, device_id, vaq::RowsRef{X, 4}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_u8(int device_id, const uint8_t *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                            int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(Form::FLAT, device_id, vaq::RowsRef{X, 1}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                int *nan_rows_out, void *stream) {
  return fit_device_entry(Form::FLAT, device_id, vaq::RowsRef{d_X, 4}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}
int vaqhip_fit_codebooks_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                   const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                   int *nan_rows_out, void *stream) {
  return fit_device_entry(Form::FLAT, device_id, vaq::RowsRef{d_X, 1}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}

// ---- vaqhip_internal.h: what the sharded fit takes from here ----
int vaqhip_internal_fit_codebooks_check(const void *X, int64_t n, int D, int M, const int *bits, int max_iter,
                                        const void *centroids_out) {
  cb::Plan plan;
  return check_args(X, n, D, M, bits, max_iter, centroids_out, &plan);
}
int vaqhip_internal_fit_codebooks_rows_device(int device, const void *d_X, int elem, int64_t n, int D, int M,
                                              const int *bits, const float *eigvec, int max_iter, float *centroids_out,
                                              int *iters_out, int *nan_rows_out) {
  return fit_codebooks_rows_device(Form::FLAT, device, vaq::RowsRef{d_X, elem}, n, D, M, bits, eigvec, max_iter, centroids_out,
                                   iters_out, nan_rows_out);
}
int vaqhip_internal_fit_codebooks_timing_on(void) { return g_cb_timing; }

int vaqhip_fit_codebooks_set_timing(int on) {
  g_cb_timing = on != 0;
  return VAQHIP_OK;
}

int vaqhip_last_fit_codebooks_timing(vaqhip_fit_codebooks_timing *out) {
  if (!out) return fail(VAQHIP_EINVAL, "null pointer");
  *out = g_cb_last;
  return VAQHIP_OK;
}

}  // extern "C"
