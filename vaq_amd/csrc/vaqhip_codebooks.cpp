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

// which of the three forms an entry point is
enum Form { FLAT = 0, HIER, BIN };

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

// device pointers throughout (bits, iters_out, nan_rows_out: host), the device current; the outputs are written only
// when the fit succeeds
int fit_core(vaq::RowsRef d_X, int64_t n, int D, const cb::Plan &plan, const float *d_eig, int max_iter,
             float *d_cent_out, int *iters_out, int *nan_rows_out, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  const int M = (int)plan.sub.size(), L = D / M;
  const size_t cent_floats = (size_t)plan.n_cent * L;
  DevBuf b_means;
  HIP_TRY(b_means.ensure(cent_floats * sizeof(float)));
  std::vector<int> iters((size_t)M, 0);
  int no_centre = 0;
  vaq::CodebookPhases ph;
  HIP_TRY(vaq::codebooks_fit(d_X, n, D, L, plan, d_eig, max_iter, b_means.as<float>(), iters.data(), &no_centre,
                             g_cb_timing ? &ph : nullptr, st));  // synchronises
  if (no_centre)
    return fail(VAQHIP_EINVAL, "a row is at a distance >= FLT_MAX (or NaN) from every centre: the reference indexes row -1");
  std::vector<float> means(cent_floats);
  HIP_TRY(hipMemcpyAsync(means.data(), b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(d_cent_out, b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  int max_iters = 0;
  for (int s = 0; s < M; s++) {
    const cb::Sub &sd = plan.sub[(size_t)s];
    if (iters_out) iters_out[s] = iters[(size_t)s];
    if (nan_rows_out) nan_rows_out[s] = vaq::nan_rows(means.data() + (size_t)sd.cent_off * L, sd.k, L);
    max_iters = std::max(max_iters, iters[(size_t)s]);
  }
  g_cb_last = vaqhip_fit_codebooks_timing{};
  g_cb_last.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g_cb_last.gather_ms = (float)ph.gather_ms;
  g_cb_last.assign_ms = (float)ph.assign_ms;
  g_cb_last.accumulate_ms = (float)ph.accumulate_ms;
  g_cb_last.update_ms = (float)ph.update_ms;
  g_cb_last.iterations = max_iters;
  g_cb_last.sample_rows = plan.sample;
  g_cb_last.rows = n;
  g_cb_last.dims = D;
  g_cb_last.subspaces = M;
  return VAQHIP_OK;
}

// ---- the hierarchical form: subspaces above 8 bits in two stages (fit_codebooks_hier_plan.h) ----
// what the hierarchical form refuses beyond check_args, and its plan; hp->hsub stays empty when no subspace is above
// 8 bits: the call is then the flat fit, bit for bit
int plan_hier(int64_t n, int D, int M, const int *bits, ch::Plan *hp) {
  const int s = ch::first_short_subspace(n, M, bits);
  if (s >= 0)
    return fail(VAQHIP_EINVAL, "bits[%d]=%d: %d centres from %lld rows (the reference seeds from rows out of bounds)", s,
                bits[s], 1 << bits[s], (long long)n);
  bool any = false;
  for (int i = 0; i < M; i++) any |= ch::hierarchical(bits[i]);
  if (any) *hp = ch::make_plan(n, D, M, bits);
  return VAQHIP_OK;
}

// the last hierarchical call's figures when it was the flat fit (no subspace above 8 bits)
void note_flat_as_hier() {
  g_cbh_last = vaqhip_fit_codebooks_hier_timing{};
  g_cbh_last.total_ms = g_cbh_last.stage1_ms = g_cb_last.total_ms;
  g_cbh_last.stage1_iterations = g_cb_last.iterations;
  g_cbh_last.subspaces = g_cb_last.subspaces;
  g_cbh_last.dims = g_cb_last.dims;
  g_cbh_last.rows = g_cb_last.rows;
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

// fit_core's twin over a plan with a hierarchical subspace
int fit_core_hier(vaq::RowsRef d_X, int64_t n, int D, const ch::Plan &hp, const float *d_eig, int max_iter, float *d_cent_out,
                  int *iters_out, int *nan_rows_out, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  const int M = (int)hp.flat.sub.size(), L = D / M, H = (int)hp.hsub.size();
  const size_t cent_floats = (size_t)hp.n_cent * L;
  DevBuf b_means;  // the final centres, the stage-1 centres behind them
  HIP_TRY(b_means.ensure((cent_floats + (size_t)H * ch::K1 * L) * sizeof(float)));
  std::vector<int> iters((size_t)M, 0);
  int no_centre = 0;
  ch::Refusal refusal;
  vaq::CodebookHierStats hs;
  vaq::CodebookPhases ph;
  HIP_TRY(vaq::codebooks_fit_hier(d_X, n, D, L, hp, d_eig, max_iter, b_means.as<float>(), iters.data(), &no_centre, &refusal,
                                  &hs, g_cb_timing ? &ph : nullptr, st));  // synchronises
  if (refusal.kind != ch::OK) return refuse_hier(refusal);
  if (no_centre)
    return fail(VAQHIP_EINVAL, "a row is at a distance >= FLT_MAX (or NaN) from every centre: the reference indexes row -1");
  std::vector<float> means(cent_floats);
  HIP_TRY(hipMemcpyAsync(means.data(), b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(d_cent_out, b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  int max_iters = 0;
  for (int s = 0; s < M; s++) {
    const cb::Sub &sd = hp.flat.sub[(size_t)s];
    if (iters_out) iters_out[s] = iters[(size_t)s];
    if (nan_rows_out) nan_rows_out[s] = vaq::nan_rows(means.data() + (size_t)sd.cent_off * L, sd.k, L);
    max_iters = std::max(max_iters, iters[(size_t)s]);
  }
  const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g_cb_last = vaqhip_fit_codebooks_timing{};
  g_cb_last.total_ms = total;
  g_cb_last.gather_ms = (float)ph.gather_ms;
  g_cb_last.assign_ms = (float)ph.assign_ms;
  g_cb_last.accumulate_ms = (float)ph.accumulate_ms;
  g_cb_last.update_ms = (float)ph.update_ms;
  g_cb_last.iterations = max_iters;
  g_cb_last.sample_rows = std::max(hp.gathered, hp.n_full ? n : (int64_t)0);
  g_cb_last.rows = n;
  g_cb_last.dims = D;
  g_cb_last.subspaces = M;
  g_cbh_last = vaqhip_fit_codebooks_hier_timing{};
  g_cbh_last.total_ms = total;
  g_cbh_last.stage1_ms = (float)hs.stage1_ms;
  g_cbh_last.regroup_ms = (float)hs.regroup_ms;
  g_cbh_last.stage2_ms = (float)hs.stage2_ms;
  g_cbh_last.groups = hs.groups;
  g_cbh_last.min_group_rows = hs.min_group;
  g_cbh_last.max_group_rows = hs.max_group;
  g_cbh_last.stage1_iterations = hs.stage1_iters;
  g_cbh_last.stage2_iterations = hs.stage2_iters;
  g_cbh_last.hier_subspaces = H;
  g_cbh_last.subspaces = M;
  g_cbh_last.dims = D;
  g_cbh_last.rows = n;
  return VAQHIP_OK;
}

// ---- the binary-tree form: subspaces above 8 bits as a tree of 2-centre fits (fit_codebooks_bin_plan.h) ----
// the plans of a call: the flat one always, and the form's own where a subspace is above 8 bits (else the call is the
// flat fit, bit for bit)
struct Plans {
  Form form = FLAT;
  cb::Plan flat;
  ch::Plan hier;
  cn::Plan bin;
  bool wide() const { return !hier.hsub.empty() || !bin.bsub.empty(); }
};

// every refusal that needs no device, for any form; fills the plans
int plan_call(Form form, const void *X, int64_t n, int D, int M, const int *bits, int max_iter, const void *cent, Plans *p) {
  p->form = form;
  if (int rc = check_args(X, n, D, M, bits, max_iter, cent, &p->flat)) return rc;
  if (form == HIER) return plan_hier(n, D, M, bits, &p->hier);
  if (form != BIN) return VAQHIP_OK;
  const int s = ch::first_short_subspace(n, M, bits);  // (the same subspaces, the same rows)
  if (s >= 0)
    return fail(VAQHIP_EINVAL, "bits[%d]=%d: %d centres from %lld rows (the reference seeds from rows out of bounds)", s,
                bits[s], 1 << bits[s], (long long)n);
  bool any = false;
  for (int i = 0; i < M; i++) any |= cn::binary(bits[i]);
  if (any) p->bin = cn::make_plan(n, M, bits);
  return VAQHIP_OK;
}

// the last binary call's figures when it was the flat fit (no subspace above 8 bits)
void note_flat_as_bin() {
  g_cbn_last = vaqhip_fit_codebooks_bin_timing{};
  g_cbn_last.total_ms = g_cbn_last.fit_ms = g_cb_last.total_ms;
  g_cbn_last.max_iterations = g_cb_last.iterations;
  g_cbn_last.subspaces = g_cb_last.subspaces;
  g_cbn_last.dims = g_cb_last.dims;
  g_cbn_last.rows = g_cb_last.rows;
}

// fit_core's twin over a plan with a binary subspace
int fit_core_bin(vaq::RowsRef d_X, int64_t n, int D, const cn::Plan &bp, const float *d_eig, int max_iter, float *d_cent_out,
                 int *iters_out, int *nan_rows_out, hipStream_t st) {
  const int M = (int)bp.flat.sub.size(), L = D / M;
  const size_t cent_floats = (size_t)bp.n_cent * L;
  DevBuf b_means;
  HIP_TRY(b_means.ensure(cent_floats * sizeof(float)));
  std::vector<int> iters((size_t)M, 0);
  int no_centre = 0;
  vaq::CodebookBinStats bs;
  vaq::CodebookPhases ph;
  HIP_TRY(vaq::codebooks_fit_bin(d_X, n, D, L, bp, d_eig, max_iter, g_cbn_sums == 0, b_means.as<float>(), iters.data(), &no_centre,
                                 &bs, g_cb_timing ? &ph : nullptr, st));  // synchronises
  if (no_centre)
    return fail(VAQHIP_EINVAL, "a row is at a distance >= FLT_MAX (or NaN) from every centre: the reference indexes row -1");
  std::vector<float> means(cent_floats);
  HIP_TRY(hipMemcpyAsync(means.data(), b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(d_cent_out, b_means.p, cent_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int s = 0; s < M; s++) {
    const cb::Sub &sd = bp.flat.sub[(size_t)s];
    if (iters_out) iters_out[s] = iters[(size_t)s];
    if (nan_rows_out) nan_rows_out[s] = vaq::nan_rows(means.data() + (size_t)sd.cent_off * L, sd.k, L);
  }
  g_cb_last = vaqhip_fit_codebooks_timing{};
  g_cb_last.total_ms = (float)bs.total_ms;
  g_cb_last.gather_ms = (float)ph.gather_ms;
  g_cb_last.assign_ms = (float)ph.assign_ms;
  g_cb_last.accumulate_ms = (float)ph.accumulate_ms;
  g_cb_last.update_ms = (float)ph.update_ms;
  g_cb_last.iterations = bs.max_iters;
  g_cb_last.sample_rows = std::max(bp.gathered, bp.n_full ? n : (int64_t)0);
  g_cb_last.rows = n;
  g_cb_last.dims = D;
  g_cb_last.subspaces = M;
  g_cbn_last = vaqhip_fit_codebooks_bin_timing{};
  g_cbn_last.total_ms = (float)bs.total_ms;
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
  g_cbn_last.bin_subspaces = (int)bp.bsub.size();
  g_cbn_last.subspaces = M;
  g_cbn_last.dims = D;
  g_cbn_last.rows = n;
  return VAQHIP_OK;
}

// the form's own fit where a subspace is above 8 bits; else the flat one
int fit_either(vaq::RowsRef d_X, int64_t n, int D, const Plans &p, const float *d_eig, int max_iter, float *d_cent_out,
               int *iters_out, int *nan_rows_out, hipStream_t st) {
  if (!p.hier.hsub.empty()) return fit_core_hier(d_X, n, D, p.hier, d_eig, max_iter, d_cent_out, iters_out, nan_rows_out, st);
  if (!p.bin.bsub.empty()) return fit_core_bin(d_X, n, D, p.bin, d_eig, max_iter, d_cent_out, iters_out, nan_rows_out, st);
  const int rc = fit_core(d_X, n, D, p.flat, d_eig, max_iter, d_cent_out, iters_out, nan_rows_out, st);
  if (p.form == HIER && rc == VAQHIP_OK) note_flat_as_hier();
  if (p.form == BIN && rc == VAQHIP_OK) note_flat_as_bin();
  return rc;
}

// form: the hierarchical or the binary form's refusals and plan on top (vaqhip_fit_codebooks_hier*, _bin*)
int fit_device_entry(int device_id, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits, const float *d_eigvec,
                     int max_iter, float *d_centroids_out, int *iters_out, int *nan_rows_out, void *stream, Form form = FLAT) {
  Plans p;
  if (int rc = plan_call(form, d_X.p, n, D, M, bits, max_iter, d_centroids_out, &p)) return rc;
  DeviceGuard g(device_id);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device_id);
  return fit_either(d_X, n, D, p, d_eigvec, max_iter, d_centroids_out, iters_out, nan_rows_out, static_cast<hipStream_t>(stream));
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
  if (int rc = fit_either(d_X, n, D, p, eigvec ? d_eig.as<float>() : nullptr, max_iter, d_cent.as<float>(), iters_out,
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
int fit_host_entry(int device_id, vaq::RowsRef X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                   int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out, Form form = FLAT) {
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

// a form over rows resident on `device` (n x D, complete), the outputs the host's
int rows_device_entry(Form form, int device, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                      int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  Plans p;
  if (int rc = plan_call(form, d_X.p, n, D, M, bits, max_iter, centroids_out, &p)) return rc;
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed (no CPU path)", device);
  return fit_to_host(d_X, n, D, p, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
}  // namespace

// vaqhip_refiner.cpp calls this over its resident rows (n x D on `device`, complete), its lock held
int vaqhost::fit_codebooks_rows_device(int device, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits,
                                       const float *eigvec, int max_iter, float *centroids_out, int *iters_out,
                                       int *nan_rows_out) {
  return rows_device_entry(FLAT, device, d_X, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}

// the hierarchical twin (vaqhip_refiner_fit_codebooks_hier)
int vaqhost::fit_codebooks_hier_rows_device(int device, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits,
                                            const float *eigvec, int max_iter, float *centroids_out, int *iters_out,
                                            int *nan_rows_out) {
  return rows_device_entry(HIER, device, d_X, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}

// the binary twin (vaqhip_refiner_fit_codebooks_bin)
int vaqhost::fit_codebooks_bin_rows_device(int device, vaq::RowsRef d_X, int64_t n, int D, int M, const int *bits,
                                           const float *eigvec, int max_iter, float *centroids_out, int *iters_out,
                                           int *nan_rows_out) {
  return rows_device_entry(BIN, device, d_X, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}

extern "C" {

int vaqhip_fit_codebooks_hier(int device_id, const float *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                              int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 4}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out, HIER);
}
int vaqhip_fit_codebooks_hier_u8(int device_id, const uint8_t *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                                 int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 1}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out, HIER);
}
int vaqhip_fit_codebooks_hier_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                     const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                     int *nan_rows_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream, HIER);
}
int vaqhip_fit_codebooks_hier_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                        const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                        int *nan_rows_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream, HIER);
}
int vaqhip_last_fit_codebooks_hier_timing(vaqhip_fit_codebooks_hier_timing *out) {
  if (!out) return fail(VAQHIP_EINVAL, "null pointer");
  *out = g_cbh_last;
  return VAQHIP_OK;
}

int vaqhip_fit_codebooks_bin(int device_id, const float *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                             int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 4}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out, BIN);
}
int vaqhip_fit_codebooks_bin_u8(int device_id, const uint8_t *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                                int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 1}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out, BIN);
}
int vaqhip_fit_codebooks_bin_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                    const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                    int *nan_rows_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream, BIN);
}
int vaqhip_fit_codebooks_bin_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                       const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                       int *nan_rows_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream, BIN);
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
  return fit_host_entry(device_id, vaq::RowsRef{X, 4}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_u8(int device_id, const uint8_t *X, int64_t n, int D, int M, const int *bits, const float *eigvec,
                            int max_iter, float *centroids_out, int *iters_out, int *nan_rows_out) {
  return fit_host_entry(device_id, vaq::RowsRef{X, 1}, n, D, M, bits, eigvec, max_iter, centroids_out, iters_out, nan_rows_out);
}
int vaqhip_fit_codebooks_device(int device_id, const float *d_X, int64_t n, int D, int M, const int *bits,
                                const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                int *nan_rows_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 4}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
                          nan_rows_out, stream);
}
int vaqhip_fit_codebooks_u8_device(int device_id, const uint8_t *d_X, int64_t n, int D, int M, const int *bits,
                                   const float *d_eigvec, int max_iter, float *d_centroids_out, int *iters_out,
                                   int *nan_rows_out, void *stream) {
  return fit_device_entry(device_id, vaq::RowsRef{d_X, 1}, n, D, M, bits, d_eigvec, max_iter, d_centroids_out, iters_out,
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
  return fit_codebooks_rows_device(device, vaq::RowsRef{d_X, elem}, n, D, M, bits, eigvec, max_iter, centroids_out,
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
