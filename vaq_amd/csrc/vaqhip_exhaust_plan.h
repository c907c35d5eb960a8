// vaqhip_exhaust_plan.h -- what the two hosts of the exhaustive form share (vaqhip_refiner.cpp: one device;
// vaqhip_multi_refiner_search.cpp: the rows cut over shards): the split and group plan of a select launch, the
// workspace of one device, and the launches of one set of queries over one device's rows.  A shard of the multi
// refiner runs xs_select_merge over its own rows; the single refiner, and the multi refiner with one shard, run
// xs_search_set.
// Every function returns the first HIP error; the hosts put their own text around it.
#ifndef VAQHIP_EXHAUST_PLAN_H
#define VAQHIP_EXHAUST_PLAN_H
#include "vaqhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "vaq_exact.h"
#include "vaq_exhaust_launch.h"
#include "vaq_merge.h"
#include "vaqhip_dev.h"

// (hidden: none of this joins the library's exported symbols)
namespace vaqhost __attribute__((visibility("hidden"))) {

constexpr size_t XS_LIST_BYTES = (size_t)256 << 20;  // candidate lists of one launch (the queries are cut to fit)

#define XS_TRY(expr)                   \
  do {                                 \
    const hipError_t xe_ = (expr);     \
    if (xe_ != hipSuccess) return xe_; \
  } while (0)

struct XsPlan {
  int S, qg, chunk;  // splits, queries per workgroup, queries per launch
};

// One device's workspace (grow-only): candidate lists, the splits' lists, the merge's scratch, and with "exact_ties"
// the k + 1 lists and the replay list (count behind the entries).  ev: option "timing".
struct XsWork {
  int n_cu = 0, blocks_per_cu = 0, sized_elem = 0;
  DevBuf buf_d, buf_id, part_d, part_id, ms_d, ms_id, k1_l, k1_d, list;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};

  // the sizing of the plan: once per device, row width and row type (the byte-row kernels are other kernels)
  hipError_t size_for(int device, int D, int elem) {
    if (n_cu && sized_elem == elem) return hipSuccess;
    XS_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    if (n_cu < 1) n_cu = 1;
    blocks_per_cu = vaq::exhaust_blocks_per_cu(D, elem);
    sized_elem = elem;
    return hipSuccess;
  }
  // bytes every buffer needs under `pl`; `own_k1`: the k + 1 lists and the replay list are this workspace's
  bool fits(const XsPlan &pl, int k1, bool own_k1) const {
    const size_t cap = (size_t)vaq::exhaust_list_cap(k1), c = (size_t)pl.chunk;
    const size_t ms = vaq::merge_scratch_elems(pl.S, pl.chunk, k1);
    return c * pl.S * cap * 4 <= buf_d.cap && c * pl.S * cap * 4 <= buf_id.cap && c * pl.S * k1 * 4 <= part_d.cap &&
           c * pl.S * k1 * 4 <= part_id.cap && ms * 4 <= ms_d.cap && ms * 4 <= ms_id.cap &&
           (!own_k1 || (c * k1 * 4 <= k1_l.cap && c * k1 * 4 <= k1_d.cap && (c + 1) * 4 <= list.cap));
  }
  hipError_t fit(const XsPlan &pl, int k1, bool own_k1, bool timing) {
    const size_t cap = (size_t)vaq::exhaust_list_cap(k1), c = (size_t)pl.chunk;
    XS_TRY(buf_d.ensure(c * pl.S * cap * sizeof(float)));
    XS_TRY(buf_id.ensure(c * pl.S * cap * sizeof(int)));
    XS_TRY(part_d.ensure(c * pl.S * k1 * sizeof(float)));
    XS_TRY(part_id.ensure(c * pl.S * k1 * sizeof(int)));
    const size_t ms = vaq::merge_scratch_elems(pl.S, pl.chunk, k1);
    XS_TRY(ms_d.ensure(ms * sizeof(float)));
    XS_TRY(ms_id.ensure(ms * sizeof(int)));
    if (own_k1) {
      XS_TRY(k1_l.ensure(c * k1 * sizeof(int32_t)));
      XS_TRY(k1_d.ensure(c * k1 * sizeof(float)));
      XS_TRY(list.ensure((c + 1) * sizeof(int)));
    }
    if (timing) XS_TRY(ensure_events(ev));
    return hipSuccess;
  }
  // with the workspace's device current and its streams idle
  void release() { release_all({&buf_d, &buf_id, &part_d, &part_id, &ms_d, &ms_id, &k1_l, &k1_d, &list}), destroy_events(ev); }
};

// N rows on the workspace's device against nq queries, lists of k1; opt_splits: "exhaustive_splits"; max_chunk: a
// bound on the queries per launch from elsewhere (the multi refiner's gathered lists, its other shards)
inline XsPlan xs_plan(const XsWork &w, int64_t N, int opt_splits, int nq, int k1, int max_chunk = 0x7fffffff) {
  // ONE round of resident workgroups: with equal shares they end together, and no partly filled second round runs
  const int target = std::max(w.n_cu, 1) * std::max(w.blocks_per_cu, 1);
  const int64_t tiles = std::max<int64_t>(1, (N + vaq::XS_TILE - 1) / vaq::XS_TILE);
  XsPlan pl;
  if (opt_splits > 0) {
    pl.S = opt_splits;
  } else {  // few queries: many splits fill the device; many queries: few splits, the lists stay small
    const int g0 = (nq + 63) / 64;
    pl.S = (int)std::min<int64_t>(std::min<int64_t>(64, tiles), std::max(1, (target + g0 - 1) / g0));
  }
  const size_t per_query = (size_t)pl.S * vaq::exhaust_list_cap(k1) * (sizeof(float) + sizeof(int));
  const int fit = (int)std::min<size_t>(std::min(nq, std::max(max_chunk, 1)), std::max<size_t>(1, XS_LIST_BYTES / per_query));
  const int sets = (nq + fit - 1) / fit;
  pl.chunk = (nq + sets - 1) / sets;  // equal sets: the last one fills the device like the others
  const int g_want = std::max(1, target / pl.S);  // S * groups <= target
  pl.qg = std::min(vaq::XS_MAX_QG, std::max((pl.chunk + g_want - 1) / g_want, std::min(pl.chunk, 8)));
  return pl;
}

// the rows one call searches: N x D floats or bytes on the current device, row i carries label id_base + i
struct XsRows {
  vaq::RowsRef rows;
  int64_t N, id_base;
  int D;
};

// n <= pl.chunk queries: select per split, merge the splits into m_l / m_d [n][k1] (-1 / FLT_MAX in empty slots).
// after_select (optional) is recorded between the two; geometry (optional): S * G and qg of the launch.
inline hipError_t xs_select_merge(XsWork &w, const XsPlan &pl, const XsRows &x, const float *d_q, int n, int k1,
                                  int32_t *m_l, float *m_d, hipStream_t st, hipEvent_t after_select = nullptr,
                                  int *workgroups = nullptr, int *queries_per_group = nullptr) {
  vaq::XsParams p;
  p.nq = n;
  p.D = x.D;
  p.N = x.N;
  p.id_base = x.id_base;
  p.k = k1;
  p.cap = vaq::exhaust_list_cap(k1);
  p.S = pl.S;
  p.qg = std::min(pl.qg, n);
  p.G = (n + p.qg - 1) / p.qg;
  p.split_rows = (x.N + pl.S - 1) / pl.S;
  p.buf_d = w.buf_d.as<float>();
  p.buf_id = w.buf_id.as<int>();
  p.part_d = w.part_d.as<float>();
  p.part_id = w.part_id.as<int>();
  XS_TRY(vaq::launch_exhaust_select(p, d_q, x.rows, st));
  if (after_select) XS_TRY(hipEventRecord(after_select, st));
  XS_TRY(vaq::launch_merge(p.part_d, p.part_id, nullptr, p.S, (int64_t)n * k1, (int64_t)k1, n, k1, 0, 1, m_l, m_d, nullptr,
                           w.ms_d.as<float>(), w.ms_id.as<int>(), st));
  if (workgroups) *workgroups = p.S * p.G;
  if (queries_per_group) *queries_per_group = p.qg;
  return hipSuccess;
}

// One set of queries on one device: select per split, merge, and with `exact` flag + replay.  timing (optional):
// events around the phases, a synchronise, and the figures added to *timing.
inline hipError_t xs_search_set(XsWork &w, const XsPlan &pl, const XsRows &x, const float *d_q, int n, int k, bool exact,
                                int32_t *d_lout, float *d_dout, hipStream_t st, vaqhip_refiner_search_timing *timing) {
  const int k1 = exact ? k + 1 : k;
  int32_t *m_l = exact ? w.k1_l.as<int32_t>() : d_lout;
  float *m_d = exact ? w.k1_d.as<float>() : d_dout;
  int *list = w.list.as<int>();
  unsigned *count = reinterpret_cast<unsigned *>(list + n);
  int wgs = 0, qg = 0;
  if (timing) XS_TRY(hipEventRecord(w.ev[0], st));
  XS_TRY(xs_select_merge(w, pl, x, d_q, n, k1, m_l, m_d, st, timing ? w.ev[1] : nullptr, &wgs, &qg));
  if (timing) XS_TRY(hipEventRecord(w.ev[2], st));
  if (exact) {
    XS_TRY(vaq::launch_exact_flag(n, k, m_l, m_d, d_lout, d_dout, list, count, st));
    if (timing) XS_TRY(hipEventRecord(w.ev[3], st));
    XS_TRY(vaq::launch_exhaust_replay(d_q, n, x.D, x.rows, x.N, x.id_base, k, list, count, d_lout, d_dout, st));
  } else if (timing) {
    XS_TRY(hipEventRecord(w.ev[3], st));
  }
  if (timing) {  // (the option is a measurement: it synchronises after every set)
    XS_TRY(hipEventRecord(w.ev[4], st));
    XS_TRY(hipEventSynchronize(w.ev[4]));
    float ms[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) XS_TRY(hipEventElapsedTime(&ms[i], w.ev[i], w.ev[i + 1]));
    unsigned listed = 0;
    if (exact) XS_TRY(hipMemcpy(&listed, count, sizeof(unsigned), hipMemcpyDeviceToHost));
    timing->select_ms += ms[0];
    timing->merge_ms += ms[1];
    timing->flag_ms += ms[2];
    timing->replay_ms += ms[3];
    timing->listed_queries += (int)listed;
    timing->workgroups = wgs;
    timing->queries_per_group = qg;
  }
  return hipSuccess;
}

}  // namespace vaqhost
#endif
