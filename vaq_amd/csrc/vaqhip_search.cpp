// vaqhip_search.cpp -- the scan driver of the single-device index: search_core and its stages, the
// bucket-major rounds, the staged begin / finish, option "exact_ties", and the search entry points.
#include "vaqhip_index.h"
#include "vaq_exact.h"
#include "vaq_front.h"
#include "vaq_merge.h"
#include "vaq_ti.h"

using namespace vaqhost;

int vaqhost::check_search_args(const vaqhip_index *ix, const float *d_queries, int nq, int k, const int32_t *d_labels,
                               const float *d_dist, const char *method_err) {
  if (ix->N < 0) return fail(VAQHIP_ESTATE, "search before codes were set");
  if (ix->staged.open)
    return fail(VAQHIP_ESTATE, "a staged search is open on this index: call vaqhip_search_finish_device first");
  if (method_err) return fail(VAQHIP_ESTATE, "%s", method_err);
  if (nq < 0 || k <= 0) return fail(VAQHIP_EINVAL, "nq=%d k=%d", nq, k);
  if (k > VAQHIP_MAX_K) return fail(VAQHIP_EUNSUPPORTED, "k=%d > %d", k, VAQHIP_MAX_K);
  if (nq > 0 && (!d_queries || !d_labels || !d_dist)) return fail(VAQHIP_EINVAL, "null pointer");
  return VAQHIP_OK;
}

namespace {
// diagnostic (synchronises): what round r planned and appended
int report_bm_debug(vaqhip_index *ix, const vaq::BmParams &bp, const int *limits, int r, const BmRoundInfo &bi,
                    hipStream_t st) {
  const int chunk = bi.chunk, n = bi.n;
  std::vector<unsigned> hq((size_t)3 * chunk);
  std::vector<int> hcnt((size_t)ix->n_buckets);
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(hq.data(), ix->w_bm_query.p, hq.size() * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hcnt.data(), bp.cnt, hcnt.size() * 4, hipMemcpyDeviceToHost));
  unsigned long long handed = 0, appended = 0, over = 0, maxc = 0, pairs = 0, groups = 0, work = 0;
  for (int i = 0; i < n; i++) {
    if (hq[i] != 0xffffffffu) handed++;
    const unsigned c = hq[(size_t)chunk + i];
    appended += c;
    over += c > (unsigned)bi.cap;
    maxc = std::max<unsigned long long>(maxc, c);
  }
  std::vector<int> hb((size_t)ix->n_buckets + 1);
  HIP_TRY(hipMemcpy(hb.data(), ix->d_bstart.p, hb.size() * 4, hipMemcpyDeviceToHost));
  for (int b = 0; b < ix->n_buckets; b++) {
    pairs += hcnt[b];
    const unsigned long long g = (hcnt[b] + bi.qb - 1) / bi.qb;
    groups += g;
    work += g * (unsigned long long)(hb[b + 1] - hb[b]);
  }
  std::fprintf(stderr, "[VAQHIP_BM_DEBUG] round %d (limit %d): queries %d still open after it %llu; (query, bucket) pairs %llu, items %llu, row-steps x QB "
                       "%.3e (= %.2f %% of rows per query slot); candidates appended %llu (max %llu per query), overflowed "
                       "queries %llu; pass A units %d\n",
               r, limits[r], n, handed, pairs, groups, (double)work * bi.qb, 100.0 * (double)work * bi.qb / ((double)n * (double)ix->N),
               appended, maxc, over, bi.units);
  return VAQHIP_OK;
}

// rounds [r0, r1) of nr: plan, scan, select
int bm_run_rounds(vaqhip_index *ix, vaq::BmParams &bp, const int *limits, int r0, int r1, int nr, const BmRoundInfo &bi,
                  hipStream_t st) {
  for (int r = r0; r < r1; r++) {
    bp.retry = r + 1 < nr ? 1 : 0;
    bp.limit = limits[r];
    bp.init64 = r == 0 ? 1 : 0;
    HIP_TRY(vaq::launch_bm_plan(bp, st));
    HIP_TRY(vaq::launch_scan_bm(bp, ix->n_cu, st));
    HIP_TRY(vaq::launch_bm_select(bp, st));
    if (getenv("VAQHIP_BM_DEBUG"))
      if (int rc = report_bm_debug(ix, bp, limits, r, bi, st)) return rc;
  }
  return VAQHIP_OK;
}

// what the expensive / overflowed queries have left: the best-first form's second launch, DEFER_SLICES
// workgroups per listed query (those beyond the list's length return at once), merged into the results
int bm_fallback(vaqhip_index *ix, const vaq::ScanParams &sp, int defer_cap, int k, int32_t *labels, float *dist,
                hipStream_t st) {
  vaq::ScanParams s2 = sp;
  s2.defer_units = 0;
  s2.defer_mode = 1;
  s2.bm_done = nullptr;
  s2.qorder = nullptr;
  s2.nq = defer_cap;
  s2.n_slices = DEFER_SLICES;
  const int step2 = vaq::scan_wg_step_rows(ix->layout, ix->M);
  int64_t rows2 = (ix->N + DEFER_SLICES - 1) / DEFER_SLICES;
  rows2 = std::max<int64_t>(step2, ((rows2 + step2 - 1) / step2) * step2);
  s2.slice_rows = rows2;
  s2.slice_stride = rows2;
  s2.share_thr = 1;
  s2.final_labels = nullptr;
  s2.final_dist = nullptr;
  int grid2 = 0;
  HIP_TRY(vaq::launch_scan(s2, &grid2, st));
  HIP_TRY(vaq::launch_defer_merge(sp.defer_count, defer_cap, sp.defer_list, DEFER_SLICES, k, sp.part_d, sp.part_id,
                                  sp.part_cnt, ix->id_base, labels, dist, st));
  return VAQHIP_OK;
}

// every workspace a scan of `chunk` queries needs
int ensure_scan_workspaces(vaqhip_index *ix, const Plan &pl, int chunk, int k, bool do_project) {
  if (do_project) HIP_TRY(ix->w_qproj.ensure((size_t)chunk * ix->D * sizeof(float)));
  HIP_TRY(ix->w_lut.ensure((size_t)chunk * ix->lut_floats * sizeof(float)));
  const int nslots = std::max(pl.n_slices, pl.seed_slices);
  HIP_TRY(ix->w_part_d.ensure((size_t)chunk * nslots * k * sizeof(float)));
  HIP_TRY(ix->w_part_id.ensure((size_t)chunk * nslots * k * sizeof(int)));
  HIP_TRY(ix->w_part_cnt.ensure((size_t)chunk * nslots * sizeof(int)));
  HIP_TRY(ix->w_thr.ensure((size_t)chunk * sizeof(unsigned)));
  if (pl.cost_order) {
    HIP_TRY(ix->w_qorder.ensure((size_t)chunk * sizeof(int)));
    HIP_TRY(ix->w_cost.ensure((size_t)chunk * sizeof(unsigned long long)));
  }
  if (pl.bm) {
    const size_t K0 = (size_t)ix->n_buckets;
    HIP_TRY(ix->w_bm_small.ensure(vaq::bm_plan_small_words(ix->n_buckets) * 4));
    HIP_TRY(ix->w_bm_mask.ensure((size_t)chunk * (K0 / 32) * 4));
    HIP_TRY(ix->w_bm_qlist.ensure((size_t)chunk * K0 * sizeof(int)));
    HIP_TRY(ix->w_bm_cand_d.ensure((size_t)chunk * pl.bm_cap * sizeof(float)));
    HIP_TRY(ix->w_bm_cand_id.ensure((size_t)chunk * pl.bm_cap * sizeof(int)));
    // per query: done_key, candidate count, scale, next done_key, fresh, histogram, list keys (16 x 2 bytes)
    HIP_TRY(ix->w_bm_query.ensure((size_t)chunk * (5 + vaq::BM_HIST_BINS + 8) * 4));
    HIP_TRY(ix->w_bm_thr64.ensure((size_t)chunk * sizeof(unsigned long long)));
    // overflowed queries are finished by the best-first form's second launch
    HIP_TRY(ix->w_defer.ensure(16 + (size_t)chunk * sizeof(vaq::DeferRec)));
    HIP_TRY(ix->w_part_d.ensure((size_t)chunk * DEFER_SLICES * k * sizeof(float)));
    HIP_TRY(ix->w_part_id.ensure((size_t)chunk * DEFER_SLICES * k * sizeof(int)));
    HIP_TRY(ix->w_part_cnt.ensure((size_t)chunk * DEFER_SLICES * sizeof(int)));
  } else if (pl.defer_units > 0) {
    HIP_TRY(ix->w_defer.ensure(16 + (size_t)DEFER_CAP * sizeof(vaq::DeferRec)));
    HIP_TRY(ix->w_part_d.ensure((size_t)DEFER_CAP * DEFER_SLICES * k * sizeof(float)));
    HIP_TRY(ix->w_part_id.ensure((size_t)DEFER_CAP * DEFER_SLICES * k * sizeof(int)));
    HIP_TRY(ix->w_part_cnt.ensure((size_t)DEFER_CAP * DEFER_SLICES * sizeof(int)));
  }
  {
    const size_t ms = vaq::merge_scratch_elems(nslots, chunk, k);
    HIP_TRY(ix->w_ms_d.ensure(std::max<size_t>(ms, 1) * sizeof(float)));
    HIP_TRY(ix->w_ms_id.ensure(std::max<size_t>(ms, 1) * sizeof(int)));
  }

  if (ix->ti_T > 0) {
    HIP_TRY(ix->w_ti_order.ensure((size_t)chunk * ix->ti_T * sizeof(int)));
    HIP_TRY(ix->w_ti_qcc.ensure((size_t)chunk * ix->ti_T * sizeof(float)));
    HIP_TRY(ix->w_ti_nvisit.ensure((size_t)chunk * sizeof(int)));
  }
  return VAQHIP_OK;
}

// what every launch of a chunk's n queries shares; the fields left out are 0 / nullptr until a stage sets them
vaq::ScanParams base_scan_params(const vaqhip_index *ix, const Plan &pl, int n, int k) {
  vaq::ScanParams sp = {};
  sp.codes = ix->d_codes.as<uint32_t>();
  sp.n_rows = ix->N;
  sp.layout = ix->layout;
  sp.M = ix->M;
  sp.W = ix->W;
  sp.sub = ix->d_sub.as<vaq::SubDesc>();
  sp.first_sub = ix->d_first_sub.as<int>();
  sp.perm = ix->d_perm.as<uint32_t>();
  sp.bucket_start = ix->d_bstart.as<int>();
  sp.n_buckets = ix->n_buckets;
  sp.bucket_shift = ix->bucket_shift;
  sp.bucket_t = ix->bucket_t;
  sp.no_skip = ix->opt_no_skip;
  sp.lut = ix->w_lut.as<float>();
  sp.lut_floats = ix->lut_floats;
  sp.lds_subs = pl.lds_subs;
  sp.lut_lds_entries = pl.lut_lds_entries;
  sp.nq = n;
  sp.k = k;
  sp.kp = pl.kp;
  sp.ccap = pl.ccap;
  sp.qcap = pl.qcap;
  sp.ea = pl.ea;
  sp.seq = ix->seq;
  sp.nwaves = pl.nwaves;
  sp.g_thr = ix->w_thr.as<unsigned>();
  sp.qb = pl.qb;
  sp.part_d = ix->w_part_d.as<float>();
  sp.part_id = ix->w_part_id.as<int>();
  sp.part_cnt = ix->w_part_cnt.as<int>();
  sp.id_base = ix->id_base;
  sp.ti_rowcap = 0x7fffffff;
  return sp;
}

// the index as the replay of option "exact_ties" sees it (vaq_exact.hip) and the tables of the launch set in
// flight; a caller adds its output, or its list and chain fields
vaq::ExactParams exact_params(const vaqhip_index *ix, int k) {
  vaq::ExactParams p = {};
  p.codes = ix->d_codes.as<uint32_t>();
  p.layout = ix->layout;
  p.M = ix->M;
  p.W = ix->W;
  p.sub = ix->d_sub.as<vaq::SubDesc>();
  p.inv = ix->d_inv.as<uint32_t>();
  p.row_bucket = ix->N > 0 ? ix->d_rowbucket.as<unsigned short>() : nullptr;
  p.n_buckets = ix->n_buckets;
  p.bucket_shift = ix->bucket_shift;
  p.bucket_t = ix->bucket_t;
  p.n_rows = ix->N;
  p.lut = ix->w_lut.as<float>();
  p.lut_floats = ix->lut_floats;
  p.seq = ix->seq;
  p.k = k;
  p.id_base = ix->id_base;
  return p;
}

#if defined(VAQ_STATS) || defined(VAQ_PHASES)
int attach_stats(vaq::ScanParams &sp, hipStream_t st) {
  static unsigned long long *d_stats = nullptr;
  if (!d_stats) HIP_TRY(hipMalloc(&d_stats, 24 * sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(d_stats, 0, 24 * sizeof(unsigned long long), st));
  sp.stats = d_stats;
  return VAQHIP_OK;
}
#endif
#ifdef VAQ_PHASES
int report_phases(const vaq::ScanParams &sp, hipStream_t st) {
  unsigned long long h[11];
  HIP_TRY(hipMemcpyAsync(h, sp.stats, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const double w = (double)std::max<unsigned long long>(h[10], 1);  // reporting waves
  std::fprintf(stderr,
               "[VAQ_PHASES] cycles per wave: tables %.0f keys %.0f bootstrap %.0f round prep %.0f scan %.0f "
               "round end %.0f tail %.0f final (wave 0 works): read count %.0f cut %.0f order + write %.0f | sum %.0f\n",
               h[0] / w, h[1] / w, h[2] / w, h[3] / w, h[4] / w, h[5] / w, h[6] / w, h[8] / w, h[9] / w, h[7] / w,
               (h[0] + h[1] + h[2] + h[3] + h[4] + h[5] + h[6] + h[7] + h[8] + h[9]) / w);
  return VAQHIP_OK;
}
#endif
#ifdef VAQ_STATS
int report_stats(const vaq::ScanParams &sp, int grid, hipStream_t st) {
  unsigned long long h[24];
  HIP_TRY(hipMemcpyAsync(h, sp.stats, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const double w = (double)grid * sp.nwaves;
  std::fprintf(stderr,
               "[VAQ_STATS] per wave: steps %.1f alive_A %.1f alive_A2 %.1f drains %.2f admits %.2f folds %.2f "
               "buckets tested %.1f visited %.1f | cycles total %.0f setup %.0f stepload-wait %.0f admit %.0f "
               "(fold %.0f lock-wait %.0f) drain %.0f | best-first: bootstrap %.0f round prep %.0f final (wave 0) %.0f setup up to the tables %.0f\n",
               h[0] / w, h[1] / w, h[2] / w, h[3] / w, h[4] / w, h[5] / w, h[9] / w, h[10] / w, h[6] / w, h[11] / w,
               h[12] / w, h[7] / w, h[13] / w, h[14] / w, h[8] / w, h[15] / w, h[16] / w, (double)h[17] / grid, h[18] / w);
  return VAQHIP_OK;
}
#endif

// Multi-query passes over a streamed database: put queries with the same nearest first and
// second codes into the same pass (a pass visits the union of its queries' buckets).
// "group_queries": 1 = when it pays (streamed codes, several passes), 2 = always, 0 = never.
int group_queries(vaqhip_index *ix, const Plan &pl, int n, vaq::ScanParams &sp, hipStream_t st) {
  if (!(ix->ti_T == 0 && pl.qb > 1 && ix->M > 1 && n <= 16384 && !pl.ordered &&
        (ix->opt_group == 2 ||
         (ix->opt_group == 1 && n >= 4 * pl.qb && (double)ix->N * ((ix->total_bits + 7) / 8) > 256e6))))
    return VAQHIP_OK;
  HIP_TRY(ix->w_qorder.ensure((size_t)n * sizeof(int)));
  HIP_TRY(vaq::launch_query_order(ix->w_lut.as<float>(), ix->lut_floats, n, ix->sub[0].ncent, ix->sub[1].lut_off,
                                  ix->sub[1].ncent, ix->w_qorder.as<int>(), st));
  sp.qorder = ix->w_qorder.as<int>();
  return VAQHIP_OK;
}

// The TI form of a chunk: VAQ::search's TI branch (VAQ.cpp:799-826) then VAQ::searchTriangleInequality
// (:1540-1692).  ev: the call's timing events, or nullptr
int scan_chunk_ti(vaqhip_index *ix, const Plan &pl, const float *qp, int n, int k, vaq::ScanParams sp, int32_t *labels,
                  float *dist, hipEvent_t *ev, int *grid, hipStream_t st) {
  const int T = ix->ti_T;
  const int max_visit = ix->ti_visit < 1.0f ? (int)((float)T * ix->ti_visit) : T;  // :1548-1551
  HIP_TRY(vaq::launch_ti_plan(qp, n, ix->D, ix->ti_seg * ix->L, ix->d_ti_clusters_t.as<float>(), T,
                              ix->d_bstart.as<int>(), max_visit, k, ix->w_ti_order.as<int>(),
                              ix->w_ti_qcc.as<float>(), ix->w_ti_nvisit.as<int>(), st));
  if (ev) HIP_TRY(hipEventRecord(ev[3], st));
  sp.ti = 1;
  sp.ti_order = ix->w_ti_order.as<int>();
  sp.ti_qcc = ix->w_ti_qcc.as<float>();
  sp.ti_nvisit = ix->w_ti_nvisit.as<int>();
  sp.ti_xcc = ix->d_ti_xcc.as<float>();
  // without EA the reference never admits a row after the first k of the visiting order
  // (bsfKSquared stays 0, VAQ.cpp:1617-1686): reproduce that by taking only those rows
  sp.ti_rowcap = (ix->methods & VAQHIP_METHOD_EA) ? 0x7fffffff : k;
  sp.ti_cap = pl.ti_cap;
  sp.sqrt_out = 1;
  sp.n_slices = pl.n_slices;
  sp.share_thr = pl.n_slices > 1;
  const bool direct = pl.n_slices == 1 && ix->N > 0;
  if (direct) {
    sp.final_labels = labels;
    sp.final_dist = dist;
  }
  if (ix->N > 0) HIP_TRY(vaq::launch_scan(sp, grid, st));
  if (ev) HIP_TRY(hipEventRecord(ev[4], st));
  if (!direct)
    HIP_TRY(vaq::launch_merge(sp.part_d, sp.part_id, nullptr, ix->N > 0 ? pl.n_slices : 0, k,
                              (int64_t)pl.n_slices * k, n, k, ix->id_base, 0, labels, dist, nullptr,
                              ix->w_ms_d.as<float>(), ix->w_ms_id.as<int>(), st));
  if (ev) HIP_TRY(hipEventRecord(ev[5], st));
  return VAQHIP_OK;
}

// whether this chunk's queries are ranked by cost, and whether the table build makes the keys of that ranking (it
// does wherever its batched kernel computes table 0: from 8 centroids on; n >= COST_ORDER_MIN_QUERIES is batched)
bool ranks_queries(const vaqhip_index *ix, const Plan &pl, int n) {
  return pl.bf && pl.cost_order && pl.n_slices == 1 && ix->N > 0 && n >= COST_ORDER_MIN_QUERIES;
}
bool keys_from_table_build(const vaqhip_index *ix, const Plan &pl, int n) {
  return ranks_queries(ix, pl, n) && ix->sub[0].ncent >= 8;
}

// what runs before the scan proper: the sampling pre-pass with its threshold merge, the ranking of the queries
int seed_prepass(vaqhip_index *ix, const Plan &pl, int n, int k, vaq::ScanParams &sp, hipStream_t st) {
  if (ix->N > 0 && pl.seed_slices > 0) {
    sp.n_slices = pl.seed_slices;
    sp.slice_rows = pl.seed_rows;
    sp.slice_stride = pl.seed_stride;
    sp.share_thr = 1;
    sp.nwaves = 4;
    HIP_TRY(vaq::launch_scan(sp, nullptr, st));
    sp.nwaves = pl.nwaves;
    // (the pre-pass ran cold: its lists are full, so the plain 16-way tree, not the compacting level)
    HIP_TRY(vaq::launch_merge(sp.part_d, sp.part_id, nullptr, pl.seed_slices, k, (int64_t)pl.seed_slices * k, n,
                              k, 0, 0, nullptr, nullptr, ix->w_thr.as<unsigned>(),
                              ix->w_ms_d.as<float>(), ix->w_ms_id.as<int>(), st));
  }
  // (the ranking of the queries counts as a pre-pass in the timing: "seed_ms")
  if (ranks_queries(ix, pl, n)) {
    if (keys_from_table_build(ix, pl, n))  // (the keys are there: search_core asked the table build for them)
      HIP_TRY(vaq::launch_cost_scatter(ix->w_cost.as<unsigned long long>(), n, ix->w_qorder.as<int>(), st));
    else
      HIP_TRY(vaq::launch_cost_order(ix->w_lut.as<float>(), ix->lut_floats, n, ix->sub[0].ncent, ix->bucket_shift,
                                     ix->w_cost.as<unsigned long long>(), ix->w_qorder.as<int>(), st));
    sp.qorder = ix->w_qorder.as<int>();
  }
  return VAQHIP_OK;
}

// the geometry and the form of the full scan (and, for ordered slices, their order per query batch)
int full_scan_params(vaqhip_index *ix, const Plan &pl, int n, vaq::ScanParams &sp, int32_t *labels, float *dist,
                     hipStream_t st) {
  sp.n_slices = pl.n_slices;
  sp.slice_rows = pl.slice_rows;
  sp.slice_stride = pl.slice_rows;
  sp.share_thr = pl.n_slices > 1;
  if (pl.ordered && ix->N > 0) {
    const int nqb = (n + pl.qb - 1) / pl.qb;
    HIP_TRY(ix->w_order.ensure((size_t)nqb * pl.n_slices * sizeof(int)));
    HIP_TRY(vaq::launch_slice_order(ix->w_lut.as<float>(), ix->lut_floats, n, pl.qb, ix->d_bstart.as<int>(),
                                    ix->n_buckets, ix->bucket_shift, pl.slice_rows, pl.n_slices, ix->N,
                                    ix->w_order.as<int>(), st));
    sp.slice_order = ix->w_order.as<int>();
  }
  if (pl.n_slices == 1 && ix->N > 0) {  // the single list per query is the result
    sp.final_labels = labels;
    sp.final_dist = dist;
  }
  // best-first buckets pay when a workgroup's slice spans many buckets
  // (its ranking scratch, one word per bucket, borrows the LDS region of the lookup tables)
  sp.n_hot = (ix->opt_hot && sp.n_buckets >= 16 && sp.n_buckets <= 4096 &&
              (int64_t)sp.n_buckets <= (int64_t)(ix->layout == vaq::LAYOUT_BYTES ? ix->M * 256 : pl.lut_lds_entries) * pl.qb &&
              pl.slice_rows >= 8 * (ix->N / sp.n_buckets + 1)) ? ix->opt_hot : 0;
  sp.bf = pl.bf ? 1 : 0;
  sp.bf_carry = pl.bf_carry;
  sp.bf_pool = pl.bf_pool;
  return VAQHIP_OK;
}

// the rounds' view of a chunk whose pass A is `sp`; init64, limit and retry are set per round (bm_run_rounds)
vaq::BmParams bm_params(const vaqhip_index *ix, const Plan &pl, const vaq::ScanParams &sp, int chunk, int n, int k,
                        int32_t *labels, float *dist) {
  unsigned *qw = ix->w_bm_query.as<unsigned>();
  vaq::BmParams bp = {};
  bp.codes = sp.codes;
  bp.perm = sp.perm;
  bp.bucket_start = sp.bucket_start;
  bp.n_buckets = sp.n_buckets;
  bp.bucket_t = sp.bucket_t;
  bp.sub_start = (ix->sub_fine > 0 && ix->sub_fine + ix->bucket_t == 8 && ix->opt_bm_sub) ? ix->d_substart.as<int>() : nullptr;
  bp.M = ix->M;
  bp.lut = sp.lut;
  bp.lut_floats = sp.lut_floats;
  bp.nq = n;
  bp.k = k;
  bp.qb = pl.bm_qb;
  bp.nwaves = pl.bm_nwaves;
  bp.g_thr = sp.g_thr;
  bp.thr64 = ix->w_bm_thr64.as<unsigned long long>();
  bp.done_key = qw;
  bp.cand_cnt = qw + (size_t)chunk;
  bp.scale = reinterpret_cast<float *>(qw + (size_t)2 * chunk);
  bp.done_next = qw + (size_t)3 * chunk;
  bp.fresh = qw + (size_t)4 * chunk;
  bp.hist = qw + (size_t)5 * chunk;
  bp.qkey = reinterpret_cast<unsigned short *>(qw + (size_t)(5 + vaq::BM_HIST_BINS) * chunk);
  bp.mask = ix->w_bm_mask.as<unsigned>();
  int *sm = ix->w_bm_small.as<int>();
  const int K0 = ix->n_buckets;
  bp.cnt = sm;
  bp.qoff = sm + K0;
  bp.fill = sm + 2 * K0 + 1;
  bp.border = sm + 3 * K0 + 1;
  bp.ioff = sm + 4 * K0 + 1;
  bp.tickets = reinterpret_cast<unsigned *>(sm + vaq::bm_plan_small_words(K0) - vaq::BM_XCDS);
  bp.qlist = ix->w_bm_qlist.as<int>();
  bp.cap = pl.bm_cap;
  bp.cand_d = ix->w_bm_cand_d.as<float>();
  bp.cand_id = ix->w_bm_cand_id.as<int>();
  bp.labels = labels;
  bp.dist = dist;
  bp.id_base = ix->id_base;
  bp.defer_count = sp.defer_count;
  bp.defer_list = sp.defer_list;
  bp.defer_cap = sp.defer_cap;
  return bp;
}

// A capped first pass (bucket-major: pass A) over every query's nearest buckets; what is left in reach is handed
// over: to the rounds (bm; `bp` is made for them) or to the second launch of the "defer_units" form
int cap_first_pass(vaqhip_index *ix, const Plan &pl, bool bm, int chunk, int n, int k, int32_t *labels, float *dist,
                   vaq::ScanParams &sp, vaq::BmParams &bp, hipStream_t st) {
  sp.defer_units = pl.defer_units;
  sp.defer_cap = bm ? n : DEFER_CAP;
  sp.defer_count = ix->w_defer.as<unsigned>();
  sp.defer_list = reinterpret_cast<vaq::DeferRec *>(ix->w_defer.as<unsigned char>() + 16);
  HIP_TRY(hipMemsetAsync(sp.defer_count, 0, sizeof(unsigned), st));
  if (!bm) return VAQHIP_OK;
  sp.bm_done = ix->w_bm_query.as<unsigned>();
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sp.bm_done), 0xffffffffu, n, st));
  bp = bm_params(ix, pl, sp, chunk, n, k, labels, dist);
  HIP_TRY(hipMemsetAsync(bp.fresh, 0, (size_t)n * 4, st));
  return VAQHIP_OK;
}

// Rounds of plan, scan, select (vaq_scan_bm.hip): each query's nearest bucket [after a sampled
// threshold], its next few, then everything still in reach -- thresholds are near their final
// values before the bulk of the rows is met.  Queries whose candidate buffer overflows join
// the defer list.
// A query whose candidate buffer overflows in a round keeps its place: what was stored tightens
// its threshold and the next round plans the same buckets again; one more round (nothing to do
// when no buffer overflowed) gives the last regular round that second try too, and only what
// overflows THERE is left to the best-first form.
// stage_thr_out: a staged search (vaqhip_search_begin_device) -- the limited rounds now; the thresholds they
// leave go to the caller, who exchanges them with the other shards; vaqhip_search_finish_device goes on
// from ix->staged
int run_bucket_major(vaqhip_index *ix, vaq::BmParams &bp, const vaq::ScanParams &sp, const BmRoundInfo &bi, bool boot,
                     int k, int32_t *stage_thr_out, int32_t *d_labels, float *d_dist, hipStream_t st) {
  int limits[4], nr = 0;
  if (boot) limits[nr++] = 1;
  if (ix->opt_bm_round > 0) limits[nr++] = ix->opt_bm_round;
  limits[nr++] = 0;
  limits[nr++] = 0;
  if (!stage_thr_out) return bm_run_rounds(ix, bp, limits, 0, nr, nr, bi, st);
  int r_split = 0;
  while (r_split < nr && limits[r_split] > 0) r_split++;
  if (int rc = bm_run_rounds(ix, bp, limits, 0, r_split, nr, bi, st)) return rc;
  // (no limited round in this plan: the 64-bit words still have to be made from g_thr)
  HIP_TRY(vaq::launch_bm_thresholds(bp, nullptr, stage_thr_out, r_split == 0 ? 1 : 0, st));
  StagedState &ss = ix->staged;
  ss.open = true;
  ss.bp = bp;
  ss.sp = sp;
  ss.bi = bi;
  ss.k = k;
  ss.defer_cap = sp.defer_cap;
  ss.nr = nr;
  ss.r_next = r_split;
  for (int r = 0; r < 4; r++) ss.limits[r] = limits[r];
  ss.labels = d_labels;
  ss.dist = d_dist;
  return VAQHIP_OK;
}

// what vaqhip_last_timing reports of the plan: the TI form of a chunk, and the plain one
void fill_timing_ti(vaqhip_timing &tm, const Plan &pl, int n, int grid) {
  tm.seed_slices = 0;
  tm.early_abandon = pl.ea;
  tm.queries_per_pass = 1;
  tm.slices = pl.n_slices;
  tm.workgroups = grid;
  tm.passes = n;
  tm.lds_bytes = (int)pl.lds;
}
void fill_timing(vaqhip_timing &tm, const Plan &pl, int n, int grid, bool bm, bool defer) {
  tm.seed_slices = pl.seed_slices;
  tm.early_abandon = pl.ea;
  tm.best_first = pl.bf ? 1 : 0;
  tm.deferred_queries = (defer || bm) ? 0 : -1;  // (bucket-major: queries whose candidate buffer overflowed)
  tm.bucket_major = bm ? 1 : 0;
  tm.queries_per_pass = pl.qb;
  tm.slices = pl.n_slices;
  tm.workgroups = grid;
  tm.passes = (n + pl.qb - 1) / pl.qb;
  tm.lds_bytes = (int)pl.lds;
}

// core: device pointers in, device pointers out, enqueue only
int search_core(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                int32_t *d_labels, float *d_dist, hipStream_t st, int32_t *stage_thr_out = nullptr) {
  const char *method_err = nullptr;
  if (((ix->methods & VAQHIP_METHOD_TI) != 0) != (ix->ti_T > 0))
    method_err = ix->ti_T > 0 ? "the rows are grouped by TI cluster: the method must include TI"
                              : "method TI needs vaqhip_index_set_ti_clusters first";
  if (int rc = check_search_args(ix, d_queries, nq, k, d_labels, d_dist, method_err)) return rc;
  if (nq == 0) return VAQHIP_OK;
  WS_SCOPE(ws, ix, st);
  bool timing = ix->opt_timing != 0;
  hipEvent_t *ev = nullptr;
  if (timing) {
    if (int rc = ensure_events(ix)) return rc;
    if (ix->ev_used >= vaqhip_index::EV_SETS) timing = false;  // ring full: stop recording
    else ev = ix->ev.data() + (size_t)ix->ev_used * 6;
  }
  vaqhip_timing tm = {};
  tm.deferred_queries = -1;
  Plan pl;
  const bool ti = ix->ti_T > 0;
  const int chunk = std::min(nq, QUERY_CHUNK);
  if (int rc = ti ? make_ti_plan(ix, chunk, k, &pl) : make_plan(ix, chunk, k, &pl)) return rc;
  if (stage_thr_out) {
    if (!(pl.bm && pl.bf && pl.n_slices == 1 && ix->N > 0 && nq <= QUERY_CHUNK && !ti))
      return fail(VAQHIP_EUNSUPPORTED, "a staged search needs the bucket-major rounds (streamed byte codes, >= 8 queries, "
                                       "at most %d per call)", QUERY_CHUNK);
    timing = false;
  }
  // (BitVecEngine::queryLUT projects with checking, BitVecEngine.hpp:1226: non-finite coordinates -> 0,
  //  which needs a pass over the queries even without a rotation)
  const bool do_project = !projected && (ix->has_eig || ix->seq);
  if (int rc = ensure_scan_workspaces(ix, pl, chunk, k, do_project)) return rc;
  if (timing && nq > chunk)
    return fail(VAQHIP_EUNSUPPORTED, "timing supports at most %d queries per call", QUERY_CHUNK);

  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    const float *dq = d_queries + (size_t)q0 * ix->D;
    const float *qp = dq;
    int32_t *labels = d_labels + (size_t)q0 * k;
    float *dist = d_dist + (size_t)q0 * k;
    if (timing) HIP_TRY(hipEventRecord(ev[0], st));
    if (do_project) {
      HIP_TRY(vaq::launch_project(dq, n, ix->D, ix->has_eig ? ix->d_eig.as<float>() : nullptr, ix->w_qproj.as<float>(), st,
                                  ix->seq ? 1 : 0));
      qp = ix->w_qproj.as<float>();
    }
    if (timing) HIP_TRY(hipEventRecord(ev[1], st));
    // (a ranking of the queries takes its keys from the table build: seed_prepass only places the queries)
    const vaq::CostKeys ck = {ix->w_cost.as<unsigned long long>(), ix->sub[0].ncent, ix->bucket_shift};
    HIP_TRY(vaq::launch_lut_build(qp, n, ix->D, ix->M, ix->L, ix->d_sub.as<vaq::SubDesc>(),
                                  ix->d_cent_t.as<float>(), ix->lut_floats, 1 << ix->max_bits, ix->w_lut.as<float>(), st,
                                  1 << ix->min_bits, !ti && keys_from_table_build(ix, pl, n) ? &ck : nullptr));
    if (timing) HIP_TRY(hipEventRecord(ev[2], st));
    vaq::ScanParams sp = base_scan_params(ix, pl, n, k);
#if defined(VAQ_STATS) || defined(VAQ_PHASES)
    if (int rc = attach_stats(sp, st)) return rc;
#endif
    int grid = 0;
    if (int rc = group_queries(ix, pl, n, sp, st)) return rc;
    // shared admission thresholds start at heap_heapify's neutral FLT_MAX (0x7f7fffff); a query
    // served by ONE workgroup and no pre-pass never reads the word (share_thr = 0 below)
    if (pl.n_slices > 1 || pl.seed_slices > 0 || pl.bm)
      HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ix->w_thr.p), 0x7f7fffff, n, st));
    if (ti) {
      if (int rc = scan_chunk_ti(ix, pl, qp, n, k, sp, labels, dist, timing ? ev : nullptr, &grid, st)) return rc;
      fill_timing_ti(tm, pl, n, grid);
      continue;
    }
    if (int rc = seed_prepass(ix, pl, n, k, sp, st)) return rc;
    if (timing) HIP_TRY(hipEventRecord(ev[3], st));
    if (int rc = full_scan_params(ix, pl, n, sp, labels, dist, st)) return rc;
    const bool direct = pl.n_slices == 1 && ix->N > 0;
    const bool bm = pl.bm && pl.bf && direct;
    const bool defer = pl.bf && pl.defer_units > 0 && direct && !bm;
    vaq::BmParams bp = {};
    if (bm || defer)
      if (int rc = cap_first_pass(ix, pl, bm, chunk, n, k, labels, dist, sp, bp, st)) return rc;
    if (bm && pl.bm_boot) {
      // no best-first pass: a threshold per query from a sample of its nearest rows, then the
      // nearest bucket of every query is the first bucket-major round
      HIP_TRY(vaq::launch_bm_boot(bp, ix->N, st));
    } else if (ix->N > 0) {
      HIP_TRY(vaq::launch_scan(sp, &grid, st));
    }
    if (bm) {
      const BmRoundInfo bi = {chunk, n, pl.bm_cap, pl.bm_qb, pl.defer_units};
      if (int rc = run_bucket_major(ix, bp, sp, bi, pl.bm_boot, k, stage_thr_out, d_labels, d_dist, st)) return rc;
      if (stage_thr_out) {
        ix->last = tm;
        return ws.finish();
      }
    }
    if (defer || bm)
      if (int rc = bm_fallback(ix, sp, sp.defer_cap, k, labels, dist, st)) return rc;
#ifdef VAQ_PHASES
    if (pl.bf)
      if (int rc = report_phases(sp, st)) return rc;
#endif
#ifdef VAQ_STATS
    if (int rc = report_stats(sp, grid, st)) return rc;
#endif
    if (timing) HIP_TRY(hipEventRecord(ev[4], st));
    if (!direct)
      // after a seeded scan most lists are empty: let the first merge level gather by the counts
      HIP_TRY(vaq::launch_merge(sp.part_d, sp.part_id, (pl.seed_slices > 0 || pl.ordered) ? sp.part_cnt : nullptr,
                                ix->N > 0 ? pl.n_slices : 0, k, (int64_t)pl.n_slices * k, n, k, ix->id_base, 0, labels,
                                dist, nullptr, ix->w_ms_d.as<float>(), ix->w_ms_id.as<int>(), st));
    if (timing) HIP_TRY(hipEventRecord(ev[5], st));
    fill_timing(tm, pl, n, grid, bm, defer);
  }
  tm.n_searches = 0;
  ix->last = tm;
  if (timing) ix->ev_used++;
  return ws.finish();
}

// original row -> bucketed row and bucket, for the replay of option "exact_ties": made at the first such search
// after the codes changed
int ensure_inverse_perm(vaqhip_index *ix, hipStream_t st) {
  if (ix->N <= 0 || ix->inv_valid) return VAQHIP_OK;
  HIP_TRY(ix->d_inv.ensure((size_t)ix->N * sizeof(uint32_t)));
  HIP_TRY(ix->d_rowbucket.ensure((size_t)ix->N * sizeof(unsigned short)));
  HIP_TRY(vaq::launch_inverse_perm(ix->d_perm.as<uint32_t>(), ix->N, ix->d_inv.as<uint32_t>(), ix->d_bstart.as<int>(),
                                   ix->n_buckets, ix->d_rowbucket.as<unsigned short>(), st));
  ix->inv_valid = true;
  return VAQHIP_OK;
}

// the reference's member order of a TI index, for option "exact_ties": made at the first such search after the
// rows were (re)grouped
int ensure_ti_walk(vaqhip_index *ix, hipStream_t st) {
  if (ix->N <= 0 || ix->ti_walk_valid) return VAQHIP_OK;
  HIP_TRY(ix->d_ti_walk.ensure((size_t)ix->N * sizeof(uint32_t)));
  HIP_TRY(vaq::ti_build_walk(ix->d_perm.as<uint32_t>(), ix->d_bstart.as<int>(), ix->d_ti_xcc.as<float>(), ix->N, ix->ti_T,
                             ix->d_ti_walk.as<uint32_t>(), st));  // synchronises
  ix->ti_walk_valid = true;
  return VAQHIP_OK;
}

// Option "exact_ties" on a TI index: every query is answered by a replay of VAQ::searchTriangleInequality's walk
// (vaq_exact.hip) over the reference's own cluster order and member order (vaq_ti.hip).  Timing: the plan is
// reported as seed_ms, the replay as scan_ms; nothing is merged, so merge_ms is always 0 on this path (its two
// events are recorded back to back), and the plan figures are one workgroup and one pass per query.
int search_ti_exact(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected, int32_t *d_labels,
                    float *d_dist, hipStream_t st) {
  if (int rc = check_search_args(ix, d_queries, nq, k, d_labels, d_dist, nullptr)) return rc;
  if (nq == 0) return VAQHIP_OK;
  WS_SCOPE(ws, ix, st);
  bool timing = ix->opt_timing != 0;
  hipEvent_t *ev = nullptr;
  if (timing) {
    if (int rc = ensure_events(ix)) return rc;
    if (ix->ev_used >= vaqhip_index::EV_SETS) timing = false;  // ring full: stop recording
    else ev = ix->ev.data() + (size_t)ix->ev_used * 6;
  }
  const int chunk = std::min(nq, QUERY_CHUNK);
  if (timing && nq > chunk) return fail(VAQHIP_EUNSUPPORTED, "timing supports at most %d queries per call", QUERY_CHUNK);
  const int T = ix->ti_T;
  const bool do_project = !projected && ix->has_eig;
  if (do_project) HIP_TRY(ix->w_qproj.ensure((size_t)chunk * ix->D * sizeof(float)));
  HIP_TRY(ix->w_lut.ensure((size_t)chunk * ix->lut_floats * sizeof(float)));
  HIP_TRY(ix->w_ti_order.ensure((size_t)chunk * T * sizeof(int)));
  HIP_TRY(ix->w_ti_qcc.ensure((size_t)chunk * T * sizeof(float)));
  HIP_TRY(ix->w_ti_nvisit.ensure((size_t)chunk * sizeof(int)));
  if (int rc = ensure_ti_walk(ix, st)) return rc;
  const int max_visit = ix->ti_visit < 1.0f ? (int)((float)T * ix->ti_visit) : T;  // VAQ.cpp:1548-1551
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    const float *qp = d_queries + (size_t)q0 * ix->D;
    if (timing) HIP_TRY(hipEventRecord(ev[0], st));
    if (do_project) {
      HIP_TRY(vaq::launch_project(qp, n, ix->D, ix->d_eig.as<float>(), ix->w_qproj.as<float>(), st, 0));
      qp = ix->w_qproj.as<float>();
    }
    if (timing) HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(vaq::launch_lut_build(qp, n, ix->D, ix->M, ix->L, ix->d_sub.as<vaq::SubDesc>(), ix->d_cent_t.as<float>(),
                                  ix->lut_floats, 1 << ix->max_bits, ix->w_lut.as<float>(), st, 1 << ix->min_bits));
    if (timing) HIP_TRY(hipEventRecord(ev[2], st));
    HIP_TRY(vaq::launch_ti_plan(qp, n, ix->D, ix->ti_seg * ix->L, ix->d_ti_clusters_t.as<float>(), T,
                                ix->d_bstart.as<int>(), max_visit, k, ix->w_ti_order.as<int>(), ix->w_ti_qcc.as<float>(),
                                ix->w_ti_nvisit.as<int>(), st, 1));
    if (timing) HIP_TRY(hipEventRecord(ev[3], st));
    vaq::TiExactParams tp = {};
    tp.x = exact_params(ix, k);
    tp.x.labels = d_labels + (size_t)q0 * k;
    tp.x.dist = d_dist + (size_t)q0 * k;
    tp.perm = ix->d_perm.as<uint32_t>();
    tp.walk = ix->d_ti_walk.as<uint32_t>();
    tp.start = ix->d_bstart.as<int>();
    tp.xcc = ix->d_ti_xcc.as<float>();
    tp.T = T;
    tp.order = ix->w_ti_order.as<int>();
    tp.qcc = ix->w_ti_qcc.as<float>();
    tp.nvisit = ix->w_ti_nvisit.as<int>();
    tp.ea = (ix->methods & VAQHIP_METHOD_EA) ? 1 : 0;
    HIP_TRY(vaq::launch_ti_exact_replay(tp, n, st));
    if (timing) {
      HIP_TRY(hipEventRecord(ev[4], st));
      HIP_TRY(hipEventRecord(ev[5], st));
    }
  }
  vaqhip_timing tm = {};
  tm.deferred_queries = -1;
  tm.queries_per_pass = 1;
  tm.slices = 1;
  tm.workgroups = std::min(nq, chunk);
  tm.passes = std::min(nq, chunk);
  ix->last = tm;
  if (timing) ix->ev_used++;
  return ws.finish();
}

// Option "exact_ties": the scan runs with k + 1; queries whose k + 1 smallest distances are distinct
// have a unique answer and are copied out, the others are replayed through the reference's heap in
// original row order (vaq_exact.hip).  One internal launch set (<= QUERY_CHUNK queries) at a time: the
// replay reads that set's lookup tables.
int search_device_locked(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                         int32_t *d_labels, float *d_dist, hipStream_t st) {
  if (fast_only(ix)) return search_fast(ix, d_queries, nq, k, projected, d_labels, d_dist, st);
  if (ix->opt_exact && !ix->sharded && ix->ti_T > 0 && (ix->methods & VAQHIP_METHOD_TI))
    return search_ti_exact(ix, d_queries, nq, k, projected, d_labels, d_dist, st);
  const bool exact =ix->opt_exact && ix->ti_T == 0 && nq > 0 && k > 0 && k < VAQHIP_MAX_K && ix->N >= 0 &&
                     d_queries && d_labels && d_dist;
  if (!exact) return search_core(ix, d_queries, nq, k, projected, d_labels, d_dist, st);
  const int chunk = std::min(nq, QUERY_CHUNK);
  HIP_TRY(ix->w_ex_labels.ensure((size_t)chunk * (k + 1) * sizeof(int32_t)));
  HIP_TRY(ix->w_ex_dist.ensure((size_t)chunk * (k + 1) * sizeof(float)));
  HIP_TRY(ix->w_ex_list.ensure((size_t)chunk * sizeof(int) + 16));
  if (int rc = ensure_inverse_perm(ix, st)) return rc;
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = std::min(chunk, nq - q0);
    if (int rc = search_core(ix, d_queries + (size_t)q0 * ix->D, n, k + 1, projected, ix->w_ex_labels.as<int32_t>(),
                             ix->w_ex_dist.as<float>(), st))
      return rc;
    WS_SCOPE(ws, ix, st);
    vaq::ExactParams p = exact_params(ix, k);
    p.labels = d_labels + (size_t)q0 * k;
    p.dist = d_dist + (size_t)q0 * k;
    int *list = reinterpret_cast<int *>(ix->w_ex_list.as<unsigned char>() + 16);
    unsigned *count = ix->w_ex_list.as<unsigned>();
    p.list = list;
    p.count = count;
    HIP_TRY(vaq::launch_exact_flag(n, k, ix->w_ex_labels.as<int32_t>(), ix->w_ex_dist.as<float>(), p.labels, p.dist, list,
                                   count, st));
    HIP_TRY(vaq::launch_exact_replay(p, n, st));
    if (int rc = ws.finish()) return rc;
  }
  return VAQHIP_OK;
}

// second half of a staged search: take over the exchanged thresholds, the remaining rounds, the fallback
int search_finish_locked(vaqhip_index *ix, const int32_t *d_thr_in, hipStream_t st) {
  StagedState &ss = ix->staged;
  if (!ss.open) return fail(VAQHIP_ESTATE, "no staged search is open on this index");
  WS_SCOPE(ws, ix, st);
  ss.open = false;
  if (d_thr_in) HIP_TRY(vaq::launch_bm_thresholds(ss.bp, d_thr_in, nullptr, 0, st));
  if (int rc = bm_run_rounds(ix, ss.bp, ss.limits, ss.r_next, ss.nr, ss.nr, ss.bi, st)) return rc;
  if (int rc = bm_fallback(ix, ss.sp, ss.defer_cap, ss.k, ss.labels, ss.dist, st)) return rc;
  return ws.finish();
}

int search_host(vaqhip_index *ix, const float *queries, int nq, int k, int projected, int32_t *labels,
                float *distances) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (nq < 0 || k <= 0) return fail(VAQHIP_EINVAL, "nq=%d k=%d", nq, k);
  if (nq == 0) return VAQHIP_OK;
  if (!queries || !labels || !distances) return fail(VAQHIP_EINVAL, "null pointer");
  ENTRY(ix);
  const size_t qbytes = (size_t)nq * ix->D * sizeof(float);
  const size_t rbytes = (size_t)nq * k * sizeof(float);
  HIP_TRY(ix->w_q.ensure(qbytes));
  HIP_TRY(ix->w_labels.ensure(rbytes));
  HIP_TRY(ix->w_dist.ensure(rbytes));
  WS_SCOPE(ws, ix, ix->stream);
  HIP_TRY(hipMemcpyAsync(ix->w_q.p, queries, qbytes, hipMemcpyHostToDevice, ix->stream));
  int rc = search_device_locked(ix, ix->w_q.as<float>(), nq, k, projected, ix->w_labels.as<int32_t>(),
                                ix->w_dist.as<float>(), ix->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(labels, ix->w_labels.p, rbytes, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipMemcpyAsync(distances, ix->w_dist.p, rbytes, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return ws.finish();
}

} // namespace

extern "C" {
int vaqhip_search_device(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                         int32_t *d_labels, float *d_dist, void *stream) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  ENTRY(ix);
  return search_device_locked(ix, d_queries, nq, k, projected, d_labels, d_dist,
                              static_cast<hipStream_t>(stream));
}

int vaqhip_search(vaqhip_index *ix, const float *queries, int nq, int k, int32_t *labels,
                  float *distances) {
  return search_host(ix, queries, nq, k, 0, labels, distances);
}

int vaqhip_search_projected(vaqhip_index *ix, const float *qproj, int nq, int k, int32_t *labels,
                            float *distances) {
  return search_host(ix, qproj, nq, k, 1, labels, distances);
}

int vaqhip_search_staged_supported(vaqhip_index *ix, int nq, int k) {
  if (!ix || nq <= 0 || k <= 0 || k > VAQHIP_MAX_K) return 0;
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->N <= 0 || ix->ti_T > 0 || nq > QUERY_CHUNK || ix->opt_exact || fast_only(ix)) return 0;
  Plan pl;
  if (make_plan(ix, nq, k, &pl)) return 0;
  return (pl.bm && pl.bf && pl.n_slices == 1) ? 1 : 0;
}

int vaqhip_search_begin_device(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                               int32_t *d_labels, float *d_distances, int32_t *d_thresholds_out, void *stream) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (!d_thresholds_out) return fail(VAQHIP_EINVAL, "null pointer");
  ENTRY(ix);
  if (ix->opt_exact) return fail(VAQHIP_EUNSUPPORTED, "exact_ties is a property of ONE index; shards merge by (distance, label)");
  if (fast_only(ix)) return fail(VAQHIP_EUNSUPPORTED, "method FAST has no staged form");
  return search_core(ix, d_queries, nq, k, projected, d_labels, d_distances, static_cast<hipStream_t>(stream),
                     d_thresholds_out);
}

int vaqhip_search_finish_device(vaqhip_index *ix, const int32_t *d_thresholds_in, void *stream) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  ENTRY(ix);
  return search_finish_locked(ix, d_thresholds_in, static_cast<hipStream_t>(stream));
}

// ---- "exact_ties" across the shards of a multi-device index (vaqhip_internal.h) ----
int vaqhip_internal_query_chunk(void) { return QUERY_CHUNK; }

int vaqhip_internal_exact_applies(vaqhip_index *ix, int k) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lk(ix->mu);
  return ix->opt_exact && !fast_only(ix) && ix->ti_T == 0 && k > 0 && k < VAQHIP_MAX_K ? 1 : 0;
}

void vaqhip_internal_set_sharded(vaqhip_index *ix, int sharded) {
  if (!ix) return;
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->sharded = sharded != 0;
}

int vaqhip_internal_exact_state_words(vaqhip_index *ix, int k) {
  if (!ix || k <= 0) return 0;
  std::lock_guard<std::mutex> lk(ix->mu);
  return vaq::exact_state_words(k, ix->seq);
}

int vaqhip_internal_search_plain_device(vaqhip_index *ix, const float *d_queries, int nq, int k, int projected,
                                        int32_t *d_labels, float *d_dist, void *stream) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (nq > QUERY_CHUNK) return fail(VAQHIP_EINVAL, "nq=%d > %d", nq, QUERY_CHUNK);
  ENTRY(ix);
  if (fast_only(ix)) return fail(VAQHIP_EUNSUPPORTED, "method FAST has no chained form");
  return search_core(ix, d_queries, nq, k, projected, d_labels, d_dist, static_cast<hipStream_t>(stream));
}

int vaqhip_internal_exact_flag_device(int device, int nq, int k, const int32_t *d_in_labels, const float *d_in_dist,
                                      int32_t *d_labels, float *d_dist, int *d_list, unsigned *d_count, void *stream) {
  if (nq <= 0 || k <= 0 || !d_in_labels || !d_in_dist || !d_labels || !d_dist || !d_list || !d_count)
    return fail(VAQHIP_EINVAL, "bad arguments");
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", device);
  HIP_TRY(vaq::launch_exact_flag(nq, k, d_in_labels, d_in_dist, d_labels, d_dist, d_list, d_count,
                                 static_cast<hipStream_t>(stream)));
  return VAQHIP_OK;
}

int vaqhip_internal_exact_link_device(vaqhip_index *ix, int k, int64_t row0, const int *d_list, const unsigned *d_count,
                                      int e0, int n_entries, const int32_t *d_state_in, int32_t *d_state_out,
                                      void *stream) {
  if (!ix) return fail(VAQHIP_EINVAL, "index is null");
  if (k <= 0 || k >= VAQHIP_MAX_K || row0 < 0 || e0 < 0 || n_entries < 0 || !d_list || !d_count || !d_state_out)
    return fail(VAQHIP_EINVAL, "bad arguments");
  ENTRY(ix);
  if (ix->N < 0) return fail(VAQHIP_ESTATE, "search before codes were set");
  if (ix->ti_T > 0 || fast_only(ix)) return fail(VAQHIP_EUNSUPPORTED, "no replay for this method");
  hipStream_t st = static_cast<hipStream_t>(stream);
  WS_SCOPE(ws, ix, st);
  if (int rc = ensure_inverse_perm(ix, st)) return rc;
  vaq::ExactParams p = exact_params(ix, k);
  p.list = d_list;
  p.count = d_count;
  p.chain = 1;
  p.row0 = row0;
  p.e0 = e0;
  p.state_in = d_state_in;
  p.state_out = d_state_out;
  HIP_TRY(vaq::launch_exact_replay(p, n_entries, st));
  return ws.finish();
}

int vaqhip_internal_exact_finish_device(int device, const int32_t *d_state, const int *d_list, const unsigned *d_count,
                                        int n_entries, int seq, int k, int32_t *d_labels, float *d_dist, void *stream) {
  if (n_entries < 0 || k <= 0 || k >= VAQHIP_MAX_K || !d_state || !d_list || !d_count || !d_labels || !d_dist)
    return fail(VAQHIP_EINVAL, "bad arguments");
  DeviceGuard g(device);
  if (!g.ok) return fail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", device);
  HIP_TRY(vaq::launch_exact_finish(d_state, d_list, d_count, n_entries, seq, k, d_labels, d_dist,
                                   static_cast<hipStream_t>(stream)));
  return VAQHIP_OK;
}
} // extern "C"
