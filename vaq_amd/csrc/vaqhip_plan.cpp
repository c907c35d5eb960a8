// vaqhip_plan.cpp -- the launch planner of the single-device index: which form of the scan serves a
// call, with what geometry.  The thresholds are measurements; the comments next to them are the record.
#include "vaqhip_index.h"

using namespace vaqhost;

namespace {

constexpr size_t LDS_LIMIT = 160 * 1024;       // per CU on gfx950
#ifndef VAQ_BF_WAVES_PER_SIMD
#define VAQ_BF_WAVES_PER_SIMD 8
#endif
constexpr int BF_WAVES_PER_CU = 4 * VAQ_BF_WAVES_PER_SIMD;  // what the best-first kernels' register budget admits
constexpr size_t LDS_GRANULE = 1280;           // allocation unit assumed when counting resident workgroups
constexpr int64_t MIN_SLICE_ROWS = 16384;      // do not cut slices finer than this
constexpr double BM_QB2_MAX_BYTES = 4.5e9;  // bucket-major rounds, 16-byte rows: two queries per group up to this many code bytes
// Best-first form, one workgroup per query, option "defer_units" (OFF by default): a first round
// takes at most that many work units and what is still in reach after it is scanned by DEFER_SLICES
// workgroups per query in a second launch (at most DEFER_CAP queries; the others scan on in place).
// A query's cost spans 6x (C2: 318 wave steps on average, 1857 for the top 1 %) and a launch ends
// with its most expensive workgroups -- but the second launch has a tail of its own (a workgroup's
// setup, first round and final cut: ~0.1 ms with the chip nearly empty) and every handed-over query
// pays the per-workgroup costs twice more: C2 0.715 ms without, 0.74-0.77 with 48-128 units, 0.88
// with 24 (tools/exp_lpt_oracle.py has the cost statistics).  Kept as an option; -1 = the automatic
// rule below, which no default selects.
constexpr int DEFER_MIN_QUERIES = 4096, DEFER_UNITS = 96;  // (DEFER_SLICES, DEFER_CAP: vaqhip_index.h)
constexpr int64_t SEED_MIN_ROWS = 1 << 21;     // below this a scan is too short to need seeding
constexpr int64_t SEED_MIN_SLICES = 256;       // fewer, longer slices warm themselves up
constexpr int BF_STREAMED_MIN_QUERIES = 128;    // from here on the best-first form also takes streamed databases
constexpr int INPLACE_MAX_BATCHES = 4;         // query batches per scan up to which EA_INPLACE is chosen
// Bucket-major second pass (vaq_scan_bm.hip): a streamed database and so many queries that every
// bucket is wanted by several of them.  Pass A (best-first, one workgroup per query) is cut after
// about one average bucket's worth of work units; BM_CAND_CAP candidate slots per query.
constexpr int BM_MIN_QUERIES = 8;   // (125M x 16 B: 1 / 2 / 8 / 32 queries 0.45 / 0.58 / 1.15 / 2.44 ms with the shared-stream forms,
                                    //  0.63 / 0.63 / 0.72 / 0.87 ms with the rounds -- a chain of ~20 launches is their floor)
constexpr int BM_CAND_CAP = 4096;
constexpr int BM_QB = 4, BM_NWAVES = 16;
constexpr int BM_BOOT_MIN_UNITS = 24;

} // namespace

int vaqhost::make_plan(const vaqhip_index *ix, int nq, int k, Plan *pl) {
  // early-abandon form: 1 = queue, 2 = in place, 3 = auto (in place when few
  // query batches stream a database that does not fit the 256 MB Infinity
  // Cache, i.e. the scan is HBM-bound rather than instruction-bound)
  int ea = ix->opt_ea;
  if (ea == 3) {
    const double stream_bytes = (double)ix->N * ((ix->total_bits + 7) / 8);
    const int nqb_est = (nq + 1) / 2;
    ea = (stream_bytes > 256e6 && nqb_est <= INPLACE_MAX_BATCHES) ? vaq::EA_INPLACE : vaq::EA_QUEUE;
  }
  // default queries per pass: 2 for byte codes (one ds_read_b64 serves both), 1 for the
  // bit-packed path (more whole buckets are skipped when only one query has to agree)
  // ... and 1 as well for byte codes that stay cache-resident (<= 128 MB): sharing the code
  // stream between two queries buys nothing there, per-query bucket skipping does
  const bool resident = (double)ix->N * ((ix->total_bits + 7) / 8) <= 128e6;
  // ... and 4 for a streamed (non-resident) byte-coded database once there are enough queries to
  // fill the passes (250M x 16 B: 256 queries 18.4 -> 15.4 ms, 32 queries 3.6 -> 3.4 ms; no gain
  // below)
  int qb = ix->opt_qb > 0 ? ix->opt_qb
                          : ((ix->layout == vaq::LAYOUT_BYTES && !resident) ? (nq >= 32 ? 4 : 2) : 1);
  // ... but with MANY queries the best-first form (one query per workgroup, vaq_scan_bf.h) wins on
  // streamed databases as well: each query reads only the buckets in its own reach, nearest first,
  // and concurrent workgroups share what they read through L2 / Infinity Cache.  1B x 16 B encoded:
  // 2048 queries 367 -> 201 ms, 10 k queries 1275 -> 807 ms; 250M, 256 queries 14.5 -> 9.7 ms; at 64
  // queries the two are level (8.0 vs 8.3 ms at 500M) and below that the shared stream wins.
  const bool bf_streamed = ix->opt_qb == 0 && ix->opt_bf && !resident && nq >= BF_STREAMED_MIN_QUERIES && ea == vaq::EA_QUEUE &&
                           ix->ti_T == 0 && !ix->opt_order &&
                           vaq::scan_bf_supported(ix->layout, ix->M, 1, ea, ix->n_buckets, ix->seq);
  if (bf_streamed) qb = 1;
  // ... and with MORE queries still, several of them want every bucket: after a capped best-first
  // pass (one workgroup per query, its nearest buckets) the rest is scanned bucket-major, each
  // bucket streamed once for all the queries that reach it (vaq_scan_bm.hip)
  const bool bm = ix->opt_bm && ix->opt_bf && ix->ti_T == 0 && !ix->opt_order && !ix->opt_no_skip && ix->opt_slices <= 1 &&
                  (ix->opt_qb == 0 || ix->opt_bm == 2) && (ea == vaq::EA_QUEUE || ix->opt_bm == 2) && k <= 256 && ix->N > 0 &&
                  ((!resident && nq >= BM_MIN_QUERIES) || ix->opt_bm == 2) &&
                  vaq::scan_bm_supported(ix->layout, ix->M, ix->n_buckets, ix->bucket_shift, ix->seq, k) &&
                  vaq::scan_bf_supported(ix->layout, ix->M, 1, vaq::EA_QUEUE, ix->n_buckets, ix->seq);
  if (bm) {
    qb = 1;
    ea = vaq::EA_QUEUE;
  }
  if (nq < qb) qb = nq >= 2 ? 2 : 1;
  // Pick the workgroup size that puts the most wavefronts on a CU: the LUT and
  // the selection state are per workgroup, the survivor queues per wave; a CU
  // holds 160 KB of LDS and 32 waves (the scan kernels stay within 64 VGPRs
  // for Qb <= 2; Qb = 4 needs about twice that, i.e. half the waves).
  const int wave_cap = qb <= 2 ? 32 : 24;
  // LUT tables are staged in LDS for a prefix of the subspaces (all of them whenever they
  // fit; the byte-code kernels need all).  The bit-packed kernel reads the tail tables from
  // global memory, so big allocations (32 x up to 13 bits) still run; only table 0
  // (bucket bounds) must be resident.
  const int need = ix->layout == vaq::LAYOUT_BYTES ? ix->M : 1;
  int best_nw = 0, best_waves = 0, subs = ix->M, entries = ix->lut_floats;
  for (;;) {
    for (subs = ix->M; subs >= need; subs--) {
      entries = subs == ix->M ? ix->lut_floats : ix->sub[subs].lut_off;
      best_nw = 0;
      best_waves = 0;
      for (int nw : {4, 8, 16}) {
        if (ix->opt_nwaves > 0 && nw != ix->opt_nwaves) continue;
        const size_t lds = vaq::scan_lds_bytes(ix->layout, ix->M, entries, qb, k, ea, nw, ix->n_buckets,
                                               ix->bucket_shift, ix->bucket_t);
        if (lds > LDS_LIMIT) continue;
        const int wgs = (int)std::min<size_t>(LDS_LIMIT / lds, (size_t)(wave_cap / nw));
        // 16 waves share one admission lock and one ticket: measured much slower than 8 at equal
        // residency (C3: 5.8 vs 3.1 ms), so they must buy > 1.5x the waves to be chosen
        // (not when every bucket is streamed in place, where the lock is taken for admitted rows
        //  only and the waves just keep loads in flight: 1B rows, 16 waves x 2 workgroups per CU
        //  2.78 ms, 8 x 3 2.90 ms; with bucket skipping on it is the other way round, 250M rows x 2
        //  queries 0.27 vs 0.23 ms)
        const bool streaming = ea == vaq::EA_INPLACE && ix->opt_no_skip;
        const int score = (nw == 16 && !streaming) ? (wgs * nw * 2) / 3 : wgs * nw;
        if (score > best_waves) { best_waves = score; best_nw = nw; }
      }
      if (best_nw) break;
    }
    if (best_nw && subs < ix->M && qb > 2) best_nw = 0;  // spilled tables: kernels exist for Qb <= 2 only
    if (best_nw) break;
    if (qb > 1) qb >>= 1;
    else
      return fail(VAQHIP_EUNSUPPORTED,
                  "the lookup tables of the first %d subspaces plus top-%d buffers do not fit %zu B of LDS",
                  need, k, LDS_LIMIT);
  }
  pl->lds_subs = subs;
  pl->lut_lds_entries = entries;
  pl->qb = qb;
  pl->ea = ea;
  pl->nwaves = best_nw;
  vaq::scan_geometry(ix->layout, ix->M, k, ea, &pl->kp, &pl->ccap, &pl->qcap);
  pl->lds = vaq::scan_lds_bytes(ix->layout, ix->M, entries, qb, k, ea, best_nw, ix->n_buckets,
                                ix->bucket_shift, ix->bucket_t);
  const int step = vaq::scan_wg_step_rows(ix->layout, ix->M);
  const int64_t N = ix->N;
  const int nqb = (nq + qb - 1) / qb;
  int64_t s;
  if (bm) s = 1;
  else if (ix->opt_slices > 0) s = ix->opt_slices;
  else {
    // workgroups wanted in flight; the best-first form on a streamed database likes four times as
    // many (shorter workgroups: a query's cost varies tenfold and the launch ends with the longest;
    // 1B rows: 2048 queries x 1 / 2 / 4 / 8 / 16 slices 337 / 254 / 201 / 205 / 228 ms) and no slice
    // of more than 2^29 rows (10 k queries x 1 / 2 / 4 slices: 887 / 807 / 823 ms)
    const int64_t target = (int64_t)ix->n_cu * (bf_streamed ? 32 : 8);
    s = (target + nqb - 1) / nqb;
    if (bf_streamed) s = std::max<int64_t>(s, (N + ((int64_t)1 << 29) - 1) >> 29);
    const int64_t max_s = std::max<int64_t>(1, N / MIN_SLICE_ROWS);
    s = std::min(s, max_s);
  }
  s = std::max<int64_t>(1, s);
  int64_t rows = (N + s - 1) / s;
  rows = std::max<int64_t>(step, ((rows + step - 1) / step) * step);
  s = N > 0 ? (N + rows - 1) / rows : 1;
  pl->n_slices = (int)s;
  pl->slice_rows = rows;
  // Threshold seeding: when a query's rows are split over several workgroups,
  // each would otherwise warm its admission threshold up on its own slice
  // (k-th best of the few rows it has seen).  A pre-pass scans ~1/64 of the
  // rows, spread evenly, merges its top-k and publishes the k-th distance as
  // the starting threshold of every workgroup of the full scan: an upper
  // bound of the final k-th, so results are unchanged.
  pl->seed_slices = 0;
  pl->seed_rows = pl->seed_stride = 0;
  // best-first slice order (slice_order_kernel): an alternative to the pre-pass, off by default --
  // measured slower (250M rows, 2 queries: 1.21 vs 0.70 ms; 32 queries: 8.7 vs 5.6 ms): the first
  // wave of workgroups all starts cold, and batches no longer share a slice's rows through L2
  pl->ordered = ea && ix->opt_order && s > 1 && s <= 4096 && ix->n_buckets <= 4096 && ix->bucket_t == 0;
  if (ea && ix->opt_seed && !pl->ordered && s >= SEED_MIN_SLICES && N >= SEED_MIN_ROWS) {
    const int64_t sample = std::max<int64_t>(N / ix->opt_seed_frac, (int64_t)16 * k);
    // small workgroups (4 waves) and many slices: the pre-pass runs with cold
    // thresholds, where the waves of a workgroup queue on its admission lock
    int64_t ss = std::min<int64_t>(1024, std::max<int64_t>(8, sample / 8192));
    int64_t srows = ((sample / ss + step - 1) / step) * step;
    int64_t stride = (N / ss / step) * step;
    if (stride >= srows && srows > 0) {
      pl->seed_slices = (int)ss;
      pl->seed_rows = srows;
      pl->seed_stride = stride;
    }
  }
  // Best-first form: when a workgroup's slice spans many buckets (the cache-resident databases), all
  // of them are visited in ascending order of their bound with work units handed out by ticket.
  pl->bf = false;
  if (ix->opt_bf && ea == vaq::EA_QUEUE && qb == 1 && !pl->ordered && subs == ix->M &&
      vaq::scan_bf_supported(ix->layout, ix->M, qb, ea, ix->n_buckets, ix->seq) && ix->n_buckets >= 16 &&
      pl->slice_rows >= 8 * (N / ix->n_buckets + 1)) {
    int bnw = 0, bscore = 0, bpool = 0;
    size_t blds = 0;
    int pool_lo, pool_hi;
    vaq::scan_bf_pool_range(k, &pool_lo, &pool_hi);
    // bit-packed rows: when every field after the first group lies in the last dword, it is queued
    const int carry = (ix->layout == vaq::LAYOUT_BITS && ix->M > 4 && ix->sub[4].word == ix->W - 1) ? 1 : 0;
    for (int nw : {4, 8, 16}) {
      if (ix->opt_nwaves > 0 && nw != ix->opt_nwaves) continue;
      size_t lds = vaq::scan_bf_lds_bytes(ix->layout, ix->M, entries, pool_lo, nw, ix->n_buckets, carry);
      if (lds > LDS_LIMIT) continue;
      const int wgs = (int)std::min<size_t>(LDS_LIMIT / lds, (size_t)(32 / nw));
      // the largest k-min pool that keeps that many workgroups resident (LDS is handed out in
      // LDS_GRANULE pieces; at 72 VGPRs a SIMD holds 7 waves, so 4-wave workgroups stop at 7)
      const size_t budget = LDS_LIMIT / (size_t)std::min(wgs, std::max(1, BF_WAVES_PER_CU / nw)) / LDS_GRANULE * LDS_GRANULE;
      int pool = pool_lo;
      while (pool + 64 <= pool_hi &&
             vaq::scan_bf_lds_bytes(ix->layout, ix->M, entries, pool + 64, nw, ix->n_buckets, carry) <= budget)
        pool += 64;
      lds = vaq::scan_bf_lds_bytes(ix->layout, ix->M, entries, pool, nw, ix->n_buckets, carry);
      // small workgroups win here even at lower residency: setup, bootstrap and the final sort
      // are per workgroup and leave its other waves idle (C2: 4 waves x 6 workgroups per CU
      // 1.02 ms, 8 x 4 1.15 ms, 16 x 2 1.8 ms)
      const int score = nw == 4 ? wgs * nw * 10 : nw == 8 ? wgs * nw * 7 : wgs * nw * 4;
      if (score > bscore) { bscore = score; bnw = nw; blds = lds; bpool = pool; }
    }
    if (bnw) {
      pl->bf = true;
      pl->bf_carry = carry;
      pl->bf_pool = bpool;
      if (s == 1 && k <= 256 && (ix->opt_defer > 0 || (ix->opt_defer < 0 && nq >= DEFER_MIN_QUERIES)))
        pl->defer_units = ix->opt_defer > 0 ? ix->opt_defer : DEFER_UNITS;
      // more queries than workgroups resident at a time: start the expensive ones first
      // (calls of more than QUERY_CHUNK queries are served chunk by chunk, each ranked on its own)
      pl->cost_order = s == 1 && ix->opt_cost_order && nq >= COST_ORDER_MIN_QUERIES &&
                       (ix->sub[0].ncent >> ix->bucket_shift) <= 1024;
      pl->nwaves = bnw;
      pl->lds = blds;
      if (bm && s == 1) {
        pl->bm = true;
        pl->bm_qb = ix->opt_bm_qb > 0 ? ix->opt_bm_qb : BM_QB;
        // 16-byte rows: four queries' tables are 64 KB, one 16-wave workgroup per CU.  Two queries per group
        // in 8-wave workgroups are two workgroups per CU at twice the passes over a bucket's rows -- that
        // pays while those passes come out of L2, i.e. on shards up to about 4 GB of codes (10 k queries:
        // 62.5M / 125M / 250M rows 13.2 -> 12.2 / 16.6 -> 15.6 / 23.8 -> 23.3 ms; 500M 37.7 -> 39.0, 1B 65.6 -> 82.1)
        if (ix->opt_bm_qb <= 0 && ix->M == 16 && (double)N * 16.0 <= BM_QB2_MAX_BYTES) pl->bm_qb = 2;
        pl->bm_nwaves = ix->opt_bm_nwaves > 0 ? ix->opt_bm_nwaves : BM_NWAVES;
        if (ix->opt_bm_nwaves <= 0) {
          // 16 or 8 waves per workgroup: whichever keeps more waves resident on a CU, and on a tie the
          // smaller workgroups (more items in flight, shorter waits at an item's barriers).  8-byte rows:
          // 16 waves need 90 KB (one workgroup), 8 waves 65 KB (two): C4 7.9 -> 6.8 ms; 16-byte rows have
          // room for one workgroup either way, and 16 waves are 66 ms at 1B rows where 8 are 92.
          int best_res = 0;
          for (int nw : {16, 8}) {
            const size_t lds = vaq::scan_bm_lds_bytes(ix->M, pl->bm_qb, nw) + 8192;
            if (lds > LDS_LIMIT) continue;
            const int res = std::min<int>(32, nw * (int)(LDS_LIMIT / lds));
            if (res >= best_res) { best_res = res; pl->bm_nwaves = nw; }
          }
        }
        pl->bm_cap = ix->opt_bm_cap > 0 ? ix->opt_bm_cap : BM_CAND_CAP;
        while (vaq::scan_bm_lds_bytes(ix->M, pl->bm_qb, pl->bm_nwaves) + 8192 > LDS_LIMIT && pl->bm_nwaves > 4) pl->bm_nwaves >>= 1;
        // pass A: about one average bucket per query (a work unit = 64 wave steps)
        const int64_t unit_rows = 64 * (int64_t)(vaq::scan_wg_step_rows(ix->layout, ix->M) / vaq::SCAN_MAX_WAVES);
        const int64_t avg = N / ix->n_buckets + 1;
        const int64_t bucket_units = (avg + unit_rows - 1) / unit_rows;
        pl->defer_units = ix->opt_bm_units > 0 ? ix->opt_bm_units
                                               : (int)std::min<int64_t>(4096, std::max<int64_t>(8, bucket_units));
        // Small buckets: a best-first pass over each query's nearest one is cheap and leaves a better
        // threshold than a sample (100M x 8 B, 10 k queries: 9.4 ms against 13.8).  Large buckets: that
        // pass streams 10 k buckets from HBM with nothing shared (1B x 16 B: 63 ms of 161), so a
        // sampled threshold and the nearest bucket as the first bucket-major round (11 ms).
        pl->bm_boot = ix->opt_bm_boot == 1 ? bucket_units >= BM_BOOT_MIN_UNITS : ix->opt_bm_boot != 0;
      }
    }
  }
  return VAQHIP_OK;
}

// Launch geometry of the TI form: one query per workgroup (Qb = 1, survivors queued), each
// query's work units spread over `n_slices` workgroups when there are few queries.
int vaqhost::make_ti_plan(const vaqhip_index *ix, int nq, int k, Plan *pl) {
  const int qb = 1, ea = vaq::EA_QUEUE;
  // the visiting list is int(T * visit) clusters long unless the until-k-rows rule extends it:
  // stage that many (rounded up to a wave's worth) at a time; longer lists go in chunks
  const int max_visit = ix->ti_visit < 1.0f ? (int)((float)ix->ti_T * ix->ti_visit) : ix->ti_T;
  pl->ti_cap = std::min(ix->ti_T, std::max(64, ((max_visit + 63) / 64) * 64));
  const size_t ti_bytes = vaq::scan_ti_lds_bytes(pl->ti_cap);
  const int need = ix->layout == vaq::LAYOUT_BYTES ? ix->M : 1;
  int best_nw = 0, best_waves = 0, subs = ix->M, entries = ix->lut_floats;
  for (subs = ix->M; subs >= need; subs--) {
    entries = subs == ix->M ? ix->lut_floats : ix->sub[subs].lut_off;
    best_nw = 0;
    best_waves = 0;
    for (int nw : {4, 8, 16}) {
      if (ix->opt_nwaves > 0 && nw != ix->opt_nwaves) continue;
      const size_t lds = vaq::scan_lds_bytes(ix->layout, ix->M, entries, qb, k, ea, nw, ix->ti_T, 0, 0) + ti_bytes;
      if (lds > LDS_LIMIT) continue;
      const int wgs = (int)std::min<size_t>(LDS_LIMIT / lds, (size_t)(32 / nw));
      if (wgs * nw > best_waves) { best_waves = wgs * nw; best_nw = nw; }
    }
    if (best_nw) break;
  }
  if (!best_nw)
    return fail(VAQHIP_EUNSUPPORTED,
                "the lookup tables of the first %d subspaces, top-%d buffers and %d clusters do not fit "
                "%zu B of LDS", need, k, ix->ti_T, LDS_LIMIT);
  pl->lds_subs = subs;
  pl->lut_lds_entries = entries;
  pl->qb = qb;
  pl->ea = ea;
  pl->nwaves = best_nw;
  vaq::scan_geometry(ix->layout, ix->M, k, ea, &pl->kp, &pl->ccap, &pl->qcap);
  pl->lds = vaq::scan_lds_bytes(ix->layout, ix->M, entries, qb, k, ea, best_nw, ix->ti_T, 0, 0) + ti_bytes;
  int64_t s;
  if (ix->opt_slices > 0) s = ix->opt_slices;
  else {
    // enough workgroups to fill the chip, but no more than the visited rows give work units
    // (one unit = 16 wave steps) to two rounds of a workgroup's waves
    const int64_t target = (int64_t)ix->n_cu * 8;
    s = (target + nq - 1) / nq;
    const int64_t unit_rows = 16 * (vaq::scan_wg_step_rows(ix->layout, ix->M) / vaq::SCAN_MAX_WAVES);
    const double frac = ix->ti_visit < 1.0f ? std::max(ix->ti_visit, 1.0f / ix->ti_T) : 1.0;
    const int64_t units = (int64_t)(frac * ((double)ix->N / unit_rows + ix->ti_T));
    s = std::min<int64_t>(s, std::max<int64_t>(1, units / (2 * best_nw)));
  }
  pl->n_slices = (int)std::max<int64_t>(1, std::min<int64_t>(s, 4096));
  pl->slice_rows = 0;
  pl->seed_slices = 0;
  pl->seed_rows = pl->seed_stride = 0;
  pl->ordered = false;
  return VAQHIP_OK;
}
