// vaq_scan_bm.h -- bucket-major second pass of a streamed database with many queries (vaq_scan_bm.hip).
// After a capped best-first first pass (ScanParams::bm_done) every query knows the buckets it has
// finished (keys <= done_key) and an upper bound of its k-th distance (g_thr).  What is left in
// reach is turned round: per BUCKET the list of the queries that still want it, and workgroups
// that stream a bucket's rows once for QB queries whose lookup tables sit interleaved in LDS --
// the groups of one bucket run back to back on one XCD, so the bucket comes from HBM once and from
// that XCD's L2 for everybody else.  Survivors (complete sum not above the query's threshold) are
// appended to a per-query candidate buffer; a per-query histogram of the appended distances moves
// the shared threshold.  bm_select then takes the k best of (first pass list + candidates); a
// query whose buffer overflowed goes to the defer list and is finished by the best-first form.
#ifndef VAQ_SCAN_BM_H_
#define VAQ_SCAN_BM_H_

#include "vaq_scan_params.h"  // DeferRec

namespace vaq {

constexpr int BM_HIST_BINS = 64;
constexpr int BM_XCDS = 8;
struct BmParams {
  const uint32_t *codes;
  const uint32_t *perm;      // sorted row -> label, or nullptr = identity
  const int *bucket_start;   // [n_buckets + 1]
  int n_buckets, bucket_t;   // bucket = first code << bucket_t | top bucket_t bits of the second (bucket_shift == 0)
  const int *sub_start;      // [(n_buckets << (8 - bucket_t)) + 1] first row of every (first code, second code) run
                             //    when the rows of a bucket are ordered by the second code, else nullptr
  int M;
  const float *lut;          // [nq][lut_floats]
  int lut_floats;
  int nq, k, qb;
  int nwaves;
  unsigned *g_thr;           // [nq] float bits: thresholds of the best-first form (rows AT them stay admissible):
                             //      what a best-first first pass leaves, and what its second launch (overflow) starts from
  unsigned long long *thr64; // [nq] the rounds' thresholds: distance bits << 32 | label bound -- a row is a candidate iff
                             //      its (distance bits << 32 | label) is BELOW this word; label bound 0x7fffffff keeps every
                             //      row at that distance.  init64: bm_mark sets it from g_thr first (a search's first round)
  int init64;
  unsigned *done_key;        // [nq] buckets with keys <= this are finished; 0xffffffff: the query is complete
  unsigned *done_next;       // [nq] what done_key becomes when the round's select succeeds
  unsigned *fresh;           // [nq] 1: no bucket of the query is finished yet (done_key is ignored: set by
                             //      launch_bm_boot, cleared by the query's first successful select)
  int limit;                 // buckets a query takes in this round, nearest first (<= 0: all in reach)
  int retry;                 // 1: a query whose candidate buffer overflows only gets a tighter threshold from what was
                             //    stored and tries the same buckets again next round; 0 (last round): defer list
  // plan (device, written by launch_bm_plan)
  unsigned *mask;            // [nq][n_buckets / 32] buckets still in reach
  int *cnt;                  // [n_buckets] queries per bucket
  int *qoff;                 // [n_buckets + 1]
  int *fill;                 // [n_buckets]
  int *qlist;                // [nq * n_buckets] (worst case) queries of bucket b at qoff[b], similar ones next to each other
  unsigned short *qkey;      // [nq][1 << bucket_t] per query and group of second codes: its nearest and second nearest
                             //      second code inside the group -- the bucket's list is ordered by it, so that the
                             //      queries of a group of QB want the same runs of the bucket
  int *border;               // [n_buckets] buckets by descending work
  int *ioff;                 // [BM_XCDS][n_buckets / BM_XCDS + 2] prefix of the work items of each XCD's buckets
  unsigned *tickets;         // [BM_XCDS]
  // candidates
  int cap;                   // slots per query
  float *cand_d;             // [nq][cap]
  int *cand_id;              // [nq][cap] labels (without id_base)
  unsigned *cand_cnt;        // [nq] candidates appended (beyond cap: not stored -> overflow)
  unsigned *hist;            // [nq][BM_HIST_BINS]
  float *scale;              // [nq] bins / H, 0 = histogram off
  // first-pass results (the API's format) and the final output, in place
  int32_t *labels;           // [nq][k]
  float *dist;
  int64_t id_base;
  // overflow -> defer list
  unsigned *defer_count;
  struct DeferRec *defer_list;
  int defer_cap;
};
bool scan_bm_supported(int layout, int M, int n_buckets, int bucket_shift, int seq, int k);
size_t scan_bm_lds_bytes(int M, int qb, int nwaves);
// words of the plan arrays above, for the caller's allocation: mask, cnt + qoff + fill + border + ioff + tickets
size_t bm_plan_small_words(int n_buckets);
// mark + count, order + prefix, fill (three launches)
hipError_t launch_bm_plan(const BmParams &p, hipStream_t st);
// instead of a best-first first pass: per query a threshold from a sample of its nearest rows (the k-th
// smallest complete sum of up to 4096 rows starting at the nearest run of the nearest bucket), an empty
// result list, nothing finished (the first round is then planned with BmParams::first = 1)
hipError_t launch_bm_boot(const BmParams &p, int64_t n_rows, hipStream_t st);
// staged search: thr64 = min(thr64, thr_in << 32 | 0x7fffffff) (thr_in optional); thr_out (optional) = distance bits
// of thr64; init: thr64 is first made from g_thr
hipError_t launch_bm_thresholds(const BmParams &p, const int32_t *thr_in, int32_t *thr_out, int init, hipStream_t st);
hipError_t launch_scan_bm(const BmParams &p, int n_cu, hipStream_t st);
hipError_t launch_bm_select(const BmParams &p, hipStream_t st);

} // namespace vaq
#endif
