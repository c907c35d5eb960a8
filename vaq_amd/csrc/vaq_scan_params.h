// vaq_scan_params.h -- what the host sees of the scan: the parameter block of a launch, the LDS geometry of a scan
// workgroup and launch_scan() (vaq_scan_launch.hip), and the host-side questions of the best-first form
// (vaq_scan_bf.hip), whose own header is device code the host files cannot read.  vaq_scan.h, and through it every
// scan unit, starts from here.
#ifndef VAQ_SCAN_PARAMS_H_
#define VAQ_SCAN_PARAMS_H_

#include "vaq_common.h"

namespace vaq {

// early-abandon forms of the scan (identical results):
//   EA_NONE    every row summed completely (VAQ::searchHeap as written)
//   EA_QUEUE   survivors of the first group compacted into an LDS queue and
//              finished 64 at a time (best when many query batches share the
//              code stream through cache: instruction-bound)
//   EA_INPLACE survivors finish in place under the EXEC mask (no queue, no
//              re-read of their codes: best for a single HBM-bound pass)
enum EarlyAbandon { EA_NONE = 0, EA_QUEUE = 1, EA_INPLACE = 2 };

// most wavefronts a scan workgroup may have (the host picks 4, 8 or 16)
constexpr int SCAN_MAX_WAVES = 16;

// one query handed from the first launch of the best-first form to the second (ScanParams::defer_*)
struct DeferRec {
  int q;              // query (index within the call)
  unsigned done_key;  // buckets with keys <= this were scanned by the first launch
  unsigned thr;       // its threshold when it stopped (float bits): an upper bound of the final k-th distance
  int pad;            // != 0: no bucket is finished yet (done_key is not a key)
};

struct ScanParams {
  const uint32_t *codes;  // packed codes (layout-specific)
  int64_t n_rows;         // local rows
  int layout;             // Layout
  int M;                  // subspaces
  int W;                  // dwords per row (bit-packed layout)
  const SubDesc *sub;     // [M]
  const uint32_t *perm;   // [n_rows] sorted row -> original row (labels), or nullptr = identity
  const int *bucket_start;// [n_buckets + 1] first sorted row of each subspace-0 code
  int n_buckets;          // 1 << (bits[0] - bucket_shift)
  int bucket_shift;       // bucket = first code >> bucket_shift
  int bucket_t;           // (bucket_shift == 0) bucket = first code << bucket_t | top bucket_t bits of code 1
  int n_hot;              // buckets a workgroup scans best-first before the rest (0 = off, <= 32)
  unsigned long long *stats; // diagnostic builds (-DVAQ_STATS): event counters, else nullptr
  int no_skip;            // 1: visit every bucket (measurement only: the streaming rate of the scan)
  const int *first_sub;   // [W+1] first subspace starting in word w (bit-packed layout)
  const float *lut;       // [nq][lut_floats]
  int lut_floats;
  int lds_subs;           // tables of subspaces [0, lds_subs) are staged in LDS ...
  int lut_lds_entries;    // ... = this many packed LUT entries; the rest is read from `lut`
  int nq;
  int k;
  int kp;                 // power of two >= k: slots of a workgroup's best list (per query)
  int ccap;               // slots of its candidate region
  int qcap;               // slots of a wave's survivor queue (early abandon)
  int q_cw_words;         // code dwords per queue entry (set by launch_scan)
  int nwaves;             // wavefronts per workgroup
  int ea;                 // EarlyAbandon
  unsigned *g_thr;        // [nq] shared threshold distances (float bits), preset to FLT_MAX
  int qb;                 // queries per pass (1, 2, 4)
  int n_slices;           // row slices per query batch
  int64_t slice_rows;     // rows per slice (multiple of the workgroup step)
  int64_t slice_stride;   // rows between slice starts (== slice_rows for a full scan,
                          // larger for the sampling pre-pass)
  int share_thr;          // 1: exchange thresholds between workgroups through g_thr
  const int *slice_order; // [query batches][n_slices] best-first slice order, or nullptr = row order
  const int *qorder;      // [nq] the i-th query a pass takes (similar queries share a pass), or nullptr = i
  int seq;                // 1: sequential row sum (BitVecEngine::queryLUT) instead of groups of 4
  int32_t *final_labels;  // non-null (needs n_slices == 1): results written directly, [nq][k]
  float *final_dist;
  int64_t id_base;
  int *part_cnt;          // [nq][n_slices] real entries of each list
  // triangle-inequality form (VAQ::searchTriangleInequality): rows are grouped by cluster
  // (bucket_start = cluster starts, n_buckets = clusters, farthest-from-centre first) and
  // each query visits its own list of clusters; needs qb == 1 and ea == EA_QUEUE
  int bf_carry;           // bit-packed best-first form: 1 = the groups after the first lie in the row's last
                          //    dword, which is carried through the survivor queue
  int bf_pool;            // best-first form: slots of the k-min pool (scan_bf_pool_range, multiple of 64)
  // best-first form, ONE workgroup per query (n_slices == 1): the expensive queries are cut in two.
  //   defer_units > 0   the first round takes at most this many work units (nearest buckets first);
  //                     what is still in reach when it is over goes to defer_list instead of a
  //                     second round, and a SECOND launch serves it with n_slices workgroups each
  //   defer_mode == 1   this is that second launch: workgroup v serves entry v / n_slices of
  //                     defer_list, rows of slice v % n_slices, starting from the entry's threshold
  //                     and skipping the buckets at or below its done_key; lists go to part_d/part_id
  int defer_units, defer_mode, defer_cap;
  unsigned *defer_count;  // entries asked for so far (beyond defer_cap: not handed over, scanned in place)
  struct DeferRec *defer_list;
  // bucket-major second pass (vaq_scan_bm.hip): with defer_units > 0 and bm_done set, EVERY query whose
  // capped first round left buckets in reach stores its done_key here (preset 0xffffffff = nothing
  // left) and its threshold -- lowered to its exact k-th distance when it has k rows -- in g_thr,
  // instead of joining defer_list
  unsigned *bm_done;
  int bf;                 // 1: best-first form (vaq_scan_bf.h): all buckets of the slice in ascending order
                          //    of their bound, work units by ticket (needs qb == 1, ea == EA_QUEUE, no TI)
  int ti;                 // 1: TI form
  const int *ti_order;    // [nq][n_buckets] clusters in visiting order
  const float *ti_qcc;    // [nq][n_buckets] query-to-centre distances, same order
  const int *ti_nvisit;   // [nq] clusters visited
  const float *ti_xcc;    // [n_rows] row-to-centre distances (index order)
  int ti_rowcap;          // rows taken from the visiting order (INT_MAX = all)
  int ti_cap;             // entries of the visiting list a workgroup stages in LDS at a time
  int sqrt_out;           // 1: the k-min is kept on sqrt(distance), as the reference stores it
                          //    (VAQ.cpp:1583); partial lists and g_thr then hold square roots
  float *part_d;          // [nq][n_slices][k]
  int *part_id;
};

// ---- vaq_scan_launch.hip ----
// LDS geometry of a scan workgroup for top-k = k
void scan_geometry(int layout, int M, int k, int ea, int *kp, int *ccap, int *qcap);
// bytes of LDS a scan workgroup of `nwaves` wavefronts needs
size_t scan_lds_bytes(int layout, int M, int lut_floats, int qb, int k, int ea, int nwaves,
                      int n_buckets, int bucket_shift, int bucket_t);
// extra LDS bytes of a TI scan workgroup staging `cap` entries of its visiting list
size_t scan_ti_lds_bytes(int cap);
// rows one step of the LARGEST workgroup covers: slice_rows and the code
// buffer's padding must be multiples of it
int scan_wg_step_rows(int layout, int M);
hipError_t launch_scan(const ScanParams &p, int *grid_out, hipStream_t st);

// ---- vaq_scan_bf.hip ----
// best-first form (vaq_scan_bf.h): is there a kernel for this plan, and its LDS bytes
bool scan_bf_supported(int layout, int M, int qb, int ea, int n_buckets, int seq);
// `pool`: slots of the k-min pool (ScanParams::bf_pool), a multiple of 64 within scan_bf_pool_range(k)
size_t scan_bf_lds_bytes(int layout, int M, int lut_entries, int pool, int nwaves, int n_buckets, int bf_carry);
void scan_bf_pool_range(int k, int *lo, int *hi);
// dwords the code buffer must hold beyond its padded rows: the best-first form starts a unit on a 128-byte
// line, and the unit's last wave step may reach that far past the end (vaq_scan_bf.h, ALIGN_ROWS)
int64_t scan_bf_slack_words(int layout, int M);

} // namespace vaq
#endif
