// vaq_exhaust_launch.h -- the launches of the exhaustive form of VAQ::refine (vaq_exhaust.hip): every resident row a
// candidate, in row order.  (vaq_exhaust.h holds the per-pair arithmetic, free of HIP, for the host tests.)
#ifndef VAQ_EXHAUST_LAUNCH_H_
#define VAQ_EXHAUST_LAUNCH_H_

#include "vaq_common.h"

namespace vaq {

constexpr int XS_TILE = 256;      // rows a workgroup takes at a time
constexpr int XS_MAX_QG = 1024;   // queries a workgroup owns (their thresholds and counts sit in LDS)
constexpr int XS_MAX_K1 = 1025;   // entries per list: VAQHIP_MAX_K, and one more for the flag step of "exact_ties"
// The plan of one launch: S splits of split_rows rows each (the last may be short or empty), G = ceil(nq / qg) groups
// of qg queries; workgroup (s, g) streams split s against group g.  buf_*: [nq][S][cap] candidate lists,
// cap = exhaust_list_cap(k); part_*: [S][nq][k] the splits' k best, labels with id_base, -1 / FLT_MAX in empty slots
// (launch_merge's in_final format).  The answer does not depend on S, qg or the tile.
struct XsParams {
  int nq, D;
  int64_t N, id_base;
  int k, cap;
  int S, G, qg;
  int64_t split_rows;
  float *buf_d;
  int *buf_id;
  float *part_d;
  int *part_id;
};
int exhaust_list_cap(int k);
size_t exhaust_register_max_dim();  // widest row of the register form
int exhaust_blocks_per_cu(int D, int elem);  // resident workgroups per CU of the select kernel for this width and row type
// Q: nq x D, rows: N x D; D <= refine_rows_max_dim(); rows of up to XS_MAX_DIM columns (vaq_exhaust.h) take the
// register form, wider ones the general path
hipError_t launch_exhaust_select(const XsParams &p, const float *Q, RowsRef rows, hipStream_t st);
// "exact_ties": block e replays query list[e] over all rows through the reference's heap and writes its k slots of
// labels / dist; blocks at or beyond *count exit at once (launch nq of them)
hipError_t launch_exhaust_replay(const float *Q, int nq, int D, RowsRef rows, int64_t N, int64_t id_base, int k,
                                 const int *list, const unsigned *count, int32_t *labels, float *dist, hipStream_t st);
// The same as one link of a chain over shards: `rows` are the shard's n rows, id_base its first label.  Entry e of
// the list starts from the raw heap arrays hin_v / hin_i [e][k] the link before left (nullptr: the empty heap).
// finish == 0: its raw arrays go to hout_v / hout_i [e][k].  finish != 0: heap_reorder, the k slots go to labels / dist
// [query][k], or with labels == nullptr to hout_v / hout_i [e][k], which launch_exhaust_scatter -- on the device of
// the caller's buffers, after a copy -- places at query list[e].  launch_exhaust_replay is the chain of one link.
hipError_t launch_exhaust_replay_link(const float *Q, int nq, int D, RowsRef rows, int64_t N, int64_t id_base, int k,
                                      const int *list, const unsigned *count, const float *hin_v, const int *hin_i,
                                      float *hout_v, int *hout_i, int finish, int32_t *labels, float *dist,
                                      hipStream_t st);
hipError_t launch_exhaust_scatter(int nq, int k, const int *list, const unsigned *count, const float *src_v,
                                  const int *src_i, int32_t *labels, float *dist, hipStream_t st);

} // namespace vaq
#endif
