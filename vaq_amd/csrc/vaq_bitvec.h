// vaq_bitvec.h -- the Hamming half of BitVecEngine (BitVecEngine.cpp:60-76 query_sort, :454-466
// rerankUsingEuclideanDistance): the scan of packed bit rows against many queries and the Euclidean rerank of the
// Hamming candidates.  The selection between them is FAST's (vaq_fast.h: launch_fast_head_sort, launch_fast_select):
// KNNFromDists over 16-bit integer distances.  DESIGN.md section 4h has the specification and the layout.
#ifndef VAQ_BITVEC_H_
#define VAQ_BITVEC_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_common.h"
#include "vaq_fast.h"
#include "vaq_restated.h"

namespace vaq {

constexpr int BITVEC_MAX_WORDS = 16;   // uint64 words per row: at most 1024 bits, so every distance fits 16 bits
constexpr int BITVEC_QT = 64;          // queries a thread meets per read of its rows (the query tile)
constexpr int BITVEC_THREADS = 256;    // threads per workgroup of the scan
constexpr int BITVEC_ROWS_PER_THREAD = 2;  // adjacent rows, so that a lane stores both distances as one dword
constexpr int BITVEC_ROW_TILE = BITVEC_THREADS * BITVEC_ROWS_PER_THREAD;  // rows per workgroup
constexpr int BITVEC_RERANK_MAX = 1024;  // candidates per query of the rerank (VAQHIP_MAX_K)

// the `M` launch_fast_select sizes its histogram by (255 * M + 1 bins) so that every distance a row of W words can
// have, 64 * W with the tail bits counted, has a bin of its own
inline int bitvec_select_m(int W) { return (64 * W + 254) / 255; }

// dist[q][r] = sum_w popcount(rows[r][w] ^ queries[q][w]) for q < nq, r < n_pad: hammingDist
// (utils/DistanceFunctions.hpp:164-172) over all actBitVLen words, no masking.  rows holds n_pad rows of W words
// (n_pad a multiple of FAST_ROW_PAD; rows past the caller's n are read and their distances written, whatever they
// hold), dist is [nq][n_pad].  1 <= W <= BITVEC_MAX_WORDS.
hipError_t launch_bitvec_scan(const uint64_t *rows, int64_t n_pad, int W, const uint64_t *queries, int nq,
                              uint16_t *dist, hipStream_t st);

// rerankUsingEuclideanDistance for nq queries: candidate c of query q is the row labelled cand[q * cand_stride + c],
// c < R <= BITVEC_RERANK_MAX, in the order the Hamming selection left them.  Its distance is euclideanDistNoSQRT
// (utils/DistanceFunctions.hpp:232-239): distance += (a - b) * (a - b) in dimension order from 0.0f, the subtraction,
// the product and the addition apart (a byte row is widened where it is loaded).  Then
// KNNFromDistsIndicesSupplied (BitVecEngine.hpp:171-187): std::sort of the first kk = min(k, R) (dist, idx) pairs
// by distance alone, every later candidate behind its equals -- the kk smallest by (dist, position), the head's
// position being the one std::sort left it at.  Slots >= kk are -1 / FLT_MAX.  A label outside
// [id_base, id_base + N) is never read: it ranks last with an infinite distance and label -1.
hipError_t launch_bitvec_rerank(const float *queries, int nq, int D, RowsRef rows, int64_t N, int64_t id_base,
                                const int32_t *cand, int64_t cand_stride, int R, int k, int32_t *labels,
                                float *out_dist, hipStream_t st);
// floats of a query row the rerank can stage (the workgroup's LDS beside its candidate arrays)
size_t bitvec_rerank_max_dim();

// One (dist, idx) pair of the rerank and the comparator KNNFromDistsIndicesSupplied hands std::sort
struct RerankPair {
  float dist;
  int idx;
};
struct RerankLt {
  __host__ __device__ inline bool operator()(const RerankPair &a, const RerankPair &b) const { return a.dist < b.dist; }
};
// std::sort of n <= 1024 pairs.  Guarded: with finite distances (the contract) the walk is std::sort's own; with a
// NaN the real function may leave the array, this one stops at its ends.
__host__ __device__ inline void rerank_sort(RerankPair *f, int n) { stdsort::sort_by<10, true>(f, n, RerankLt{}); }

}  // namespace vaq
#endif  // VAQ_BITVEC_H_
