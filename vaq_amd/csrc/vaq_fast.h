// vaq_fast.h -- the FAST search method (VAQ::searchFast, VAQ.cpp:1778-1834): uint8 lookup tables
// over codes of at most 4 bits, integer row sums, top-k by KNNFromDists (utils/Experiment.hpp:40-56).
// DESIGN.md section "FAST" has the specification and the (dist, seq) argument.
#ifndef VAQ_FAST_H_
#define VAQ_FAST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaq_restated.h"

namespace vaq {

// rows of the FAST code image are padded to this (the reference pads mCodebookCMajor to 32, VAQ.cpp:666-670)
constexpr int FAST_ROW_PAD = 32;
// dwords per (row, lane group) of the FAST code image: code s = 4t + h sits in group h, nibble t
__host__ __device__ inline int fast_code_words(int M) { return (M / 4 + 7) / 8; }

// FAST code image: row r, group h (s % 4), dword w holds the codes of subspaces 4(8w + i) + h in nibble i.
// Rows [row_begin, row_end) of `out` are written from codes_u16 (CodebookType rows, first = row_begin).
hipError_t launch_fast_pack_codes(const uint16_t *codes_u16, int64_t row_begin, int64_t row_end, int M,
                                  uint32_t *out, hipStream_t st);
// smallQuantize (utils/Math.hpp:215-224) of the reference LUTType lut_ref[q][s][ksub] (rows >= 1 << bits[s]
// zero, as CreateLUT leaves them): small[q][s][c] = min(floor(max(lut - off[s], 0) * scale[s]), 255) for
// c < ksub, 0 for ksub <= c < 16
hipError_t launch_fast_quantize(const float *lut_ref, int nq, int M, int ksub, const float *offsets,
                                const float *scale, uint8_t *small, hipStream_t st);
// dist[q][r] = sum_s small[q][s][code(r, s)] for rows [0, n_pad) (n_pad a multiple of FAST_ROW_PAD) as an
// int8 GEMM on the matrix cores: A = one-hot rows, B = small - 128
hipError_t launch_fast_scan(const uint32_t *codes, int64_t n_pad, int M, const uint8_t *small, int nq,
                            uint16_t *dist, int n_cu, hipStream_t st);
// KNNFromDists' std::sort of the first kk = min(k, n) rows by distance only (libstdc++ introsort, one
// thread per query): order[q][p] = row at position p, for p < kk
hipError_t launch_fast_head_sort(const uint16_t *dist, int64_t n_pad, int nq, int kk, uint32_t *scratch,
                                 uint16_t *order, hipStream_t st);
// the same with explicit element strides per query for all three arrays; scratch[q * scratch_stride + p] is
// left holding the sorted items themselves, (dist << 16) | row
hipError_t launch_fast_head_sort_strided(const uint16_t *dist, int64_t dist_stride, int nq, int kk, uint32_t *scratch,
                                         int64_t scratch_stride, uint16_t *order, int64_t order_stride, hipStream_t st);
// the k smallest rows by (dist, seq) per query: seq = position in `order` for rows < kk, the row itself after.
// Slots >= min(k, n) are -1 / FLT_MAX.
hipError_t launch_fast_select(const uint16_t *dist, int64_t n_pad, int64_t n, int nq, int k, int M,
                              const uint16_t *order, int64_t id_base, int32_t *labels, float *out_dist,
                              hipStream_t st);
// One shard's part of a sharded FAST search ("FAST across shards"): the first
// head_rows rows are left out, the others are ranked by (dist, row); slots >= min(k, n - head_rows) are
// -1 / FLT_MAX.  head_rows = 0 is a plain (dist, row) top-k.
hipError_t launch_fast_select_tail(const uint16_t *dist, int64_t n_pad, int64_t n, int64_t head_rows, int nq, int k,
                                   int M, int64_t id_base, int32_t *labels, float *out_dist, hipStream_t st);
// out[q * out_stride + i] = dist[q * n_pad + i] for i < h: a shard's head distances into its exchange buffer
hipError_t launch_fast_head_copy(const uint16_t *dist, int64_t n_pad, int nq, int h, uint16_t *out,
                                 int64_t out_stride, hipStream_t st);
// head[q][p] for p < kk from the gathered planes of n_parts shards: part g owns positions
// [start[g], start[g + 1]) and holds them at planes[g * plane_stride + q * kk + p]
constexpr int FAST_MAX_LISTS = 16;
struct FastHeadParts {
  int n_parts;
  int start[FAST_MAX_LISTS + 1];
};
hipError_t launch_fast_head_gather(const uint16_t *planes, int64_t plane_stride, FastHeadParts parts, int nq, int kk,
                                   uint16_t *head, hipStream_t st);
// The first k of the stable merge by distance alone of: the head list -- head_sorted[q * head_stride + p] =
// (dist << 16) | head row, p < kk, in the order launch_fast_head_sort_strided left them -- then n_lists <=
// FAST_MAX_LISTS lists of k slots each, ascending, empty slots label < 0 (candidate i of list l of query q at
// l * list_stride + q * query_stride + i).  Ties go to the earlier list, then to the earlier position.  Labels of
// head rows are head_label_base + row.  head_sorted may be the query's own row of `labels` (it is read whole
// before anything is written); slots past the number of entries are -1 / FLT_MAX.
hipError_t launch_fast_merge(const uint32_t *head_sorted, int64_t head_stride, int kk, int64_t head_label_base,
                             const float *dist_lists, const int32_t *label_lists, int n_lists, int64_t list_stride,
                             int64_t query_stride, int nq, int k, int32_t *labels, float *out_dist, hipStream_t st);

// KNNFromDists' std::sort (launch_fast_head_sort): vaq_restated.h's stdsort over uint32 items compared by the
// top 16 bits (the distance; the low 16 bits are the row and ride along), n <= 1024 (VAQHIP_MAX_K): depth <=
// 2 * 10 frames below the root
namespace stdsort {
__host__ __device__ inline bool lt(uint32_t a, uint32_t b) { return (a >> 16) < (b >> 16); }
struct Lt16 {
  __host__ __device__ inline bool operator()(uint32_t a, uint32_t b) const { return lt(a, b); }
};
__host__ __device__ inline void sort(uint32_t *f, int n) { sort_by<10, false>(f, n, Lt16{}); }
}  // namespace stdsort

}  // namespace vaq
#endif  // VAQ_FAST_H_
