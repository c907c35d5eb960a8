// vaq_bitvec_tile.h -- the tile loaders of the exact forms over raw rows (vaq_bitvec_naive.hip: the exact cluster form;
// vaq_bitvec_ti.hip: the triangle-inequality form).  A tile is 256 raw rows reached through an index list; it goes
// through LDS in chunks of DC = 32 dimensions at a row stride of 33 dwords: eight adjacent lanes load the eight 16-byte
// pieces of a row's chunk (thirty-two adjacent lanes its elements one by one where the row is not a whole number of
// aligned pieces), and each lane then walks its own row.  Device code only; every function is inlined into its kernel.
#ifndef VAQ_BITVEC_TILE_H_
#define VAQ_BITVEC_TILE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vaq {

constexpr int BITVEC_EXACT_DC = 32;  // dimensions of a chunk: a tile of 256 rows is staged in LDS DC floats at a time

namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_WAVE = 64;
constexpr int EX_DC = BITVEC_EXACT_DC;
constexpr int EX_STRIDE = EX_DC + 1;  // dwords between two rows of the tile: odd, so lane-per-row reads meet 64 banks
static_assert(EX_DC == 32, "a thread carries 8 pieces of 4, or 32 elements, of a chunk: 256 rows x 32 over 256 threads");

__device__ __forceinline__ void ex_load4(const float *y, float *v) {
  const float4 t = *reinterpret_cast<const float4 *>(y);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void ex_load4(const uint8_t *y, float *v) {
  const uint32_t t = *reinterpret_cast<const uint32_t *>(y);
  v[0] = (float)(t & 255u); v[1] = (float)((t >> 8) & 255u); v[2] = (float)((t >> 16) & 255u); v[3] = (float)(t >> 24);
}

// The elements [d0, d0 + DC) of the tile's rows from global memory into a thread's registers.  VEC: thread = piece
// tid % 8 of rows tid / 8 + 32 i; otherwise element tid % 32 of rows tid / 32 + 8 i.  s_row holds the tile's raw rows,
// -1 behind the last candidate; nothing is read past a row's D elements.
template <typename T, bool VEC>
__device__ __forceinline__ void ex_fetch(const T *__restrict__ rows, int D, const int32_t *s_row, int d0, float (&v)[EX_DC]) {
  const int tid = threadIdx.x;
  if constexpr (VEC) {
    const int e = d0 + (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int row = s_row[i * 32 + (tid >> 3)];
      if (row >= 0 && e < D) {  // (D % 4 == 0: the piece is inside the row)
        ex_load4(rows + (size_t)row * D + e, &v[4 * i]);
      } else {
        v[4 * i] = v[4 * i + 1] = v[4 * i + 2] = v[4 * i + 3] = 0.0f;
      }
    }
  } else {
    const int e = d0 + (tid & 31);
#pragma unroll
    for (int i = 0; i < 32; i++) {
      const int row = s_row[i * 8 + (tid >> 5)];
      v[i] = (row >= 0 && e < D) ? (float)rows[(size_t)row * D + e] : 0.0f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void ex_stage(float *tile, const float (&v)[EX_DC]) {
  const int tid = threadIdx.x;
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      float *t = tile + (i * 32 + (tid >> 3)) * EX_STRIDE + (tid & 7) * 4;
#pragma unroll
      for (int j = 0; j < 4; j++) t[j] = v[4 * i + j];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 32; i++) tile[(i * 8 + (tid >> 5)) * EX_STRIDE + (tid & 31)] = v[i];
  }
}

}  // namespace

}  // namespace vaq
#endif  // VAQ_BITVEC_TILE_H_
