// vaq_common.h -- what several device modules and their hosts share: the subspace descriptor, the two code layouts,
// the tile and sentinel constants, and a reference to rows of either element type.  Every module's launchers and
// parameter blocks are declared in the header of the .hip that defines them (vaq_front.h, vaq_codes.h,
// vaq_scan_params.h, vaq_merge.h, vaq_scan_bm.h, vaq_exact.h, ...), never here.
//
// Numerics, for every unit of the library: compiled with -ffp-contract=off, so every float add is a plain IEEE fp32
// add in the order the reference's source spells out, and fused multiply-adds appear only as explicit
// __builtin_fmaf (utils/AVXUtils.hpp:11-15 is a real vfmadd231ps).
#ifndef VAQ_COMMON_H_
#define VAQ_COMMON_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vaq {

// Per-subspace descriptor, one table per index in device memory.
struct SubDesc {
  int ncent;    // mCentroidsNum[s] = 1 << bits
  int bits;     // mBitsAlloc[s]
  int bit_off;  // first bit of the field inside a packed row (LSB-first)
  int lut_off;  // entry offset inside the packed per-query LUT
  int cent_off; // float offset inside the concatenated centroid buffer
  int word;     // bit_off / 32
  int shift;    // bit_off % 32
  int pad;
};

enum Layout { LAYOUT_BYTES = 0, LAYOUT_BITS = 1 };

// rows per planar tile of the bit-packed layout (one wavefront step)
constexpr int TILE_ROWS = 64;
// sentinel id of an empty candidate slot (sorts after every real id)
constexpr int ID_SENTINEL = 0x7fffffff;

// Resident rows are held as float32 or as uint8 (a bvecs dataset as it is stored): elem is the element's size, 4 or 1.
// (float)uint8 is exact, so a kernel over byte rows runs the float form's operations on the float form's operands;
// only the load differs.  Queries are float either way.
struct RowsRef {
  const void *p;
  int elem;
};
// the rows from element `elems` on
inline RowsRef rows_at(RowsRef r, size_t elems) {
  return RowsRef{static_cast<const char *>(r.p) + elems * (size_t)r.elem, r.elem};
}

} // namespace vaq
#endif
