// vaq_scan_launch.hip -- the LDS geometry of a scan workgroup and launch_scan(), which picks among the scan units
// (vaq_scan_bytes.hip, vaq_scan_bits.hip, vaq_scan_bf.hip).  No kernel is defined here.
// vaq_scan.h: SCAN_MAX_THREADS, VAQ_CCAP, SEL_HDR_WORDS, GMIN_MAX_BITS, hot_bytes, ti_lds_bytes and the declarations
// of launch_scan_bytes / launch_scan_bits; vaq_scan_bf.h: the declaration of launch_scan_bf, nothing else.
#include "vaq_scan_params.h"
#include "vaq_scan.h"
#include "vaq_scan_bf.h"

namespace vaq {
static int rows_per_item(int layout, int M) { return (layout == LAYOUT_BYTES && M < 16) ? 16 / M : 1; }

// rows the code buffer and every slice are padded to: one step of the largest workgroup
int scan_wg_step_rows(int layout, int M) { return SCAN_MAX_THREADS * rows_per_item(layout, M); }

// code dwords a survivor-queue entry carries besides the row id and the partial sums: the
// rest of the row for byte codes of up to 16 subspaces (phase B then needs no re-read)
static int queue_code_words(int layout, int M, int ea) {
  return (layout == LAYOUT_BYTES && M <= 16 && ea == EA_QUEUE) ? M / 4 - 1 : 0;
}

void scan_geometry(int layout, int M, int k, int ea, int *kp, int *ccap, int *qcap) {
  int p2 = 1;
  while (p2 < k) p2 <<= 1;
  *kp = p2;
  *ccap = VAQ_CCAP;  // a wave appends at most 64 rows per lock hold
  *qcap = ea == EA_QUEUE ? 128 : 0;  // at most 63 left over + 64 pushed before the next drain
}

// lut_floats: LUT entries staged in LDS (all of them, or the resident prefix of the bit-packed path)
size_t scan_lds_bytes(int layout, int M, int lut_floats, int qb, int k, int ea, int nwaves,
                      int n_buckets, int bucket_shift, int bucket_t) {
  int kp, ccap, qcap;
  scan_geometry(layout, M, k, ea, &kp, &ccap, &qcap);
  size_t lut = (size_t)(layout == LAYOUT_BYTES ? M * 256 : lut_floats) * 4 * qb;
  lut = (lut + 15) & ~(size_t)15;
  const size_t sb = ((size_t)SEL_HDR_WORDS * 4 + (size_t)(kp + ccap) * 8 + 15) & ~(size_t)15;
  const size_t lbb = (bucket_shift > 0 || bucket_t > 0) ? (((size_t)n_buckets * 4 * qb + 15) & ~(size_t)15) : 0;
  return lut + (size_t)qb * sb + lbb + hot_bytes(n_buckets) +
         (size_t)nwaves * qcap * 4 * (1 + qb + queue_code_words(layout, M, ea));
}

size_t scan_ti_lds_bytes(int n_clusters) { return ti_lds_bytes(n_clusters); }

hipError_t launch_scan(const ScanParams &p_in, int *grid_out, hipStream_t st) {
  ScanParams p = p_in;
  p.q_cw_words = queue_code_words(p.layout, p.M, p.ea);
  const int nqb = (p.nq + p.qb - 1) / p.qb;
  const int total = nqb * p.n_slices;
  const int grid = ((total + 7) / 8) * 8;
  if (grid_out) *grid_out = grid;
  if (total == 0) return hipSuccess;
  if (p.bf) return launch_scan_bf(p, grid, st);
  size_t lds = scan_lds_bytes(p.layout, p.M, p.lut_lds_entries, p.qb, p.k, p.ea, p.nwaves, p.n_buckets,
                              p.bucket_shift, p.bucket_t);
  if (p.bucket_t < 0 || p.bucket_t > GMIN_MAX_BITS || (p.bucket_t > 0 && p.bucket_shift != 0))
    return hipErrorInvalidValue;
  if (p.ti) {
    if (p.qb != 1 || p.ea != EA_QUEUE || p.bucket_shift != 0 || p.bucket_t != 0 || p.n_hot != 0 || !p.sqrt_out)
      return hipErrorInvalidValue;
    if (p.ti_cap < 1 || p.ti_cap > p.n_buckets) return hipErrorInvalidValue;
    lds += ti_lds_bytes(p.ti_cap);
  } else if (p.sqrt_out) {
    return hipErrorInvalidValue;  // only the TI kernels select on square roots
  }
  return p.layout == LAYOUT_BYTES ? launch_scan_bytes(p, lds, grid, st) : launch_scan_bits(p, lds, grid, st);
}

} // namespace vaq
