// vaq_codes.h -- building an index (vaq_codes.hip): the encoder, the packers and the stable sort by first code.
#ifndef VAQ_CODES_H_
#define VAQ_CODES_H_

#include "vaq_common.h"

namespace vaq {

// VAQ::encodeImpl: Xp is n x D already in PCA space; codes is n x M uint16 row-major
hipError_t launch_encode(const float *Xp, int64_t n, int D, int M, int L, const SubDesc *sub,
                         const float *cent, uint16_t *codes, hipStream_t st);
// dwords the packed layout needs for `rows` rows
int64_t packed_words(int64_t rows, int M, int layout, int W);
// Pack rows [row_begin, row_end) (codes_u16 points at row_begin; row_begin a
// multiple of 64) and zero-fill the packed words up to out_row_end.
// perm (optional): packed row r is source row perm[r] (the bucketed order)
hipError_t launch_pack_codes(const uint16_t *codes_u16, int64_t row_begin, int64_t row_end,
                             int64_t out_row_end, int M, int layout, int W, const SubDesc *sub,
                             const uint32_t *perm, uint32_t *out, hipStream_t st);
// Stable sort of rows by their subspace-0 code: d_perm[n] (sorted row -> original
// row) and d_bucket_start[(1<<bits0)+1] (first sorted row of each code that
// occurs, -1 otherwise; the caller back-fills).  Synchronises the stream.
// fine > 0 (shift == 0): the rows of a bucket are also ordered by the next `fine` bits of the second
// code, and d_sub_start[((1 << kbits) << fine) + 1] receives the first row of every run (-1: back-fill)
hipError_t sort_by_first_code(const uint16_t *d_codes, int64_t n, int M, int bits0, int shift, int bits1,
                              int t, uint32_t *d_perm, int *d_bucket_start, hipStream_t st, int fine = 0,
                              int *d_sub_start = nullptr);
// Appending: merge the (separately sorted and packed) new rows into the bucketed order, bucket by
// bucket; *_start have K0 + 1 entries (back-filled); out_* are the new buffers
hipError_t launch_merge_rows(const uint32_t *old_codes, const uint32_t *old_perm, const int *old_start,
                             const uint32_t *new_codes, const uint32_t *new_perm, const int *new_start, int K0,
                             int64_t n_old, int64_t n_total, int M, int layout, int W, uint32_t *out_codes,
                             uint32_t *out_perm, hipStream_t st);

} // namespace vaq
#endif
