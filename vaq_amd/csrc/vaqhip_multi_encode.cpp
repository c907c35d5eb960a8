// vaqhip_multi_encode.cpp -- VAQ::encode across the shards of the multi-device index (include/vaqhip.h, "Encode
// across the shards"): every shard encodes the rows it will hold on its own device and takes the codes from there.
//
// A row's code depends on that row and the codebooks only (VAQ.cpp:736-745), and every shard holds the codebooks and
// the rotation.  So shard g encodes rows [lo_g, lo_g + n_g) of the cut vaqhip_multi_set_codes_u16 would make and hands
// its index the same n_g x M matrix that call would have uploaded: the index ends in the same state, bit for bit,
// without a chain, an exchange or a tie question.  No kernel of its own: the shard's vaqhip_encode_device (project,
// encode) and vaqhip_index_set_codes_u16_device / _add_codes_u16_device (sort, pack, merge).
// The vaqhip_multi_encode_lut_* calls are the same calls with the engine's rule (vaqhip_encode_lut_device,
// encodeToLUTCode) in the place of VAQ::encode's: one flag on the call, everything else shared.
//
// Two phases, each on every shard's worker at once (on_shards):
//   1 encode  the rows -- uploaded slice by slice in chunks (host form; byte rows as the bytes they are), or read where
//             a multi refiner holds them (refiner form) -- into a scratch buffer of n_g x M uint16 on the shard's
//             device.  Byte rows go to the shard's vaqhip_encode[_lut]_u8_device, whose projection widens a byte where
//             it loads it ((float)uint8 is exact).  The stream is synchronised, so whatever fails has failed before any
//             shard's rows change
//   2 set     the index takes the buffer (set: every shard, an empty one is emptied; append: the last shard), the
//             codes go to the host only when the caller asked for them
// The scratch is released by the calling thread once both phases are over, whichever way they ended.  It is the
// call's, not the handle's, on purpose: n_g x M x 2 bytes per shard (4 GB at 125M x 16) that nothing needs between two
// builds; the price is two hipMalloc / hipFree and four events per shard and call.
// All row and element offsets are int64_t / size_t: a shard of 125M x 16 codes has 2e9 elements.
#include "vaqhip_shard_run.h"

#include <chrono>
#include <cstring>

using namespace vaqhost;

namespace {

constexpr int64_t ENCODE_CHUNK_ROWS = (int64_t)1 << 20;  // rows per upload / project chunk (vaqhip_encode's)

// one shard's part of the call in flight
struct EncodePart {
  int64_t lo = 0, n = 0;           // rows [lo, lo + n) of the call's matrix
  vaq::RowsRef d_rows = {nullptr, 4};  // refiner form: the shard's resident rows, float or byte
  DevBuf chunk, codes;             // host form: [chunk rows][D] of the call's element; uint16 [n][M]
  hipEvent_t t[4] = {nullptr, nullptr, nullptr, nullptr};  // phase 1: start, encoded; phase 2: start, set
  float encode_ms = 0, set_ms = 0;
  bool held() const { return codes.p || chunk.p || t[0]; }
  void release() { release_all({&chunk, &codes}), destroy_events(t); }
};

struct EncodeCall {
  vaq::RowsRef X = {nullptr, 4};  // host form: the call's matrix, float or byte
  int projected = 0;
  bool lut = false;          // the engine's encoder (vaqhip_encode_lut_device) in the place of vaqhip_encode_device
  int64_t id_base = 0;       // set: the label of the matrix's first row
  bool append = false;
  uint16_t *codes_out = nullptr;
  int64_t chunk = ENCODE_CHUNK_ROWS;
  std::vector<EncodePart> part;
};

// what vaqhip_index_set_codes_u16 refuses on the shard that takes rows [lo, lo + n) from label id_base + lo
int check_labels(int64_t n, int64_t first_label) {
  if (n > 0x7fffffffLL - 1 || first_label + n > 0x7fffffffLL)
    return mfail(VAQHIP_ERANGE, "labels are 32-bit ints (utils/Types.hpp:100): id_base+N = %lld", (long long)(first_label + n));
  return VAQHIP_OK;
}

// phase 1 on shard g's worker
int encode_part(vaqhip_multi *mx, const EncodeCall &c, EncodePart &p, Shard &s) {
  if (p.n == 0) return 0;
  const size_t D = (size_t)mx->D, M = (size_t)mx->M;
  MHIP(hipSetDevice(s.device));
  MHIP(ensure_events(p.t));
  MHIP(p.codes.ensure((size_t)p.n * M * sizeof(uint16_t)));
  const size_t elem = (size_t)(c.X.p ? c.X.elem : p.d_rows.elem);
  if (c.X.p) MHIP(p.chunk.ensure((size_t)std::min(c.chunk, p.n) * D * elem));  // (sized in bytes)
  MHIP(hipEventRecord(p.t[0], s.stream));
  for (int64_t r = 0; r < p.n; r += c.chunk) {
    const int64_t m = std::min(c.chunk, p.n - r);
    const void *d_x = p.chunk.p;
    if (c.X.p)  // (one chunk buffer: the stream orders this copy behind the encode of the chunk before)
      MHIP(hipMemcpyAsync(p.chunk.p, vaq::rows_at(c.X, (size_t)(p.lo + r) * D).p, (size_t)m * D * elem, hipMemcpyHostToDevice, s.stream));
    else d_x = vaq::rows_at(p.d_rows, (size_t)r * D).p;
    uint16_t *d_codes = p.codes.as<uint16_t>() + (size_t)r * M;
    if (elem == 1) {
      const uint8_t *x = static_cast<const uint8_t *>(d_x);
      if (c.lut) MIX(vaqhip_encode_lut_u8_device(s.ix, x, m, c.projected, d_codes, s.stream));
      else MIX(vaqhip_encode_u8_device(s.ix, x, m, c.projected, d_codes, s.stream));
    } else {
      const float *x = static_cast<const float *>(d_x);
      if (c.lut) MIX(vaqhip_encode_lut_device(s.ix, x, m, c.projected, d_codes, s.stream));
      else MIX(vaqhip_encode_device(s.ix, x, m, c.projected, d_codes, s.stream));
    }
  }
  MHIP(hipEventRecord(p.t[1], s.stream));
  MHIP(hipStreamSynchronize(s.stream));
  return 0;
}

// phase 2 on shard g's worker
int set_part(vaqhip_multi *mx, const EncodeCall &c, EncodePart &p, Shard &s, bool takes) {
  if (!takes) return 0;
  const size_t M = (size_t)mx->M;
  MHIP(hipSetDevice(s.device));
  const uint16_t *d_codes = p.n > 0 ? p.codes.as<uint16_t>() : nullptr;
  // (its own start: between t[1] and here lie the wait for the slowest shard's phase 1 and the host's hand-over)
  if (p.n > 0) MHIP(hipEventRecord(p.t[2], s.stream));
  if (c.append) MIX(vaqhip_index_add_codes_u16_device(s.ix, d_codes, p.n, s.stream));
  else MIX(vaqhip_index_set_codes_u16_device(s.ix, d_codes, p.n, c.id_base + p.lo, s.stream));
  if (p.n > 0) MHIP(hipEventRecord(p.t[3], s.stream));
  if (p.n > 0 && c.codes_out)
    MHIP(hipMemcpyAsync(c.codes_out + (size_t)p.lo * M, p.codes.p, (size_t)p.n * M * sizeof(uint16_t), hipMemcpyDeviceToHost, s.stream));
  MHIP(hipStreamSynchronize(s.stream));
  if (p.n == 0) return 0;
  MHIP(hipEventElapsedTime(&p.encode_ms, p.t[0], p.t[1]));
  MHIP(hipEventElapsedTime(&p.set_ms, p.t[2], p.t[3]));
  return 0;
}

// the scratch of every shard, by the calling thread; the handle's streams are idle first (a phase may have failed part-way)
void release_parts(vaqhip_multi *mx, EncodeCall &c) {
  idle_then_release(c.part, [&](int g) { return ShardAt{mx->sh[g].device, mx->sh[g].stream}; });
}

// Both phases over the parts in c.part; mx->mu held, everything refused that can be.  A set gives the shards the parts'
// row ranges once phase 1 is through (a failure of phase 2 is vaqhip_multi_set_codes_u16's, which cuts first too).
int run_encode(vaqhip_multi *mx, EncodeCall &c, int64_t rows) {
  const auto t0 = std::chrono::steady_clock::now();
  DeviceGuard keep(DeviceGuard::restore_only);
  c.chunk = mx->opt_encode_chunk > 0 ? mx->opt_encode_chunk : ENCODE_CHUNK_ROWS;
  int rc = on_shards(mx, [&](int g, Shard &s) { return encode_part(mx, c, c.part[g], s); });
  if (!rc) {
    for (int g = 0; !c.append && g < mx->G; g++) mx->sh[g].lo = c.part[g].lo, mx->sh[g].n = c.part[g].n;
    rc = on_shards(mx, [&](int g, Shard &s) { return set_part(mx, c, c.part[g], s, !c.append || g == mx->G - 1); });
  }
  release_parts(mx, c);
  if (rc) return rc;
  mx->has_codes = true;
  vaqhip_multi_encode_timing &t = mx->enc_last;
  t = vaqhip_multi_encode_timing{};
  for (const EncodePart &p : c.part) {
    t.encode_ms = std::max(t.encode_ms, p.encode_ms);
    t.set_codes_ms = std::max(t.set_codes_ms, p.set_ms);
  }
  t.rows = rows;
  t.n_devices = mx->G;
  t.total_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return VAQHIP_OK;
}

}  // namespace

int vaqhost::set_encode_chunk_rows(vaqhip_multi *mx, int64_t value) {
  if (value < 0) return mfail(VAQHIP_EINVAL, "encode_chunk_rows=%lld: 0 (1 << 20 rows) or a number of rows", (long long)value);
  std::lock_guard<std::mutex> lk(mx->mu);
  mx->opt_encode_chunk = value;
  return VAQHIP_OK;
}

namespace {

// the engine's encoder needs Q on every shard (mx->mu held)
int check_lut(const vaqhip_multi *mx, bool lut) {
  if (lut && !mx->lut_q) return mfail(VAQHIP_ESTATE, "vaqhip_multi_encode_lut_* needs vaqhip_multi_set_lut_quantiles first");
  return VAQHIP_OK;
}

int encode_set_codes(vaqhip_multi *mx, vaq::RowsRef X, int64_t N, int projected, int64_t id_base, uint16_t *codes_out,
                     bool lut) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (N < 0 || (N > 0 && !X.p) || id_base < 0) return mfail(VAQHIP_EINVAL, "bad rows/N/id_base");
  std::lock_guard<std::mutex> lk(mx->mu);
  if (const int rc = check_lut(mx, lut)) return rc;
  EncodeCall c;
  c.lut = lut;
  c.X = X;
  c.projected = projected;
  c.id_base = id_base;
  c.codes_out = codes_out;
  c.part.resize((size_t)mx->G);
  for (int g = 0; g < mx->G; g++) {
    shard_cut(N, mx->G, g, &c.part[g].lo, &c.part[g].n);
    if (const int rc = check_labels(c.part[g].n, id_base + c.part[g].lo)) return rc;
  }
  if (const int rc = run_encode(mx, c, N)) return rc;
  mx->N = N;
  mx->id_base = id_base;
  return VAQHIP_OK;
}

int encode_add_codes(vaqhip_multi *mx, vaq::RowsRef X, int64_t n_new, int projected, uint16_t *codes_out, bool lut) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (n_new < 0 || (n_new > 0 && !X.p)) return mfail(VAQHIP_EINVAL, "bad rows/N");
  std::lock_guard<std::mutex> lk(mx->mu);
  if (const int rc = check_lut(mx, lut)) return rc;
  if (!mx->has_codes) return mfail(VAQHIP_ESTATE, "no codes yet: vaqhip_multi_encode_set_codes (or set_codes_u16) first");
  // the new rows continue the numbering: they extend the LAST shard (vaqhip_multi_add_codes_u16) and are encoded there
  Shard &last = mx->sh[mx->G - 1];
  if (const int rc = check_labels(last.n + n_new, mx->id_base + last.lo)) return rc;
  EncodeCall c;
  c.lut = lut;
  c.X = X;
  c.projected = projected;
  c.append = true;
  c.codes_out = codes_out;
  c.part.resize((size_t)mx->G);
  c.part[mx->G - 1].n = n_new;  // (rows [0, n_new) of X)
  if (const int rc = run_encode(mx, c, n_new)) return rc;
  last.n += n_new;
  mx->N += n_new;
  return VAQHIP_OK;
}

int encode_from_refiner(vaqhip_multi *mx, vaqhip_multi_refiner *r, uint16_t *codes_out, bool lut) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  std::lock_guard<std::mutex> lr(r->mu);  // (the order of vaqhip_multi_search_refine: the refiner, then the index)
  std::lock_guard<std::mutex> lk(mx->mu);
  if (const int rc = check_lut(mx, lut)) return rc;
  if (const int rc = check_refiner_pair(mx, r)) return rc;
  EncodeCall c;
  c.lut = lut;
  c.id_base = r->id_base;
  c.codes_out = codes_out;
  c.part.resize((size_t)mx->G);
  for (int g = 0; g < mx->G; g++) {
    const ResidentRows rows = resident_rows(r, g);
    c.part[g].lo = rows.first_label - r->id_base;
    c.part[g].n = rows.n;
    c.part[g].d_rows = rows.rows;
    if (const int rc = check_labels(rows.n, rows.first_label)) return rc;
  }
  if (const int rc = run_encode(mx, c, r->N)) return rc;
  mx->N = r->N;
  mx->id_base = r->id_base;
  return VAQHIP_OK;
}

}  // namespace

extern "C" {

int vaqhip_multi_encode_set_codes(vaqhip_multi *mx, const float *X, int64_t N, int projected, int64_t id_base,
                                  uint16_t *codes_out) {
  return encode_set_codes(mx, vaq::RowsRef{X, 4}, N, projected, id_base, codes_out, false);
}
int vaqhip_multi_encode_set_codes_u8(vaqhip_multi *mx, const uint8_t *X, int64_t N, int projected, int64_t id_base, uint16_t *codes_out) {
  return encode_set_codes(mx, vaq::RowsRef{X, 1}, N, projected, id_base, codes_out, false);
}
int vaqhip_multi_encode_add_codes(vaqhip_multi *mx, const float *X, int64_t n_new, int projected, uint16_t *codes_out) {
  return encode_add_codes(mx, vaq::RowsRef{X, 4}, n_new, projected, codes_out, false);
}
int vaqhip_multi_encode_add_codes_u8(vaqhip_multi *mx, const uint8_t *X, int64_t n_new, int projected, uint16_t *codes_out) {
  return encode_add_codes(mx, vaq::RowsRef{X, 1}, n_new, projected, codes_out, false);
}
int vaqhip_multi_encode_from_refiner(vaqhip_multi *mx, vaqhip_multi_refiner *r, uint16_t *codes_out) {
  return encode_from_refiner(mx, r, codes_out, false);
}
int vaqhip_multi_encode_lut_set_codes(vaqhip_multi *mx, const float *X, int64_t N, int projected, int64_t id_base,
                                      uint16_t *codes_out) {
  return encode_set_codes(mx, vaq::RowsRef{X, 4}, N, projected, id_base, codes_out, true);
}
int vaqhip_multi_encode_lut_set_codes_u8(vaqhip_multi *mx, const uint8_t *X, int64_t N, int projected, int64_t id_base, uint16_t *codes_out) {
  return encode_set_codes(mx, vaq::RowsRef{X, 1}, N, projected, id_base, codes_out, true);
}
int vaqhip_multi_encode_lut_add_codes(vaqhip_multi *mx, const float *X, int64_t n_new, int projected,
                                      uint16_t *codes_out) {
  return encode_add_codes(mx, vaq::RowsRef{X, 4}, n_new, projected, codes_out, true);
}
int vaqhip_multi_encode_lut_add_codes_u8(vaqhip_multi *mx, const uint8_t *X, int64_t n_new, int projected, uint16_t *codes_out) {
  return encode_add_codes(mx, vaq::RowsRef{X, 1}, n_new, projected, codes_out, true);
}
int vaqhip_multi_encode_lut_from_refiner(vaqhip_multi *mx, vaqhip_multi_refiner *r, uint16_t *codes_out) {
  return encode_from_refiner(mx, r, codes_out, true);
}

int vaqhip_multi_last_encode_timing(vaqhip_multi *mx, vaqhip_multi_encode_timing *out) {
  if (!mx || !out) return mfail(VAQHIP_EINVAL, "null pointer");
  std::lock_guard<std::mutex> lk(mx->mu);
  *out = mx->enc_last;
  return VAQHIP_OK;
}

}  // extern "C"
