// vaq_kmeans.hip -- the k-means inside VAQ::clusterTI(true) on gfx950: KMeans::staticFitCodebook ->
// staticFitSampling (KMeans.hpp:487-652, called at VAQ.cpp:896-900), centre for centre and bit for bit.
//
// Compiled with -ffp-contract=off like every file of the library.  Every operation that decides a bit is a
// plain fp32 operation in the reference's order:
//   assign      sqrt((x - mean).squaredNorm()) per (row, centre), centres ascending, strict `<` on the square
//               roots (the first minimum wins, a NaN never does).  squaredNorm is Eigen's linear vectorised
//               reduction (Eigen/src/Core/Redux.h, 8-float packets, two accumulators, unaligned start 0):
//               sq_norm_eigen (vaq_restated.h)
//   accumulate  the reference runs two OpenMP threads with a static schedule: rows [0, ceil(n/2)) and the rest.
//               Per thread, centre and column a float sum from +0 in ascending row order -- here a stable sort
//               of the rows by (half, centre) and one thread per (half, centre, column) walking its run
//   update      new = ((0 + p0) + p1) / float(c0 + c1); a centre whose new row is not elementwise == to the old
//               one is replaced (an empty cluster is 0 / 0 = NaN, unequal for ever: the loop then runs to
//               max_iter, as the reference's does)
// No float atomics, no MFMA, no reassociation.
#include "kmeans_sample.h"
#include "vaq_kmeans.h"
#include "vaq_restated.h"
#include "vaqhip_dev.h"

#include <algorithm>
#include <chrono>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>

#include <float.h>
#include <math.h>

namespace vaq {

// floats of centres a workgroup of the assign kernel stages in LDS at a time
constexpr int KM_STAGE_FLOATS = 4096;
// bytes of LDS its tile of decoded rows may take; wider rows are read from global memory
constexpr int KM_TILE_BYTES = 40 * 1024;

// The sample's codes straight from the packed rows (index order, either layout: unpack_codes_kernel in vaq_ti.hip
// has the two addressings).  One thread per packed row: its original row perm[r] is looked up in the sampled rows
// (rows_sorted ascending, slots[i] = the sample position of rows_sorted[i]; nullptr: every row is sampled at
// slot = its original row) and only a hit writes its first seg codes to scodes[slot][seg].
__global__ void km_gather_packed_kernel(const uint32_t *__restrict__ packed, int64_t n, int M, int layout, int W,
                                        const SubDesc *__restrict__ sub, const uint32_t *__restrict__ perm,
                                        const unsigned *__restrict__ rows_sorted, const unsigned *__restrict__ slots,
                                        int n_sample, int seg, uint16_t *__restrict__ scodes) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const unsigned orig = perm ? perm[r] : (unsigned)r;
  int64_t slot = orig;
  if (rows_sorted) {
    int lo = 0, hi = n_sample;  // the first entry >= orig
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (rows_sorted[mid] < orig) lo = mid + 1;
      else hi = mid;
    }
    if (lo == n_sample || rows_sorted[lo] != orig) return;
    slot = slots[lo];
  }
  if (slot >= n_sample) return;
  uint16_t *o = scodes + slot * seg;
  if (layout == LAYOUT_BYTES) {
    const uint32_t *rp = packed + r * (M / 4);
    for (int s = 0; s < seg; s++) o[s] = (uint16_t)((rp[s >> 2] >> ((s & 3) * 8)) & 0xffu);
  } else {
    const uint32_t *rp = packed + (r / TILE_ROWS) * (int64_t)(TILE_ROWS * W) + (r % TILE_ROWS);
    for (int s = 0; s < seg; s++) {
      const SubDesc sd = sub[s];
      const uint32_t lo = rp[sd.word * TILE_ROWS];
      const uint32_t hi = (sd.word + 1 < W) ? rp[(sd.word + 1) * TILE_ROWS] : 0u;
      const uint64_t both = ((uint64_t)hi << 32) | lo;
      o[s] = (uint16_t)((both >> sd.shift) & (uint64_t)(sd.ncent - 1));
    }
  }
}

// X[r] = the centroids of row r's codes side by side (KMeans.hpp:631-646)
__global__ void km_decode_kernel(const uint16_t *__restrict__ scodes, int64_t rows, int seg, int L,
                                 const SubDesc *__restrict__ sub, const float *__restrict__ cent,
                                 float *__restrict__ X) {
  const int d = seg * L;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * d) return;
  const int64_t r = i / d;
  const int c = (int)(i % d), s = c / L, j = c % L;
  const SubDesc sd = sub[s];
  X[i] = cent[sd.cent_off + (size_t)(scodes[r * seg + s] & (sd.ncent - 1)) * L + j];
}

// means[i] = X[seed_rows[i]] (KMeans.hpp:516-520)
__global__ void km_seed_kernel(const float *__restrict__ X, int d, const int *__restrict__ seed_rows, int T,
                               float *__restrict__ means) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * d) return;
  means[i] = X[(size_t)seed_rows[i / d] * d + i % d];
}

// One row per thread.  X_LDS: the workgroup's decoded rows sit in LDS as [dim][row] (each thread reads its own
// column, conflict-free); else every thread reads its row from global memory.  The centres pass through LDS
// `stage` at a time and are read with wave-uniform addresses (broadcast).
// keys[r] = half * T + centre, vals[r] = the row: the input of the stable sort that orders the accumulation.
// X, keys and vals are a slice of the sample that starts at its row `row_off` (one device's share of the step);
// the half and the row emitted are positions in the whole sample.
template <bool X_LDS>
__global__ void km_assign_kernel(const float *__restrict__ X, int n, int d, const float *__restrict__ means, int T,
                                 int stage, int half_rows, int row_off, unsigned *__restrict__ keys,
                                 unsigned *__restrict__ vals, int *__restrict__ flags) {
  extern __shared__ float km_lds[];
  float *cs = km_lds;                         // [stage][d]
  float *xt = km_lds + (size_t)stage * d;     // [d][R]
  const int R = blockDim.x, tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int64_t r = r0 + tid;
  const int64_t rr = r < n ? r : n - 1;  // (rows past the end work on the last row and store nothing)
  if (X_LDS) {
    const int64_t lim = (int64_t)n * d;
    for (int i = tid; i < R * d; i += R) {
      const int64_t g = r0 * d + i;
      xt[(size_t)(i % d) * R + i / d] = g < lim ? X[g] : 0.0f;
    }
  }
  float best = FLT_MAX;
  int idx = -1;
  for (int c0 = 0; c0 < T; c0 += stage) {
    const int cn = min(stage, T - c0);
    __syncthreads();  // the last stage is read, the tile is written
    for (int i = tid; i < cn * d; i += R) cs[i] = means[(size_t)c0 * d + i];
    __syncthreads();
    for (int c = 0; c < cn; c++) {
      const float d2 = X_LDS ? sq_norm_eigen<false>(xt + tid, R, cs + (size_t)c * d, d)
                             : sq_norm_eigen<true>(X + (size_t)rr * d, 1, cs + (size_t)c * d, d);
      const float dist = sqrtf(d2);
      if (dist < best) {
        best = dist;
        idx = c0 + c;
      }
    }
  }
  if (r < n) {
    if (idx < 0) flags[1] = 1;  // the reference indexes row -1 here
    const int64_t gr = r + row_off;
    keys[r] = (unsigned)((gr >= half_rows ? T : 0) + max(idx, 0));
    vals[r] = (unsigned)gr;
  }
}

// run [start, end) of every key in the sorted keys (both preset to 0: keys that do not occur are empty)
__global__ void km_bounds_kernel(const unsigned *__restrict__ keys, int n, int *__restrict__ start,
                                 int *__restrict__ end) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned k = keys[i];
  if (i == 0 || keys[i - 1] != k) start[k] = i;
  if (i == n - 1 || keys[i + 1] != k) end[k] = i + 1;
}

// part[(half * T + c) * d + col] = the rows of that run added from +0 in ascending row order; neighbouring
// threads take neighbouring columns of the same run
__global__ void km_accumulate_kernel(const float *__restrict__ X, int d, const unsigned *__restrict__ rows_sorted,
                                     const int *__restrict__ start, const int *__restrict__ end, int n_runs,
                                     float *__restrict__ part) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)n_runs * d) return;
  const int g = (int)(gid / d), col = (int)(gid % d);
  float sum = 0.0f;
  for (int i = start[g], e = end[g]; i < e; i++) sum += X[(size_t)rows_sorted[i] * d + col];
  part[gid] = sum;
}

// one wavefront per centre (KMeans.hpp:586-604)
__global__ __launch_bounds__(64) void km_update_kernel(const float *__restrict__ part, const int *__restrict__ start,
                                                      const int *__restrict__ end, int T, int d,
                                                      float *__restrict__ means, int *__restrict__ flags) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int count = (end[c] - start[c]) + (end[T + c] - start[T + c]);
  const float *p0 = part + (size_t)c * d, *p1 = part + (size_t)(T + c) * d;
  float *m = means + (size_t)c * d;
  bool differs = false;
  for (int j = lane; j < d; j += 64) {
    const float v = ((0.0f + p0[j]) + p1[j]) / (float)count;
    if (!(v == m[j])) differs = true;
  }
  if (!__any(differs)) return;
  for (int j = lane; j < d; j += 64) m[j] = ((0.0f + p0[j]) + p1[j]) / (float)count;
  if (lane == 0) flags[0] = 1;
}

hipError_t kmeans_gather_packed(const uint32_t *d_packed, int64_t n, int M, int layout, int W, const SubDesc *sub,
                                const uint32_t *d_perm, const int *sample_rows, int n_sample, int seg,
                                uint16_t *d_scodes, hipStream_t st) {
  if (n == 0 || n_sample == 0) return hipSuccess;
  if (!sample_rows && n_sample != n) return hipErrorInvalidValue;
  hipError_t e;
  // (freed on return, after the stream is synchronised)
  vaqhost::DevBuf b_rows_in, b_rows_out, b_slots_in, b_slots_out, b_temp;
  const unsigned *rows_sorted = nullptr, *slots = nullptr;
  if (sample_rows) {
    // the sampled rows ascending, each with its position in the sample
    const size_t bytes = (size_t)n_sample * sizeof(unsigned);
    std::vector<unsigned> iota((size_t)n_sample);
    for (int i = 0; i < n_sample; i++) iota[(size_t)i] = (unsigned)i;
    if ((e = b_rows_in.ensure(bytes)) != hipSuccess || (e = b_rows_out.ensure(bytes)) != hipSuccess ||
        (e = b_slots_in.ensure(bytes)) != hipSuccess || (e = b_slots_out.ensure(bytes)) != hipSuccess ||
        (e = hipMemcpyAsync(b_rows_in.p, sample_rows, bytes, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(b_slots_in.p, iota.data(), bytes, hipMemcpyHostToDevice, st)) != hipSuccess)
      return e;
    unsigned row_bits = 1;
    while (row_bits < 32 && ((int64_t)1 << row_bits) < n) row_bits++;
    size_t temp_bytes = 0;
    if ((e = rocprim::radix_sort_pairs(nullptr, temp_bytes, b_rows_in.as<unsigned>(), b_rows_out.as<unsigned>(),
                                       b_slots_in.as<unsigned>(), b_slots_out.as<unsigned>(), (size_t)n_sample, 0u,
                                       row_bits, st)) != hipSuccess ||
        (e = b_temp.ensure(temp_bytes ? temp_bytes : 16)) != hipSuccess ||
        (e = rocprim::radix_sort_pairs(b_temp.p, temp_bytes, b_rows_in.as<unsigned>(), b_rows_out.as<unsigned>(),
                                       b_slots_in.as<unsigned>(), b_slots_out.as<unsigned>(), (size_t)n_sample, 0u,
                                       row_bits, st)) != hipSuccess)
      return e;
    rows_sorted = b_rows_out.as<unsigned>();
    slots = b_slots_out.as<unsigned>();
  }
  hipLaunchKernelGGL(km_gather_packed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_packed, n, M,
                     layout, W, sub, d_perm, rows_sorted, slots, n_sample, seg, d_scodes);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

namespace {
double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// One device's share of the assign step: rows [row0, row0 + n) of the sample.  Device 0 works in the buffers of
// the whole sample; the others own a copy of their slice (and of the centres), freed by KmParts.
struct KmPart {
  int row0 = 0, n = 0;
  vaqhost::DevBuf scodes, x, means, keys, vals, flags;
  hipEvent_t assigned = nullptr;  // this iteration's keys, values and flag are complete
};

struct KmParts {
  const KmeansDev *devs;
  int G;
  std::vector<KmPart> part;
  hipEvent_t fed = nullptr;  // device 0: the sample codes, then every iteration's centres, are there to be copied
  KmParts(const KmeansDev *devs, int G) : devs(devs), G(G), part((size_t)G) {}
  KmParts(const KmParts &) = delete;
  // (one device: it is current already, as the single index's entry left it)
  hipError_t use(int g) const { return G > 1 ? hipSetDevice(devs[g].device) : hipSuccess; }
  ~KmParts() {
    for (int g = G - 1; g >= 0; g--) {
      if (g > 0 && part[(size_t)g].n == 0) continue;
      (void)use(g);
      if (G > 1) (void)hipStreamSynchronize(devs[g].st);
      KmPart &p = part[(size_t)g];
      if (p.assigned) (void)hipEventDestroy(p.assigned);
      for (vaqhost::DevBuf *b : {&p.scodes, &p.x, &p.means, &p.keys, &p.vals, &p.flags}) b->release();
    }
    if (fed) (void)hipEventDestroy(fed);  // (device 0 is current again: the caller's buffers are freed there)
  }
};
} // namespace

hipError_t kmeans_fit(const KmeansDev *devs, int G, const uint16_t *d_scodes, int rows, int seg, int L,
                      const int *seed_rows, int T, int max_iter, float *d_means, int *iters_out, int *no_centre_out,
                      KmeansPhases *phases, int *failed_dev) {
  const int d = seg * L, n = rows, n_runs = 2 * T;
  if (G < 1 || G > KMEANS_MAX_DEVS) return hipErrorInvalidValue;
  hipStream_t st = devs[0].st;
  hipError_t e;
  int at = 0;  // the device the current call belongs to
  if (failed_dev) *failed_dev = 0;
#define KM_TRY(expr)                         \
  do {                                       \
    if ((e = (expr)) != hipSuccess) {        \
      if (failed_dev) *failed_dev = at;      \
      return e;                              \
    }                                        \
  } while (0)
  // device 0's buffers (freed on return, after the streams are synchronised)
  vaqhost::DevBuf b_x, b_seed, b_keys_in, b_keys_out, b_vals_in, b_vals_out, b_bounds, b_part, b_flags, b_temp;
  KmParts ps(devs, G);
  KM_TRY(ps.use(0));
  const int n_flags = 2 + G;  // centres changed, a row without a centre on device 0, the same from devices 1..
  KM_TRY(b_x.ensure((size_t)n * d * sizeof(float)));
  KM_TRY(b_seed.ensure((size_t)T * sizeof(int)));
  KM_TRY(b_keys_in.ensure((size_t)n * 4));
  KM_TRY(b_keys_out.ensure((size_t)n * 4));
  KM_TRY(b_vals_in.ensure((size_t)n * 4));
  KM_TRY(b_vals_out.ensure((size_t)n * 4));
  KM_TRY(b_bounds.ensure((size_t)2 * n_runs * sizeof(int)));
  KM_TRY(b_part.ensure((size_t)n_runs * d * sizeof(float)));
  KM_TRY(b_flags.ensure((size_t)n_flags * sizeof(int)));
  float *X = b_x.as<float>();
  unsigned *keys_in = b_keys_in.as<unsigned>(), *keys_out = b_keys_out.as<unsigned>();
  unsigned *vals_in = b_vals_in.as<unsigned>(), *vals_out = b_vals_out.as<unsigned>();
  int *start = b_bounds.as<int>(), *end = start + n_runs, *flags = b_flags.as<int>();
  unsigned key_bits = 1;
  while ((1u << key_bits) < (unsigned)n_runs) key_bits++;
  size_t temp_bytes = 0;
  KM_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, key_bits,
                                   st));
  KM_TRY(b_temp.ensure(temp_bytes ? temp_bytes : 16));

  // device 0 holds every decoded row (the sums are its alone) and the centres
  const int64_t nd = (int64_t)n * d;
  hipLaunchKernelGGL(km_decode_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, d_scodes, (int64_t)n,
                     seg, L, devs[0].sub, devs[0].cent, X);
  KM_TRY(hipGetLastError());
  KM_TRY(hipMemcpyAsync(b_seed.p, seed_rows, (size_t)T * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(km_seed_kernel, dim3((unsigned)((T * d + 255) / 256)), dim3(256), 0, st, X, d,
                     b_seed.as<int>(), T, d_means);
  KM_TRY(hipGetLastError());
  // devices 1..: their slice of the sample's codes by peer copy, decoded there
  for (int g = 0; g < G; g++) {
    int slice_end = 0;
    kmeans_assign_slice(n, G, g, &ps.part[(size_t)g].row0, &slice_end);
    ps.part[(size_t)g].n = slice_end - ps.part[(size_t)g].row0;
  }
  if (G > 1) {
    KM_TRY(hipEventCreateWithFlags(&ps.fed, hipEventDisableTiming));
    KM_TRY(hipEventRecord(ps.fed, st));
  }
  for (int g = 1; g < G; g++) {
    KmPart &p = ps.part[(size_t)g];
    if (p.n == 0) continue;
    at = g;
    KM_TRY(ps.use(g));
    KM_TRY(hipEventCreateWithFlags(&p.assigned, hipEventDisableTiming));
    KM_TRY(p.scodes.ensure((size_t)p.n * seg * sizeof(uint16_t)));
    KM_TRY(p.x.ensure((size_t)p.n * d * sizeof(float)));
    KM_TRY(p.means.ensure((size_t)T * d * sizeof(float)));
    KM_TRY(p.keys.ensure((size_t)p.n * 4));
    KM_TRY(p.vals.ensure((size_t)p.n * 4));
    KM_TRY(p.flags.ensure(2 * sizeof(int)));
    KM_TRY(hipStreamWaitEvent(devs[g].st, ps.fed, 0));
    KM_TRY(hipMemcpyPeerAsync(p.scodes.p, devs[g].device, d_scodes + (size_t)p.row0 * seg, devs[0].device,
                              (size_t)p.n * seg * sizeof(uint16_t), devs[g].st));
    const int64_t pd = (int64_t)p.n * d;
    hipLaunchKernelGGL(km_decode_kernel, dim3((unsigned)((pd + 255) / 256)), dim3(256), 0, devs[g].st,
                       p.scodes.as<uint16_t>(), (int64_t)p.n, seg, L, devs[g].sub, devs[g].cent, p.x.as<float>());
    KM_TRY(hipGetLastError());
  }
  at = 0;
  KM_TRY(ps.use(0));

  // launch shape of the assign kernel: the widest workgroup whose tile of decoded rows fits
  int R = 256;
  while (R > 64 && (size_t)R * d * sizeof(float) > KM_TILE_BYTES) R >>= 1;
  const bool x_lds = (size_t)R * d * sizeof(float) <= KM_TILE_BYTES;
  const int stage = std::max(1, std::min(T, KM_STAGE_FLOATS / d));
  const size_t lds = ((size_t)stage * d + (x_lds ? (size_t)R * d : 0)) * sizeof(float);
  const int half_rows = (n + 1) / 2;  // schedule(static) over two threads
  auto assign = [&](int g, const float *x, const float *means, unsigned *keys, unsigned *vals, int *fl) {
    const KmPart &p = ps.part[(size_t)g];
    const unsigned grid = (unsigned)((p.n + R - 1) / R);
    if (x_lds)
      hipLaunchKernelGGL(km_assign_kernel<true>, dim3(grid), dim3(R), lds, devs[g].st, x, p.n, d, means, T, stage,
                         half_rows, p.row0, keys, vals, fl);
    else
      hipLaunchKernelGGL(km_assign_kernel<false>, dim3(grid), dim3(R), lds, devs[g].st, x, p.n, d, means, T, stage,
                         half_rows, p.row0, keys, vals, fl);
    return hipGetLastError();
  };

  if (phases) *phases = KmeansPhases{};
  auto phase_end = [&](double *acc, std::chrono::steady_clock::time_point &t0) -> hipError_t {
    if (!phases) return hipSuccess;
    hipError_t pe = hipStreamSynchronize(st);
    *acc += ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    return pe;
  };
  int iters = 0, no_centre = 0, host_flags[2 + KMEANS_MAX_DEVS] = {1, 0};
  if (phases) KM_TRY(hipStreamSynchronize(st));
  auto t0 = std::chrono::steady_clock::now();
  while (host_flags[0] && iters < max_iter) {
    // assign: every device its slice against the current centres.  Every call is checked here, on the host,
    // before device 0 is made to wait for any of it: a device that fails leaves no stream waiting.
    KM_TRY(hipMemsetAsync(flags, 0, (size_t)n_flags * sizeof(int), st));
    KM_TRY(hipMemsetAsync(start, 0, (size_t)2 * n_runs * sizeof(int), st));
    if (ps.part[0].n > 0) KM_TRY(assign(0, X, d_means, keys_in, vals_in, flags));
    for (int g = 1; g < G; g++) {
      KmPart &p = ps.part[(size_t)g];
      if (p.n == 0) continue;
      at = g;
      KM_TRY(ps.use(g));
      KM_TRY(hipStreamWaitEvent(devs[g].st, ps.fed, 0));
      KM_TRY(hipMemcpyPeerAsync(p.means.p, devs[g].device, d_means, devs[0].device, (size_t)T * d * sizeof(float),
                                devs[g].st));
      KM_TRY(hipMemsetAsync(p.flags.p, 0, 2 * sizeof(int), devs[g].st));
      KM_TRY(assign(g, p.x.as<float>(), p.means.as<float>(), p.keys.as<unsigned>(), p.vals.as<unsigned>(),
                    p.flags.as<int>()));
      KM_TRY(hipEventRecord(p.assigned, devs[g].st));
    }
    at = 0;
    KM_TRY(ps.use(0));
    for (int g = 1; g < G; g++) {
      const KmPart &p = ps.part[(size_t)g];
      if (p.n == 0) continue;
      KM_TRY(hipStreamWaitEvent(st, p.assigned, 0));
      KM_TRY(hipMemcpyPeerAsync(keys_in + p.row0, devs[0].device, p.keys.p, devs[g].device, (size_t)p.n * 4, st));
      KM_TRY(hipMemcpyPeerAsync(vals_in + p.row0, devs[0].device, p.vals.p, devs[g].device, (size_t)p.n * 4, st));
      KM_TRY(hipMemcpyPeerAsync(flags + 2 + g, devs[0].device, p.flags.as<int>() + 1, devs[g].device, sizeof(int), st));
    }
    KM_TRY(phase_end(phases ? &phases->assign_ms : nullptr, t0));
    // stable: rows of equal (half, centre) stay in ascending order
    KM_TRY(rocprim::radix_sort_pairs(b_temp.p, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u,
                                     key_bits, st));
    hipLaunchKernelGGL(km_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys_out, n, start, end);
    KM_TRY(hipGetLastError());
    hipLaunchKernelGGL(km_accumulate_kernel, dim3((unsigned)(((int64_t)n_runs * d + 255) / 256)), dim3(256), 0, st, X,
                       d, vals_out, start, end, n_runs, b_part.as<float>());
    KM_TRY(hipGetLastError());
    KM_TRY(phase_end(phases ? &phases->accumulate_ms : nullptr, t0));
    hipLaunchKernelGGL(km_update_kernel, dim3(T), dim3(64), 0, st, b_part.as<float>(), start, end, T, d, d_means,
                       flags);
    KM_TRY(hipGetLastError());
    if (G > 1) KM_TRY(hipEventRecord(ps.fed, st));
    KM_TRY(hipMemcpyAsync(host_flags, flags, (size_t)n_flags * sizeof(int), hipMemcpyDeviceToHost, st));
    KM_TRY(hipStreamSynchronize(st));
    KM_TRY(phase_end(phases ? &phases->update_ms : nullptr, t0));
    iters++;
    for (int i = 1; i < n_flags; i++) no_centre |= host_flags[i];
    if (no_centre) break;
  }
  KM_TRY(hipStreamSynchronize(st));
#undef KM_TRY
  *iters_out = iters;
  *no_centre_out = no_centre;
  return hipSuccess;
}

} // namespace vaq
