// vaqhip_multi_learn.cpp -- learnQuantization's device forms on the multi-device index (include/vaqhip.h, "Learning on
// the device").  _u8 is shard 0's vaqhip_learn_quantization_u8, replicated as the float form is.  _from_refiner reads
// the rows a multi refiner holds, where they are:
//   1 gather  the sample (permutation_head) is cut by the shard that holds each row (kmeans_split_sample); every shard,
//             on its own worker, device and stream, gathers its rows as floats (vaq_learn.hip, a byte widened), copies
//             the block to the first device and records an event behind the copy
//   2 place   the first device's stream waits for those events and puts the blocks' rows at their sample positions
//             (the same gather kernel over the staged blocks); the host waits for that stream alone
//   3 learn   vaqhip_internal_learn_sample_device on shard 0, the result to every other shard through
//             vaqhip_index_set_lut_quantization
// The scratch is the call's: two sample x D float buffers on the first device, one block per shard (released by
// idle_then_release, vaqhip_shard_run.h).
#include "vaqhip_shard_run.h"

#include <chrono>
#include <cstring>

#include "kmeans_sample.h"
#include "vaq_learn.h"

using namespace vaqhost;

namespace {

struct GatherPart {
  DevBuf idx, block;  // the shard's sampled rows (local), gathered as floats [cnt][D]
  int64_t at = 0;     // the block's first row among the staged blocks
  hipEvent_t copied = nullptr;  // the block is on the first device
  bool held() const { return idx.p || block.p || copied; }
  void release() { release_all({&idx, &block}), destroy_events(&copied, 1); }
};

// every shard gets shard 0's result (mx->mu held)
int replicate(vaqhip_multi *mx, int rc, const std::vector<float> &off, const std::vector<float> &sc, float *offsets_out,
              float *scale_out) {
  for (int g = 1; !rc && g < mx->G; g++) rc = vaqhip_index_set_lut_quantization(mx->sh[g].ix, off.data(), sc.data());
  if (forward(rc)) return rc;
  mx->fast_q = true;
  if (offsets_out) std::memcpy(offsets_out, off.data(), off.size() * sizeof(float));
  if (scale_out) std::memcpy(scale_out, sc.data(), sc.size() * sizeof(float));
  return VAQHIP_OK;
}

}  // namespace

extern "C" {

int vaqhip_multi_learn_quantization_u8(vaqhip_multi *mx, const uint8_t *X, int64_t n, int projected, float sample_ratio,
                                       float *offsets_out, float *scale_out) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  std::lock_guard<std::mutex> lk(mx->mu);
  DeviceGuard keep(DeviceGuard::restore_only);
  std::vector<float> off((size_t)mx->M), sc((size_t)mx->M);
  const int rc = vaqhip_learn_quantization_u8(mx->sh[0].ix, X, n, projected, sample_ratio, off.data(), sc.data());
  return replicate(mx, rc, off, sc, offsets_out, scale_out);
}

int vaqhip_multi_learn_quantization_from_refiner(vaqhip_multi *mx, vaqhip_multi_refiner *r, float sample_ratio,
                                                 float *offsets_out, float *scale_out) {
  if (!mx) return mfail(VAQHIP_EINVAL, "multi index is null");
  if (!r) return mfail(VAQHIP_EINVAL, "multi refiner is null");
  std::lock_guard<std::mutex> lr(r->mu);  // (the order of vaqhip_multi_search_refine: the refiner, then the index)
  std::lock_guard<std::mutex> lk(mx->mu);
  if (const int rc = check_refiner_pair(mx, r)) return rc;
  if (!vaqhip_internal_fast_ok(mx->sh[0].ix))
    return mfail(VAQHIP_EUNSUPPORTED, "FAST needs max bits per subspace <= 4 and the grouped row sum");
  const int64_t n = r->N;
  if (n > 0x7fffffffLL) return mfail(VAQHIP_ERANGE, "the reference's rows are int: n = %lld", (long long)n);
  const int sample = static_cast<int>(sample_ratio * (float)n);  // VAQ.cpp:1120
  if (!(sample >= 1)) return mfail(VAQHIP_EINVAL, "sampleSize = int(%g * %lld) < 1", sample_ratio, (long long)n);
  if (sample > n) return mfail(VAQHIP_EINVAL, "sampleSize = int(%g * %lld) > n: the permutation has n entries", sample_ratio, (long long)n);

  const auto t0 = std::chrono::steady_clock::now();
  const int G = r->G, D = r->D;
  int64_t lo[VAQHIP_MAX_DEVICES], cnt[VAQHIP_MAX_DEVICES];
  for (int g = 0; g < G; g++) lo[g] = r->sh[g].lo, cnt[g] = r->sh[g].n;
  const std::vector<int> perm = vaq::permutation_head(n, sample);
  const std::vector<vaq::KmeansShardSample> cut = vaq::kmeans_split_sample(perm, lo, cnt, G);
  // where each sample position's row sits among the staged blocks (shard after shard, sample order within a shard)
  std::vector<int> place((size_t)sample, -1);
  std::vector<GatherPart> part((size_t)G);
  int64_t staged = 0;
  for (int g = 0; g < G; g++) {
    part[(size_t)g].at = staged;
    for (size_t j = 0; j < cut[(size_t)g].pos.size(); j++) place[(size_t)cut[(size_t)g].pos[j]] = (int)(staged + (int64_t)j);
    staged += (int64_t)cut[(size_t)g].pos.size();
  }
  if (staged != sample) return mfail(VAQHIP_ESTATE, "the shards hold %lld of the %d sampled rows", (long long)staged, sample);

  DeviceGuard keep(DeviceGuard::restore_only);  // (declared before the buffers: it puts the device back after they went)
  const int dev0 = r->sh[0].device;
  DevBuf d_stage, d_rows, d_place;
  // the blocks are the shards': freed with their device current and every shard's stream idle, however the call ends
  struct PartsFree {
    vaqhip_multi_refiner *r;
    std::vector<GatherPart> &part;
    int dev0;
    ~PartsFree() {
      idle_then_release(part, [&](int g) { return ShardAt{r->sh[g].device, r->sh[g].stream}; });
      (void)hipSetDevice(dev0);  // (for the first device's buffers, which go next)
    }
  } parts_free{r, part, dev0};
  if (hipSetDevice(dev0) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", dev0);
  hipError_t e = d_stage.ensure((size_t)sample * D * sizeof(float));
  if (e == hipSuccess) e = d_rows.ensure((size_t)sample * D * sizeof(float));
  if (e == hipSuccess) e = d_place.ensure((size_t)sample * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(d_place.p, place.data(), (size_t)sample * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) return mfail(hip_code(e), "device %d: %s", dev0, hipGetErrorString(e));

  // 1 gather: every shard its own rows, pushed to the first device, an event behind the copy
  float *stage = d_stage.as<float>();
  if (const int rc = on_shards(r, [&](int g, RShard &s) -> int {
        const std::vector<int> &local = cut[(size_t)g].local;
        if (local.empty()) return 0;
        GatherPart &p = part[(size_t)g];
        const int m = (int)local.size();
        MHIP(hipSetDevice(s.device));
        MHIP(hipEventCreateWithFlags(&p.copied, hipEventDisableTiming));
        MHIP(p.idx.ensure((size_t)m * sizeof(int)));
        MHIP(p.block.ensure((size_t)m * D * sizeof(float)));
        MHIP(hipMemcpyAsync(p.idx.p, local.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s.stream));
        MHIP(vaq::launch_learn_gather(s.rows.rows(), p.idx.as<int>(), m, D, p.block.as<float>(), s.stream));
        float *dst = stage + (size_t)p.at * D;
        MHIP(copy_between(dst, dev0, p.block.p, s.device, (size_t)m * D * sizeof(float), s.stream));
        MHIP(hipEventRecord(p.copied, s.stream));
        return 0;
      }))
    return rc;

  // 2 place, on the first device, behind every shard's copy (`cut` and the blocks outlive the wait below)
  RShard &s0 = r->sh[0];
  if (hipSetDevice(dev0) != hipSuccess) return mfail(VAQHIP_ENODEVICE, "hipSetDevice(%d) failed", dev0);
  e = hipSuccess;
  for (int g = 0; g < G && e == hipSuccess; g++)
    if (part[(size_t)g].copied) e = hipStreamWaitEvent(s0.stream, part[(size_t)g].copied, 0);
  if (e == hipSuccess)
    e = vaq::launch_learn_gather(vaq::RowsRef{d_stage.p, 4}, d_place.as<int>(), sample, D, d_rows.as<float>(), s0.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s0.stream);
  if (e != hipSuccess) return mfail(hip_code(e), "device %d: %s", dev0, hipGetErrorString(e));
  const float gather_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();

  // 3 learn on shard 0 (raw rows: projected = 0), then every shard
  std::vector<float> off((size_t)mx->M), sc((size_t)mx->M);
  const int rc = vaqhip_internal_learn_sample_device(mx->sh[0].ix, d_rows.as<float>(), sample, 0, gather_ms, off.data(), sc.data());
  return replicate(mx, rc, off, sc, offsets_out, scale_out);
}

}  // extern "C"
