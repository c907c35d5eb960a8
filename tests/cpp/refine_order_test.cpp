// refine_order_test.cpp -- the code the refine kernel shares with the host, vaq::sq_norm_eigen and vaq::refheap
// (vaq_amd/csrc/vaq_restated.h), run as VAQ::refine's loop (VAQ.cpp:859-873) over the inputs of the fixtures under
// tests/golden/refine/ and compared with the answers recorded from the reference: distances bit for bit, labels
// exactly.
//
//   refine_order_test IN
// IN: int32 count, then per case int32 nq, D, N, R, k; XTest nq x D, XTrain N x D float32; candidates nq x R int32
// (all inside [0, N)); the recorded labels nq x k int32 and distances nq x k float32.
// Built by tests/test_refine_exact_cpu.py with plain g++ (-D__HIP_PLATFORM_AMD__ -I<rocm>/include -Ivaq_amd/csrc
// -ffp-contract=off); it is also built with -fsanitize=address,undefined and run on its own.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vaq_restated.h"

static void read_exact(void *p, size_t bytes, FILE *f) {
  if (bytes && std::fread(p, 1, bytes, f) != bytes) {
    std::fprintf(stderr, "refine_order_test: short input\n");
    std::exit(2);
  }
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: refine_order_test IN\n");
    return 2;
  }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) {
    std::fprintf(stderr, "refine_order_test: cannot open %s\n", argv[1]);
    return 2;
  }
  int32_t count;
  read_exact(&count, sizeof count, in);
  int bad = 0;
  for (int c = 0; c < count; c++) {
    int32_t h[5];
    read_exact(h, sizeof h, in);
    const int nq = h[0], D = h[1], N = h[2], R = h[3], k = h[4];
    if (nq < 0 || D < 1 || N < 1 || R < 1 || k < 1 || k > R || R > 4096 || D > 4096) {
      std::fprintf(stderr, "refine_order_test: case %d has nq=%d D=%d N=%d R=%d k=%d\n", c, nq, D, N, R, k);
      return 2;
    }
    std::vector<float> xq((size_t)nq * D), xt((size_t)N * D), want_d((size_t)nq * k);
    std::vector<int32_t> cand((size_t)nq * R), want_l((size_t)nq * k);
    read_exact(xq.data(), xq.size() * 4, in);
    read_exact(xt.data(), xt.size() * 4, in);
    read_exact(cand.data(), cand.size() * 4, in);
    read_exact(want_l.data(), want_l.size() * 4, in);
    read_exact(want_d.data(), want_d.size() * 4, in);
    std::vector<float> hv((size_t)k), out_d((size_t)k);
    std::vector<int> hi((size_t)k), out_l((size_t)k);
    bool ok = true;
    for (int q = 0; q < nq && ok; q++) {
      vaq::refheap::heapify(k, hv.data(), hi.data());
      for (int i = 0; i < R; i++) {
        const int lab = cand[(size_t)q * R + i];
        if (lab < 0 || lab >= N) {
          std::fprintf(stderr, "refine_order_test: case %d: label %d outside the rows\n", c, lab);
          return 2;
        }
        const float dist = vaq::sq_norm_eigen<true>(xq.data() + (size_t)q * D, 1, xt.data() + (size_t)lab * D, D);
        if (hv[0] > dist) {
          vaq::refheap::pop(k, hv.data(), hi.data());
          vaq::refheap::push(k, hv.data(), hi.data(), dist, lab);
        }
      }
      const int kept = vaq::refheap::reorder(k, hv.data(), hi.data());
      for (int i = 0; i < k; i++) {
        out_l[(size_t)i] = i < kept ? hi[(size_t)(k - kept + i)] : -1;
        out_d[(size_t)i] = i < kept ? hv[(size_t)(k - kept + i)] : FLT_MAX;
      }
      ok = std::memcmp(out_l.data(), want_l.data() + (size_t)q * k, (size_t)k * 4) == 0 &&
           std::memcmp(out_d.data(), want_d.data() + (size_t)q * k, (size_t)k * 4) == 0;
      if (!ok) std::fprintf(stderr, "refine_order_test: case %d (D=%d R=%d k=%d) differs at query %d\n", c, D, R, k, q);
    }
    if (!ok) bad++;
  }
  std::fclose(in);
  if (bad) {
    std::fprintf(stderr, "refine_order_test: %d of %d cases differ\n", bad, count);
    return 1;
  }
  std::printf("refine_order_test: ok (%d cases)\n", count);
  return 0;
}
