// demo_vaqhip.cpp -- the query half of the reference's examples/demo_vaq.cpp
// (:58-92 load, :336-363 search + recall) on the MI355X path.  The PCA and the
// bit allocation of VAQ::train are out of scope (they need glpk / armadillo in
// the reference), so the index is read from the files `demo_vaq --save
// <centroids> --save-enc <codebook>` writes, plus the rotation (which the
// reference never persists) as a raw D x D float32 file -- or, with
// --fit-codebooks and --encode, built here from the raw vectors, the rotation
// and the bits.
//
//   demo_vaqhip --centroids c.bin --codebook cb.bin [--eigen e.f32] \
//               --queries q.fvecs --timeseries-size 128 [--queries-size N] \
//               --method VAQ64m8min8max8var1,HEAP --k 100 \
//               [--groundtruth gt.ivecs] [--result out.csv] [--bits 8,8,...]
//               [--visit-cluster 0.25]     (demo_vaq.cpp:43,57; with a ...,EA_TI<T>m<seg> method)
//               [--ti-clusters c.f32]      (raw T x seg*L float32; default: clusterTI(true), the reference's k-means
//                                           on the GPU -- over the shards with --devices)
//               [--refine 100,200 --dataset base.fvecs [--dataset-size N]]   (or --dataset-refine)
//                                          (demo_vaq.cpp:40, :312-345 and scripts/run_demos.sh:9,22: per value R,
//                                           search R >= k candidates, then VAQ::refine re-ranks them against the
//                                           raw vectors; results go to <result>_R<R> when several R are given)
//               [--refine-resident]        (with --refine: the raw vectors are uploaded once and every R is ONE fused
//                                           call, search + refine with the candidates kept on the device; distances in
//                                           the reference's (Eigen's) summation order; needs --timeseries-size == D.
//                                           --exact-ties 1: also the reference heap's tie order.  With --devices the
//                                           raw vectors are cut over the same GPUs as the code rows: same answer)
//               [--exact-groundtruth]      (without --groundtruth: the true k nearest rows of every query are computed
//                                           on the device from the raw vectors -- --dataset, resident as with
//                                           --refine-resident; with --devices cut over the same GPUs, same answer --
//                                           and the recall lines are printed against them)
//               [--file-format-ori bvecs]  (demo_vaq.cpp:23: --dataset, --dataset-refine and --queries are bvecs files,
//                                           SIFT1B / BIGANN.  With --refine-resident and / or --exact-groundtruth the
//                                           raw vectors go to the device as the BYTES the file holds, a quarter of the
//                                           memory, same answers; everything else reads them widened to float, as the
//                                           reference does.  Default fvecs)
//               [--devices 0,1,2,3]        (shard the rows over these GPUs: RCCL all-gather + merge)
//               [--encode --dataset base.fvecs [--save-enc cb.bin]]
//                                          (instead of --codebook: VAQ::encode of the raw vectors, mEigenVectors applied.
//                                           With --devices every shard encodes the rows it will hold and keeps their
//                                           codes; with --devices and --refine-resident the rows are uploaded once, cut
//                                           over the GPUs, and encoded where they lie -- the same codes either way)
//               [--fit-codebooks --bits 8,8,... --dataset base.fvecs [--save c.bin] [--max-iter 25]]
//               [--kmeans-ver 1]                 with --fit-codebooks or --train: subspaces above 8 bits are fitted
//                                           hierarchically, 128 x 2^(bits-7) centres (demo_vaq's switch; 2 is refused)
//               [--kmeans-binary]                with --fit-codebooks or --train: the way to the binary fit -- subspaces
//                                           above 8 bits as a tree of 2-centre fits (the rule of demo_vaq's --kmeans-ver 2);
//                                           not together with --kmeans-ver 1
//                                          (instead of --centroids: the subspace codebooks are fitted on the GPU from
//                                           the raw vectors by KMeans::staticFitSampling, the call of VAQ.cpp:644-649 --
//                                           not the arma::kmeans call VAQ::train runs today; --eigen is applied first,
//                                           the bits are the caller's.  --file-format-ori bvecs fits from the bytes,
//                                           --refine-resident from the rows on the device.  With --devices the fit is
//                                           sharded: the rows are cut over the GPUs, subspace s is fitted on device
//                                           s % G, the same centres bit for bit.  --save writes them as
//                                           demo_vaq --save does; composes with --encode; without --queries it ends there)
//               [--train --bit-budget 128 --subspaces 16 [--min-bits 1 --max-bits 12 --var 1] --dataset base.fvecs]
//                                          (instead of --centroids, --eigen and --bits: VAQ::train from the raw vectors
//                                           alone -- the second moment of the sampled rows, its eigenvectors, the
//                                           partial balance, the exact bit allocation, then the codebook fit above.
//                                           min / max / var default to the method string's.  bvecs and
//                                           --refine-resident as with --fit-codebooks; no --devices.  Goes in front of
//                                           --encode: demo_vaqhip --train ... --encode --queries q.fvecs builds and
//                                           searches an index with no foreign input)
//               with a ...,FAST method (codes of at most 4 bits): --dataset base.fvecs [--dataset-size N]
//               [--learn-ratio 0.05]       (demo_vaq.cpp:42, :120-124: VAQ::learnQuantization on the raw dataset; from the
//                                           bytes with --file-format-ori bvecs, from the resident rows with --refine-resident)
//
//   demo_vaqhip --lut-bits 8,6,5,...  --dataset base.fvecs [--dataset-size N] [--eigen e.f32] \
//               --queries q.fvecs --timeseries-size 128 [--queries-size N] --k 100 [--exact-ties 1] \
//               [--result out.csv] [--save-enc cb.bin] [--groundtruth gt.ivecs] [--devices 0,1]
//       builds a queryLUT index (BitVecEngine::binaryEncodingLUT from the bit allocation on: quantile
//       codebooks and codes on the GPU; the PCA rotation and the bits per dimension are the caller's, as
//       with the reference's hardcoded solutionX) over the first len(bits) PCA dimensions and queries it.
//       With --devices the build is sharded: the fit runs over these GPUs (dimension d on device d % G, no GPU
//       holds all rows), every shard encodes the rows it will hold, and the queries go to the multi index --
//       the same codebook and answers
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>

#include "vaqhip_io.hpp"

using namespace vaqhip;

static std::vector<int> intList(const std::string &csv) {
  std::vector<int> v;
  std::stringstream ss(csv);
  std::string t;
  while (std::getline(ss, t, ',')) v.push_back(std::atoi(t.c_str()));
  return v;
}

// --file-format-ori (demo_vaq.cpp:75-83): fvecs, or bvecs widened to float as readBVecsFromExternal widens them
static bool g_bvecs = false;
static RowMatrixF readOri(const std::string &path, int N, int maxRow, int pad) {
  return g_bvecs ? readBVecs(path, N, maxRow, pad) : readFVecs(path, N, maxRow, pad);
}

// --lut-bits: build and query BitVecEngine's LUT index
static int lutMain(std::map<std::string, std::string> &a) {
  for (const char *req : {"dataset", "queries"})
    if (!a.count(req)) { std::cerr << "missing --" << req << "\n"; return 2; }
  BitVecEngineHip engine;
  engine.solutionX = intList(a["lut-bits"]);
  engine.exactTies = a.count("exact-ties") && std::atoi(a["exact-ties"].c_str()) != 0;
  if (a.count("devices")) engine.setDevices(intList(a["devices"]));
  const int D = (int)engine.solutionX.size();
  const int N = std::atoi(a["timeseries-size"].c_str());
  if (D != N) throw Error(VAQHIP_EINVAL, "--lut-bits needs one entry per dimension (--timeseries-size)");
  if (a.count("eigen")) {
    engine.eigenVectors = RowMatrixF(D, D);
    detail::File f(a["eigen"], "rb");
    f.read(engine.eigenVectors.data(), sizeof(float), (size_t)D * D);
  }
  const int dsize = a.count("dataset-size") ? std::atoi(a["dataset-size"].c_str()) : -1;
  RowMatrixF dataset;
  RowMatrix<uint8_t> dataset8;  // bvecs: the dataset as the file holds it, fitted and encoded from the bytes
  if (g_bvecs) dataset8 = readBVecsU8(a["dataset"], N, dsize);
  else dataset = readOri(a["dataset"], N, dsize, 0);
  RowMatrixF queries = readOri(a["queries"], N, std::atoi(a["queries-size"].c_str()), 0);
  const int k = std::atoi(a["k"].c_str());
  CodebookType codebook;
  auto t0 = std::chrono::steady_clock::now();
  if (g_bvecs) engine.binaryEncodingLUT(dataset8, codebook);
  else engine.binaryEncodingLUT(dataset, codebook);
  std::cout << "== Encoding time: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
            << " s (" << codebook.rows() << " rows x " << D << " dimensions, quantile codebooks + codes"
            << (g_bvecs ? ", from byte rows" : "") << ")" << std::endl;
  if (engine.multiHandle()) {
    vaqhip_multi_lut_fit_timing ft;
    vaqhip_multi_encode_timing et;
    if (vaqhip_multi_last_lut_fit_timing(&ft) == 0 && vaqhip_multi_last_encode_timing(engine.multiHandle(), &et) == 0)
      std::cout << "   across " << ft.n_devices << " shards: fit " << ft.total_ms << " ms (columns " << ft.columns_ms
                << ", copy " << ft.copy_ms << ", sort " << ft.sort_ms << ", quantiles " << ft.quantile_ms << ", means "
                << ft.means_ms << "), encode + set " << et.total_ms << " ms" << std::endl;
  }
  if (a.count("save-enc")) saveCodebook(codebook, a["save-enc"]);
  t0 = std::chrono::steady_clock::now();
  auto answers = engine.queryLUT(queries, k, codebook);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::cout << "== Querying time: " << sec << " s (" << queries.rows() / sec << " queries/s)" << std::endl;
  LabelDistVecF flat;
  for (auto &ans : answers)
    for (int i = 0; i < k; i++) {
      flat.labels.push_back(i < (int)ans.size() ? ans[i].idx : -1);
      flat.distances.push_back(i < (int)ans.size() ? ans[i].dist : 0.0f);
    }
  if (a.count("result")) writeKNNResults(a["result"], flat, queries.rows());
  if (a.count("groundtruth")) {
    RowMatrix<int> gt = readIVecs(a["groundtruth"], k);
    std::cout << "\tprecision(avg_recall): " << getAvgRecall(flat.labels, gt, k) << std::endl;
  }
  return 0;
}

int main(int argc, char **argv) {
  std::map<std::string, std::string> a = {{"k", "100"}, {"method", "VAQ64m8min8max8var1,HEAP"},
                                          {"timeseries-size", "128"}, {"queries-size", "-1"}};
  for (int i = 1; i < argc; i += 2) {
    if (std::strcmp(argv[i], "--refine-resident") == 0 || std::strcmp(argv[i], "--exact-groundtruth") == 0 ||
        std::strcmp(argv[i], "--encode") == 0 || std::strcmp(argv[i], "--fit-codebooks") == 0 ||
        std::strcmp(argv[i], "--train") == 0 || std::strcmp(argv[i], "--kmeans-binary") == 0) {
      a[argv[i] + 2] = "1";  // the switches without a value
      i--;
      continue;
    }
    if (i + 1 >= argc) break;
    if (std::strncmp(argv[i], "--", 2) != 0) { std::cerr << "bad argument " << argv[i] << "\n"; return 2; }
    a[argv[i] + 2] = argv[i + 1];
  }
  if (a.count("file-format-ori") && a["file-format-ori"] != "fvecs" && a["file-format-ori"] != "bvecs") {
    std::cerr << "--file-format-ori " << a["file-format-ori"] << ": fvecs or bvecs\n";
    return 2;
  }
  g_bvecs = a.count("file-format-ori") && a["file-format-ori"] == "bvecs";
  if (a.count("lut-bits")) {
    try {
      return lutMain(a);
    } catch (const std::exception &e) {
      std::cerr << "error: " << e.what() << std::endl;
      return 1;
    }
  }
  const bool train = a.count("train") != 0;  // PCA, bit allocation and codebooks from the raw vectors alone
  const bool encode = a.count("encode") != 0, fit = a.count("fit-codebooks") != 0 || train;
  const bool fit_only = fit && !encode && !a.count("codebook") && !a.count("queries");  // fit, --save, done
  std::vector<std::string> required = {train ? "bit-budget" : fit ? "bits" : "centroids"};
  if (train) required.push_back("subspaces");
  if (fit || encode) required.push_back("dataset");
  if (!encode && !fit_only) required.push_back("codebook");
  if (!fit_only) required.push_back("queries");
  for (const std::string &req : required)
    if (!a.count(req)) { std::cerr << "missing --" << req << "\n"; return 2; }
  try {
    VaqHipFast vaq;  // VaqHip plus the FAST method
    vaq.parseMethodString(a["method"]);
    if (!fit) vaq.mCentroidsPerSubs = loadCentroids(a["centroids"]);
    if (a.count("kmeans-ver")) {  // demo_vaq's switch: 0 flat, 1 hierarchical (subspaces above 8 bits), 2 binary
      const int ver = std::atoi(a["kmeans-ver"].c_str());
      if (ver == 2) throw Error(VAQHIP_EUNSUPPORTED, "--kmeans-ver 2: binary k-means is not built");
      if (ver != 0 && ver != 1) throw Error(VAQHIP_EINVAL, "--kmeans-ver takes 0 or 1");
      vaq.mHierarchicalKmeans = ver == 1;
    }
    if (a.count("kmeans-binary")) {  // the binary-tree fit (the rule of demo_vaq's --kmeans-ver 2)
      if (vaq.mHierarchicalKmeans) throw Error(VAQHIP_EINVAL, "--kmeans-binary and --kmeans-ver 1 name two different fits");
      vaq.mBinaryKmeans = true;
    }
    if (!encode && !fit_only) vaq.mCodebook = loadCodebook(a["codebook"]);
    if (train) {  // the method string's min / max / var hold unless the flags name others
      if (a.count("devices")) throw Error(VAQHIP_EUNSUPPORTED, "--train has no multi-device form");
      if (a.count("eigen") || a.count("bits")) throw Error(VAQHIP_EINVAL, "--train computes the rotation and the bits: no --eigen, no --bits");
      vaq.mBitBudget = std::atoi(a["bit-budget"].c_str());
      vaq.mSubspaceNum = std::atoi(a["subspaces"].c_str());
      if (a.count("min-bits")) vaq.mMinBitsPerSubs = std::atoi(a["min-bits"].c_str());
      if (a.count("max-bits")) vaq.mMaxBitsPerSubs = std::atoi(a["max-bits"].c_str());
      if (a.count("var")) vaq.mPercentVarExplained = (float)std::atof(a["var"].c_str());
    }
    const int M = train ? vaq.mSubspaceNum : fit ? (int)intList(a["bits"]).size() : (int)vaq.mCentroidsPerSubs.size();
    if (train) {
    } else if (a.count("bits")) {  // --hc-bitalloc style list (demo_vaq.cpp:94-97)
      std::stringstream ss(a["bits"]);
      std::string t;
      while (std::getline(ss, t, ',')) vaq.mBitsAlloc.push_back(std::atoi(t.c_str()));
    } else {
      for (int s = 0; s < M; s++) vaq.mBitsAlloc.push_back((int)std::lround(std::log2((double)vaq.mCentroidsPerSubs[s].rows())));
    }
    const int N = std::atoi(a["timeseries-size"].c_str());
    const int D = fit ? N : vaq.mTotalDim();  // (a fit works on the raw vectors as they are: no padding)
    if (a.count("eigen")) {
      vaq.mEigenVectors = RowMatrixF(D, D);
      detail::File f(a["eigen"], "rb");
      f.read(vaq.mEigenVectors.data(), sizeof(float), (size_t)D * D);
    }
    if (a.count("devices")) {
      std::vector<int> devs;
      std::stringstream ss(a["devices"]);
      std::string t;
      while (std::getline(ss, t, ',')) devs.push_back(std::atoi(t.c_str()));
      vaq.setDevices(devs);
      std::cout << "sharding the rows over " << devs.size() << " device entr" << (devs.size() == 1 ? "y" : "ies") << std::endl;
    }
    RowMatrixF datasetrefine;
    RowMatrix<uint8_t> datasetrefine8;  // bvecs: the raw vectors of the resident paths, as bytes
    // the raw vectors of a resident path: read as the file holds them and uploaded that way
    auto uploadRefine = [&](const std::string &path, int maxRow) -> size_t {
      if (g_bvecs) {
        datasetrefine8 = readBVecsU8(path, N, maxRow);
        vaq.setRefineDataset(datasetrefine8);
        return datasetrefine8.rows();
      }
      if (datasetrefine.rows() == 0) datasetrefine = readFVecs(path, N, maxRow, 0);
      vaq.setRefineDataset(datasetrefine);
      return datasetrefine.rows();
    };
    size_t resident_rows = 0;
    bool uploaded = false;  // the raw vectors are resident already (--encode with --refine-resident)
    if (fit) {  // VAQ.cpp:628-660 by the call of :644-649
      const int dsize = a.count("dataset-size") ? std::atoi(a["dataset-size"].c_str()) : -1;
      const int max_iter = a.count("max-iter") ? std::atoi(a["max-iter"].c_str()) : 25;
      const char *from = "";
      auto t0 = std::chrono::steady_clock::now();
      if (a.count("refine-resident")) {  // (with --devices: the rows cut over them, fitted where they lie)
        resident_rows = uploadRefine(a.count("dataset-refine") ? a["dataset-refine"] : a["dataset"], dsize);
        uploaded = true;
        t0 = std::chrono::steady_clock::now();
        if (train) vaq.trainRefineDataset(max_iter);
        else vaq.fitCodebooksRefineDataset(max_iter);
        from = " (from the resident rows)";
      } else if (g_bvecs) {
        RowMatrix<uint8_t> dataset8 = readBVecsU8(a["dataset"], N, dsize);
        t0 = std::chrono::steady_clock::now();
        if (train) vaq.train(dataset8, max_iter);
        else vaq.fitCodebooks(dataset8, max_iter);
        from = " (from the byte rows of the bvecs file)";
      } else {
        RowMatrixF dataset = readFVecs(a["dataset"], N, dsize, 0);
        t0 = std::chrono::steady_clock::now();
        if (train) vaq.train(dataset, max_iter);
        else vaq.fitCodebooks(dataset, max_iter);
      }
      if (train) {  // VAQ.cpp:11-524: what the reference prints of its allocation
        vaqhip_train_timing tt;
        check(vaqhip_last_train_timing(&tt));
        std::cout << "== PCA computation time: " << (tt.moment_ms + tt.eigen_ms) / 1000.0 << " s (second moment of "
                  << tt.sample_rows << " rows " << tt.moment_ms << " ms, " << tt.sweeps << " Jacobi sweeps " << tt.eigen_ms
                  << " ms, plan and allocation " << tt.plan_ms << " ms)" << std::endl << "bit allocation: ";
        for (int b : vaq.mBitsAlloc) std::cout << b << ", ";
        std::cout << std::endl;
      }
      std::cout << "== Codebook fit time: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
                << " s" << from << "; iterations";
      for (int it : vaq.mCodebookIters) std::cout << " " << it;
      std::cout << "; NaN centres";
      for (int nn : vaq.mCodebookNanRows) std::cout << " " << nn;
      std::cout << std::endl;
      if (a.count("devices")) {
        vaqhip_multi_fit_codebooks_timing ft;
        if (vaqhip_multi_last_fit_codebooks_timing(&ft) == VAQHIP_OK && ft.n_devices > 0) {
          std::cout << "   across " << ft.n_devices << " shards: fit " << ft.total_ms << " ms (columns " << ft.columns_ms
                    << ", copy " << ft.copy_ms << ", place " << ft.place_ms << "); subspaces per owner";
          for (int g = 0; g < ft.n_devices; g++) std::cout << " " << ft.owner_subspaces[g];
          std::cout << std::endl;
        }
      }
      if (a.count("save")) saveCentroids(vaq.mCentroidsPerSubs, a["save"]);
      if (fit_only) return 0;
    }
    if (encode) {  // demo_vaq.cpp:126-135, from the raw vectors
      const int dsize = a.count("dataset-size") ? std::atoi(a["dataset-size"].c_str()) : -1;
      auto t0 = std::chrono::steady_clock::now();
      // (the TI centres come from the codes: encode under the method without TI, as clusterTI(true) pushes the codes)
      const uint32_t methods = vaq.mMethods, plain = methods & ~(uint32_t)VaqHip::NNMethod::TI;
      vaq.mMethods = plain ? plain : (uint32_t)VaqHip::NNMethod::Heap;
      if (a.count("devices") && a.count("refine-resident")) {
        if (N != D) throw Error(VAQHIP_EINVAL, "--encode with --refine-resident encodes the resident raw rows: --timeseries-size must be D");
        if (!uploaded) {  // (--fit-codebooks with --refine-resident has left them there)
          t0 = std::chrono::steady_clock::now();
          resident_rows = uploadRefine(a.count("dataset-refine") ? a["dataset-refine"] : a["dataset"], dsize);
          uploaded = true;
          std::cout << "== Refine dataset read + upload: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
                    << " s (" << resident_rows << " rows resident" << (g_bvecs ? ", as bytes" : "") << ")" << std::endl;
        }
        t0 = std::chrono::steady_clock::now();
        vaq.encodeRefineDataset();
      } else {
        if (a.count("refine-resident"))
          std::cout << "(--refine-resident without --devices: one device does not encode its resident rows in place, "
                       "the rows are encoded from the host matrix)" << std::endl;
        if (g_bvecs && N == D) {  // the bytes the file holds: a quarter of the host memory and of the upload
          RowMatrix<uint8_t> dataset8 = readBVecsU8(a["dataset"], N, dsize);
          t0 = std::chrono::steady_clock::now();
          vaq.encode(dataset8, false);
          std::cout << "(encoded from the byte rows of the bvecs file)" << std::endl;
        } else {  // (padded rows, D > N, are floats)
          RowMatrixF dataset = readOri(a["dataset"], N, dsize, D - N);
          t0 = std::chrono::steady_clock::now();
          vaq.encode(dataset, false);
        }
      }
      vaq.mMethods = methods;
      std::cout << "== Encoding time: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s ("
                << vaq.mCodebook.rows() << " rows" << (uploaded ? ", from the resident rows" : "") << ")" << std::endl;
      vaqhip_multi_encode_timing et;
      if (vaq.multiHandle() && vaqhip_multi_last_encode_timing(vaq.multiHandle(), &et) == 0)
        std::cout << "   across " << et.n_devices << " shards: total " << et.total_ms << " ms, encode " << et.encode_ms
                  << " ms, set codes " << et.set_codes_ms << " ms (slowest shard)" << std::endl;
      if (a.count("save-enc")) saveCodebook(vaq.mCodebook, a["save-enc"]);
    }
    if (vaq.searchMethod() & VaqHip::NNMethod::TI) {  // demo_vaq.cpp:57, :263-267
      if (a.count("visit-cluster")) vaq.mVisit = (float)std::atof(a["visit-cluster"].c_str());
      if (vaq.mTISegmentNum == -1) vaq.mTISegmentNum = M;
      if (a.count("ti-clusters")) {
        vaq.mTIClusters = RowMatrixF((size_t)vaq.mTIClusterNum, (size_t)vaq.mTISegmentNum * vaq.mSubsLen());
        detail::File f(a["ti-clusters"], "rb");
        f.read(vaq.mTIClusters.data(), sizeof(float), vaq.mTIClusters.rows() * vaq.mTIClusters.cols());
      }
      // without --ti-clusters: the reference's own k-means (demo_vaq.cpp:265), on one device or over the shards
      vaq.clusterTI(!a.count("ti-clusters"), true);
    }
    RowMatrixF queries = readOri(a["queries"], N, std::atoi(a["queries-size"].c_str()), D - N);
    const int k = std::atoi(a["k"].c_str());
    std::cout << "index: " << vaq.mCodebook.rows() << " rows x " << M << " subspaces, D=" << D
              << ", queries " << queries.rows() << ", k=" << k << std::endl;
    // --refine R1,R2,... (demo_vaq.cpp:312-323); without it one plain search (refine = 0)
    std::vector<int> refines;
    if (a.count("refine")) {
      std::stringstream ss(a["refine"]);
      std::string t;
      while (std::getline(ss, t, ',')) refines.push_back(std::atoi(t.c_str()));
    }
    if (refines.empty()) refines.push_back(0);
    bool any_refine = false;
    for (const int r : refines) any_refine = any_refine || r >= k;
    const bool resident = (any_refine && a.count("refine-resident")) || uploaded;
    const int dsize_raw = a.count("dataset-size") ? std::atoi(a["dataset-size"].c_str()) : -1;
    std::string raw_refine;
    if (any_refine) {
      // the reference re-reads --dataset for this (demo_vaq.cpp:320-333); --dataset-refine names another file
      raw_refine = a.count("dataset-refine") ? a["dataset-refine"] : (a.count("dataset") ? a["dataset"] : "");
      if (raw_refine.empty()) throw Error(VAQHIP_EINVAL, "--refine needs the raw vectors: --dataset <.fvecs> (or --dataset-refine)");
      if (!resident) datasetrefine = readOri(raw_refine, N, dsize_raw, 0);  // (a resident path reads it where it uploads)
    }
    if (resident && uploaded) vaq.refineExactTies = a.count("exact-ties") && std::atoi(a["exact-ties"].c_str()) != 0;
    if (resident && !uploaded) {
      if (N != D) throw Error(VAQHIP_EINVAL, "--refine-resident searches and refines with the same raw query: --timeseries-size must be D");
      vaq.refineExactTies = a.count("exact-ties") && std::atoi(a["exact-ties"].c_str()) != 0;
      auto t0 = std::chrono::steady_clock::now();
      resident_rows = uploadRefine(raw_refine, dsize_raw);
      std::cout << "== Refine dataset read + upload: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
                << " s (" << resident_rows << " rows resident" << (g_bvecs ? ", as bytes" : "") << ")" << std::endl;
      if (vaq.multiRefinerHandle()) {
        vaqhip_multi_refiner_info inf;
        if (vaqhip_multi_refiner_get_info(vaq.multiRefinerHandle(), &inf) == 0)
          for (int g = 0; g < inf.n_devices; g++)
            std::cout << "   shard " << g << " (device " << inf.device_ids[g] << "): " << inf.shard_rows[g]
                      << " rows resident" << std::endl;
      }
    }
    RowMatrix<int> gt;
    if (a.count("groundtruth")) {
      gt = readIVecs(a["groundtruth"], k);
    } else if (a.count("exact-groundtruth")) {
      if (N != D) throw Error(VAQHIP_EINVAL, "--exact-groundtruth compares raw vectors: --timeseries-size must be D");
      if (!resident) {  // (with --refine-resident the rows are there already)
        const std::string raw = a.count("dataset-refine") ? a["dataset-refine"] : (a.count("dataset") ? a["dataset"] : "");
        if (raw.empty()) throw Error(VAQHIP_EINVAL, "--exact-groundtruth needs the raw vectors: --dataset <.fvecs>");
        resident_rows = uploadRefine(raw, dsize_raw);  // (float rows a --refine read are there already)
      }
      auto t0 = std::chrono::steady_clock::now();
      const LabelDistVecF exact = vaq.searchExhaustive(queries, k);
      gt = RowMatrix<int>((size_t)queries.rows(), (size_t)k);
      for (size_t i = 0; i < gt.rows(); i++)
        for (size_t j = 0; j < gt.cols(); j++) gt(i, j) = exact.labels[i * k + j];
      std::cout << "== Exact ground truth: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
                << " s (" << resident_rows << " rows x " << queries.rows() << " queries, exhaustive)" << std::endl;
      a["groundtruth"] = "(exact)";
    }
    if (vaq.searchMethod() & VaqHip::NNMethod::Fast) {  // demo_vaq.cpp:120-124
      if (!a.count("dataset")) throw Error(VAQHIP_EINVAL, "a FAST method learns its quantisation from --dataset <.fvecs>");
      const int lsize = a.count("dataset-size") ? std::atoi(a["dataset-size"].c_str()) : -1;
      const float ratio = (float)std::atof(a.count("learn-ratio") ? a["learn-ratio"].c_str() : "0.05");
      // the same mOffsets / mScale three ways: from the rows --refine-resident left on the device(s) when they are
      // --dataset's, from the bytes of a bvecs file, or from the host float matrix as the reference does
      const bool same_rows = !a.count("dataset-refine") || a["dataset-refine"] == a["dataset"];
      const char *from = "";
      auto t0 = std::chrono::steady_clock::now();
      if (a.count("refine-resident") && same_rows && N == D && (vaq.refinerHandle() || vaq.multiRefinerHandle())) {
        vaq.learnQuantizationRefineDataset(ratio);
        from = " (from the resident rows)";
      } else if (g_bvecs && N == D) {
        RowMatrix<uint8_t> dataset8 = readBVecsU8(a["dataset"], N, lsize);
        t0 = std::chrono::steady_clock::now();
        vaq.learnQuantization(dataset8, ratio);
        from = " (from the byte rows of the bvecs file)";
      } else {
        RowMatrixF dataset = readOri(a["dataset"], N, lsize, D - N);
        t0 = std::chrono::steady_clock::now();
        vaq.learnQuantization(dataset, ratio);
      }
      std::cout << "== Learn Quantization time: "
                << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s" << from << std::endl;
    }
    vaq.sync();
    for (const int refine : refines) {
      auto t0 = std::chrono::steady_clock::now();
      const int searchK = refine >= k ? refine : k;  // demo_vaq.cpp:338
      LabelDistVecF answers;
      if (resident && refine >= k) {
        std::cout << "Refining the answer with Refine = " << refine << " (resident rows, fused with the search)" << std::endl;
        answers = vaq.search(queries, k, refine);
      } else {
        answers = vaq.search(queries, searchK, true);
      }
      if (refine >= k && !resident) {
        std::cout << "Refining the answer with Refine = " << refine << std::endl;
        // the raw queries (first N dims), as the reference passes them (demo_vaq.cpp:342)
        RowMatrixF qraw((size_t)queries.rows(), (size_t)N);
        for (size_t i = 0; i < qraw.rows(); i++)
          for (size_t j = 0; j < qraw.cols(); j++) qraw(i, j) = queries(i, j);
        answers = vaq.refine(qraw, answers, datasetrefine, k);
      }
      double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      std::cout << "== Querying time: " << sec << " s (" << queries.rows() / sec
                << " queries/s, host buffers in and out)" << std::endl;
      if (a.count("result")) {
        std::string fp = a["result"];
        if (refines.size() > 1) fp += "_R" + std::to_string(refine);  // demo_vaq.cpp:349-351
        writeKNNResults(fp, answers, queries.rows());
      }
      if (a.count("groundtruth"))
        std::cout << "\tprecision(avg_recall): " << getAvgRecall(answers.labels, gt, k)
                  << "\n\trecall@R: " << getRecallAtR(answers.labels, gt, k) << std::endl;
    }
  } catch (const std::exception &e) {
    std::cerr << "error: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
