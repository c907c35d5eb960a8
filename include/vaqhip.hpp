// vaqhip.hpp -- header-only C++ adapter over the C ABI (vaqhip.h) with the
// reference's own names, so driver code written against `class VAQ`
// (bitvecengine/VAQ.hpp:36-113) swaps the type and keeps its calls:
//
//     VaqHip vaq;                                   // was: VAQ vaq;
//     vaq.parseMethodString(args["method"]);        // demo_vaq.cpp:59
//     vaq.mCentroidsPerSubs = ...; vaq.mBitsAlloc = ...; vaq.mCodebook = ...;
//     LabelDistVecF answers = vaq.search(queries, k, true);   // demo_vaq.cpp:339
//
// No Eigen dependency: matrices are passed as any type with data()/rows()/
// cols() in row-major float (Eigen's RowMatrixXf qualifies), or as the plain
// RowMatrixF below.  VaqHip::fromReference() copies the state out of a
// reference VAQ object by duck typing (compiled only where that class exists).
#ifndef VAQHIP_HPP_
#define VAQHIP_HPP_

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "vaqhip.h"

namespace vaqhip {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc) {
  if (rc < 0) throw Error(rc, std::string("vaqhip: ") + vaqhip_last_error());
}

// utils/Types.hpp:98-104
template <typename T = float> struct LabelDistVec {
  std::vector<int> labels;
  std::vector<T> distances;
};
using LabelDistVecF = LabelDistVec<>;

// minimal row-major matrix (stands in for RowMatrixXf / CodebookType)
template <typename T> struct RowMatrix {
  std::vector<T> v;
  size_t r = 0, c = 0;
  RowMatrix() = default;
  RowMatrix(size_t rows_, size_t cols_) : v(rows_ * cols_), r(rows_), c(cols_) {}
  T *data() { return v.data(); }
  const T *data() const { return v.data(); }
  size_t rows() const { return r; }
  size_t cols() const { return c; }
  T &operator()(size_t i, size_t j) { return v[i * c + j]; }
  const T &operator()(size_t i, size_t j) const { return v[i * c + j]; }
};
using RowMatrixF = RowMatrix<float>;
using CodebookType = RowMatrix<uint16_t>;  // utils/Types.hpp:31

class VaqHip {
public:
  struct NNMethod {  // VAQ.hpp:38-49
    enum { Sort = 0x01u, EA = 0x02u, TI = 0x04u, Fast = 0x08u, Fast2 = 0x10u, Fast3 = 0x20u,
           Fast4 = 0x40u, Heap = 0x80u };
  };

  // VAQ.hpp:51-75 (the members search() reads)
  int mBitBudget = 0, mSubspaceNum = 0;
  float mPercentVarExplained = 1.0f;
  int mMinBitsPerSubs = 0, mMaxBitsPerSubs = 0;
  uint32_t mMethods = NNMethod::Heap;
  RowMatrixF mEigenVectors;                  // real part of the reference's complex matrix; empty = identity
  std::vector<RowMatrixF> mCentroidsPerSubs;  // K_s x L each
  std::vector<int> mBitsAlloc;
  CodebookType mCodebook;                     // N x M uint16
  // VAQ.hpp:77-84: triangle-inequality clusters.  mTIClusters is T x (mTISegmentNum * mSubsLen);
  // the reference fills it in clusterTI() with a k-means over decoded codes: clusterTI(true) does the
  // same on the GPU, clusterTI(false) draws random decoded rows, or the caller provides it.
  int mTIClusterNum = 0, mTISegmentNum = -1;
  float mTIVariance = 1.0f;
  float mVisit = 1.0f;
  RowMatrixF mTIClusters;
  int64_t mIdBase = 0;                        // shard offset (not in the reference: single node)
  // option "exact_ties" (vaqhip.h; not in the reference, which IS the order it asks for): labels and distances
  // identical to VAQ::search's slot for slot -- HEAP / EA through the reference's heap, and after clusterTI()
  // the whole walk of VAQ::searchTriangleInequality over the reference's cluster and member orders (single
  // device; with setDevices() a TI search keeps the default tie contract).  Takes effect at the next search().
  // The member is pushed when the index is made and whenever its value has changed since the last push; between
  // such pushes an option set directly on handle() stays as it was set.
  bool exactTies = false;
  int mDevice = 0;
  // Several GPUs of the node (not in the reference, which is one host thread on one CPU): with
  // setDevices({0, 1, ..}) the code rows are sharded contiguously over them and search() ends
  // with the RCCL all-gather + merge of vaqhip_multi_search; results are unchanged.
  std::vector<int> mDevices;
  void setDevices(const std::vector<int> &devices) {
    invalidate();
    if (devices != mDevices) dropRefiners();  // (they live on the devices named before: setRefineDataset() comes after)
    mDevices = devices;
    if (!devices.empty()) mDevice = devices[0];
  }

  VaqHip() = default;
  VaqHip(const VaqHip &) = delete;
  VaqHip &operator=(const VaqHip &) = delete;
  ~VaqHip() {
    dropRefiners();
    vaqhip_index_destroy(h_);
    vaqhip_multi_destroy(mh_);
  }

  int mHighestSubs() const { return (int)mBitsAlloc.size(); }
  int mSubsLen() const { return mCentroidsPerSubs.empty() ? 0 : (int)mCentroidsPerSubs[0].cols(); }
  int mTotalDim() const { return mHighestSubs() * mSubsLen(); }
  uint32_t searchMethod() const { return mMethods; }  // VAQ.hpp:106-108

  // VAQ::parseMethodString, VAQ.cpp:1189-1267.  HEAP, EA and TI<T>[m<seg>] are this
  // path; other search tokens throw (the reference would run a different algorithm).
  // FAST is taken by VaqHipFast below, which has the quantisation members it needs.
  void parseMethodString(const std::string &methodString) {
    std::stringstream ss(methodString);
    std::string token;
    while (std::getline(ss, token, ',')) {
      if (token.rfind("VAQ", 0) == 0) {
        int tb, sv, mn, mx;
        float var;
        if (std::sscanf(token.c_str(), "VAQ%dm%dmin%dmax%dvar%f", &tb, &sv, &mn, &mx, &var) == 5) {
          mBitBudget = tb; mSubspaceNum = sv; mMinBitsPerSubs = mn; mMaxBitsPerSubs = mx;
          mPercentVarExplained = var;
        }
      } else if (token.find("SORT") != std::string::npos || token.find("HEAP") != std::string::npos ||
                 token.find("EA") != std::string::npos || token.find("TI") != std::string::npos ||
                 token.find("FAST") != std::string::npos) {
        uint32_t m = 0;
        std::stringstream sm(token);
        std::string t;
        while (std::getline(sm, t, '_')) {
          if (t.find("SORT") != std::string::npos) m |= NNMethod::Sort;
          else if (t.find("HEAP") != std::string::npos) m |= NNMethod::Heap;
          else if (t.find("EA") != std::string::npos) m |= NNMethod::EA;
          else if (t.find("TI") != std::string::npos) {  // VAQ.cpp:1236-1251
            unsigned long cluster = 0, segment = 0;
            float minvar = 1.0f;
            if (std::sscanf(t.c_str(), "TI%luvar%f", &cluster, &minvar) == 2) {
              m |= NNMethod::TI; mTIClusterNum = (int)cluster; mTIVariance = minvar;
            } else if (std::sscanf(t.c_str(), "TI%lum%lu", &cluster, &segment) == 2) {
              m |= NNMethod::TI; mTIClusterNum = (int)cluster; mTISegmentNum = (int)segment;
            } else if (std::sscanf(t.c_str(), "TI%lu", &cluster) == 1) {
              m |= NNMethod::TI; mTIClusterNum = (int)cluster;
            }
          }
          else if (t.find("FAST3") != std::string::npos) m |= NNMethod::Fast3;
          else if (t.find("FAST2") != std::string::npos) m |= NNMethod::Fast2;
          else if (t.find("FAST") != std::string::npos) m |= NNMethod::Fast;
        }
        if (m & ~methodsAllowed_)
          throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: method '" + token + "' is outside the HEAP/EA/TI path");
        mMethods = m;
      }
    }
  }

  // Push the public members to the GPU (called lazily by search()).
  void sync() {
    const int M = mHighestSubs();
    if (M == 0 || (int)mCentroidsPerSubs.size() != M) throw Error(VAQHIP_EINVAL, "vaqhip: state not set");
    if (!mDevices.empty()) {
      syncMulti();
      return;
    }
    if (!h_) {
      std::vector<const float *> cp(M);
      for (int s = 0; s < M; s++) {
        if ((int)mCentroidsPerSubs[s].rows() != (1 << mBitsAlloc[s]))
          throw Error(VAQHIP_EINVAL, "vaqhip: centroid rows != 1 << bits");
        cp[s] = mCentroidsPerSubs[s].data();
      }
      check(vaqhip_index_create(&h_, mTotalDim(), M, mBitsAlloc.data(), cp.data(),
                                mEigenVectors.rows() ? mEigenVectors.data() : nullptr, mDevice));
      codes_set_ = false;
      ti_set_ = false;
      exact_pushed_ = 0;  // (a new index has the option off)
    }
    if ((mMethods & NNMethod::TI) && !ti_set_) {  // before the codes: they are then grouped once
      const int seg = mTISegmentNum == -1 ? M : mTISegmentNum;  // VAQ.cpp:890-892
      if (mTIClusters.rows() == 0 || (int)mTIClusters.cols() != seg * mSubsLen())
        throw Error(VAQHIP_ESTATE, "vaqhip: method TI needs mTIClusters (T x seg*L); see clusterTI()");
      check(vaqhip_index_set_ti_clusters(h_, mTIClusters.data(), (int)mTIClusters.rows(), seg));
      ti_set_ = true;
    } else if (!(mMethods & NNMethod::TI) && ti_set_) {
      check(vaqhip_index_set_ti_clusters(h_, nullptr, 0, 0));
      ti_set_ = false;
    }
    check(vaqhip_index_set_method(h_, mMethods, mVisit));
    if (exact_pushed_ != (exactTies ? 1 : 0)) {
      check(vaqhip_set_option(h_, "exact_ties", exactTies ? 1 : 0));
      exact_pushed_ = exactTies ? 1 : 0;
    }
    if (!codes_set_) {
      if (mCodebook.cols() != (size_t)M && mCodebook.rows() != 0)
        throw Error(VAQHIP_EINVAL, "vaqhip: mCodebook is not N x M");
      check(vaqhip_index_set_codes_u16(h_, mCodebook.data(), (int64_t)mCodebook.rows(), mIdBase));
      codes_set_ = true;
    }
  }
  // the same for the multi-device index (mDevices set)
  void syncMulti() {
    const int M = mHighestSubs();
    if (!mh_) {
      std::vector<const float *> cp(M);
      for (int s = 0; s < M; s++) {
        if ((int)mCentroidsPerSubs[s].rows() != (1 << mBitsAlloc[s]))
          throw Error(VAQHIP_EINVAL, "vaqhip: centroid rows != 1 << bits");
        cp[s] = mCentroidsPerSubs[s].data();
      }
      checkMulti(vaqhip_multi_create(&mh_, mTotalDim(), M, mBitsAlloc.data(), cp.data(),
                                     mEigenVectors.rows() ? mEigenVectors.data() : nullptr, (int)mDevices.size(),
                                     mDevices.data(), 0u));
      codes_set_ = false;
      ti_set_ = false;
      exact_pushed_ = 0;  // (a new index has the option off)
      fastQuantPushed_ = false;
    }
    if ((mMethods & NNMethod::TI) && !ti_set_) {
      const int seg = mTISegmentNum == -1 ? M : mTISegmentNum;
      if (mTIClusters.rows() == 0 || (int)mTIClusters.cols() != seg * mSubsLen())
        throw Error(VAQHIP_ESTATE, "vaqhip: method TI needs mTIClusters (T x seg*L); see clusterTI()");
      checkMulti(vaqhip_multi_set_ti_clusters(mh_, mTIClusters.data(), (int)mTIClusters.rows(), seg));
      ti_set_ = true;
    } else if (!(mMethods & NNMethod::TI) && ti_set_) {
      checkMulti(vaqhip_multi_set_ti_clusters(mh_, nullptr, 0, 0));
      ti_set_ = false;
    }
    // (FAST alone is only taken once the quantisation is on the shards: VaqHipFast pushes it and sets the method)
    if (!fastOnly() || fastQuantPushed_) checkMulti(vaqhip_multi_set_method(mh_, mMethods, mVisit));
    if (exact_pushed_ != (exactTies ? 1 : 0)) {
      checkMulti(vaqhip_multi_set_option(mh_, "exact_ties", exactTies ? 1 : 0));
      exact_pushed_ = exactTies ? 1 : 0;
    }
    if (!codes_set_) {
      if (mCodebook.cols() != (size_t)M && mCodebook.rows() != 0)
        throw Error(VAQHIP_EINVAL, "vaqhip: mCodebook is not N x M");
      checkMulti(vaqhip_multi_set_codes_u16(mh_, mCodebook.data(), (int64_t)mCodebook.rows(), mIdBase));
      codes_set_ = true;
    }
  }
  // call after changing any public member
  void invalidate() {
    vaqhip_multi_destroy(mh_);
    mh_ = nullptr;
    vaqhip_index_destroy(h_);
    h_ = nullptr;
    codes_set_ = false;
    ti_set_ = false;
  }

  // VAQ::clusterTI, VAQ.hpp:106 / VAQ.cpp:878-999.  useKMeans = false is the reference's
  // other branch (:901-911): mTIClusterNum random code rows, decoded over the first
  // mTISegmentNum subspaces; the grouping itself then happens on the GPU at the next search().
  // useKMeans = true is the reference's k-means over decoded code rows (:897-900,
  // KMeans::staticFitCodebook with max_iter = 50) on the GPU, centre for centre what the reference
  // computes (vaqhip_index_cluster_ti_kmeans); it pushes mCodebook first and groups at once.
  // With setDevices() the same centres come from the shards (vaqhip_multi_cluster_ti_kmeans).
  int mKMeansIterations = 0, mKMeansNanRows = 0;  // how the last k-means ended (not in the reference)
  void clusterTI(bool useKMeans = false, bool verbose = false) {
    (void)verbose;
    if (mTIVariance < 1.0f)
      throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: TI<T>var<v> needs train()'s variance profile; use TI<T>m<seg>");
    if (mTISegmentNum == -1) mTISegmentNum = mHighestSubs();
    if (mTIClusters.rows() == 0 && useKMeans) {
      const uint32_t methods = mMethods;
      mMethods = (methods & ~(uint32_t)NNMethod::TI) ? (methods & ~(uint32_t)NNMethod::TI) : (uint32_t)NNMethod::Heap;
      try { sync(); } catch (...) { mMethods = methods; throw; }  // the codes, in the exhaustive order
      mMethods = methods;
      mTIClusters = RowMatrixF((size_t)(mTIClusterNum > 0 ? mTIClusterNum : 0), (size_t)mTISegmentNum * mSubsLen());
      const int rc = mh_ ? vaqhip_multi_cluster_ti_kmeans(mh_, mTIClusterNum, mTISegmentNum, 50, mTIClusters.data(),
                                                          &mKMeansIterations, &mKMeansNanRows)
                         : vaqhip_index_cluster_ti_kmeans(h_, mTIClusterNum, mTISegmentNum, 50, mTIClusters.data(),
                                                          &mKMeansIterations, &mKMeansNanRows);
      if (rc) mTIClusters = RowMatrixF();
      if (mh_) checkMulti(rc);
      else check(rc);
      mMethods |= NNMethod::TI;
      ti_set_ = true;  // the index holds these centres already
      return;
    }
    if (mTIClusters.rows() == 0) {
      if (mCodebook.rows() == 0) throw Error(VAQHIP_ESTATE, "vaqhip: clusterTI needs mCodebook");
      const int L = mSubsLen();
      mTIClusters = RowMatrixF((size_t)mTIClusterNum, (size_t)mTISegmentNum * L);
      for (int i = 0; i < mTIClusterNum; i++) {
        const size_t r = (size_t)std::rand() % mCodebook.rows();  // VAQ.cpp:903
        for (int s = 0; s < mTISegmentNum; s++)
          for (int j = 0; j < L; j++) mTIClusters(i, (size_t)s * L + j) = mCentroidsPerSubs[s](mCodebook(r, s), j);
      }
    }
    mMethods |= NNMethod::TI;
    ti_set_ = false;
  }

  // VAQ::search, VAQ.hpp:102 / VAQ.cpp:776-847
  template <class Mat> LabelDistVecF search(const Mat &XTest, const int k, bool verbose = false) {
    (void)verbose;
    if (!(mMethods & methodsAllowed_))
      throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: only HEAP / EA / TI are implemented on this path");
    sync();
    LabelDistVecF ret;
    const size_t nq = (size_t)XTest.rows();
    ret.labels.resize(k * nq);
    ret.distances.resize(k * nq);
    if ((int)XTest.cols() != mTotalDim()) throw Error(VAQHIP_EINVAL, "vaqhip: XTest has the wrong width");
    if (mh_)
      checkMulti(vaqhip_multi_search(mh_, XTest.data(), (int)nq, k, 0, ret.labels.data(), ret.distances.data()));
    else
      check(vaqhip_search(h_, XTest.data(), (int)nq, k, ret.labels.data(), ret.distances.data()));
    return ret;
  }

  // VAQ::encode, VAQ.cpp:663-748: fills mCodebook from rows already in PCA
  // space (as the reference expects after train()); projected = false applies
  // mEigenVectors first.
  template <class Mat> void encode(const Mat &XTrain, bool projected = true) {
    encodeRows(XTrain.data(), (int64_t)XTrain.rows(), projected);
  }
  // The same from byte rows (a bvecs dataset as its file holds it, vaqhip_io.hpp readBVecsU8): the codes of the float
  // overload on the widened rows, code for code, from a quarter of the upload (vaqhip_encode_u8,
  // vaqhip_multi_encode_set_codes_u8 after setDevices()).
  void encode(const RowMatrix<uint8_t> &XTrain, bool projected = true) {
    encodeRows(XTrain.data(), (int64_t)XTrain.rows(), projected);
  }

private:
  static int encodeCall(vaqhip_index *h, const float *X, int64_t n, int projected, uint16_t *codes) {
    return vaqhip_encode(h, X, n, projected, codes);
  }
  static int encodeCall(vaqhip_index *h, const uint8_t *X, int64_t n, int projected, uint16_t *codes) {
    return vaqhip_encode_u8(h, X, n, projected, codes);
  }
  static int encodeCall(vaqhip_multi *h, const float *X, int64_t n, int projected, int64_t id_base, uint16_t *codes) {
    return vaqhip_multi_encode_set_codes(h, X, n, projected, id_base, codes);
  }
  static int encodeCall(vaqhip_multi *h, const uint8_t *X, int64_t n, int projected, int64_t id_base, uint16_t *codes) {
    return vaqhip_multi_encode_set_codes_u8(h, X, n, projected, id_base, codes);
  }
  template <class T> void encodeRows(const T *X, int64_t n, bool projected) {
    const bool had = codes_set_;
    codes_set_ = true;  // sync() must not try to upload the (empty) codebook first
    try { sync(); } catch (...) { codes_set_ = had; throw; }
    codes_set_ = false;
    mCodebook = CodebookType((size_t)n, (size_t)mHighestSubs());
    if (mh_) {
      // every shard encodes the rows it will hold and keeps their codes (vaqhip.h, "Encode across the shards");
      // mCodebook is filled all the same (saveCodebook and callers read it), but search() need not upload it again
      checkMulti(encodeCall(mh_, X, n, projected ? 1 : 0, mIdBase, mCodebook.data()));
      codes_set_ = true;
      return;
    }
    check(encodeCall(h_, X, n, projected ? 1 : 0, mCodebook.data()));
  }

public:
  // encode() from the rows setRefineDataset() left on the devices (after setDevices(); the RAW rows, so mEigenVectors
  // are applied): nothing is uploaded, every shard encodes its resident rows in place, and mCodebook is filled as
  // encode(XTrain, false) fills it.  On one device the rows of a refiner are not encoded in place: VAQHIP_EUNSUPPORTED.
  void encodeRefineDataset() {
    if (mDevices.empty()) throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: encodeRefineDataset needs setDevices()");
    if (!mrf_) throw Error(VAQHIP_ESTATE, "vaqhip: encodeRefineDataset needs setRefineDataset() first");
    const bool had = codes_set_;
    codes_set_ = true;  // (as encode(): the codebook is not there yet)
    try { sync(); } catch (...) { codes_set_ = had; throw; }
    codes_set_ = false;
    vaqhip_multi_refiner_info inf;
    checkMulti(vaqhip_multi_refiner_get_info(mrf_, &inf));
    mCodebook = CodebookType((size_t)inf.N, (size_t)mHighestSubs());
    checkMulti(vaqhip_multi_encode_from_refiner(mh_, mrf_, mCodebook.data()));
    codes_set_ = true;
  }

  // The codebook step of VAQ::train (VAQ.cpp:628-660) by the call of :644-649, KMeans::staticFitSampling per subspace
  // (NOT the arma::kmeans call that runs beside it today): fills mCentroidsPerSubs from mBitsAlloc and mEigenVectors
  // (empty: XTrain is in PCA space already), every centre the reference's bit for bit (vaqhip_fit_codebooks on
  // mDevice; after setDevices() vaqhip_multi_fit_codebooks: the rows cut over mDevices, subspace s fitted on device
  // s % G, the same centres bit for bit).  XTrain: raw rows, as wide as the index.  mCodebookIters / mCodebookNanRows: per subspace the
  // reference's iter_count and the centres an empty cluster left NaN.  PCA and bit allocation are the caller's, or train()'s below.
  // mHierarchicalKmeans (demo_vaq --kmeans-ver 1, VAQ.cpp:546-594): every subspace above 8 bits is fitted as 128 centres
  // and 1 << (bits - 7) centres inside each of their groups (vaqhip_fit_codebooks_hier; include/vaqhip.h has the
  // contract).  fitCodebooks, fitCodebooksRefineDataset and train honour it; after setDevices() it is
  // VAQHIP_EUNSUPPORTED: the hierarchical fit has no multi-device form.
  // mBinaryKmeans (demo_vaq --kmeans-ver 2, hierarchicalBinKmeans, VAQ.cpp:1293-1371): every subspace above 8 bits is
  // fitted as a binary tree of 2-centre fits (vaqhip_fit_codebooks_bin); honoured by the same calls, refused after
  // setDevices() in the same way.  As in the reference's if / else if, mHierarchicalKmeans wins when both are set.
  bool mHierarchicalKmeans = false;
  bool mBinaryKmeans = false;
  std::vector<int> mCodebookIters, mCodebookNanRows;
  void fitCodebooks(const RowMatrixF &XTrain, int maxIter = 25) { fitCodebooksRows(XTrain.data(), (int64_t)XTrain.rows(), (int)XTrain.cols(), maxIter); }
  // from byte rows (readBVecsU8): the float overload's centres on the widened rows, bit for bit
  void fitCodebooks(const RowMatrix<uint8_t> &XTrain, int maxIter = 25) { fitCodebooksRows(XTrain.data(), (int64_t)XTrain.rows(), (int)XTrain.cols(), maxIter); }
  // from the rows setRefineDataset() left on the device, float or byte, read in place; after setDevices() over the
  // multi refiner's shards (vaqhip_multi_refiner_fit_codebooks)
  void fitCodebooksRefineDataset(int maxIter = 25) {
    if (!(mDevices.empty() ? (bool)rf_ : (bool)mrf_))
      throw Error(VAQHIP_ESTATE, "vaqhip: fitCodebooksRefineDataset needs setRefineDataset() first");
    refuseHierarchicalMulti();
    if (mrf_) {
      fitCodebooksWith(rf_dim_, [&](const float *eig, float *cent) {
        return vaqhip_multi_refiner_fit_codebooks(mrf_, mHighestSubs(), mBitsAlloc.data(), eig, maxIter, cent,
                                                  mCodebookIters.data(), mCodebookNanRows.data());
      }, true);
      return;
    }
    fitCodebooksWith(rf_dim_, [&](const float *eig, float *cent) {
      return (mHierarchicalKmeans ? vaqhip_refiner_fit_codebooks_hier : mBinaryKmeans ? vaqhip_refiner_fit_codebooks_bin : vaqhip_refiner_fit_codebooks)(
          rf_, mHighestSubs(), mBitsAlloc.data(), eig, maxIter, cent, mCodebookIters.data(), mCodebookNanRows.data());
    });
  }

  // VAQ::train (VAQ.cpp:11-524, and the codebook step above) from raw rows: driven by mBitBudget, mSubspaceNum,
  // mPercentVarExplained, mMinBitsPerSubs, mMaxBitsPerSubs (parseMethodString sets them), it fills mEigenVectors (the
  // columns in balanced order), mEigenValues (in that order), mBitsAlloc and mCentroidsPerSubs -- vaqhip_train_rotation
  // on mDevice, then fitCodebooks.  What is the reference's and what is not (the solver's bits, glpk's choice among
  // tied optima): include/vaqhip.h.  VAQHIP_EUNSUPPORTED when mPercentVarExplained < 1 leaves fewer than mSubspaceNum
  // subspaces or one without bits (the codebook fit takes at least 1 bit everywhere), and after setDevices(): the
  // training front half has no multi-device form.  mTrainSweeps: the Jacobi sweeps that rotated.
  std::vector<float> mEigenValues;
  int mTrainSweeps = 0;
  void train(const RowMatrixF &XTrain, int maxIter = 25) { trainRows(XTrain.data(), (int64_t)XTrain.rows(), (int)XTrain.cols(), maxIter); }
  // from byte rows (readBVecsU8): the float overload's result on the widened rows, bit for bit
  void train(const RowMatrix<uint8_t> &XTrain, int maxIter = 25) { trainRows(XTrain.data(), (int64_t)XTrain.rows(), (int)XTrain.cols(), maxIter); }
  // from the rows setRefineDataset() left on the device, float or byte, read in place
  void trainRefineDataset(int maxIter = 25) {
    if (!mDevices.empty()) throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: train has no multi-device form");
    if (!rf_) throw Error(VAQHIP_ESTATE, "vaqhip: trainRefineDataset needs setRefineDataset() first");
    trainWith(rf_dim_, [&](float *eig, float *ev, int *bits, int *highest) {
      return vaqhip_refiner_train_rotation(rf_, mSubspaceNum, mBitBudget, mMinBitsPerSubs, mMaxBitsPerSubs,
                                           mPercentVarExplained, eig, ev, bits, highest);
    });
    fitCodebooksRefineDataset(maxIter);
  }

private:
  static int trainCall(int dev, const float *X, int64_t n, int D, int M, int B, int lo, int hi, float pv, float *eig,
                       float *ev, int *bits, int *highest) {
    return vaqhip_train_rotation(dev, X, n, D, M, B, lo, hi, pv, eig, ev, bits, highest);
  }
  static int trainCall(int dev, const uint8_t *X, int64_t n, int D, int M, int B, int lo, int hi, float pv, float *eig,
                       float *ev, int *bits, int *highest) {
    return vaqhip_train_rotation_u8(dev, X, n, D, M, B, lo, hi, pv, eig, ev, bits, highest);
  }
  template <class T> void trainRows(const T *X, int64_t n, int D, int maxIter) {
    if (!mDevices.empty()) throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: train has no multi-device form");
    trainWith(D, [&](float *eig, float *ev, int *bits, int *highest) {
      return trainCall(mDevice, X, n, D, mSubspaceNum, mBitBudget, mMinBitsPerSubs, mMaxBitsPerSubs, mPercentVarExplained,
                       eig, ev, bits, highest);
    });
    fitCodebooksRows(X, n, D, maxIter);
  }
  // the rotation and the bits into the members; the outputs are kept only when the allocation can be fitted
  template <class Call> void trainWith(int D, Call call) {
    const int M = mSubspaceNum;
    if (M < 1 || D < 1) throw Error(VAQHIP_EINVAL, "vaqhip: train needs mSubspaceNum and rows");
    RowMatrixF eig((size_t)D, (size_t)D);
    std::vector<float> ev((size_t)D);
    std::vector<int> bits((size_t)M, 0);
    int highest = 0;
    check(call(eig.data(), ev.data(), bits.data(), &highest));
    bool fits = highest == M;
    for (int s = 0; s < highest; s++) fits = fits && bits[(size_t)s] >= 1;
    if (!fits)
      throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: train: the allocation leaves a subspace without bits (mPercentVarExplained < 1): "
                                       "the codebook fit takes at least 1 bit in every subspace");
    vaqhip_train_timing tt;
    if (vaqhip_last_train_timing(&tt) == VAQHIP_OK) mTrainSweeps = tt.sweeps;
    mEigenVectors = eig;
    mEigenValues = ev;
    mBitsAlloc = bits;
  }
  void refuseHierarchicalMulti() const {
    if (mHierarchicalKmeans && !mDevices.empty())
      throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: mHierarchicalKmeans has no multi-device form");
    if (mBinaryKmeans && !mDevices.empty())
      throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: mBinaryKmeans has no multi-device form");
  }
  int fitCodebooksCall(int dev, const float *X, int64_t n, int D, int M, const int *bits, const float *eig, int it,
                       float *cent, int *iters, int *nan) const {
    return (mHierarchicalKmeans ? vaqhip_fit_codebooks_hier : mBinaryKmeans ? vaqhip_fit_codebooks_bin : vaqhip_fit_codebooks)(dev, X, n, D, M, bits, eig, it, cent, iters, nan);
  }
  int fitCodebooksCall(int dev, const uint8_t *X, int64_t n, int D, int M, const int *bits, const float *eig, int it,
                       float *cent, int *iters, int *nan) const {
    return (mHierarchicalKmeans ? vaqhip_fit_codebooks_hier_u8 : mBinaryKmeans ? vaqhip_fit_codebooks_bin_u8 : vaqhip_fit_codebooks_u8)(dev, X, n, D, M, bits, eig, it, cent, iters, nan);
  }
  static int fitCodebooksCall(const std::vector<int> &devs, const float *X, int64_t n, int D, int M, const int *bits,
                              const float *eig, int it, float *cent, int *iters, int *nan) {
    return vaqhip_multi_fit_codebooks((int)devs.size(), devs.data(), X, n, D, M, bits, eig, it, cent, iters, nan);
  }
  static int fitCodebooksCall(const std::vector<int> &devs, const uint8_t *X, int64_t n, int D, int M, const int *bits,
                              const float *eig, int it, float *cent, int *iters, int *nan) {
    return vaqhip_multi_fit_codebooks_u8((int)devs.size(), devs.data(), X, n, D, M, bits, eig, it, cent, iters, nan);
  }
  template <class T> void fitCodebooksRows(const T *X, int64_t n, int D, int maxIter) {
    refuseHierarchicalMulti();
    if (!mDevices.empty()) {
      fitCodebooksWith(D, [&](const float *eig, float *cent) {
        return fitCodebooksCall(mDevices, X, n, D, mHighestSubs(), mBitsAlloc.data(), eig, maxIter, cent, mCodebookIters.data(),
                                mCodebookNanRows.data());
      }, true);
      return;
    }
    fitCodebooksWith(D, [&](const float *eig, float *cent) {
      return fitCodebooksCall(mDevice, X, n, D, mHighestSubs(), mBitsAlloc.data(), eig, maxIter, cent, mCodebookIters.data(),
                              mCodebookNanRows.data());
    });
  }
  template <class Call> void fitCodebooksWith(int D, Call call, bool multi = false) {
    const int M = mHighestSubs();
    if (M < 1 || D < 1 || D % M != 0) throw Error(VAQHIP_EINVAL, "vaqhip: fitCodebooks needs mBitsAlloc, and rows of M subspaces");
    if (mEigenVectors.rows() && ((int)mEigenVectors.rows() != D || (int)mEigenVectors.cols() != D))
      throw Error(VAQHIP_EINVAL, "vaqhip: mEigenVectors is not D x D");
    const int L = D / M;
    size_t total = 0;
    for (int b : mBitsAlloc) total += (b > 0 && b < 31) ? ((size_t)1 << b) * L : 0;  // (bits out of range: the call refuses them)
    std::vector<float> cent(total ? total : 1);
    mCodebookIters.assign((size_t)M, 0);
    mCodebookNanRows.assign((size_t)M, 0);
    const int rc = call(mEigenVectors.rows() ? mEigenVectors.data() : nullptr, cent.data());
    if (multi) checkMulti(rc);  // (a sharded call's text is vaqhip_multi_last_error's)
    else check(rc);
    invalidate();  // (an index made from other centres)
    mCentroidsPerSubs.clear();
    size_t off = 0;
    for (int s = 0; s < M; s++) {
      RowMatrixF c((size_t)1 << mBitsAlloc[s], (size_t)L);
      std::copy(cent.begin() + off, cent.begin() + off + c.rows() * c.cols(), c.data());
      off += c.rows() * c.cols();
      mCentroidsPerSubs.push_back(std::move(c));
    }
  }

public:
  // VAQ::refine, VAQ.hpp:104 / VAQ.cpp:849-876
  template <class MatQ, class MatT>
  LabelDistVecF refine(const MatQ &XTest, const LabelDistVecF &answersIn, const MatT &XTrain, const int k) {
    const int nq = (int)XTest.rows();
    const int R = nq ? (int)(answersIn.labels.size() / nq) : 0;
    LabelDistVecF ret;
    ret.labels.resize((size_t)k * nq);
    ret.distances.resize((size_t)k * nq);
    check(vaqhip_refine(mDevice, XTest.data(), nq, (int)XTest.cols(), XTrain.data(), (int64_t)XTrain.rows(),
                        answersIn.labels.data(), R, k, ret.labels.data(), ret.distances.data()));
    return ret;
  }

  // The refine loop of demo_vaq.cpp:336-345 without the round trips (vaqhip.h, "Resident refiner"; not in the
  // reference, whose XTrain is in host memory anyway): setRefineDataset uploads the raw rows once -- row i has label
  // mIdBase + i --, search(XTest, k, refineNum) is search(XTest, refineNum) followed by refine(.., k) with the
  // candidates kept on the device, distances in Eigen's summation order.  refineExactTies: the k best are the
  // reference heap's, slot for slot (option "exact_ties" of the refiner).  After setDevices() the rows are cut over
  // the same devices as the code rows (vaqhip.h, "Multi-device refiner") and the answer is the same, slot for slot.
  // XTest is the raw query, as wide as the index.
  bool refineExactTies = false;
  template <class MatT> void setRefineDataset(const MatT &XTrain) {
    if (rf_dim_ != (int)XTrain.cols()) dropRefiners();
    rf_dim_ = (int)XTrain.cols();
    if (!mDevices.empty()) {
      if (!mrf_) checkMulti(vaqhip_multi_refiner_create(&mrf_, rf_dim_, (int)mDevices.size(), mDevices.data()));
      checkMulti(vaqhip_multi_refiner_set_rows(mrf_, XTrain.data(), (int64_t)XTrain.rows(), mIdBase));
      return;
    }
    if (!rf_) check(vaqhip_refiner_create(&rf_, mDevice, rf_dim_));
    check(vaqhip_refiner_set_rows(rf_, XTrain.data(), (int64_t)XTrain.rows(), mIdBase));
  }
  // The same with the rows kept as the BYTES a bvecs file holds (readBVecsU8; vaqhip.h, "byte rows"): a quarter of
  // the device memory, and every answer -- search(XTest, k, refineNum), searchExhaustive, encodeRefineDataset -- as
  // over the widened matrix, bit for bit.
  void setRefineDataset(const RowMatrix<uint8_t> &XTrain) {
    if (rf_dim_ != (int)XTrain.cols()) dropRefiners();
    rf_dim_ = (int)XTrain.cols();
    if (!mDevices.empty()) {
      if (!mrf_) checkMulti(vaqhip_multi_refiner_create(&mrf_, rf_dim_, (int)mDevices.size(), mDevices.data()));
      checkMulti(vaqhip_multi_refiner_set_rows_u8(mrf_, XTrain.data(), (int64_t)XTrain.rows(), mIdBase));
      return;
    }
    if (!rf_) check(vaqhip_refiner_create(&rf_, mDevice, rf_dim_));
    check(vaqhip_refiner_set_rows_u8(rf_, XTrain.data(), (int64_t)XTrain.rows(), mIdBase));
  }
  template <class Mat> LabelDistVecF search(const Mat &XTest, const int k, const int refineNum) {
    if (!(mMethods & methodsAllowed_))
      throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: only HEAP / EA / TI are implemented on this path");
    if (!(mDevices.empty() ? (bool)rf_ : (bool)mrf_))
      throw Error(VAQHIP_ESTATE, "vaqhip: search(XTest, k, refineNum) needs setRefineDataset() first");
    sync();
    if ((int)XTest.cols() != mTotalDim()) throw Error(VAQHIP_EINVAL, "vaqhip: XTest has the wrong width");
    LabelDistVecF ret;
    const size_t nq = (size_t)XTest.rows();
    ret.labels.resize(k * nq);
    ret.distances.resize(k * nq);
    if (mh_) {
      checkMulti(vaqhip_multi_refiner_set_option(mrf_, "exact_ties", refineExactTies ? 1 : 0));
      checkMulti(vaqhip_multi_search_refine(mh_, mrf_, XTest.data(), (int)nq, refineNum, k, ret.labels.data(),
                                            ret.distances.data()));
      return ret;
    }
    check(vaqhip_refiner_set_option(rf_, "exact_ties", refineExactTies ? 1 : 0));
    check(vaqhip_search_refine(h_, rf_, XTest.data(), (int)nq, refineNum, k, ret.labels.data(), ret.distances.data()));
    return ret;
  }
  // The exhaustive form of refine(): refine(XTest, <every row of the refine dataset in row order>, XTrain, k) without
  // the candidate list -- the true k nearest rows of every query with the reference's own distances, and with
  // refineExactTies its heap's choice among equal ones (vaqhip.h, "Exhaustive form of the resident refiner").  Ground
  // truth for recall when no file exists.  Needs setRefineDataset(); after setDevices() the rows are cut over the
  // devices and the answer is the single device's, slot for slot (vaqhip.h, "Exhaustive form across the shards").
  // XTest is the raw query.
  template <class Mat> LabelDistVecF searchExhaustive(const Mat &XTest, const int k) {
    if (!rf_ && !mrf_) throw Error(VAQHIP_ESTATE, "vaqhip: searchExhaustive needs setRefineDataset() first");
    if ((int)XTest.cols() != rf_dim_) throw Error(VAQHIP_EINVAL, "vaqhip: XTest has the wrong width");
    LabelDistVecF ret;
    const size_t nq = (size_t)XTest.rows();
    ret.labels.resize((size_t)(k > 0 ? k : 0) * nq);
    ret.distances.resize((size_t)(k > 0 ? k : 0) * nq);
    if (mrf_) {
      checkMulti(vaqhip_multi_refiner_set_option(mrf_, "exact_ties", refineExactTies ? 1 : 0));
      checkMulti(vaqhip_multi_refiner_search(mrf_, XTest.data(), (int)nq, k, ret.labels.data(), ret.distances.data()));
      return ret;
    }
    check(vaqhip_refiner_set_option(rf_, "exact_ties", refineExactTies ? 1 : 0));
    check(vaqhip_refiner_search(rf_, XTest.data(), (int)nq, k, ret.labels.data(), ret.distances.data()));
    return ret;
  }
  vaqhip_refiner *refinerHandle() { return rf_; }
  vaqhip_multi_refiner *multiRefinerHandle() { return mrf_; }

  // Copy the search state out of a reference `VAQ` object (duck-typed: the
  // members of VAQ.hpp:51-75, Eigen matrices).  Instantiate only in a
  // translation unit that includes the reference's VAQ.hpp.
  template <class RefVAQ> void fromReference(const RefVAQ &v) {
    invalidate();
    mBitBudget = v.mBitBudget; mSubspaceNum = v.mSubspaceNum;
    mMinBitsPerSubs = v.mMinBitsPerSubs; mMaxBitsPerSubs = v.mMaxBitsPerSubs;
    mMethods = v.mMethods;
    mBitsAlloc.assign(v.mBitsAlloc.begin(), v.mBitsAlloc.begin() + v.mHighestSubs);
    mCentroidsPerSubs.clear();
    for (int s = 0; s < v.mHighestSubs; s++) {
      const auto &c = v.mCentroidsPerSubs[s];  // RowMatrix<float>
      RowMatrixF m(c.rows(), c.cols());
      for (size_t i = 0; i < m.rows(); i++)
        for (size_t j = 0; j < m.cols(); j++) m(i, j) = c(i, j);
      mCentroidsPerSubs.push_back(m);
    }
    const size_t D = v.mEigenVectors.rows();
    mEigenVectors = RowMatrixF(D, v.mEigenVectors.cols());
    for (size_t i = 0; i < D; i++)
      for (size_t j = 0; j < mEigenVectors.cols(); j++) mEigenVectors(i, j) = v.mEigenVectors(i, j).real();
    mCodebook = CodebookType(v.mCodebook.rows(), v.mCodebook.cols());
    // VAQ::clusterTI ends by REGROUPING mCodebook (VAQ.cpp:984-996: row r of the grouped matrix
    // is original row mTIClustersMember[c][r - start_c]) while search() keeps returning ORIGINAL
    // row numbers (VAQ.cpp:1575-1590).  This index regroups its own copy and labels by position
    // in the matrix it is given, so a codebook that was already regrouped is put back into
    // original order first; before clusterTI (no members yet) it is copied as it is.
    size_t members = 0;
    for (const auto &cm : v.mTIClustersMember) members += cm.size();
    if (members == 0) {
      for (size_t i = 0; i < mCodebook.rows(); i++)
        for (size_t j = 0; j < mCodebook.cols(); j++) mCodebook(i, j) = v.mCodebook(i, j);
    } else {
      if (members != mCodebook.rows())
        throw Error(VAQHIP_ESTATE, "vaqhip: mTIClustersMember does not cover mCodebook");
      size_t r = 0;
      for (const auto &cm : v.mTIClustersMember)
        for (const int idx : cm) {
          for (size_t j = 0; j < mCodebook.cols(); j++) mCodebook((size_t)idx, j) = v.mCodebook(r, j);
          r++;
        }
    }
    // the TI state search() reads (VAQ.hpp:77-84)
    mTIClusterNum = v.mTIClusterNum;
    mTISegmentNum = v.mTISegmentNum;
    mVisit = v.mVisit;
    mTIClusters = RowMatrixF((size_t)v.mTIClusters.rows(), (size_t)v.mTIClusters.cols());
    for (size_t i = 0; i < mTIClusters.rows(); i++)
      for (size_t j = 0; j < mTIClusters.cols(); j++) mTIClusters(i, j) = v.mTIClusters(i, j);
    if ((mMethods & NNMethod::TI) && mTIClusters.rows() == 0)
      throw Error(VAQHIP_ESTATE, "vaqhip: the reference object selects TI but has no mTIClusters yet "
                                 "(call its clusterTI() first, or clusterTI() here)");
  }

  vaqhip_index *handle() { return h_; }
  vaqhip_multi *multiHandle() { return mh_; }

protected:
  // NNMethod bits parseMethodString accepts and search() runs
  uint32_t methodsAllowed_ = NNMethod::Heap | NNMethod::EA | NNMethod::TI;
  bool fastOnly() const { return (mMethods & NNMethod::Fast) && !(mMethods & (NNMethod::TI | NNMethod::EA | NNMethod::Heap)); }
  bool fastQuantPushed_ = false;  // the current multi-device index holds a FAST quantisation

private:
  static void checkMulti(int rc) {
    if (rc < 0) throw Error(rc, std::string("vaqhip: ") + vaqhip_multi_last_error());
  }
  vaqhip_index *h_ = nullptr;
  vaqhip_multi *mh_ = nullptr;
  void dropRefiners() {
    vaqhip_refiner_destroy(rf_);
    rf_ = nullptr;
    vaqhip_multi_refiner_destroy(mrf_);
    mrf_ = nullptr;
  }
  vaqhip_refiner *rf_ = nullptr;
  vaqhip_multi_refiner *mrf_ = nullptr;  // after setDevices(): the rows cut over mDevices
  int rf_dim_ = 0;
  bool codes_set_ = false;
  bool ti_set_ = false;
  int exact_pushed_ = 0;  // the value of exactTies the index holds from the last push
};

// ---------------------------------------------------------------------------
// VAQ with the FAST search method (VAQ::searchFast, VAQ.cpp:1778-1834; vaqhip.h,
// vaqhip_index_set_lut_quantization): uint8 tables over codes of at most 4 bits,
// labels and distances as the reference returns them, slot for slot.  The extra
// members are the reference's: mOffsets, mScale (set by learnQuantization, or by
// hand) and mCodebookCMajor (filled by encode).  Method precedence is the
// reference's, TI > EA > HEAP > FAST.  With setDevices the quantisation goes to every shard and the sharded
// search returns the same slots (vaqhip.h, vaqhip_multi_set_lut_quantization).
// ---------------------------------------------------------------------------
class VaqHipFast : public VaqHip {
public:
  std::vector<float> mOffsets, mScale;  // [M] each (VAQ.hpp: RowVector<float>, ColVector<float>)
  // mCodebook as FAST reads it (VAQ.cpp:666-670, 718): uint8, column-major, rows padded to 32 with code 0;
  // entry (row i, subspace s) at mCodebookCMajor[s * mCodebookCMajorRows + i]
  std::vector<uint8_t> mCodebookCMajor;
  size_t mCodebookCMajorRows = 0;

  VaqHipFast() { methodsAllowed_ |= NNMethod::Fast; }

  // VAQ::parseMethodString with FAST, and the reference's check after it (VAQ.cpp:1263-1266)
  void parseMethodString(const std::string &methodString) {
    VaqHip::parseMethodString(methodString);
    if ((mMethods & NNMethod::Fast) && mMaxBitsPerSubs > 4)
      throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: max bit per subs couldn't be > 4 when using FAST query method");
  }

  // VAQ::encode, plus the column-major copy
  template <class Mat> void encode(const Mat &XTrain, bool projected = true) {
    VaqHip::encode(XTrain, projected);
    const size_t N = mCodebook.rows(), M = mCodebook.cols();
    mCodebookCMajorRows = (N + 31) / 32 * 32;
    mCodebookCMajor.assign(mCodebookCMajorRows * M, 0);
    for (size_t i = 0; i < N; i++)
      for (size_t s = 0; s < M; s++) mCodebookCMajor[s * mCodebookCMajorRows + i] = (uint8_t)mCodebook(i, s);
  }

  // VAQ::learnQuantization(XTrain, sampleRatio), VAQ.cpp:1118-1187: XTrain unprojected, as the reference
  // takes it (demo_vaq.cpp:120-124 passes the dataset).  Call it after the codes are set (or encode).
  template <class Mat> void learnQuantization(const Mat &XTrain, float sampleRatio) {
    if ((int)XTrain.cols() != mTotalDim()) throw Error(VAQHIP_EINVAL, "vaqhip: XTrain has the wrong width");
    sync();
    mOffsets.assign((size_t)mHighestSubs(), 0.0f);
    mScale.assign((size_t)mHighestSubs(), 0.0f);
    if (multiHandle())
      checkFast(vaqhip_multi_learn_quantization(multiHandle(), XTrain.data(), (int64_t)XTrain.rows(), 0, sampleRatio,
                                                mOffsets.data(), mScale.data()), true),
          fastQuantPushed_ = true;
    else
      check(vaqhip_learn_quantization(handle(), XTrain.data(), (int64_t)XTrain.rows(), 0, sampleRatio, mOffsets.data(),
                                      mScale.data()));
    pushedFor_ = current();
    pushedOffsets_ = mOffsets;
    pushedScale_ = mScale;
  }
  // ... from byte rows (a bvecs dataset as its file holds it): only the sampled rows are uploaded, as bytes, and
  // mOffsets / mScale are those of the float form over the widened rows, bit for bit (vaqhip_learn_quantization_u8,
  // vaqhip_multi_learn_quantization_u8 after setDevices())
  void learnQuantization(const RowMatrix<uint8_t> &XTrain, float sampleRatio) {
    if ((int)XTrain.cols() != mTotalDim()) throw Error(VAQHIP_EINVAL, "vaqhip: XTrain has the wrong width");
    learnWith([&](float *off, float *sc) {
      return multiHandle() ? vaqhip_multi_learn_quantization_u8(multiHandle(), XTrain.data(), (int64_t)XTrain.rows(), 0,
                                                                sampleRatio, off, sc)
                           : vaqhip_learn_quantization_u8(handle(), XTrain.data(), (int64_t)XTrain.rows(), 0, sampleRatio,
                                                          off, sc);
    });
  }
  // ... from the rows setRefineDataset() left on the device, float or byte, read in place (the resident refiner on
  // one device, the multi refiner after setDevices(): vaqhip_[multi_]learn_quantization_from_refiner)
  void learnQuantizationRefineDataset(float sampleRatio) {
    if (!refinerHandle() && !multiRefinerHandle())
      throw Error(VAQHIP_ESTATE, "vaqhip: learnQuantizationRefineDataset needs setRefineDataset() first");
    learnWith([&](float *off, float *sc) {
      return multiHandle() ? vaqhip_multi_learn_quantization_from_refiner(multiHandle(), multiRefinerHandle(), sampleRatio, off, sc)
                           : vaqhip_learn_quantization_from_refiner(handle(), refinerHandle(), sampleRatio, off, sc);
    });
  }

  // VAQ::search: pushes mOffsets / mScale when they changed, then runs the method in force
  template <class Mat> LabelDistVecF search(const Mat &XTest, const int k, bool verbose = false) {
    pushQuantization();
    return VaqHip::search(XTest, k, verbose);
  }
  // ... and the search fused with the resident refine (VaqHip::search(XTest, k, refineNum))
  template <class Mat> LabelDistVecF search(const Mat &XTest, const int k, const int refineNum) {
    pushQuantization();
    return VaqHip::search(XTest, k, refineNum);
  }

private:
  // one of the device forms: call(offsets, scale) -> code; mOffsets / mScale change on success only
  template <class Call> void learnWith(Call &&call) {
    sync();
    std::vector<float> off((size_t)mHighestSubs(), 0.0f), sc((size_t)mHighestSubs(), 0.0f);
    const bool multi = multiHandle() != nullptr;
    checkFast(call(off.data(), sc.data()), multi);
    if (multi) fastQuantPushed_ = true;
    mOffsets = off;
    mScale = sc;
    pushedFor_ = current();
    pushedOffsets_ = mOffsets;
    pushedScale_ = mScale;
  }
  void pushQuantization() {
    sync();
    if (mOffsets.size() == (size_t)mHighestSubs() && mScale.size() == mOffsets.size() &&
        (pushedFor_ != current() || pushedOffsets_ != mOffsets || pushedScale_ != mScale ||
         (multiHandle() && !fastQuantPushed_))) {
      if (multiHandle())
        checkFast(vaqhip_multi_set_lut_quantization(multiHandle(), mOffsets.data(), mScale.data()), true),
            fastQuantPushed_ = true;
      else
        check(vaqhip_index_set_lut_quantization(handle(), mOffsets.data(), mScale.data()));
      pushedFor_ = current();
      pushedOffsets_ = mOffsets;
      pushedScale_ = mScale;
    }
    if (multiHandle() && fastOnly() && !fastQuantPushed_)
      throw Error(VAQHIP_ESTATE, "vaqhip: method FAST needs mOffsets / mScale (learnQuantization) first");
  }
  // the index the quantisation was last pushed to: the multi-device one when setDevices is in force
  const void *current() { return multiHandle() ? (const void *)multiHandle() : (const void *)handle(); }
  static void checkFast(int rc, bool multi) {
    if (rc < 0) throw Error(rc, std::string("vaqhip: ") + (multi ? vaqhip_multi_last_error() : vaqhip_last_error()));
  }
  const void *pushedFor_ = nullptr;
  std::vector<float> pushedOffsets_, pushedScale_;
};

// ---------------------------------------------------------------------------
// BitVecEngine::queryLUT (BitVecEngine.hpp:1222-1343), the reference's other
// entry on this path: one scalar quantiser per PCA dimension, columns summed
// one by one.  The engine keeps its state private (centroidsMat, solutionX,
// eigenVectors, nonZeroAllocCount: BitVecEngine.hpp:33-39); here it is public.
// ---------------------------------------------------------------------------
struct IdxDistPairFloat {  // utils/Types.hpp:41-57
  int idx;
  float dist;
};
struct IdxDistPair {  // utils/Types.hpp:51 (IdxDistPairBase<uint32_t>)
  int idx;
  uint32_t dist;
};
using bitv = std::vector<uint64_t>;  // BitVector.hpp: actBitVLen words a vector
using bitvectors = std::vector<bitv>;

class BitVecEngineHip {
public:
  std::vector<float> centroidsMat;  // column-major, `centroidRows` (256) rows x nonZeroAllocCount columns
  int centroidRows = 256;
  std::vector<int> solutionX;       // bits per dimension
  RowMatrixF eigenVectors;          // real part, D x D, D = nonZeroAllocCount (empty = identity)
  int mDevice = 0;
  // option "exact_ties" (vaqhip.h): queryLUT's own order among equal distances, from its std heap
  bool exactTies = false;

  BitVecEngineHip() = default;
  BitVecEngineHip(const BitVecEngineHip &) = delete;
  BitVecEngineHip &operator=(const BitVecEngineHip &) = delete;
  ~BitVecEngineHip() {
    invalidate();
    vaqhip_bitvec_destroy(bv_);
    vaqhip_refiner_destroy(ori_);
  }
  void invalidate() {
    vaqhip_index_destroy(h_);
    h_ = nullptr;
    vaqhip_multi_destroy(mh_);
    mh_ = nullptr;
  }

  // ---- the Hamming queries (vaqhip_bitvec_* of vaqhip.h), on mDevice ----
  struct QueryMethod {  // BitVecEngine.hpp:82-84
    enum { Heap, Sort, HeapEarlyAbandon, SortEarlyAbandon };
  };
  // BitVecEngine::loadBitV: the bit vectors, all of one length (at most 16 words), copied to the device
  void loadBitV(const bitvectors &bitVectors) {
    const size_t W = bitVectors.empty() ? 1 : bitVectors[0].size();
    std::vector<uint64_t> flat;
    flat.reserve(bitVectors.size() * W);
    for (const bitv &v : bitVectors) {
      if (v.size() != W) throw Error(VAQHIP_EINVAL, "vaqhip: loadBitV: bit vectors of different lengths");
      flat.insert(flat.end(), v.begin(), v.end());
    }
    vaqhip_bitvec_destroy(bv_);
    bv_ = nullptr;
    bitWords_ = (int)W;
    check(vaqhip_bitvec_create(&bv_, mDevice, (int)(64 * W)));
    check(vaqhip_bitvec_set_rows(bv_, flat.data(), (int64_t)bitVectors.size(), 0));
  }
  // BitVecEngine::loadOriginal: the raw rows queryRerank measures, kept on the device as floats or as bytes
  void loadOriginal(const RowMatrix<float> &oriDataset) {
    newOriginal((int)oriDataset.cols());
    check(vaqhip_refiner_set_rows(ori_, oriDataset.data(), (int64_t)oriDataset.rows(), 0));
  }
  void loadOriginal(const RowMatrix<uint8_t> &oriDataset) {
    newOriginal((int)oriDataset.cols());
    check(vaqhip_refiner_set_rows_u8(ori_, oriDataset.data(), (int64_t)oriDataset.rows(), 0));
  }
  // BitVecEngine::query: min(k, rows) pairs per query.  Only QueryMethod::Sort is provided: the other three keep
  // other rows among equal distances (vaqhip.h), and throw as parseMethodString does for a token it does not serve
  std::vector<std::vector<IdxDistPair>> query(const bitvectors &queries, const int k, int method = QueryMethod::Sort) {
    if (!bv_) throw Error(VAQHIP_ESTATE, "vaqhip: query before loadBitV");
    const std::vector<uint64_t> q = flatQueries(queries);
    const int nq = (int)queries.size();
    std::vector<int> lab((size_t)nq * k);
    std::vector<float> dis((size_t)nq * k);
    check(vaqhip_bitvec_query(bv_, q.data(), nq, k, method, lab.data(), dis.data()));
    std::vector<std::vector<IdxDistPair>> answers(nq);
    for (int i = 0; i < nq; i++)
      for (int j = 0; j < k && lab[(size_t)i * k + j] >= 0; j++)
        answers[i].push_back({lab[(size_t)i * k + j], (uint32_t)dis[(size_t)i * k + j]});
    return answers;
  }
  // BitVecEngine::queryRerank with earlyAbandonRank = false: squared Euclidean distances, as the reference's
  template <class Mat>
  std::vector<std::vector<IdxDistPairFloat>> queryRerank(const bitvectors &queries, const Mat &oriQueries, const int k,
                                                         const int factor = 2, int method = QueryMethod::Sort) {
    if (!bv_ || !ori_) throw Error(VAQHIP_ESTATE, "vaqhip: queryRerank before loadBitV and loadOriginal");
    if (method != QueryMethod::Sort)
      throw Error(VAQHIP_EUNSUPPORTED, "vaqhip: queryRerank: only QueryMethod::Sort is provided");
    const std::vector<uint64_t> q = flatQueries(queries);
    const int nq = (int)queries.size();
    if ((int)oriQueries.rows() != nq || (int)oriQueries.cols() != oriDim_)
      throw Error(VAQHIP_EINVAL, "vaqhip: queryRerank: oriQueries must have one row of the original dimension per query");
    std::vector<int> lab((size_t)nq * k);
    std::vector<float> dis((size_t)nq * k);
    check(vaqhip_bitvec_query_rerank(bv_, ori_, q.data(), oriQueries.data(), nq, k, factor, lab.data(), dis.data()));
    std::vector<std::vector<IdxDistPairFloat>> answers(nq);
    for (int i = 0; i < nq; i++)
      for (int j = 0; j < k && lab[(size_t)i * k + j] >= 0; j++)
        answers[i].push_back({lab[(size_t)i * k + j], dis[(size_t)i * k + j]});
    return answers;
  }
  vaqhip_bitvec *bitvecHandle() const { return bv_; }
  // Several devices (a device named several times: logical shards on that GPU): binaryEncodingLUT then fits over
  // them (vaqhip_multi_lut_fit_quantiles), builds a VAQHIP_SUM_SEQUENTIAL multi index, gives it Q and encodes across
  // the shards (vaqhip_multi_encode_lut_set_codes), and queryLUT answers from that multi index -- the same members
  // and answers as on one device.  An empty list: back to mDevice.
  void setDevices(const std::vector<int> &devices) {
    invalidate();
    mDevices = devices;
  }
  vaqhip_multi *multiHandle() const { return mh_; }

  // queries: any row-major float matrix with data()/rows()/cols() (the reference
  // takes a column-major Eigen::MatrixXf: pass its transpose's storage or a RowMatrixF)
  template <class Mat, class Codebook>
  std::vector<std::vector<IdxDistPairFloat>> queryLUT(const Mat &queries, const int k, const Codebook &codebook) {
    ensureIndex();
    const int nq = (int)queries.rows();
    std::vector<int> lab((size_t)nq * k);
    std::vector<float> dis((size_t)nq * k);
    if (mh_) {
      checkMulti(vaqhip_multi_set_option(mh_, "exact_ties", exactTies ? 1 : 0));
      // (as on one device: the codebook handed in is the one searched, whatever binaryEncodingLUT left on the shards)
      checkMulti(vaqhip_multi_set_codes_u16(mh_, codebook.data(), (int64_t)codebook.rows(), 0));
      checkMulti(vaqhip_multi_search(mh_, queries.data(), nq, k, 0, lab.data(), dis.data()));
    } else {
      check(vaqhip_set_option(h_, "exact_ties", exactTies ? 1 : 0));
      check(vaqhip_index_set_codes_u16(h_, codebook.data(), (int64_t)codebook.rows(), 0));
      check(vaqhip_search(h_, queries.data(), nq, k, lab.data(), dis.data()));
    }
    std::vector<std::vector<IdxDistPairFloat>> answers(nq);  // min(k, rows) pairs each, as the reference's
    for (int q = 0; q < nq; q++)
      for (int i = 0; i < k && lab[(size_t)q * k + i] >= 0; i++)
        answers[q].push_back({lab[(size_t)q * k + i], dis[(size_t)q * k + i]});
    return answers;
  }

  // BitVecEngine::binaryEncodingLUT (BitVecEngine.hpp:594-935) from the bit allocation on, on the GPU.  The PCA
  // (:596-617) and the glpk bit allocation (:622-809) stay the caller's: with solutionX (1..8 bits per dimension, as
  // hardcodedSolutionX gives them) and eigenVectors set, this fills centroidsMat (256 x nonZeroAllocCount) and
  // `quantiles` as centroidsQuantile does (:811-867), then codebookOut as encodeToLUTCode does (:889-934), bit for
  // bit (vaqhip_lut_fit_quantiles, vaqhip_encode_lut).  XTrain: row-major, unprojected -- projected here without
  // checking, as :620 does.  A NaN or infinite projected value is refused (VAQHIP_EINVAL).
  std::vector<float> quantiles;  // nonZeroAllocCount x 257: row d = Q[d][0 .. 1 << solutionX[d]], the rest 0
  template <class Mat>
  void binaryEncodingLUT(const Mat &XTrain, CodebookType &codebookOut) {
    buildFromRows(XTrain.data(), (int64_t)XTrain.rows(), (int)XTrain.cols(), codebookOut);
  }
  // The same from byte rows (a bvecs dataset as its file holds it): the members and codebookOut of the float overload
  // on the widened rows, bit for bit (the *_u8 forms of the same calls).
  void binaryEncodingLUT(const RowMatrix<uint8_t> &XTrain, CodebookType &codebookOut) {
    buildFromRows(XTrain.data(), (int64_t)XTrain.rows(), (int)XTrain.cols(), codebookOut);
  }

private:
  // the float calls and their byte twins under one name each
  static int fitCall(int dev, const float *X, int64_t n, int D, const int *bits, const float *eig, float *c, float *q) {
    return vaqhip_lut_fit_quantiles(dev, X, n, D, bits, eig, c, q);
  }
  static int fitCall(int dev, const uint8_t *X, int64_t n, int D, const int *bits, const float *eig, float *c, float *q) {
    return vaqhip_lut_fit_quantiles_u8(dev, X, n, D, bits, eig, c, q);
  }
  static int fitCall(const std::vector<int> &devs, const float *X, int64_t n, int D, const int *bits, const float *eig,
                     float *c, float *q) {
    return vaqhip_multi_lut_fit_quantiles((int)devs.size(), devs.data(), X, n, D, bits, eig, c, q);
  }
  static int fitCall(const std::vector<int> &devs, const uint8_t *X, int64_t n, int D, const int *bits, const float *eig,
                     float *c, float *q) {
    return vaqhip_multi_lut_fit_quantiles_u8((int)devs.size(), devs.data(), X, n, D, bits, eig, c, q);
  }
  static int encodeCall(vaqhip_index *h, const float *X, int64_t n, uint16_t *codes) { return vaqhip_encode_lut(h, X, n, 0, codes); }
  static int encodeCall(vaqhip_index *h, const uint8_t *X, int64_t n, uint16_t *codes) { return vaqhip_encode_lut_u8(h, X, n, 0, codes); }
  static int encodeCall(vaqhip_multi *h, const float *X, int64_t n, uint16_t *codes) {
    return vaqhip_multi_encode_lut_set_codes(h, X, n, 0, 0, codes);
  }
  static int encodeCall(vaqhip_multi *h, const uint8_t *X, int64_t n, uint16_t *codes) {
    return vaqhip_multi_encode_lut_set_codes_u8(h, X, n, 0, 0, codes);
  }
  template <class T> void buildFromRows(const T *X, int64_t n, int cols, CodebookType &codebookOut) {
    const int nd = (int)solutionX.size();
    if (cols != nd) throw Error(VAQHIP_EINVAL, "vaqhip: XTrain must have one column per entry of solutionX");
    centroidRows = 256;
    std::vector<float> cent((size_t)centroidRows * nd), q((size_t)257 * nd);
    const float *eig = eigenVectors.rows() ? eigenVectors.data() : nullptr;
    if (mDevices.empty()) check(fitCall(mDevice, X, n, nd, solutionX.data(), eig, cent.data(), q.data()));
    else checkMulti(fitCall(mDevices, X, n, nd, solutionX.data(), eig, cent.data(), q.data()));
    centroidsMat.swap(cent);
    quantiles.swap(q);
    invalidate();
    ensureIndex();
    codebookOut = CodebookType((size_t)n, (size_t)nd);
    if (mh_) {
      checkMulti(vaqhip_multi_set_lut_quantiles(mh_, quantiles.data()));
      checkMulti(encodeCall(mh_, X, n, codebookOut.data()));
      return;
    }
    check(vaqhip_index_set_lut_quantiles(h_, quantiles.data()));
    check(encodeCall(h_, X, n, codebookOut.data()));
  }

  static void checkMulti(int rc) {
    if (rc < 0) throw Error(rc, std::string("vaqhip: ") + vaqhip_multi_last_error());
  }
  void ensureIndex() {
    if (h_ || mh_) return;
    const int nd = (int)solutionX.size();
    std::vector<std::vector<float>> cols(nd);
    std::vector<const float *> cp(nd);
    for (int d = 0; d < nd; d++) {
      cols[d].assign(centroidsMat.begin() + (size_t)d * centroidRows,
                     centroidsMat.begin() + (size_t)d * centroidRows + ((size_t)1 << solutionX[d]));
      cp[d] = cols[d].data();
    }
    const float *eig = eigenVectors.rows() ? eigenVectors.data() : nullptr;
    if (!mDevices.empty()) {
      checkMulti(vaqhip_multi_create(&mh_, nd, nd, solutionX.data(), cp.data(), eig, (int)mDevices.size(), mDevices.data(),
                                     VAQHIP_SUM_SEQUENTIAL));
      return;
    }
    check(vaqhip_index_create_ex(&h_, nd, nd, solutionX.data(), cp.data(), eig, mDevice, VAQHIP_SUM_SEQUENTIAL));
  }
  std::vector<uint64_t> flatQueries(const bitvectors &queries) const {
    std::vector<uint64_t> flat;
    flat.reserve(queries.size() * (size_t)bitWords_);
    for (const bitv &v : queries) {
      if ((int)v.size() != bitWords_) throw Error(VAQHIP_EINVAL, "vaqhip: a query's length differs from the bit vectors'");
      flat.insert(flat.end(), v.begin(), v.end());
    }
    return flat;
  }
  void newOriginal(int D) {
    vaqhip_refiner_destroy(ori_);
    ori_ = nullptr;
    oriDim_ = D;
    check(vaqhip_refiner_create(&ori_, mDevice, D));
  }
  vaqhip_index *h_ = nullptr;
  vaqhip_multi *mh_ = nullptr;
  std::vector<int> mDevices;
  vaqhip_bitvec *bv_ = nullptr;   // loadBitV
  vaqhip_refiner *ori_ = nullptr;  // loadOriginal
  int bitWords_ = 0, oriDim_ = 0;
};

} // namespace vaqhip
#endif
