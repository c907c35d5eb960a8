// vaq_codebooks.h -- the subspace codebooks (vaq_codebooks.hip): staticFitSampling per subspace, all subspaces per
// launch; the hierarchical and the binary-tree form for subspaces above 8 bits; the shard steps of the sharded fit.
#ifndef VAQ_CODEBOOKS_H_
#define VAQ_CODEBOOKS_H_

#include <chrono>

#include "vaq_common.h"

namespace vaq {

namespace cbfit {
struct Plan;  // fit_codebooks_plan.h
}
// host time per phase over all iterations, each phase ended by a stream synchronisation
struct CodebookPhases {
  double gather_ms = 0, assign_ms = 0, accumulate_ms = 0, update_ms = 0;
};
// d_X: n x D device rows of either type (any byte address for byte rows), the device current (plan.gather cleared:
// the plan.gathered rows of the sample, in its order).  The source is chosen per subspace, as every call of the
// reference samples for itself: a subspace with plan.sub[s].full reads all n rows in their own order, widened and
// projected whole by launch_project's chain (d_eig null and float rows: read in place); the others read the first
// plan.sub[s].rows rows of permutation_head(n, plan.gathered), gathered once (from the projected matrix where there
// is one, else gathered first and projected then).  Subspace s = columns [s * L, (s + 1) * L) of its rows, seeded
// from permutation_head(rows, k), then Lloyd iterations until its centres stop changing or max_iter.  d_means: the M
// matrices back to back (plan.n_cent x L floats, device).
// iters_out[M] (host): the reference's iter_count per subspace.  *no_centre_out != 0: some row had no centre at a
// distance below FLT_MAX (the reference indexes row -1 there); the centres are then not to be used.  phases
// (optional) adds one synchronisation per phase.  Synchronises the stream; plan.n_pairs must be below 2^31 (it is
// for every M and bits the library accepts).
hipError_t codebooks_fit(RowsRef d_X, int64_t n, int D, int L, const cbfit::Plan &plan, const float *d_eig,
                         int max_iter, float *d_means, int *iters_out, int *no_centre_out, CodebookPhases *phases,
                         hipStream_t st);
// codebooks_fit from its two sources on (it ends in this): Ps the sample (plan.gathered x D), Pf the full matrix
// (n x D), floats on the current device and complete on `st`, either null when no subspace reads it; no eigvec, no
// gather.  The owners of the sharded fit call it over their compact matrices with D = D_w and their sub-plan.
// began: when the caller started preparing the sources (phases->gather_ms counts from it).
hipError_t codebooks_lloyd(const float *Ps, const float *Pf, int D, int L, const cbfit::Plan &plan, int max_iter,
                           float *d_means, int *iters_out, int *no_centre_out, CodebookPhases *phases,
                           std::chrono::steady_clock::time_point began, hipStream_t st);
// ---- the hierarchical form (fit_codebooks_hier_plan.h): subspaces above 8 bits in two stages ----
namespace cbhier {
struct Plan;
struct Refusal;
}
struct CodebookHierStats {
  double stage1_ms = 0, regroup_ms = 0, stage2_ms = 0;  // host time, each ended by a stream synchronisation
  int groups = 0, min_group = 0, max_group = 0;          // 128 per hierarchical subspace; rows of the smallest and largest
  int stage1_iters = 0, stage2_iters = 0;                // the largest iteration count of a fit of the stage
};
// d_X, d_eig, max_iter, iters_out[M], phases, st: as codebooks_fit.  The flat subspaces and the 128-centre fits of the
// hierarchical ones run as one batch; then the membership of all rows of R_s by squaredNorm (no sqrt), the stable
// regroup, and the K2-centre fits of all groups as one batch.  d_means: plan.n_cent final centres followed by 128
// stage-1 centres per hierarchical subspace (device).  A refusal known only on the device is reported in *refusal
// (kind != OK) or *no_centre_out, with hipSuccess: the centres are then not to be used.  The plan must hold a
// hierarchical subspace.  Synchronises the stream.
hipError_t codebooks_fit_hier(RowsRef d_X, int64_t n, int D, int L, const cbhier::Plan &plan, const float *d_eig,
                              int max_iter, float *d_means, int *iters_out, int *no_centre_out, cbhier::Refusal *refusal,
                              CodebookHierStats *stats, CodebookPhases *phases, hipStream_t st);
// ---- the binary-tree form (fit_codebooks_bin_plan.h): subspaces above 8 bits as a tree of 2-centre fits ----
namespace cbbin {
struct Plan;
}
struct CodebookBinStats {
  double total_ms = 0, fit_ms = 0, split_ms = 0, cut_ms = 0;  // host time, each ended by a stream synchronisation
  int levels = 0, nodes = 0, cut_nodes = 0, leaf_nodes = 0;   // nodes: 2-centre fits run; leaves: nodes at depth bits[s]
  int resampled_fits = 0;                                    // fits (2-centre or cut) that sampled their node's rows
  int min_leaf_rows = 0, max_leaf_rows = 0;                  // 0 where no path reached leaf depth
  int max_iters = 0;
};
// d_X, d_eig, max_iter, iters_out[M], phases, st: as codebooks_fit.  Level by level: the 2-centre fits of all live nodes
// of all binary subspaces as one batch (the first one carries the flat subspaces), the split of their rows by
// squaredNorm (left iff left < right), the counts back to the host, the flat fits of the cut nodes as one more batch,
// the stable regroup into the next level's compact matrix.  staged_sums: the batches' ordered sums by the staged
// kernel (the same bits as cb_accumulate_kernel's).  d_means: plan.n_cent centres (device).  *no_centre_out: as
// codebooks_fit.  The plan must hold a binary subspace.  Synchronises the stream.
hipError_t codebooks_fit_bin(RowsRef d_X, int64_t n, int D, int L, const cbbin::Plan &plan, const float *d_eig, int max_iter,
                             bool staged_sums, float *d_means, int *iters_out, int *no_centre_out, CodebookBinStats *stats,
                             CodebookPhases *phases, hipStream_t st);
// The sharded fit's shard step: out [cnt][D_w] = the compact columns of one owner (d_subs: its subspaces, D_w / L of
// them, device) for the rows a shard contributes -- X's local rows d_rows[0 .. cnt) (device), or first + i where
// d_rows is null.  X: the shard's rows, float or byte, D wide; d_eig null: the rows' own values, else
// launch_project's fmaf chain per value.  cnt == 0 launches nothing.
hipError_t launch_codebook_columns(RowsRef X, int D, const float *d_eig, const int *d_rows, int64_t first, int64_t cnt,
                                   const int *d_subs, int L, int D_w, float *out, hipStream_t st);
// the owner's placement: d_Ps[d_pos[i]][.] = d_stage[i][.] for i < rows, D_w floats per row
hipError_t launch_codebook_place(const float *d_stage, const int *d_pos, int64_t rows, int D_w, float *d_Ps, hipStream_t st);
// an owner that holds all rows gathers the sample of its other subspaces: d_Ps[i][.] = d_Pf[d_rows[i]][.], i < S
hipError_t launch_codebook_gather(const float *d_Pf, int D_w, const int *d_rows, int64_t S, float *d_Ps, hipStream_t st);

} // namespace vaq
#endif
