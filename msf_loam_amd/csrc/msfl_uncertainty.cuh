// msfl_uncertainty.cuh — per-registration information matrix, its eigen-decomposition and covariance
// (msfl_match_uncertainty, include/msfl_c_api.h; docs/kernels/uncertainty.md).
//
// One kernel, launched after the LAST solve of a registration call, one workgroup per registration with the block
// width of that call's lm_solve_kernel.  It does not touch the solve: it re-evaluates the solved problem once.
//
//   evaluation   one evaluate_pass<BLOCK, true> + block_reduce at the returned pose over the records the last
//                association pass left in the record buffer: {cost, g, H} exactly as the solve's first pass of an outer
//                iteration forms them (same device functions, same summation order), so H is the robustified J^T J
//                that Ceres' Covariance would be handed at that pose.
//   gating       status[b] != 0 (nothing was solved, or the scan-to-scan gate refused the LAST solve) or fewer
//                correspondences than the solve requires: the record is all zero, valid = 0.
//   eigen        cyclic Jacobi on the 6 x 6 in f64 ON LANE 0, matrix and vectors in registers (every index is a
//                compile-time constant after unrolling).  Chosen over the three disjoint rotations of a round-robin
//                sweep on three lanes: those exchange rows through LDS behind a barrier per round (5 rounds x ~7
//                sweeps), and the serial chain of one rotation (two divisions, two square roots) is the same
//                either way, so the parallel form saves the ~50 independent multiply-adds of a rotation and pays a
//                barrier for them.  The whole section is a few thousand f64 instructions on one lane: it is
//                latency, not throughput, and 1 024 workgroups hide it behind each other (measured times in
//                docs/kernels/uncertainty.md).
//   prior        with a pose prior on the solve (uncertainty_prior_kernel) lane 0 adds the prior's J^T J to the reduced sums with
//                the solve's own prior_accumulate before the matrices are read: `information` is then the posterior one.
//   stores       the record is assembled in LDS and written with plain 8-byte vector stores by all lanes.
#pragma once
#include "msfl_kernels.cuh"

namespace msfl {

struct UncRecord {   // mirrors msfl_match_uncertainty
  double information[36];
  double eigenvalues[6];
  double eigenvectors[36];
  double covariance[36];
  double sigma2;
  int n_residuals, n_degenerate, valid, reserved_;
};
static_assert(sizeof(UncRecord) == 936, "msfl_match_uncertainty layout");
constexpr int kUncWords = (int)(sizeof(UncRecord) / 8);

// Eigen-decomposition of a symmetric 6 x 6 by cyclic Jacobi rotations (Rutishauser's form: tan of the rotation angle
// from the smaller root, entries that no longer change the diagonal are set to zero from the fifth sweep on).
// a: in the matrix (both triangles), out its diagonal holds the eigenvalues; v: out, COLUMN k is the eigenvector of
// a[k][k].  Converges quadratically: 6-8 sweeps for the matrices met here.  Single lane.
__device__ __forceinline__ void sym_eigen6_jacobi(double (&a)[6][6], double (&v)[6][6]) {
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; sweep++) {
    double off = 0.0;
#pragma unroll
    for (int p = 0; p < 5; p++)
#pragma unroll
      for (int q = p + 1; q < 6; q++) off += fabs(a[p][q]);
    if (!(off > 0.0)) break;
#pragma unroll
    for (int p = 0; p < 5; p++) {
#pragma unroll
      for (int q = p + 1; q < 6; q++) {
        const double apq = a[p][q];
        const double g = 100.0 * fabs(apq);
        if (sweep >= 4 && fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
          a[p][q] = 0.0; a[q][p] = 0.0;
        } else if (apq != 0.0) {
          const double hd = a[q][q] - a[p][p];
          double t;
          if (fabs(hd) + g == fabs(hd)) {
            t = apq / hd;
          } else {
            const double theta = 0.5 * hd / apq;
            t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0.0) t = -t;
          }
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          a[p][p] -= t * apq; a[q][q] += t * apq;
          a[p][q] = 0.0; a[q][p] = 0.0;
#pragma unroll
          for (int k = 0; k < 6; k++) {
            if (k == p || k == q) continue;
            const double akp = a[k][p], akq = a[k][q];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            a[k][p] = np_; a[p][k] = np_; a[k][q] = nq_; a[q][k] = nq_;
          }
#pragma unroll
          for (int k = 0; k < 6; k++) {
            const double vkp = v[k][p], vkq = v[k][q];
            v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
          }
        }
      }
    }
  }
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, MSFL_LM_WAVES)
uncertainty_kernel(BatchView bv, const double* __restrict__ pprime_all, const double* __restrict__ rec_all,
                   const double* __restrict__ poses, const int* __restrict__ status, const DevMatchInfo* __restrict__ info,
                   int outer_it, double huber, int min_correspondences, double min_eigenvalue, UncRecord* __restrict__ out) {
#define MSFL_UNC_PRIOR 0
#include "msfl_uncertainty_body.inc"
#undef MSFL_UNC_PRIOR
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, MSFL_LM_WAVES) MSFL_PRIOR_TEXT
uncertainty_prior_kernel(BatchView bv, const double* __restrict__ pprime_all, const double* __restrict__ rec_all,
                         const double* __restrict__ poses, const int* __restrict__ status, const DevMatchInfo* __restrict__ info,
                         int outer_it, double huber, int min_correspondences, double min_eigenvalue, UncRecord* __restrict__ out,
                         const PosePrior* __restrict__ prior_all) {
#define MSFL_UNC_PRIOR 1
#include "msfl_uncertainty_body.inc"
#undef MSFL_UNC_PRIOR
}

// The one launch helper of all six solve sites: `out` null = feature off (nothing is launched).
// `info` must not be null when `out` is not: sigma2 is formed from the solve's own final cost.
// `prior`: what the solve was launched with (launch_lm_solve), null = no pose prior.
template <int BLOCK>
inline void launch_uncertainty(hipStream_t st, int n_scans, const BatchView& bv, const double* pprime, const double* records,
                               const double* poses, const int* status, const DevMatchInfo* info, int last_outer_it,
                               const SolverParams& sp, double min_eigenvalue, UncRecord* out, const PosePrior* prior = nullptr) {
  if (!out || n_scans <= 0) return;
  if (!prior)
    hipLaunchKernelGGL(uncertainty_kernel<BLOCK>, dim3(n_scans), dim3(BLOCK), 0, st, bv, pprime, records, poses, status, info,
                       last_outer_it, sp.huber, sp.min_correspondences, min_eigenvalue, out);
  else
    hipLaunchKernelGGL(uncertainty_prior_kernel<BLOCK>, dim3(n_scans), dim3(BLOCK), 0, st, bv, pprime, records, poses, status, info,
                       last_outer_it, sp.huber, sp.min_correspondences, min_eigenvalue, out, prior);
}

}  // namespace msfl
