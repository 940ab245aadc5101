// msfl_degeneracy.cuh — degeneracy-aware solve: solution remapping after Zhang & Singh (msfl_set_degeneracy,
// include/msfl_c_api.h; docs/kernels/degeneracy.md).
//
// lm_solve_degen_kernel is the third sibling over msfl_lm_solve_body.inc.  At iteration 0 of every solve lane 0 decomposes
// the entry matrix H0 (lidar rows + prior block, if any) with the uncertainty kernel's cyclic Jacobi and holds every
// eigen-direction below the threshold: the solve is then Ceres' trust-region LM on the reduced problem
// Plus_r(x, y) = Plus(x, V_k y).  Realisation: after each reduction {g, H} are rotated into the eigenbasis and the held
// coordinates decoupled (zero gradient, zero off-diagonals, unit diagonal), so the 6 x 6 factorisation of tr_propose is
// reused — the held coordinates come first (ascending eigenvalues), every multiply-add they enter adds an exact zero, and
// the kept block is factorised as a k x k on its own would be.  With nothing held the kernel calls tr_propose / tr_decide
// on the untouched sums: that registration is bit for bit the feature-off one.
//
// Everything here runs on lane 0 between the evaluation passes, on LDS-resident data, with plain vector loads and stores.
#pragma once
#include "msfl_uncertainty.cuh"

namespace msfl {

struct DegenRecord {   // mirrors msfl_degeneracy_record; index = outer iteration
  double eigenvalues[2][6];
  double eigenvectors[2][36];
  int n_held[2];
  int valid[2];
};
static_assert(sizeof(DegenRecord) == 688, "msfl_degeneracy_record layout");

// Per-solve state in LDS, lane 0 only.
struct DegenState {
  double V[6][6];        // ROW k = eigenvector k of H0, ascending eigenvalue order, sign as in msfl_match_uncertainty
  double lambda[6];
  double y[6], d[6];     // degen_map_step: step in the eigenbasis -> pose tangent
  int n_held;            // the n_held smallest are held
};

// Feature-on code gets a section name of its own, as the prior's does (MSFL_PRIOR_TEXT): it is emitted behind the plain
// kernels and does not move them relative to tr_propose / tr_decide.
#define MSFL_DEGEN_TEXT __attribute__((section(".text.msfl_degen")))

// Decomposes H0 (packed in red[7..27]) and classifies: direction k is held when lambda_k < max(min_eig, 1e-14 lambda_max),
// the rule of msfl_match_uncertainty.n_degenerate.  Returns n_held.
__device__ __noinline__ MSFL_DEGEN_TEXT int degen_decompose(const double* red, double min_eig, DegenState& dg) {
  double a[6][6], v[6][6], g[6];
  unpack_system(red, a, g);
  sym_eigen6_jacobi(a, v);
  double lmax = a[0][0];
#pragma unroll
  for (int k = 1; k < 6; k++) lmax = fmax(lmax, a[k][k]);
  const double thr = fmax(min_eig, 1e-14 * lmax);
  int n_held = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    // ascending position of eigenpair k (stable) and the sign convention of uncertainty_kernel: the largest-magnitude
    // component (lowest index on ties) is positive
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) rank += (a[j][j] < a[k][k] || (a[j][j] == a[k][k] && j < k)) ? 1 : 0;
    double big = fabs(v[0][k]), sgn = v[0][k] < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 1; i < 6; i++)
      if (fabs(v[i][k]) > big) { big = fabs(v[i][k]); sgn = v[i][k] < 0.0 ? -1.0 : 1.0; }
    dg.lambda[rank] = a[k][k];
#pragma unroll
    for (int i = 0; i < 6; i++) dg.V[rank][i] = sgn * v[i][k];
    n_held += a[k][k] < thr ? 1 : 0;
  }
  dg.n_held = n_held;
  return n_held;
}

// {g, H} in red -> the reduced problem's, embedded in 6 x 6: g' = V g, H' = V H V^T (rows of V are the eigenvectors), then
// the held coordinates decoupled: g'_k = 0, H'_kk = 1, H'_kj = 0.  The cost red[0] is untouched.
__device__ __noinline__ MSFL_DEGEN_TEXT void degen_rotate(const DegenState& dg, double* red) {
  double H[6][6], g[6], T[6][6];
  unpack_system(red, H, g);
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) s += dg.V[k][i] * g[i];
    red[1 + k] = k < dg.n_held ? 0.0 : s;
  }
#pragma unroll
  for (int i = 0; i < 6; i++)            // T = H V^T
#pragma unroll
    for (int k = 0; k < 6; k++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 6; j++) s += H[i][j] * dg.V[k][j];
      T[i][k] = s;
    }
  int n = 7;
#pragma unroll
  for (int p = 0; p < 6; p++)
#pragma unroll
    for (int q = p; q < 6; q++) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < 6; i++) s += dg.V[p][i] * T[i][q];
      red[n++] = p < dg.n_held ? (p == q ? 1.0 : 0.0) : s;      // p <= q: a held q implies a held p
    }
}

// dg.d = V_k dg.y: the tangent step applied to the pose.  The held coordinates are left out of the sum, so the step has no
// component along a held eigenvector whatever dg.y holds there.
__device__ __noinline__ MSFL_DEGEN_TEXT void degen_map_step(DegenState& dg) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) s += k < dg.n_held ? 0.0 : dg.V[k][i] * dg.y[k];
    dg.d[i] = s;
  }
}

// Gradient max norm of the reduced problem, |x - Plus_r(x, -g_r)|_inf = |x - Plus(x, -V_k g_r)|_inf; gr = tr.sys + 1 as
// degen_rotate left it.  The shortcut of gradient_max_norm_for_test holds for the mapped gradient as for any other.
__device__ __noinline__ MSFL_DEGEN_TEXT double degen_gradient_max_norm(const DegenState& dg, const double* x7, const double* gr,
                                                                       double gtol) {
  double gf[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) s += k < dg.n_held ? 0.0 : dg.V[k][i] * gr[k];
    gf[i] = s;
  }
  return gradient_max_norm_for_test(load_pose(x7), gf, gtol);
}

// tr_propose on the rotated system; the step goes to the pose through V_k.
__device__ __noinline__ MSFL_DEGEN_TEXT int tr_propose_degen(TrState& tr, const SolverParams prm, DegenState& dg) {
#define MSFL_TR_DEGEN 1
#include "msfl_tr_propose_body.inc"
#undef MSFL_TR_DEGEN
}

// The per-solve record of registration b, outer iteration it: lane 0, 44 plain stores.
__device__ __forceinline__ void degen_write_record(const DegenState& dg, DegenRecord* out, int it) {
#pragma unroll
  for (int k = 0; k < 6; k++) out->eigenvalues[it][k] = dg.lambda[k];
#pragma unroll
  for (int k = 0; k < 6; k++)
#pragma unroll
    for (int i = 0; i < 6; i++) out->eigenvectors[it][6 * k + i] = dg.V[k][i];
  out->n_held[it] = dg.n_held;
  out->valid[it] = 1;
}

// The sibling with solution remapping.  prior_all may be null (no pose prior): there is no fourth sibling.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, MSFL_LM_WAVES) MSFL_DEGEN_TEXT
lm_solve_degen_kernel(BatchView bv, const double* __restrict__ pprime_all, const double* __restrict__ rec_all,
                      double* __restrict__ poses, int* __restrict__ status, DevMatchInfo* __restrict__ info,
                      int outer_it, SolverParams prm, const PosePrior* __restrict__ prior_all, double degen_min_eig,
                      DegenRecord* __restrict__ degen_out) {
#define MSFL_LM_PRIOR 0
#define MSFL_LM_DEGEN 1
#include "msfl_lm_solve_body.inc"
#undef MSFL_LM_DEGEN
#undef MSFL_LM_PRIOR
}

}  // namespace msfl
