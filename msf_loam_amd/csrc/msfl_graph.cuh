// Pose-graph optimisation (msfl_graph_*): Ceres' trust-region / LM loop over a chain of poses with a few long edges, all f64.
// docs/kernels/graph.md holds the definition.  The step (Js^T Js + D^2) s = -Js^T r is solved by PCG whose preconditioner is the
// exact solve of the block-tridiagonal part T (block cyclic reduction); long edges enter through the mat-vec only.
//
// Rules every kernel here keeps:
//   - no floating-point atomics: factors are gathered per node in adjacency order, sums (maxima, minima) over nodes / factors go
//     through graph_block_reduce (a fixed LDS tree) into one partial per workgroup and graph_total (the same tree over the partials);
//   - no grid-wide barrier: a reduction level is a launch, the tail of the reduction is one workgroup;
//   - a kernel that finds GraphState::done (or cg_done) set returns at once: the host enqueues a fixed launch pattern.
// One lane owns one factor or one node; 6 x 6 blocks live in registers (fully unrolled loops), so the block kernels run 64 lanes
// per workgroup and take what VGPRs they need.
//
// The solve (one right-hand side: the step) and the marginals (six per requested node: unit columns) share every body of the cyclic
// reduction and the mat-vec's operator.  The bodies are templates over the column count W of a node's 6 x W right-hand side (1 or 6)
// and over kPivot (the marginals' pivot test in the factor half); a small column-set type (GraphSolveCols, GraphMargCols) says where
// the levels live and when the kernel may return.  What differs stays apart: the two CG state machines and their kernels.
//
// Factors are numbered edges, fixes, information edges, information fixes.  The first two kinds (k < n_plain) are the reference's and
// keep their kernels; the information kinds (a full square-root information matrix L per factor) have kernels of their own over
// [n_plain, n_factors), launched only when the graph holds one.  Everything behind the 78-double linearised record is generic.
#pragma once
#include <hip/hip_runtime.h>

#include "msfl_graph_host.h"

namespace msfl {

constexpr int kGraphBlock = 64;      // block kernels: one factor / node per lane
constexpr int kGraphVec = 256;       // vector kernels: one node (6 values) per lane; also the partial size of every sum
constexpr int kGraphJ = 78;          // doubles per linearised factor: Ji (36, row-major), Jj (36), r (6), after the corrector

enum { kGraphEmpty = 0, kGraphGradient, kGraphMaxIter, kGraphMinRadius, kGraphInvalid, kGraphParameter, kGraphFunction };

struct GraphOpt {
  int max_iter, max_invalid, jacobi;
  double huber, radius0, radius_max, radius_min, min_rel, lm_min, lm_max, ftol, gtol, ptol, cg_tol;
};

struct GraphState {                  // one record; the host reads it once per LM iteration
  double radius, decrease_factor, cost, x_norm, gmax, initial_cost, final_cost;
  double rz[2], rz0;
  int iterations, successful, invalid, step_successful, termination, done, commit, first;
  int cg_done, cg_it, cg_total, cg_unconverged, n_trace, pad;
};

struct GraphDev {
  int n_nodes, n_free, n_edges, n_factors;
  const int* free_of;                // [nodes]: free index or -1
  const int* node_of;                // [free]
  const int* adj_off; const int* adj;       // per free node: 2 * factor + side, in the factor numbering (each kind in insertion order)
  const int* ladj_off; const int* ladj;     // the long factors among them
  const int* fac_ij;                 // [factors x 2]: node indices
  const double* fac_data;            // [factors x 9]: edge z[7], sr, st; fix t, p[3], st
  double* x; double* cand;           // [nodes x 7]
  double* J;                         // [factors x kGraphJ]
  double* fcost; double* fmodel;     // [factors]: rho / 2 per block; the block's share of the model cost change
  double* H; double* Lb; double* g; double* scale;   // [free x 36, 36, 6, 6]: unscaled diagonal block, block (f, f-1), gradient, Jacobi scale
  double* nxx; double* ngmax; double* nstep;         // [free]: |x|^2, max |x - Plus(x, -g)|, |x - cand|^2
  double* D; double* L; double* Dinv;                // cyclic reduction levels; level 0 of D, L is the damped scaled T
  double* rhs; double* sol;          // levels 1.. of the right-hand side / solution (level 0: r and z)
  double* b; double* xs; double* r; double* z; double* p[2]; double* q;   // [free x 6]
  double* part;                      // [2 x workgroups]: partials of p.q, of r.z
  GraphState* st;
  int* tr_accepted; double* tr_cost; // [max_iter]
  int n_plain, n_einfo;              // edges + fixes; information edges (factors n_plain + n_einfo .. are information fixes)
  const double* fac_L;               // [information factors x 36]: L row-major (6 x 6; a fix's 3 x 3 in the first 9); their fac_data: edge z[7]; fix t, p[3]
};

// msfl_graph_marginals (section "marginals" below)
struct GraphMargCol { double rz[2], rz0; int it, done; };
struct GraphMargState { double min_pivot; int singular, pad; };
struct GraphMarg {
  int n_cols, n_part;                // column nodes of this chunk; workgroups per column node of the node-per-lane kernels
  const int* col_free;               // [n_cols]: free index of the column node
  double* X; double* R; double* Z; double* P[2]; double* Q;   // [n_cols x free x 36]
  double* rhs; double* sol;          // [n_cols x (blocks - free) x 36]: levels 1.. of the reduction
  double* part;                      // [2 x n_cols x 6 x n_part]: partials of p . q, then of r . z
  GraphMargCol* col;                 // [n_cols x 6]
  GraphMargState* st;
  double* piv;                       // one partial minimum per workgroup of the invert launches, level after level
};

// ---- sums, maxima and minima with one stated order -------------------------------------------------------------------------
enum { kGraphSum, kGraphMax, kGraphMin };
template <int kThreads, int kOp>
__device__ __forceinline__ double graph_block_reduce(double v, double* lds) {
  const int t = (int)threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) lds[t] = kOp == kGraphMax ? fmax(lds[t], lds[t + s]) : kOp == kGraphMin ? fmin(lds[t], lds[t + s]) : lds[t] + lds[t + s];
    __syncthreads();
  }
  const double out = lds[0];
  __syncthreads();
  return out;
}
// every lane of the workgroup gets the total of a[0 .. n): lane t adds a[t], a[t + kThreads], ... in that order, then the tree
template <int kThreads, int kOp>
__device__ __forceinline__ double graph_total(const double* __restrict__ a, int n, double* lds) {
  static_assert(kOp != kGraphMin, "a minimum has no neutral start here");
  double v = 0.0;
  for (int i = (int)threadIdx.x; i < n; i += kThreads) v = kOp == kGraphMax ? fmax(v, a[i]) : v + a[i];
  return graph_block_reduce<kThreads, kOp>(v, lds);
}

// ---- quaternions [x y z w] and 6 x 6 blocks (row-major) ------------------------------------------------------------------
__device__ __forceinline__ void gq_mul(const double* a, const double* b, double* o) {
  o[0] = a[3] * b[0] + b[3] * a[0] + (a[1] * b[2] - a[2] * b[1]);
  o[1] = a[3] * b[1] + b[3] * a[1] + (a[2] * b[0] - a[0] * b[2]);
  o[2] = a[3] * b[2] + b[3] * a[2] + (a[0] * b[1] - a[1] * b[0]);
  o[3] = a[3] * b[3] - (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}
// Eigen's unit-quaternion q * v = v + 2 w (u x v) + 2 u x (u x v)
__device__ __forceinline__ void gq_rot(const double* q, const double* v, double* o) {
  const double c0 = q[1] * v[2] - q[2] * v[1], c1 = q[2] * v[0] - q[0] * v[2], c2 = q[0] * v[1] - q[1] * v[0];
  o[0] = v[0] + 2.0 * (q[3] * c0 + (q[1] * c2 - q[2] * c1));
  o[1] = v[1] + 2.0 * (q[3] * c1 + (q[2] * c0 - q[0] * c2));
  o[2] = v[2] + 2.0 * (q[3] * c2 + (q[0] * c1 - q[1] * c0));
}
__device__ __forceinline__ void gq_to_R(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
// EigenQuaternionParameterization::Plus on the rotation, t + dt on the translation
__device__ __forceinline__ void graph_plus(const double* x, const double* d, double* o) {
  o[0] = x[0] + d[0]; o[1] = x[1] + d[1]; o[2] = x[2] + d[2];
  const double n = sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  if (n > 0.0) {
    const double k = sin(n) / n;
    const double dq[4] = {k * d[3], k * d[4], k * d[5], cos(n)};
    gq_mul(dq, x + 3, o + 3);
  } else {
    o[3] = x[3]; o[4] = x[4]; o[5] = x[5]; o[6] = x[6];
  }
}

template <int kN = 36>
__device__ __forceinline__ void g6_load(const double* __restrict__ p, double* a) {
#pragma unroll
  for (int i = 0; i < kN; i++) a[i] = p[i];
}
template <int kN = 36>
__device__ __forceinline__ void g6_store(double* __restrict__ p, const double* a) {
#pragma unroll
  for (int i = 0; i < kN; i++) p[i] = a[i];
}
// The one block product: Y (6 x W, row-major) from op(A) (6 x 6) and op(X) (6 x W; kTX needs W = 6).  How the six-term sum s of an
// entry meets Y is the caller's choice, because it rounds differently: kG6Set Y = s; kG6Chain the sum starts at Y and goes on term by
// term; kG6Add Y += sign * s.
enum { kG6Set, kG6Chain, kG6Add };
template <int W, int kForm, bool kTA, bool kTX = false>
__device__ __forceinline__ void g6_mul(const double* A, const double* X, double* Y, double sign = 1.0) {
  static_assert(!kTX || W == 6, "only a square block can be transposed");
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < W; j++) {
      double s = kForm == kG6Chain ? Y[i * W + j] : 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) s += (kTA ? A[k * 6 + i] : A[i * 6 + k]) * (kTX ? X[j * 6 + k] : X[k * W + j]);
      if (kForm == kG6Add) Y[i * W + j] += sign * s;
      else Y[i * W + j] = s;
    }
}
// y (+)= A x, y (+)= A^T x
template <bool kAcc, bool kTrans>
__device__ __forceinline__ void g6_mv(const double* A, const double* x, double* y) { g6_mul<1, kAcc ? kG6Chain : kG6Set, kTrans>(A, x, y); }
// C += sign * op(A) op(B): kTA / kTB transpose the operand
template <bool kTA, bool kTB>
__device__ __forceinline__ void g6_mma(const double* A, const double* B, double* Cm, double sign) { g6_mul<6, kG6Add, kTA, kTB>(A, B, Cm, sign); }
// In the bodies shared by the solve (W = 1) and the marginals (W = 6) the two column counts do not use the same form, and must not be
// given the same one: the results of both paths are pinned to the bit (tests/golden/graph_parent_v1.npz and the byte tests).
//   T = op(A) X:   W = 1 overwrites; W = 6 adds the sum to zero (a sum of -0.0 becomes +0.0);
//   Q += op(A) X:  W = 1 continues Q's sum term by term; W = 6 adds the finished sum.
// Q -= op(A) X is kG6Add with sign -1 for both: Q + (-1 s) and Q - s are the same operation.
template <int W, bool kTA>
__device__ __forceinline__ void g6_fresh(const double* A, const double* X, double* T) {
  if (W == 1) { g6_mul<W, kG6Set, kTA>(A, X, T); return; }
#pragma unroll
  for (int i = 0; i < 6 * W; i++) T[i] = 0.0;
  g6_mul<W, kG6Add, kTA>(A, X, T);
}
template <int W, bool kTA>
__device__ __forceinline__ void g6_accum(const double* A, const double* X, double* Q) { g6_mul<W, W == 1 ? kG6Chain : kG6Add, kTA>(A, X, Q); }
// inverse of a symmetric positive definite block through its Cholesky factor (a block that is not gives NaN: an invalid step).  With
// kPivot it returns the block's smallest pivot^2 / a_jj (-1 when one is not finite); without, 1.
template <bool kPivot>
__device__ __forceinline__ double g6_inv_spd(double* a) {
  double ratio = 1.0;
#pragma unroll
  for (int j = 0; j < 6; j++) {                    // A = C C^T, C lower, in place
    const double ajj = a[j * 6 + j];
    double d = ajj;
#pragma unroll
    for (int k = 0; k < j; k++) d -= a[j * 6 + k] * a[j * 6 + k];
    if (kPivot) {
      const double q = d / ajj;
      ratio = fmin(ratio, isfinite(q) ? q : -1.0);
    }
    d = sqrt(d);
    a[j * 6 + j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = a[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= a[i * 6 + k] * a[j * 6 + k];
      a[i * 6 + j] = s / d;
    }
  }
#pragma unroll
  for (int j = 0; j < 6; j++) {                    // W = C^-1, lower, into the upper triangle's mirror: w(i, j) kept at a[j * 6 + i], i > j
    a[j * 6 + j] = 1.0 / a[j * 6 + j];
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = 0.0;
#pragma unroll
      for (int k = j; k < i; k++) s -= a[i * 6 + k] * (k == j ? a[j * 6 + j] : a[j * 6 + k]);
      a[j * 6 + i] = s / a[i * 6 + i];
    }
  }
  double w[36];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) w[i * 6 + j] = i == j ? a[i * 6 + i] : (i > j ? a[j * 6 + i] : 0.0);
#pragma unroll
  for (int i = 0; i < 6; i++)                      // A^-1 = W^T W
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = i; k < 6; k++) s += w[k * 6 + i] * w[k * 6 + j];
      a[i * 6 + j] = s; a[j * 6 + i] = s;
    }
  return ratio;
}

// ---- factors -----------------------------------------------------------------------------------------------------------
// residual of factor k at poses `x` (before the corrector); rows 3..5 of a fix are zero.  With kJac also Ji, Jj (row-major 6 x 6).
template <bool kJac>
__device__ __forceinline__ void graph_factor(const GraphDev& G, const double* __restrict__ x, int k, double* r, double* Ji, double* Jj) {
  const int ni = G.fac_ij[2 * k], nj = G.fac_ij[2 * k + 1];
  const double* d = G.fac_data + (size_t)k * 9;
  const double* xi = x + (size_t)ni * 7; const double* xj = x + (size_t)nj * 7;
  if (kJac) {
#pragma unroll
    for (int i = 0; i < 36; i++) { Ji[i] = 0.0; Jj[i] = 0.0; }
  }
  if (k >= G.n_edges) {                            // position fix: t, p[3], st
    const double t = d[0], st = d[4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      r[c] = ((1.0 - t) * xi[c] + t * xj[c] - d[1 + c]) / st;
      r[3 + c] = 0.0;
      if (kJac) { Ji[c * 6 + c] = (1.0 - t) / st; Jj[c * 6 + c] = t / st; }
    }
    return;
  }
  const double sr = d[7], st = d[8];
  const double qi[4] = {xi[3], xi[4], xi[5], xi[6]}, qz[4] = {d[3], d[4], d[5], d[6]};
  const double A[4] = {-xj[3], -xj[4], -xj[5], xj[6]};
  double a[3], v[3], B[4], e[3], qe[4];
  gq_rot(qi, d, a);                                // R_i t_z
#pragma unroll
  for (int c = 0; c < 3; c++) v[c] = a[c] + xi[c] - xj[c];
  gq_mul(qi, qz, B);
  gq_rot(A, v, e);
  gq_mul(A, B, qe);
#pragma unroll
  for (int c = 0; c < 3; c++) { r[c] = e[c] / st; r[3 + c] = qe[c] / sr; }
  if (!kJac) return;
  double R[9];
  gq_to_R(xj + 3, R);
  // translation rows: d/dt_i = R_j^T / st, d/dd_i = R_j^T (-2 [a]x) / st, d/dt_j = -R_j^T / st, d/dd_j = R_j^T (2 [v]x) / st
  const double Sa[9] = {0.0, 2.0 * a[2], -2.0 * a[1], -2.0 * a[2], 0.0, 2.0 * a[0], 2.0 * a[1], -2.0 * a[0], 0.0};     // -2 [a]x
  const double Sv[9] = {0.0, -2.0 * v[2], 2.0 * v[1], 2.0 * v[2], 0.0, -2.0 * v[0], -2.0 * v[1], 2.0 * v[0], 0.0};     //  2 [v]x
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double rt = R[j * 3 + i];               // R_j^T (i, j)
      Ji[i * 6 + j] = rt / st; Jj[i * 6 + j] = -rt / st;
      double sa = 0.0, sv = 0.0;
#pragma unroll
      for (int m = 0; m < 3; m++) { sa += R[m * 3 + i] * Sa[m * 3 + j]; sv += R[m * 3 + i] * Sv[m * 3 + j]; }
      Ji[i * 6 + 3 + j] = sa / st; Jj[i * 6 + 3 + j] = sv / st;
    }
  // rotation rows: column c of M is vec(A (x) [e_c, 0] (x) B); d/dd_i = M / sr, d/dd_j = -M / sr
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double ec[4] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0, 0.0};
    double t1[4], t2[4];
    gq_mul(A, ec, t1);
    gq_mul(t1, B, t2);
#pragma unroll
    for (int i = 0; i < 3; i++) { Ji[(3 + i) * 6 + 3 + c] = t2[i] / sr; Jj[(3 + i) * 6 + 3 + c] = -(t2[i] / sr); }
  }
}

// HuberLoss through the rho'' <= 0 corrector: *half_rho = rho / 2, returns sqrt(rho')
__device__ __forceinline__ double graph_huber(const double* r, double a, double* half_rho) {
  double sq = 0.0;
#pragma unroll
  for (int c = 0; c < 6; c++) sq += r[c] * r[c];
  const double b = a * a;
  if (a > 0.0 && sq > b) {
    const double n = sqrt(sq);
    *half_rho = 0.5 * (2.0 * a * n - b);
    return sqrt(fmax(2.2250738585072014e-308, a / n));
  }
  *half_rho = 0.5 * sq;
  return 1.0;
}
// rho' of the same loss alone (msfl_graph_factor_weights)
__device__ __forceinline__ double graph_huber_weight(double sq, double a) {
  return a > 0.0 && sq > a * a ? fmax(2.2250738585072014e-308, a / sqrt(sq)) : 1.0;
}

// A loss per factor (msfl_graph_set_losses): rho and rho' (clamped) of kind / a at s = |r|^2, b = a^2, in Ceres' forms; all six kinds
// have rho'' <= 0, so the corrector is graph_huber's.  DEFAULT is HuberLoss(huber), no loss when huber <= 0.  One lane per factor:
// the lanes of a wavefront branch on their kinds.  msfl_graph_host.h has the host's twin, operation for operation.
__device__ __forceinline__ double graph_loss_rho(double s, int kind, double a, double huber, double* rho1) {
  if (kind == kGraphLossDefault) { kind = huber > 0.0 ? kGraphLossHuber : kGraphLossNone; a = huber; }
  const double b = a * a;
  double rho = s, w = 1.0;
  if (kind == kGraphLossHuber) {
    if (s > b) { const double n = sqrt(s); rho = 2.0 * a * n - b; w = a / n; }
  } else if (kind == kGraphLossSoftLOne) {
    const double t = sqrt(1.0 + s / b);
    rho = 2.0 * b * (t - 1.0); w = 1.0 / t;
  } else if (kind == kGraphLossCauchy) {
    const double q = 1.0 + s / b;
    rho = b * log(q); w = 1.0 / q;
  } else if (kind == kGraphLossGemanMcClure) {
    const double q = b / (b + s);
    rho = q * s; w = q * q;
  }
  *rho1 = fmax(2.2250738585072014e-308, w);
  return rho;
}
// The loss of factor k as the factor kernels see it, graph_huber's contract (*half_rho = rho / 2, returns sqrt(rho')) and rho' alone at
// |r|^2 = sq.  The kernels end in a parameter pack that is empty for the graph that never set a loss (every factor under
// HuberLoss(huber): the kernels, arguments and instructions there always were) or holds the two per-factor arrays, in the factor
// numbering (their siblings, launched once msfl_graph_set_losses has allocated the arrays).
struct GraphLossDev { const int* kind; const double* a; };
__device__ __forceinline__ double graph_factor_scale(int, const double* r, double huber, double* half_rho) { return graph_huber(r, huber, half_rho); }
__device__ __forceinline__ double graph_factor_scale(int k, const double* r, double huber, double* half_rho, const GraphLossDev& L) {
  double sq = 0.0, w;
#pragma unroll
  for (int c = 0; c < 6; c++) sq += r[c] * r[c];
  *half_rho = 0.5 * graph_loss_rho(sq, L.kind[k], L.a[k], huber, &w);
  return sqrt(w);
}
__device__ __forceinline__ double graph_factor_weight(int, double sq, double huber) { return graph_huber_weight(sq, huber); }
__device__ __forceinline__ double graph_factor_weight(int k, double sq, double huber, const GraphLossDev& L) {
  double w;
  (void)graph_loss_rho(sq, L.kind[k], L.a[k], huber, &w);
  return w;
}

__global__ __launch_bounds__(kGraphVec) void graph_commit_kernel(GraphDev G) {
  if (!G.st->commit) return;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < G.n_nodes * 7) G.x[i] = G.cand[i];
}

template <class... Loss>
__global__ __launch_bounds__(kGraphBlock) void graph_linearize_kernel(GraphDev G, double huber, Loss... loss) {
  if (G.st->done) return;
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= G.n_plain) return;
  double r[6], Ji[36], Jj[36], hr;
  graph_factor<true>(G, G.x, k, r, Ji, Jj);
  const double s = graph_factor_scale(k, r, huber, &hr, loss...);
  double* o = G.J + (size_t)k * kGraphJ;
#pragma unroll
  for (int i = 0; i < 36; i++) { o[i] = s * Ji[i]; o[36 + i] = s * Jj[i]; }
#pragma unroll
  for (int i = 0; i < 6; i++) o[72 + i] = s * r[i];
  G.fcost[k] = hr;
}

// factor k's share of the model cost change -m . (r + m / 2), m = Js step, from its linearised record
__device__ __forceinline__ double graph_model_share(const GraphDev& G, int k) {
  const double* Jk = G.J + (size_t)k * kGraphJ;
  double m[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const int f = G.free_of[G.fac_ij[2 * k + side]];
    if (f < 0) continue;
    double sx[6];
#pragma unroll
    for (int c = 0; c < 6; c++) sx[c] = G.scale[(size_t)f * 6 + c] * G.xs[(size_t)f * 6 + c];
    g6_mv<true, false>(Jk + 36 * side, sx, m);
  }
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 6; c++) s += m[c] * (Jk[72 + c] + 0.5 * m[c]);
  return -s;
}

// cost of every plain block at `x` into fcost; with kModel also the block's share of the model cost change
template <bool kModel, class... Loss>
__global__ __launch_bounds__(kGraphBlock) void graph_cost_kernel(GraphDev G, const double* __restrict__ x, double huber, Loss... loss) {
  if (kModel && G.st->done) return;
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= G.n_plain) return;
  double r[6], hr;
  graph_factor<false>(G, x, k, r, nullptr, nullptr);
  (void)graph_factor_scale(k, r, huber, &hr, loss...);
  G.fcost[k] = hr;
  if (!kModel) return;
  G.fmodel[k] = graph_model_share(G, k);
}

// ---- information factors (docs/kernels/graph.md): r = L e with a full square-root information matrix per factor -----------------------
// information edge k: e = [R_i^T (t_j - t_i) - z.t ; 2 s vec(qe)], qe = conj(z.q) (x) conj(q_i) (x) q_j, s = -1 when qe.w < 0.
// With kJac also the three 3 x 3 blocks de/d. is made of (row-major): Rt = R_i^T, B = 2 R_i^T [t_j - t_i]x and M, whose column c is
// 2 s vec(conj(z.q) (x) conj(q_i) (x) [e_c, 0] (x) q_j):
//   de/d(dt_i, d_i) = [-Rt  B ; 0  -M],   de/d(dt_j, d_j) = [Rt  0 ; 0  M].
// Every product that holds z.q holds it once, so -z.q negates qe and M's columns exactly and s undoes it: the same bits.
template <bool kJac>
__device__ __forceinline__ void graph_info_edge_error(const GraphDev& G, const double* __restrict__ x, int k, double* e, double* Rt, double* B, double* M) {
  const double* d = G.fac_data + (size_t)k * 9;
  const double* xi = x + (size_t)G.fac_ij[2 * k] * 7; const double* xj = x + (size_t)G.fac_ij[2 * k + 1] * 7;
  const double ci[4] = {-xi[3], -xi[4], -xi[5], xi[6]}, cz[4] = {-d[3], -d[4], -d[5], d[6]}, qj[4] = {xj[3], xj[4], xj[5], xj[6]};
  const double u[3] = {xj[0] - xi[0], xj[1] - xi[1], xj[2] - xi[2]};
  double tij[3], A[4], qe[4];
  gq_rot(ci, u, tij);
  gq_mul(cz, ci, A);
  gq_mul(A, qj, qe);
  const double s2 = qe[3] < 0.0 ? -2.0 : 2.0;
#pragma unroll
  for (int c = 0; c < 3; c++) { e[c] = tij[c] - d[c]; e[3 + c] = s2 * qe[c]; }
  if (!kJac) return;
  double R[9];
  gq_to_R(xi + 3, R);
  const double S[9] = {0.0, -2.0 * u[2], 2.0 * u[1], 2.0 * u[2], 0.0, -2.0 * u[0], -2.0 * u[1], 2.0 * u[0], 0.0};       // 2 [u]x
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      Rt[i * 3 + j] = R[j * 3 + i];
      double b = 0.0;
#pragma unroll
      for (int m = 0; m < 3; m++) b += R[m * 3 + i] * S[m * 3 + j];
      B[i * 3 + j] = b;
    }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double ec[4] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0, 0.0};
    double t1[4], t2[4];
    gq_mul(A, ec, t1);
    gq_mul(t1, qj, t2);
#pragma unroll
    for (int i = 0; i < 3; i++) M[i * 3 + c] = s2 * t2[i];
  }
}
// information fix k: e = (1 - t) t_i + t t_j - p
__device__ __forceinline__ void graph_info_fix_error(const GraphDev& G, const double* __restrict__ x, int k, double* e) {
  const double* d = G.fac_data + (size_t)k * 9;
  const double* xi = x + (size_t)G.fac_ij[2 * k] * 7; const double* xj = x + (size_t)G.fac_ij[2 * k + 1] * 7;
#pragma unroll
  for (int c = 0; c < 3; c++) e[c] = (1.0 - d[0]) * xi[c] + d[0] * xj[c] - d[1 + c];
}
// residual of information factor m (factor n_plain + m) at poses `x`, before the corrector; rows 3..5 of a fix are zero
__device__ __forceinline__ void graph_info_residual(const GraphDev& G, const double* __restrict__ x, int m, double* r) {
  const int k = G.n_plain + m;
  const double* __restrict__ L = G.fac_L + (size_t)m * 36;
  if (m >= G.n_einfo) {
    double e[3];
    graph_info_fix_error(G, x, k, e);
#pragma unroll
    for (int i = 0; i < 3; i++) { r[i] = L[i * 3] * e[0] + L[i * 3 + 1] * e[1] + L[i * 3 + 2] * e[2]; r[3 + i] = 0.0; }
    return;
  }
  double e[6];
  graph_info_edge_error<false>(G, x, k, e, nullptr, nullptr, nullptr);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) s += L[i * 6 + c] * e[c];
    r[i] = s;
  }
}

// graph_linearize_kernel for the information factors.  J = L (de/d.) row by row from L's column halves against the 3 x 3 blocks:
//   Ji row = [-(l Rt), l B - l' M],  Jj row = [l Rt, l' M],  l = L[row][0:3], l' = L[row][3:6];
// a row is stored as it completes (L is read a second time for that, after the corrector's scale is known).
template <class... Loss>
__global__ __launch_bounds__(kGraphBlock) void graph_linearize_info_kernel(GraphDev G, double huber, Loss... loss) {
  if (G.st->done) return;
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m >= G.n_factors - G.n_plain) return;
  const int k = G.n_plain + m;
  const double* __restrict__ L = G.fac_L + (size_t)m * 36;
  double* __restrict__ o = G.J + (size_t)k * kGraphJ;
  double r[6], hr;
  if (m >= G.n_einfo) {                            // information fix: Ji = (1 - t) L3, Jj = t L3 in the translation columns
    const double t = G.fac_data[(size_t)k * 9];
    double e[3];
    graph_info_fix_error(G, G.x, k, e);
#pragma unroll
    for (int i = 0; i < 3; i++) { r[i] = L[i * 3] * e[0] + L[i * 3 + 1] * e[1] + L[i * 3 + 2] * e[2]; r[3 + i] = 0.0; }
    const double s = graph_factor_scale(k, r, huber, &hr, loss...);
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
      for (int c = 0; c < 6; c++) {
        const double l = (i < 3 && c < 3) ? s * L[i * 3 + c] : 0.0;
        o[i * 6 + c] = (1.0 - t) * l; o[36 + i * 6 + c] = t * l;
      }
      o[72 + i] = s * r[i];
    }
    G.fcost[k] = hr;
    return;
  }
  double e[6], Rt[9], B[9], M[9];
  graph_info_edge_error<true>(G, G.x, k, e, Rt, B, M);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) a += L[i * 6 + c] * e[c];
    r[i] = a;
  }
  const double s = graph_factor_scale(k, r, huber, &hr, loss...);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const double l0 = s * L[i * 6], l1 = s * L[i * 6 + 1], l2 = s * L[i * 6 + 2], l3 = s * L[i * 6 + 3], l4 = s * L[i * 6 + 4], l5 = s * L[i * 6 + 5];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double a = l0 * Rt[c] + l1 * Rt[3 + c] + l2 * Rt[6 + c];
      const double b = l0 * B[c] + l1 * B[3 + c] + l2 * B[6 + c];
      const double w = l3 * M[c] + l4 * M[3 + c] + l5 * M[6 + c];
      o[i * 6 + c] = -a; o[i * 6 + 3 + c] = b - w;
      o[36 + i * 6 + c] = a; o[36 + i * 6 + 3 + c] = w;
    }
    o[72 + i] = s * r[i];
  }
  G.fcost[k] = hr;
}

// graph_cost_kernel for the information factors
template <bool kModel, class... Loss>
__global__ __launch_bounds__(kGraphBlock) void graph_cost_info_kernel(GraphDev G, const double* __restrict__ x, double huber, Loss... loss) {
  if (kModel && G.st->done) return;
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m >= G.n_factors - G.n_plain) return;
  const int k = G.n_plain + m;
  double r[6], hr;
  graph_info_residual(G, x, m, r);
  (void)graph_factor_scale(k, r, huber, &hr, loss...);
  G.fcost[k] = hr;
  if (!kModel) return;
  G.fmodel[k] = graph_model_share(G, k);
}

// msfl_graph_factor_chi2: |r|^2 of factors first .. first + n at the current poses, before the loss; writes nothing else
__global__ __launch_bounds__(kGraphBlock) void graph_chi2_kernel(GraphDev G, int first, int n, double* __restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int k = first + i;
  double r[6], sq = 0.0;
  if (k < G.n_plain) graph_factor<false>(G, G.x, k, r, nullptr, nullptr);
  else graph_info_residual(G, G.x, k - G.n_plain, r);
#pragma unroll
  for (int c = 0; c < 6; c++) sq += r[c] * r[c];
  out[i] = sq;
}

// msfl_graph_factor_weights: rho'(|r|^2) of the same factors under each one's loss; writes nothing else
template <class... Loss>
__global__ __launch_bounds__(kGraphBlock) void graph_weights_kernel(GraphDev G, int first, int n, double* __restrict__ out, double huber, Loss... loss) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int k = first + i;
  double r[6], sq = 0.0;
  if (k < G.n_plain) graph_factor<false>(G, G.x, k, r, nullptr, nullptr);
  else graph_info_residual(G, G.x, k - G.n_plain, r);
#pragma unroll
  for (int c = 0; c < 6; c++) sq += r[c] * r[c];
  out[i] = graph_factor_weight(k, sq, huber, loss...);
}

// one free node per lane: gathers its factors in adjacency order into the unscaled diagonal block, the block towards f - 1 and the gradient
__global__ __launch_bounds__(kGraphBlock) void graph_assemble_kernel(GraphDev G) {
  if (G.st->done) return;
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= G.n_free) return;
  double H[36], Lb[36], g[6];
#pragma unroll
  for (int i = 0; i < 36; i++) { H[i] = 0.0; Lb[i] = 0.0; }
#pragma unroll
  for (int i = 0; i < 6; i++) g[i] = 0.0;
  for (int e = G.adj_off[f]; e < G.adj_off[f + 1]; e++) {
    const int k = G.adj[e] >> 1, side = G.adj[e] & 1;
    const double* Jk = G.J + (size_t)k * kGraphJ;
    double Js[36];
    g6_load(Jk + 36 * side, Js);
    g6_mma<true, false>(Js, Js, H, 1.0);
    g6_mv<true, true>(Js, Jk + 72, g);
    const int fo = G.free_of[G.fac_ij[2 * k + (side ^ 1)]];
    if (fo >= 0 && fo == f - 1) {
      double Jo[36];
      g6_load(Jk + 36 * (side ^ 1), Jo);
      g6_mma<true, false>(Js, Jo, Lb, 1.0);
    }
  }
  g6_store(G.H + (size_t)f * 36, H);
  g6_store(G.Lb + (size_t)f * 36, Lb);
  const double* x = G.x + (size_t)G.node_of[f] * 7;
  double mg[6], xm[7], xx = 0.0, gm = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) { G.g[(size_t)f * 6 + i] = g[i]; mg[i] = -g[i]; }
  graph_plus(x, mg, xm);
#pragma unroll
  for (int i = 0; i < 7; i++) { xx += x[i] * x[i]; gm = fmax(gm, fabs(x[i] - xm[i])); }
  G.nxx[f] = xx; G.ngmax[f] = gm;
}

__global__ __launch_bounds__(kGraphVec) void graph_scale_kernel(GraphDev G, int jacobi) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= G.n_free * 6) return;
  const int f = i / 6, c = i - 6 * f;
  G.scale[i] = jacobi ? 1.0 / (1.0 + sqrt(G.H[(size_t)f * 36 + c * 7])) : 1.0;
}

// the top of TrustRegionMinimizer's loop: iteration 0's bookkeeping, then FinalizeIterationAndCheckIfMinimizerCanContinue
__global__ __launch_bounds__(kGraphVec) void graph_tr_begin_kernel(GraphDev G, GraphOpt o) {
  __shared__ double lds[kGraphVec];
  GraphState* s = G.st;
  if (s->done) return;
  const double xx = graph_total<kGraphVec, kGraphSum>(G.nxx, G.n_free, lds);
  const double gmax = graph_total<kGraphVec, kGraphMax>(G.ngmax, G.n_free, lds);
  const double cost = s->first ? graph_total<kGraphVec, kGraphSum>(G.fcost, G.n_factors, lds) : 0.0;
  if (threadIdx.x != 0) return;
  s->commit = 0;
  s->x_norm = sqrt(xx); s->gmax = gmax;
  if (s->first) {
    s->first = 0;
    s->cost = s->initial_cost = s->final_cost = cost;
    if (gmax <= o.gtol) { s->termination = kGraphGradient; s->done = 1; return; }
  }
  if (s->iterations >= o.max_iter) { s->termination = kGraphMaxIter; s->done = 1; return; }
  if (s->step_successful && gmax <= o.gtol) { s->termination = kGraphGradient; s->done = 1; return; }
  if (s->radius < o.radius_min) { s->termination = kGraphMinRadius; s->done = 1; return; }
  s->iterations += 1;
  s->cg_done = 0; s->cg_it = 0;
}

// level 0 of the reduction: T = the scaled blocks plus the LM diagonal; b = -(scale . g); r = b, step = 0
__global__ __launch_bounds__(kGraphVec) void graph_damp_kernel(GraphDev G, GraphOpt o) {
  if (G.st->done) return;
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= G.n_free) return;
  const double radius = G.st->radius;
  const double* s = G.scale + (size_t)f * 6;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double h = s[i] * s[j] * G.H[(size_t)f * 36 + i * 6 + j];
      if (i == j) h += fmin(fmax(h, o.lm_min), o.lm_max) / radius;
      G.D[(size_t)f * 36 + i * 6 + j] = h;
      G.L[(size_t)f * 36 + i * 6 + j] = f > 0 ? s[i] * G.scale[(size_t)(f - 1) * 6 + j] * G.Lb[(size_t)f * 36 + i * 6 + j] : 0.0;
    }
  for (int i = 0; i < 6; i++) {
    const double b = -(s[i] * G.g[(size_t)f * 6 + i]);
    G.b[(size_t)f * 6 + i] = b; G.r[(size_t)f * 6 + i] = b; G.xs[(size_t)f * 6 + i] = 0.0;
  }
}

// ---- block cyclic reduction of T x = y: level l keeps its even blocks; odd block k is x_k = D_k^-1 (y_k - L_k x_k-1 - L_k+1^T x_k+1) ----
// inverts odd block 2 j + 1 of level l; returns g6_inv_spd's pivot ratio
template <bool kPivot>
__device__ __forceinline__ double graph_cr_invert_node(const GraphDev& G, const GraphLevels& V, int l, int j) {
  const int k = V.n[l] == 1 ? 0 : 2 * j + 1;       // the last level's single block is inverted too
  double a[36];
  g6_load(G.D + (size_t)(V.off[l] + k) * 36, a);
  const double ratio = g6_inv_spd<kPivot>(a);
  g6_store(G.Dinv + (size_t)(V.ioff[l] + j) * 36, a);
  return ratio;
}
// block m of level l + 1 from block k = 2 m of level l:
//   D' = D_k - L_k Dinv_k-1 L_k^T - L_k+1^T Dinv_k+1 L_k+1,   L' = -L_k Dinv_k-1 L_k-1
__device__ __forceinline__ void graph_cr_reduce_node(const GraphDev& G, const GraphLevels& V, int l, int m) {
  const int k = 2 * m, n = V.n[l];
  const double* Dl = G.D + (size_t)V.off[l] * 36; const double* Ll = G.L + (size_t)V.off[l] * 36;
  const double* Il = G.Dinv + (size_t)V.ioff[l] * 36;
  double Dn[36], Ln[36], A[36], W[36], T[36];
  g6_load(Dl + (size_t)k * 36, Dn);
#pragma unroll
  for (int i = 0; i < 36; i++) Ln[i] = 0.0;
  if (k >= 1) {
    g6_load(Ll + (size_t)k * 36, A);
    g6_load(Il + (size_t)(m - 1) * 36, W);
#pragma unroll
    for (int i = 0; i < 36; i++) T[i] = 0.0;
    g6_mma<false, false>(A, W, T, 1.0);            // L_k Dinv_k-1
    g6_mma<false, true>(T, A, Dn, -1.0);
    if (k >= 2) {
      g6_load(Ll + (size_t)(k - 1) * 36, W);
      g6_mma<false, false>(T, W, Ln, -1.0);
    }
  }
  if (k + 1 < n) {
    g6_load(Ll + (size_t)(k + 1) * 36, A);
    g6_load(Il + (size_t)m * 36, W);
#pragma unroll
    for (int i = 0; i < 36; i++) T[i] = 0.0;
    g6_mma<true, false>(A, W, T, 1.0);             // L_k+1^T Dinv_k+1
    g6_mma<false, false>(T, A, Dn, -1.0);
  }
  g6_store(G.D + (size_t)(V.off[l + 1] + m) * 36, Dn);
  g6_store(G.L + (size_t)(V.off[l + 1] + m) * 36, Ln);
}
// right-hand side (6 x W per block) of block m of level l + 1: y' = y_k - L_k Dinv_k-1 y_k-1 - L_k+1^T Dinv_k+1 y_k+1
template <int W>
__device__ __forceinline__ void graph_cr_rhs_node(const GraphDev& G, const GraphLevels& V, int l, int m, const double* __restrict__ y,
                                                  double* __restrict__ yn) {
  const int k = 2 * m, n = V.n[l];
  const double* Ll = G.L + (size_t)V.off[l] * 36; const double* Il = G.Dinv + (size_t)V.ioff[l] * 36;
  double o[6 * W], t[6 * W];
  g6_load<6 * W>(y + (size_t)k * 6 * W, o);
  if (k >= 1) {
    g6_fresh<W, false>(Il + (size_t)(m - 1) * 36, y + (size_t)(k - 1) * 6 * W, t);
    g6_mul<W, kG6Add, false>(Ll + (size_t)k * 36, t, o, -1.0);
  }
  if (k + 1 < n) {
    g6_fresh<W, false>(Il + (size_t)m * 36, y + (size_t)(k + 1) * 6 * W, t);
    g6_mul<W, kG6Add, true>(Ll + (size_t)(k + 1) * 36, t, o, -1.0);
  }
  g6_store<6 * W>(yn + (size_t)m * 6 * W, o);
}
// solution of block k of level l from the solution xn of level l + 1 (even blocks copy, odd blocks substitute)
template <int W>
__device__ __forceinline__ void graph_cr_back_node(const GraphDev& G, const GraphLevels& V, int l, int k, const double* __restrict__ y,
                                                   const double* __restrict__ xn, double* __restrict__ x) {
  const int n = V.n[l], m = k >> 1;
  double t[6 * W], b[6 * W];
  if (!(k & 1)) {
    g6_load<6 * W>(xn + (size_t)m * 6 * W, t);
    g6_store<6 * W>(x + (size_t)k * 6 * W, t);
    return;
  }
  const double* Ll = G.L + (size_t)V.off[l] * 36; const double* Il = G.Dinv + (size_t)V.ioff[l] * 36;
  g6_load<6 * W>(y + (size_t)k * 6 * W, t);
  g6_mul<W, kG6Add, false>(Ll + (size_t)k * 36, xn + (size_t)m * 6 * W, t, -1.0);
  if (k + 1 < n) g6_mul<W, kG6Add, true>(Ll + (size_t)(k + 1) * 36, xn + (size_t)(m + 1) * 6 * W, t, -1.0);
  g6_fresh<W, false>(Il + (size_t)m * 36, t, b);
  g6_store<6 * W>(x + (size_t)k * 6 * W, b);
}

// The right-hand sides the kernels of the right-hand-side half work on: W columns, where level l lives, how many lanes the per-level
// kernels run, and when there is nothing left to do.
// The solve's one column: r -> z at level 0, levels 1.. in G.rhs / G.sol; returns with the LM loop or the CG.
struct GraphSolveCols {
  static constexpr int W = 1, kLanes = kGraphVec;
  __device__ bool done(const GraphDev& G) const { return G.st->done || G.st->cg_done; }
  __device__ double* rhs_up(const GraphDev& G, const GraphLevels& V, int l) const { return G.rhs + (size_t)V.off[l] * 6; }
  __device__ const double* rhs(const GraphDev& G, const GraphLevels& V, int l) const { return l == 0 ? G.r : rhs_up(G, V, l); }
  __device__ double* sol(const GraphDev& G, const GraphLevels& V, int l) const { return l == 0 ? G.z : G.sol + (size_t)V.off[l] * 6; }
};
// the six columns of column node c are all done
__device__ __forceinline__ bool graph_marg_all_done(const GraphMarg& M, int c) {
  int d = 1;
#pragma unroll
  for (int j = 0; j < 6; j++) d &= M.col[c * 6 + j].done;
  return d != 0;
}
// The marginals' six columns of column node blockIdx.y: y0 -> x0 at level 0 ([n_cols x free x 36]), levels 1.. in M.rhs / M.sol; returns
// when the node's six CGs are done.  64 lanes: a lane carries 6 x 6 blocks and takes 250 - 256 VGPRs.
struct GraphMargCols {
  static constexpr int W = 6, kLanes = kGraphBlock;
  GraphMarg M; const double* y0; double* x0;
  __device__ bool done(const GraphDev&) const { return graph_marg_all_done(M, (int)blockIdx.y); }
  __device__ size_t at(const GraphDev& G, const GraphLevels& V, int l) const {
    return l == 0 ? (size_t)blockIdx.y * G.n_free * 36 : ((size_t)blockIdx.y * (size_t)(V.off[V.count - 1] + 1 - G.n_free) + (size_t)(V.off[l] - G.n_free)) * 36;
  }
  __device__ double* rhs_up(const GraphDev& G, const GraphLevels& V, int l) const { return M.rhs + at(G, V, l); }
  __device__ const double* rhs(const GraphDev& G, const GraphLevels& V, int l) const { return l == 0 ? y0 + at(G, V, 0) : rhs_up(G, V, l); }
  __device__ double* sol(const GraphDev& G, const GraphLevels& V, int l) const { return (l == 0 ? x0 : M.sol) + at(G, V, l); }
};

// the factor half, once per LM iteration: invert the odd blocks of level l, then form level l + 1.  With kPivot (the marginals) the
// workgroup's smallest pivot ratio goes to M.piv[first + blockIdx.x]; without, M and first are not looked at.
template <bool kPivot>
__global__ __launch_bounds__(kGraphBlock) void graph_cr_invert_kernel(GraphDev G, GraphLevels V, int l, GraphMarg M, int first) {
  if (G.st->done) return;
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  double ratio = 1.0;
  if (j < V.n[l] / 2) ratio = graph_cr_invert_node<kPivot>(G, V, l, j);
  if constexpr (kPivot) {
    __shared__ double lds[kGraphBlock];
    ratio = graph_block_reduce<kGraphBlock, kGraphMin>(ratio, lds);
    if (threadIdx.x == 0) M.piv[first + blockIdx.x] = ratio;
  }
}
__global__ __launch_bounds__(kGraphBlock) void graph_cr_reduce_kernel(GraphDev G, GraphLevels V, int l) {
  if (G.st->done) return;
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m < V.n[l + 1]) graph_cr_reduce_node(G, V, l, m);
}
// one workgroup finishes the factor half from level V.tail on.  With kPivot it makes the pivot test: the minimum over its own blocks and
// the n_piv partials of the launches before it, into M.st.
template <bool kPivot>
__global__ __launch_bounds__(kGraphVec) void graph_cr_factor_tail_kernel(GraphDev G, GraphLevels V, GraphMarg M, int n_piv, double min_ratio) {
  if (G.st->done) return;
  double ratio = 1.0;
  for (int l = V.tail; l < V.count; l++) {
    const int inv = V.n[l] == 1 ? 1 : V.n[l] / 2;
    for (int j = (int)threadIdx.x; j < inv; j += kGraphVec) ratio = fmin(ratio, graph_cr_invert_node<kPivot>(G, V, l, j));
    __syncthreads();
    if (l + 1 < V.count)
      for (int m = (int)threadIdx.x; m < V.n[l + 1]; m += kGraphVec) graph_cr_reduce_node(G, V, l, m);
    __syncthreads();
  }
  if constexpr (kPivot) {
    __shared__ double lds[kGraphVec];
    for (int i = (int)threadIdx.x; i < n_piv; i += kGraphVec) ratio = fmin(ratio, M.piv[i]);
    ratio = graph_block_reduce<kGraphVec, kGraphMin>(ratio, lds);
    if (threadIdx.x == 0) { M.st->min_pivot = ratio; M.st->singular = ratio >= min_ratio ? 0 : 1; }
  }
}
// the right-hand-side half, once per CG iteration: x0 = T^-1 y0 for the columns of C
template <class C>
__global__ __launch_bounds__(C::kLanes) void graph_cr_rhs_kernel(GraphDev G, GraphLevels V, int l, C cols) {
  if (cols.done(G)) return;
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m < V.n[l + 1]) graph_cr_rhs_node<C::W>(G, V, l, m, cols.rhs(G, V, l), cols.rhs_up(G, V, l + 1));
}
template <class C>
__global__ __launch_bounds__(kGraphVec) void graph_cr_tail_kernel(GraphDev G, GraphLevels V, C cols) {
  constexpr int W = C::W;
  if (cols.done(G)) return;
  const int last = V.count - 1;
  for (int l = V.tail; l < last; l++) {
    for (int m = (int)threadIdx.x; m < V.n[l + 1]; m += kGraphVec) graph_cr_rhs_node<W>(G, V, l, m, cols.rhs(G, V, l), cols.rhs_up(G, V, l + 1));
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double b[6 * W], t[6 * W];
    g6_load<6 * W>(cols.rhs(G, V, last), b);
    g6_fresh<W, false>(G.Dinv + (size_t)V.ioff[last] * 36, b, t);
    g6_store<6 * W>(cols.sol(G, V, last), t);
  }
  __syncthreads();
  for (int l = last - 1; l >= V.tail; l--) {
    for (int k = (int)threadIdx.x; k < V.n[l]; k += kGraphVec)
      graph_cr_back_node<W>(G, V, l, k, cols.rhs(G, V, l), cols.sol(G, V, l + 1), cols.sol(G, V, l));
    __syncthreads();
  }
}
template <class C>
__global__ __launch_bounds__(C::kLanes) void graph_cr_back_kernel(GraphDev G, GraphLevels V, int l, C cols) {
  if (cols.done(G)) return;
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k < V.n[l]) graph_cr_back_node<C::W>(G, V, l, k, cols.rhs(G, V, l), cols.sol(G, V, l + 1), cols.sol(G, V, l));
}

// ---- PCG ---------------------------------------------------------------------------------------------------------------
// partial of r . z per workgroup
__global__ __launch_bounds__(kGraphVec) void graph_dot_kernel(GraphDev G, int n_part) {
  __shared__ double lds[kGraphVec];
  if (G.st->done || G.st->cg_done) return;
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  double s = 0.0;
  if (f < G.n_free)
    for (int i = 0; i < 6; i++) s += G.r[(size_t)f * 6 + i] * G.z[(size_t)f * 6 + i];
  s = graph_block_reduce<kGraphVec, kGraphSum>(s, lds);
  if (threadIdx.x == 0) G.part[n_part + blockIdx.x] = s;
}

// the CG direction of free node f over W columns (6 x W): column j is z + beta_j p_old, z alone in the first iteration
template <int W>
__device__ __forceinline__ void graph_cg_dir(const double* __restrict__ z, const double* __restrict__ po, int f, const double* beta, bool first, double* p) {
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < W; j++) p[i * W + j] = z[((size_t)f * 6 + i) * W + j] + (first ? 0.0 : beta[j] * po[((size_t)f * 6 + i) * W + j]);
}
// q = A p for free node f and W columns, p = graph_cg_dir (left in pf for f itself): D_f p_f + L_f p_f-1 + L_f+1^T p_f+1, then the long
// factors in adjacency order, s_f . Jf^T (Jo (s_o . p_o))
template <int W>
__device__ __forceinline__ void graph_apply(const GraphDev& G, int f, const double* z, const double* po, const double* beta, bool first, double* pf, double* q) {
  double pm[6 * W], t[6 * W];
  graph_cg_dir<W>(z, po, f, beta, first, pf);
  g6_fresh<W, false>(G.D + (size_t)f * 36, pf, q);
  if (f > 0) {
    graph_cg_dir<W>(z, po, f - 1, beta, first, pm);
    g6_accum<W, false>(G.L + (size_t)f * 36, pm, q);
  }
  if (f + 1 < G.n_free) {
    graph_cg_dir<W>(z, po, f + 1, beta, first, pm);
    g6_accum<W, true>(G.L + (size_t)(f + 1) * 36, pm, q);
  }
  const double* sf = G.scale + (size_t)f * 6;
  for (int e = G.ladj_off[f]; e < G.ladj_off[f + 1]; e++) {
    const int k = G.ladj[e] >> 1, side = G.ladj[e] & 1;
    const int fo = G.free_of[G.fac_ij[2 * k + (side ^ 1)]];
    const double* Jk = G.J + (size_t)k * kGraphJ;
    const double* so = G.scale + (size_t)fo * 6;
    graph_cg_dir<W>(z, po, fo, beta, first, pm);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < W; j++) pm[i * W + j] *= so[i];
    g6_fresh<W, false>(Jk + 36 * (side ^ 1), pm, t);
    g6_fresh<W, true>(Jk + 36 * side, t, pm);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < W; j++) q[i * W + j] += sf[i] * pm[i * W + j];
  }
}

// CG iteration `it`: the convergence test on r . z, p = z + beta p (written to p[it & 1], read from the other), q = A p, partial p . q
__global__ __launch_bounds__(kGraphVec) void graph_matvec_kernel(GraphDev G, int it, int n_part, double cg_tol, int direct) {
  __shared__ double lds[kGraphVec];
  GraphState* s = G.st;
  if (s->done || s->cg_done) return;
  const int c = it & 1;
  const double rz = graph_total<kGraphVec, kGraphSum>(G.part + n_part, n_part, lds);
  const double rz0 = it == 0 ? rz : s->rz0;
  const bool stop = it == 0 ? !(rz > 0.0) : (!direct && sqrt(rz) <= cg_tol * sqrt(rz0));
  if (stop) {
    if (blockIdx.x == 0 && threadIdx.x == 0) s->cg_done = 1;
    return;
  }
  const double beta = it == 0 ? 0.0 : rz / s->rz[c ^ 1];
  if (blockIdx.x == 0 && threadIdx.x == 0) { s->rz[c] = rz; if (it == 0) s->rz0 = rz; }
  const double* po = G.p[c ^ 1]; double* pn = G.p[c];
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  double pq = 0.0;
  if (f < G.n_free) {
    double pf[6], q[6];
    graph_apply<1>(G, f, G.z, po, &beta, it == 0, pf, q);
#pragma unroll
    for (int i = 0; i < 6; i++) { pn[(size_t)f * 6 + i] = pf[i]; G.q[(size_t)f * 6 + i] = q[i]; pq += pf[i] * q[i]; }
  }
  pq = graph_block_reduce<kGraphVec, kGraphSum>(pq, lds);
  if (threadIdx.x == 0) G.part[blockIdx.x] = pq;
}

// step += alpha p, r -= alpha q, alpha = r . z / p . q
__global__ __launch_bounds__(kGraphVec) void graph_cg_update_kernel(GraphDev G, int it, int n_part) {
  __shared__ double lds[kGraphVec];
  GraphState* s = G.st;
  if (s->done || s->cg_done) return;
  const double pq = graph_total<kGraphVec, kGraphSum>(G.part, n_part, lds);
  const double alpha = s->rz[it & 1] / pq;
  const double* p = G.p[it & 1];
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f < G.n_free)
    for (int i = 0; i < 6; i++) {
      G.xs[(size_t)f * 6 + i] += alpha * p[(size_t)f * 6 + i];
      G.r[(size_t)f * 6 + i] -= alpha * G.q[(size_t)f * 6 + i];
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) s->cg_it = it + 1;
}

// after the last enqueued iteration: a solve that has not met the tolerance hands over its iterate and is counted
__global__ __launch_bounds__(kGraphVec) void graph_cg_end_kernel(GraphDev G, int n_part, double cg_tol, int direct) {
  __shared__ double lds[kGraphVec];
  GraphState* s = G.st;
  if (s->done) return;
  const double rz = graph_total<kGraphVec, kGraphSum>(G.part + n_part, n_part, lds);
  if (threadIdx.x != 0) return;
  if (!s->cg_done && !direct && !(sqrt(rz) <= cg_tol * sqrt(s->rz0))) s->cg_unconverged += 1;
  s->cg_total += s->cg_it;
  s->cg_done = 0;
}

// candidate = Plus(x, scale . step) per free node, and |x - candidate|^2
__global__ __launch_bounds__(kGraphVec) void graph_plus_kernel(GraphDev G) {
  if (G.st->done) return;
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= G.n_free) return;
  const double* x = G.x + (size_t)G.node_of[f] * 7;
  double d[6], o[7], s = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) d[i] = G.xs[(size_t)f * 6 + i] * G.scale[(size_t)f * 6 + i];
  graph_plus(x, d, o);
#pragma unroll
  for (int i = 0; i < 7; i++) { G.cand[(size_t)G.node_of[f] * 7 + i] = o[i]; s += (x[i] - o[i]) * (x[i] - o[i]); }
  G.nstep[f] = s;
}

// the rest of one TrustRegionMinimizer iteration, in the order of tests/ceres_numpy.solve
__global__ __launch_bounds__(kGraphVec) void graph_tr_kernel(GraphDev G, GraphOpt o) {
  __shared__ double lds[kGraphVec];
  GraphState* s = G.st;
  if (s->done) return;
  const double model = graph_total<kGraphVec, kGraphSum>(G.fmodel, G.n_factors, lds);
  const double cand_cost = graph_total<kGraphVec, kGraphSum>(G.fcost, G.n_factors, lds);
  const double step2 = graph_total<kGraphVec, kGraphSum>(G.nstep, G.n_free, lds);
  if (threadIdx.x != 0) return;
  const int slot = s->n_trace++;
  const bool valid = isfinite(model) && isfinite(step2) && model > 0.0;
  if (!valid) {
    G.tr_accepted[slot] = -1; G.tr_cost[slot] = s->cost;
    s->invalid += 1;
    if (s->invalid >= o.max_invalid) { s->termination = kGraphInvalid; s->done = 1; return; }
    s->radius *= 0.5;
    s->step_successful = 0;
    return;
  }
  s->invalid = 0;
  G.tr_cost[slot] = cand_cost;
  const double step_norm = sqrt(step2);
  if (step_norm <= o.ptol * (s->x_norm + o.ptol)) { G.tr_accepted[slot] = 0; s->termination = kGraphParameter; s->done = 1; return; }
  const double change = s->cost - cand_cost;
  if (fabs(change) <= o.ftol * s->cost) { G.tr_accepted[slot] = 0; s->termination = kGraphFunction; s->done = 1; return; }
  const double rel = change / model;
  const bool ok = rel > o.min_rel;
  G.tr_accepted[slot] = ok ? 1 : 0;
  if (ok) {
    s->commit = 1;
    s->cost = s->final_cost = cand_cost;
    const double w = 2.0 * rel - 1.0;
    s->radius = fmin(s->radius / fmax(1.0 / 3.0, 1.0 - w * w * w), o.radius_max);
    s->decrease_factor = 2.0; s->step_successful = 1; s->successful += 1;
  } else {
    s->radius /= s->decrease_factor;
    s->decrease_factor *= 2.0;
    s->step_successful = 0;
  }
}

// msfl_graph_cost: the total of fcost into out[0]
__global__ __launch_bounds__(kGraphVec) void graph_cost_total_kernel(GraphDev G, double* out) {
  __shared__ double lds[kGraphVec];
  const double c = graph_total<kGraphVec, kGraphSum>(G.fcost, G.n_factors, lds);
  if (threadIdx.x == 0) out[0] = c;
}

// ---- marginals (msfl_graph_marginals; docs/kernels/graph.md, "Marginals") -----------------------------------------------------------
// Sigma = H^-1 at the current poses, H = J^T J undamped.  With the Jacobi scale S of this linearisation Hs = S H S is factored as the
// solve factors its damped T, and Hs X = E_b is solved for the six unit columns of every requested free column node b by the same PCG
// (chain part by cyclic reduction, long factors in the mat-vec); Sigma_ab = S_a X_a S_b.  blockIdx.y selects the column node, one lane
// owns one free node and carries its 6 x 6 block (row = the node's coordinate, column = which of b's six unit vectors) through the W = 6
// instances of the reduction's bodies and of graph_apply, so Dinv and L are loaded once per six columns; the factor half is the solve's
// with kPivot.  Each of the six columns is a CG of its own (GraphMargCol), so the CG kernels below are the marginals' own: sums per
// (column, workgroup) in index order; a converged column freezes; a workgroup whose six are done returns.

// level 0 of the reduction without the LM diagonal, under the Jacobi scale of this linearisation (written to G.scale for the mat-vec).
// graph_damp_kernel's two products per entry are not shared: there the scale is read from G.scale inside rolled loops with the LM term
// between them, here it is computed into registers.
__global__ __launch_bounds__(kGraphVec) void graph_marg_setup_kernel(GraphDev G) {
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= G.n_free) return;
  double s[6], sp[6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    s[c] = 1.0 / (1.0 + sqrt(G.H[(size_t)f * 36 + c * 7]));
    sp[c] = f > 0 ? 1.0 / (1.0 + sqrt(G.H[(size_t)(f - 1) * 36 + c * 7])) : 0.0;
    G.scale[(size_t)f * 6 + c] = s[c];
  }
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) {
      G.D[(size_t)f * 36 + i * 6 + j] = s[i] * s[j] * G.H[(size_t)f * 36 + i * 6 + j];
      G.L[(size_t)f * 36 + i * 6 + j] = f > 0 ? s[i] * sp[j] * G.Lb[(size_t)f * 36 + i * 6 + j] : 0.0;
    }
}

// X = 0, R = the unit columns of the column node, every column's CG record cleared
__global__ __launch_bounds__(kGraphVec) void graph_marg_init_kernel(GraphDev G, GraphMarg M) {
  const int c = (int)blockIdx.y;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < 6) { GraphMargCol z{}; M.col[c * 6 + i] = z; }
  if (i >= G.n_free * 36) return;
  const int f = i / 36, e = i - 36 * f;
  const size_t at = (size_t)c * G.n_free * 36 + i;
  M.X[at] = 0.0;
  M.R[at] = (f == M.col_free[c] && e % 7 == 0) ? 1.0 : 0.0;
}

// partials of r . z, one per (column, workgroup)
__global__ __launch_bounds__(kGraphBlock) void graph_marg_dot_kernel(GraphDev G, GraphMarg M) {
  __shared__ double lds[kGraphBlock];
  const int c = (int)blockIdx.y;
  if (graph_marg_all_done(M, c)) return;
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  double s[6] = {0, 0, 0, 0, 0, 0};
  if (f < G.n_free) {
    const double* r = M.R + ((size_t)c * G.n_free + f) * 36; const double* z = M.Z + ((size_t)c * G.n_free + f) * 36;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 6; j++) s[j] += r[i * 6 + j] * z[i * 6 + j];
  }
  double* part = M.part + (size_t)M.n_cols * 6 * M.n_part;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const double v = graph_block_reduce<kGraphBlock, kGraphSum>(s[j], lds);
    if (threadIdx.x == 0) part[(size_t)(c * 6 + j) * M.n_part + blockIdx.x] = v;
  }
}

// graph_matvec_kernel per column node: every column's convergence test on its r . z, p = z + beta p, q = A p, partials of p . q
__global__ __launch_bounds__(kGraphBlock) void graph_marg_matvec_kernel(GraphDev G, GraphMarg M, int it, double cg_tol) {
  __shared__ double lds[kGraphBlock];
  const int c = (int)blockIdx.y;
  if (graph_marg_all_done(M, c)) return;
  const int w = it & 1;
  const double* part_rz = M.part + (size_t)M.n_cols * 6 * M.n_part;
  double beta[6];
  int done[6], all = 1;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    GraphMargCol* s = M.col + c * 6 + j;
    done[j] = s->done;
    const double rz = graph_total<kGraphBlock, kGraphSum>(part_rz + (size_t)(c * 6 + j) * M.n_part, M.n_part, lds);
    const double rz0 = it == 0 ? rz : s->rz0;
    const bool stop = it == 0 ? !(rz > 0.0) : sqrt(rz) <= cg_tol * sqrt(rz0);
    beta[j] = it == 0 ? 0.0 : rz / s->rz[w ^ 1];
    if (!done[j] && blockIdx.x == 0 && threadIdx.x == 0) {
      if (stop) s->done = 1;
      else { s->rz[w] = rz; if (it == 0) s->rz0 = rz; }
    }
    done[j] |= stop ? 1 : 0;
    all &= done[j];
  }
  if (all) return;
  const size_t base = (size_t)c * G.n_free * 36;
  const double* Z = M.Z + base; const double* po = M.P[w ^ 1] + base; double* pn = M.P[w] + base; double* Q = M.Q + base;
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  double pq[6] = {0, 0, 0, 0, 0, 0};
  if (f < G.n_free) {
    double pf[36], q[36];
    graph_apply<6>(G, f, Z, po, beta, it == 0, pf, q);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 6; j++)
        if (!done[j]) {
          pn[(size_t)f * 36 + i * 6 + j] = pf[i * 6 + j]; Q[(size_t)f * 36 + i * 6 + j] = q[i * 6 + j];
          pq[j] += pf[i * 6 + j] * q[i * 6 + j];
        }
  }
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const double v = graph_block_reduce<kGraphBlock, kGraphSum>(pq[j], lds);
    if (threadIdx.x == 0) M.part[(size_t)(c * 6 + j) * M.n_part + blockIdx.x] = v;
  }
}

// x += alpha p, r -= alpha q per column that is still running
__global__ __launch_bounds__(kGraphBlock) void graph_marg_update_kernel(GraphDev G, GraphMarg M, int it) {
  __shared__ double lds[kGraphBlock];
  const int c = (int)blockIdx.y;
  if (graph_marg_all_done(M, c)) return;
  double alpha[6];
  int done[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    GraphMargCol* s = M.col + c * 6 + j;
    done[j] = s->done;
    const double pq = graph_total<kGraphBlock, kGraphSum>(M.part + (size_t)(c * 6 + j) * M.n_part, M.n_part, lds);
    alpha[j] = s->rz[it & 1] / pq;
  }
  const size_t base = (size_t)c * G.n_free * 36;
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f < G.n_free) {
    const double* p = M.P[it & 1] + base + (size_t)f * 36; const double* q = M.Q + base + (size_t)f * 36;
    double* x = M.X + base + (size_t)f * 36; double* r = M.R + base + (size_t)f * 36;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 6; j++)
        if (!done[j]) { x[i * 6 + j] += alpha[j] * p[i * 6 + j]; r[i * 6 + j] -= alpha[j] * q[i * 6 + j]; }
  }
  if (blockIdx.x == 0 && threadIdx.x < 6 && !M.col[c * 6 + threadIdx.x].done) M.col[c * 6 + threadIdx.x].it = it + 1;
}

// the end of a slice of `it` iterations: the test graph_marg_matvec_kernel would make next, so that the host's poll sees a column that
// converged in the slice's last iteration
__global__ __launch_bounds__(kGraphBlock) void graph_marg_check_kernel(GraphMarg M, int it, double cg_tol) {
  __shared__ double lds[kGraphBlock];
  const int c = (int)blockIdx.x;
  const double* part_rz = M.part + (size_t)M.n_cols * 6 * M.n_part;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    GraphMargCol* s = M.col + c * 6 + j;
    const double rz = graph_total<kGraphBlock, kGraphSum>(part_rz + (size_t)(c * 6 + j) * M.n_part, M.n_part, lds);
    if (threadIdx.x == 0 && !s->done && sqrt(rz) <= cg_tol * sqrt(s->rz0)) s->done = 1;
  }
}

// one lane per delivered entry: Sigma_ab(i, j) = s_a[i] X_a(i, j) s_b[j], rotational rows and columns doubled; a == b computes the lower
// triangle and mirrors it; a fixed end gives zeros; `singular` gives NaN.  pair_fa: free index of a (-1: fixed); pair_col: index of b
// among the column nodes (-1: fixed); this launch writes the pairs whose column lies in [col_first, col_first + M.n_cols).
__global__ __launch_bounds__(kGraphVec) void graph_marg_gather_kernel(GraphDev G, GraphMarg M, const int* __restrict__ pair_fa, const int* __restrict__ pair_col,
                                                                      int n_pairs, int col_first, int singular, double* __restrict__ out) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (idx >= n_pairs * 36) return;
  const int k = idx / 36, e = idx - 36 * k;
  int i = e / 6, j = e - 6 * (e / 6);
  const int fa = pair_fa[k], col = pair_col[k];
  if (singular) { out[idx] = __longlong_as_double(0x7ff8000000000000LL); return; }
  if (fa < 0 || col < 0) { out[idx] = 0.0; return; }
  const int c = col - col_first;
  if (c < 0 || c >= M.n_cols) return;
  const int fb = M.col_free[c];
  if (fa == fb && i < j) { const int t = i; i = j; j = t; }
  const double v = M.X[((size_t)c * G.n_free + fa) * 36 + i * 6 + j];
  const double si = G.scale[(size_t)fa * 6 + i] * (i >= 3 ? 2.0 : 1.0), sj = G.scale[(size_t)fb * 6 + j] * (j >= 3 ? 2.0 : 1.0);
  out[idx] = (v * si) * sj;
}

}  // namespace msfl
