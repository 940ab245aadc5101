// Host-side bookkeeping of the pose graph (msfl_api_graph.inc): free-node numbering, adjacency lists, long / chain classification and
// the level sizes of the cyclic reduction, and the arithmetic that turns a registration's eigen-decomposition or a 3 x 3 covariance
// into an information factor, or a joint marginal into the covariance of a relative pose, and the validation and rho / rho' of a
// factor's loss record.  Plain C++ over plain arrays, no HIP: tests/cpp/graph_structure_check.cpp, tests/cpp/graph_info_check.cpp,
// tests/cpp/graph_marginals_check.cpp and tests/cpp/graph_loss_check.cpp run it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace msfl {

constexpr int kGraphTail = 1024;     // blocks the one-workgroup tail of the cyclic reduction takes over
constexpr int kGraphMaxLevels = 32;

struct GraphLevels {                 // cyclic reduction: level l has n[l] blocks; off / ioff: where its D, L (rhs, sol) / D^-1 start
  int count, tail;                   // levels; first level the one-workgroup tail owns (n[tail] <= kGraphTail)
  int n[kGraphMaxLevels], off[kGraphMaxLevels], ioff[kGraphMaxLevels];
};

struct GraphStructure {
  int n_free = 0, n_long = 0;
  std::vector<int> free_of, node_of, adj_off, adj, ladj_off, ladj, fac_ij;
};

// factor k (edges, fixes, information edges, information fixes) joins nodes ij[2k], ij[2k + 1]; adjacency per free node in factor order; a factor is long when both
// ends are free and more than one apart in the free numbering
inline void graph_build_structure(int n_nodes, const unsigned char* fixed, const std::vector<int>& ij, GraphStructure* s) {
  const int nf = (int)(ij.size() / 2);
  s->free_of.assign((size_t)n_nodes, -1); s->node_of.clear();
  for (int i = 0; i < n_nodes; i++)
    if (!fixed[i]) { s->free_of[i] = (int)s->node_of.size(); s->node_of.push_back(i); }
  s->n_free = (int)s->node_of.size(); s->n_long = 0;
  s->fac_ij = ij;
  s->adj_off.assign((size_t)s->n_free + 1, 0); s->ladj_off.assign((size_t)s->n_free + 1, 0);
  std::vector<unsigned char> is_long((size_t)nf, 0);
  for (int k = 0; k < nf; k++) {
    const int a = s->free_of[ij[2 * k]], b = s->free_of[ij[2 * k + 1]];
    is_long[k] = a >= 0 && b >= 0 && std::abs(a - b) > 1;
    s->n_long += is_long[k];
    for (int f : {a, b})
      if (f >= 0) { s->adj_off[f + 1]++; s->ladj_off[f + 1] += is_long[k]; }
  }
  for (int f = 0; f < s->n_free; f++) { s->adj_off[f + 1] += s->adj_off[f]; s->ladj_off[f + 1] += s->ladj_off[f]; }
  s->adj.assign((size_t)s->adj_off[s->n_free], 0); s->ladj.assign((size_t)s->ladj_off[s->n_free], 0);
  std::vector<int> at(s->adj_off.begin(), s->adj_off.end() - 1), lat(s->ladj_off.begin(), s->ladj_off.end() - 1);
  for (int k = 0; k < nf; k++)
    for (int side = 0; side < 2; side++) {
      const int f = s->free_of[ij[2 * k + side]];
      if (f < 0) continue;
      s->adj[at[f]++] = 2 * k + side;
      if (is_long[k]) s->ladj[lat[f]++] = 2 * k + side;
    }
}

// level sizes of the cyclic reduction over n blocks, any n >= 1: halve (rounding up) down to one block
inline GraphLevels graph_levels(int n) {
  GraphLevels v{};
  int off = 0, ioff = 0;
  v.tail = -1;
  for (;;) {
    v.n[v.count] = n; v.off[v.count] = off; v.ioff[v.count] = ioff;
    if (v.tail < 0 && n <= kGraphTail) v.tail = v.count;
    v.count++;
    off += n; ioff += std::max(1, n / 2);
    if (n == 1) break;
    n = (n + 1) / 2;
  }
  return v;
}

// ---- information factors: the arithmetic of msfl_graph_edge_from_uncertainty / msfl_graph_fix_from_covariance ----------------
inline bool graph_all_finite(const double* v, int n) {
  for (int k = 0; k < n; k++)
    if (!(v[k] - v[k] == 0.0)) return false;          // NaN and +-inf fail
  return true;
}
// a square-root information matrix the graph accepts: finite, not all zero (any rank but zero)
inline bool graph_sqrt_information_ok(const double* L, int n) {
  if (!graph_all_finite(L, n)) return false;
  for (int k = 0; k < n; k++)
    if (L[k] != 0.0) return true;
  return false;
}
inline void graph_host_quat_to_R(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
// z = T_i^-1 T_j for poses [t, qx qy qz qw] with unit quaternions
inline void graph_host_relative_pose(const double* pi, const double* pj, double* z) {
  const double a[4] = {-pi[3], -pi[4], -pi[5], pi[6]}, b[4] = {pj[3], pj[4], pj[5], pj[6]};
  const double v[3] = {pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]};
  const double c0 = a[1] * v[2] - a[2] * v[1], c1 = a[2] * v[0] - a[0] * v[2], c2 = a[0] * v[1] - a[1] * v[0];
  z[0] = v[0] + 2.0 * (a[3] * c0 + (a[1] * c2 - a[2] * c1));
  z[1] = v[1] + 2.0 * (a[3] * c1 + (a[2] * c0 - a[0] * c2));
  z[2] = v[2] + 2.0 * (a[3] * c2 + (a[0] * c1 - a[1] * c0));
  z[3] = a[3] * b[0] + b[3] * a[0] + (a[1] * b[2] - a[2] * b[1]);
  z[4] = a[3] * b[1] + b[3] * a[1] + (a[2] * b[0] - a[0] * b[2]);
  z[5] = a[3] * b[2] + b[3] * a[2] + (a[0] * b[1] - a[1] * b[0]);
  z[6] = a[3] * b[3] - (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}
// The edge a registration gives.  `eigenvalues` (ascending) / `eigenvectors` (row k = eigenvector k) decompose the information H of
// pose_j in the tangent [dt (parent frame) ; dtheta (body frame)]; the first n_degenerate pairs are dropped.  z = T_i^-1 T_j, and row k
// of L is sqrt(lambda_k / scale) v_k^T diag(R_i, I), so that L^T L = diag(R_i^T, I) H_kept diag(R_i, I) / scale in the tangent of z.
// false (nothing written): a non-finite input, a zero quaternion, scale <= 0, n_degenerate outside [0, 5], a kept eigenvalue < 0, or
// an L that came out all zero.
inline bool graph_edge_from_eigen(const double* pose_i, const double* pose_j, const double* eigenvalues, const double* eigenvectors,
                                  int n_degenerate, double scale, double* z, double* L) {
  if (!graph_all_finite(pose_i, 7) || !graph_all_finite(pose_j, 7) || !graph_all_finite(eigenvalues, 6) || !graph_all_finite(eigenvectors, 36) ||
      !graph_all_finite(&scale, 1) || !(scale > 0.0) || n_degenerate < 0 || n_degenerate > 5)
    return false;
  if (!(pose_i[3] * pose_i[3] + pose_i[4] * pose_i[4] + pose_i[5] * pose_i[5] + pose_i[6] * pose_i[6] > 0.0) ||
      !(pose_j[3] * pose_j[3] + pose_j[4] * pose_j[4] + pose_j[5] * pose_j[5] + pose_j[6] * pose_j[6] > 0.0))
    return false;
  double R[9], zz[7], LL[36];
  graph_host_quat_to_R(pose_i + 3, R);
  graph_host_relative_pose(pose_i, pose_j, zz);
  for (int k = 0; k < 6; k++) {
    const double* v = eigenvectors + 6 * k;
    if (k < n_degenerate) {
      for (int c = 0; c < 6; c++) LL[6 * k + c] = 0.0;
      continue;
    }
    if (eigenvalues[k] < 0.0) return false;
    const double s = std::sqrt(eigenvalues[k] / scale);
    for (int c = 0; c < 3; c++) {
      LL[6 * k + c] = s * (v[0] * R[c] + v[1] * R[3 + c] + v[2] * R[6 + c]);
      LL[6 * k + 3 + c] = s * v[3 + c];
    }
  }
  if (!graph_sqrt_information_ok(LL, 36) || !graph_all_finite(zz, 7)) return false;
  std::copy(zz, zz + 7, z);
  std::copy(LL, LL + 36, L);
  return true;
}
// L3 = the upper Cholesky factor of covariance^-1 (L3^T L3 = covariance^-1).  false (nothing written) for a covariance that is not
// finite, not symmetric (beyond 1e-12 of its largest entry) or not positive definite.
inline bool graph_fix_from_covariance(const double* cov, double* L3) {
  if (!graph_all_finite(cov, 9)) return false;
  double big = 0.0;
  for (int k = 0; k < 9; k++) big = std::max(big, std::fabs(cov[k]));
  double c[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      if (std::fabs(cov[3 * i + j] - cov[3 * j + i]) > 1e-12 * big) return false;
      c[3 * i + j] = 0.5 * (cov[3 * i + j] + cov[3 * j + i]);
    }
  // covariance = C C^T, C lower; W = C^-1; P = covariance^-1 = W^T W; P = G G^T, G lower; L3 = G^T
  double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int stage = 0; stage < 2; stage++) {
    double* a = c;
    for (int j = 0; j < 3; j++) {
      double d = a[3 * j + j];
      for (int k = 0; k < j; k++) d -= C[3 * j + k] * C[3 * j + k];
      if (!(d > 0.0) || !graph_all_finite(&d, 1)) return false;
      d = std::sqrt(d);
      C[3 * j + j] = d;
      for (int i = j + 1; i < 3; i++) {
        double s = a[3 * i + j];
        for (int k = 0; k < j; k++) s -= C[3 * i + k] * C[3 * j + k];
        C[3 * i + j] = s / d;
      }
    }
    if (stage == 1) break;
    double W[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 3; j++) {
      W[3 * j + j] = 1.0 / C[3 * j + j];
      for (int i = j + 1; i < 3; i++) {
        double s = 0.0;
        for (int k = j; k < i; k++) s -= C[3 * i + k] * W[3 * k + j];
        W[3 * i + j] = s / C[3 * i + i];
      }
    }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s += W[3 * k + i] * W[3 * k + j];
        c[3 * i + j] = s;
      }
    for (int k = 0; k < 9; k++) C[k] = 0.0;
  }
  double out[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) out[3 * i + j] = C[3 * j + i];
  if (!graph_all_finite(out, 9)) return false;
  std::copy(out, out + 9, L3);
  return true;
}

// ---- a loss per factor: the records of msfl_graph_set_losses (MSFL_GRAPH_LOSS_*, the same numbers) ------------------------------
enum { kGraphLossDefault = 0, kGraphLossNone, kGraphLossHuber, kGraphLossSoftLOne, kGraphLossCauchy, kGraphLossGemanMcClure, kGraphLossKinds };
constexpr double kGraphDblMin = 2.2250738585072014e-308;
// a record the graph accepts: a known kind, and on a kind that reads `a` a finite a > 0
inline bool graph_loss_ok(int kind, double a) {
  if (kind < 0 || kind >= kGraphLossKinds) return false;
  return kind < kGraphLossHuber || (graph_all_finite(&a, 1) && a > 0.0);
}
// rho(s) and rho'(s) (clamped from below at DBL_MIN) at s = |r|^2, b = a^2.  DEFAULT is HuberLoss(huber), no loss when huber <= 0.
// The device's graph_loss_rho (msfl_graph.cuh) is this function operation for operation.
inline double graph_host_loss_rho(double s, int kind, double a, double huber, double* rho1) {
  if (kind == kGraphLossDefault) { kind = huber > 0.0 ? kGraphLossHuber : kGraphLossNone; a = huber; }
  const double b = a * a;
  double rho = s, w = 1.0;
  if (kind == kGraphLossHuber) {
    if (s > b) { const double n = std::sqrt(s); rho = 2.0 * a * n - b; w = a / n; }
  } else if (kind == kGraphLossSoftLOne) {
    const double t = std::sqrt(1.0 + s / b);
    rho = 2.0 * b * (t - 1.0); w = 1.0 / t;
  } else if (kind == kGraphLossCauchy) {
    const double q = 1.0 + s / b;
    rho = b * std::log(q); w = 1.0 / q;
  } else if (kind == kGraphLossGemanMcClure) {
    const double q = b / (b + s);
    rho = q * s; w = q * q;
  }
  *rho1 = std::max(kGraphDblMin, w);
  return rho;
}

// ---- marginals: the arithmetic of msfl_graph_relative_covariance ---------------------------------------------------------------
// Covariance of T_ab = T_a^-1 T_b in the tangent of an information edge (z.t + dt, z.q (x) dq(dtheta)) from the joint marginal of a and
// b in the delivered coordinates [dt ; dtheta], both world frame, rotation on the left.  With u = t_b - t_a:
//   J_a = [-R_a^T  R_a^T [u]x ; 0  -R_b^T],   J_b = [R_a^T  0 ; 0  R_b^T],   out = [J_a J_b] [S_aa S_ab; S_ab^T S_bb] [J_a J_b]^T,
// symmetrised.  false (nothing written): a non-finite input or a zero quaternion.
inline bool graph_relative_covariance(const double* pose_a, const double* pose_b, const double* Saa, const double* Sab, const double* Sbb,
                                      double* out) {
  if (!graph_all_finite(pose_a, 7) || !graph_all_finite(pose_b, 7) || !graph_all_finite(Saa, 36) || !graph_all_finite(Sab, 36) ||
      !graph_all_finite(Sbb, 36))
    return false;
  double qa[4], qb[4];
  for (int side = 0; side < 2; side++) {
    const double* p = side ? pose_b : pose_a;
    const double n = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]);
    if (!(n > 0.0) || !graph_all_finite(&n, 1)) return false;
    for (int c = 0; c < 4; c++) (side ? qb : qa)[c] = p[3 + c] / n;
  }
  double Ra[9], Rb[9];
  graph_host_quat_to_R(qa, Ra);
  graph_host_quat_to_R(qb, Rb);
  const double u[3] = {pose_b[0] - pose_a[0], pose_b[1] - pose_a[1], pose_b[2] - pose_a[2]};
  const double ux[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
  double J[6][12], S[12][12];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 12; j++) J[i][j] = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double b = 0.0;
      for (int m = 0; m < 3; m++) b += Ra[3 * m + i] * ux[3 * m + j];      // R_a^T [u]x
      J[i][j] = -Ra[3 * j + i]; J[i][3 + j] = b; J[3 + i][3 + j] = -Rb[3 * j + i];
      J[i][6 + j] = Ra[3 * j + i]; J[3 + i][9 + j] = Rb[3 * j + i];
    }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      S[i][j] = Saa[6 * i + j]; S[i][6 + j] = Sab[6 * i + j]; S[6 + j][i] = Sab[6 * i + j]; S[6 + i][6 + j] = Sbb[6 * i + j];
    }
  double JS[6][12], C[36];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 12; j++) {
      double s = 0.0;
      for (int m = 0; m < 12; m++) s += J[i][m] * S[m][j];
      JS[i][j] = s;
    }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
      for (int m = 0; m < 12; m++) s += JS[i][m] * J[j][m];
      C[6 * i + j] = s;
    }
  double sym[36];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) sym[6 * i + j] = 0.5 * (C[6 * i + j] + C[6 * j + i]);
  if (!graph_all_finite(sym, 36)) return false;
  std::copy(sym, sym + 36, out);
  return true;
}

}  // namespace msfl
