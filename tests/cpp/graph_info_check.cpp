// The arithmetic behind msfl_graph_edge_from_uncertainty / msfl_graph_fix_from_covariance (msf_loam_amd/csrc/msfl_graph_host.h) under the
// host sanitizers: no GPU, no HIP.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I msf_loam_amd/csrc tests/cpp/graph_info_check.cpp -o graph_info_check
// For seeded poses and symmetric positive definite matrices with a known eigen-decomposition (H = sum lambda_k v_k v_k^T over a rotated
// orthonormal basis): L^T L = diag(R_i^T, I) H_kept diag(R_i, I) / scale for n_degenerate = 0 .. 5, the dropped rows are zero, z composed
// with pose_i gives pose_j back; for seeded covariances: L3 is upper triangular and L3^T L3 covariance = I; and every refusal (non-finite
// value, zero quaternion, scale <= 0, n_degenerate outside [0, 5], a covariance that is not symmetric positive definite) writes nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "msfl_graph_host.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static double unit() { return std::rand() / (double)RAND_MAX * 2.0 - 1.0; }

static void random_pose(double* p) {
  for (int c = 0; c < 3; c++) p[c] = 10.0 * unit();
  double n = 0.0;
  for (int c = 3; c < 7; c++) { p[c] = unit(); n += p[c] * p[c]; }
  n = std::sqrt(n);
  for (int c = 3; c < 7; c++) p[c] /= n > 0.0 ? n : 1.0;
  if (!(n > 0.0)) p[6] = 1.0;
}

// an orthonormal basis (rows) by Gram-Schmidt over random vectors
static void random_basis(int n, double* V) {
  for (int k = 0; k < n; k++) {
    double* v = V + n * k;
    double norm = 0.0;
    do {
      for (int c = 0; c < n; c++) v[c] = unit();
      for (int m = 0; m < k; m++) {
        double d = 0.0;
        for (int c = 0; c < n; c++) d += v[c] * V[n * m + c];
        for (int c = 0; c < n; c++) v[c] -= d * V[n * m + c];
      }
      norm = 0.0;
      for (int c = 0; c < n; c++) norm += v[c] * v[c];
      norm = std::sqrt(norm);
    } while (norm < 1e-3);
    for (int c = 0; c < n; c++) v[c] /= norm;
  }
}

static int check_edge(unsigned seed) {
  std::srand(seed);
  double pi[7], pj[7], lam[6], V[36], R[9];
  random_pose(pi); random_pose(pj);
  random_basis(6, V);
  lam[0] = 0.5 + std::fabs(unit());
  for (int k = 1; k < 6; k++) lam[k] = lam[k - 1] * (1.5 + std::fabs(unit()) * 20.0);      // ascending, spread like a registration's
  const double scale = 0.01 + std::fabs(unit());
  msfl::graph_host_quat_to_R(pi + 3, R);
  double big = 0.0;
  for (int nd = 0; nd <= 5; nd++) {
    double z[7], L[36];
    REQUIRE(msfl::graph_edge_from_eigen(pi, pj, lam, V, nd, scale, z, L));
    // want = D^T H_kept D / scale, D = diag(R_i, I)
    double H[36], D[36], HD[36];
    for (int a = 0; a < 36; a++) { H[a] = 0.0; D[a] = 0.0; }
    for (int k = nd; k < 6; k++)
      for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) H[6 * a + b] += lam[k] * V[6 * k + a] * V[6 * k + b];
    for (int a = 0; a < 3; a++) { D[6 * (3 + a) + 3 + a] = 1.0; for (int b = 0; b < 3; b++) D[6 * a + b] = R[3 * a + b]; }
    for (int a = 0; a < 6; a++)
      for (int b = 0; b < 6; b++) { double s = 0.0; for (int m = 0; m < 6; m++) s += H[6 * a + m] * D[6 * m + b]; HD[6 * a + b] = s; }
    for (int a = 0; a < 36; a++) big = std::fmax(big, std::fabs(H[a]) / scale);
    for (int a = 0; a < 6; a++)
      for (int b = 0; b < 6; b++) {
        double want = 0.0, got = 0.0;
        for (int m = 0; m < 6; m++) { want += D[6 * m + a] * HD[6 * m + b]; got += L[6 * m + a] * L[6 * m + b]; }
        REQUIRE(std::fabs(got - want / scale) <= 1e-12 * big);
      }
    for (int k = 0; k < nd; k++)
      for (int c = 0; c < 6; c++) REQUIRE(L[6 * k + c] == 0.0);
    // T_i z = T_j
    double Rz[3] = {R[0] * z[0] + R[1] * z[1] + R[2] * z[2], R[3] * z[0] + R[4] * z[1] + R[5] * z[2], R[6] * z[0] + R[7] * z[1] + R[8] * z[2]};
    for (int c = 0; c < 3; c++) REQUIRE(std::fabs(pi[c] + Rz[c] - pj[c]) <= 1e-13 * 40.0);
    const double* a = pi + 3; const double* b = z + 3;
    const double q[4] = {a[3] * b[0] + b[3] * a[0] + (a[1] * b[2] - a[2] * b[1]), a[3] * b[1] + b[3] * a[1] + (a[2] * b[0] - a[0] * b[2]),
                         a[3] * b[2] + b[3] * a[2] + (a[0] * b[1] - a[1] * b[0]), a[3] * b[3] - (a[0] * b[0] + a[1] * b[1] + a[2] * b[2])};
    for (int c = 0; c < 4; c++) REQUIRE(std::fabs(q[c] - pj[3 + c]) <= 1e-14);
  }
  // refusals write nothing
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double z[7], L[36];
  for (int c = 0; c < 7; c++) z[c] = -7.0;
  for (int c = 0; c < 36; c++) L[c] = -7.0;
  double bad[7];
  for (int c = 0; c < 7; c++) bad[c] = pi[c];
  bad[1] = nan;
  REQUIRE(!msfl::graph_edge_from_eigen(bad, pj, lam, V, 0, scale, z, L) && !msfl::graph_edge_from_eigen(pi, bad, lam, V, 0, scale, z, L));
  bad[1] = inf;
  REQUIRE(!msfl::graph_edge_from_eigen(bad, pj, lam, V, 0, scale, z, L));
  bad[1] = pi[1]; bad[3] = bad[4] = bad[5] = bad[6] = 0.0;
  REQUIRE(!msfl::graph_edge_from_eigen(bad, pj, lam, V, 0, scale, z, L) && !msfl::graph_edge_from_eigen(pi, bad, lam, V, 0, scale, z, L));
  REQUIRE(!msfl::graph_edge_from_eigen(pi, pj, lam, V, 6, scale, z, L) && !msfl::graph_edge_from_eigen(pi, pj, lam, V, -1, scale, z, L));
  REQUIRE(!msfl::graph_edge_from_eigen(pi, pj, lam, V, 0, 0.0, z, L) && !msfl::graph_edge_from_eigen(pi, pj, lam, V, 0, -1.0, z, L));
  REQUIRE(!msfl::graph_edge_from_eigen(pi, pj, lam, V, 0, nan, z, L) && !msfl::graph_edge_from_eigen(pi, pj, lam, V, 0, inf, z, L));
  double lb[6], Vb[36];
  for (int c = 0; c < 6; c++) lb[c] = lam[c];
  for (int c = 0; c < 36; c++) Vb[c] = V[c];
  lb[5] = nan; Vb[7] = inf;
  REQUIRE(!msfl::graph_edge_from_eigen(pi, pj, lb, V, 0, scale, z, L) && !msfl::graph_edge_from_eigen(pi, pj, lam, Vb, 0, scale, z, L));
  lb[5] = -1.0;
  REQUIRE(!msfl::graph_edge_from_eigen(pi, pj, lb, V, 0, scale, z, L));
  for (int c = 0; c < 6; c++) lb[c] = 0.0;                       // every kept eigenvalue zero: L would be all zero
  REQUIRE(!msfl::graph_edge_from_eigen(pi, pj, lb, V, 2, scale, z, L));
  for (int c = 0; c < 7; c++) REQUIRE(z[c] == -7.0);
  for (int c = 0; c < 36; c++) REQUIRE(L[c] == -7.0);
  return 0;
}

static int check_fix(unsigned seed) {
  std::srand(seed);
  double Q[9], sig[3], cov[9], L3[9];
  random_basis(3, Q);
  for (int c = 0; c < 3; c++) sig[c] = 0.005 + 0.1 * std::fabs(unit());
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double s = 0.0;
      for (int m = 0; m < 3; m++) s += Q[3 * m + a] * sig[m] * sig[m] * Q[3 * m + b];
      cov[3 * a + b] = s;
    }
  for (int a = 0; a < 3; a++)
    for (int b = a + 1; b < 3; b++) cov[3 * b + a] = cov[3 * a + b];
  REQUIRE(msfl::graph_fix_from_covariance(cov, L3));
  REQUIRE(L3[3] == 0.0 && L3[6] == 0.0 && L3[7] == 0.0 && L3[0] > 0.0 && L3[4] > 0.0 && L3[8] > 0.0);
  // (L3^T L3) cov = I, to the condition of the covariance (sigma ratios up to 21: 441) times a few roundings
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double s = 0.0;
      for (int m = 0; m < 3; m++) {
        double p = 0.0;
        for (int k = 0; k < 3; k++) p += L3[3 * k + a] * L3[3 * k + m];
        s += p * cov[3 * m + b];
      }
      REQUIRE(std::fabs(s - (a == b ? 1.0 : 0.0)) <= 1e-12);
    }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double out[9], bad[9];
  for (int c = 0; c < 9; c++) { out[c] = -7.0; bad[c] = cov[c]; }
  bad[4] = nan;
  REQUIRE(!msfl::graph_fix_from_covariance(bad, out));
  bad[4] = cov[4]; bad[1] = cov[1] + 1e-3 * cov[0];               // not symmetric
  REQUIRE(!msfl::graph_fix_from_covariance(bad, out));
  bad[1] = cov[1]; bad[8] = -cov[8];                               // indefinite
  REQUIRE(!msfl::graph_fix_from_covariance(bad, out));
  const double singular[9] = {1, 1, 0, 1, 1, 0, 0, 0, 1}, zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  REQUIRE(!msfl::graph_fix_from_covariance(singular, out) && !msfl::graph_fix_from_covariance(zero, out));
  for (int c = 0; c < 9; c++) REQUIRE(out[c] == -7.0);
  return 0;
}

int main() {
  for (unsigned seed = 1; seed <= 200; seed++)
    if (check_edge(seed) || check_fix(seed)) { std::fprintf(stderr, "seed %u\n", seed); return 1; }
  const double L0[36] = {0};
  double L1[36] = {0};
  L1[35] = 1e-300;
  if (msfl::graph_sqrt_information_ok(L0, 36) || !msfl::graph_sqrt_information_ok(L1, 36)) return 1;
  L1[3] = std::numeric_limits<double>::infinity();
  if (msfl::graph_sqrt_information_ok(L1, 36)) return 1;
  std::printf("graph info ok\n");
  return 0;
}
