// The loss records of msfl_graph_set_losses on the host (msf_loam_amd/csrc/msfl_graph_host.h: graph_loss_ok, graph_host_loss_rho) under the
// host sanitizers: no GPU, no HIP.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I msf_loam_amd/csrc tests/cpp/graph_loss_check.cpp -o graph_loss_check
// Validation: every known kind passes, kinds outside do not; a <= 0, NaN and +-inf are refused exactly on the kinds that read a.
// rho / rho' of every kind over s = 0 .. 1e6 and a = 0.1 .. 10: rho(0) = 0, rho' = 1 at s = 0, 0 < rho' <= 1, rho <= s, rho' against the
// central difference of rho, rho' not increasing in s (rho'' <= 0), the closed forms at s = b, DEFAULT equal to HUBER at huber_delta bit
// for bit and to NONE at huber_delta = 0, and the DBL_MIN clamp at s = 1e300 and at s = +inf.
#include <cmath>
#include <cstdio>
#include <limits>

#include "msfl_graph_host.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using namespace msfl;

static int check_validation() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double bad[] = {0.0, -0.0, -1.0, nan, inf, -inf};
  for (int kind = -2; kind <= kGraphLossKinds + 1; kind++) {
    const bool known = kind >= 0 && kind < kGraphLossKinds;
    REQUIRE(graph_loss_ok(kind, 1.0) == known);
    REQUIRE(graph_loss_ok(kind, 1e-300) == known && graph_loss_ok(kind, 1e300) == known);
    for (double a : bad) REQUIRE(graph_loss_ok(kind, a) == (known && kind < kGraphLossHuber));
  }
  return 0;
}

static int check_kind(int kind, double a) {
  const double b = a * a;
  double w0 = 0.0, w = 0.0, prev = 1.0;
  REQUIRE(graph_host_loss_rho(0.0, kind, a, 1.0, &w0) == 0.0 && w0 == 1.0);
  for (int i = 0; i <= 600; i++) {
    const double s = i == 0 ? 0.0 : std::pow(10.0, -4.0 + i / 60.0);           // 0, then 1e-4 .. 1e6
    const double rho = graph_host_loss_rho(s, kind, a, 1.0, &w);
    REQUIRE(w > 0.0 && w <= 1.0 && rho <= s * (1.0 + 1e-15) && rho >= 0.0);
    REQUIRE(w <= prev * (1.0 + 1e-15));                                          // rho'' <= 0
    prev = w;
    if (s > 0.0 && !(kind == kGraphLossHuber && std::fabs(s - b) <= 2e-3 * b)) { // Huber's rho' has its kink at s = b
      // h = 1e-3 s: truncation rho''' h^2 / 6 <= 1e-6 rho' for these forms, rounding eps rho / h ~ 1e-13 / rho'
      const double h = 1e-3 * s;
      double t;
      const double num = (graph_host_loss_rho(s + h, kind, a, 1.0, &t) - graph_host_loss_rho(s - h, kind, a, 1.0, &t)) / (2.0 * h);
      REQUIRE(std::fabs(num - w) <= 2e-6 * w + 1e-9);
    }
  }
  const double rho_b = graph_host_loss_rho(b, kind, a, 1.0, &w);
  if (kind == kGraphLossNone) REQUIRE(rho_b == b && w == 1.0);
  if (kind == kGraphLossHuber) REQUIRE(rho_b == b && w == 1.0);
  if (kind == kGraphLossSoftLOne) REQUIRE(std::fabs(rho_b - 2.0 * b * (std::sqrt(2.0) - 1.0)) <= 1e-15 * b * 4 && std::fabs(w - std::sqrt(0.5)) <= 1e-15);
  if (kind == kGraphLossCauchy) REQUIRE(std::fabs(rho_b - b * std::log(2.0)) <= 1e-15 * b && std::fabs(w - 0.5) <= 1e-15);
  if (kind == kGraphLossGemanMcClure) REQUIRE(std::fabs(rho_b - 0.5 * b) <= 1e-15 * b && std::fabs(w - 0.25) <= 1e-15);
  // far out: finite, and never below DBL_MIN
  const double inf = std::numeric_limits<double>::infinity();
  for (double s : {1e300, inf}) {
    (void)graph_host_loss_rho(s, kind, a, 1.0, &w);
    REQUIRE(w >= kGraphDblMin && w <= 1.0);
    if (kind >= kGraphLossSoftLOne && s == inf) REQUIRE(w == kGraphDblMin);
  }
  return 0;
}

int main() {
  if (check_validation()) return 1;
  for (int kind = kGraphLossNone; kind < kGraphLossKinds; kind++)
    for (double a : {0.1, 0.5, 1.0, 3.0, 10.0})
      if (check_kind(kind, a)) { std::fprintf(stderr, "kind %d a %g\n", kind, a); return 1; }
  // DEFAULT is HuberLoss(huber_delta), bit for bit, and no loss at huber_delta = 0; its own `a` is not read
  for (double s : {0.0, 0.3, 1.0, 1.0000001, 7.0, 4.5e3}) {
    double wd, wh, wn;
    for (double huber : {0.5, 1.0, 2.0}) {
      const double rd = graph_host_loss_rho(s, kGraphLossDefault, -7.0, huber, &wd), rh = graph_host_loss_rho(s, kGraphLossHuber, huber, 123.0, &wh);
      if (rd != rh || wd != wh) return 1;
    }
    const double rd = graph_host_loss_rho(s, kGraphLossDefault, -7.0, 0.0, &wd), rn = graph_host_loss_rho(s, kGraphLossNone, -7.0, 1.0, &wn);
    if (rd != rn || wd != wn || rn != s || wn != 1.0) return 1;
  }
  std::printf("graph loss ok\n");
  return 0;
}
