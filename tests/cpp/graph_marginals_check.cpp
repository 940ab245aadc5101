// Host arithmetic of msfl_graph_relative_covariance (msfl_graph_host.h) as a stand-alone program: tests/test_graph_marginals_model.py
// builds it with -fsanitize=address,undefined and compares what it prints with the numpy model.
//   graph_marginals_check <in.bin>     in.bin: n (int32, padded to 8 bytes), then per record pose_a[7] pose_b[7] S_aa[36] S_ab[36] S_bb[36]
// Prints 36 values per record ("%.17g"), then checks that every refusal leaves `out` untouched and prints "graph marginals ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "msfl_graph_host.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  long long n = 0;
  if (std::fread(&n, sizeof(n), 1, f) != 1 || n < 1 || n > 1000) return 2;
  std::vector<double> rec((size_t)n * 122);
  if (std::fread(rec.data(), sizeof(double), rec.size(), f) != rec.size()) return 2;
  std::fclose(f);
  for (long long k = 0; k < n; k++) {
    const double* r = rec.data() + 122 * k;
    double out[36];
    if (!msfl::graph_relative_covariance(r, r + 7, r + 14, r + 50, r + 86, out)) { std::printf("record %lld refused\n", k); return 1; }
    for (int i = 0; i < 36; i++) std::printf("%.17g%c", out[i], i == 35 ? '\n' : ' ');
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++)
        if (out[6 * i + j] != out[6 * j + i]) { std::printf("record %lld is not symmetric\n", k); return 1; }
  }
  // refusals: a non-finite value anywhere, a zero quaternion
  const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
  double mark[36], out[36];
  for (int i = 0; i < 36; i++) mark[i] = 1000.0 + i;
  int refused = 0;
  for (int at = 0; at < 122; at += 5)
    for (double b : bad) {
      std::vector<double> r(rec.begin(), rec.begin() + 122);
      r[at] = b;
      std::memcpy(out, mark, sizeof(out));
      if (msfl::graph_relative_covariance(r.data(), r.data() + 7, r.data() + 14, r.data() + 50, r.data() + 86, out)) { std::printf("accepted a non-finite input at %d\n", at); return 1; }
      if (std::memcmp(out, mark, sizeof(out)) != 0) { std::printf("a refusal wrote to out\n"); return 1; }
      refused++;
    }
  for (int side = 0; side < 2; side++) {
    std::vector<double> r(rec.begin(), rec.begin() + 122);
    for (int c = 3; c < 7; c++) r[7 * side + c] = 0.0;
    std::memcpy(out, mark, sizeof(out));
    if (msfl::graph_relative_covariance(r.data(), r.data() + 7, r.data() + 14, r.data() + 50, r.data() + 86, out) || std::memcmp(out, mark, sizeof(out)) != 0) {
      std::printf("a zero quaternion was accepted or out was written\n");
      return 1;
    }
    refused++;
  }
  std::printf("graph marginals ok (%d refusals)\n", refused);
  return 0;
}
