// The uncertainty output through the C++ mirror (include/msfl/scan_matcher.hpp): MappingScanMatcher with EnableUncertainty,
// one LiDAR-only MatchScan2Map, then CovarianceInParentFrame scaled by the record's sigma2.
//   in : n_map_corner, points | n_map_surf, points | n_corner, points | n_surf, points | guess[7] | min_eigenvalue
//   out: pose[7] | msfl_match_uncertainty (936 bytes) | covariance in the parent frame (36 doubles)
// Compiled by tests/test_gpu_uncertainty.py with plain g++; tests/cpp/Makefile does not know it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl/scan_matcher.hpp"

static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "uncertainty_check: %s\n", what); std::exit(2); } }

static void read_cloud(std::FILE* f, msfl::PointCloud<msfl::PointType>* c) {
  int n = 0;
  need(std::fread(&n, sizeof(int), 1, f) == 1 && n >= 0, "cloud size");
  c->points.resize(static_cast<std::size_t>(n));
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  need(n == 0 || std::fread(c->points.data(), 16, static_cast<std::size_t>(n), f) == static_cast<std::size_t>(n), "cloud points");
}

int main(int argc, char** argv) {
  need(argc == 3, "usage: uncertainty_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
  need(f != nullptr, "cannot open the input");
  msfl::TimestampedPointCloud<msfl::PointType> map, scan;
  read_cloud(f, map.cloud_corner_less_sharp.get());
  read_cloud(f, map.cloud_surf_less_flat.get());
  read_cloud(f, scan.cloud_corner_less_sharp.get());
  read_cloud(f, scan.cloud_surf_less_flat.get());
  std::array<double, 7> guess;
  double min_eigenvalue = 0.0;
  need(std::fread(guess.data(), sizeof(double), 7, f) == 7 && std::fread(&min_eigenvalue, sizeof(double), 1, f) == 1, "guess / threshold");
  std::fclose(f);

  msfl::MappingScanMatcher matcher(0);
  need(matcher.last_uncertainty().valid == 0, "a fresh matcher holds no record");
  matcher.EnableUncertainty(min_eigenvalue);
  msfl::Rigid3d pose(guess);
  need(matcher.MatchScan2Map(map, scan, false, nullptr, &pose, nullptr), "MatchScan2Map returned false");
  const msfl_match_uncertainty& u = matcher.last_uncertainty();
  double parent[36];
  msfl::CovarianceInParentFrame(pose, u, u.sigma2, parent);

  std::FILE* o = std::fopen(argv[2], "wb");
  need(o != nullptr, "cannot open the output");
  const std::array<double, 7> v = pose.ToVector7();
  std::fwrite(v.data(), sizeof(double), 7, o);
  std::fwrite(&u, sizeof(u), 1, o);
  std::fwrite(parent, sizeof(double), 36, o);
  std::fclose(o);
  return 0;
}
