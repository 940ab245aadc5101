// The pose prior through the C++ mirror (include/msfl/scan_matcher.hpp): MappingScanMatcher with SetPosePrior, one LiDAR-only
// MatchScan2Map, then the same call after ClearPosePrior; SqrtInformationFromCovariance on a given covariance.
//   in : n_map_corner, points | n_map_surf, points | n_corner, points | n_surf, points | guess[7] | prior mean[7] |
//        sqrt_information[36] | covariance[36]
//   out: pose with the prior[7] | pose after ClearPosePrior[7] | SqrtInformationFromCovariance(covariance)[36]
// Compiled by tests/test_gpu_pose_prior.py with plain g++; tests/cpp/Makefile does not know it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl/scan_matcher.hpp"

static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "prior_check: %s\n", what); std::exit(2); } }

static void read_cloud(std::FILE* f, msfl::PointCloud<msfl::PointType>* c) {
  int n = 0;
  need(std::fread(&n, sizeof(int), 1, f) == 1 && n >= 0, "cloud size");
  c->points.resize(static_cast<std::size_t>(n));
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  need(n == 0 || std::fread(c->points.data(), 16, static_cast<std::size_t>(n), f) == static_cast<std::size_t>(n), "cloud points");
}

int main(int argc, char** argv) {
  need(argc == 3, "usage: prior_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
  need(f != nullptr, "cannot open the input");
  msfl::TimestampedPointCloud<msfl::PointType> map, scan;
  read_cloud(f, map.cloud_corner_less_sharp.get());
  read_cloud(f, map.cloud_surf_less_flat.get());
  read_cloud(f, scan.cloud_corner_less_sharp.get());
  read_cloud(f, scan.cloud_surf_less_flat.get());
  std::array<double, 7> guess, mean;
  msfl::Matrix6d sqrt_information, covariance;
  need(std::fread(guess.data(), sizeof(double), 7, f) == 7 && std::fread(mean.data(), sizeof(double), 7, f) == 7, "guess / mean");
  need(std::fread(sqrt_information.data(), sizeof(double), 36, f) == 36 && std::fread(covariance.data(), sizeof(double), 36, f) == 36, "matrices");
  std::fclose(f);

  msfl::MappingScanMatcher matcher(0);
  matcher.SetPosePrior(msfl::Rigid3d(mean), sqrt_information);
  msfl::Rigid3d with_prior(guess);
  need(matcher.MatchScan2Map(map, scan, false, nullptr, &with_prior, nullptr), "MatchScan2Map returned false");
  matcher.ClearPosePrior();
  msfl::Rigid3d without(guess);
  need(matcher.MatchScan2Map(map, scan, false, nullptr, &without, nullptr), "MatchScan2Map returned false");
  const msfl::Matrix6d L = msfl::SqrtInformationFromCovariance(covariance);

  std::FILE* o = std::fopen(argv[2], "wb");
  need(o != nullptr, "cannot open the output");
  const std::array<double, 7> a = with_prior.ToVector7(), b = without.ToVector7();
  std::fwrite(a.data(), sizeof(double), 7, o);
  std::fwrite(b.data(), sizeof(double), 7, o);
  std::fwrite(L.data(), sizeof(double), 36, o);
  std::fclose(o);
  return 0;
}
