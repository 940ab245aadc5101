// Outlier rejection through the C++ mirror (include/msfl/scan_matcher.hpp): MappingScanMatcher with SetOutlierRejection, one
// LiDAR-only MatchScan2Map, then the same call after ClearOutlierRejection.
//   in : n_map_corner, points | n_map_surf, points | n_corner, points | n_surf, points | guess[7] | threshold
//   out: pose with the feature[7] | pose after ClearOutlierRejection[7] | the first call's msfl_rejection_record (56 bytes)
// Compiled by tests/test_gpu_rejection.py with plain g++; tests/cpp/Makefile does not know it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl/scan_matcher.hpp"

static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "rejection_check: %s\n", what); std::exit(2); } }

static void read_cloud(std::FILE* f, msfl::PointCloud<msfl::PointType>* c) {
  int n = 0;
  need(std::fread(&n, sizeof(int), 1, f) == 1 && n >= 0, "cloud size");
  c->points.resize(static_cast<std::size_t>(n));
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  need(n == 0 || std::fread(c->points.data(), 16, static_cast<std::size_t>(n), f) == static_cast<std::size_t>(n), "cloud points");
}

int main(int argc, char** argv) {
  need(argc == 3, "usage: rejection_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
  need(f != nullptr, "cannot open the input");
  msfl::TimestampedPointCloud<msfl::PointType> map, scan;
  read_cloud(f, map.cloud_corner_less_sharp.get());
  read_cloud(f, map.cloud_surf_less_flat.get());
  read_cloud(f, scan.cloud_corner_less_sharp.get());
  read_cloud(f, scan.cloud_surf_less_flat.get());
  std::array<double, 7> guess;
  double threshold = 0.0;
  need(std::fread(guess.data(), sizeof(double), 7, f) == 7 && std::fread(&threshold, sizeof(double), 1, f) == 1, "guess / threshold");
  std::fclose(f);

  static_assert(sizeof(msfl_rejection_record) == 56, "record layout");
  msfl::MappingScanMatcher matcher(0);
  matcher.SetOutlierRejection(MSFL_REJECT_THRESHOLD, threshold);
  msfl::Rigid3d with(guess);
  need(matcher.MatchScan2Map(map, scan, false, nullptr, &with, nullptr), "MatchScan2Map returned false");
  const msfl_rejection_record rec = matcher.last_rejection();
  matcher.ClearOutlierRejection();
  msfl::Rigid3d without(guess);
  need(matcher.MatchScan2Map(map, scan, false, nullptr, &without, nullptr), "MatchScan2Map returned false");

  std::FILE* o = std::fopen(argv[2], "wb");
  need(o != nullptr, "cannot open the output");
  const std::array<double, 7> a = with.ToVector7(), b = without.ToVector7();
  std::fwrite(a.data(), sizeof(double), 7, o);
  std::fwrite(b.data(), sizeof(double), 7, o);
  std::fwrite(&rec, sizeof(rec), 1, o);
  std::fclose(o);
  return 0;
}
