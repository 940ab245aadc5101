// msfl_search_poses and msfl_relocalize through the C++ mirror (include/msfl/scan_matcher.hpp): MappingScanMatcher::MatchScan2Map
// makes the map resident, SearchPoses and Relocalize then look for the scan round the guess.
//   in : n_map_corner, points | n_map_surf, points | n_corner, points | n_surf, points | start[7] | guess[7] |
//        msfl_search_config (72 bytes) | capacity | n_candidates | max_dist | n_refine | min_fitness
//   out: n | n records of msfl_pose_candidate (88 bytes each) | m | m records of msfl_reloc_result (216 bytes each)
// Compiled by tests/test_gpu_search.py with plain g++; tests/cpp/Makefile does not know it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl/scan_matcher.hpp"

static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "search_check: %s\n", what); std::exit(2); } }

static void read_cloud(std::FILE* f, msfl::PointCloud<msfl::PointType>* c) {
  int n = 0;
  need(std::fread(&n, sizeof(int), 1, f) == 1 && n >= 0, "cloud size");
  c->points.resize(static_cast<std::size_t>(n));
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  need(n == 0 || std::fread(c->points.data(), 16, static_cast<std::size_t>(n), f) == static_cast<std::size_t>(n), "cloud points");
}

int main(int argc, char** argv) {
  need(argc == 3, "usage: search_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
  need(f != nullptr, "cannot open the input");
  msfl::TimestampedPointCloud<msfl::PointType> map, scan;
  read_cloud(f, map.cloud_corner_less_sharp.get());
  read_cloud(f, map.cloud_surf_less_flat.get());
  read_cloud(f, scan.cloud_corner_less_sharp.get());
  read_cloud(f, scan.cloud_surf_less_flat.get());
  std::array<double, 7> start, guess;
  msfl_search_config cfg = msfl::adapter::SearchDefaultConfig();
  static_assert(sizeof(msfl_search_config) == 72 && sizeof(msfl_pose_candidate) == 88 && sizeof(msfl_reloc_result) == 216, "record sizes");
  int capacity = 0, n_candidates = 0, n_refine = 0;
  double max_dist = 0.0, min_fitness = 0.0;
  need(std::fread(start.data(), sizeof(double), 7, f) == 7 && std::fread(guess.data(), sizeof(double), 7, f) == 7 &&
           std::fread(&cfg, sizeof(cfg), 1, f) == 1 && std::fread(&capacity, sizeof(int), 1, f) == 1 &&
           std::fread(&n_candidates, sizeof(int), 1, f) == 1 && std::fread(&max_dist, sizeof(double), 1, f) == 1 &&
           std::fread(&n_refine, sizeof(int), 1, f) == 1 && std::fread(&min_fitness, sizeof(double), 1, f) == 1, "poses / config / counts");
  std::fclose(f);

  msfl::MappingScanMatcher matcher(0);
  msfl::Rigid3d pose(start);
  need(matcher.MatchScan2Map(map, scan, false, nullptr, &pose, nullptr), "MatchScan2Map returned false");
  const std::vector<msfl_pose_candidate> cand = matcher.SearchPoses(scan, msfl::Rigid3d(guess), cfg, capacity);
  const std::vector<msfl_reloc_result> res = matcher.Relocalize(scan, msfl::Rigid3d(guess), cfg, n_candidates, max_dist, n_refine, min_fitness);

  std::FILE* o = std::fopen(argv[2], "wb");
  need(o != nullptr, "cannot open the output");
  const int n = static_cast<int>(cand.size()), m = static_cast<int>(res.size());
  std::fwrite(&n, sizeof(int), 1, o);
  if (n) std::fwrite(cand.data(), sizeof(msfl_pose_candidate), cand.size(), o);
  std::fwrite(&m, sizeof(int), 1, o);
  if (m) std::fwrite(res.data(), sizeof(msfl_reloc_result), res.size(), o);
  std::fclose(o);
  return 0;
}
