// msfl_search_pairs through the C++ mirror (include/msfl/scan_matcher.hpp): MappingScanMatcher::SetPairMaps makes the P maps
// resident, SearchPairs then looks for scan p round guess p in map p.
//   in : P | per pair: n_map_corner, points | n_map_surf, points | n_corner, points | n_surf, points | guess[7] |
//        then msfl_search_config (72 bytes) | capacity
//   out: per pair: n | n records of msfl_pose_candidate (88 bytes each)
// Compiled by tests/test_gpu_search_pairs.py with plain g++; tests/cpp/Makefile does not know it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl/scan_matcher.hpp"

static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "search_pairs_check: %s\n", what); std::exit(2); } }

static void read_cloud(std::FILE* f, msfl::PointCloud<msfl::PointType>* c) {
  int n = 0;
  need(std::fread(&n, sizeof(int), 1, f) == 1 && n >= 0, "cloud size");
  c->points.resize(static_cast<std::size_t>(n));
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  need(n == 0 || std::fread(c->points.data(), 16, static_cast<std::size_t>(n), f) == static_cast<std::size_t>(n), "cloud points");
}

int main(int argc, char** argv) {
  need(argc == 3, "usage: search_pairs_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
  need(f != nullptr, "cannot open the input");
  int P = 0;
  need(std::fread(&P, sizeof(int), 1, f) == 1 && P >= 0, "pair count");
  std::vector<msfl::TimestampedPointCloud<msfl::PointType>> maps(static_cast<std::size_t>(P)), scans(static_cast<std::size_t>(P));
  std::vector<msfl::Rigid3d> guesses;
  for (int p = 0; p < P; ++p) {
    read_cloud(f, maps[p].cloud_corner_less_sharp.get());
    read_cloud(f, maps[p].cloud_surf_less_flat.get());
    read_cloud(f, scans[p].cloud_corner_less_sharp.get());
    read_cloud(f, scans[p].cloud_surf_less_flat.get());
    std::array<double, 7> g;
    need(std::fread(g.data(), sizeof(double), 7, f) == 7, "guess");
    guesses.push_back(msfl::Rigid3d(g));
  }
  msfl_search_config cfg = msfl::adapter::SearchDefaultConfig();
  static_assert(sizeof(msfl_search_config) == 72 && sizeof(msfl_pose_candidate) == 88, "record sizes");
  int capacity = 0;
  need(std::fread(&cfg, sizeof(cfg), 1, f) == 1 && std::fread(&capacity, sizeof(int), 1, f) == 1, "config / capacity");
  std::fclose(f);

  msfl::MappingScanMatcher matcher(0);
  matcher.SetPairMaps(maps);
  const std::vector<std::vector<msfl_pose_candidate>> cand = matcher.SearchPairs(scans, guesses, cfg, capacity);
  need(static_cast<int>(cand.size()) == P, "one candidate list per pair");

  std::FILE* o = std::fopen(argv[2], "wb");
  need(o != nullptr, "cannot open the output");
  for (int p = 0; p < P; ++p) {
    const int n = static_cast<int>(cand[p].size());
    std::fwrite(&n, sizeof(int), 1, o);
    if (n) std::fwrite(cand[p].data(), sizeof(msfl_pose_candidate), cand[p].size(), o);
  }
  std::fclose(o);
  return 0;
}
