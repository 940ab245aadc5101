// The resident pair maps through the C++ mirror (include/msfl/scan_matcher.hpp): MappingScanMatcher::SetPairMaps indexes the P maps,
// ScorePairs grades every scan at its hypotheses, MatchPairsResident registers every scan from its guess, ScorePairs then grades the
// results on the same index.
//   in : n_pairs | per pair: n_map_corner, points | n_map_surf, points | n_corner, points | n_surf, points | guess[7] | n_poses | poses[7 n]
//      | max_dist
//   out: the records of all hypotheses in pair order (32 bytes each) | per pair: status (int) | per pair: pose[7] | per pair: the
//        record of its registered pose
// Compiled by tests/test_score_pairs_model.py (compile only) and tests/test_gpu_score_pairs.py with plain g++; tests/cpp/Makefile does
// not know it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl/scan_matcher.hpp"

static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "score_pairs_check: %s\n", what); std::exit(2); } }

static void read_cloud(std::FILE* f, msfl::PointCloud<msfl::PointType>* c) {
  int n = 0;
  need(std::fread(&n, sizeof(int), 1, f) == 1 && n >= 0, "cloud size");
  c->points.resize(static_cast<std::size_t>(n));
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  need(n == 0 || std::fread(c->points.data(), 16, static_cast<std::size_t>(n), f) == static_cast<std::size_t>(n), "cloud points");
}

int main(int argc, char** argv) {
  need(argc == 3, "usage: score_pairs_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
  need(f != nullptr, "cannot open the input");
  int n_pairs = 0;
  need(std::fread(&n_pairs, sizeof(int), 1, f) == 1 && n_pairs >= 0, "n_pairs");
  std::vector<msfl::TimestampedPointCloud<msfl::PointType>> maps(static_cast<std::size_t>(n_pairs)), scans(static_cast<std::size_t>(n_pairs));
  std::vector<msfl::Rigid3d> guesses;
  std::vector<std::vector<msfl::Rigid3d>> poses(static_cast<std::size_t>(n_pairs));
  for (int p = 0; p < n_pairs; ++p) {
    read_cloud(f, maps[p].cloud_corner_less_sharp.get());
    read_cloud(f, maps[p].cloud_surf_less_flat.get());
    read_cloud(f, scans[p].cloud_corner_less_sharp.get());
    read_cloud(f, scans[p].cloud_surf_less_flat.get());
    std::array<double, 7> v;
    int n_poses = 0;
    need(std::fread(v.data(), sizeof(double), 7, f) == 7 && std::fread(&n_poses, sizeof(int), 1, f) == 1 && n_poses >= 0, "guess / n_poses");
    guesses.push_back(msfl::Rigid3d(v));
    for (int i = 0; i < n_poses; ++i) {
      need(std::fread(v.data(), sizeof(double), 7, f) == 7, "pose");
      poses[p].push_back(msfl::Rigid3d(v));
    }
  }
  double max_dist = 0.0;
  need(std::fread(&max_dist, sizeof(double), 1, f) == 1, "max_dist");
  std::fclose(f);

  msfl::MappingScanMatcher matcher(0);
  matcher.SetPairMaps(maps);
  const std::vector<std::vector<msfl::PoseScore>> scores = matcher.ScorePairs(scans, poses, max_dist);
  need(scores.size() == poses.size(), "one record list per pair");
  const std::vector<int> status = matcher.MatchPairsResident(scans, &guesses);
  need(status.size() == scans.size(), "one status per pair");
  std::vector<std::vector<msfl::Rigid3d>> refined;
  for (const msfl::Rigid3d& g : guesses) refined.push_back(std::vector<msfl::Rigid3d>(1, g));
  const std::vector<std::vector<msfl::PoseScore>> after = matcher.ScorePairs(scans, refined, max_dist);

  std::FILE* o = std::fopen(argv[2], "wb");
  need(o != nullptr, "cannot open the output");
  static_assert(sizeof(msfl::PoseScore) == 32, "record size");
  for (std::size_t p = 0; p < scores.size(); ++p) {
    need(scores[p].size() == poses[p].size(), "one record per pose");
    if (!scores[p].empty()) std::fwrite(scores[p].data(), 32, scores[p].size(), o);
  }
  if (!status.empty()) std::fwrite(status.data(), sizeof(int), status.size(), o);
  for (msfl::Rigid3d& g : guesses) { const auto v = g.ToVector7(); std::fwrite(v.data(), sizeof(double), 7, o); }
  for (const std::vector<msfl::PoseScore>& a : after) { need(a.size() == 1, "one record per registered pose"); std::fwrite(a.data(), 32, 1, o); }
  std::fclose(o);
  return 0;
}
