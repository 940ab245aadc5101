// msfl_score_poses through the C++ mirror (include/msfl/scan_matcher.hpp): MappingScanMatcher::MatchScan2Map makes the map
// resident, ScorePoses then scores the scan at the given poses.
//   in : n_map_corner, points | n_map_surf, points | n_corner, points | n_surf, points | guess[7] | max_dist | n_poses | poses[7 n]
//   out: n_poses records of msfl_pose_score (32 bytes each) | Fitness, Rmse of each (doubles)
// Compiled by tests/test_gpu_score.py with plain g++; tests/cpp/Makefile does not know it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl/scan_matcher.hpp"

static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "score_check: %s\n", what); std::exit(2); } }

static void read_cloud(std::FILE* f, msfl::PointCloud<msfl::PointType>* c) {
  int n = 0;
  need(std::fread(&n, sizeof(int), 1, f) == 1 && n >= 0, "cloud size");
  c->points.resize(static_cast<std::size_t>(n));
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  need(n == 0 || std::fread(c->points.data(), 16, static_cast<std::size_t>(n), f) == static_cast<std::size_t>(n), "cloud points");
}

int main(int argc, char** argv) {
  need(argc == 3, "usage: score_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
  need(f != nullptr, "cannot open the input");
  msfl::TimestampedPointCloud<msfl::PointType> map, scan;
  read_cloud(f, map.cloud_corner_less_sharp.get());
  read_cloud(f, map.cloud_surf_less_flat.get());
  read_cloud(f, scan.cloud_corner_less_sharp.get());
  read_cloud(f, scan.cloud_surf_less_flat.get());
  std::array<double, 7> guess;
  double max_dist = 0.0;
  int n_poses = 0;
  need(std::fread(guess.data(), sizeof(double), 7, f) == 7 && std::fread(&max_dist, sizeof(double), 1, f) == 1 &&
           std::fread(&n_poses, sizeof(int), 1, f) == 1 && n_poses >= 0, "guess / max_dist / n_poses");
  std::vector<msfl::Rigid3d> poses;
  for (int i = 0; i < n_poses; ++i) {
    std::array<double, 7> v;
    need(std::fread(v.data(), sizeof(double), 7, f) == 7, "pose");
    poses.push_back(msfl::Rigid3d(v));
  }
  std::fclose(f);

  msfl::MappingScanMatcher matcher(0);
  msfl::Rigid3d pose(guess);
  need(matcher.MatchScan2Map(map, scan, false, nullptr, &pose, nullptr), "MatchScan2Map returned false");
  const std::vector<msfl::PoseScore> scores = matcher.ScorePoses(scan, poses, max_dist);
  need(scores.size() == poses.size(), "one record per pose");

  std::FILE* o = std::fopen(argv[2], "wb");
  need(o != nullptr, "cannot open the output");
  static_assert(sizeof(msfl::PoseScore) == 32, "record size");
  if (!scores.empty()) std::fwrite(scores.data(), 32, scores.size(), o);
  const std::size_t n_features = scan.cloud_corner_less_sharp->size() + scan.cloud_surf_less_flat->size();
  for (const msfl::PoseScore& s : scores) {
    const double fr[2] = {s.Fitness(n_features), s.Rmse()};
    std::fwrite(fr, sizeof(double), 2, o);
  }
  std::fclose(o);
  return 0;
}
