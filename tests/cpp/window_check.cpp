// The windowed map through the C++ mirror (include/msfl/scan_matcher.hpp): HybridGrid::InsertScan + Crop with the evicted points,
// and LaserSlam::SetMapWindow / MapWindow / ClearMapWindow over a few scans.
//   in : resolution, leaf (f32) | centre[3] (f64) | half_cells[3] (i32) | n, points (the cloud to insert)
//        | n_scans (i32), then per scan: n, {x, y, z, intensity (f32), ring (i32)} per point
//   out: msfl_grid_crop_info (8 i32) | n_evicted (i32), points | per scan: corner info, surf info (2 x 8 i32)
// The window is (2, 2, 1) after every scan; the last scan is fed after ClearMapWindow (all-zero records).
// Compiled by tests/test_gpu_grid_window.py with plain g++; tests/cpp/Makefile does not know it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl/scan_matcher.hpp"

static void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "window_check: %s\n", what); std::exit(2); } }

int main(int argc, char** argv) {
  need(argc == 3, "usage: window_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
  need(f != nullptr, "cannot open the input");
  float res_leaf[2];
  std::array<double, 3> centre;
  std::array<int, 3> half;
  int n = 0;
  need(std::fread(res_leaf, sizeof(float), 2, f) == 2 && std::fread(centre.data(), sizeof(double), 3, f) == 3 &&
       std::fread(half.data(), sizeof(int), 3, f) == 3 && std::fread(&n, sizeof(int), 1, f) == 1 && n > 0, "header");
  auto cloud = std::make_shared<msfl::PointCloud<msfl::PointType>>();
  static_assert(sizeof(msfl::PointType) == 16, "packed point");
  cloud->points.resize(static_cast<std::size_t>(n));
  need(std::fread(cloud->points.data(), 16, static_cast<std::size_t>(n), f) == static_cast<std::size_t>(n), "cloud");
  int n_scans = 0;
  need(std::fread(&n_scans, sizeof(int), 1, f) == 1 && n_scans > 1, "scan count");
  std::vector<msfl::PointCloud<msfl::PointTypeOriginal>> scans(static_cast<std::size_t>(n_scans));
  int cap = 0, rings = 0;
  for (auto& s : scans) {
    int m = 0;
    need(std::fread(&m, sizeof(int), 1, f) == 1 && m > 0, "scan size");
    for (int i = 0; i < m; ++i) {
      float p[4]; int ring;
      need(std::fread(p, sizeof(float), 4, f) == 4 && std::fread(&ring, sizeof(int), 1, f) == 1, "scan point");
      s.push_back(msfl::PointXYZIRT{p[0], p[1], p[2], p[3], static_cast<std::uint16_t>(ring), 0.f});
      if (ring + 1 > rings) rings = ring + 1;
    }
    if (m > cap) cap = m;
  }
  std::fclose(f);
  std::FILE* o = std::fopen(argv[2], "wb");
  need(o != nullptr, "cannot open the output");
  {
    msfl::HybridGrid grid(res_leaf[0], res_leaf[1], 0);
    grid.InsertScan(cloud);
    std::vector<msfl_point> evicted;
    const msfl_grid_crop_info info = grid.Crop(centre, half, &evicted);
    const int n_ev = static_cast<int>(evicted.size());
    std::fwrite(&info, sizeof(info), 1, o);
    std::fwrite(&n_ev, sizeof(int), 1, o);
    std::fwrite(evicted.data(), sizeof(msfl_point), evicted.size(), o);
  }
  {
    msfl::LaserSlam slam(0, cap, rings);
    slam.SetMapWindow({{2, 2, 1}}, 1);
    for (int k = 0; k < n_scans; ++k) {
      if (k == n_scans - 1) slam.ClearMapWindow();
      slam.AddLaserScan(scans[static_cast<std::size_t>(k)]);
      msfl_grid_crop_info w[2];
      slam.MapWindow(k, &w[0], &w[1]);
      std::fwrite(w, sizeof(msfl_grid_crop_info), 2, o);
    }
  }
  std::fclose(o);
  return 0;
}
