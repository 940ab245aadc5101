// The C++ mirror of the place database (msfl::PlaceDatabase, include/msfl/scan_matcher.hpp) on the scans of a file:
//   place_check <in.bin> <out.bin>
// in : int n_db, int n_query, int k, int n_prefilter, then per scan (database scans first) int n and n points of 16 bytes
// out: per query k msfl_place_match records, then per query one double: Yaw() of its first record
// tests/test_gpu_place.py compares the file with the ctypes path byte for byte.
#include <cstdio>
#include <vector>

#include "msfl/scan_matcher.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[4];
  if (std::fread(hdr, sizeof(int), 4, f) != 4) return 2;
  const int n_db = hdr[0], n_query = hdr[1], k = hdr[2], n_prefilter = hdr[3];
  std::vector<msfl::PointCloud<msfl::PointXYZI>> scans(static_cast<std::size_t>(n_db + n_query));
  for (auto& c : scans) {
    int n = 0;
    if (std::fread(&n, sizeof(int), 1, f) != 1) return 2;
    c.points.resize(static_cast<std::size_t>(n));
    if (n > 0 && std::fread(c.points.data(), 16, static_cast<std::size_t>(n), f) != static_cast<std::size_t>(n)) return 2;
  }
  std::fclose(f);
  msfl::PlaceDatabase db;
  for (int i = 0; i < n_db; ++i)
    if (db.Add(scans[static_cast<std::size_t>(i)]) != i) return 3;
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::vector<double> yaw;
  for (int i = 0; i < n_query; ++i) {
    const std::vector<msfl::PlaceMatch> m = db.Query(scans[static_cast<std::size_t>(n_db + i)], -1, n_prefilter, k);
    std::fwrite(m.data(), sizeof(msfl::PlaceMatch), m.size(), o);
    yaw.push_back(db.Yaw(m[0]));
  }
  std::fwrite(yaw.data(), sizeof(double), yaw.size(), o);
  std::fclose(o);
  return 0;
}
