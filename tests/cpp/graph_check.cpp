// The C++ face of the pose graph (msfl::GpsFusion, msfl::PoseGraph, include/msfl/pose_graph.hpp) on the problems of a file:
//   graph_check <in.bin> <out.bin>
// in : int n, int n_fixed_points; n local poses of 7 doubles (pose k is stamped k seconds); per fixed point double time, double p[3];
//      then int n, int n_edges, int n_fixes; n poses of 7 doubles; n ints (1 = fixed node); the msfl_graph_edge and msfl_graph_fix records
// out: GpsFusion: the n - 1 edge records and the fix records Optimize() built, the n optimised poses, the msfl_graph_summary;
//      PoseGraph: the n optimised poses, the msfl_graph_summary
// tests/test_gpu_graph.py compares the file with the ctypes path byte for byte.
#include <cstdio>
#include <vector>

#include "msfl/pose_graph.hpp"

template <class T>
static bool rd(std::FILE* f, T* p, std::size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int hdr[2];
  if (!rd(f, hdr, 2)) return 2;
  {
    std::vector<double> poses(static_cast<std::size_t>(hdr[0]) * 7), fp(static_cast<std::size_t>(hdr[1]) * 4);
    if (!rd(f, poses.data(), poses.size()) || !rd(f, fp.data(), fp.size())) return 2;
    msfl::GpsFusion fusion;
    for (int k = 0; k < hdr[0]; ++k) {
      const double* p = poses.data() + 7 * k;
      fusion.AddLocalPose(static_cast<double>(k), msfl::Rigid3d(std::array<double, 7>{{p[0], p[1], p[2], p[3], p[4], p[5], p[6]}}));
    }
    for (int k = 0; k < hdr[1]; ++k) fusion.AddFixedPoint(fp[4 * k], msfl::Vector3d{{fp[4 * k + 1], fp[4 * k + 2], fp[4 * k + 3]}});
    if (!fusion.Optimize()) return 3;
    std::fwrite(fusion.edges().data(), sizeof(msfl_graph_edge), fusion.edges().size(), o);
    std::fwrite(fusion.fixes().data(), sizeof(msfl_graph_fix), fusion.fixes().size(), o);
    for (const auto& lp : fusion.local_poses()) {
      const std::array<double, 7> v = lp.pose.ToVector7();
      std::fwrite(v.data(), sizeof(double), 7, o);
    }
    std::fwrite(&fusion.summary(), sizeof(msfl_graph_summary), 1, o);
  }
  int h3[3];
  if (!rd(f, h3, 3)) return 2;
  {
    const int n = h3[0];
    std::vector<double> poses(static_cast<std::size_t>(n) * 7);
    std::vector<int> fixed(static_cast<std::size_t>(n));
    std::vector<msfl_graph_edge> edges(static_cast<std::size_t>(h3[1]));
    std::vector<msfl_graph_fix> fixes(static_cast<std::size_t>(h3[2]));
    if (!rd(f, poses.data(), poses.size()) || !rd(f, fixed.data(), fixed.size()) || !rd(f, edges.data(), edges.size()) || !rd(f, fixes.data(), fixes.size()))
      return 2;
    msfl_graph_config c = msfl::PoseGraph::DefaultConfig();
    c.max_nodes = n; c.max_edges = h3[1]; c.max_fixes = h3[2];
    msfl::PoseGraph graph(&c);
    std::vector<msfl::Rigid3d> nodes;
    for (int k = 0; k < n; ++k) {
      const double* p = poses.data() + 7 * k;
      nodes.emplace_back(std::array<double, 7>{{p[0], p[1], p[2], p[3], p[4], p[5], p[6]}});
    }
    if (graph.AddNodes(nodes) != 0) return 3;
    for (int k = 0; k < n; ++k)
      if (fixed[static_cast<std::size_t>(k)]) graph.SetFixed(k);
    graph.AddEdges(edges);
    graph.AddFixes(fixes);
    const msfl_graph_summary s = graph.Optimize();
    for (const msfl::Rigid3d& p : graph.Poses()) {
      const std::array<double, 7> v = p.ToVector7();
      std::fwrite(v.data(), sizeof(double), 7, o);
    }
    std::fwrite(&s, sizeof(s), 1, o);
  }
  std::fclose(f);
  std::fclose(o);
  return 0;
}
