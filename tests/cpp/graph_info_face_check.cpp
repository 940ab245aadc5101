// The information-factor part of the C++ face (msfl::PoseGraphEdgeInfo, PoseGraph::AddEdgesInfo / AddFixesInfo / Chi2,
// include/msfl/pose_graph.hpp) on the problem of a file:
//   graph_info_face_check <in.bin> <out.bin>
// in : int n, n_edges, n_info, n_fixes_info; n poses of 7 doubles; n ints (1 = fixed node); the msfl_graph_edge records; per information
//      edge: int i, j, double pose_i[7], pose_j[7], scale, the msfl_match_uncertainty record; the msfl_graph_fix_info records
// out: the msfl_graph_edge_info records PoseGraphEdgeInfo built, the n optimised poses, the msfl_graph_summary, then the chi-squares at
//      the optimised poses: n_edges (plain edges), n_info, n_fixes_info doubles
// tests/test_gpu_graph_info.py compares the file with the ctypes path byte for byte.
#include <cstdio>
#include <vector>

#include "msfl/pose_graph.hpp"

template <class T>
static bool rd(std::FILE* f, T* p, std::size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

static msfl::Rigid3d rigid(const double* p) { return msfl::Rigid3d(std::array<double, 7>{{p[0], p[1], p[2], p[3], p[4], p[5], p[6]}}); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int h[4];
  if (!rd(f, h, 4)) return 2;
  const int n = h[0];
  std::vector<double> poses(static_cast<std::size_t>(n) * 7);
  std::vector<int> fixed(static_cast<std::size_t>(n));
  std::vector<msfl_graph_edge> edges(static_cast<std::size_t>(h[1]));
  if (!rd(f, poses.data(), poses.size()) || !rd(f, fixed.data(), fixed.size()) || !rd(f, edges.data(), edges.size())) return 2;
  std::vector<msfl_graph_edge_info> info;
  for (int k = 0; k < h[2]; ++k) {
    int ij[2];
    double pp[15];
    msfl_match_uncertainty unc;
    if (!rd(f, ij, 2) || !rd(f, pp, 15) || !rd(f, &unc, 1)) return 2;
    info.push_back(msfl::PoseGraphEdgeInfo(ij[0], ij[1], rigid(pp), rigid(pp + 7), unc, pp[14]));
  }
  std::vector<msfl_graph_fix_info> fixes(static_cast<std::size_t>(h[3]));
  if (!rd(f, fixes.data(), fixes.size())) return 2;
  msfl_graph_config c = msfl::PoseGraph::DefaultConfig();
  c.max_nodes = n; c.max_edges = h[1] + h[2]; c.max_fixes = h[3] > 0 ? h[3] : 1;
  msfl::PoseGraph graph(&c);
  std::vector<msfl::Rigid3d> nodes;
  for (int k = 0; k < n; ++k) nodes.push_back(rigid(poses.data() + 7 * k));
  if (graph.AddNodes(nodes) != 0) return 3;
  for (int k = 0; k < n; ++k)
    if (fixed[static_cast<std::size_t>(k)]) graph.SetFixed(k);
  graph.AddEdges(edges);
  graph.AddEdgesInfo(info);
  graph.AddFixesInfo(fixes);
  const msfl_graph_summary s = graph.Optimize();
  std::fwrite(info.data(), sizeof(msfl_graph_edge_info), info.size(), o);
  for (const msfl::Rigid3d& p : graph.Poses()) {
    const std::array<double, 7> v = p.ToVector7();
    std::fwrite(v.data(), sizeof(double), 7, o);
  }
  std::fwrite(&s, sizeof(s), 1, o);
  const int kind[3] = {MSFL_GRAPH_FACTOR_EDGE, MSFL_GRAPH_FACTOR_EDGE_INFO, MSFL_GRAPH_FACTOR_FIX_INFO}, count[3] = {h[1], h[2], h[3]};
  for (int q = 0; q < 3; ++q) {
    const std::vector<double> chi = graph.Chi2(kind[q], 0, count[q]);
    std::fwrite(chi.data(), sizeof(double), chi.size(), o);
  }
  std::fclose(f);
  std::fclose(o);
  return 0;
}
