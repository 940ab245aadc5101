// The marginals part of the C++ face (msfl::PoseGraph::Marginals, msfl::RelativeCovariance, include/msfl/pose_graph.hpp) on the problem
// of a file:
//   graph_marginals_face_check <in.bin> <out.bin>
// in : int n, n_edges, n_info, n_pairs; n poses of 7 doubles; n ints (1 = fixed node); the msfl_graph_edge records; the
//      msfl_graph_edge_info records; n_pairs pairs of ints
// out: the n_pairs blocks of 36 doubles, the msfl_graph_marginals_summary, then RelativeCovariance of pairs 0, 1, 2 taken as
//      (a, a), (a, b), (b, b): 36 doubles
// tests/test_gpu_graph_marginals.py compares the file with the ctypes path byte for byte.
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
  std::vector<int> fixed(static_cast<std::size_t>(n)), flat(static_cast<std::size_t>(h[3]) * 2);
  std::vector<msfl_graph_edge> edges(static_cast<std::size_t>(h[1]));
  std::vector<msfl_graph_edge_info> info(static_cast<std::size_t>(h[2]));
  if (!rd(f, poses.data(), poses.size()) || !rd(f, fixed.data(), fixed.size()) || !rd(f, edges.data(), edges.size()) ||
      !rd(f, info.data(), info.size()) || !rd(f, flat.data(), flat.size()) || h[3] < 3)
    return 2;
  msfl_graph_config c = msfl::PoseGraph::DefaultConfig();
  c.max_nodes = n; c.max_edges = h[1] + h[2] > 0 ? h[1] + h[2] : 1; c.max_fixes = 1;
  msfl::PoseGraph graph(&c);
  std::vector<msfl::Rigid3d> nodes;
  for (int k = 0; k < n; ++k) nodes.push_back(rigid(poses.data() + 7 * k));
  if (graph.AddNodes(nodes) != 0) return 3;
  for (int k = 0; k < n; ++k)
    if (fixed[static_cast<std::size_t>(k)]) graph.SetFixed(k);
  graph.AddEdges(edges);
  graph.AddEdgesInfo(info);
  std::vector<std::pair<int, int>> pairs;
  for (int k = 0; k < h[3]; ++k) pairs.emplace_back(flat[2 * static_cast<std::size_t>(k)], flat[2 * static_cast<std::size_t>(k) + 1]);
  const msfl::PoseGraph::MarginalBlocks m = graph.Marginals(pairs);
  for (const std::array<double, 36>& b : m.blocks) std::fwrite(b.data(), sizeof(double), 36, o);
  std::fwrite(&m.summary, sizeof(m.summary), 1, o);
  const std::array<double, 36> rel = msfl::RelativeCovariance(nodes[static_cast<std::size_t>(pairs[0].first)], nodes[static_cast<std::size_t>(pairs[2].first)],
                                                              m.blocks[0], m.blocks[1], m.blocks[2]);
  std::fwrite(rel.data(), sizeof(double), 36, o);
  std::fclose(f);
  std::fclose(o);
  return 0;
}
