// The pose graph's host-side bookkeeping (msf_loam_amd/csrc/msfl_graph_host.h) under the host sanitizers: no GPU, no HIP.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I msf_loam_amd/csrc tests/cpp/graph_structure_check.cpp -o graph_structure_check
// Checks, for chains of every length up to 2 100 and a few large ones, that the reduction's level sizes halve down to one block, that
// the offsets are the running sums and that the tail starts at the first level of at most kGraphTail blocks; and for seeded graphs with
// fixed nodes, hubs and double edges that the adjacency lists hold every (factor, side) of a free node exactly once in factor order and
// that the long list is the sub-list of the factors whose ends are both free and more than one apart.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msfl_graph_host.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int check_levels(int n) {
  const msfl::GraphLevels v = msfl::graph_levels(n);
  REQUIRE(v.count >= 1 && v.count <= msfl::kGraphMaxLevels);
  REQUIRE(v.n[0] == n && v.n[v.count - 1] == 1 && v.off[0] == 0 && v.ioff[0] == 0);
  for (int l = 0; l + 1 < v.count; l++) {
    REQUIRE(v.n[l] >= 2 && v.n[l + 1] == (v.n[l] + 1) / 2);
    REQUIRE(v.off[l + 1] == v.off[l] + v.n[l] && v.ioff[l + 1] == v.ioff[l] + v.n[l] / 2);
  }
  REQUIRE(v.tail >= 0 && v.tail < v.count && v.n[v.tail] <= msfl::kGraphTail && (v.tail == 0 || v.n[v.tail - 1] > msfl::kGraphTail));
  return 0;
}

static int check_structure(int n_nodes, int n_factors, unsigned seed) {
  std::srand(seed);
  std::vector<unsigned char> fixed((size_t)n_nodes, 0);
  for (int i = 0; i < n_nodes; i++) fixed[i] = std::rand() % 7 == 0;
  std::vector<int> ij;
  for (int k = 0; k < n_factors; k++) {
    int a = std::rand() % n_nodes, b = k % 3 == 0 ? (a + 1) % n_nodes : (k % 5 == 0 ? 0 : std::rand() % n_nodes);   // chain edges, a hub at node 0, random pairs
    if (a == b) b = (a + 1) % n_nodes;
    ij.push_back(a); ij.push_back(b);
  }
  msfl::GraphStructure s;
  msfl::graph_build_structure(n_nodes, fixed.data(), ij, &s);
  int n_free = 0, n_long = 0;
  for (int i = 0; i < n_nodes; i++) {
    REQUIRE(s.free_of[i] == (fixed[i] ? -1 : n_free));
    if (!fixed[i]) { REQUIRE(s.node_of[(size_t)n_free] == i); n_free++; }
  }
  REQUIRE(s.n_free == n_free && (int)s.adj_off.size() == n_free + 1 && (int)s.ladj_off.size() == n_free + 1);
  std::vector<int> seen(2 * (size_t)n_factors, 0);
  for (int f = 0; f < n_free; f++) {
    int last = -1, li = s.ladj_off[f];
    for (int e = s.adj_off[f]; e < s.adj_off[f + 1]; e++) {
      const int code = s.adj[(size_t)e], k = code >> 1, side = code & 1;
      REQUIRE(code > last); last = code;
      REQUIRE(k >= 0 && k < n_factors && s.free_of[ij[2 * k + side]] == f);
      seen[(size_t)code]++;
      const int o = s.free_of[ij[2 * k + (side ^ 1)]];
      if (o >= 0 && std::abs(o - f) > 1) { REQUIRE(li < s.ladj_off[f + 1] && s.ladj[(size_t)li] == code); li++; }
    }
    REQUIRE(li == s.ladj_off[f + 1]);
  }
  for (int k = 0; k < n_factors; k++) {
    const int a = s.free_of[ij[2 * k]], b = s.free_of[ij[2 * k + 1]];
    REQUIRE(seen[2 * (size_t)k] == (a >= 0) && seen[2 * (size_t)k + 1] == (b >= 0));
    n_long += a >= 0 && b >= 0 && std::abs(a - b) > 1;
  }
  REQUIRE(s.n_long == n_long && (int)s.ladj.size() == 2 * n_long);
  return 0;
}

int main() {
  for (int n = 1; n <= 2100; n++)
    if (check_levels(n)) return 1;
  for (int n : {4095, 4096, 4097, 65537, 100000, 1 << 20, (1 << 24) + 1})
    if (check_levels(n)) return 1;
  for (unsigned seed = 1; seed <= 40; seed++)
    if (check_structure(2 + (int)(seed * 37 % 300), (int)(seed * 53 % 700), seed)) return 1;
  {                                                   // nothing free, nothing at all
    msfl::GraphStructure s;
    std::vector<unsigned char> fixed(3, 1);
    msfl::graph_build_structure(3, fixed.data(), {0, 1, 1, 2}, &s);
    REQUIRE(s.n_free == 0 && s.adj.empty() && s.n_long == 0);
    msfl::graph_build_structure(0, nullptr, {}, &s);
    REQUIRE(s.n_free == 0 && s.adj_off.size() == 1);
  }
  std::puts("graph structure ok");
  return 0;
}
