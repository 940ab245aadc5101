// The pose graph's host-side bookkeeping (msf_loam_amd/csrc/msfl_graph_host.h) under the host sanitizers: no GPU, no HIP.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I msf_loam_amd/csrc tests/cpp/graph_structure_check.cpp -o graph_structure_check
// Checks, for chains of every length up to 2 100 and a few large ones, that the reduction's level sizes halve down to one block, that
// the offsets are the running sums and that the tail starts at the first level of at most kGraphTail blocks; and for seeded graphs with
// fixed nodes, hubs and double edges that the adjacency lists hold every (factor, side) of a free node exactly once in factor order and
// that the long list is the sub-list of the factors whose ends are both free and more than one apart.  At the sizes where the layout
// changes (1, 2, 3, 1 024 / 1 025, 2 048 / 2 049, 4 097) the level list is written out and no level's range may reach into the next;
// and the layouts `span`, `runs` and `hub_across_fixed` of tests/graph_structure_cases.py are written out with the classification and
// the adjacency they must give.
#include <cstdio>
#include <initializer_list>
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

// the level list at a size where the layout changes: what it must be, written out, and that no level's D / L (off) or D^-1 (ioff)
// range reaches into the next one's or past the totals the work area is carved by
static int check_levels_at(int n, int count, int tail, std::initializer_list<int> sizes) {
  const msfl::GraphLevels v = msfl::graph_levels(n);
  REQUIRE(v.count == count && v.tail == tail && (int)sizes.size() == count);
  int l = 0;
  for (int want : sizes) { REQUIRE(v.n[l] == want); l++; }
  const int blocks = v.off[v.count - 1] + 1, inv = v.ioff[v.count - 1] + 1;
  for (l = 0; l < v.count; l++) {
    const int n_inv = v.n[l] == 1 ? 1 : v.n[l] / 2;                 // blocks the level inverts: its odd ones, or the last one
    const int off_end = v.off[l] + v.n[l], ioff_end = v.ioff[l] + n_inv;
    REQUIRE(v.off[l] >= 0 && v.ioff[l] >= 0 && off_end <= blocks && ioff_end <= inv);
    if (l + 1 < v.count) REQUIRE(off_end <= v.off[l + 1] && ioff_end <= v.ioff[l + 1]);
  }
  int sum = 0;
  for (l = 0; l < v.count; l++) sum += v.n[l];
  REQUIRE(blocks == sum);
  // launched levels: every one before the tail is larger than the tail's capacity, the tail's own is not
  for (l = 0; l < v.count; l++) REQUIRE((v.n[l] > msfl::kGraphTail) == (l < v.tail));
  return 0;
}

// a layout written out: fixed nodes, factors (i, j), and per factor whether it must be long; the adjacency of every free node is then
// the factors that touch it, in factor order, and the long list its long ones
static int check_layout(int n_nodes, std::initializer_list<int> fixed_nodes, const std::vector<int>& ij, const std::vector<int>& want_long,
                        int want_free) {
  std::vector<unsigned char> fixed((size_t)n_nodes, 0);
  for (int k : fixed_nodes) fixed[(size_t)k] = 1;
  const int nf = (int)(ij.size() / 2);
  REQUIRE((int)want_long.size() == nf);
  msfl::GraphStructure s;
  msfl::graph_build_structure(n_nodes, fixed.data(), ij, &s);
  REQUIRE(s.n_free == want_free);
  int n_long = 0;
  for (int k = 0; k < nf; k++) n_long += want_long[(size_t)k];
  REQUIRE(s.n_long == n_long && (int)s.ladj.size() == 2 * n_long);
  for (int i = 0, f = 0; i < n_nodes; i++) {
    if (fixed[(size_t)i]) { REQUIRE(s.free_of[(size_t)i] == -1); continue; }
    REQUIRE(s.free_of[(size_t)i] == f && s.node_of[(size_t)f] == i);
    std::vector<int> adj, ladj;
    for (int k = 0; k < nf; k++)
      for (int side = 0; side < 2; side++)
        if (ij[2 * (size_t)k + side] == i) { adj.push_back(2 * k + side); if (want_long[(size_t)k]) ladj.push_back(2 * k + side); }
    REQUIRE(std::vector<int>(s.adj.begin() + s.adj_off[(size_t)f], s.adj.begin() + s.adj_off[(size_t)f + 1]) == adj);
    REQUIRE(std::vector<int>(s.ladj.begin() + s.ladj_off[(size_t)f], s.ladj.begin() + s.ladj_off[(size_t)f + 1]) == ladj);
    f++;
  }
  return 0;
}

// the chain 0 - 1 - ... - (n - 1) and `extra` factors behind it
static std::vector<int> chain_and(int n, std::initializer_list<int> extra) {
  std::vector<int> ij;
  for (int k = 0; k + 1 < n; k++) { ij.push_back(k); ij.push_back(k + 1); }
  ij.insert(ij.end(), extra.begin(), extra.end());
  return ij;
}

static int check_named_layouts() {
  const int n = 40;
  std::vector<int> none((size_t)n - 1, 0);
  auto with = [&](std::initializer_list<int> tail) { std::vector<int> v = none; v.insert(v.end(), tail.begin(), tail.end()); return v; };
  // span: (9, 12) and (19, 21) reach over the fixed nodes 10, 11 and 20, as an edge and as a fix: neighbours in the free numbering
  if (check_layout(n, {10, 11, 20}, chain_and(n, {9, 12, 19, 21, 9, 12}), with({0, 0, 0}), 37)) return 1;
  {
    msfl::GraphStructure s;
    std::vector<unsigned char> fixed((size_t)n, 0);
    fixed[10] = fixed[11] = fixed[20] = 1;
    msfl::graph_build_structure(n, fixed.data(), chain_and(n, {9, 12, 19, 21, 9, 12}), &s);
    REQUIRE(s.free_of[9] == 9 && s.free_of[12] == 10 && s.free_of[19] == 17 && s.free_of[21] == 18);
    // node 12's list: its chain factors (11, 12) and (12, 13), then side 1 of the two spanning factors
    const int f = s.free_of[12];
    REQUIRE(s.adj_off[(size_t)f + 1] - s.adj_off[(size_t)f] == 4);
    REQUIRE(s.adj[(size_t)s.adj_off[(size_t)f] + 2] == 2 * (n - 1) + 1 && s.adj[(size_t)s.adj_off[(size_t)f] + 3] == 2 * (n + 1) + 1);
  }
  // runs: {0, 1, 2} and {20, 21} fixed; (20, 21), (21, 20) and a fix over them have no free end and appear in no list
  if (check_layout(n, {0, 1, 2, 20, 21}, chain_and(n, {21, 20, 20, 21}), with({0, 0}), 35)) return 1;
  {
    msfl::GraphStructure s;
    std::vector<unsigned char> fixed((size_t)n, 0);
    for (int k : {0, 1, 2, 20, 21}) fixed[(size_t)k] = 1;
    const std::vector<int> ij = chain_and(n, {21, 20, 20, 21});
    msfl::graph_build_structure(n, fixed.data(), ij, &s);
    for (int code : s.adj) REQUIRE(code >> 1 != 0 && code >> 1 != 1 && code >> 1 != 20 && code >> 1 != n - 1 && code >> 1 != n);
    // the chain's 78 sides less the 9 that sit on a fixed node
    REQUIRE(s.free_of[3] == 0 && s.free_of[19] == 16 && s.free_of[22] == 17 && (int)s.adj.size() == 2 * (n - 1) - 9);
  }
  // hub_across_fixed: (14, 16) is long while 15 is free, a chain factor once 15 is fixed; a last node that is fixed, for good measure
  if (check_layout(n, {}, chain_and(n, {14, 16}), with({1}), 40)) return 1;
  if (check_layout(n, {15}, chain_and(n, {14, 16}), with({0}), 39)) return 1;
  if (check_layout(n, {15, n - 1}, chain_and(n, {14, 16, 16, 14}), with({0, 0}), 38)) return 1;
  if (check_layout(n, {n - 1}, chain_and(n, {16, 14}), with({1}), 39)) return 1;
  return 0;
}

int main() {
  if (check_levels_at(1, 1, 0, {1})) return 1;
  if (check_levels_at(2, 2, 0, {2, 1})) return 1;
  if (check_levels_at(3, 3, 0, {3, 2, 1})) return 1;
  if (check_levels_at(1024, 11, 0, {1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1})) return 1;
  if (check_levels_at(1025, 12, 1, {1025, 513, 257, 129, 65, 33, 17, 9, 5, 3, 2, 1})) return 1;
  if (check_levels_at(2048, 12, 1, {2048, 1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1})) return 1;
  if (check_levels_at(2049, 13, 2, {2049, 1025, 513, 257, 129, 65, 33, 17, 9, 5, 3, 2, 1})) return 1;
  if (check_levels_at(4097, 14, 3, {4097, 2049, 1025, 513, 257, 129, 65, 33, 17, 9, 5, 3, 2, 1})) return 1;
  if (check_named_layouts()) return 1;
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
