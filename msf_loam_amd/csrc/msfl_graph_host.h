// Host-side bookkeeping of the pose graph (msfl_api_graph.inc): free-node numbering, adjacency lists, long / chain classification and
// the level sizes of the cyclic reduction.  Plain C++ over plain arrays, no HIP: tests/cpp/graph_structure_check.cpp runs it under the
// host sanitizers.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

namespace msfl {

constexpr int kGraphTail = 1024;     // blocks the one-workgroup tail of the cyclic reduction takes over
constexpr int kGraphMaxLevels = 32;

struct GraphLevels {                 // cyclic reduction: level l has n[l] blocks; off / ioff: where its D, L (rhs, sol) / D^-1 start
  int count, tail;                   // levels; first level the one-workgroup tail owns (n[tail] <= kGraphTail)
  int n[kGraphMaxLevels], off[kGraphMaxLevels], ioff[kGraphMaxLevels];
};

struct GraphStructure {
  int n_free = 0, n_long = 0;
  std::vector<int> free_of, node_of, adj_off, adj, ladj_off, ladj, fac_ij;
};

// factor k (edges first, then fixes) joins nodes ij[2k], ij[2k + 1]; adjacency per free node in factor order; a factor is long when both
// ends are free and more than one apart in the free numbering
inline void graph_build_structure(int n_nodes, const unsigned char* fixed, const std::vector<int>& ij, GraphStructure* s) {
  const int nf = (int)(ij.size() / 2);
  s->free_of.assign((size_t)n_nodes, -1); s->node_of.clear();
  for (int i = 0; i < n_nodes; i++)
    if (!fixed[i]) { s->free_of[i] = (int)s->node_of.size(); s->node_of.push_back(i); }
  s->n_free = (int)s->node_of.size(); s->n_long = 0;
  s->fac_ij = ij;
  s->adj_off.assign((size_t)s->n_free + 1, 0); s->ladj_off.assign((size_t)s->n_free + 1, 0);
  std::vector<unsigned char> is_long((size_t)nf, 0);
  for (int k = 0; k < nf; k++) {
    const int a = s->free_of[ij[2 * k]], b = s->free_of[ij[2 * k + 1]];
    is_long[k] = a >= 0 && b >= 0 && std::abs(a - b) > 1;
    s->n_long += is_long[k];
    for (int f : {a, b})
      if (f >= 0) { s->adj_off[f + 1]++; s->ladj_off[f + 1] += is_long[k]; }
  }
  for (int f = 0; f < s->n_free; f++) { s->adj_off[f + 1] += s->adj_off[f]; s->ladj_off[f + 1] += s->ladj_off[f]; }
  s->adj.assign((size_t)s->adj_off[s->n_free], 0); s->ladj.assign((size_t)s->ladj_off[s->n_free], 0);
  std::vector<int> at(s->adj_off.begin(), s->adj_off.end() - 1), lat(s->ladj_off.begin(), s->ladj_off.end() - 1);
  for (int k = 0; k < nf; k++)
    for (int side = 0; side < 2; side++) {
      const int f = s->free_of[ij[2 * k + side]];
      if (f < 0) continue;
      s->adj[at[f]++] = 2 * k + side;
      if (is_long[k]) s->ladj[lat[f]++] = 2 * k + side;
    }
}

// level sizes of the cyclic reduction over n blocks, any n >= 1: halve (rounding up) down to one block
inline GraphLevels graph_levels(int n) {
  GraphLevels v{};
  int off = 0, ioff = 0;
  v.tail = -1;
  for (;;) {
    v.n[v.count] = n; v.off[v.count] = off; v.ioff[v.count] = ioff;
    if (v.tail < 0 && n <= kGraphTail) v.tail = v.count;
    v.count++;
    off += n; ioff += std::max(1, n / 2);
    if (n == 1) break;
    n = (n + 1) / 2;
  }
  return v;
}


}  // namespace msfl
