// msfl_pairs.cuh — one grid index per (map, scan) PAIR, built for a whole batch of pairs at once.
//
// The reference registers one scan against one map per MatchScan2Map call and rebuilds both kd-trees inside the call
// (mapping_scan_matcher.cc:66-73; call site laser_mapping.cc:304-311).  `msfl_match_scan2map_batch` covers "many scans, one map";
// this is the other shape the north star names, "many map-submap pairs": P maps (corner + surf cloud each), P scans, scan p is
// registered against map p only.  The P exact-kNN grids (msfl_knn_index.cuh) live in ONE set of arrays:
//   sorted map   all P clouds concatenated, each pair's points ordered by ITS grid's cells; the index word keeps the point's
//                position in the concatenated input, so ties break exactly as in a single call on that pair's cloud
//   cell table   pair p owns the slice [cell_base[p], cell_base[p + 1]) of one dense count / start array (the slice sizes are
//                host-known bounds, 2 x points + 4 096; the device grows a pair's cell edge until its grid fits its slice),
//                unused cells count zero, so ONE exclusive scan over the whole array yields every pair's cell starts
//   descriptors  GridDesc[P]
// Five launches + one rocPRIM scan per cloud kind, whatever P is.
#pragma once
#include <hip/hip_runtime.h>

#include "msfl_kernels.cuh"

namespace msfl {

// per-pair bounding boxes as six order-preserving ints (the encoding of grid_bbox_kernel): armed, then one thread per map point
// of the concatenated clouds; a workgroup that lies inside one pair (nearly all do) reduces first and issues six atomics
__global__ void __launch_bounds__(256) pairs_arm_kernel(int* __restrict__ bbox, int n_pairs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * n_pairs) bbox[i] = (i % 6) < 3 ? 0x7fffffff : (int)0x80000000;
}

// Launch geometry of the three per-point kernels: blockIdx.y = pair, blockIdx.x = a chunk of kPairChunk points inside the pair
// (grid.x = the longest pair's chunk count; a pair's surplus workgroups leave at once).  A 1-D launch over the concatenated cloud
// needs every wavefront to find its pair first (a binary search over the offsets: eight dependent loads before the point is even
// requested), and that search, not the atomics, was what the first version of these kernels spent its time in.
constexpr int kPairChunk = 1024;                   // points per workgroup: four per lane, their loads issued together
__global__ void __launch_bounds__(256)
pairs_bbox_kernel(const float4* __restrict__ pts, const int* __restrict__ off, int* __restrict__ bbox) {
  const int pp = blockIdx.y;
  const int lo = off[pp] + (int)blockIdx.x * kPairChunk, hi = min(off[pp + 1], lo + kPairChunk);
  if (lo >= hi) return;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  float4 q[4];
#pragma unroll
  for (int u = 0; u < 4; u++) { const int i = lo + u * 256 + (int)threadIdx.x; q[u] = pts[min(i, hi - 1)]; }
#pragma unroll
  for (int u = 0; u < 4; u++) grid_bbox_take(mn, mx, q[u], lo + u * 256 + (int)threadIdx.x < hi);
  grid_bbox_publish(mn, mx, bbox + 6 * pp);
}

// one thread per pair: its GridDesc (cell edge grown until the grid fits the pair's slice of the cell table)
__global__ void __launch_bounds__(256)
pairs_desc_kernel(const int* __restrict__ bbox, int n_pairs, const int* __restrict__ cell_base, double radius, GridDesc* __restrict__ gdesc) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  gdesc[p] = grid_desc_from_bbox(bbox + 6 * p, radius, cell_base[p + 1] - cell_base[p]);
}

// one thread per map point of the concatenated clouds: its pair, its cell in that pair's grid
__global__ void __launch_bounds__(256)
pairs_count_kernel(const float4* __restrict__ pts, const int* __restrict__ off, const int* __restrict__ cell_base,
                   const GridDesc* __restrict__ gdesc, int* __restrict__ cell_of, int* __restrict__ count) {
  const int p = blockIdx.y;
  const int lo = off[p] + (int)blockIdx.x * kPairChunk, hi = min(off[p + 1], lo + kPairChunk);
  if (lo >= hi) return;
  const GridDesc g = gdesc[p];
  const int base = cell_base[p], o0 = off[0];
  float4 q[4];
#pragma unroll
  for (int u = 0; u < 4; u++) { const int i = lo + u * 256 + (int)threadIdx.x; q[u] = pts[min(i, hi - 1)]; }
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int i = lo + u * 256 + (int)threadIdx.x;
    if (i >= hi) break;
    int c = -1;
    if (grid_indexed(q[u])) { c = base + grid_cell_of(g, q[u]); atomicAdd(&count[c], 1); }
    cell_of[i - o0] = c;
  }
}

// cursor[] = the counts on entry, consumed back to zero (as grid_scatter_kernel); sorted / pos_of are indexed from the
// concatenated cloud's first point (off[0])
__global__ void __launch_bounds__(256)
pairs_scatter_kernel(const float4* __restrict__ pts, int n, const int* __restrict__ off, const int* __restrict__ cell_of,
                     const int* __restrict__ cell_start, int* __restrict__ cursor, float4* __restrict__ sorted, int* __restrict__ pos_of) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  // the index word is k, the index inside the concatenated cloud: unique, and ordered like the pair's own indices
  grid_scatter_point(&pts[off[0] + k], k, cell_of[k], cell_start, 0, cursor, sorted, pos_of);
}

}  // namespace msfl
