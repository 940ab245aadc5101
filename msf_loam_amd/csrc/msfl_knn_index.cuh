// msfl_knn_index.cuh — the exact-kNN grid index over a map cloud (gfx950 / CDNA4): its geometry, stated once.
//
//   build   bounding box -> GridDesc -> cell of every point -> (prefix sums by the host's scan) -> points sorted by cell
//           grid_bbox_publish, grid_desc_from_bbox, grid_cell_of, grid_scatter_point; the single and the two-map launch chains
//   query   GridQuery (cell coordinates and x reach), GridRowOrder (the nine (y, z) rows, nearest first), grid_x_bounds
//   walks   grid_walk_exact (pruned on the caller's bound; knn5_grid here, nn1_grid in msfl_score.cuh) and knn5_grid_k32 (the
//           hot truncated-key form); the latency form (knn5_scan2map_rows_kernel, msfl_kernels.cuh) takes GridQuery
// The per-pair builds of msfl_pairs.cuh use the same cell rule, scatter step and bounding-box tail.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msfl_math.cuh"

namespace msfl {

// ---------------------------------------------------------------------------------------------
// K3: uniform-grid index.  Cell edge >= 1.001 * sqrt(max_sq_dist) so the 27-cell neighbourhood
// of a query contains every map point whose f32 distance can pass the reference's
// `pointSearchSqDis[4] < 1.0` gate: exact-kNN-equivalent on every ACCEPTED query.
// ---------------------------------------------------------------------------------------------
#ifndef MSFL_GRID_XSUB
#define MSFL_GRID_XSUB 3
#endif
constexpr int kGridXSub = MSFL_GRID_XSUB;

struct GridDesc {
  float ox, oy, oz;   // origin = bbox min
  float inv_cell;     // 1 / cell edge in y and z
  float inv_cell_x;   // cells are kGridXSub times finer along x (the fastest index): a (y,z) row of 2*kGridXSub+1 cells
                      // is still ONE contiguous range, but its ends can be trimmed in finer steps
  int dx, dy, dz;
  int n_pts;          // finite points indexed
  int n_cells;
  int reach;          // cells scanned on each side of the query cell (1)
  int want_cells;     // cells the bbox needs at the base cell edge (saturated); host feedback for the next build
  float cell2, cellx2;  // (1 / inv_cell)^2 and (1 / inv_cell_x)^2 in f32: every query needs them, computed once per build
};

// order-preserving float <-> int encoding for atomicMin/Max
__device__ __forceinline__ int float_to_ordered(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float ordered_to_float(int i) {
  const int j = i >= 0 ? i : i ^ 0x7fffffff;
#if defined(__HIP_DEVICE_COMPILE__)
  return __int_as_float(j);
#else
  float f; __builtin_memcpy(&f, &j, 4); return f;
#endif
}

// The bounding box of the finite points, as six order-preserving ints: bbox[0..2] = min, bbox[3..5] = max; armed to
// INT_MAX / INT_MIN (grid_bbox_rearm).
__device__ __forceinline__ bool grid_indexed(float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }   // the points a map index holds
__device__ __forceinline__ void grid_bbox_take(float (&mn)[3], float (&mx)[3], float4 p, bool live = true) {
  if (grid_indexed(p) && live) {         // `live` last: tested first, the compiler moves the caller's loads behind a branch per point
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
}
// The tail of every bounding-box kernel (workgroups of 256 threads, all of them arrive): wave shuffle, four LDS rows, then
// six lanes with one atomic each per workgroup (they all land on one cache line: keep them few).
__device__ __forceinline__ void grid_bbox_publish(float (&mn)[3], float (&mx)[3], int* __restrict__ bbox) {
  __shared__ float s_mn[4][3], s_mx[4][3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) { s_mn[wave][a] = mn[a]; s_mx[wave][a] = mx[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    const float v = fminf(fminf(s_mn[0][a], s_mn[1][a]), fminf(s_mn[2][a], s_mn[3][a]));
    if (v != INFINITY) atomicMin(&bbox[a], float_to_ordered(v));
  } else if (threadIdx.x < 6) {
    const int a = threadIdx.x - 3;
    const float v = fmaxf(fmaxf(s_mx[0][a], s_mx[1][a]), fmaxf(s_mx[2][a], s_mx[3][a]));
    if (v != -INFINITY) atomicMax(&bbox[3 + a], float_to_ordered(v));
  }
}
__device__ __forceinline__ void grid_bbox_body(const float4* __restrict__ pts, int n, int* __restrict__ bbox, int block, int n_blocks) {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int stride = n_blocks * blockDim.x;
  int i = block * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {       // four independent loads in flight per lane
    const float4 p0 = pts[i], p1 = pts[i + stride], p2 = pts[i + 2 * stride], p3 = pts[i + 3 * stride];
    grid_bbox_take(mn, mx, p0); grid_bbox_take(mn, mx, p1); grid_bbox_take(mn, mx, p2); grid_bbox_take(mn, mx, p3);
  }
  for (; i < n; i += stride) grid_bbox_take(mn, mx, pts[i]);
  grid_bbox_publish(mn, mx, bbox);
}
// n_dev (optional): the number of valid points lives on the device (a surrounded cloud that never visits the host);
// `n` is then the launch's upper bound
__global__ void __launch_bounds__(256) grid_bbox_kernel(const float4* __restrict__ pts, int n, int* __restrict__ bbox, const int* __restrict__ n_dev = nullptr) {
  if (n_dev) n = min(n, max(*n_dev, 0));
  grid_bbox_body(pts, n, bbox, (int)blockIdx.x, (int)gridDim.x);
}

__device__ __forceinline__ int grid_coord(float v, float o, float inv, int dim) {
  // clamp in float first: far-away queries must not overflow the int conversion
  float u = floorf((v - o) * inv);
  u = fminf(fmaxf(u, -2.0f), (float)dim + 1.0f);
  return (int)u;
}

__device__ __forceinline__ void grid_desc_squares(GridDesc& g) {
  const float cell = 1.0f / g.inv_cell, cellx = 1.0f / g.inv_cell_x;
  g.cell2 = cell * cell; g.cellx2 = cellx * cellx;
}
// Most cells along one axis (x: sub-cells).  The walk's two margins are ABSOLUTE, in cells: the cell edge exceeds the radius by
// 0.1 % (two points inside the gate are at most 0.999001 cells apart, so the reach of one cell, kGridXSub sub-cells, has 9.99e-4
// cells to spare) and axis_gap shrinks every lower bound by 1e-3 cell.  The rounding error of u = fl(fl(v - o) * inv) is
// RELATIVE: fl(v - o) is off by at most half an ulp, <= 2^-24 |v - o|, which the product scales to <= 2^-24 |u| cells, and the
// product's own rounding adds <= 2^-24 |u|.  The difference of two computed coordinates near |u| (a query and a map point; a
// lower bound measures the query against an integer that the point's computed coordinate does not pass) is therefore within
// 4 * 2^-24 |u| = 2^-22 |u| cells of the true one.  A query that matters lies within one cell of the box, so |u| <= dim + 1, and
//   2^-22 * (4096 + 1) = 9.768e-4 < 9.99e-4 < 1e-3
// (the error reaches 1e-3 at |u| = 4194).  The f32 rounding of inv itself is a common scale factor (6e-8 of a difference of at
// most kGridXSub cells) and the bounds' own arithmetic is relative 2^-23 or so of bounds below 2 cells: both far inside the
// 2.2e-5 cells left.  Beyond the limit the skipped-row and trimmed-cell tests DO lose true neighbours (tests/test_knn_grid_model.py
// finds them from |u| ~ 12 000 in y and ~ 18 000 in x), so such a box gets larger cells, like one that exceeds the table.
constexpr int kGridMaxDim = 4096;

// bbox -> grid descriptor, entirely on the device so that msfl_set_map needs no host round trip.
// Cell edge = 1.001 * acceptance radius, grown by 26 % steps until the dense table fits `cap_cells` and no axis has more than
// kGridMaxDim cells (larger cells stay exact: tested to 12 km extents, docs/kernels/scan2map.md "Index geometry").  A box
// within both limits at the base edge keeps the descriptor it always had.  An empty cloud yields n_cells = 1, n_pts = 0.
__device__ __forceinline__ GridDesc grid_desc_from_bbox(const int* __restrict__ bbox, double radius, int cap_cells) {
  GridDesc g;
  const int b0 = bbox[0];
  g.n_pts = 0; g.reach = 1;
  if (b0 == 0x7fffffff) {            // no finite point
    g.ox = g.oy = g.oz = 0.f; g.inv_cell = 1.f; g.inv_cell_x = (float)kGridXSub; g.dx = g.dy = g.dz = 1; g.n_cells = 1; g.want_cells = 1;
    grid_desc_squares(g);
    return g;
  }
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) { mn[a] = ordered_to_float(bbox[a]); mx[a] = ordered_to_float(bbox[3 + a]); }
  double cell = 1.001 * radius;
  int dims[3];
  bool first = true;
  g.want_cells = 1;
  for (;;) {
    double total = 1.0;
    for (int a = 0; a < 3; a++) {
      const double edge = a == 0 ? cell / kGridXSub : cell;
      dims[a] = (int)floor(((double)mx[a] - (double)mn[a]) / edge) + 2;   // +1 spare cell: f32 rounding of (v-o)*inv
      if (dims[a] < 2) dims[a] = 2;
      total *= dims[a];
    }
    if (first) { g.want_cells = total < 2.0e9 ? (int)total : 2000000000; first = false; }
    if (total <= (double)cap_cells && max(dims[0], max(dims[1], dims[2])) <= kGridMaxDim) break;
    cell *= 1.26;
  }
  g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
  g.inv_cell = (float)(1.0 / cell);
  g.inv_cell_x = (float)((double)kGridXSub / cell);
  g.dx = dims[0]; g.dy = dims[1]; g.dz = dims[2];
  g.n_cells = g.dx * g.dy * g.dz;
  grid_desc_squares(g);
  return g;
}

__device__ __forceinline__ void grid_bbox_rearm(int* __restrict__ bbox) {
  for (int a = 0; a < 3; a++) { bbox[a] = 0x7fffffff; bbox[3 + a] = (int)0x80000000; }
}

// A build's last words, by one thread of its last launch: the number of indexed (finite) points, the wanted table size into
// the pinned host word `want_host` (a hint for the span of the NEXT build's table: whichever build's value the host happens
// to see is fine, the descriptor never depends on it) and the bbox armed for the next build.
__device__ __forceinline__ void grid_build_done(GridDesc* __restrict__ g, int n_pts, int* __restrict__ want_host, int* __restrict__ bbox) {
  g->n_pts = n_pts;
  *want_host = g->want_cells;
  grid_bbox_rearm(bbox);
}

// Only launched for an EMPTY cloud (nothing else runs then); a non-empty build derives the descriptor
// inside grid_count_kernel and finishes in grid_scatter_kernel.
__global__ void grid_setup_kernel(int* __restrict__ bbox, double radius, int cap_cells, GridDesc* __restrict__ out, int* __restrict__ want_host) {
  *out = grid_desc_from_bbox(bbox, radius, cap_cells);
  grid_build_done(out, 0, want_host, bbox);
}

// The cell of an indexed map point (grid_indexed): its coordinates clamped into the grid, x fastest.  A point that is not
// indexed has the cell -1 in the builds' cell_of arrays; the callers write that themselves, so that "count it" stays inside
// the one branch on grid_indexed.
__device__ __forceinline__ int grid_cell_of(const GridDesc& g, float4 p) {
  const int cx = min(max(grid_coord(p.x, g.ox, g.inv_cell_x, g.dx), 0), g.dx - 1);
  const int cy = min(max(grid_coord(p.y, g.oy, g.inv_cell, g.dy), 0), g.dy - 1);
  const int cz = min(max(grid_coord(p.z, g.oz, g.inv_cell, g.dz), 0), g.dz - 1);
  return (cz * g.dy + cy) * g.dx + cx;
}

// Every workgroup derives the (identical) descriptor from the finished bbox itself: one launch less
// per build than a separate one-thread setup kernel; workgroup 0 publishes it.
__device__ __forceinline__ void grid_count_body(const float4* __restrict__ pts, int n, const int* __restrict__ bbox,
                                                double radius, int cap_cells, GridDesc* __restrict__ gout,
                                                int* __restrict__ cell_of, int* __restrict__ count, int block) {
  __shared__ GridDesc s_g;
  if (threadIdx.x == 0) {
    s_g = grid_desc_from_bbox(bbox, radius, cap_cells);
    if (block == 0) *gout = s_g;
  }
  __syncthreads();
  const int i = block * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const GridDesc g = s_g;
  const float4 p = pts[i];
  int c = -1;
  if (grid_indexed(p)) { c = grid_cell_of(g, p); atomicAdd(&count[c], 1); }
  cell_of[i] = c;
}
__global__ void __launch_bounds__(256) grid_count_kernel(const float4* __restrict__ pts, int n, const int* __restrict__ bbox,
                                                          double radius, int cap_cells, GridDesc* __restrict__ gout,
                                                          int* __restrict__ cell_of, int* __restrict__ count, const int* __restrict__ n_dev = nullptr) {
  if (n_dev) n = min(n, max(*n_dev, 0));
  grid_count_body(pts, n, bbox, radius, cap_cells, gout, cell_of, count, (int)blockIdx.x);
}

// One point into the sorted copy.  c: its cell in `cursor` and `start` (< 0: not indexed); start[c] - sub: the cell's first position.
// cursor[] holds the per-cell counts on entry and is consumed — it is all zeros again afterwards, so
// the next build needs no memset; the order inside a cell is arbitrary, which is harmless because
// the kNN selection uses the total order (d2, original index).  The index word `i` is what breaks ties.
__device__ __forceinline__ void grid_scatter_point(const float4* __restrict__ src, int i, int c, const int* __restrict__ start, int sub,
                                                   int* __restrict__ cursor, float4* __restrict__ sorted, int* __restrict__ pos_of) {
  if (c < 0) { pos_of[i] = -1; return; }
  const int k = atomicSub(&cursor[c], 1) - 1;
  float4 p = *src;
  p.w = __int_as_float(i);
  const int at = start[c] - sub + k;
  sorted[at] = p;
  pos_of[i] = at;                       // original index -> position (the fit kernel fetches by index)
}
__global__ void __launch_bounds__(256) grid_scatter_kernel(const float4* __restrict__ pts, int n,
                                                            const int* __restrict__ cell_of,
                                                            const int* __restrict__ cell_start, int* __restrict__ cursor,
                                                            float4* __restrict__ sorted, int* __restrict__ pos_of,
                                                            GridDesc* __restrict__ g, int* __restrict__ bbox, int* __restrict__ want_host,
                                                            const int* __restrict__ n_dev = nullptr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (n_dev) n = min(n, max(*n_dev, 0));
  if (i == 0) grid_build_done(g, cell_start[g->n_cells], want_host, bbox);
  if (i >= n) return;
  grid_scatter_point(pts + i, i, cell_of[i], cell_start, 0, cursor, sorted, pos_of);
}

// ---- both maps of msfl_set_map through ONE chain of launches (round 6) -------------------------------------------------------
// The corner map (a few thousand points) and the surf map used to be indexed one after the other: ten launches and two 4-byte
// read-back copies in front of every batch, ~45 us of mostly launch-to-launch latency.  Here every launch serves both clouds
// (blocks [0, blocks0) the first, the rest the second), the two count tables sit back to back and are prefix-summed by ONE
// rocPRIM scan, and the scatter launch also writes each map's own cell table from the combined sums (the second map's minus the
// first map's total) and the grids' wanted size straight into pinned host memory.  Same descriptors, same tables, same sorted
// copies up to the (arbitrary, never observable) order inside a cell as two single builds.
struct GridPairJob {
  const float4* pts[2]; int n[2];
  int* bbox[2]; GridDesc* gdesc[2]; int cap[2];
  int* cell_of;              // [n[0] | n[1]]
  int* count;                // [cap[0] + 1 | cap[1] + 1], zero on entry, zero again on exit
  int* scanned;              // exclusive prefix sums of `count` over both tables (the scatter launch reads them)
  int* cell_start[2]; float4* sorted[2]; int* pos_of[2];
  int* want_host[2];         // pinned host words: cells the bounding box needs at the base cell edge (feedback for the next build)
  int blocks0;               // workgroups of the per-point launches that serve map 0
  int bbox_blocks0;          // the same for the bounding-box launch
  double radius;
};
__global__ void __launch_bounds__(256) grid_bbox_pair_kernel(GridPairJob j) {
  const int m = (int)blockIdx.x < j.bbox_blocks0 ? 0 : 1;
  const int block = m ? (int)blockIdx.x - j.bbox_blocks0 : (int)blockIdx.x;
  grid_bbox_body(j.pts[m], j.n[m], j.bbox[m], block, m ? (int)gridDim.x - j.bbox_blocks0 : j.bbox_blocks0);
}
__global__ void __launch_bounds__(256) grid_count_pair_kernel(GridPairJob j) {
  const int m = (int)blockIdx.x < j.blocks0 ? 0 : 1;
  const int block = m ? (int)blockIdx.x - j.blocks0 : (int)blockIdx.x;
  grid_count_body(j.pts[m], j.n[m], j.bbox[m], j.radius, j.cap[m], j.gdesc[m], j.cell_of + (m ? j.n[0] : 0), j.count + (m ? j.cap[0] + 1 : 0), block);
}
__global__ void __launch_bounds__(256) grid_scatter_pair_kernel(GridPairJob j) {
  const int t0 = j.cap[0] + 1, t_all = t0 + j.cap[1] + 1;
  const int base1 = j.scanned[t0];                         // = the first map's indexed points (its table's last entries count nothing)
  // (a) each map's own cell table, by every thread of the launch in turn
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < t_all; t += gridDim.x * blockDim.x) {
    if (t < t0) j.cell_start[0][t] = j.scanned[t];
    else j.cell_start[1][t - t0] = j.scanned[t] - base1;
  }
  // (b) the points
  const int m = (int)blockIdx.x < j.blocks0 ? 0 : 1;
  const int block = m ? (int)blockIdx.x - j.blocks0 : (int)blockIdx.x;
  const int i = block * blockDim.x + threadIdx.x;
  const int* scanned = j.scanned + (m ? t0 : 0);
  const int sub = m ? base1 : 0;
  if (i == 0) grid_build_done(j.gdesc[m], scanned[j.gdesc[m]->n_cells] - sub, j.want_host[m], j.bbox[m]);
  if (i >= j.n[m]) return;
  grid_scatter_point(j.pts[m] + i, i, (j.cell_of + (m ? j.n[0] : 0))[i], scanned, sub, j.count + (m ? t0 : 0), j.sorted[m], j.pos_of[m]);
}

// ---------------------------------------------------------------------------------------------
// The running best lists of the 5-NN walks
// ---------------------------------------------------------------------------------------------

// Running 5 best as packed 64-bit keys (f32 distance bits << 32 | original map index): distances
// are >= 0 so the bit pattern is monotone, and one unsigned compare realises the total order
// (distance, index).  Branch-free sorted insertion: 5 compares + 10 selects on register pairs.
struct Top5 {
  unsigned long long k0, k1, k2, k3, k4;
};

// Every slot starts at (bound, 0xffffffff): a result is only ACCEPTED when its 5th distance is below the
// reference's gate (< 1.0, mapping_scan_matcher.cc:128,198), so candidates at or beyond the gate can be
// dropped at the pre-filter and rows / end cells farther than it pruned from the first row on.  A query
// with fewer than five neighbours inside the gate keeps the sentinel in k4 and is rejected.
__device__ __forceinline__ void top5_init(Top5& t, float bound) {
  t.k0 = t.k1 = t.k2 = t.k3 = t.k4 = ((unsigned long long)__float_as_uint(bound) << 32) | 0xffffffffull;
}
__device__ __forceinline__ float top5_d4(const Top5& t) { return __uint_as_float((unsigned int)(t.k4 >> 32)); }  // the gate while < 5 found

// The inline assembly below (v_min_f64 / v_max_f64 / v_med3_u32 by their gfx950 mnemonics) is written for the one target this library
// has: a device pass for anything else stops here with a message instead of an assembler error deep in a template.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libmsfl_hip is written for gfx950 (MI355X) only: build with --offload-arch=gfx950"
#endif
// unsigned 64-bit min / max of two keys whose high words are < 2^31, on the f64 min / max unit (see top5_insert)
__device__ __forceinline__ unsigned long long u64_min_f(unsigned long long a, unsigned long long b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(__longlong_as_double((long long)a)), "v"(__longlong_as_double((long long)b)));
  return (unsigned long long)__double_as_longlong(r);
}
__device__ __forceinline__ unsigned long long u64_max_f(unsigned long long a, unsigned long long b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(__longlong_as_double((long long)a)), "v"(__longlong_as_double((long long)b)));
  return (unsigned long long)__double_as_longlong(r);
}
__device__ __forceinline__ void top5_insert(Top5& t, float d, int idx) {
  // cheap pre-filter on the distance word alone (a full-rate 32-bit compare; the bit pattern of a
  // non-negative float is monotone), then the exact 64-bit (distance, index) order
  if (__float_as_uint(d) > (unsigned int)(t.k4 >> 32)) return;
  const unsigned long long x = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)idx;
  if (!(x < t.k4)) return;
  // Sorted insertion as a min / max chain on the keys READ AS DOUBLES.  A key's high word is the bit pattern of a non-negative f32
  // (< 2^31), so as an f64 it is a non-negative finite number or denormal (exponent field = the top 11 bits of the f32 pattern:
  // <= 0x7fc even for an f32 NaN), and for non-negative doubles the IEEE order IS the unsigned order of the bit patterns; f64
  // denormals are preserved (the default f64 mode), min / max select one operand bit for bit.  8 instructions instead of
  // 5 x v_cmp_lt_u64 + 16 x v_cndmask_b32 (all of the 4-clock class): the insertion pass runs for the whole wavefront whenever one
  // lane inserts and was ~30 % of the kernel.
  const unsigned long long c0 = u64_max_f(t.k0, x); t.k0 = u64_min_f(t.k0, x);
  const unsigned long long c1 = u64_max_f(t.k1, c0); t.k1 = u64_min_f(t.k1, c0);
  const unsigned long long c2 = u64_max_f(t.k2, c1); t.k2 = u64_min_f(t.k2, c1);
  const unsigned long long c3 = u64_max_f(t.k3, c2); t.k3 = u64_min_f(t.k3, c2);
  t.k4 = c3;                    // = min(k4, c3): x < k4 (the guard above) and k3 <= k4, so the largest of {k0..k3, x} is below k4
}

// Round 4, the walk's own top list: SIX 32-bit keys (distance bits & ~7) | slot, sorted, and the candidates' positions in the
// sorted map kept per (slot, lane) in LDS.  A candidate that passes the pre-filter takes the slot of the key it can only evict
// (the 6th), stores its position there and goes through 1 x v_min_u32 + 5 x v_med3_u32 — ~45 clocks per insertion pass of the
// wavefront instead of ~78 for the 64-bit min / max chain above (the pass runs for all 64 lanes whenever one lane inserts:
// ~47 passes per wavefront).  The keys order candidates by their distance truncated to 29 bits (t = bits >> 3); the result is
// the exact top-5 by (distance, index) whenever the six final keys have six different t:
//  * a candidate dropped at the pre-filter had t > t(5th at that time) >= t(final 5th);
//  * every other candidate was offered to the list, which keeps the six smallest keys offered, so a candidate outside the final
//    top-5 with t == t(final 5th) implies t(final 6th) == t(final 5th);
//  * with different t the truncated order IS the order of the exact distances, and the index word is never consulted.
// A lane whose final keys show an equal-t neighbour pair (or whose 5th shares its t with the acceptance gate) is AMBIGUOUS and
// is searched again with the exact 64-bit keys (Top5): two distances within 2^-21 relative of each other, ~1e-6 of the queries
// on a scanned surface, every query on an exact lattice.  The 6th key's stored position may be stale (a candidate that tied
// with it overwrote the slot without entering); the 6th is never output and can only leave the list.
constexpr unsigned int kTopSentinel = 0xffffff00u;      // sentinels 0xffffff00 + 9 i: six different t, slots 0..5, above every f32 distance pattern
// k = med3(below, k, x) IN PLACE (below <= k): the sorted list's element after x has been inserted somewhere
__device__ __forceinline__ void u32_med3_into(unsigned int& k, unsigned int below, unsigned int x) {
  asm("v_med3_u32 %0, %1, %0, %2" : "+v"(k) : "v"(below), "v"(x));
}
struct Top6K {
  unsigned int k0, k1, k2, k3, k4, k5;
  unsigned int bound;               // min(k4 | 7, gate bits): the pre-filter, a conservative 5th distance for the row / cell bounds
  unsigned int gate;                // acceptance gate bits
  int* col;                         // this lane's column of the slot table: col[slot * kTopSlotStride]
};
constexpr int kTopSlots = 6;
__device__ __forceinline__ void top_init(Top6K& t, float bound, int* col) {
  t.k0 = kTopSentinel; t.k1 = kTopSentinel + 9; t.k2 = kTopSentinel + 18; t.k3 = kTopSentinel + 27; t.k4 = kTopSentinel + 36; t.k5 = kTopSentinel + 45;
  t.gate = __float_as_uint(bound); t.bound = t.gate; t.col = col;
}
__device__ __forceinline__ float top_d4(const Top6K& t) { return __uint_as_float(t.bound); }
// true: the five nearest and their order are decided by the truncated keys (see above); false: search again with Top5
__device__ __forceinline__ bool top_settled(const Top6K& t, float accept_gate) {
  const unsigned int amb = min(min(min(t.k0 ^ t.k1, t.k1 ^ t.k2), min(t.k2 ^ t.k3, t.k3 ^ t.k4)), min(t.k4 ^ t.k5, t.k4 ^ __float_as_uint(accept_gate)));
  return amb >= 8u;
}
__device__ __forceinline__ bool top_found(const Top6K& t) { return t.k4 < kTopSentinel; }     // five real candidates within the gate
template <int STRIDE>
__device__ __forceinline__ int top_pos(const Top6K& t, unsigned int k) { return (int)((unsigned int)t.col[(k & 7u) * STRIDE] >> 4); }   // stored: byte offset

// flann::L2_Simple<float>: ((dx*dx) + dy*dy) + dz*dz, every operation rounded to f32
__device__ __forceinline__ float l2_simple(float4 a, float3 q) {
  const float dx = a.x - q.x, dy = a.y - q.y, dz = a.z - q.z;
  float r = dx * dx;
  r = r + dy * dy;
  r = r + dz * dz;
  return r;
}
// the same arithmetic with x and y in one packed-f32 lane pair (v_pk_add_f32 / v_pk_mul_f32: two
// IEEE operations per instruction, individually rounded, so the result is bit-identical)
typedef float msfl_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float l2_simple_pk(float4 a, msfl_f2 qxy, float qz) {
  const msfl_f2 axy = {a.x, a.y};
  const msfl_f2 dxy = axy - qxy;
  const msfl_f2 sxy = dxy * dxy;
  const float dz = a.z - qz;
  float r = sxy.x + sxy.y;
  r = r + dz * dz;
  return r;
}

// ---------------------------------------------------------------------------------------------
// The query side.  A query's 27-cell neighbourhood is nine (y, z) rows of 2 * kGridXSub + 1 x-adjacent cells, each row ONE
// contiguous range of the sorted array.  A row / an end cell of a row is skipped when a LOWER BOUND of its distance to the
// query already exceeds the walk's pruning distance, so the result is identical to scanning all 27 cells.  The bound is
// shrunk by 1e-3 cell to stay conservative under the f32 rounding of cell coordinates (kGridMaxDim above).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float axis_gap(float u, int c) {
  // distance (in cell units) from coordinate u to the interval [c, c+1], minus slack, floored at 0
  const float g = fmaxf((float)c - u, u - (float)(c + 1));
  return fmaxf(g - 1e-3f, 0.0f);
}

struct GridQuery {
  float ux, uy, uz;   // the query in cell units from the grid's origin
  int cx, cy, cz;     // its cell (grid_coord: up to two cells outside the grid)
  int xs, xe;         // the x cells of its reach that exist; xs > xe: none, the query has no neighbour within the radius
};
__device__ __forceinline__ GridQuery grid_query(const GridDesc& g, float3 q) {
  GridQuery w;
  w.ux = (q.x - g.ox) * g.inv_cell_x; w.uy = (q.y - g.oy) * g.inv_cell; w.uz = (q.z - g.oz) * g.inv_cell;
  w.cx = grid_coord(q.x, g.ox, g.inv_cell_x, g.dx);
  w.cy = grid_coord(q.y, g.oy, g.inv_cell, g.dy);
  w.cz = grid_coord(q.z, g.oz, g.inv_cell, g.dz);
  w.xs = max(w.cx - kGridXSub, 0); w.xe = min(w.cx + kGridXSub, g.dx - 1);
  return w;
}
// squared lower bounds of the kGridXSub cells at the left (gxa, from xs) and the right end (gxb, from xe) of the reach, outermost
// first: they are the same for all nine rows, so the per-row trimming is two adds and two compares per side.  MONOTONE: a cell
// at or beyond the query's own cell (only where the grid's border cuts the reach short) gets 0, so the bounds never increase
// inwards and the leading run of cells out of reach can be COUNTED (knn5_grid_k32).
template <bool MONOTONE = false>
__device__ __forceinline__ void grid_x_bounds(const GridDesc& g, const GridQuery& w, float (&gxa)[kGridXSub], float (&gxb)[kGridXSub]) {
#pragma unroll
  for (int k = 0; k < kGridXSub; k++) {
    const float ga = axis_gap(w.ux, w.xs + k), gb = axis_gap(w.ux, w.xe - k);
    gxa[k] = !MONOTONE || w.xs + k < w.cx ? ga * ga * g.cellx2 : 0.0f;
    gxb[k] = !MONOTONE || w.xe - k > w.cx ? gb * gb * g.cellx2 : 0.0f;
  }
}

// Visit order of the 9 (dy, dz) rows, PER QUERY: centre, then the two side rows on the query's near sides (smaller
// gap first), the two far side rows, the near-near diagonal, the two mixed diagonals, the far-far diagonal.  Any
// order is exact (a row is only skipped on a lower bound); this one makes the 64 queries of a wavefront need the
// same loop POSITIONS: with a fixed (-y, +y, -z, +z) order each position ran for the ~19 lanes whose near side it
// happened to be and cost the longest of their ranges, now the first two positions carry nearly all of that work
// and the later ones are skipped by the whole wavefront; the pruning distance also tightens sooner.
struct GridRowOrder {
  float gy1, gz1;                 // gaps (cells) to the query's own row of cells: 0 unless the query lies outside the grid
  float g_ny, g_fy, g_nz, g_fz;   // gaps to the near (smaller gap) and far neighbour rows, per axis
  int sy, sz;                     // the near side's step, -1 or +1
  bool ny_first, fy_first;        // the y side row before the z side row, among the near / the far ones
  bool e_first;                   // (near y, far z) before (far y, near z)
};
__device__ __forceinline__ GridRowOrder grid_row_order(const GridQuery& w) {
  GridRowOrder o;
  const float gy0 = axis_gap(w.uy, w.cy - 1), gy2 = axis_gap(w.uy, w.cy + 1);
  const float gz0 = axis_gap(w.uz, w.cz - 1), gz2 = axis_gap(w.uz, w.cz + 1);
  o.gy1 = axis_gap(w.uy, w.cy); o.gz1 = axis_gap(w.uz, w.cz);
  const bool y_lo = gy0 <= gy2, z_lo = gz0 <= gz2;                 // near side: the smaller gap
  o.sy = y_lo ? -1 : 1; o.sz = z_lo ? -1 : 1;
  o.g_ny = y_lo ? gy0 : gy2; o.g_fy = y_lo ? gy2 : gy0;
  o.g_nz = z_lo ? gz0 : gz2; o.g_fz = z_lo ? gz2 : gz0;
  o.ny_first = o.g_ny <= o.g_nz; o.fy_first = o.g_fy <= o.g_fz;
  o.e_first = o.g_ny * o.g_ny + o.g_fz * o.g_fz <= o.g_fy * o.g_fy + o.g_nz * o.g_nz;
  return o;
}

// The exact walk: every candidate that can lie within bound() of q is handed to scan.  bound() is the caller's current pruning
// distance (squared, f32; it may only shrink), scan(s, e) takes the positions [s, e) of the sorted array and may tighten it.
template <class Bound, class Scan>
__device__ __forceinline__ void grid_walk_exact(const GridDesc& g, const int* __restrict__ cell_start, float3 q, Bound bound, Scan scan) {
  const GridQuery w = grid_query(g, q);
  if (w.xs > w.xe) return;
  const GridRowOrder o = grid_row_order(w);
  float gxa[kGridXSub], gxb[kGridXSub];
  grid_x_bounds(g, w, gxa, gxb);
  const int sy = o.sy, sz = o.sz;
#pragma unroll
  for (int r = 0; r < 9; r++) {
    int dy, dz; float gy, gz;
    if (r == 0) { dy = 0; dz = 0; gy = o.gy1; gz = o.gz1; }
    else if (r == 1 || r == 2) {                                    // near side rows
      const bool yrow = (r == 1) == o.ny_first;
      dy = yrow ? sy : 0; dz = yrow ? 0 : sz; gy = yrow ? o.g_ny : o.gy1; gz = yrow ? o.gz1 : o.g_nz;
    } else if (r == 3 || r == 4) {                                  // far side rows
      const bool yrow = (r == 3) == o.fy_first;
      dy = yrow ? -sy : 0; dz = yrow ? 0 : -sz; gy = yrow ? o.g_fy : o.gy1; gz = yrow ? o.gz1 : o.g_fz;
    } else if (r == 5) { dy = sy; dz = sz; gy = o.g_ny; gz = o.g_nz; }
    else if (r == 6 || r == 7) {                                    // mixed diagonals
      const bool e = (r == 6) == o.e_first;                         // e: (near y, far z)
      dy = e ? sy : -sy; dz = e ? -sz : sz; gy = e ? o.g_ny : o.g_fy; gz = e ? o.g_fz : o.g_nz;
    } else { dy = -sy; dz = -sz; gy = o.g_fy; gz = o.g_fz; }
    const int y = w.cy + dy, z = w.cz + dz;
    if (y < 0 || y >= g.dy || z < 0 || z >= g.dz) continue;
    const float row2 = (gy * gy + gz * gz) * g.cell2;
    const int row = (z * g.dy + y) * g.dx;
    const float d = bound();
    if (row2 > d) continue;
    // trim the x range: a cell is dropped when its lower bound exceeds d; the bounds shrink towards the query, so count the
    // leading run of dropped cells on each side
    int a = w.xs, b = w.xe;
    bool da = true, db = true;
#pragma unroll
    for (int k = 0; k < kGridXSub; k++) {
      da = da && (row2 + gxa[k] > d); a += da ? 1 : 0;
      db = db && (row2 + gxb[k] > d); b -= db ? 1 : 0;
    }
    if (a > b) continue;                      // only near the grid border: every remaining cell is out of reach
    scan(cell_start[row + a], cell_start[row + b + 1]);
  }
}

// Exact 5-NN on 64-bit keys (Top5, initialised by the caller with the acceptance gate, which prunes until five neighbours are
// known): the search again of a query that the truncated-key walk below (knn5_grid_k32) leaves ambiguous.
__device__ __forceinline__ void knn5_grid(const GridDesc& g, const float4* __restrict__ sorted,
                                          const int* __restrict__ cell_start, float3 q, Top5& t,
                                          int& n_cand) {      // n_cand: candidates evaluated (dead code unless the caller reads it)
  const msfl_f2 qxy = {q.x, q.y};
  grid_walk_exact(g, cell_start, q, [&]() __attribute__((always_inline)) { return top5_d4(t); },
                  [&](int s, int e) __attribute__((always_inline)) {
    n_cand += e - s;
    const float4* p = sorted + s;
    const float4* const pe = sorted + e;
    for (; p + 1 < pe; p += 2) {            // two loads in flight, one address register
      float4 m0 = p[0], m1 = p[1];
      // keep the index word in the 16-byte load: left alone, the compiler splits it off into a second,
      // dependent load inside the (latency-critical) insertion path
      asm volatile("" : "+v"(m0.w));
      top5_insert(t, l2_simple_pk(m0, qxy, q.z), __float_as_int(m0.w));
      asm volatile("" : "+v"(m1.w));
      top5_insert(t, l2_simple_pk(m1, qxy, q.z), __float_as_int(m1.w));
    }
    if (p < pe) { float4 m = p[0]; asm volatile("" : "+v"(m.w)); top5_insert(t, l2_simple_pk(m, qxy, q.z), __float_as_int(m.w)); }
  });
}

// The same walk for Top6K, written for the instruction count (the kernel is VALU-issue bound: every wave instruction of a
// visited row is paid 64 lanes wide).  Differences to knn5_grid, none of which changes the result:
//  * candidates are addressed by 32-bit BYTE offsets from the (scalar) map base (saddr loads, 32-bit loop control; a map is
//    < 2^28 points: msfl_set_map refuses more) and the slot table stores the byte offset (position = offset >> 4 at the end);
//  * a row's end cells are trimmed by COUNTING the cells whose bound exceeds (5th distance - row bound): the per-side bounds
//    are made monotone at set-up (a cell at or beyond the query's own cell gets 0), so the count is the leading run;
//  * row validity (y, z inside the grid) and the row bases come from six set-up compares / two offsets instead of four
//    compares and two 32-bit multiplies per row.
template <int STRIDE>
__device__ __forceinline__ void top_insert_off(Top6K& t, float d, unsigned int off) {
  const unsigned int db = __float_as_uint(d);
  if (db > t.bound) return;
  const unsigned int slot = t.k5 & 7u;
  const unsigned int x = (db & ~7u) | slot;
  t.col[slot * STRIDE] = (int)off;
  u32_med3_into(t.k5, t.k4, x); u32_med3_into(t.k4, t.k3, x); u32_med3_into(t.k3, t.k2, x);
  u32_med3_into(t.k2, t.k1, x); u32_med3_into(t.k1, t.k0, x);
  t.k0 = min(t.k0, x);
  t.bound = min(t.k4 | 7u, t.gate);
}
// DEFER (the whole-batch kernel; docs/kernels/scan2map.md, "Capped row visits"): a row visit walks at most kDeferCaps[position]
// pair-iterations; the lane pushes the rest of its range, {start, end} as byte offsets, onto a stack of kDeferDepth entries in LDS
// (layout [entry][word][lane] right after its column of the slot table: t.col + kTopSlots * STRIDE) and goes on to the next row.
// After the ninth row one loop walks the stored ranges.  A position then costs the wavefront min(longest range, cap) iterations,
// and the long lanes of different positions, which are different lanes, catch up side by side.  A full stack walks the range in
// place.  The candidates offered are those of the plain walk or more (a stored range was cut under a bound no smaller than any
// later one), so the lists are the plain walk's, bit for bit.
#ifndef MSFL_KNN_DEFER_CAPS
#define MSFL_KNN_DEFER_CAPS 8, 4, 4, 1, 1, 1, 1, 1, 1
#endif
#ifndef MSFL_KNN_DEFER_DEPTH
#define MSFL_KNN_DEFER_DEPTH 4
#endif
#ifndef MSFL_KNN_DEFER_FLAT
#define MSFL_KNN_DEFER_FLAT 1         // 1: one flat loop over a lane's stored ranges; 0: entry by entry (the k-th range of every lane together)
#endif
constexpr int kDeferCaps[9] = {MSFL_KNN_DEFER_CAPS};   // pair-iterations per row position, in visit order
constexpr int kDeferDepth = MSFL_KNN_DEFER_DEPTH;
constexpr int kDeferSlots = 2 * kDeferDepth;           // LDS dwords per lane
template <int STRIDE, bool DEFER = false>
__device__ __forceinline__ void knn5_grid_k32(const GridDesc& g, const float4* __restrict__ sorted,
                                              const int* __restrict__ cell_start, float3 q, Top6K& t, int& n_cand,
                                              int cell_base = 0) {        // cell_base: this map's slice of a shared cell table (pairs)
  const GridQuery w = grid_query(g, q);
  const int cy = w.cy, cz = w.cz, xs = w.xs, xe = w.xe;
  if (xs > xe) return;
  const float cell2 = g.cell2;
  float gxa[kGridXSub], gxb[kGridXSub];       // outermost first, non-increasing
  grid_x_bounds<true>(g, w, gxa, gxb);
  const msfl_f2 qxy = {q.x, q.y};
  const GridRowOrder o = grid_row_order(w);
  const float q_ny = o.g_ny * o.g_ny, q_fy = o.g_fy * o.g_fy, q_nz = o.g_nz * o.g_nz, q_fz = o.g_fz * o.g_fz, q_y1 = o.gy1 * o.gy1, q_z1 = o.gz1 * o.gz1;
  // validity of the three y and three z cell coordinates, near / centre / far
  const int sy = o.sy, sz = o.sz;
  const bool v_y1 = (unsigned int)cy < (unsigned int)g.dy, v_ny = (unsigned int)(cy + sy) < (unsigned int)g.dy, v_fy = (unsigned int)(cy - sy) < (unsigned int)g.dy;
  const bool v_z1 = (unsigned int)cz < (unsigned int)g.dz, v_nz = (unsigned int)(cz + sz) < (unsigned int)g.dz, v_fz = (unsigned int)(cz - sz) < (unsigned int)g.dz;
  const int base0 = (cz * g.dy + cy) * g.dx + cell_base;           // only used where the row is valid
  const int off_y = sy < 0 ? -g.dx : g.dx;                         // near-side steps
  const int zstep = g.dy * g.dx;
  const int off_z = sz < 0 ? -zstep : zstep;
  const char* const mapb = (const char*)sorted;
  int* const stack = t.col + kTopSlots * STRIDE;         // DEFER: this lane's stack, entry k at stack[2 k STRIDE] (start) and [(2 k + 1) STRIDE] (end)
  int* sp = stack;                                        // next free entry
  auto visit = [&](int pos, bool valid, int row, float rowq) __attribute__((always_inline)) {
    const float row2 = rowq * cell2;
    const float d4 = top_d4(t);
    if (!valid || row2 > d4) return;           // d4: the acceptance gate until five neighbours are known, then >= the 5th distance
    const float room = d4 - row2;
    int a = xs, b = xe;
#pragma unroll
    for (int k = 0; k < kGridXSub; k++) { a += gxa[k] > room ? 1 : 0; b -= gxb[k] > room ? 1 : 0; }
    if (a > b) return;
    const unsigned int s = (unsigned int)cell_start[(unsigned int)(row + a)], e = (unsigned int)cell_start[(unsigned int)(row + b + 1)];
    if (s == e) return;
    unsigned int off = s << 4;
    unsigned int end = e << 4;
    if constexpr (DEFER) {
      const unsigned int cut = off + 32u * (unsigned int)kDeferCaps[pos];
      if (end > cut && sp < stack + kDeferSlots * STRIDE) {       // longer than the cap and room on the stack: the rest waits
        sp[0] = (int)cut; sp[STRIDE] = (int)end; sp += 2 * STRIDE;
        end = cut;
      }
      n_cand += (int)((end - off) >> 4);
    } else {
      n_cand += (int)(e - s);
    }
    const unsigned int last = end - 16u;       // last: offset of the range's last point (>= off)
    for (; off < last; off += 32u) {           // two loads in flight
      float4 m0 = *(const float4*)(mapb + off), m1 = *(const float4*)(mapb + off + 16u);
      asm volatile("" : "+v"(m0.w));           // keep the 16-byte loads (12-byte loads: slower in rounds 1-2, no change in round 4b)
      top_insert_off<STRIDE>(t, l2_simple_pk(m0, qxy, q.z), off);
      asm volatile("" : "+v"(m1.w));
      top_insert_off<STRIDE>(t, l2_simple_pk(m1, qxy, q.z), off + 16u);
    }
    if (off < end) { float4 m = *(const float4*)(mapb + off); asm volatile("" : "+v"(m.w)); top_insert_off<STRIDE>(t, l2_simple_pk(m, qxy, q.z), off); }
  };
  // the row order of grid_walk_exact: centre, near sides (smaller gap first), far sides, near-near, mixed diagonals, far-far
  visit(0, v_y1 && v_z1, base0, q_y1 + q_z1);
  {
    const bool va = v_ny && v_z1, vb = v_y1 && v_nz;               // A: near-y side row, B: near-z side row
    const float ra = q_ny + q_z1, rb = q_y1 + q_nz;
    visit(1, o.ny_first ? va : vb, base0 + (o.ny_first ? off_y : off_z), o.ny_first ? ra : rb);
    visit(2, o.ny_first ? vb : va, base0 + (o.ny_first ? off_z : off_y), o.ny_first ? rb : ra);
  }
  {
    const bool va = v_fy && v_z1, vb = v_y1 && v_fz;
    const float ra = q_fy + q_z1, rb = q_y1 + q_fz;
    visit(3, o.fy_first ? va : vb, base0 - (o.fy_first ? off_y : off_z), o.fy_first ? ra : rb);
    visit(4, o.fy_first ? vb : va, base0 - (o.fy_first ? off_z : off_y), o.fy_first ? rb : ra);
  }
  visit(5, v_ny && v_nz, base0 + off_y + off_z, q_ny + q_nz);
  {
    const bool va = v_ny && v_fz, vb = v_fy && v_nz;               // A: (near y, far z)
    const float ra = q_ny + q_fz, rb = q_fy + q_nz;
    const int oa = off_y - off_z, ob = off_z - off_y;
    visit(6, o.e_first ? va : vb, base0 + (o.e_first ? oa : ob), o.e_first ? ra : rb);
    visit(7, o.e_first ? vb : va, base0 + (o.e_first ? ob : oa), o.e_first ? rb : ra);
  }
  visit(8, v_fy && v_fz, base0 - off_y - off_z, q_fy + q_fz);
  if constexpr (DEFER) {
    // the stored ranges, in stack order
    if (MSFL_KNN_DEFER_FLAT) {
      // one loop: a lane that has finished a range takes its next one in the same iteration, so the trip count is the longest lane's SUM.
      // An odd range's last iteration loads its last point twice and offers the copy with a key that the pre-filter always refuses.
      unsigned int off = 0, end = 0;
      for (const int* rp = stack;; off += 32u) {
        if (off >= end) {
          if (rp >= sp) break;
          off = (unsigned int)rp[0]; end = (unsigned int)rp[STRIDE]; rp += 2 * STRIDE;
          n_cand += (int)((end - off) >> 4);
        }
        const bool two = off + 16u < end;
        const unsigned int off1 = two ? off + 16u : off;
        float4 m0 = *(const float4*)(mapb + off), m1 = *(const float4*)(mapb + off1);
        asm volatile("" : "+v"(m0.w));
        top_insert_off<STRIDE>(t, l2_simple_pk(m0, qxy, q.z), off);
        asm volatile("" : "+v"(m1.w));
        top_insert_off<STRIDE>(t, two ? l2_simple_pk(m1, qxy, q.z) : __uint_as_float(0xffffffffu), off1);
      }
    } else {
      // entry by entry: the k-th stored range of every lane together, with the row visit's own loop
      for (const int* rp = stack; rp < sp; rp += 2 * STRIDE) {
        unsigned int off = (unsigned int)rp[0];
        const unsigned int end = (unsigned int)rp[STRIDE], last = end - 16u;
        n_cand += (int)((end - off) >> 4);
        for (; off < last; off += 32u) {
          float4 m0 = *(const float4*)(mapb + off), m1 = *(const float4*)(mapb + off + 16u);
          asm volatile("" : "+v"(m0.w));
          top_insert_off<STRIDE>(t, l2_simple_pk(m0, qxy, q.z), off);
          asm volatile("" : "+v"(m1.w));
          top_insert_off<STRIDE>(t, l2_simple_pk(m1, qxy, q.z), off + 16u);
        }
        if (off < end) { float4 m = *(const float4*)(mapb + off); asm volatile("" : "+v"(m.w)); top_insert_off<STRIDE>(t, l2_simple_pk(m, qxy, q.z), off); }
      }
    }
  }
}

}  // namespace msfl
