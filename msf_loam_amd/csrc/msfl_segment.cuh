// msfl_segment.cuh — scan segmentation in front of the extraction (docs/kernels/segment.md): every sweep of a batch is laid into its
// range image, the ground goes by the slope between neighbouring beams, the rest is connected into clusters by an angle test between
// neighbouring pixels, and every input point gets a class.  After LeGO-LOAM's image projection; not in the reference.
//
//   seg_clear_kernel     the images of one chunk of scans: winner keys empty, every pixel its own parent, statistics and counters zero
//   seg_fill_kernel      one lane per point: its pixel, a 64-bit integer minimum on (bits(r), index in the scan)
//   seg_ground_kernel    one lane per pixel pair (k, k+1) of a column: both ground iff the slope of the winners' difference is small
//   seg_union_kernel     one lane per pixel, its left and its upper edge: lock-free union-find, the larger root hooked onto the smaller;
//                        the run of connected pixels inside a wavefront hooks onto its first lane directly
//   seg_flatten_kernel   one lane per pixel: its root (nothing written on the way), the root's pixel count and 128-bit row mask, one
//                        add and one OR per (root, row) of a wavefront
//   seg_classify_kernel  one lane per point: class, component id, masked copy; class counts by ballot, one atomic per wavefront
//   seg_finish_kernel    one lane per scan: the info record
//
// blockIdx.y is the scan inside the chunk in every kernel, so a wavefront never spans two scans.  A pixel is found by f32 compares
// against host-built tables (the convention of msfl_place.cuh and carve_pixel: no atan2); a minimum, an OR and an integer sum do not
// depend on order and a component's id is its smallest pixel, so the result does not depend on the launch shape or the schedule.
// No kernel waits for a value another workgroup has yet to write: a parent index only ever decreases, so every walk ends by itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msfl {

constexpr int kSegMaxCol = 2048;
constexpr int kSegMaxRow = 128;
constexpr int kSegBlock = 256;
constexpr int kSegMaxTab = kSegMaxCol + 2 * (kSegMaxRow - 1);      // cc, cs [n_col / 2 each], vs, vc [n_row - 1 each]
constexpr unsigned long long kSegEmpty = ~0ull;                    // a pixel without a winner
constexpr int kSegPixelBytes = 8 + 4 * 4 + 16;                     // key, ground, parent, label, count, row mask
enum { SEG_NONE = 0, SEG_SHADOWED, SEG_GROUND, SEG_SEGMENT, SEG_OUTLIER, SEG_CLASSES };
// counters of one scan of the chunk in flight
enum { SEG_CTR_PIXELS = SEG_CLASSES, SEG_CTR_COMPONENTS, SEG_CTR_SEGMENTS, SEG_CTR_WORDS };
// msfl_segment_info, 10 ints
enum { SEG_INFO_PIXELS = SEG_CLASSES, SEG_INFO_COMPONENTS, SEG_INFO_SEGMENTS, SEG_INFO_KEPT, SEG_INFO_RESERVED, SEG_INFO_WORDS };

// The configuration as the kernels see it.  tab: cc[n_col / 2], cs[n_col / 2], vs[n_row - 1], vc[n_row - 1] (f32, built by the host in double).
struct SegCfg {
  int n_col, n_row, ground_rows;
  int min_points, min_points_tall, min_rows_tall, keep;
  float min_range, max_range;
  float up[3];
  float hs, hc, g2, t;
  const float* tab;
};

// The images of one chunk, `scans` of them back to back in every array.
struct SegImages {
  unsigned long long* key;     // (bits(r) << 32) | index in the scan of the pixel's winner
  int* ground;                 // 1: a ground pixel
  int* parent;                 // union-find, pixel indices inside the image
  int* label;                  // the root of a pixel that takes part, else -1
  int* count;                  // at a root: pixels of the component
  unsigned* rows;              // at a root: 4 words, bit `row` set when the component touches the row
  int* ctr;                    // SEG_CTR_WORDS per scan
};

__host__ __device__ inline int seg_tab_size(int n_col, int n_row) { return n_col + 2 * (n_row - 1); }

// Pixel (row * n_col + col) and range of a sensor point; false: the point has no pixel.  cc, cs: the column boundaries (LDS).  The
// bisection keeps "the boundary test holds at lo and fails at hi" and IS the definition (the model runs the same steps).
__device__ __forceinline__ bool seg_pixel(const SegCfg& c, const float* __restrict__ cc, const float* __restrict__ cs, float x, float y, float z,
                                          unsigned ring, float& r, int& pix) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  const float rho2 = x * x + y * y;
  if (rho2 == 0.f) return false;
  r = sqrtf(rho2 + z * z);                             // correctly rounded in this build, as in carve_pixel
  if (!(r >= c.min_range) || r > c.max_range) return false;
  if (ring >= (unsigned)c.n_row) return false;
  const int half = c.n_col >> 1;
  const float t0 = cc[0] * y - cs[0] * x, u0 = cc[0] * x + cs[0] * y;
  const bool upper = t0 > 0.f || (t0 == 0.f && u0 > 0.f);
  const float xp = upper ? x : -x, yp = upper ? y : -y;
  int lo = 0, hi = half;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cc[mid] * yp - cs[mid] * xp >= 0.f) lo = mid; else hi = mid;
  }
  pix = (int)ring * c.n_col + lo + (upper ? 0 : half);
  return true;
}

__device__ __forceinline__ void seg_load_cols(const SegCfg& c, float* __restrict__ s_tab) {
  for (int i = threadIdx.x; i < c.n_col; i += blockDim.x) s_tab[i] = c.tab[i];
}

// ---- 1: clear -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock)
seg_clear_kernel(SegImages im, int npix) {
  const size_t base = (size_t)blockIdx.y * (size_t)npix;
  const int i = blockIdx.x * kSegBlock + threadIdx.x;
  if (i < npix) {
    im.key[base + i] = kSegEmpty;
    im.ground[base + i] = 0;
    im.parent[base + i] = i;
    im.count[base + i] = 0;
    reinterpret_cast<uint4*>(im.rows)[base + i] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (blockIdx.x == 0 && threadIdx.x < SEG_CTR_WORDS) im.ctr[blockIdx.y * SEG_CTR_WORDS + threadIdx.x] = 0;
}

// ---- 2: fill ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock)
seg_fill_kernel(SegCfg c, SegImages im, const float4* __restrict__ pts, const uint16_t* __restrict__ ring, const int* __restrict__ off, int scan0) {
  __shared__ float s_tab[kSegMaxCol];
  seg_load_cols(c, s_tab);
  __syncthreads();
  const int o = off[scan0 + blockIdx.y], n = off[scan0 + blockIdx.y + 1] - o;
  unsigned long long* key = im.key + (size_t)blockIdx.y * (size_t)(c.n_col * c.n_row);
  for (int i = blockIdx.x * kSegBlock + threadIdx.x; i < n; i += gridDim.x * kSegBlock) {
    const float4 p = pts[(size_t)o + i];
    float r; int pix;
    if (seg_pixel(c, s_tab, s_tab + (c.n_col >> 1), p.x, p.y, p.z, ring[(size_t)o + i], r, pix))
      atomicMin(&key[pix], ((unsigned long long)__float_as_uint(r) << 32) | (unsigned)i);      // r > 0: the unsigned order is the float order
  }
}

// ---- 3: ground --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock)
seg_ground_kernel(SegCfg c, SegImages im, const float4* __restrict__ pts, const int* __restrict__ off, int scan0) {
  const int idx = blockIdx.x * kSegBlock + threadIdx.x;
  if (idx >= c.ground_rows * c.n_col) return;
  const size_t base = (size_t)blockIdx.y * (size_t)(c.n_col * c.n_row);
  const int lo = idx, hi = idx + c.n_col;                                 // idx = k * n_col + col is the lower pixel itself
  const unsigned long long ka = im.key[base + lo], kb = im.key[base + hi];
  if (ka == kSegEmpty || kb == kSegEmpty) return;
  const size_t o = (size_t)off[scan0 + blockIdx.y];
  const float4 a = pts[o + (unsigned)ka], b = pts[o + (unsigned)kb];
  const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  const float v = ((c.up[0] * dx) + (c.up[1] * dy)) + (c.up[2] * dz);
  const float n2 = ((dx * dx) + (dy * dy)) + (dz * dz);
  if (v * v <= c.g2 * n2) { im.ground[base + lo] = 1; im.ground[base + hi] = 1; }      // every writer stores the same value
}

// ---- 4: union ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int seg_peek(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x as of some moment during the call.  Every value a parent word ever held is a member of x's component smaller than
// its owner (or the owner itself, while it is a root), so x strictly decreases and the walk ends.  Path halving by atomicMin.
__device__ __forceinline__ int seg_find(int* __restrict__ parent, int x) {
  int p = seg_peek(&parent[x]);
  while (p != x) {
    const int gp = seg_peek(&parent[p]);
    if (gp != p) atomicMin(&parent[x], gp);
    x = p; p = gp;
  }
  return x;
}

// Hook the larger root onto the smaller one.  The atomic returns what the larger one's parent word held: itself, and the hook stands;
// or it had been hooked meanwhile, its word now holds the smaller of the two, and what it pointed to is united with the other side.
// max(a, b) strictly decreases from one round to the next.
__device__ __forceinline__ void seg_unite(int* __restrict__ parent, int a, int b) {
  for (;;) {
    a = seg_find(parent, a);
    b = seg_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

__device__ __forceinline__ bool seg_connected(float ra, float rb, float s, float co, float t) {
  const float d1 = fmaxf(ra, rb), d2 = fminf(ra, rb);
  return d2 * s > t * (d1 - d2 * co);
}

__global__ void __launch_bounds__(kSegBlock)
seg_union_kernel(SegCfg c, SegImages im) {
  const int npix = c.n_col * c.n_row;
  const int p = blockIdx.x * kSegBlock + threadIdx.x;
  const size_t base = (size_t)blockIdx.y * (size_t)npix;
  const int lane = threadIdx.x & 63;
  int* parent = im.parent + base;
  // The edge to the LEFT neighbour (the same set of edges as every pixel's right one).  Inside a wavefront the pixels of one row are
  // consecutive lanes: a lane whose left edge holds and whose left neighbour is the lane before it belongs to that lane's run, and
  // hooks onto the run's first lane directly (a star per run instead of a chain along the row).  The first lane of a run keeps its
  // left edge as it is: the neighbour lies in another wavefront, or across the turn.
  bool takes_part = false, left = false;
  unsigned long long kp = kSegEmpty;
  int row = 0, col = 0, ql = 0;
  if (p < npix) {
    kp = im.key[base + p];
    takes_part = kp != kSegEmpty && !im.ground[base + p];
    row = p / c.n_col; col = p - row * c.n_col;
    ql = col == 0 ? p + c.n_col - 1 : p - 1;
    if (takes_part) {
      const unsigned long long kq = im.key[base + ql];
      left = kq != kSegEmpty && !im.ground[base + ql] &&
             seg_connected(__uint_as_float((unsigned)(kp >> 32)), __uint_as_float((unsigned)(kq >> 32)), c.hs, c.hc, c.t);
    }
  }
  const bool in_run = left && col != 0 && lane != 0;
  const unsigned long long starts = __ballot(!in_run);                       // lane 0 is always one
  if (!takes_part) return;
  const float rp = __uint_as_float((unsigned)(kp >> 32));
  if (in_run) {
    const int first = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
    seg_unite(parent, p, p - (lane - first));
  } else if (left) {
    seg_unite(parent, p, ql);
  }
  if (row + 1 < c.n_row) {
    const int q = p + c.n_col;
    const unsigned long long kq = im.key[base + q];
    const float* vs = c.tab + c.n_col;
    const float* vc = vs + (c.n_row - 1);
    if (kq != kSegEmpty && !im.ground[base + q] && seg_connected(rp, __uint_as_float((unsigned)(kq >> 32)), vs[row], vc[row], c.t)) seg_unite(parent, p, q);
  }
}

// ---- 5: flatten + statistics -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock)
seg_flatten_kernel(SegCfg c, SegImages im) {
  const int npix = c.n_col * c.n_row;
  const int p = blockIdx.x * kSegBlock + threadIdx.x;
  const size_t base = (size_t)blockIdx.y * (size_t)npix;
  bool occupied = false, is_root = false, takes_part = false;
  int root = -1, row = 0;
  if (p < npix) {
    occupied = im.key[base + p] != kSegEmpty;
    takes_part = occupied && !im.ground[base + p];
    if (takes_part) {
      const int* parent = im.parent + base;
      root = p;
      for (int q = parent[root]; q != root; q = parent[root]) root = q;     // the union kernel is done: plain loads, nothing written
      is_root = root == p;
      row = p / c.n_col;
    }
    im.label[base + p] = root;
  }
  // one add and one OR per (root, row) of the wavefront, not per pixel: its pixels are neighbours in a row and mostly share both
  unsigned long long todo = __ballot(takes_part);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lroot = __shfl(root, leader), lrow = __shfl(row, leader);
    const unsigned long long same = __ballot(takes_part && root == lroot && row == lrow);
    if ((threadIdx.x & 63) == leader) {
      atomicAdd(&im.count[base + lroot], __popcll(same));
      atomicOr(&im.rows[4 * (base + lroot) + (lrow >> 5)], 1u << (lrow & 31));
    }
    todo &= ~same;
  }
  const unsigned long long bo = __ballot(occupied), br = __ballot(is_root);
  if ((threadIdx.x & 63) == 0) {
    if (bo) atomicAdd(&im.ctr[blockIdx.y * SEG_CTR_WORDS + SEG_CTR_PIXELS], __popcll(bo));
    if (br) atomicAdd(&im.ctr[blockIdx.y * SEG_CTR_WORDS + SEG_CTR_COMPONENTS], __popcll(br));
  }
}

// ---- 6: classify ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock)
seg_classify_kernel(SegCfg c, SegImages im, const float4* __restrict__ pts, const uint16_t* __restrict__ ring, const int* __restrict__ off, int scan0,
                    uint8_t* __restrict__ cls_out, int* __restrict__ segment_out, float4* __restrict__ masked_out) {
  __shared__ float s_tab[kSegMaxCol];
  seg_load_cols(c, s_tab);
  __syncthreads();
  const int o = off[scan0 + blockIdx.y], n = off[scan0 + blockIdx.y + 1] - o;
  const size_t base = (size_t)blockIdx.y * (size_t)(c.n_col * c.n_row);
  int tally[SEG_CLASSES + 1] = {0, 0, 0, 0, 0, 0};                        // per wavefront (every lane holds the same): classes, then segments
  for (int first = blockIdx.x * kSegBlock; first < n; first += gridDim.x * kSegBlock) {
    const int i = first + threadIdx.x;
    int cls = -1, seg = -1;
    bool counts_segment = false;
    if (i < n) {
      const float4 p = pts[(size_t)o + i];
      float r; int pix;
      cls = SEG_NONE;
      if (seg_pixel(c, s_tab, s_tab + (c.n_col >> 1), p.x, p.y, p.z, ring[(size_t)o + i], r, pix)) {
        if (im.key[base + pix] != (((unsigned long long)__float_as_uint(r) << 32) | (unsigned)i)) cls = SEG_SHADOWED;
        else if (im.ground[base + pix]) cls = SEG_GROUND;
        else {
          seg = im.label[base + pix];
          const int cnt = im.count[base + seg];
          const uint4 m = reinterpret_cast<const uint4*>(im.rows)[base + seg];
          const int nrows = __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
          const bool valid = cnt >= c.min_points || (cnt >= c.min_points_tall && nrows >= c.min_rows_tall);
          cls = valid ? SEG_SEGMENT : SEG_OUTLIER;
          counts_segment = valid && seg == pix;                              // a root pixel has exactly one winner
        }
      }
      cls_out[(size_t)o + i] = (uint8_t)cls;
      if (segment_out) segment_out[(size_t)o + i] = seg;
      if (masked_out) {
        float4 q = p;
        if (!((c.keep >> cls) & 1)) { const float nan = __uint_as_float(0x7fc00000u); q.x = nan; q.y = nan; q.z = nan; }
        masked_out[(size_t)o + i] = q;
      }
    }
#pragma unroll
    for (int k = 0; k < SEG_CLASSES; k++) tally[k] += __popcll(__ballot(cls == k));
    tally[SEG_CLASSES] += __popcll(__ballot(counts_segment));
  }
  if ((threadIdx.x & 63) == 0) {
    int* ctr = im.ctr + blockIdx.y * SEG_CTR_WORDS;
#pragma unroll
    for (int k = 0; k < SEG_CLASSES; k++) if (tally[k]) atomicAdd(&ctr[k], tally[k]);
    if (tally[SEG_CLASSES]) atomicAdd(&ctr[SEG_CTR_SEGMENTS], tally[SEG_CLASSES]);
  }
}

// ---- 7: finish --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock)
seg_finish_kernel(const int* __restrict__ ctr, int n_chunk, int keep, int* __restrict__ info) {
  const int s = blockIdx.x * kSegBlock + threadIdx.x;
  if (s >= n_chunk) return;
  const int* c = ctr + s * SEG_CTR_WORDS;
  int* out = info + s * SEG_INFO_WORDS;
  int kept = 0;
  for (int k = 0; k < SEG_CLASSES; k++) { out[k] = c[k]; if ((keep >> k) & 1) kept += c[k]; }
  out[SEG_INFO_PIXELS] = c[SEG_CTR_PIXELS];
  out[SEG_INFO_COMPONENTS] = c[SEG_CTR_COMPONENTS];
  out[SEG_INFO_SEGMENTS] = c[SEG_CTR_SEGMENTS];
  out[SEG_INFO_KEPT] = kept;
  out[SEG_INFO_RESERVED] = 0;
}

}  // namespace msfl
