// msfl_carve.cuh — the map store's visibility check (docs/kernels/grid_store.md, "Carve"): one scan, taken from a known pose,
// removes every stored point it sees through.  HybridGrid never removes anything (hybrid_grid.cc:462-534); this is beyond it.
//
//   carve_fill_kernel     the scan's range image: per pixel the minimum range, a 32-bit integer minimum on the bit pattern
//   carve_limit_kernel    the limit image: 0 where the centre pixel is empty, else the minimum of the range image over a window
//   carve_count_kernel    one workgroup per candidate cell: how many of its points the scan sees through (culled cells: none)
//   carve_scan_kernel     one workgroup: rank among the surviving cells, offset among the removed points (rocPRIM beyond 2^17 cells)
//   carve_apply_kernel    the table into the other buffer; per carved cell a stable in-place compaction of its slab in chunks of one
//                         workgroup, the removed points to their place in msfl_grid_dump order.  Refused: the table is carried over.
//   carve_finish_kernel   one thread: fold the counts into GridState, write the info record and the report
//
// A pixel is found by f32 compares against host-built tables (the convention of msfl_place.cuh: no atan2), every decision is
// a function of the point alone and a minimum does not depend on order, so the result does not depend on the launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msfl_grid.cuh"

namespace msfl {

constexpr int kCarveMaxCol = 2048;
constexpr int kCarveMaxRow = 128;
constexpr int kCarveMaxWindow = 4;
constexpr int kCarveBlock = 256;                     // one compaction chunk = one point per thread
constexpr int kCarveMaxTab = kCarveMaxCol + 2 * (kCarveMaxRow + 1);
constexpr unsigned kCarveEmpty = 0x7f800000u;        // +inf: an empty pixel of the range image

// The configuration as the kernels see it.  tab: cc[n_col / 2], cs[n_col / 2], ec[n_row + 1], es[n_row + 1] (f32, built by the host in double).
struct CarveCfg {
  int n_col, n_row, window_col, window_row;
  float min_range, max_range, margin_abs, margin_rel;
  const float* tab;
};
__host__ __device__ inline int carve_tab_size(int n_col, int n_row) { return n_col + 2 * (n_row + 1); }

// what one carve did, as the host sees it (msfl_grid_carve_info, 8 ints)
enum { CARVE_POINTS_REMOVED = 0, CARVE_CELLS_EMPTIED, CARVE_CELLS, CARVE_POINTS, CARVE_TESTED, CARVE_PIXELS, CARVE_APPLIED, CARVE_RESERVED, CARVE_WORDS };
// counters of the call in flight (zero between calls: carve_finish_kernel leaves them so)
enum { CARVE_CTR_PIXELS = 0, CARVE_CTR_TESTED, CARVE_CTR_WORDS = 4 };

__device__ __forceinline__ void carve_load_tab(const CarveCfg& c, float* __restrict__ s_tab) {
  const int nt = carve_tab_size(c.n_col, c.n_row);
  for (int i = threadIdx.x; i < nt; i += blockDim.x) s_tab[i] = c.tab[i];
}

// Pixel (row * n_col + col) and range of a sensor-frame point; false: the point has no pixel.  Both bisections keep "the
// boundary test holds at lo and fails at hi" and ARE the definition (the model runs the same steps).
__device__ __forceinline__ bool carve_pixel(const CarveCfg& c, const float* __restrict__ tab, float x, float y, float z, float& r, int& pix) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  const float rho2 = x * x + y * y;
  if (rho2 == 0.f) return false;
  const float rho = sqrtf(rho2);                     // correctly rounded in this build (the IEEE expansion, not v_sqrt_f32 alone)
  r = sqrtf(rho2 + z * z);
  if (!(r >= c.min_range) || r > c.max_range) return false;
  const int half = c.n_col >> 1;
  const float* cc = tab;
  const float* cs = tab + half;
  const float* ec = cs + half;
  const float* es = ec + (c.n_row + 1);
  if (z * ec[0] - rho * es[0] < 0.f || z * ec[c.n_row] - rho * es[c.n_row] >= 0.f) return false;      // outside the field of view
  const bool upper = y > 0.f || (y == 0.f && x > 0.f);
  const float xp = upper ? x : -x, yp = upper ? y : -y;
  int lo = 0, hi = half;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cc[mid] * yp - cs[mid] * xp >= 0.f) lo = mid; else hi = mid;
  }
  const int col = lo + (upper ? 0 : half);
  lo = 0; hi = c.n_row;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (z * ec[mid] - rho * es[mid] >= 0.f) lo = mid; else hi = mid;
  }
  pix = lo * c.n_col + col;
  return true;
}

// ---- step 1 (after the image was set to +inf): near[pixel] = min range of the scan's points there -------------------------------
__global__ void __launch_bounds__(kCarveBlock)
carve_fill_kernel(CarveCfg c, const float4* __restrict__ scan, int n, unsigned* __restrict__ near_img) {
  __shared__ float s_tab[kCarveMaxTab];
  carve_load_tab(c, s_tab);
  __syncthreads();
  for (int i = blockIdx.x * kCarveBlock + threadIdx.x; i < n; i += gridDim.x * kCarveBlock) {
    const float4 p = scan[i];
    float r; int pix;
    if (carve_pixel(c, s_tab, p.x, p.y, p.z, r, pix)) atomicMin(&near_img[pix], __float_as_uint(r));   // r > 0: the unsigned order is the float order
  }
}

// ---- step 2: lim[pixel] = 0 (no evidence) where the centre is empty, else min of near over rows +-window_row (clamped) and
// columns +-window_col (wrapping) ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCarveBlock)
carve_limit_kernel(CarveCfg c, const unsigned* __restrict__ near_img, float* __restrict__ lim, int* __restrict__ ctr) {
  const int npix = c.n_col * c.n_row;
  const int pix = blockIdx.x * kCarveBlock + threadIdx.x;
  bool full = false;
  if (pix < npix) {
    const int row = pix / c.n_col, col = pix - row * c.n_col;
    unsigned m = near_img[pix];
    full = m != kCarveEmpty;
    if (full) {
      const int r0 = max(row - c.window_row, 0), r1 = min(row + c.window_row, c.n_row - 1);
      for (int rr = r0; rr <= r1; rr++)
        for (int dc = -c.window_col; dc <= c.window_col; dc++) {
          const int cw = ((col + dc) % c.n_col + c.n_col) % c.n_col;
          m = min(m, near_img[rr * c.n_col + cw]);
        }
    }
    lim[pix] = full ? __uint_as_float(m) : 0.f;
  }
  const unsigned long long b = __ballot(full);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ctr[CARVE_CTR_PIXELS], __popcll(b));
}

// The sensor's pose inverted in f64: q' = conj(q), t' = -rotate(conj(q), t); a stored point goes through it exactly as
// msfl_transform_cloud transforms (f32 -> f64 -> q' p + t' -> f32).  ok: every component finite.  unit: |q|^2 within 1e-3 of 1, so
// the map-frame distance of a cell from the sensor bounds the range of its points (the cull below).
struct CarvePose { pose7 inv; d3 t; bool ok, unit; };
__device__ __forceinline__ CarvePose carve_pose(const double* __restrict__ pose) {
  CarvePose P;
  const pose7 T = load_pose(pose);
  P.ok = isfinite(T.t.x) && isfinite(T.t.y) && isfinite(T.t.z) && isfinite(T.q.x) && isfinite(T.q.y) && isfinite(T.q.z) && isfinite(T.q.w);
  P.t = T.t;
  P.inv.q.x = -T.q.x; P.inv.q.y = -T.q.y; P.inv.q.z = -T.q.z; P.inv.q.w = T.q.w;
  const d3 rt = quat_rotate(P.inv.q, T.t);
  P.inv.t = mk3(-rt.x, -rt.y, -rt.z);
  const double n2 = T.q.x * T.q.x + T.q.y * T.q.y + T.q.z * T.q.z + T.q.w * T.q.w;
  P.unit = fabs(n2 - 1.0) < 1e-3;
  return P;
}

// the per-point rule: removed iff the point has a pixel and (r (1 + margin_rel)) + margin_abs < lim[pixel]
__device__ __forceinline__ bool carve_sees_through(const CarveCfg& c, const float* __restrict__ tab, const pose7& inv, const float* __restrict__ lim,
                                                   float4 p, bool& tested) {
  const float3 q = transform_point_f32(inv, p.x, p.y, p.z);
  float r; int pix;
  tested = carve_pixel(c, tab, q.x, q.y, q.z, r, pix);
  if (!tested) return false;
  return (r * (1.0f + c.margin_rel)) + c.margin_abs < lim[pix];
}

// ---- step 3: per cell the number of points the scan sees through; keep = the cell survives ------------------------------------------
// A cell whose centre lies further from the sensor than max_range + half a cell's diagonal + 1 m holds no point with a pixel (its
// points lie within half a cell of the centre per axis, up to the rounding of a centroid) and is left unread.  Both arrays are 0
// beyond the live cells, so the device-wide scans need no tail pass.
__global__ void __launch_bounds__(kCarveBlock)
carve_count_kernel(CarveCfg c, const double* __restrict__ pose, const float* __restrict__ lim, const unsigned long long* __restrict__ keys,
                   const int* __restrict__ cell_start, const int* __restrict__ cell_cnt, const float4* __restrict__ pool, int bound,
                   float resolution, int* __restrict__ keep, int* __restrict__ rcnt, int* __restrict__ ctr, const GridState* __restrict__ st) {
  __shared__ float s_tab[kCarveMaxTab];
  __shared__ int s_removed, s_tested;
  const int nc = min(st->n_cells, bound);
  const CarvePose P = carve_pose(pose);
  carve_load_tab(c, s_tab);
  if (threadIdx.x == 0) { s_removed = 0; s_tested = 0; }
  __syncthreads();
  for (int cell = blockIdx.x; cell < bound; cell += gridDim.x) {
    if (cell >= nc) { if (threadIdx.x == 0) { keep[cell] = 0; rcnt[cell] = 0; } continue; }
    int ix, iy, iz;
    grid_cell_of_key(keys[cell], ix, iy, iz);
    const double dx = (double)ix * (double)resolution - P.t.x, dy = (double)iy * (double)resolution - P.t.y, dz = (double)iz * (double)resolution - P.t.z;
    const double reach = (double)c.max_range + 0.8661 * (double)resolution + 1.0;
    if (!P.ok || (P.unit && dx * dx + dy * dy + dz * dz > reach * reach)) {
      if (threadIdx.x == 0) { keep[cell] = 1; rcnt[cell] = 0; }
      continue;
    }
    const int s = cell_start[cell], m = cell_cnt[cell];
    int removed = 0, tested = 0;
    for (int i = threadIdx.x; i < m; i += kCarveBlock) {
      bool t;
      removed += carve_sees_through(c, s_tab, P.inv, lim, pool[s + i], t) ? 1 : 0;
      tested += t ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { removed += __shfl_down(removed, o); tested += __shfl_down(tested, o); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_removed, removed); atomicAdd(&s_tested, tested); }
    __syncthreads();
    if (threadIdx.x == 0) {
      keep[cell] = m - s_removed > 0 ? 1 : 0; rcnt[cell] = s_removed;
      if (s_tested) atomicAdd(&ctr[CARVE_CTR_TESTED], s_tested);
      s_removed = 0; s_tested = 0;
    }
    __syncthreads();
  }
}

// ---- step 4, one workgroup: the two exclusive scans (the shape of grid_crop_scan_kernel) ------------------------------------------
__global__ void __launch_bounds__(1024)
carve_scan_kernel(const int* __restrict__ keep, const int* __restrict__ rcnt, int bound, int* __restrict__ rank, int* __restrict__ roff,
                  const GridState* __restrict__ st) {
  __shared__ int s_wave[16];
  bound = min(bound, st->n_cells);                       // carve_apply_kernel reads none of the arrays beyond the live cells
  int carry_k = 0, carry_r = 0;
  for (int base = 0; base < bound; base += 4 * 1024) {
    const int c0 = base + 4 * (int)threadIdx.x;
    int k[4], e[4], tk = 0, te = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int cell = c0 + u;
      k[u] = cell < bound ? keep[cell] : 0; e[u] = cell < bound ? rcnt[cell] : 0;
      tk += k[u]; te += e[u];
    }
    int total_k, total_r;
    int run_k = carry_k + block_incl_scan_1024(tk, s_wave, total_k) - tk;
    int run_r = carry_r + block_incl_scan_1024(te, s_wave, total_r) - te;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int cell = c0 + u;
      if (cell < bound) { rank[cell] = run_k; roff[cell] = run_r; }
      run_k += k[u]; run_r += e[u];
    }
    carry_k += total_k; carry_r += total_r;
  }
}

// the decision every kernel after the scan takes alike
__device__ __forceinline__ bool carve_refused(bool pose_ok, const int* __restrict__ rcnt, const int* __restrict__ roff, int nc, int has_removed, int capacity) {
  return !pose_ok || (has_removed && nc > 0 && roff[nc - 1] + rcnt[nc - 1] > capacity);
}

// ---- steps 5 + 6: the table into the other buffer (one thread per cell), then the carved slabs (one workgroup per cell) ------------
// A surviving cell keeps start and stamp, its count drops by what it lost; an emptied cell leaves the table.  A carved slab is
// compacted in place, stably, a chunk of kCarveBlock points at a time: every point of the chunk is in a register before the
// barrier that precedes the chunk's first store, and the output index never overtakes the input index, so no store lands on a
// point that has not been read.  The removed points go to removed[roff[cell] + ...] in stored order: msfl_grid_dump order.
__global__ void __launch_bounds__(kCarveBlock)
carve_apply_kernel(CarveCfg c, const double* __restrict__ pose, const float* __restrict__ lim, const unsigned long long* __restrict__ keys_in,
                   const int* __restrict__ start_in, const int* __restrict__ cnt_in, const int* __restrict__ stamp_in,
                   unsigned long long* __restrict__ keys_out, int* __restrict__ start_out, int* __restrict__ cnt_out, int* __restrict__ stamp_out,
                   float4* __restrict__ pool, const int* __restrict__ keep, const int* __restrict__ rank, const int* __restrict__ rcnt,
                   const int* __restrict__ roff, int bound, float4* __restrict__ removed, int capacity, const GridState* __restrict__ st) {
  __shared__ float s_tab[kCarveMaxTab];
  __shared__ int s_k[kCarveBlock / 64], s_r[kCarveBlock / 64];
  const int nc = min(st->n_cells, bound);
  if (nc == 0) return;
  const CarvePose P = carve_pose(pose);
  const bool refused = carve_refused(P.ok, rcnt, roff, nc, removed != nullptr, capacity);
  for (int cell = blockIdx.x * kCarveBlock + threadIdx.x; cell < nc; cell += gridDim.x * kCarveBlock) {
    if (!refused && !keep[cell]) continue;
    const int o = refused ? cell : rank[cell];
    keys_out[o] = keys_in[cell]; start_out[o] = start_in[cell]; stamp_out[o] = stamp_in[cell];
    cnt_out[o] = refused ? cnt_in[cell] : cnt_in[cell] - rcnt[cell];
  }
  if (refused) return;
  carve_load_tab(c, s_tab);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int cell = blockIdx.x; cell < nc; cell += gridDim.x) {
    if (rcnt[cell] == 0) continue;
    const int s = start_in[cell], m = cnt_in[cell], ro = roff[cell];
    int kept = 0, gone = 0;                                // of the chunks before this one
    for (int base = 0; base < m; base += kCarveBlock) {
      const int i = base + (int)threadIdx.x;
      const bool valid = i < m;
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      bool rm = false, t;
      if (valid) { p = pool[s + i]; rm = carve_sees_through(c, s_tab, P.inv, lim, p, t); }
      const unsigned long long kb = __ballot(valid && !rm), rb = __ballot(rm);
      const unsigned long long below = (1ull << lane) - 1ull;
      if (lane == 0) { s_k[wave] = __popcll(kb); s_r[wave] = __popcll(rb); }
      __syncthreads();                                     // every point of the chunk is in a register
      int pk = __popcll(kb & below), pr = __popcll(rb & below), tk = 0, tr = 0;
#pragma unroll
      for (int w = 0; w < kCarveBlock / 64; w++) { const int a = s_k[w], b = s_r[w]; tk += a; tr += b; if (w < wave) { pk += a; pr += b; } }
      if (valid && !rm) pool[s + kept + pk] = p;
      if (rm && removed && ro + gone + pr < capacity) removed[ro + gone + pr] = p;
      kept += tk; gone += tr;
      __syncthreads();                                     // s_k / s_r are rewritten by the next chunk
    }
  }
}

// ---- step 7, one thread: fold the carve into the state, write the info record and the report (bound == 0: the table is empty,
// nothing but the two image launches ran before this) ----------------------------------------------------------------------------
__global__ void carve_finish_kernel(GridState* __restrict__ st, const double* __restrict__ pose, const int* __restrict__ keep, const int* __restrict__ rank,
                                    const int* __restrict__ rcnt, const int* __restrict__ roff, int bound, int has_removed, int capacity,
                                    int* __restrict__ ctr, int* __restrict__ info, int* __restrict__ report) {
  const int nc = min(st->n_cells, bound);
  const CarvePose P = carve_pose(pose);
  const int n_keep = nc > 0 ? rank[nc - 1] + keep[nc - 1] : 0, n_gone = nc > 0 ? roff[nc - 1] + rcnt[nc - 1] : 0;
  const int n_emptied = nc - n_keep;
  const int applied = carve_refused(P.ok, rcnt, roff, nc, has_removed, capacity) ? 0 : 1;
  if (applied) { st->n_cells -= n_emptied; st->n_points -= n_gone; }
  if (info) {
    info[CARVE_POINTS_REMOVED] = n_gone; info[CARVE_CELLS_EMPTIED] = n_emptied; info[CARVE_CELLS] = st->n_cells; info[CARVE_POINTS] = st->n_points;
    info[CARVE_TESTED] = ctr[CARVE_CTR_TESTED]; info[CARVE_PIXELS] = ctr[CARVE_CTR_PIXELS]; info[CARVE_APPLIED] = applied; info[CARVE_RESERVED] = 0;
  }
  if (report) {
    report[0] = st->n_points; report[1] = st->n_cells; report[2] = st->pool_top;
    report[3] = 0; report[4] = 0; report[5] = 0; report[6] = 0; report[7] = st->surround_total;
  }
  ctr[CARVE_CTR_PIXELS] = 0; ctr[CARVE_CTR_TESTED] = 0;
  st->bad = 0; st->overflow = 0; st->n_touched = 0; st->n_new_cells = 0; st->work = 0; st->delta_points = 0; st->n_big = 0;
}

}  // namespace msfl
