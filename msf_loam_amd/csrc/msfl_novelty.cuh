// msfl_novelty.cuh — the carve's mirror image (docs/kernels/novelty.md): the range image a map store predicts for a sensor at a given
// pose, and one class per scan point against it.  msfl_carve.cuh asks which STORED points a scan sees through; this file asks which
// SCAN points stand in space the map saw through.  The pixel rule, the pose and the tables are the carve's own (carve_pixel,
// carve_pose, carve_load_tab): nothing of them is written a second time.
//
//   render_clear_kernel     the image to +inf (accumulate = 0), the call's counter to zero, the pose's verdict into the applied word
//   render_cells_kernel     one workgroup per cell (the shape and cull of carve_count_kernel): every stored point through the inverse
//                           pose and carve_pixel, a no-return 32-bit minimum on the bit pattern into the image
//   novelty_window_kernel   one thread per pixel: mlim = minimum of the map image over the window, support = its non-empty positions
//   novelty_label_kernel    one lane per scan point: pixel -> class -> cls_out, the masked copy, the counts
//
// Every decision is a function of one point and of the image alone and a minimum does not depend on order, so nothing depends on the
// launch shape.  Integer atomics only; no workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msfl_carve.cuh"

namespace msfl {

enum { NOV_NONE = 0, NOV_UNSEEN = 1, NOV_COVERED = 2, NOV_IN_FRONT = 3, NOV_CLASSES = 4 };
// The counters of the handle: words 0..7 are msfl_novelty_info as the host reads it back, words 8..9 msfl_grid_render_info.
enum { NOV_CTR_CLASS = 0, NOV_CTR_MAP_PIXELS = 4, NOV_CTR_KEPT = 5, NOV_CTR_APPLIED = 6, NOV_CTR_RESERVED = 7, NOV_CTR_TESTED = 8,
       NOV_CTR_RENDERED = 9, NOV_CTR_WORDS = 16 };

// ---- render, step 1: npix = 0 with accumulate = 1 (the image stays); block 0 clears the counter and publishes the pose's verdict ------
__global__ void __launch_bounds__(kCarveBlock)
render_clear_kernel(const double* __restrict__ pose, unsigned* __restrict__ img, int npix, int* __restrict__ ctr) {
  const int i = blockIdx.x * kCarveBlock + threadIdx.x;
  if (i < npix) img[i] = kCarveEmpty;
  if (i == 0) { ctr[NOV_CTR_TESTED] = 0; ctr[NOV_CTR_RENDERED] = carve_pose(pose).ok ? 1 : 0; }
}

// ---- render, step 2: img[pixel] = min(img[pixel], range of every stored point there).  A pose that is not finite renders nothing; a
// cell beyond the carve's reach (carve_count_kernel has the bound) holds no point with a pixel and is left unread. ----------------------
__global__ void __launch_bounds__(kCarveBlock)
render_cells_kernel(CarveCfg c, const double* __restrict__ pose, const unsigned long long* __restrict__ keys, const int* __restrict__ cell_start,
                    const int* __restrict__ cell_cnt, const float4* __restrict__ pool, int bound, float resolution, unsigned* __restrict__ img,
                    int* __restrict__ ctr, const GridState* __restrict__ st) {
  __shared__ float s_tab[kCarveMaxTab];
  __shared__ int s_tested;
  const CarvePose P = carve_pose(pose);
  if (!P.ok) return;
  const int nc = min(st->n_cells, bound);
  carve_load_tab(c, s_tab);
  if (threadIdx.x == 0) s_tested = 0;
  __syncthreads();
  int tested = 0;                                          // of this wavefront, the same in every lane
  for (int cell = blockIdx.x; cell < nc; cell += gridDim.x) {
    int ix, iy, iz;
    grid_cell_of_key(keys[cell], ix, iy, iz);
    const double dx = (double)ix * (double)resolution - P.t.x, dy = (double)iy * (double)resolution - P.t.y, dz = (double)iz * (double)resolution - P.t.z;
    const double reach = (double)c.max_range + 0.8661 * (double)resolution + 1.0;
    if (P.unit && dx * dx + dy * dy + dz * dz > reach * reach) continue;
    const int s = cell_start[cell], m = cell_cnt[cell];
    for (int base = 0; base < m; base += kCarveBlock) {
      const int i = base + (int)threadIdx.x;
      bool t = false;
      if (i < m) {
        const float4 p = pool[s + i];
        const float3 q = transform_point_f32(P.inv, p.x, p.y, p.z);
        float r; int pix;
        t = carve_pixel(c, s_tab, q.x, q.y, q.z, r, pix);
        if (t) atomicMin(&img[pix], __float_as_uint(r));   // r > 0: the unsigned order is the float order
      }
      tested += __popcll(__ballot(t));
    }
  }
  if ((threadIdx.x & 63) == 0 && tested) atomicAdd(&s_tested, tested);
  __syncthreads();
  if (threadIdx.x == 0 && s_tested) atomicAdd(&ctr[NOV_CTR_TESTED], s_tested);
}

// ---- label, step 1: per pixel the window's minimum and support.  Rows clamp (a repeated edge row is counted again, as
// carve_numpy.limit_image repeats it), columns wrap; unlike the carve's limit image an empty centre does not void the window. ---------
__global__ void __launch_bounds__(kCarveBlock)
novelty_window_kernel(CarveCfg c, const unsigned* __restrict__ map_img, unsigned* __restrict__ mlim, int* __restrict__ support, int* __restrict__ ctr) {
  const int npix = c.n_col * c.n_row;
  const int pix = blockIdx.x * kCarveBlock + threadIdx.x;
  bool full = false;
  if (pix < npix) {
    const int row = pix / c.n_col, col = pix - row * c.n_col;
    full = map_img[pix] != kCarveEmpty;
    unsigned m = kCarveEmpty;
    int sup = 0;
    for (int dr = -c.window_row; dr <= c.window_row; dr++) {
      const int rr = min(max(row + dr, 0), c.n_row - 1);
      for (int dc = -c.window_col; dc <= c.window_col; dc++) {
        const int cw = ((col + dc) % c.n_col + c.n_col) % c.n_col;
        const unsigned v = map_img[rr * c.n_col + cw];
        sup += v != kCarveEmpty ? 1 : 0;
        m = min(m, v);
      }
    }
    mlim[pix] = m; support[pix] = sup;
  }
  const unsigned long long b = __ballot(full);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ctr[NOV_CTR_MAP_PIXELS], __popcll(b));
}

// ---- label, step 2.  rendered: null, or the applied word of the render this image came from (msfl_grids_scan_novelty): 0 means the
// pose was refused, nothing is known about any ray and every point is NONE. ---------------------------------------------------------------
__global__ void __launch_bounds__(kCarveBlock)
novelty_label_kernel(CarveCfg c, int min_support, int keep, const float4* __restrict__ scan, int n, const unsigned* __restrict__ mlim,
                     const int* __restrict__ support, const int* __restrict__ rendered, uint8_t* __restrict__ cls_out, float4* __restrict__ masked,
                     int* __restrict__ ctr) {
  __shared__ float s_tab[kCarveMaxTab];
  carve_load_tab(c, s_tab);
  __syncthreads();
  const bool ok = rendered ? *rendered != 0 : true;
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctr[NOV_CTR_APPLIED] = ok ? 1 : 0; ctr[NOV_CTR_RESERVED] = 0; }
  int n_cls[NOV_CLASSES] = {0, 0, 0, 0}, n_kept = 0;       // of this wavefront, the same in every lane
  for (int base = blockIdx.x * kCarveBlock; base < n; base += gridDim.x * kCarveBlock) {
    const int i = base + (int)threadIdx.x;
    const bool valid = i < n;
    int cls = NOV_NONE;
    bool kept = false;
    if (valid) {
      float4 p = scan[i];
      float r; int pix;
      if (ok && carve_pixel(c, s_tab, p.x, p.y, p.z, r, pix)) {
        if (support[pix] < min_support) cls = NOV_UNSEEN;
        else cls = (r * (1.0f + c.margin_rel)) + c.margin_abs < __uint_as_float(mlim[pix]) ? NOV_IN_FRONT : NOV_COVERED;
      }
      kept = (keep >> cls) & 1;
      cls_out[i] = (uint8_t)cls;
      if (masked) {
        if (!kept) { const float nan = __uint_as_float(0x7fc00000u); p.x = nan; p.y = nan; p.z = nan; }
        masked[i] = p;
      }
    }
#pragma unroll
    for (int k = 0; k < NOV_CLASSES; k++) n_cls[k] += __popcll(__ballot(valid && cls == k));
    n_kept += __popcll(__ballot(kept));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NOV_CLASSES; k++) if (n_cls[k]) atomicAdd(&ctr[NOV_CTR_CLASS + k], n_cls[k]);
    if (n_kept) atomicAdd(&ctr[NOV_CTR_KEPT], n_kept);
  }
}

}  // namespace msfl
