// msfl_search.cuh — hit-count lattice correlation of one scan against a bit-per-voxel volume of the resident map (gfx950 / CDNA4).
// Definition: docs/kernels/search.md and include/msfl_c_api.h (msfl_search_poses).  Integers only after the voxel of a point is
// taken, so every output is bit-reproducible whatever the launch shape.
//
//   search_clear_kernel      zeroes the volumes of both kinds, the peak counter and the candidate count (a kernel, not a memset node)
//   search_fill_kernel       one lane per point of the map index's sorted copy: atomicOr of its voxel's bit
//   search_dilate_kernel     one lane per 64-bit word, out of place: x inside the word with the neighbour words' carry bits, y and z
//                            as the OR of the neighbour rows
//   search_table_kernel      one lane per (yaw sample, feature): transform_point_f32 at pose(a, k = 0), voxel as int4 (x, y, z, kind)
//   search_correlate_kernel  one wavefront per (a, kz', ky', 64 x-shifts): lanes stride the features, two 64-bit loads and a funnel
//                            shift give a feature's 64 x-shifts as one mask; masks are added into per-lane bit-sliced carry-save
//                            counters and turned into 64 counts (lane t owns shift t) by ballots once at the end
//   search_peaks_kernel      one lane per hypothesis: the key ((0xffffffff - total) << 32) | h, the peak test, peaks appended
//   search_select_kernel     ONE workgroup: exact radix select of the K smallest keys, bitonic sort, candidate records
//
// Every kernel is a thin wrapper round a __device__ body, and has a second wrapper, <name>_pairs_kernel, for msfl_search_pairs:
// blockIdx.y is the pair inside the chunk of pairs in flight, blockIdx.x what it is in the single form (a pair's surplus
// workgroups leave at once).  All pairs share one SearchGeom but the box origin; what differs sits in a SearchPair table.
//
// Volume layout: bit x & 63 of word [(z * dims.y + y) * W + (x >> 6)], W = ceil(dims.x / 64) + 1.  Bits at x >= dims.x and the last
// word of every row stay zero; a window that hangs over either end of a row reads zero words there (range checks, no over-read).
#pragma once
#include "msfl_kernels.cuh"

namespace msfl {

constexpr int kSearchBlock = 256;
constexpr int kSearchPlanes = 8;                 // carry-save planes per lane: 255 masks between two flushes
constexpr int kSearchSelectBlock = 1024;
constexpr int kSearchMaxK = 1024;
constexpr int kSearchNoVoxel = -2147483647 - 1;         // table sentinel (x): the feature never hits

struct SearchGeom {
  float ox, oy, oz, inv;
  int dx, dy, dz, W;                             // voxels per axis, words per row
  int nx, ny, nz, n_yaw;
  int hx, hy, hz;                                // half
};

struct SearchCand {                              // msfl_pose_candidate
  double pose[7];
  int h, a, kx, ky, kz;
  int hits[2];
  int reserved_;
};

// ---- the pairs form: C pairs in flight, every per-pair array a dense [C] x (the single form's array) -------------------------------
struct SearchPair {                              // one pair of msfl_search_pairs, host-built
  float ox, oy, oz;                              // its box origin; the rest of SearchGeom is the call's
  int n_corner, n_surf;
  int corner0, surf0;                            // its first feature in the call's scan clouds
  int reserved_;
  unsigned long long tab0;                       // its first entry in the chunk's table
};
struct SearchPairsView {
  const SearchPair* pair;                        // [C]
  const double* qtab;                            // [C] x (4 n_yaw quaternion entries, then the pair's guess)
  unsigned long long* vol;                       // raw volumes [C][kind], then with dilate = 1 the dilated ones [C][kind]
  size_t vol_words;                              // words of one volume
  int4* tab;
  int* hits;                                     // [C][kind][H]
  unsigned long long* peaks;                     // [C][H]
  int* ctr;                                      // [C][2]
  SearchCand* cand;                              // [C][K]
  int* n_out;                                    // [C], or null
  int n_pairs, dilate, H, K;
};
// (flat offsets over a chunk go through size_t: C x H passes 2^31 quickly; what is indexed inside a pair stays 32-bit)
__device__ __forceinline__ SearchGeom search_pair_geom(SearchGeom g, const SearchPair& p) { g.ox = p.ox; g.oy = p.oy; g.oz = p.oz; return g; }
__device__ __forceinline__ const double* search_pair_qtab(const SearchPairsView& v, const SearchGeom& g, int p) {
  return v.qtab + (size_t)p * (4 * (size_t)g.n_yaw + 7);
}
__device__ __forceinline__ const unsigned long long* search_pair_vol(const SearchPairsView& v, int p, int kind) {
  return v.vol + ((v.dilate ? 2 * (size_t)v.n_pairs : 0) + 2 * (size_t)p + kind) * v.vol_words;
}

// words: 2 volumes (x 2 when dilated) back to back, of every pair in flight.  ctr, per pair: [0] peaks appended, [1] candidates written (the kernel's own n_out)
__global__ void __launch_bounds__(kSearchBlock) search_clear_kernel(unsigned long long* __restrict__ words, size_t n, int* __restrict__ ctr, int n_ctr) {
  const size_t i = (size_t)blockIdx.x * kSearchBlock + threadIdx.x;
  if (i < n) words[i] = 0ull;
  if (i < (size_t)n_ctr) ctr[i] = 0;                       // 2 per pair
}

// voxel coordinate of one axis as a float: the two f32 operations of the definition (the library is built without contraction)
__device__ __forceinline__ float search_voxel(float x, float o, float inv) { return floorf((x - o) * inv); }

// point i of the n finite points of one map
__device__ __forceinline__ void search_fill_body(const SearchGeom& g, int n, const float4* __restrict__ pts, unsigned long long* __restrict__ vol, int i) {
  if (i >= n) return;
  const float4 p = pts[i];
  const float fx = search_voxel(p.x, g.ox, g.inv), fy = search_voxel(p.y, g.oy, g.inv), fz = search_voxel(p.z, g.oz, g.inv);
  // (a NaN fails every comparison)
  if (!(fx >= 0.f && fx < (float)g.dx && fy >= 0.f && fy < (float)g.dy && fz >= 0.f && fz < (float)g.dz)) return;
  const int x = (int)fx, y = (int)fy, z = (int)fz;
  atomicOr(&vol[((size_t)z * g.dy + y) * g.W + (x >> 6)], 1ull << (x & 63));
}
__global__ void __launch_bounds__(kSearchBlock) search_fill_kernel(SearchGeom g, const GridDesc* __restrict__ gd,
                                                                    const float4* __restrict__ pts, unsigned long long* __restrict__ vol) {
  search_fill_body(g, gd->n_pts, pts, vol, blockIdx.x * kSearchBlock + threadIdx.x);   // the index's sorted copy holds the map's finite points
}
// The pair index keeps no point count in GridDesc[p]; a pair's finite points are what its slice of the cell table holds, the
// positions [cell_start[cell_base[p]], cell_start[cell_base[p + 1]]) of the concatenated sorted copy.
__global__ void __launch_bounds__(kSearchBlock) search_fill_pairs_kernel(SearchGeom g, SearchPairsView v, int kind, const int* __restrict__ cell_start,
                                                                          const int* __restrict__ cell_base, const float4* __restrict__ sorted) {
  const int p = blockIdx.y;
  const int lo = cell_start[cell_base[p]], n = cell_start[cell_base[p + 1]] - lo;
  if ((int)blockIdx.x * kSearchBlock >= n) return;
  search_fill_body(search_pair_geom(g, v.pair[p]), n, sorted + lo, v.vol + (2 * (size_t)p + kind) * v.vol_words, blockIdx.x * kSearchBlock + threadIdx.x);
}

// word i of one volume
__device__ __forceinline__ void search_dilate_body(const SearchGeom& g, const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out, size_t i) {
  const size_t n = (size_t)g.dz * g.dy * g.W;
  if (i >= n) return;
  const int w = (int)(i % g.W);
  const size_t row = i / g.W;
  const int y = (int)(row % g.dy), z = (int)(row / g.dy);
  unsigned long long acc = 0ull;
  for (int oz = -1; oz <= 1; oz++) {
    const int zz = z + oz;
    if (zz < 0 || zz >= g.dz) continue;
    for (int oy = -1; oy <= 1; oy++) {
      const int yy = y + oy;
      if (yy < 0 || yy >= g.dy) continue;
      const unsigned long long* r = in + ((size_t)zz * g.dy + yy) * g.W;
      const unsigned long long c = r[w];
      const unsigned long long lo = w > 0 ? r[w - 1] : 0ull, hi = w + 1 < g.W ? r[w + 1] : 0ull;
      acc |= c | (c << 1) | (c >> 1) | (lo >> 63) | (hi << 63);
    }
  }
  // clipped at the box: bits at x >= dims.x stay zero
  const int first = w * 64;
  unsigned long long keep = 0ull;
  if (first + 64 <= g.dx) keep = ~0ull;
  else if (first < g.dx) keep = (1ull << (g.dx - first)) - 1ull;
  out[i] = acc & keep;
}
__global__ void __launch_bounds__(kSearchBlock) search_dilate_kernel(SearchGeom g, const unsigned long long* __restrict__ in,
                                                                      unsigned long long* __restrict__ out) {
  search_dilate_body(g, in, out, (size_t)blockIdx.x * kSearchBlock + threadIdx.x);
}
// flat over the 2 C equal-sized raw volumes of the chunk (the origin plays no part)
__global__ void __launch_bounds__(kSearchBlock) search_dilate_pairs_kernel(SearchGeom g, SearchPairsView v) {
  const size_t i = (size_t)blockIdx.x * kSearchBlock + threadIdx.x;
  const size_t vi = i / v.vol_words;
  if (vi >= 2 * (size_t)v.n_pairs) return;
  const unsigned long long* in = v.vol + vi * v.vol_words;
  search_dilate_body(g, in, v.vol + (2 * (size_t)v.n_pairs + vi) * v.vol_words, i - vi * v.vol_words);
}

// qtab: n_yaw x 4 doubles, the normalised quaternion of every yaw sample (host-computed: the device copies, it does not redo
// the trigonometry); guess: the guess pose (its translation is that of pose(a, 0)).  tab[a * F + f], corner features first.
__device__ __forceinline__ void search_table_body(const SearchGeom& g, const float4* __restrict__ corner, int n_corner,
                                                  const float4* __restrict__ surf, int n_surf, const double* __restrict__ qtab,
                                                  const double* __restrict__ guess, int4* __restrict__ tab, size_t i) {
  const int F = n_corner + n_surf;
  if (i >= (size_t)g.n_yaw * F) return;
  const int a = (int)(i / F), f = (int)(i % F);
  const int kind = f < n_corner ? 0 : 1;
  const float4 p = kind ? surf[f - n_corner] : corner[f];
  pose7 T;
  T.t = mk3(guess[0], guess[1], guess[2]);
  T.q.x = qtab[4 * a + 0]; T.q.y = qtab[4 * a + 1]; T.q.z = qtab[4 * a + 2]; T.q.w = qtab[4 * a + 3];
  int4 e = make_int4(kSearchNoVoxel, 0, 0, kind);
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    const float3 w = transform_point_f32(T, p.x, p.y, p.z);
    const float fx = search_voxel(w.x, g.ox, g.inv), fy = search_voxel(w.y, g.oy, g.inv), fz = search_voxel(w.z, g.oz, g.inv);
    // beyond 2^21 cells from the origin no shift of at most 2^20 cells reaches the box of at most 2^20 cells (and the int stays exact)
    const float lim = 2097152.f;
    if (fabsf(fx) < lim && fabsf(fy) < lim && fabsf(fz) < lim) { e.x = (int)fx; e.y = (int)fy; e.z = (int)fz; }
  }
  tab[(size_t)a * F + f] = e;
}
__global__ void __launch_bounds__(kSearchBlock) search_table_kernel(SearchGeom g, const float4* __restrict__ corner, int n_corner,
                                                                     const float4* __restrict__ surf, int n_surf,
                                                                     const double* __restrict__ qtab, const double* __restrict__ guess,
                                                                     int4* __restrict__ tab) {
  search_table_body(g, corner, n_corner, surf, n_surf, qtab, guess, tab, (size_t)blockIdx.x * kSearchBlock + threadIdx.x);
}
// ragged: grid.x serves the pair with the most features
__global__ void __launch_bounds__(kSearchBlock) search_table_pairs_kernel(SearchGeom g, SearchPairsView v, const float4* __restrict__ corner,
                                                                           const float4* __restrict__ surf) {
  const int p = blockIdx.y;
  const SearchPair pr = v.pair[p];
  if ((size_t)blockIdx.x * kSearchBlock >= (size_t)g.n_yaw * (pr.n_corner + pr.n_surf)) return;
  const double* qt = search_pair_qtab(v, g, p);
  search_table_body(search_pair_geom(g, pr), corner + pr.corner0, pr.n_corner, surf + pr.surf0, pr.n_surf, qt, qt + 4 * (size_t)g.n_yaw, v.tab + pr.tab0,
                    (size_t)blockIdx.x * kSearchBlock + threadIdx.x);
}

// grid.x = ((a * nz + kz') * ny + ky') * chunks + chunk; one wavefront.  Lane t owns x-shift kx' = 64 chunk + t.
__device__ __forceinline__ void search_correlate_body(const SearchGeom& g, const int4* __restrict__ tab, int n_corner, int n_surf,
                                                      const unsigned long long* __restrict__ vol_c,
                                                      const unsigned long long* __restrict__ vol_s, int chunks,
                                                      int* __restrict__ hits, int H) {
  const int lane = threadIdx.x;
  int b = blockIdx.x;
  const int chunk = b % chunks; b /= chunks;
  const int kyp = b % g.ny; b /= g.ny;
  const int kzp = b % g.nz;
  const int a = b / g.nz;
  const int ky = kyp - g.hy, kz = kzp - g.hz;
  const int x0 = 64 * chunk - g.hx;                        // x-shift of bit 0 of the mask
  const int F = n_corner + n_surf;
  const int4* row_tab = tab + (size_t)a * F;
  const size_t h0 = (((size_t)a * g.nz + kzp) * g.ny + kyp) * g.nx + 64 * chunk;
#pragma unroll 1
  for (int kind = 0; kind < 2; kind++) {
    const int f0 = kind ? n_corner : 0, nf = kind ? n_surf : n_corner;
    const unsigned long long* vol = kind ? vol_s : vol_c;
    unsigned long long pl[kSearchPlanes];
#pragma unroll
    for (int j = 0; j < kSearchPlanes; j++) pl[j] = 0ull;
    int count = 0;                                         // lane t: hits of shift t
    int since = 0;                                         // masks added since the last flush (wave-uniform)
    for (int base = 0; base < nf; base += 64) {
      const int f = base + lane;
      unsigned long long m = 0ull;
      if (f < nf) {
        const int4 e = row_tab[f0 + f];
        const int y = e.y + ky, z = e.z + kz;
        if (e.x != kSearchNoVoxel && y >= 0 && y < g.dy && z >= 0 && z < g.dz) {
          const unsigned long long* r = vol + ((size_t)z * g.dy + y) * g.W;
          const int s = e.x + x0;                          // first bit of the window, may lie outside [0, 64 W)
          const int wi = s >> 6, sh = s & 63;              // (arithmetic shift: floor)
          const unsigned long long lo = (wi >= 0 && wi < g.W) ? r[wi] : 0ull;
          const unsigned long long hi = (wi + 1 >= 0 && wi + 1 < g.W) ? r[wi + 1] : 0ull;
          m = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
        }
      }
      // bit-sliced add of the mask: plane j holds bit j of 64 counters
      unsigned long long carry = m;
#pragma unroll
      for (int j = 0; j < kSearchPlanes; j++) { const unsigned long long t = pl[j] & carry; pl[j] ^= carry; carry = t; }
      since++;
      if (since == (1 << kSearchPlanes) - 1 || base + 64 >= nf) {
        // flush: for plane j and shift t, lane t adds 2^j times the lanes that hold the bit
#pragma unroll
        for (int j = 0; j < kSearchPlanes; j++) {
          if (__ballot(pl[j] != 0ull) == 0ull) continue;
          for (int t = 0; t < 64; t++) {
            const int c = __popcll(__ballot((pl[j] >> t) & 1ull));
            if (lane == t) count += c << j;
          }
          pl[j] = 0ull;
        }
        since = 0;
      }
    }
    const int kxp = 64 * chunk + lane;
    if (kxp < g.nx) hits[(size_t)kind * H + h0 + lane] = count;
  }
}
__global__ void __launch_bounds__(64) search_correlate_kernel(SearchGeom g, const int4* __restrict__ tab, int n_corner, int n_surf,
                                                               const unsigned long long* __restrict__ vol_c,
                                                               const unsigned long long* __restrict__ vol_s, int chunks,
                                                               int* __restrict__ hits, int H) {
  search_correlate_body(g, tab, n_corner, n_surf, vol_c, vol_s, chunks, hits, H);
}
// grid (the single form's grid.x, C): workgroups are handed out x first, so those of one pair are neighbours in dispatch order and
// its two volumes stay in the reach of few L2s -- a guess about placement, not a measured fact
__global__ void __launch_bounds__(64) search_correlate_pairs_kernel(SearchGeom g, SearchPairsView v, int chunks) {
  const int p = blockIdx.y;
  const SearchPair pr = v.pair[p];
  search_correlate_body(g, v.tab + pr.tab0, pr.n_corner, pr.n_surf, search_pair_vol(v, p, 0), search_pair_vol(v, p, 1), chunks,
                        v.hits + 2 * (size_t)p * v.H, v.H);
}

__device__ __forceinline__ unsigned long long search_key(int total, int h) {
  return ((unsigned long long)(0xffffffffu - (unsigned)total) << 32) | (unsigned)h;
}

// peaks: keys of the peaks, appended in no particular order (they are unique, the select orders them); ctr[0] counts them
__device__ __forceinline__ void search_peaks_body(const SearchGeom& g, const int* __restrict__ hits, int H, int nms_cells, int nms_yaws,
                                                  int wraps, unsigned long long* __restrict__ peaks, int* __restrict__ ctr) {
  const int h = blockIdx.x * kSearchBlock + threadIdx.x;
  bool peak = false;
  unsigned long long key = 0ull;
  if (h < H) {
    int r = h;
    const int kx = r % g.nx; r /= g.nx;
    const int ky = r % g.ny; r /= g.ny;
    const int kz = r % g.nz;
    const int a = r / g.nz;
    key = search_key(hits[h] + hits[(size_t)H + h], h);
    peak = true;
    for (int da = -nms_yaws; da <= nms_yaws && peak; da++) {
      int aa = a + da;
      if (wraps) { aa %= g.n_yaw; if (aa < 0) aa += g.n_yaw; }
      else if (aa < 0 || aa >= g.n_yaw) continue;
      for (int z = max(kz - nms_cells, 0); z <= min(kz + nms_cells, g.nz - 1) && peak; z++)
        for (int y = max(ky - nms_cells, 0); y <= min(ky + nms_cells, g.ny - 1) && peak; y++)
          for (int x = max(kx - nms_cells, 0); x <= min(kx + nms_cells, g.nx - 1); x++) {
            const int o = ((aa * g.nz + z) * g.ny + y) * g.nx + x;
            if (o != h && search_key(hits[o] + hits[(size_t)H + o], o) < key) { peak = false; break; }
          }
    }
  }
  const unsigned long long m = __ballot(peak);
  if (m == 0ull) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == __ffsll((long long)m) - 1) base = atomicAdd(&ctr[0], __popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1);
  if (peak) peaks[base + __popcll(m & ((1ull << lane) - 1ull))] = key;
}
__global__ void __launch_bounds__(kSearchBlock) search_peaks_kernel(SearchGeom g, const int* __restrict__ hits, int H, int nms_cells,
                                                                     int nms_yaws, int wraps, unsigned long long* __restrict__ peaks,
                                                                     int* __restrict__ ctr) {
  search_peaks_body(g, hits, H, nms_cells, nms_yaws, wraps, peaks, ctr);
}
// pair p appends into its own key range with its own counter
__global__ void __launch_bounds__(kSearchBlock) search_peaks_pairs_kernel(SearchGeom g, SearchPairsView v, int nms_cells, int nms_yaws, int wraps) {
  const int p = blockIdx.y;
  search_peaks_body(g, v.hits + 2 * (size_t)p * v.H, v.H, nms_cells, nms_yaws, wraps, v.peaks + (size_t)p * v.H, v.ctr + 2 * p);
}

// ONE workgroup.  The K smallest of the ctr[0] peak keys (exact radix select, 8 bits per pass from the top, the pattern of
// place_prefilter_kernel; keys are unique), sorted, as candidate records; ctr[1] = n_out = records written.
__device__ __forceinline__ void search_select_body(const SearchGeom& g, const unsigned long long* __restrict__ peaks, int* __restrict__ ctr, int K,
                                                   const int* __restrict__ hits, int H, const double* __restrict__ qtab,
                                                   const double* __restrict__ guess, double step, SearchCand* __restrict__ out,
                                                   int* __restrict__ n_out) {
  __shared__ int s_hist[256];
  __shared__ int s_bin, s_left, s_fill;
  __shared__ unsigned long long s_key[kSearchMaxK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = ctr[0];
  const int k = min(K, n);
  unsigned long long cut = ~0ull;                          // k == n: every key
  if (k < n) {
    cut = 0ull;
    int left = k;
    for (int pass = 0; pass < 8; pass++) {
      const int shift = 56 - 8 * pass;
      if (tid < 256) s_hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += kSearchSelectBlock) {
        const unsigned long long key = peaks[i];
        if (pass == 0 || (key >> (shift + 8)) == (cut >> (shift + 8))) atomicAdd(&s_hist[(int)(key >> shift) & 255], 1);
      }
      __syncthreads();
      if (wave == 0) {                                     // lane l holds bins 4 l .. 4 l + 3, ascending
        int hb[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) { hb[u] = s_hist[4 * lane + u]; sum += hb[u]; }
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
        int below = incl - sum;
        if (below < left && left <= incl) {                // exactly one lane
#pragma unroll
          for (int u = 0; u < 4; u++) {
            if (below < left && left <= below + hb[u]) { s_bin = 4 * lane + u; s_left = left - below; below = left; }
            else below += hb[u];
          }
        }
      }
      __syncthreads();
      cut |= (unsigned long long)s_bin << shift;
      left = s_left;
      __syncthreads();
    }
  }
  // the k keys <= cut, in any order, padded to a power of two for the sort
  if (tid == 0) s_fill = 0;
  s_key[tid] = ~0ull;                                      // (kSearchSelectBlock == kSearchMaxK)
  __syncthreads();
  for (int i = tid; i < n; i += kSearchSelectBlock) {
    const unsigned long long key = peaks[i];
    if (key <= cut) { const int at = atomicAdd(&s_fill, 1); if (at < kSearchMaxK) s_key[at] = key; }
  }
  __syncthreads();
  for (int size = 2; size <= kSearchMaxK; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int partner = tid ^ stride;
      if (partner > tid) {
        const unsigned long long x = s_key[tid], y = s_key[partner];
        const bool up = (tid & size) == 0;
        if ((x > y) == up) { s_key[tid] = y; s_key[partner] = x; }
      }
      __syncthreads();
    }
  }
  if (tid == 0) { ctr[1] = k; if (n_out) *n_out = k; }
  if (tid < k) {
    const int h = (int)(unsigned)s_key[tid];
    int r = h;
    const int kxp = r % g.nx; r /= g.nx;
    const int kyp = r % g.ny; r /= g.ny;
    const int kzp = r % g.nz;
    const int a = r / g.nz;
    SearchCand c;
    c.h = h; c.a = a; c.kx = kxp - g.hx; c.ky = kyp - g.hy; c.kz = kzp - g.hz;
    c.pose[0] = guess[0] + step * (double)c.kx;
    c.pose[1] = guess[1] + step * (double)c.ky;
    c.pose[2] = guess[2] + step * (double)c.kz;
#pragma unroll
    for (int u = 0; u < 4; u++) c.pose[3 + u] = qtab[4 * a + u];
    c.hits[0] = hits[h]; c.hits[1] = hits[(size_t)H + h];
    c.reserved_ = 0;
    out[tid] = c;
  } else if (tid < K) {
    // the slots past n_out are all zero: a device-memory caller gets all K slots, never what an earlier search left in scratch
    SearchCand c;
    for (int u = 0; u < 7; u++) c.pose[u] = 0.0;
    c.h = 0; c.a = 0; c.kx = 0; c.ky = 0; c.kz = 0; c.hits[0] = 0; c.hits[1] = 0; c.reserved_ = 0;
    out[tid] = c;
  }
}
__global__ void __launch_bounds__(kSearchSelectBlock) search_select_kernel(SearchGeom g, const unsigned long long* __restrict__ peaks,
                                                                            int* __restrict__ ctr, int K, const int* __restrict__ hits,
                                                                            int H, const double* __restrict__ qtab,
                                                                            const double* __restrict__ guess, double step,
                                                                            SearchCand* __restrict__ out, int* __restrict__ n_out) {
  search_select_body(g, peaks, ctr, K, hits, H, qtab, guess, step, out, n_out);
}
// one workgroup per pair
__global__ void __launch_bounds__(kSearchSelectBlock) search_select_pairs_kernel(SearchGeom g, SearchPairsView v, double step) {
  const int p = blockIdx.y;
  const double* qt = search_pair_qtab(v, g, p);
  search_select_body(g, v.peaks + (size_t)p * v.H, v.ctr + 2 * p, v.K, v.hits + 2 * (size_t)p * v.H, v.H, qt, qt + 4 * (size_t)g.n_yaw, step,
                     v.cand + (size_t)p * v.K, v.n_out ? v.n_out + p : nullptr);
}

}  // namespace msfl
