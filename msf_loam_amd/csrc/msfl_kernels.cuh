// msfl_kernels.cuh — HIP kernels of the scan-to-map registration path (gfx950 / CDNA4).
//
//   K3  map grid index      replaces pcl::KdTreeFLANN::setInputCloud   mapping_scan_matcher.cc:66-73   (msfl_knn_index.cuh)
//   K4 assoc_scan2map      replaces the two association loops         mapping_scan_matcher.cc:109-246
//   K5+K6 lm_solve          replaces ceres::Solve (LM, Huber)          mapping_scan_matcher.cc:250-272
//
// Data layout in HBM:
//   features     float4 {x,y,z,t} per point, scans concatenated, B+1 prefix offsets
//   map (sorted) float4 {x,y,z, bits(original index)} ordered by grid cell (x fastest)
//   cell_start   int[n_cells+1]
//   records      per scan: n_corner edge records {C[3], N[3]} (48 B) followed by n_surf plane records
//                {N[3], N.C} (32 B); N == 0 marks a rejected correspondence.  Scan b starts at
//                6*(corner_off[b]-corner_off[0]) + 4*(surf_off[b]-surf_off[0]) doubles.
//   poses        7 doubles per scan
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msfl_math.cuh"
#include "msfl_record_tiles.h"
#include "msfl_knn_index.cuh"

namespace msfl {

// ---------------------------------------------------------------------------------------------
// K4: association = transform + exact 5-NN (the walks of msfl_knn_index.cuh) + line / plane fit -> {C, N} record
// ---------------------------------------------------------------------------------------------

struct FitOut { d3 C, N; bool ok; };

// mapping_scan_matcher.cc:130-151
__device__ __forceinline__ FitOut edge_fit(const float4 (&nb)[5], double ratio) {
  FitOut o; o.ok = false; o.C = mk3(0, 0, 0); o.N = mk3(0, 0, 0);
  d3 m[5];
  d3 c = mk3(0, 0, 0);
#pragma unroll
  for (int j = 0; j < 5; j++) { m[j] = mk3((double)nb[j].x, (double)nb[j].y, (double)nb[j].z); c = c + m[j]; }
  c = mk3(c.x / 5.0, c.y / 5.0, c.z / 5.0);
  sym3 S = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const d3 d = m[j] - c;
    S.a00 += d.x * d.x; S.a01 += d.x * d.y; S.a02 += d.x * d.z;
    S.a11 += d.y * d.y; S.a12 += d.y * d.z; S.a22 += d.z * d.z;
  }
  double e1, e2; d3 dir;
  sym_eigen3_top(S, e1, e2, dir);
  if (!(e2 > ratio * e1)) return o;
  const d3 pa = mk3(0.1 * dir.x + c.x, 0.1 * dir.y + c.y, 0.1 * dir.z + c.z);
  const d3 pb = mk3(-0.1 * dir.x + c.x, -0.1 * dir.y + c.y, -0.1 * dir.z + c.z);
  o.N = normalized(pa - pb);
  o.C = pa;
  o.ok = true;
  return o;
}

// mapping_scan_matcher.cc:199-222
__device__ __forceinline__ FitOut plane_fit(const float4 (&nb)[5], double tol) {
  FitOut o; o.ok = false; o.C = mk3(0, 0, 0); o.N = mk3(0, 0, 0);
  d3 c = mk3(0, 0, 0);
#pragma unroll
  for (int j = 0; j < 5; j++) c = c + mk3((double)nb[j].x, (double)nb[j].y, (double)nb[j].z);
  c = mk3(c.x / 5.0, c.y / 5.0, c.z / 5.0);
  bool well = false;
  d3 x = mk3(0, 0, 0);
  if (!MSFL_IEEE_DIV) {                            // direction of the least-squares solution only: all the fit uses
    double q[5][3];                                // centred points (not kept across the fallback: the distance test re-forms them)
#pragma unroll
    for (int j = 0; j < 5; j++) { q[j][0] = (double)nb[j].x - c.x; q[j][1] = (double)nb[j].y - c.y; q[j][2] = (double)nb[j].z - c.z; }
    x = plane_normal_centred(q, c, well);
  }
  if (!well) {                           // ill-conditioned or rank-deficient: the reference's pivoted QR decides
    double A[5][3], b[5];
#pragma unroll
    for (int j = 0; j < 5; j++) { A[j][0] = (double)nb[j].x; A[j][1] = (double)nb[j].y; A[j][2] = (double)nb[j].z; b[j] = -1.0; }
    x = lstsq5x3(A, b);
  }
  const d3 n = normalized_rsq(x);
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const double d = n.x * ((double)nb[j].x - c.x) + n.y * ((double)nb[j].y - c.y) + n.z * ((double)nb[j].z - c.z);
    if (fabs(d) > tol) ok = false;
  }
  if (!ok) return o;
  o.C = c; o.N = n; o.ok = true;
  return o;
}

struct BatchView {
  const float4* corner; const int* corner_off;
  const float4* surf;   const int* surf_off;
  const int* rec_off;       // rec_off[b] = corner_off[b] + surf_off[b]
  int n_scans;
  int n_records;            // rec_off[n_scans]; for the association kernels: one past the last record of this launch
  int rec_begin = 0;        // association kernels: first record of this launch (a host-buffer batch is associated chunk by chunk as it arrives)
  int c0, s0;               // corner_off[0], surf_off[0] (host copies)
  int n_surf_total;         // surf_off[n_scans] - surf_off[0]
  int dyn = 0;              // 1: the offsets were written on the device (per-scan SLAM step); n_records is then an upper bound and the
                            // record count is rec_off[n_scans]; c0 = s0 = 0 and n_surf_total is the surf cloud's CAPACITY (a layout constant)
};
__device__ __forceinline__ int batch_records(const BatchView& bv) {
  return bv.dyn ? min(bv.n_records, bv.rec_off[bv.n_scans]) : bv.n_records;
}

// scan owning global record index g (upper bound - 1 over rec_off)
__device__ __forceinline__ int find_scan(const int* __restrict__ rec_off, int n_scans, int g);
// the same for a whole wavefront of consecutive g: the binary search runs once on the scalar unit for
// the first lane's g, every lane then steps forward over the (rare) scan boundaries inside the wave
__device__ __forceinline__ int find_scan_wave(const int* __restrict__ rec_off, int n_scans, int g) {
  const int g0 = __builtin_amdgcn_readfirstlane(g);
  int b = __builtin_amdgcn_readfirstlane(find_scan(rec_off, n_scans, g0));
  while (b + 1 < n_scans && g >= rec_off[b + 1]) b++;
  return b;
}
__device__ __forceinline__ int find_scan(const int* __restrict__ rec_off, int n_scans, int g) {
  int lo = 0, hi = n_scans;      // invariant: rec_off[lo] <= g < rec_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rec_off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// Neighbour lists of the WHOLE-BATCH kernels (knn5_scan2map_split_kernel -> fit_scan2map_split_kernel; round 6): the five neighbours of
// corner feature f sit at slot (f - c0) of `nn`, those of surf feature f in the record tile that its plane record will occupy
// (plane_nn_store / plane_nn_load below) -- functions of the feature's index in its cloud array alone, like the record offsets.  The
// per-record kernels number `nn` by record (scan by scan, corners then surfs), which costs a wavefront the scan search and the offset
// loads before its first useful load; the fit kernel is a short latency chain at four wavefronts per SIMD and that prologue was a
// tenth of it.  Producer and consumer of a batch always use the same numbering.
__device__ __forceinline__ size_t corner_slot(const BatchView& bv, int f) { return (size_t)(f - bv.c0); }

// Record buffer (msfl_record_tiles.h): the PLANE records of the whole batch first, in lane-transposed tiles of 64 rows, then the edge
// records (6 doubles each); both are indexed by the feature's index in its cloud, so a record can be written from any processing
// order.  A plane row is only ever reached through plane_slot + plane_rec_load / plane_rec_store:
__device__ __forceinline__ size_t plane_slot(const BatchView& bv, int fi_surf) { return (size_t)(fi_surf - bv.s0); }
__device__ __forceinline__ size_t edge_rec_off(const BatchView& bv, int fi_corner) {
  return rec_edge((size_t)bv.n_surf_total, (size_t)(fi_corner - bv.c0));
}
// row {N.x, N.y, N.z, N.C} of plane slot g; rec: start of the record buffer
__device__ __forceinline__ void plane_rec_load(const double* rec, size_t g, double (&r)[4]) {
  const double2 a = *(const double2*)(rec + rec_tile_xy(g)), b = *(const double2*)(rec + rec_tile_zc(g));
  r[0] = a.x; r[1] = a.y; r[2] = b.x; r[3] = b.y;
}
__device__ __forceinline__ void plane_rec_store(double* rec, size_t g, double nx, double ny, double nz, double d0) {
  *(double2*)(rec + rec_tile_xy(g)) = make_double2(nx, ny);
  *(double2*)(rec + rec_tile_zc(g)) = make_double2(nz, d0);
}
// The whole-batch 5-NN list of plane slot g, kept in the tile between the 5-NN launch and the fit launch that turns the tile into
// records: {p0..p3} of the 64 lanes are the tile's first 1 024 bytes, p4 of the 64 lanes the next 256 -- whole lines either way.
__device__ __forceinline__ void plane_nn_store(double* rec, size_t g, int p0, int p1, int p2, int p3, int p4) {
  char* t = (char*)rec;
  *(int4*)(t + rec_tile_nn4(g)) = make_int4(p0, p1, p2, p3);
  *(int*)(t + rec_tile_nn1(g)) = p4;
}
__device__ __forceinline__ void plane_nn_load(const double* rec, size_t g, int (&p)[5]) {
  const char* t = (const char*)rec;
  const int4 a = *(const int4*)(t + rec_tile_nn4(g));
  p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = *(const int*)(t + rec_tile_nn1(g));
}

struct DeskewView {
  // all null for the plain (LiDAR-only) branch
  const double* corner_dq; const double* corner_dp;
  const double* surf_dq;   const double* surf_dp;
  const double* V;          // n_scans x 3 (device): Vi of every scan
  double G[3];
  const double* G_dev;      // gravity in device memory (the SLAM step's per-scan IMU block); null: G above
  double* pprime;           // out: n_records x 3, p' = dq*p + dp
};

// K4a: transform + exact 5-NN.  Low register count (no f64 fits here) -> 8 waves/SIMD to hide the
// latency of the scattered 16-byte candidate loads.  nn[5*g..] = positions in the sorted map (nearest first),
// nn[5*g] = -1 when the feature is rejected by the `pointSearchSqDis[4] < 1.0` gate (:128 / :198).
#ifndef MSFL_ASSOC_BLOCK
#define MSFL_ASSOC_BLOCK 64
#endif
constexpr int kAssocBlock = MSFL_ASSOC_BLOCK;      // threads per workgroup of the 5-NN and fit kernels
// PAIRS: scan b is registered against ITS OWN map (msfl_pairs.cuh): descriptor gcp[b] / gsp[b], cell table slice at cbase_*[b]
// DEFER: the capped walk of the whole-batch kernel (knn5_grid_k32), only for the counting instantiation: the candidate counter then
// reports what the timed launch evaluates
template <bool DESKEW, bool COUNT = false, bool PAIRS = false, bool DEFER = false>
__global__ void __launch_bounds__(kAssocBlock)
knn5_scan2map_kernel(BatchView bv, const double* __restrict__ poses, const int* __restrict__ status,
                     const GridDesc* __restrict__ gcp, const float4* __restrict__ map_c, const int* __restrict__ cs_c,
                     const GridDesc* __restrict__ gsp, const float4* __restrict__ map_s, const int* __restrict__ cs_s,
                     const int* __restrict__ pos_c, const int* __restrict__ pos_s,
                     float max_sq_dist, DeskewView dv, int* __restrict__ nn, unsigned long long* __restrict__ n_candidates = nullptr,
                     const int* __restrict__ cbase_c = nullptr, const int* __restrict__ cbase_s = nullptr) {
  const int g = bv.rec_begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= batch_records(bv)) return;
  const int b = find_scan_wave(bv.rec_off, bv.n_scans, g);
  int* out = nn + 5 * (size_t)g;
  if (status[b] != 0) { out[0] = -1; out[1] = -1; out[2] = -1; out[3] = -1; out[4] = -1; return; }
  const int local = g - bv.rec_off[b];
  const int nc = bv.corner_off[b + 1] - bv.corner_off[b];
  const bool is_edge = local < nc;
  const int fi = is_edge ? bv.corner_off[b] + local : bv.surf_off[b] + (local - nc);
  const float4 f = is_edge ? bv.corner[fi] : bv.surf[fi];
  const pose7 T = load_pose(poses + 7 * b);
  float3 q;
  if (DESKEW) {
    // mapping_scan_matcher.cc:120 / :190: pose * Rigid3d{q^-1 (Vi dt - G dt^2/2) + dp, dq}
    const double* dqp = is_edge ? dv.corner_dq + 4 * (size_t)fi : dv.surf_dq + 4 * (size_t)fi;
    const double* dpp = is_edge ? dv.corner_dp + 3 * (size_t)fi : dv.surf_dp + 3 * (size_t)fi;
    quat dq; dq.x = dqp[0]; dq.y = dqp[1]; dq.z = dqp[2]; dq.w = dqp[3];
    const d3 dp = mk3(dpp[0], dpp[1], dpp[2]);
    const double dt = (double)f.w;
    const double* Vb = dv.V + 3 * (size_t)b;
    const double Gv[3] = {dv.G_dev ? dv.G_dev[0] : dv.G[0], dv.G_dev ? dv.G_dev[1] : dv.G[1], dv.G_dev ? dv.G_dev[2] : dv.G[2]};
    const d3 shift = mk3(Vb[0] * dt - 0.5 * Gv[0] * dt * dt, Vb[1] * dt - 0.5 * Gv[1] * dt * dt,
                         Vb[2] * dt - 0.5 * Gv[2] * dt * dt);
    quat qc; qc.x = -T.q.x; qc.y = -T.q.y; qc.z = -T.q.z; qc.w = T.q.w;
    pose7 full;
    full.t = quat_rotate(T.q, quat_rotate(qc, shift) + dp) + T.t;       // Rigid3d operator*
    full.q = quat_normalized(quat_mul(T.q, dq));
    q = transform_point_f32(full, f.x, f.y, f.z);
    const d3 pp = quat_rotate(dq, mk3((double)f.x, (double)f.y, (double)f.z)) + dp;
    dv.pprime[3 * (size_t)g + 0] = pp.x; dv.pprime[3 * (size_t)g + 1] = pp.y; dv.pprime[3 * (size_t)g + 2] = pp.z;
  } else {
    q = transform_point_f32(T, f.x, f.y, f.z);                          // :123 / :193
  }
  Top5 t;
  int n_cand = 0;
  // the walk on truncated 32-bit keys first (Top6K); a lane it leaves ambiguous is searched again with the exact keys below
  __shared__ int s_slot[(kTopSlots + (DEFER ? kDeferSlots : 0)) * kAssocBlock];
  Top6K tk;
  top_init(tk, max_sq_dist, s_slot + threadIdx.x);
  if (is_edge) { const GridDesc gc = gcp[PAIRS ? b : 0]; knn5_grid_k32<kAssocBlock, DEFER>(gc, map_c, cs_c, q, tk, n_cand, PAIRS ? cbase_c[b] : 0); }
  else { const GridDesc gs = gsp[PAIRS ? b : 0]; knn5_grid_k32<kAssocBlock, DEFER>(gs, map_s, cs_s, q, tk, n_cand, PAIRS ? cbase_s[b] : 0); }
  const bool settled = top_settled(tk, max_sq_dist);
  if (!settled) {
    int n_again = 0;                   // the candidate counter reports the first walk
    top5_init(t, max_sq_dist);
    if (is_edge) { const GridDesc gc = gcp[PAIRS ? b : 0]; knn5_grid(gc, map_c, cs_c + (PAIRS ? cbase_c[b] : 0), q, t, n_again); }
    else { const GridDesc gs = gsp[PAIRS ? b : 0]; knn5_grid(gs, map_s, cs_s + (PAIRS ? cbase_s[b] : 0), q, t, n_again); }
  }
  if (COUNT) {                                                  // one atomic per wavefront: sum over the lanes still here
    const unsigned long long act = __ballot(1);
    unsigned long long m = act;
    int tot = 0;
    while (m) { const int l = __ffsll((long long)m) - 1; tot += __shfl(n_cand, l); m &= m - 1; }
    if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(n_candidates, (unsigned long long)tot);
  }
  if (settled) {
    if (top_found(tk)) {                                                              // :128 / :198: the 5th is below the gate
      out[0] = top_pos<kAssocBlock>(tk, tk.k0); out[1] = top_pos<kAssocBlock>(tk, tk.k1); out[2] = top_pos<kAssocBlock>(tk, tk.k2);
      out[3] = top_pos<kAssocBlock>(tk, tk.k3); out[4] = top_pos<kAssocBlock>(tk, tk.k4);   // nearest first, positions in the sorted map
    } else {
      out[0] = -1; out[1] = -1; out[2] = -1; out[3] = -1; out[4] = -1;
    }
    return;
  }
  if ((unsigned int)t.k4 != 0xffffffffu && (double)top5_d4(t) < (double)max_sq_dist) {      // :128 / :198
    // original map index -> position in the sorted map array (the fit kernel then gathers directly);
    // done here because this kernel runs at 8 waves/SIMD and hides the extra dependent load
    const int* po = is_edge ? pos_c : pos_s;
    out[0] = po[(unsigned int)t.k0]; out[1] = po[(unsigned int)t.k1]; out[2] = po[(unsigned int)t.k2];
    out[3] = po[(unsigned int)t.k3]; out[4] = po[(unsigned int)t.k4];       // nearest first
  } else {
    out[0] = -1; out[1] = -1; out[2] = -1; out[3] = -1; out[4] = -1;   // all five: the fit kernel loads them unconditionally
  }
}

// a load the caller knows to be wave-uniform and of memory no thread of this kernel writes: emitted as a scalar load
template <class V>
__device__ __forceinline__ V uniform_load(const V* p) {
  return *(const __attribute__((address_space(4))) V*)(unsigned long long)p;
}

// K4a for a whole large batch of the plain branch: blocks [0, edge_blocks) serve the corner features (corner map index), the rest
// the surf features, so that a wavefront never holds both kinds and each body knows its map at compile time.
template <bool EDGE, bool DEFER>
__device__ __forceinline__ void knn5_one_kind(const BatchView& bv, const double* __restrict__ poses, const int* __restrict__ status,
                                              const GridDesc* __restrict__ gp, const float4* __restrict__ map, const int* __restrict__ cs,
                                              const int* __restrict__ po, float max_sq_dist, int* __restrict__ nn, double* __restrict__ rec, int block, int* s_slot) {
  const int* off = EDGE ? bv.corner_off : bv.surf_off;
  const int f_i = off[0] + block * (int)blockDim.x + (int)threadIdx.x;
  if (f_i >= off[bv.n_scans]) return;
  // Nearly every wavefront lies inside ONE scan (two boundaries per scan in ~78 wavefronts): its scan number, offsets, status and
  // pose are then read through the scalar unit — the kernel is bound by vector-memory instruction issue as much as by VALU issue
  // (texture addresser ~80 % busy, profiles/r04b_knn_ta.md), and these were ten of its ~92 vector loads per wavefront.
  const int b0 = __builtin_amdgcn_readfirstlane(find_scan(off, bv.n_scans, __builtin_amdgcn_readfirstlane(f_i)));
  int b, st; pose7 T;
  if (__all(f_i < off[b0 + 1])) {
    // loads through the constant address space (written by earlier kernels only), so that they stay scalar loads: with plain loads
    // the optimiser merges the two branches into one set of per-lane loads again
    b = b0;
    st = uniform_load(status + b0);
    const double* pp = poses + 7 * b0;
    T.t = mk3(uniform_load(pp), uniform_load(pp + 1), uniform_load(pp + 2));
    T.q.x = uniform_load(pp + 3); T.q.y = uniform_load(pp + 4); T.q.z = uniform_load(pp + 5); T.q.w = uniform_load(pp + 6);
  } else {
    b = b0;
    while (b + 1 < bv.n_scans && f_i >= off[b + 1]) b++;
    st = status[b];
    T = load_pose(poses + 7 * b);
  }
  // nearest first; all five are always written: the fit kernel loads them unconditionally.  A corner feature's list goes to its slot of
  // `nn`, a surf feature's into the record tile its plane record will occupy (msfl_record_tiles.h)
  auto put = [&](int p0, int p1, int p2, int p3, int p4) __attribute__((always_inline)) {
    if (EDGE) { int* out = nn + 5 * corner_slot(bv, f_i); out[0] = p0; out[1] = p1; out[2] = p2; out[3] = p3; out[4] = p4; }
    else plane_nn_store(rec, plane_slot(bv, f_i), p0, p1, p2, p3, p4);
  };
  if (st != 0) { put(-1, -1, -1, -1, -1); return; }
  const float4 f = EDGE ? bv.corner[f_i] : bv.surf[f_i];
  const float3 q = transform_point_f32(T, f.x, f.y, f.z);                          // :123 / :193
  int n_cand = 0;
  const GridDesc gd = *gp;
  Top6K tk;
  top_init(tk, max_sq_dist, s_slot + threadIdx.x);
  knn5_grid_k32<kAssocBlock, DEFER>(gd, map, cs, q, tk, n_cand);
  if (top_settled(tk, max_sq_dist)) {
    if (top_found(tk)) {                                                              // :128 / :198: the 5th is below the gate (t differs from the gate's)
      put(top_pos<kAssocBlock>(tk, tk.k0), top_pos<kAssocBlock>(tk, tk.k1), top_pos<kAssocBlock>(tk, tk.k2),
          top_pos<kAssocBlock>(tk, tk.k3), top_pos<kAssocBlock>(tk, tk.k4));   // positions in the sorted map
    } else {
      put(-1, -1, -1, -1, -1);
    }
    return;
  }
  // ambiguous under the truncated keys: the exact (distance, index) search
  Top5 t;
  top5_init(t, max_sq_dist);
  knn5_grid(gd, map, cs, q, t, n_cand);
  if ((unsigned int)t.k4 != 0xffffffffu && (double)top5_d4(t) < (double)max_sq_dist) {      // :128 / :198
    put(po[(unsigned int)t.k0], po[(unsigned int)t.k1], po[(unsigned int)t.k2], po[(unsigned int)t.k3], po[(unsigned int)t.k4]);
  } else {
    put(-1, -1, -1, -1, -1);
  }
}
// DEFER: capped row visits, the rest of a long range walked after the ninth row (knn5_grid_k32); the handle picks the form (MSFL_KNN_DEFER)
template <bool DEFER>
__global__ void __launch_bounds__(kAssocBlock)
knn5_scan2map_split_kernel(BatchView bv, const double* __restrict__ poses, const int* __restrict__ status,
                           const GridDesc* __restrict__ gcp, const float4* __restrict__ map_c, const int* __restrict__ cs_c,
                           const GridDesc* __restrict__ gsp, const float4* __restrict__ map_s, const int* __restrict__ cs_s,
                           const int* __restrict__ pos_c, const int* __restrict__ pos_s, float max_sq_dist, int* __restrict__ nn,
                           double* __restrict__ rec, int edge_blocks) {
  __shared__ int s_slot[(kTopSlots + (DEFER ? kDeferSlots : 0)) * kAssocBlock];        // Top6K's slot table: 6 positions per lane; DEFER: the lanes' range stacks
  if ((int)blockIdx.x < edge_blocks) knn5_one_kind<true, DEFER>(bv, poses, status, gcp, map_c, cs_c, pos_c, max_sq_dist, nn, rec, (int)blockIdx.x, s_slot);
  else knn5_one_kind<false, DEFER>(bv, poses, status, gsp, map_s, cs_s, pos_s, max_sq_dist, nn, rec, (int)blockIdx.x - edge_blocks, s_slot);
}

// K4a, latency form: the same exact 5-NN for a launch too small to fill the machine (one scan per call: ~5 000 queries are
// 80 wavefronts on 1 024 SIMDs, and a query is a chain of up to nine dependent row-bound -> candidate load round trips,
// ~35 us).  Sixteen lanes serve one query: lane r < 9 owns row r of the 3 x 3 (y, z) neighbourhood, reads its two row
// bounds and scans its candidates into a private top-5 against the acceptance gate only (rows are not pruned against
// each other: that would serialise them again), then the nine sorted lists are merged by five rounds of "smallest head
// of the group".  Keys are (distance bits, map index), so the five survivors and their order are exactly those of
// knn5_grid: an exact top-5 does not depend on the visit order.  Lanes 0..4 translate and store one neighbour each.
constexpr int kKnnRowLanes = 16;
constexpr int kKnnRowsBlock = 256;
#ifndef MSFL_KNN_ROWS_MAX
#define MSFL_KNN_ROWS_MAX 32768
#endif
constexpr int kKnnRowsMaxRecords = MSFL_KNN_ROWS_MAX;   // launches of up to this many queries take the latency form (measured crossover: DESIGN.md)
__global__ void __launch_bounds__(kKnnRowsBlock)
knn5_scan2map_rows_kernel(BatchView bv, const double* __restrict__ poses, const int* __restrict__ status,
                          const GridDesc* __restrict__ gcp, const float4* __restrict__ map_c, const int* __restrict__ cs_c,
                          const GridDesc* __restrict__ gsp, const float4* __restrict__ map_s, const int* __restrict__ cs_s,
                          const int* __restrict__ pos_c, const int* __restrict__ pos_s, float max_sq_dist, int* __restrict__ nn) {
  const int sl = threadIdx.x & (kKnnRowLanes - 1);
  const int g = bv.rec_begin + (int)((blockIdx.x * kKnnRowsBlock + threadIdx.x) / kKnnRowLanes);
  if (g >= batch_records(bv)) return;                         // whole groups leave together
  const int b = find_scan(bv.rec_off, bv.n_scans, g);
  int* out = nn + 5 * (size_t)g;
  if (status[b] != 0) { if (sl < 5) out[sl] = -1; return; }
  const int local = g - bv.rec_off[b];
  const int nc = bv.corner_off[b + 1] - bv.corner_off[b];
  const bool is_edge = local < nc;
  const int fi = is_edge ? bv.corner_off[b] + local : bv.surf_off[b] + (local - nc);
  const float4 f = is_edge ? bv.corner[fi] : bv.surf[fi];
  const pose7 T = load_pose(poses + 7 * b);
  const float3 q = transform_point_f32(T, f.x, f.y, f.z);    // :123 / :193
  const GridDesc gd = is_edge ? *gcp : *gsp;
  const float4* __restrict__ sorted = is_edge ? map_c : map_s;
  const int* __restrict__ cell_start = is_edge ? cs_c : cs_s;
  Top5 t;
  top5_init(t, max_sq_dist);
  const unsigned long long sentinel = t.k0;
  const GridQuery w = grid_query(gd, q);
  const int y = w.cy + (sl % 3) - 1, z = w.cz + (sl / 3) - 1;
  if (sl < 9 && w.xs <= w.xe && y >= 0 && y < gd.dy && z >= 0 && z < gd.dz) {
    const float gy = axis_gap(w.uy, y), gz = axis_gap(w.uz, z);
    const float row2 = (gy * gy + gz * gz) * gd.cell2;
    if (!(row2 > max_sq_dist)) {
      // end cells whose lower bound is beyond the gate hold no acceptable candidate
      float gxa[kGridXSub], gxb[kGridXSub];
      grid_x_bounds(gd, w, gxa, gxb);
      int a = w.xs, e_cell = w.xe;
      bool da = true, db = true;
#pragma unroll
      for (int k = 0; k < kGridXSub; k++) {
        da = da && (row2 + gxa[k] > max_sq_dist); a += da ? 1 : 0;
        db = db && (row2 + gxb[k] > max_sq_dist); e_cell -= db ? 1 : 0;
      }
      if (a <= e_cell) {
        const int row = (z * gd.dy + y) * gd.dx;
        const int s = cell_start[row + a], e = cell_start[row + e_cell + 1];
        const msfl_f2 qxy = {q.x, q.y};
        for (int i = s; i < e; i += 4) {                    // four loads requested together (clamped index)
          float4 m[4];
#pragma unroll
          for (int u = 0; u < 4; u++) { m[u] = sorted[min(i + u, e - 1)]; asm volatile("" : "+v"(m[u].w)); }
#pragma unroll
          for (int u = 0; u < 4; u++)
            if (i + u < e) top5_insert(t, l2_simple_pk(m[u], qxy, q.z), __float_as_int(m[u].w));
        }
      }
    }
  }
  // merge: five times the smallest head of the group's (sorted) lists; the owner pops.  Map indices are unique, so
  // real keys are too; equal heads are sentinels, and popping a sentinel list changes nothing.
  unsigned long long best[5];
#pragma unroll
  for (int j = 0; j < 5; j++) {
    unsigned long long m = t.k0;
#pragma unroll
    for (int o = kKnnRowLanes / 2; o > 0; o >>= 1) {
      const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)m, o, kKnnRowLanes), hi = (unsigned)__shfl_xor((int)(unsigned)(m >> 32), o, kKnnRowLanes);
      const unsigned long long other = ((unsigned long long)hi << 32) | lo;
      m = other < m ? other : m;
    }
    best[j] = m;
    if (t.k0 == m) { t.k0 = t.k1; t.k1 = t.k2; t.k2 = t.k3; t.k3 = t.k4; t.k4 = sentinel; }
  }
  if (sl >= 5) return;
  const bool accepted = (unsigned int)best[4] != 0xffffffffu && (double)__uint_as_float((unsigned int)(best[4] >> 32)) < (double)max_sq_dist;   // :128 / :198
  const unsigned long long mine = sl == 0 ? best[0] : sl == 1 ? best[1] : sl == 2 ? best[2] : sl == 3 ? best[3] : best[4];
  const int* po = is_edge ? pos_c : pos_s;
  out[sl] = accepted ? po[(unsigned int)mine] : -1;           // nearest first
}

// K4b: 5 neighbours -> line fit (3x3 Jacobi eigen) / plane fit (5x3 Householder QR) -> record.
// Edge: {C, N}.  Plane: {N, N.C} (the residual N.(Rp+t-C) only needs the offset N.C).
// `full` (optional, debug/parity API) receives {C, N} for every feature.
#ifndef MSFL_FIT_WAVES
#define MSFL_FIT_WAVES 1
#endif
// KIND 0: every record of [rec_begin, n_records) (one thread each, edges and planes as they come); KIND 1 / 2: the launch covers
// the batch's corner / surf features only (thread = feature index in its cloud), so that the compiler sees one of the two fits.
// The whole-batch plane form (KIND 2) reads its neighbour lists from `rec` itself: one wavefront owns one tile (thread = plane slot, 64
// consecutive slots per wavefront), loads the tile's lists and overwrites the tile with the records.  A lane's {N.z, N.C} covers the
// bytes of other lanes' p4, so `rec` is not __restrict__ and the loads are pinned ahead of everything that follows; they sit in
// uniform control flow, so all 64 lists have been requested by one instruction each before any lane can store.
template <bool DESKEW, int KIND>
__device__ __forceinline__ void fit_one(const BatchView& bv, const float4* __restrict__ map_c, const float4* __restrict__ map_s,
                                        const int* nn, double line_ratio, double plane_tol, const DeskewView& dv,
                                        double* rec, double* __restrict__ full, int block) {
  static_assert(kAssocBlock % kRecTileRows == 0, "a wavefront of the whole-batch fit owns one record tile");
  int g = 0, b = 0, local = 0, nc = 0, fi = 0;
  size_t slot = 0;
  if (KIND == 0) {
    g = bv.rec_begin + block * blockDim.x + threadIdx.x;
    if (g >= batch_records(bv)) return;
    b = find_scan_wave(bv.rec_off, bv.n_scans, g);
    local = g - bv.rec_off[b];
    nc = bv.corner_off[b + 1] - bv.corner_off[b];
    slot = (size_t)g;
  } else {
    // whole-batch form: neighbour slot and record offset are functions of the feature's index alone (corner_slot, plane_slot): no scan
    // search, the wavefront's first load is its neighbour list
    fi = (KIND == 1 ? bv.c0 : bv.s0) + block * blockDim.x + threadIdx.x;
    if (fi >= (KIND == 1 ? bv.c0 + (bv.n_records - bv.n_surf_total) : bv.s0 + bv.n_surf_total)) return;
    if (KIND == 1) slot = corner_slot(bv, fi);
  }
  const bool is_edge = KIND == 0 ? local < nc : KIND == 1;
  FitOut fo; fo.ok = false; fo.C = mk3(0, 0, 0); fo.N = mk3(0, 0, 0);
  // all five indices at once and the five neighbours unconditionally (index 0 stands in when there is no match): behind the
  // `p0 >= 0` test the loads came as three dependent round trips (first index, the other four, the points)
  int pl[5];
  if (KIND == 2) { plane_nn_load(rec, plane_slot(bv, fi), pl); asm volatile("" ::: "memory"); }
  else { const int* in = nn + 5 * slot; pl[0] = in[0]; pl[1] = in[1]; pl[2] = in[2]; pl[3] = in[3]; pl[4] = in[4]; }
  const int p0 = pl[0], p1 = pl[1], p2 = pl[2], p3 = pl[3], p4 = pl[4];
  const float4* mp = is_edge ? map_c : map_s;
  const bool have = p0 >= 0;                                  // no match: the other four slots were never written
  const float4 nb[5] = {mp[have ? p0 : 0], mp[have ? p1 : 0], mp[have ? p2 : 0], mp[have ? p3 : 0], mp[have ? p4 : 0]};
  if (p0 >= 0) {
    fo = is_edge ? edge_fit(nb, line_ratio) : plane_fit(nb, plane_tol);
    if (DESKEW && fo.ok) {
      // C' = C - (Vi dt - G dt^2/2): the velocity block is constant (mapping_scan_matcher.cc:94)
      static_assert(!DESKEW || KIND == 0, "the de-skew branch runs the per-record kernel");
      const int fd = is_edge ? bv.corner_off[b] + local : bv.surf_off[b] + (local - nc);
      const double dt = (double)(is_edge ? bv.corner[fd].w : bv.surf[fd].w);
      const double* Vb = dv.V + 3 * (size_t)b;
      const double Gv[3] = {dv.G_dev ? dv.G_dev[0] : dv.G[0], dv.G_dev ? dv.G_dev[1] : dv.G[1], dv.G_dev ? dv.G_dev[2] : dv.G[2]};
      fo.C = fo.C - mk3(Vb[0] * dt - 0.5 * Gv[0] * dt * dt, Vb[1] * dt - 0.5 * Gv[1] * dt * dt,
                        Vb[2] * dt - 0.5 * Gv[2] * dt * dt);
    }
  }
  if (is_edge) {
    double* out = rec + edge_rec_off(bv, KIND == 0 ? bv.corner_off[b] + local : fi);
    out[0] = fo.C.x; out[1] = fo.C.y; out[2] = fo.C.z;
    out[3] = fo.N.x; out[4] = fo.N.y; out[5] = fo.N.z;
  } else {
    plane_rec_store(rec, plane_slot(bv, KIND == 0 ? bv.surf_off[b] + (local - nc) : fi), fo.N.x, fo.N.y, fo.N.z, dot(fo.N, fo.C));
  }
  if (KIND == 0 && full) {                                      // (the whole-batch form is not launched with a `full` output)
    double* o = full + 6 * (size_t)g;
    o[0] = fo.C.x; o[1] = fo.C.y; o[2] = fo.C.z; o[3] = fo.N.x; o[4] = fo.N.y; o[5] = fo.N.z;
  }
}

template <bool DESKEW>
__global__ void __launch_bounds__(kAssocBlock, MSFL_FIT_WAVES)
fit_scan2map_kernel(BatchView bv, const float4* __restrict__ map_c, const float4* __restrict__ map_s,
                    const int* __restrict__ nn, double line_ratio, double plane_tol, DeskewView dv,
                    double* __restrict__ rec, double* __restrict__ full) {
  fit_one<DESKEW, 0>(bv, map_c, map_s, nn, line_ratio, plane_tol, dv, rec, full, (int)blockIdx.x);
}
// A whole large batch (plain branch): blocks [0, edge_blocks) fit the corner features, the rest the surf features, each
// through its own specialisation of the body, at four wavefronts per SIMD (the plane fit alone needs 131 registers, the
// mixed body 135: three wavefronts).  The edge blocks come first so that their longer per-record chain (the Jacobi
// eigen-solver) runs under the plane blocks instead of forming the launch's tail.
#ifndef MSFL_FIT_SPLIT_WAVES
#define MSFL_FIT_SPLIT_WAVES 4
#endif
__global__ void __launch_bounds__(kAssocBlock, MSFL_FIT_SPLIT_WAVES)
fit_scan2map_split_kernel(BatchView bv, const float4* __restrict__ map_c, const float4* __restrict__ map_s,
                          const int* nn, double line_ratio, double plane_tol, DeskewView dv,
                          double* rec, double* __restrict__ full, int edge_blocks) {      // (rec: see fit_one)
  if ((int)blockIdx.x < edge_blocks) fit_one<false, 1>(bv, map_c, map_s, nn, line_ratio, plane_tol, dv, rec, full, (int)blockIdx.x);
  else fit_one<false, 2>(bv, map_c, map_s, nn, line_ratio, plane_tol, dv, rec, full, (int)blockIdx.x - edge_blocks);
}

// {C, N} x n_records (host/debug format) -> compact internal records
__global__ void __launch_bounds__(256) pack_records_kernel(BatchView bv, const double* __restrict__ full, double* __restrict__ rec) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= batch_records(bv)) return;
  const int b = find_scan_wave(bv.rec_off, bv.n_scans, g);
  const int local = g - bv.rec_off[b];
  const int nc = bv.corner_off[b + 1] - bv.corner_off[b];
  const double* in = full + 6 * (size_t)g;
  if (local < nc) {
    double* out = rec + edge_rec_off(bv, bv.corner_off[b] + local);
#pragma unroll
    for (int k = 0; k < 6; k++) out[k] = in[k];
  } else {
    plane_rec_store(rec, plane_slot(bv, bv.surf_off[b] + (local - nc)), in[3], in[4], in[5], in[3] * in[0] + in[4] * in[1] + in[5] * in[2]);
  }
}

// ---------------------------------------------------------------------------------------------
// K5 + K6: persistent per-scan trust-region LM with Huber loss (Ceres semantics)
// ---------------------------------------------------------------------------------------------

struct SolverParams {
  int    max_iterations;
  double huber;
  double radius0, radius_max, radius_min;
  double min_relative_decrease, min_diag, max_diag;
  double ftol, gtol, ptol;
  int    max_invalid;
  int    min_correspondences;   // 0 for the mapping matcher, 10 for odometry (.cc:262)
};

struct DevMatchInfo {   // mirrors msfl_match_info
  int status;
  int n_edge[2], n_plane[2];
  int lm_iterations[2], lm_successful[2];
  double initial_cost[2], final_cost[2];
};

constexpr int kAcc = 28;   // cost + g[6] + H upper[21]
static_assert(kAcc + 2 == 30, "block_reduce folds 30 values");

// ---- robustified normal equations, one residual row at a time ----------------------------------------------
// Ceres scales residual and Jacobian of a block by sqrt(rho') (Corrector with rho'' <= 0) and then forms
// J^T J / J^T r.  The products only ever contain sqrt(rho')^2, so the accumulation below weights the row
// with w = rho' directly: no square root per record, results equal up to the rounding of sqrt(w)^2 vs w.
// j[0..2] = d r/d t, j[3..5] = d r/d theta (tangent space, lidar_factor.cc:19,39 in closed form).
__device__ __forceinline__ void acc_row_w(double (&acc)[kAcc], const double (&j)[6], double r, double w) {
  double jw[6];
#pragma unroll
  for (int k = 0; k < 6; k++) jw[k] = w * j[k];
#pragma unroll
  for (int k = 0; k < 6; k++) acc[1 + k] = __builtin_fma(jw[k], r, acc[1 + k]);
  int n = 7;
#pragma unroll
  for (int p2 = 0; p2 < 6; p2++)
#pragma unroll
    for (int q = p2; q < 6; q++) { acc[n] = __builtin_fma(jw[p2], j[q], acc[n]); n++; }
}

// HuberLoss(a) on s = |r|^2 given |r|: rho0 = rho(s), w = rho'(s) (Ceres loss_function.cc; the Corrector's
// max(DBL_MIN, .) guard is kept)
__device__ __forceinline__ void huber_weight(double a, double s, double abs_r, double& rho0, double& w) {
  const double b = a * a;
  if (s > b) {
    rho0 = 2.0 * a * abs_r - b;
    w = fmax(2.2250738585072014e-308, a * fast_rcp(abs_r));
  } else {
    rho0 = s; w = 1.0;
  }
}

// One evaluation pass of a scan's records at pose T: cost, g = J^T r, H = J^T J (robustified,
// tangent space).  lidar_factor.cc:7-44 + Ceres HuberLoss/Corrector.
// LDS-resident copy of the first K plane records + their points (44 B each, structure of arrays so
// that consecutive lanes hit consecutive banks).  A solve re-reads every record in each of its ~4-7
// evaluation passes: what fits here is fetched from HBM once per solve instead of once per pass.
#ifndef MSFL_LM_BLOCK
#define MSFL_LM_BLOCK 128
#endif
constexpr int kLmBlock = MSFL_LM_BLOCK;                        // threads per scan in the scan-to-map LM solve
#ifndef MSFL_ODOM_LM_BLOCK
#define MSFL_ODOM_LM_BLOCK 128
#endif
constexpr int kOdomLmBlock = MSFL_ODOM_LM_BLOCK;               // scan-to-scan: ~500 records per pair
// cache sizes per workgroup size: 76 KB x 2 workgroups per CU (256 threads), 36.6 KB x 4 (128: the small
// scan-to-scan problems, measured 0.365 ms per call vs 0.448 with 256 threads and 0.382 with 64), 17 KB x 8 (64:
// one wavefront per problem, no cross-wave barrier)
// 512 threads: the one-solve-per-call SLAM step, where the machine is empty and a solve is as long as its chain of passes
// (3 072 planes x 44 B = 132 KB, one workgroup per CU)
// trips of the streamed plane loop whose loads are requested together (see evaluate_pass): 512 threads have <= 10 trips in all
#ifndef MSFL_LM_GROUP_SMALL
#define MSFL_LM_GROUP_SMALL 8
#endif
#ifndef MSFL_LM_GROUP_LARGE
#define MSFL_LM_GROUP_LARGE 4
#endif
constexpr int lm_load_group(int block) { return block >= 512 ? MSFL_LM_GROUP_LARGE : MSFL_LM_GROUP_SMALL; }
constexpr int lm_plane_cache(int block) {
#ifdef MSFL_LM_PLANE_CACHE
  return block == 256 ? MSFL_LM_PLANE_CACHE : block == 128 ? 832 : block == 512 ? 3072 : 384;
#else
  return block == 256 ? 1728 : block == 128 ? 832 : block == 512 ? 3072 : 384;
#endif
}
template <int BLOCK>
struct PlaneCache {
  static constexpr int kPlanes = lm_plane_cache(BLOCK);
  double nx[kPlanes], ny[kPlanes], nz[kPlanes], d0[kPlanes];
  float px[kPlanes], py[kPlanes], pz[kPlanes];
};

// Accepted edge correspondences of a solve, in index order.  Only ~40 % of the corner features pass the line test,
// and an edge row costs 2.7 plane rows: the first pass marks the accepted ones in a bit mask, wavefront 0 turns the
// mask into a dense index list, and the later passes (4 of 5) walk the list, so their lanes are all busy.
constexpr int kEdgeListMax = 1024;                 // edges beyond this index keep the checked walk
struct EdgeList {
  unsigned mask[kEdgeListMax / 32];
  unsigned short idx[kEdgeListMax];
  int n;
};

// FILL: first pass of a solve (records come from global memory and are copied into the cache);
// later passes read the cached part from LDS.  A thread only ever re-reads entries it wrote itself
// (same i -> thread mapping in every pass), so no barrier is needed around the cache.
#ifdef MSFL_LM_PROFILE
__device__ unsigned long long g_lm_prof[8];   // cycles (lane 0, summed over workgroups): eval, reduce, serial, total, passes
#define LM_T(x) const unsigned long long x = wall_clock64()
#ifndef MSFL_LM_PROFILE_BLOCK
#define MSFL_LM_PROFILE_BLOCK 0      /* 0: every instantiation; else only the one with this many threads */
#endif
#define LM_ADD(k, v) if (threadIdx.x == 0 && (MSFL_LM_PROFILE_BLOCK == 0 || MSFL_LM_PROFILE_BLOCK == (int)blockDim.x)) atomicAdd(&g_lm_prof[k], (unsigned long long)(v))
#else
#define LM_T(x)
#define LM_ADD(k, v)
#endif

__device__ __forceinline__ d3 lm_rotate(const quat& q, d3 v) { return quat_rotate(q, v); }

template <int BLOCK, bool FILL>
__device__ __forceinline__ void evaluate_pass(const pose7& T, double huber,
                                              const float4* __restrict__ corner, int nc,
                                              const float4* __restrict__ surf, int ns,
                                              const double* __restrict__ pprime,   // may be null
                                              const double* __restrict__ rec,      // this scan's edge records
                                              const double* __restrict__ recp,     // the record buffer (plane tiles first) ...
                                              size_t g0,                           // ... and this scan's first plane slot in it
                                              PlaneCache<BLOCK>& pc, EdgeList& el,
                                              double (&acc)[kAcc], int& n_edge, int& n_plane) {
#pragma unroll
  for (int k = 0; k < kAcc; k++) acc[k] = 0.0;
  n_edge = 0; n_plane = 0;
  const mat3 R = quat_to_matrix(T.q);
  LM_T(t_eval_begin);
  // edges: {C, N}, r = N x (R p + t - C)                                       lidar_factor.cc:12
  // FILL: every edge, accepted ones marked; later passes: the dense list first, then the unlisted tail
  const int n_listed = FILL ? 0 : el.n;
  const int n_walk = FILL ? nc : n_listed + max(nc - kEdgeListMax, 0);
  auto edge_row = [&](int i, d3 C, d3 N, d3 p) __attribute__((always_inline)) {
    if (N.x == 0.0 && N.y == 0.0 && N.z == 0.0) return;        // rejected correspondence (never a listed one)
    if (FILL && i < kEdgeListMax) atomicOr(&el.mask[i >> 5], 1u << (i & 31));
    n_edge++;
    // d = R p + t - C through the rotation matrix (the quaternion sandwich costs three times the instructions; the two agree
    // to rounding), r = N x d
    const d3 d = mk3(__builtin_fma(R.m[0], p.x, __builtin_fma(R.m[1], p.y, R.m[2] * p.z)) + (T.t.x - C.x),
                     __builtin_fma(R.m[3], p.x, __builtin_fma(R.m[4], p.y, R.m[5] * p.z)) + (T.t.y - C.y),
                     __builtin_fma(R.m[6], p.x, __builtin_fma(R.m[7], p.y, R.m[8] * p.z)) + (T.t.z - C.z));
    const d3 r = mk3(__builtin_fma(N.y, d.z, -(N.z * d.y)), __builtin_fma(N.z, d.x, -(N.x * d.z)), __builtin_fma(N.x, d.y, -(N.y * d.x)));
    const double s = __builtin_fma(r.x, r.x, __builtin_fma(r.y, r.y, r.z * r.z));
    double rho0 = s, w = 1.0;
    if (s > huber * huber) {                                     // rho acts on the 3-vector norm of the block
      const double inv = fast_rsqrt(s);
      rho0 = 2.0 * huber * (s * inv) - huber * huber;
      w = fmax(2.2250738585072014e-308, huber * inv);
    }
    acc[0] += 0.5 * rho0;
    // rows of skew(N) (:18-19): a0 = (0, -Nz, Ny), a1 = (Nz, 0, -Nx), a2 = (-Ny, Nx, 0); rotation part p x (R^T a_k),
    // R^T a_k from two rows of R each
    const d3 l0 = mk3(__builtin_fma(N.y, R.m[6], -(N.z * R.m[3])), __builtin_fma(N.y, R.m[7], -(N.z * R.m[4])), __builtin_fma(N.y, R.m[8], -(N.z * R.m[5])));
    const d3 l1 = mk3(__builtin_fma(N.z, R.m[0], -(N.x * R.m[6])), __builtin_fma(N.z, R.m[1], -(N.x * R.m[7])), __builtin_fma(N.z, R.m[2], -(N.x * R.m[8])));
    const d3 l2 = mk3(__builtin_fma(N.x, R.m[3], -(N.y * R.m[0])), __builtin_fma(N.x, R.m[4], -(N.y * R.m[1])), __builtin_fma(N.x, R.m[5], -(N.y * R.m[2])));
    const d3 b0 = cross(p, l0), b1 = cross(p, l1), b2 = cross(p, l2);
    const double j0[6] = {0.0, -N.z, N.y, b0.x, b0.y, b0.z};
    const double j1[6] = {N.z, 0.0, -N.x, b1.x, b1.y, b1.z};
    const double j2[6] = {-N.y, N.x, 0.0, b2.x, b2.y, b2.z};
    acc_row_w(acc, j0, r.x, w);
    acc_row_w(acc, j1, r.y, w);
    acc_row_w(acc, j2, r.z, w);
  };
  // planes: {N, N.C}, r = N.(R p + t) - N.C                                    lidar_factor.cc:32
  const bool use_cache = (pprime == nullptr);       // deskew keeps f64 points in global memory
  auto plane_row = [&](d3 N, double d0, d3 p) __attribute__((always_inline)) {
    if (N.x == 0.0 && N.y == 0.0 && N.z == 0.0) return;        // rejected correspondence
    n_plane++;
    // r = N.(R p + t) - d0 = (R^T N).p + (N.t - d0): the vector l = R^T N is what the Jacobian's rotation part
    // p x (R^T N) needs anyway (:38-39), so the residual costs six fused multiply-adds on top of it
    const d3 l = mk3(__builtin_fma(R.m[0], N.x, __builtin_fma(R.m[3], N.y, R.m[6] * N.z)),
                     __builtin_fma(R.m[1], N.x, __builtin_fma(R.m[4], N.y, R.m[7] * N.z)),
                     __builtin_fma(R.m[2], N.x, __builtin_fma(R.m[5], N.y, R.m[8] * N.z)));
    const double nt = __builtin_fma(N.x, T.t.x, __builtin_fma(N.y, T.t.y, __builtin_fma(N.z, T.t.z, -d0)));
    const double r = __builtin_fma(l.x, p.x, __builtin_fma(l.y, p.y, __builtin_fma(l.z, p.z, nt)));
    const d3 b = cross(p, l);
    double rho0, w; huber_weight(huber, r * r, fabs(r), rho0, w);
    acc[0] += 0.5 * rho0;
    const double j[6] = {N.x, N.y, N.z, b.x, b.y, b.z};
    acc_row_w(acc, j, r, w);
  };
  // (a) the LDS-resident head of the plane list (later passes; a thread reads back what it wrote itself)
  int i = threadIdx.x;
  auto cached_planes = [&]() __attribute__((always_inline)) {
    if (!FILL && use_cache) {
      for (; i < min(ns, PlaneCache<BLOCK>::kPlanes); i += BLOCK)
        plane_row(mk3(pc.nx[i], pc.ny[i], pc.nz[i]), pc.d0[i], mk3((double)pc.px[i], (double)pc.py[i], (double)pc.pz[i]));
    }
  };
  if (pprime == nullptr) {
    // Round 6 (profiles/r06_lm_ablation.md: the edge rows were two to four DEPENDENT memory round trips per pass, 3.4 us of a 28 us pass and
    // 8 us of the first one): the loads of up to kEdgeGroup trips are requested together (clamped index, no branch around them), and in the
    // later passes the LDS-resident plane rows -- which wait for nothing -- are accumulated while those loads are in flight.  The rows of a
    // pass are therefore summed as {cached planes, edges, streamed planes} (first pass: {edges, planes} as before): a fixed order, a
    // function of the records alone.
    constexpr int kEdgeGroup = BLOCK >= 512 ? 1 : 4;
    bool first = true;
    for (int k0 = threadIdx.x; first || k0 < n_walk; k0 += kEdgeGroup * BLOCK) {
      double e6[kEdgeGroup][6];
      float4 ef[kEdgeGroup];
      int ei[kEdgeGroup];
#pragma unroll
      for (int u = 0; u < kEdgeGroup; u++) {
        const int k = min(k0 + u * BLOCK, max(n_walk - 1, 0));
        ei[u] = FILL ? k : (k < n_listed ? (int)el.idx[k] : kEdgeListMax + (k - n_listed));
      }
      if (n_walk > 0) {
#pragma unroll
        for (int u = 0; u < kEdgeGroup; u++) {
          const double* r6 = rec + 6 * (size_t)ei[u];
          e6[u][0] = r6[0]; e6[u][1] = r6[1]; e6[u][2] = r6[2]; e6[u][3] = r6[3]; e6[u][4] = r6[4]; e6[u][5] = r6[5];
          ef[u] = corner[ei[u]];                                   // curr_point: untransformed (:146)
        }
      }
      if (first) { cached_planes(); first = false; }
#pragma unroll
      for (int u = 0; u < kEdgeGroup; u++) {
        if (k0 + u * BLOCK >= n_walk) break;
        edge_row(ei[u], mk3(e6[u][0], e6[u][1], e6[u][2]), mk3(e6[u][3], e6[u][4], e6[u][5]), mk3((double)ef[u].x, (double)ef[u].y, (double)ef[u].z));
      }
    }
  } else {                                          // de-skew: the points are the records' f64 p' (no plane cache)
    for (int k = threadIdx.x; k < n_walk; k += BLOCK) {
      const bool listed = !FILL && k < n_listed;
      const int i = FILL ? k : (listed ? (int)el.idx[k] : kEdgeListMax + (k - n_listed));
      const double* r6 = rec + 6 * (size_t)i;
      const d3 C = mk3(r6[0], r6[1], r6[2]);
      const d3 N = mk3(r6[3], r6[4], r6[5]);
      const d3 p = mk3(pprime[3 * (size_t)i], pprime[3 * (size_t)i + 1], pprime[3 * (size_t)i + 2]);
      edge_row(i, C, N, p);
    }
  }
  LM_T(t_edges_done);
  // (b) the streamed rest (everything in the FILL pass): ~1 GB per launch with all 1 024 solves resident (PMC r02).  A thread's
  // trips are a chain of dependent load round trips at two wavefronts per SIMD, so the loads of kGroup trips are requested
  // together (clamped index, no branch around them) and the rows then accumulated in ascending i as before: the sums are those
  // of the plain loop bit for bit.  Measured on the bench batch: 0.227 ms per launch ungrouped, 0.221 / 0.202 / 0.190 / 0.186 with
  // 2 / 4 / 6 / 8 trips per group (248 VGPRs, no spills).  Measured and rejected earlier: software pipelining the loads 1 / 2 / 3
  // trips ahead across the loop's back edge (0.249 / 0.258 / 0.264 ms); solving the batch in 2 / 4 launches of fewer scans
  // (0.41 / 0.71 ms: a launch takes ~0.2 ms however few problems it holds).
  constexpr int kGroup = lm_load_group(BLOCK);
  if (kGroup > 1 && use_cache) {
    for (; i < ns; i += kGroup * BLOCK) {
      double gn[kGroup][4];
      float4 gf[kGroup];
#pragma unroll
      for (int u = 0; u < kGroup; u++) {
        const int iu = min(i + u * BLOCK, ns - 1);
        plane_rec_load(recp, g0 + (size_t)iu, gn[u]);
        gf[u] = surf[iu];
      }
#pragma unroll
      for (int u = 0; u < kGroup; u++) {
        const int iu = i + u * BLOCK;
        if (iu >= ns) break;
        if (FILL && iu < PlaneCache<BLOCK>::kPlanes) {
          pc.nx[iu] = gn[u][0]; pc.ny[iu] = gn[u][1]; pc.nz[iu] = gn[u][2]; pc.d0[iu] = gn[u][3];
          pc.px[iu] = gf[u].x; pc.py[iu] = gf[u].y; pc.pz[iu] = gf[u].z;
        }
        plane_row(mk3(gn[u][0], gn[u][1], gn[u][2]), gn[u][3], mk3((double)gf[u].x, (double)gf[u].y, (double)gf[u].z));
      }
    }
  }
  for (; i < ns; i += BLOCK) {
    double r4[4];
    plane_rec_load(recp, g0 + (size_t)i, r4);
    const d3 N = mk3(r4[0], r4[1], r4[2]); const double d0 = r4[3];
    d3 p;
    if (pprime) { const size_t q = (size_t)(nc + i); p = mk3(pprime[3 * q], pprime[3 * q + 1], pprime[3 * q + 2]); }
    else {
      const float4 f = surf[i];                                  // curr_point: untransformed (:221)
      p = mk3((double)f.x, (double)f.y, (double)f.z);
      if (FILL && i < PlaneCache<BLOCK>::kPlanes) {
        pc.nx[i] = N.x; pc.ny[i] = N.y; pc.nz[i] = N.z; pc.d0[i] = d0;
        pc.px[i] = f.x; pc.py[i] = f.y; pc.pz[i] = f.z;
      }
    }
    plane_row(N, d0, p);
  }
  LM_T(t_planes_done);
}

// Trust-region state of one solve.  Lives in LDS so that the evaluation passes (which every lane
// runs) keep a small register footprint; only lane 0 of the workgroup touches it.
struct TrState {
  double sys[kAcc];          // {cost, g, H upper} at the current iterate x
  double scale[6], diagonal[6];
  double x[7], cand[7];
  double cost, gmax, x_norm, radius, decrease_factor, model_cost_change;
  int iteration, invalid, successful, reuse_diagonal, step_ok;
};

template <int BLOCK>
struct LmShared {
  double part[BLOCK / 64][kAcc + 2];   // per wavefront: {cost, g, H} and the two correspondence counts (as doubles: exact)
  double red[kAcc];          // reduced {cost, g, H} of the last pass
  int    cnt[2];
  TrState tr;
  int    go;                 // 1: evaluate candidate, 0: finished
};

// deterministic block reduction, fixed order inside the wave and across waves.  Inside the wave the 30 values are not
// reduced one butterfly each (30 x 6 exchanges): every exchange step halves the number of values a lane carries — at
// offset 32 the lower half-wave keeps values 0..14 and receives the upper half's share of them while the upper half keeps
// 15..29, and so on down to one value per lane pair: 15 + 8 + 4 + 2 + 1 + 1 = 31 exchanges.  The lane whose bits say
// (b5 b4 b3 b2 b1) ends up with value 15 b5 + 8 b4 + 4 b3 + 2 b2 + b1 (slot 15 of each half is padding).
template <int BLOCK>
__device__ __forceinline__ void block_reduce(LmShared<BLOCK>& sh, double (&acc)[kAcc], int n_edge, int n_plane) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double v16[16], v8[8], v4[4], v2[2], x;
  {
    const bool up = lane & 32;
#pragma unroll
    for (int k = 0; k < 15; k++) {
      const double a = acc[k < kAcc ? k : 0];
      const double b = k + 15 < kAcc ? acc[k + 15 < kAcc ? k + 15 : 0] : (k + 15 == kAcc ? (double)n_edge : (double)n_plane);
      v16[k] = (up ? b : a) + __shfl_xor(up ? a : b, 32);
    }
    v16[15] = 0.0;
  }
  {
    const bool up = lane & 16;
#pragma unroll
    for (int k = 0; k < 8; k++) v8[k] = (up ? v16[k + 8] : v16[k]) + __shfl_xor(up ? v16[k] : v16[k + 8], 16);
  }
  {
    const bool up = lane & 8;
#pragma unroll
    for (int k = 0; k < 4; k++) v4[k] = (up ? v8[k + 4] : v8[k]) + __shfl_xor(up ? v8[k] : v8[k + 4], 8);
  }
  {
    const bool up = lane & 4;
#pragma unroll
    for (int k = 0; k < 2; k++) v2[k] = (up ? v4[k + 2] : v4[k]) + __shfl_xor(up ? v4[k] : v4[k + 2], 4);
  }
  {
    const bool up = lane & 2;
    x = (up ? v2[1] : v2[0]) + __shfl_xor(up ? v2[0] : v2[1], 2);
  }
  x += __shfl_xor(x, 1);
  const int slot = (lane >> 1) & 15;
  if (!(lane & 1) && slot != 15) sh.part[wave][15 * (lane >> 5) + slot] = x;
  __syncthreads();
  if (threadIdx.x < kAcc + 2) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) s += sh.part[w][threadIdx.x];
    if (threadIdx.x < kAcc) sh.red[threadIdx.x] = s;
    else sh.cnt[threadIdx.x - kAcc] = (int)s;
  }
  // no barrier here: the sums are written and then read (trust-region logic, lane 0) inside wavefront 0, in program
  // order; every other reader comes after the barrier that ends the serial section
}

// 6x6 SPD solve by Cholesky, fully unrolled; A symmetric (full storage), returns false if not PD
__device__ __forceinline__ bool chol_solve6(const double (&A)[6][6], const double (&b)[6], double (&x)[6]) {
  double L[6][6];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(s > 0.0)) ok = false;
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) if (!isfinite(x[i])) ok = false;
  return ok;
}

// The only use of the gradient max-norm is the test `gmax <= gradient_tolerance`.  Its translation components are
// |x_i - fl(x_i - g_i)| >= |g_i| - |x_i - g_i| 2^-53 (1 + 2^-53): for |x_i| < 1e6 that can only be <= gtol when
// |g_i| <= gtol + 2.3e-10, so a translation gradient component above 2 gtol + 1e-9 decides the test without the
// manifold step (sincos, quaternion product, normalisation) that the exact value needs.  Returns a value > gtol then.
__device__ __forceinline__ double gradient_max_norm(const pose7& x, const double* g);
__device__ __forceinline__ double gradient_max_norm_for_test(const pose7& x, const double* g, double gtol) {
  const double gt = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
  const double xt = fmax(fabs(x.t.x), fmax(fabs(x.t.y), fabs(x.t.z)));
  if (gt > 2.0 * gtol + 1e-9 && xt < 1e6) return gt;
  return gradient_max_norm(x, g);
}
__device__ __forceinline__ double gradient_max_norm(const pose7& x, const double* g) {
  const pose7 xp = pose_plus(x, mk3(-g[0], -g[1], -g[2]), mk3(-g[3], -g[4], -g[5]));
  double m = fabs(x.t.x - xp.t.x);
  m = fmax(m, fabs(x.t.y - xp.t.y)); m = fmax(m, fabs(x.t.z - xp.t.z));
  m = fmax(m, fabs(x.q.x - xp.q.x)); m = fmax(m, fabs(x.q.y - xp.q.y));
  m = fmax(m, fabs(x.q.z - xp.q.z)); m = fmax(m, fabs(x.q.w - xp.q.w));
  return m;
}
__device__ __forceinline__ double pose_norm(const pose7& x) {
  return sqrt(x.t.x * x.t.x + x.t.y * x.t.y + x.t.z * x.t.z + x.q.x * x.q.x + x.q.y * x.q.y + x.q.z * x.q.z + x.q.w * x.q.w);
}

// unpack the packed accumulator into full H (6x6), g
__device__ __forceinline__ void unpack_system(const double* sys, double (&H)[6][6], double (&g)[6]) {
#pragma unroll
  for (int k = 0; k < 6; k++) g[k] = sys[1 + k];
  int n = 7;
#pragma unroll
  for (int p = 0; p < 6; p++)
#pragma unroll
    for (int q = p; q < 6; q++) { H[p][q] = sys[n]; H[q][p] = sys[n]; n++; }
}

// FinalizeIterationAndCheckIfMinimizerCanContinue + ComputeTrustRegionStep (+ HandleInvalidStep,
// ParameterToleranceReached), lane 0 only.  Returns 1 when tr.cand holds a candidate to evaluate.
// `prm` BY VALUE: through a reference the (kernel-argument) structure is read with flat loads, and because the stores to
// the LDS state in between might alias it, every use re-read its field from memory behind an `s_waitcnt vmcnt(0)` — a
// dozen global round trips per call on a single lane (found with clock reads inside the function: the six clamps of the
// LM diagonal alone took 7 us).
__device__ __noinline__ int tr_propose(TrState& tr, const SolverParams prm) {
#define MSFL_TR_DEGEN 0
#include "msfl_tr_propose_body.inc"
#undef MSFL_TR_DEGEN
}
// The same text once more, inlined into the one kernel whose launch is a third of the batch step: lm_solve_kernel<128> (see
// lm_tr_propose below).  The call form stays for every other solve kernel.
__device__ __forceinline__ int tr_propose_inline(TrState& tr, const SolverParams prm) {
#define MSFL_TR_DEGEN 0
#include "msfl_tr_propose_body.inc"
#undef MSFL_TR_DEGEN
}

// FunctionToleranceReached / IsStepSuccessful / HandleSuccessfulStep / HandleUnsuccessfulStep,
// lane 0 only; `red` = {cost, g, H} evaluated at tr.cand.  Returns 1 to continue.
__device__ __noinline__ int tr_decide(TrState& tr, const double* red, const SolverParams prm) {
#include "msfl_tr_decide_body.inc"
}
__device__ __forceinline__ int tr_decide_inline(TrState& tr, const double* red, const SolverParams prm) {
#include "msfl_tr_decide_body.inc"
}

// MEASURED (profiles/r07_lm_pipeline.md): as calls, the two functions cost lm_solve_kernel<128> 7 % of its launch.  A call makes the
// compiler wait for every outstanding load in front of it, saves and restores the caller's registers through scratch (376 B per
// lane, all of the kernel's private segment) and keeps whatever is live across it in the callee-saved half of the register file.
// Inlined, the kernel has no private segment at all, 255 VGPRs, no spill: 0.1862 -> 0.1725 ms per launch on the bench batch, the
// results bit for bit the same (tests/test_gpu_lm_pipeline.py).  -DMSFL_LM_TR_INLINE=0 builds the calls everywhere, as before.
// Only the plain 128-thread kernel takes the inlined form: it is the one that was measured.  The prior and degeneracy siblings and the
// 512-thread SLAM solve keep the calls (INL = false is the text they always had).
#ifndef MSFL_LM_TR_INLINE
#define MSFL_LM_TR_INLINE 1
#endif
template <bool INL>
__device__ __forceinline__ int lm_tr_propose(TrState& tr, const SolverParams prm) {
  if constexpr (INL) return tr_propose_inline(tr, prm);
  else return tr_propose(tr, prm);
}
template <bool INL>
__device__ __forceinline__ int lm_tr_decide(TrState& tr, const double* red, const SolverParams prm) {
  if constexpr (INL) return tr_decide_inline(tr, red, prm);
  else return tr_decide(tr, red, prm);
}


// ---- optional Gaussian pose prior (msfl_set_pose_prior; docs/kernels/prior.md) ---------------------------------
// One more residual block of the solved problem, WITHOUT a loss function: r = L e, e = [t - t0 ; 2 vec(conj(q0) q)]
// (the quaternion taken with w >= 0), J = L blockdiag(I, w I + skew(v)) in the tangent of PoseLocalParameterization.
struct PosePrior { double pose[7]; double sqrt_information[36]; };   // mirrors msfl_pose_prior
// Code that only runs with a prior is tagged with a section name of its own.  The device link still produces one .text, but the
// tag changes where the functions are emitted: prior_accumulate then lands behind lm_solve_kernel<128> instead of between
// tr_decide and it, so the feature-off batch solve keeps its distance to tr_propose / tr_decide (checked with nm on the code
// object of both commits).  MEASURED (docs/kernels/prior.md): with the sibling kernel emitted in front of lm_solve_kernel<128>,
// the instruction-identical feature-off solve ran 1.2 % slower, from its place in the code object alone.
#define MSFL_PRIOR_TEXT __attribute__((section(".text.msfl_prior")))
constexpr int kPriorWords = (int)(sizeof(PosePrior) / sizeof(double));
static_assert(kPriorWords == 43, "msfl_pose_prior layout");

// Adds the prior's {cost, g[6], H[21]} at pose x to the packed sums in `red`.  Lane 0 only, serial (a few hundred
// flops), called AFTER the block reduction of the lidar rows: the summation order is (lidar sum) + (prior sum), the
// prior sum row by row, whatever the block width.  Shared by lm_solve_kernel's prior form and uncertainty_kernel's.
__device__ __noinline__ MSFL_PRIOR_TEXT void prior_accumulate(const pose7 x, const PosePrior* prior, double* red) {
  const double* p0 = prior->pose;
  const double* L = prior->sqrt_information;
  quat qc; qc.x = -p0[3]; qc.y = -p0[4]; qc.z = -p0[5]; qc.w = p0[6];
  quat qe = quat_mul(qc, x.q);
  if (qe.w < 0.0) { qe.x = -qe.x; qe.y = -qe.y; qe.z = -qe.z; qe.w = -qe.w; }
  const double e[6] = {x.t.x - p0[0], x.t.y - p0[1], x.t.z - p0[2], 2.0 * qe.x, 2.0 * qe.y, 2.0 * qe.z};
  // rotation block of d e / d delta at delta = 0: w I + skew(v)
  const double M[3][3] = {{qe.w, -qe.z, qe.y}, {qe.z, qe.w, -qe.x}, {-qe.y, qe.x, qe.w}};
  double s[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; k++) s[k] = 0.0;
  for (int i = 0; i < 6; i++) {
    double l[6], j[6];
#pragma unroll
    for (int k = 0; k < 6; k++) l[k] = L[6 * i + k];
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) r += l[k] * e[k];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      j[c] = l[c];
      j[3 + c] = l[3] * M[0][c] + l[4] * M[1][c] + l[5] * M[2][c];
    }
    s[0] += r * r;
#pragma unroll
    for (int k = 0; k < 6; k++) s[1 + k] += j[k] * r;
    int n = 7;
#pragma unroll
    for (int p = 0; p < 6; p++)
#pragma unroll
      for (int q = p; q < 6; q++) s[n++] += j[p] * j[q];
  }
  red[0] += 0.5 * s[0];
#pragma unroll
  for (int k = 1; k < kAcc; k++) red[k] += s[k];
}

// Registration b's prior record -> LDS (43 lanes, plain loads).  Every thread of the workgroup calls this.
// bad: some entry is not finite; use: some sqrt_information entry is non-zero (an all-zero record is SKIPPED, not added).
template <int BLOCK>
__device__ __forceinline__ void prior_stage(const PosePrior* __restrict__ src, PosePrior& dst, int& bad, int& use) {
  static_assert(BLOCK >= 64, "43 lanes stage the record");
  int my_bad = 0, my_use = 0;
  if (threadIdx.x < kPriorWords) {
    const double v = reinterpret_cast<const double*>(src)[threadIdx.x];
    reinterpret_cast<double*>(&dst)[threadIdx.x] = v;
    my_bad = !isfinite(v);
    my_use = threadIdx.x >= 7 && v != 0.0;
  }
  bad = __syncthreads_or(my_bad);
  use = __syncthreads_or(my_use);
}

// One workgroup per scan, persistent over all trust-region iterations of one ceres::Solve.
// Lane 0 runs the (serial, tiny) trust-region logic between evaluation passes; every pass
// evaluates cost AND the normal equations at the candidate, so an accepted step needs no second
// pass (Ceres re-evaluates; the values are identical).
#ifndef MSFL_LM_WAVES
#define MSFL_LM_WAVES 2
#endif
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, MSFL_LM_WAVES)
lm_solve_kernel(BatchView bv, const double* __restrict__ pprime_all, const double* __restrict__ rec_all,
                double* __restrict__ poses, int* __restrict__ status, DevMatchInfo* __restrict__ info,
                int outer_it, SolverParams prm) {
#define MSFL_LM_PRIOR 0
#define MSFL_LM_DEGEN 0
#include "msfl_lm_solve_body.inc"
#undef MSFL_LM_DEGEN
#undef MSFL_LM_PRIOR
}

// The sibling with the pose prior: prior_all[b] is one more residual block of registration b's problem.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, MSFL_LM_WAVES) MSFL_PRIOR_TEXT
lm_solve_prior_kernel(BatchView bv, const double* __restrict__ pprime_all, const double* __restrict__ rec_all,
                      double* __restrict__ poses, int* __restrict__ status, DevMatchInfo* __restrict__ info,
                      int outer_it, SolverParams prm, const PosePrior* __restrict__ prior_all) {
#define MSFL_LM_PRIOR 1
#define MSFL_LM_DEGEN 0
#include "msfl_lm_solve_body.inc"
#undef MSFL_LM_DEGEN
#undef MSFL_LM_PRIOR
}

// The sibling with solution remapping (msfl_set_degeneracy), defined in msfl_degeneracy.cuh: it needs the Jacobi routine of
// msfl_uncertainty.cuh.  `prior_all` may be null there.
struct DegenRecord;
template <int BLOCK>
__global__ void lm_solve_degen_kernel(BatchView bv, const double* __restrict__ pprime_all, const double* __restrict__ rec_all,
                                      double* __restrict__ poses, int* __restrict__ status, DevMatchInfo* __restrict__ info,
                                      int outer_it, SolverParams prm, const PosePrior* __restrict__ prior_all, double degen_min_eig,
                                      DegenRecord* __restrict__ degen_out);

// The one launch helper of all six solve sites: `prior` null and `degen_on` 0 = both features off, the kernel that was always
// launched.  With degen_on the remapping sibling runs (with or without a prior); `degen_out` may be null.
template <int BLOCK>
inline void launch_lm_solve(hipStream_t st, int n_scans, const BatchView& bv, const double* pprime, const double* records, double* poses,
                            int* status, DevMatchInfo* info, int outer_it, const SolverParams& sp, const PosePrior* prior,
                            int degen_on = 0, double degen_min_eig = 0.0, DegenRecord* degen_out = nullptr) {
  if (!degen_on && !prior)          // the plain kernel is named first: the kernels are emitted in this order (docs/kernels/prior.md)
    hipLaunchKernelGGL(lm_solve_kernel<BLOCK>, dim3(n_scans), dim3(BLOCK), 0, st, bv, pprime, records, poses, status, info, outer_it, sp);
  else if (!degen_on)
    hipLaunchKernelGGL(lm_solve_prior_kernel<BLOCK>, dim3(n_scans), dim3(BLOCK), 0, st, bv, pprime, records, poses, status, info, outer_it, sp, prior);
  else
    hipLaunchKernelGGL(lm_solve_degen_kernel<BLOCK>, dim3(n_scans), dim3(BLOCK), 0, st, bv, pprime, records, poses, status, info, outer_it, sp,
                       prior, degen_min_eig, degen_out);
}

}  // namespace msfl
