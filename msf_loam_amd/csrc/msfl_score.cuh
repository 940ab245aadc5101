// msfl_score.cuh — exact 1-NN fitness of pose hypotheses against the resident map index (gfx950 / CDNA4).
//
//   score_init_kernel    one record per hypothesis: all zero, status = MSFL_BAD_ARG for a pose with a non-finite entry; and the
//                        hypothesis' scan in a batch call
//   score_poses_kernel   one lane per (hypothesis, feature): transform, nearest map point of the feature's kind within the
//                        threshold, then an integer reduction into the hypothesis' record.  <false>: every scan against the
//                        resident single map; <true> (msfl_score_pairs): scan b against pair b of the resident pair index
//
// The walk is grid_walk_exact (msfl_knn_index.cuh), the one knn5_grid takes: nine (y, z) rows centre-first in the per-query
// near-side order, x ends trimmed on the per-side lower bounds.  Its state is
// ONE key (f32 distance bits, original index), initialised to (threshold, no index), and a row or end cell is skipped when
// its lower bound exceeds the key's distance.  A lower bound never exceeds the f32 distance of a point in the cell (that is
// what the slack is for), so a skipped cell holds no point at or below the current best: the result equals a brute-force
// search in the total order (distance, original index) over every map point within the threshold, as long as the threshold
// is not above the radius the index was built for (the 27-cell neighbourhood then holds all of them; the host checks it).
//
// The reduction is in integers: an inlier count and sum(rint(d2 * 2^32)) per feature kind.  Integer adds commute, so a
// record does not depend on the launch shape, on how a call is cut into launches or on the order workgroups arrive in.
#pragma once
#include "msfl_kernels.cuh"

namespace msfl {

constexpr int kScoreBlock = 256;
constexpr int kScoreMaxRows = 65535;        // gridDim.y of one launch: more hypotheses take several launches (row0)

struct ScoreRec {                           // msfl_pose_score
  int inliers[2];                           // corner, surf
  unsigned long long sum_sq_q32[2];
  int status;
  int reserved_;
};

// What a launch reads and writes.  Offsets are relative to the call's first feature / pose: corner, surf, poses and rec
// point at them.  d2_out / nn_out (single-scan calls only, may be null): n_features values per hypothesis.
struct ScoreJob {
  const float4* corner; const float4* surf;
  const int* corner_off; const int* surf_off; const int* pose_off;   // n_scans + 1 each
  int n_scans;
  int* scan_of;                             // per hypothesis its scan, written by score_init_kernel (null when n_scans == 1)
  const double* poses;
  ScoreRec* rec;
  float thr;
  float* d2_out; int* nn_out;
};

// What the PAIRS instantiation reads besides: the pair index's cell-table bases, and for d2_out / nn_out (whose rows are
// ragged there: F(b) values per hypothesis of scan b) the first output element of every scan's first hypothesis and where
// pair b's map clouds begin in the concatenated clouds the index words count in.
struct ScorePairsView {
  const int* cbase_c; const int* cbase_s;   // n_scans + 1 each (PairScratch::base_c / base_s)
  const int* map_c0; const int* map_s0;     // n_scans each
  const unsigned long long* out0;           // n_scans
};

__global__ void __launch_bounds__(256) score_init_kernel(ScoreJob j, int n, int bad_status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; k++) ok = ok && isfinite(j.poses[7 * (size_t)i + k]);
  ScoreRec r;
  r.inliers[0] = 0; r.inliers[1] = 0; r.sum_sq_q32[0] = 0; r.sum_sq_q32[1] = 0; r.status = ok ? 0 : bad_status; r.reserved_ = 0;
  j.rec[i] = r;
  if (j.scan_of) {
    // the hypothesis' scan: the first b with pose_off[b + 1] > i (scans without poses are passed over).  Searched once per
    // hypothesis here, not once per workgroup in front of the walk: ten dependent scalar loads there (docs/kernels/pairs.md)
    int b = 0;
    for (int hi = j.n_scans - 1; b < hi;) {
      const int mid = (b + hi) >> 1;
      if (j.pose_off[mid + 1] <= i) b = mid + 1; else hi = mid;
    }
    j.scan_of[i] = b;
  }
}

// key of a candidate: distances are non-negative floats, whose bit patterns order like the values
__device__ __forceinline__ unsigned long long score_key(float d2, unsigned int idx) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | idx;
}
constexpr unsigned int kScoreNoIndex = 0xffffffffu;   // above every original index (< 2^28): a point AT the threshold still wins

// Exact nearest neighbour of q within the distance of `best` on entry; best keeps (distance, original index) of the winner.
__device__ __forceinline__ void nn1_grid(const GridDesc& g, const float4* __restrict__ sorted, const int* __restrict__ cell_start,
                                         float3 q, unsigned long long& best) {
  grid_walk_exact(g, cell_start, q, [&]() __attribute__((always_inline)) { return __uint_as_float((unsigned int)(best >> 32)); },
                  [&](int s, int e) __attribute__((always_inline)) {
    for (int i = s; i < e; i++) {
      const float4 m = sorted[i];
      const unsigned long long k = score_key(l2_simple(m, q), __float_as_uint(m.w));
      best = k < best ? k : best;
    }
  });
}

// grid: x = workgroups of one hypothesis (its scan's corner features first, then its surf features; a workgroup holds one
// kind), y = hypothesis row0 + blockIdx.y of the call.  PAIRS: b is also the hypothesis' pair, as in
// knn5_scan2map_kernel<.., true>: descriptor b, the cell table from cell_base[b] on; b is uniform over the workgroup, so
// both are scalar loads, one per kind.
template <bool PAIRS>
__global__ void __launch_bounds__(kScoreBlock) score_poses_kernel(ScoreJob j, int row0,
                                                                   const GridDesc* __restrict__ gcp, const float4* __restrict__ map_c, const int* __restrict__ cs_c,
                                                                   const GridDesc* __restrict__ gsp, const float4* __restrict__ map_s, const int* __restrict__ cs_s,
                                                                   ScorePairsView pv) {
  __shared__ unsigned long long s_sum[kScoreBlock / 64];
  __shared__ int s_cnt[kScoreBlock / 64];
  const int hyp = row0 + (int)blockIdx.y;
  const int b = j.scan_of ? j.scan_of[hyp] : 0;
  const int c_begin = j.corner_off[b], n_c = j.corner_off[b + 1] - c_begin;
  const int s_begin = j.surf_off[b], n_s = j.surf_off[b + 1] - s_begin;
  const int blocks_c = (n_c + kScoreBlock - 1) / kScoreBlock, blocks_s = (n_s + kScoreBlock - 1) / kScoreBlock;
  const int bx = (int)blockIdx.x;
  if (bx >= blocks_c + blocks_s) return;                 // the grid is as wide as the call's largest scan
  const int kind = bx < blocks_c ? 0 : 1;
  const int f = (kind ? bx - blocks_c : bx) * kScoreBlock + (int)threadIdx.x;     // feature within its kind
  const bool live = f < (kind ? n_s : n_c);
  const double* pp = j.poses + 7 * (size_t)hyp;
  const pose7 T = load_pose(pp);
  bool pose_ok = true;
#pragma unroll
  for (int k = 0; k < 7; k++) pose_ok = pose_ok && isfinite(pp[k]);

  unsigned long long best = score_key(j.thr, kScoreNoIndex);
  if (live && pose_ok) {
    const float4 p = kind ? j.surf[s_begin + f] : j.corner[c_begin + f];
    if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
      const float3 q = transform_point_f32(T, p.x, p.y, p.z);
      if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {
        if (kind) { const GridDesc g = gsp[PAIRS ? b : 0]; nn1_grid(g, map_s, cs_s + (PAIRS ? pv.cbase_s[b] : 0), q, best); }
        else { const GridDesc g = gcp[PAIRS ? b : 0]; nn1_grid(g, map_c, cs_c + (PAIRS ? pv.cbase_c[b] : 0), q, best); }
      }
    }
  }
  const bool found = (unsigned int)best != kScoreNoIndex;
  const float d2 = __uint_as_float((unsigned int)(best >> 32));
  if (live && (j.d2_out || j.nn_out)) {
    // PAIRS: the row starts behind those of the scans before b and of b's earlier hypotheses; the index word counts in the
    // concatenated map clouds, the caller gets the position in pair b's own cloud
    const size_t row = PAIRS ? (size_t)pv.out0[b] + (size_t)(hyp - j.pose_off[b]) * (size_t)(n_c + n_s) : (size_t)hyp * (size_t)(n_c + n_s);
    const size_t o = row + (size_t)(kind ? n_c + f : f);
    if (j.d2_out) j.d2_out[o] = found ? d2 : INFINITY;
    if (j.nn_out) j.nn_out[o] = found ? (int)(unsigned int)best - (PAIRS ? (kind ? pv.map_s0[b] : pv.map_c0[b]) : 0) : -1;
  }
  // d2 <= 64 (host check), so d2 * 2^32 <= 2^38: the scaling is exact and rintf (nearest-even) only acts below 2^23
  unsigned long long sum = found ? (unsigned long long)rintf(d2 * 4294967296.0f) : 0ull;
  const int cnt = __popcll(__ballot(found));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_sum[wave] = sum; s_cnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0; int c = 0;
#pragma unroll
    for (int w = 0; w < kScoreBlock / 64; w++) { t += s_sum[w]; c += s_cnt[w]; }
    if (c) {
      ScoreRec* r = j.rec + hyp;
      atomicAdd(&r->inliers[kind], c);
      if (t) atomicAdd(&r->sum_sq_q32[kind], t);
    }
  }
}

}  // namespace msfl
