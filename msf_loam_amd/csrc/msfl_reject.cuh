// msfl_reject.cuh — opt-in outlier rejection between association and solve (gfx950 / CDNA4; docs/kernels/rejection.md).
//
//   reject_threshold_kernel   one lane per local record: the loss-free squared residual at the solve's entry pose, and a record
//                             with !(s <= thr2) becomes what association writes for a refused correspondence (N = 0)
//   reject_fraction_kernel    one workgroup per scan: the ceil(n * fraction) valid records with the largest s go, by an exact radix
//                             select over the bit patterns of s and a tie pass in local index order
//
// The reference's hooks: RefineByRejectOutliersWithThreshold / RefineByRejectOutliersWithFrac (scan_matcher.cc:13-76).
// Neither kernel shares code with evaluate_pass: the residual is restated here, so the solve kernels do not move.  Counts are
// integers and records are written with plain stores: a result does not depend on the launch shape or on how a call is batched.
#pragma once
#include <algorithm>

#include "msfl_kernels.cuh"

namespace msfl {

struct RejectRecord {   // mirrors msfl_rejection_record; index = outer iteration
  int n_edge_in[2], n_plane_in[2];
  int n_edge_rejected[2], n_plane_rejected[2];
  double cut_sq[2];
  int valid[2];
};

constexpr int kRejectBlock = 256;
constexpr int kRejectMaxRows = 65535;                          // gridDim.y of one threshold launch: more scans take several (row0)
constexpr unsigned long long kRejectNanKey = 0x7ff8000000000000ull;   // every non-finite s: above the pattern of every finite one

#define MSFL_REJECT_TEXT __attribute__((section(".text.msfl_reject")))

// What both kernels know about one scan of the batch.
struct RejectScan {
  int nc, ns;                 // corner / surf features
  const float4* corner; const float4* surf;
  double* rec;                // its edge records {C, N}
  double* recp; size_t g0;    // the record buffer and the scan's first plane slot in it: plane records {N, d0} (plane_rec_load)
  const double* pprime;       // de-skew: its f64 points p' (corner features first), else null
};

__device__ __forceinline__ RejectScan reject_scan(const BatchView& bv, const double* __restrict__ pprime_all, double* __restrict__ rec_all, int b) {
  RejectScan s;
  s.nc = bv.corner_off[b + 1] - bv.corner_off[b];
  s.ns = bv.surf_off[b + 1] - bv.surf_off[b];
  s.corner = bv.corner + bv.corner_off[b];
  s.surf = bv.surf + bv.surf_off[b];
  s.rec = rec_all + edge_rec_off(bv, bv.corner_off[b]);
  s.recp = rec_all; s.g0 = plane_slot(bv, bv.surf_off[b]);
  s.pprime = pprime_all ? pprime_all + 3 * (size_t)bv.rec_off[b] : nullptr;
  return s;
}

// Local record `i` of the scan (corner features first): is it a correspondence (N != 0), and its squared residual without the loss.
//   edge  s = |N x (R p + t - C)|^2          plane  s = (N.(R p + t) - d0)^2
__device__ __forceinline__ bool reject_residual(const RejectScan& sc, const mat3& R, const d3& t, int i, double& s) {
  const bool edge = i < sc.nc;
  const int k = edge ? i : i - sc.nc;
  d3 p;
  if (sc.pprime) p = mk3(sc.pprime[3 * (size_t)i], sc.pprime[3 * (size_t)i + 1], sc.pprime[3 * (size_t)i + 2]);
  else { const float4 f = edge ? sc.corner[k] : sc.surf[k]; p = mk3((double)f.x, (double)f.y, (double)f.z); }
  const d3 q = mk3(__builtin_fma(R.m[0], p.x, __builtin_fma(R.m[1], p.y, R.m[2] * p.z)) + t.x,
                   __builtin_fma(R.m[3], p.x, __builtin_fma(R.m[4], p.y, R.m[5] * p.z)) + t.y,
                   __builtin_fma(R.m[6], p.x, __builtin_fma(R.m[7], p.y, R.m[8] * p.z)) + t.z);
  if (edge) {
    const double* r6 = sc.rec + 6 * (size_t)k;
    const d3 N = mk3(r6[3], r6[4], r6[5]);
    if (N.x == 0.0 && N.y == 0.0 && N.z == 0.0) return false;
    const d3 d = mk3(q.x - r6[0], q.y - r6[1], q.z - r6[2]);
    const d3 r = cross(N, d);
    s = __builtin_fma(r.x, r.x, __builtin_fma(r.y, r.y, r.z * r.z));
  } else {
    double r4[4];
    plane_rec_load(sc.recp, sc.g0 + (size_t)k, r4);
    const d3 N = mk3(r4[0], r4[1], r4[2]);
    if (N.x == 0.0 && N.y == 0.0 && N.z == 0.0) return false;
    const double r = __builtin_fma(N.x, q.x, __builtin_fma(N.y, q.y, N.z * q.z)) - r4[3];
    s = r * r;
  }
  return true;
}

// A rejected record becomes a refused correspondence: N = 0 (and d0 = 0 for a plane).  Plain vector stores.
__device__ __forceinline__ void reject_zero(const RejectScan& sc, int i) {
  if (i < sc.nc) { double* r6 = sc.rec + 6 * (size_t)i; r6[3] = 0.0; r6[4] = 0.0; r6[5] = 0.0; }
  else plane_rec_store(sc.recp, sc.g0 + (size_t)(i - sc.nc), 0.0, 0.0, 0.0, 0.0);
}

// grid: x = chunks of kRejectBlock records over the call's longest scan, y = scan row0 + blockIdx.y.  `out` (may be null) was zeroed
// before the first solve of the registration: the counts are added to it, one atomic per wavefront and kind.
__global__ void __launch_bounds__(kRejectBlock) MSFL_REJECT_TEXT
reject_threshold_kernel(BatchView bv, const double* __restrict__ pprime_all, double* __restrict__ rec_all, const double* __restrict__ poses,
                        const int* __restrict__ status, RejectRecord* __restrict__ out, int outer_it, double thr2, int row0) {
  const int b = row0 + (int)blockIdx.y;
  if (status[b] != 0) return;                            // the solve skips this scan too: its slice stays zero
  const RejectScan sc = reject_scan(bv, pprime_all, rec_all, b);
  const int n = sc.nc + sc.ns;
  const int chunk0 = (int)blockIdx.x * kRejectBlock;
  if (chunk0 >= n && chunk0 > 0) return;                 // the grid is as wide as the call's longest scan
  const int i = chunk0 + (int)threadIdx.x;
  const pose7 T = load_pose(poses + 7 * (size_t)b);
  const mat3 R = quat_to_matrix(T.q);
  double s = 0.0;
  const bool live = i < n && reject_residual(sc, R, T.t, i, s);
  const bool gone = live && !(s <= thr2);                // a non-finite s goes
  if (gone) reject_zero(sc, i);
  if (!out) return;
  const bool edge = i < sc.nc;
  const int in_e = __popcll(__ballot(live && edge)), in_p = __popcll(__ballot(live && !edge));
  const int go_e = __popcll(__ballot(gone && edge)), go_p = __popcll(__ballot(gone && !edge));
  if ((threadIdx.x & 63) == 0) {
    RejectRecord* r = out + b;
    if (in_e) atomicAdd(&r->n_edge_in[outer_it], in_e);
    if (in_p) atomicAdd(&r->n_plane_in[outer_it], in_p);
    if (go_e) atomicAdd(&r->n_edge_rejected[outer_it], go_e);
    if (go_p) atomicAdd(&r->n_plane_rejected[outer_it], go_p);
    if (go_e + go_p) r->cut_sq[outer_it] = thr2;         // (every wavefront that rejected stores the same value)
    if (i == 0) r->valid[outer_it] = 1;
  }
}

// One workgroup per scan.  keys: scratch of one u64 per record of the batch (indexed like rec_off); a record's key is 1 + the bit
// pattern of its s (one canonical pattern for every non-finite s), 0 for a record that is no correspondence -- so keys order like
// (s, non-finite on top) and a record that is none sorts below every one that is.
__global__ void __launch_bounds__(kRejectBlock) MSFL_REJECT_TEXT
reject_fraction_kernel(BatchView bv, const double* __restrict__ pprime_all, double* __restrict__ rec_all, const double* __restrict__ poses,
                       const int* __restrict__ status, RejectRecord* __restrict__ out, int outer_it, double fraction,
                       unsigned long long* __restrict__ keys_all) {
  __shared__ int s_hist[256];
  __shared__ int s_cnt[4];                               // valid edges, valid planes, rejected edges, rejected planes
  __shared__ int s_wave[kRejectBlock / 64];
  __shared__ int s_bin, s_left;
  const int b = (int)blockIdx.x;
  if (status[b] != 0) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RejectScan sc = reject_scan(bv, pprime_all, rec_all, b);
  const int r0 = bv.rec_off[b];
  const int n = max(0, min(sc.nc + sc.ns, bv.n_records - r0));   // (the scratch holds bv.n_records keys)
  unsigned long long* keys = keys_all + r0;
  if (tid < 4) s_cnt[tid] = 0;
  __syncthreads();
  {
    const pose7 T = load_pose(poses + 7 * (size_t)b);
    const mat3 R = quat_to_matrix(T.q);
    for (int c = 0; c < n; c += kRejectBlock) {
      const int i = c + tid;
      double s = 0.0;
      const bool live = i < n && reject_residual(sc, R, T.t, i, s);
      if (i < n) keys[i] = live ? 1ull + (isfinite(s) ? (unsigned long long)__double_as_longlong(s) : kRejectNanKey) : 0ull;
      const bool edge = i < sc.nc;
      const int in_e = __popcll(__ballot(live && edge)), in_p = __popcll(__ballot(live && !edge));
      if (lane == 0) { if (in_e) atomicAdd(&s_cnt[0], in_e); if (in_p) atomicAdd(&s_cnt[1], in_p); }
    }
  }
  __syncthreads();                                       // (a thread only ever re-reads the keys it wrote itself)
  const int n_valid = s_cnt[0] + s_cnt[1];
  // the reference's `for (i = 0; i < n * frac; i++)`: ceil of the double product
  const int k = min(n_valid, (int)ceil((double)n_valid * fraction));
  unsigned long long cut = 0;
  int n_ties = 0, ties_gone = 0;
  if (k > 0) {
    // exact radix select of the k-th largest key: 8 bits per pass from the top
    int left = k;                                        // still to be found among the keys that share `cut`'s decided bits
    for (int pass = 0; pass < 8; pass++) {
      const int shift = 56 - 8 * pass;
      s_hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += kRejectBlock) {
        const unsigned long long key = keys[i];
        if (pass == 0 || (key >> (shift + 8)) == (cut >> (shift + 8))) atomicAdd(&s_hist[(int)(key >> shift) & 255], 1);
      }
      __syncthreads();
      if (wave == 0) {                                   // lane l holds bins 255 - 4 l .. 252 - 4 l, descending
        int h[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) { h[u] = s_hist[255 - 4 * lane - u]; sum += h[u]; }
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
        int above = incl - sum;                          // keys in higher bins
        if (above < left && left <= incl) {              // exactly one lane
#pragma unroll
          for (int u = 0; u < 4; u++) {
            if (above < left && left <= above + h[u]) { s_bin = 255 - 4 * lane - u; s_left = left - above; s_wave[0] = h[u]; above = left; }
            else above += h[u];
          }
        }
      }
      __syncthreads();
      cut |= (unsigned long long)s_bin << shift;
      left = s_left;
      n_ties = s_wave[0];
      __syncthreads();
    }
    ties_gone = left;                                    // of the n_ties keys equal to the cut, the last `left` in index order go
    // tie + apply pass: ascending local index, a running ballot prefix ranks the keys equal to the cut
    int seen = 0;
    for (int c = 0; c < n; c += kRejectBlock) {
      const int i = c + tid;
      const unsigned long long key = i < n ? keys[i] : 0ull;
      const bool tie = key == cut;
      const unsigned long long m = __ballot(tie);
      if (lane == 0) s_wave[wave] = __popcll(m);
      __syncthreads();
      int rank = seen + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
      for (int w = 0; w < kRejectBlock / 64; w++) { if (w < wave) rank += s_wave[w]; total += s_wave[w]; }
      seen += total;
      const bool gone = key > cut || (tie && rank >= n_ties - ties_gone);
      if (gone) reject_zero(sc, i);
      const bool edge = i < sc.nc;
      const int go_e = __popcll(__ballot(gone && edge)), go_p = __popcll(__ballot(gone && !edge));
      if (lane == 0) { if (go_e) atomicAdd(&s_cnt[2], go_e); if (go_p) atomicAdd(&s_cnt[3], go_p); }
      __syncthreads();
    }
  }
  if (out && tid == 0) {
    RejectRecord* r = out + b;
    r->n_edge_in[outer_it] = s_cnt[0]; r->n_plane_in[outer_it] = s_cnt[1];
    r->n_edge_rejected[outer_it] = s_cnt[2]; r->n_plane_rejected[outer_it] = s_cnt[3];
    // the smallest rejected s is the cut's (ties_gone >= 1 whenever k >= 1)
    r->cut_sq[outer_it] = k > 0 ? __longlong_as_double((long long)(cut - 1ull)) : 0.0;
    r->valid[outer_it] = 1;
  }
}

// The launch of one solve's rejection.  mode 1: threshold, 2: fraction.  longest: records of the call's longest scan (a bound will do).
inline void launch_reject(hipStream_t st, int mode, int n_scans, int longest, const BatchView& bv, const double* pprime, double* records,
                          const double* poses, const int* status, RejectRecord* out, int outer_it, double thr2, double fraction,
                          unsigned long long* keys) {
  if (n_scans <= 0) return;
  if (mode == 1) {
    const int chunks = std::max(1, (longest + kRejectBlock - 1) / kRejectBlock);
    for (int row0 = 0; row0 < n_scans; row0 += kRejectMaxRows)
      hipLaunchKernelGGL(reject_threshold_kernel, dim3(chunks, std::min(kRejectMaxRows, n_scans - row0)), dim3(kRejectBlock), 0, st, bv, pprime,
                         records, poses, status, out, outer_it, thr2, row0);
  } else {
    hipLaunchKernelGGL(reject_fraction_kernel, dim3(n_scans), dim3(kRejectBlock), 0, st, bv, pprime, records, poses, status, out, outer_it,
                       fraction, keys);
  }
}

}  // namespace msfl
