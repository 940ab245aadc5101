// msfl_place.cuh — place recognition: polar max-height scan descriptors and their all-pairs, all-rotations comparison
// (gfx950 / CDNA4; docs/kernels/place.md).
//
//   place_describe_kernel    grid (chunk, scan): a workgroup bins at most kPlaceChunk points of one scan into LDS (atomicMax on the
//                            bit pattern of a positive float) and writes its n_ring x n_sector partial
//   place_finish_kernel      one workgroup per scan: maximum over the scan's partials, ring key, f64 column norms
//   place_check_kernel       msfl_places_add_descriptors: flags a value that is negative or not finite
//   place_prefilter_kernel   one workgroup per query: ring-key distance to every candidate, exact radix select of the n smallest
//                            (d2, index) keys
//   place_match_kernel       one workgroup per (query, candidate): the column-cosine distance at every shift, minimum over shifts
//   place_topk_kernel        one workgroup per query: the k smallest (distance, index) records, in order
//
// Everything on the per-point path is f32 compares, multiplies and adds against host-built tables (no atan2, square root or
// division), and every sum runs in one stated order, so a result does not depend on the launch shape or on how a call is batched.
#pragma once
#include <hip/hip_runtime.h>

namespace msfl {

constexpr int kPlaceMaxRing = 32;
constexpr int kPlaceMaxSector = 120;
constexpr int kPlaceChunk = 8192;          // points of one scan per describe workgroup
constexpr int kPlaceBlock = 256;
constexpr int kPlaceFinishBlock = 128;     // >= kPlaceMaxSector and >= kPlaceMaxRing
constexpr int kPlaceShiftTile = 32;        // shifts whose column terms sit in LDS at once (match kernel)
constexpr int kPlaceMaxK = 64;

struct PlaceRec {   // mirrors msfl_place_match
  int index, shift, ring_key_d2, n_columns;
  double distance;
};

// The configuration as the kernels see it.  tab: e2[nr + 1], lo2, bc[ns / 2], bs[ns / 2] (f32, built by the host in double).
struct PlaceCfg {
  int nr, ns;
  float hoff;
  const float* tab;
};

__host__ __device__ inline int place_tab_size(int nr, int ns) { return nr + 2 + ns; }

// Distances order like their keys: the usual sign fold, so that a sum that rounding left a few 2^-52 below zero still sorts first.
__device__ __forceinline__ unsigned long long place_dist_key(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ unsigned long long place_shfl_down64(unsigned long long v, int o) {
  const int lo = __shfl_down((int)(unsigned)(v & 0xffffffffull), o), hi = __shfl_down((int)(unsigned)(v >> 32), o);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

// grid: x = chunk of the scan, y = scan row0 + blockIdx.y.  off: n_scans + 1 point offsets, then n_scans + 1 chunk offsets.  A scan of
// one chunk writes its entry (entry_desc + scan * nr * ns); a longer one writes partial[chunk_off[scan] + chunk].
__global__ void __launch_bounds__(kPlaceBlock)
place_describe_kernel(PlaceCfg c, const float4* __restrict__ pts, const int* __restrict__ off, int n_scans, int row0,
                      float* __restrict__ entry_desc, unsigned* __restrict__ partial) {
  extern __shared__ unsigned s_place[];
  const int b = row0 + (int)blockIdx.y;
  const int p0 = off[b], n = off[b + 1] - p0;
  const int* chunk_off = off + (n_scans + 1);
  const int chunks = chunk_off[b + 1] - chunk_off[b];
  if ((int)blockIdx.x >= chunks) return;
  const int ds = c.nr * c.ns, half = c.ns >> 1, nt = place_tab_size(c.nr, c.ns);
  unsigned* s_bin = s_place;
  float* s_tab = reinterpret_cast<float*>(s_place + ds);
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < ds; i += kPlaceBlock) s_bin[i] = 0u;
  for (int i = tid; i < nt; i += kPlaceBlock) s_tab[i] = c.tab[i];
  __syncthreads();
  const float* e2 = s_tab;
  const float lo2 = s_tab[c.nr + 1];
  const float* bc = s_tab + c.nr + 2;
  const float* bs = bc + half;
  const float hi2 = e2[c.nr];
  const int i0 = (int)blockIdx.x * kPlaceChunk, i1 = min(n, i0 + kPlaceChunk);
  for (int i = i0 + tid; i < i1; i += kPlaceBlock) {
    const float4 p = pts[(size_t)p0 + i];
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
    const float r2 = p.x * p.x + p.y * p.y;
    if (!(lo2 <= r2 && r2 < hi2)) continue;
    const float v = p.z + c.hoff;
    if (!(v > 0.f)) continue;
    int ring = 0;
    for (int k = 1; k < c.nr; k++) ring += r2 >= e2[k] ? 1 : 0;
    const bool upper = p.y > 0.f || (p.y == 0.f && p.x > 0.f);
    const float xp = upper ? p.x : -p.x, yp = upper ? p.y : -p.y;
    int sector = upper ? 0 : half;
    for (int k = 1; k < half; k++) sector += (bc[k] * yp - bs[k] * xp) >= 0.f ? 1 : 0;
    atomicMax(&s_bin[ring * c.ns + sector], __float_as_uint(v));      // v > 0: the unsigned order is the float order
  }
  __syncthreads();
  unsigned* dst = chunks == 1 ? reinterpret_cast<unsigned*>(entry_desc) + (size_t)b * ds : partial + ((size_t)chunk_off[b] + blockIdx.x) * ds;
  for (int i = tid; i < ds; i += kPlaceBlock) dst[i] = s_bin[i];
}

// One workgroup per scan (blockIdx.x).  off: as above, or null when the descriptors are in place already (add_descriptors).
__global__ void __launch_bounds__(kPlaceFinishBlock)
place_finish_kernel(PlaceCfg c, const int* __restrict__ off, int n_scans, const unsigned* __restrict__ partial, float* __restrict__ desc,
                    int* __restrict__ rkey, double* __restrict__ nrm) {
  extern __shared__ unsigned s_place[];
  float* s_d = reinterpret_cast<float*>(s_place);
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int ds = c.nr * c.ns;
  float* d = desc + (size_t)b * ds;
  int chunks = 1, ch0 = 0;
  if (off) { const int* chunk_off = off + (n_scans + 1); ch0 = chunk_off[b]; chunks = chunk_off[b + 1] - ch0; }
  if (chunks == 1) {
    for (int i = tid; i < ds; i += kPlaceFinishBlock) s_d[i] = d[i];
  } else {
    for (int i = tid; i < ds; i += kPlaceFinishBlock) {
      unsigned m = 0u;
      for (int k = 0; k < chunks; k++) m = max(m, partial[((size_t)ch0 + k) * ds + i]);
      const float v = __uint_as_float(m);
      s_d[i] = v; d[i] = v;
    }
  }
  __syncthreads();
  if (tid < c.nr) {
    int cnt = 0;
    for (int s = 0; s < c.ns; s++) cnt += s_d[tid * c.ns + s] > 0.f ? 1 : 0;
    rkey[(size_t)b * c.nr + tid] = cnt;
  }
  if (tid < c.ns) {
    double acc = 0.0;
    for (int r = 0; r < c.nr; r++) { const double v = (double)s_d[r * c.ns + tid]; acc = acc + v * v; }
    nrm[(size_t)b * c.ns + tid] = sqrt(acc);
  }
}

// *bad = 1 when a value is negative or not finite (every writer stores the same word).
__global__ void __launch_bounds__(kPlaceBlock) place_check_kernel(const float* __restrict__ v, size_t n, int* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * kPlaceBlock + threadIdx.x;
  if (i < n && !(v[i] >= 0.f && isfinite(v[i]))) *bad = 1;
}

// What the three query kernels share.  Query q of the call is entry qidx[q] of the arrays q_*; its candidates are the database entries
// [0, ncand[q]); count[q] of them are compared (all of them, or the prefilter's selection).  The kernels of one launch see the
// queries [q0, q0 + gridDim) and index their scratch by q - q0.
struct PlaceQuery {
  const float* q_desc; const int* q_rkey; const double* q_nrm;
  const float* db_desc; const int* db_rkey; const double* db_nrm;
  const int* qidx; const int* ncand; const int* count;
  int q0;
  int pitch;                    // records (and listed candidates) per query in scratch
  const int* list;              // null: candidate x is entry x
};

// One workgroup per query.  keys: pitch_keys u64 per query.  Writes the count[q] selected candidates to list in index order.
__global__ void __launch_bounds__(kPlaceBlock)
place_prefilter_kernel(PlaceCfg c, PlaceQuery j, unsigned long long* __restrict__ keys_all, int pitch_keys, int* __restrict__ list_out) {
  __shared__ int s_hist[256];
  __shared__ int s_qk[kPlaceMaxRing];
  __shared__ int s_wave[kPlaceBlock / 64];
  __shared__ int s_bin, s_left;
  const int ql = (int)blockIdx.x, q = j.q0 + ql;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = j.ncand[q], k = j.count[q];
  int* list = list_out + (size_t)ql * j.pitch;
  if (k <= 0) return;
  if (k >= n) {                                            // nothing to select
    for (int i = tid; i < n; i += kPlaceBlock) list[i] = i;
    return;
  }
  unsigned long long* keys = keys_all + (size_t)ql * pitch_keys;
  if (tid < c.nr) s_qk[tid] = j.q_rkey[(size_t)j.qidx[q] * c.nr + tid];
  __syncthreads();
  for (int i = tid; i < n; i += kPlaceBlock) {
    const int* ck = j.db_rkey + (size_t)i * c.nr;
    int d2 = 0;
    for (int r = 0; r < c.nr; r++) { const int d = s_qk[r] - ck[r]; d2 += d * d; }
    keys[i] = ((unsigned long long)(unsigned)d2 << 32) | (unsigned)i;
  }
  __syncthreads();                                         // (a thread only ever re-reads the keys it wrote itself)
  // exact radix select of the k-th smallest key, 8 bits per pass from the top (the pattern of reject_fraction_kernel); keys are unique
  unsigned long long cut = 0;
  int left = k;
  for (int pass = 0; pass < 8; pass++) {
    const int shift = 56 - 8 * pass;
    s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kPlaceBlock) {
      const unsigned long long key = keys[i];
      if (pass == 0 || (key >> (shift + 8)) == (cut >> (shift + 8))) atomicAdd(&s_hist[(int)(key >> shift) & 255], 1);
    }
    __syncthreads();
    if (wave == 0) {                                       // lane l holds bins 4 l .. 4 l + 3, ascending
      int h[4], sum = 0;
#pragma unroll
      for (int u = 0; u < 4; u++) { h[u] = s_hist[4 * lane + u]; sum += h[u]; }
      int incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
      int below = incl - sum;                              // keys in lower bins
      if (below < left && left <= incl) {                  // exactly one lane
#pragma unroll
        for (int u = 0; u < 4; u++) {
          if (below < left && left <= below + h[u]) { s_bin = 4 * lane + u; s_left = left - below; below = left; }
          else below += h[u];
        }
      }
    }
    __syncthreads();
    cut |= (unsigned long long)s_bin << shift;
    left = s_left;
    __syncthreads();
  }
  // keys <= cut are the k smallest; they leave in index order (a running ballot prefix)
  int seen = 0;
  for (int c0 = 0; c0 < n; c0 += kPlaceBlock) {
    const int i = c0 + tid;
    const bool in = i < n && keys[i] <= cut;
    const unsigned long long m = __ballot(in);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int rank = seen + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < kPlaceBlock / 64; w++) { if (w < wave) rank += s_wave[w]; total += s_wave[w]; }
    seen += total;
    if (in && rank < k) list[rank] = i;
    __syncthreads();
  }
}

// grid: x = candidate slot, y = query q0 + blockIdx.y.  LDS: both descriptors (f32), both norm vectors (f64), kPlaceShiftTile x ns terms.
__global__ void __launch_bounds__(kPlaceBlock)
place_match_kernel(PlaceCfg c, PlaceQuery j, PlaceRec* __restrict__ rec_out) {
  extern __shared__ double s_place_d[];
  __shared__ int s_d2[2];
  const int ql = (int)blockIdx.y, q = j.q0 + ql, x = (int)blockIdx.x;
  if (x >= j.count[q]) return;
  const int tid = (int)threadIdx.x;
  const int nr = c.nr, ns = c.ns, ds = nr * ns;
  const int cand = j.list ? j.list[(size_t)ql * j.pitch + x] : x;
  const int qe = j.qidx[q];
  double* s_qn = s_place_d;                 // ns
  double* s_cn = s_qn + ns;                 // ns
  double* s_term = s_cn + ns;               // kPlaceShiftTile * ns
  float* s_q = reinterpret_cast<float*>(s_term + kPlaceShiftTile * ns);   // nr * ns
  float* s_c = s_q + ds;                    // nr * ns
  {
    const float* gq = j.q_desc + (size_t)qe * ds;
    const float* gc = j.db_desc + (size_t)cand * ds;
    for (int i = tid; i < ds; i += kPlaceBlock) { s_q[i] = gq[i]; s_c[i] = gc[i]; }
    if (tid < ns) { s_qn[tid] = j.q_nrm[(size_t)qe * ns + tid]; s_cn[tid] = j.db_nrm[(size_t)cand * ns + tid]; }
    if (tid == 64) {                                       // ring-key distance of the pair (an integer: any order)
      const int* a = j.q_rkey + (size_t)qe * nr; const int* b = j.db_rkey + (size_t)cand * nr;
      int d2 = 0;
      for (int r = 0; r < nr; r++) { const int d = a[r] - b[r]; d2 += d * d; }
      s_d2[0] = d2;
    }
  }
  __syncthreads();
  // lane t < kPlaceShiftTile of wavefront 0 owns the shifts t, t + tile, ...: ascending, so a strict < keeps the lowest
  unsigned long long best_key = ~0ull;
  int best_shift = 0, best_cols = 0;
  double best_d = 0.0;
  for (int s0 = 0; s0 < ns; s0 += kPlaceShiftTile) {
    const int tile = min(kPlaceShiftTile, ns - s0);
    for (int i = tid; i < tile * ns; i += kPlaceBlock) {
      const int sl = i / ns, col = i - sl * ns;
      int cc = col + s0 + sl; if (cc >= ns) cc -= ns;
      const double nq = s_qn[col], nc = s_cn[cc];
      double term = 0.0;
      if (nq > 0.0 && nc > 0.0) {
        double dot = 0.0;
        for (int r = 0; r < nr; r++) dot = dot + (double)s_q[r * ns + col] * (double)s_c[r * ns + cc];
        term = 1.0 - dot / (nq * nc);
      }
      s_term[i] = term;
    }
    __syncthreads();
    if (tid < tile) {
      const int s = s0 + tid;
      double sum = 0.0;
      int cols = 0;
      for (int col = 0; col < ns; col++) {
        int cc = col + s; if (cc >= ns) cc -= ns;
        if (s_qn[col] > 0.0 && s_cn[cc] > 0.0) { sum = sum + s_term[tid * ns + col]; cols++; }
      }
      const double d = cols > 0 ? sum / (double)cols : __longlong_as_double(0x7ff0000000000000ll);
      const unsigned long long key = place_dist_key(d);
      if (key < best_key) { best_key = key; best_shift = s; best_cols = cols; best_d = d; }
    }
    __syncthreads();
  }
  if (tid < 64) {                                          // minimum over (distance, shift) across the lanes of wavefront 0
    if (tid >= kPlaceShiftTile) { best_key = ~0ull; best_shift = 0x7fffffff; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long ok = place_shfl_down64(best_key, o);
      const int os = __shfl_down(best_shift, o), oc = __shfl_down(best_cols, o);
      const unsigned long long od = place_shfl_down64((unsigned long long)__double_as_longlong(best_d), o);
      if (ok < best_key || (ok == best_key && os < best_shift)) {
        best_key = ok; best_shift = os; best_cols = oc; best_d = __longlong_as_double((long long)od);
      }
    }
    if (tid == 0) {
      PlaceRec r;
      r.index = cand; r.shift = best_shift; r.ring_key_d2 = s_d2[0]; r.n_columns = best_cols; r.distance = best_d;
      rec_out[(size_t)ql * j.pitch + x] = r;
    }
  }
}

// One workgroup per query: k rounds, each the smallest (distance, index) above the one before.  out: k records per query of the call.
__global__ void __launch_bounds__(kPlaceBlock)
place_topk_kernel(PlaceQuery j, const PlaceRec* __restrict__ rec_all, int k, PlaceRec* __restrict__ out_all) {
  __shared__ unsigned long long s_key[kPlaceBlock / 64];
  __shared__ int s_idx[kPlaceBlock / 64], s_pos[kPlaceBlock / 64];
  __shared__ unsigned long long s_best_key;
  __shared__ int s_best_idx, s_best_pos;
  const int ql = (int)blockIdx.x, q = j.q0 + ql;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = j.count[q];
  const PlaceRec* rec = rec_all + (size_t)ql * j.pitch;
  PlaceRec* out = out_all + (size_t)q * k;
  unsigned long long last_key = 0ull;
  int last_idx = -1;                                       // every key is above (0, -1): a finite or infinite distance has key >= 2^63 or index >= 0
  for (int round = 0; round < k; round++) {
    unsigned long long bk = ~0ull;
    int bi = 0x7fffffff, bp = -1;
    if (round < n) {
      for (int i = tid; i < n; i += kPlaceBlock) {
        const unsigned long long key = place_dist_key(rec[i].distance);
        const int idx = rec[i].index;
        const bool after = key > last_key || (key == last_key && idx > last_idx);
        if (after && (key < bk || (key == bk && idx < bi))) { bk = key; bi = idx; bp = i; }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long ok = place_shfl_down64(bk, o);
        const int oi = __shfl_down(bi, o), op = __shfl_down(bp, o);
        if (op >= 0 && (bp < 0 || ok < bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; bp = op; }
      }
      if (lane == 0) { s_key[wave] = bk; s_idx[wave] = bi; s_pos[wave] = bp; }
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < kPlaceBlock / 64; w++)
          if (s_pos[w] >= 0 && (bp < 0 || s_key[w] < bk || (s_key[w] == bk && s_idx[w] < bi))) { bk = s_key[w]; bi = s_idx[w]; bp = s_pos[w]; }
        s_best_key = bk; s_best_idx = bi; s_best_pos = bp;
      }
      __syncthreads();
      bk = s_best_key; bi = s_best_idx; bp = s_best_pos;
      __syncthreads();
    }
    if (tid == 0) {
      PlaceRec r;
      if (bp >= 0) r = rec[bp];
      else { r.index = -1; r.shift = 0; r.ring_key_d2 = 0; r.n_columns = 0; r.distance = __longlong_as_double(0x7ff0000000000000ll); }
      out[round] = r;
    }
    last_key = bk; last_idx = bi;
  }
}

}  // namespace msfl
