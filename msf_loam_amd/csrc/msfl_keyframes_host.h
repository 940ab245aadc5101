// Host-side bookkeeping of the keyframe store (msfl_api_keyframes.inc): where every keyframe's two point lists sit in the pools, the
// validation of an add / compose / insert request, the member table one gather launch reads, the totals with their overflow and
// capacity checks, and the launch shape.  Plain C++ over plain arrays, no HIP: tests/cpp/keyframes_host_check.cpp runs it under the
// host sanitizers, with made-up counts that have no memory behind them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace msfl {

constexpr int kKfChunk = 1024;        // points per workgroup of the gather kernel: four per lane of 256
constexpr int kKfMaxGridY = 65535;    // members per launch (the y extent of a grid)
constexpr int kKfCorner = 0, kKfSurf = 1;
// the msfl_status values this header hands out (msfl_api_keyframes.inc asserts that they are those)
constexpr int kKfOk = 0, kKfBadArg = 3, kKfCapacity = 7;
// KfRec::flags
constexpr int kKfCopy = 1;            // no transform: the bytes go through unchanged (add)
constexpr int kKfCheckFinite = 2;     // a source point with a non-finite x, y, z or t raises the launch's flag (add from device memory)
constexpr int kKfCheckCell = 4;       // a written point the map store would refuse raises the flag (insert)

// one member of one kind as the kernel reads it: `count` points from source position `src` on to destination position `dst`
struct KfRec { int src, count, dst, flags; };

// what the host knows of the store: per kind, where keyframe i starts in the pool and how many points it has
struct KfIndex {
  std::vector<int> start[2], count[2];
  long long top[2] = {0, 0};          // first free pool slot
  int size() const { return (int)count[0].size(); }
};

inline bool kf_finite(double v) { return v - v == 0.0; }                 // NaN and +-inf fail
inline bool kf_finite(float v) { return v - v == 0.0f; }
// first point of the list with a non-finite x, y, z or t; -1: none.  idx != null: the list is pts[idx[i]]
inline long long kf_first_non_finite(const float* pts, const int* idx, long long n) {
  for (long long i = 0; i < n; i++) {
    const float* p = pts + 4 * (idx ? (long long)idx[i] : i);
    if (!(kf_finite(p[0]) && kf_finite(p[1]) && kf_finite(p[2]) && kf_finite(p[3]))) return i;
  }
  return -1;
}
inline bool kf_leaf_ok(float leaf) { return leaf >= 0.0f && kf_finite(leaf); }   // NaN, negative and inf refused; 0 = no filter

// an add of (n_corner, n_surf) stored points: room for one more keyframe and in both pools?
inline int kf_check_add(const KfIndex& ix, int max_keyframes, const long long pool_cap[2], long long n_corner, long long n_surf, const char** why) {
  if (ix.size() >= max_keyframes) { *why = "the store holds max_keyframes keyframes"; return kKfCapacity; }
  if (ix.top[kKfCorner] + n_corner > pool_cap[kKfCorner]) { *why = "the corner pool is full (max_corner_points)"; return kKfCapacity; }
  if (ix.top[kKfSurf] + n_surf > pool_cap[kKfSurf]) { *why = "the surf pool is full (max_surf_points)"; return kKfCapacity; }
  return kKfOk;
}
inline void kf_commit_add(KfIndex* ix, int n_corner, int n_surf) {
  const int n[2] = {n_corner, n_surf};
  for (int k = 0; k < 2; k++) { ix->start[k].push_back((int)ix->top[k]); ix->count[k].push_back(n[k]); ix->top[k] += n[k]; }
}

// members [first, last) of keys / poses (absolute positions): every key a keyframe, every pose entry finite
inline int kf_check_members(int n_keyframes, const int* keys, const double* poses, long long first, long long last, const char** why) {
  for (long long m = first; m < last; m++) {
    if (keys[m] < 0 || keys[m] >= n_keyframes) { *why = "a key that is no keyframe"; return kKfBadArg; }
    for (int c = 0; c < 7; c++)
      if (!kf_finite(poses[7 * m + c])) { *why = "a pose with a non-finite entry"; return kKfBadArg; }
  }
  return kKfOk;
}

// One compose request, validated and laid out.  Members are renumbered from 0 (member m of the plan is position member_off[0] + m of
// keys / poses).  Per kind the outputs are written back to back in member order: rec[k][m].dst is the running sum of the counts before
// it, off[k][b] the sum before submap b's first member.
struct KfPlan {
  int n_members = 0;
  std::vector<KfRec> rec[2];
  std::vector<double> poses;          // 8 doubles per member: the seven of the pose and one of padding (64-byte stride)
  std::vector<int> off[2];            // n_submaps + 1
  long long total[2] = {0, 0};
  int max_count = 0;                  // longest list of any member and kind: the x extent of the launch
};

inline int kf_plan_compose(const KfIndex& ix, int n_submaps, const int* member_off, const int* keys, const double* poses, float leaf_corner,
                           float leaf_surf, long long cap_corner, long long cap_surf, KfPlan* plan, const char** why) {
  if (n_submaps < 0 || !member_off || !plan) { *why = "bad argument"; return kKfBadArg; }
  if (!kf_leaf_ok(leaf_corner) || !kf_leaf_ok(leaf_surf)) { *why = "a leaf that is negative or not finite"; return kKfBadArg; }
  if (member_off[0] < 0) { *why = "a negative member offset"; return kKfBadArg; }
  for (int b = 0; b < n_submaps; b++)
    if (member_off[b + 1] < member_off[b]) { *why = "decreasing member offsets"; return kKfBadArg; }
  const long long first = member_off[0], last = member_off[n_submaps];
  if (last > first && (!keys || !poses)) { *why = "members without keys or poses"; return kKfBadArg; }
  const int s = kf_check_members(ix.size(), keys, poses, first, last, why);
  if (s) return s;
  // totals first, from the counts alone: nothing is sized before they are known to fit
  long long total[2] = {0, 0};
  for (long long m = first; m < last; m++)
    for (int k = 0; k < 2; k++) total[k] += ix.count[k][keys[m]];
  const long long cap[2] = {cap_corner, cap_surf};
  for (int k = 0; k < 2; k++) {
    if (total[k] > (long long)INT32_MAX) { *why = "a kind's member counts sum to 2^31 or more"; return kKfCapacity; }
    if (cap[k] < total[k]) { *why = "an output capacity below the sum of the member counts (msfl_keyframes_sizes)"; return kKfCapacity; }
  }
  const int M = (int)(last - first);
  plan->n_members = M;
  plan->poses.assign((size_t)M * 8, 0.0);
  plan->max_count = 0;
  for (int k = 0; k < 2; k++) {
    plan->rec[k].assign((size_t)M, KfRec{0, 0, 0, 0});
    plan->off[k].assign((size_t)n_submaps + 1, 0);
    plan->total[k] = total[k];
    long long run = 0;
    int b = 0;
    for (int m = 0; m < M; m++) {
      while (b < n_submaps && member_off[b] - first <= m) plan->off[k][b++] = (int)run;     // submaps that start at m (empty ones too)
      const int key = keys[first + m];
      plan->rec[k][m] = KfRec{ix.start[k][key], ix.count[k][key], (int)run, 0};
      run += ix.count[k][key];
      plan->max_count = std::max(plan->max_count, ix.count[k][key]);
    }
    while (b <= n_submaps) plan->off[k][b++] = (int)run;
  }
  for (int m = 0; m < M; m++)
    for (int c = 0; c < 7; c++) plan->poses[(size_t)8 * m + c] = poses[7 * (first + m) + c];
  return kKfOk;
}

// launch shape of the gather kernel: x = 1 024-point chunks of the longest member, y = members (at most kKfMaxGridY per launch: a
// longer table goes out in slices), z = the two kinds
struct KfGrid { unsigned x, y, z; };
inline KfGrid kf_grid_shape(int max_count, int n_members) {
  return KfGrid{(unsigned)((max_count + kKfChunk - 1) / kKfChunk), (unsigned)std::min(n_members, kKfMaxGridY), 2u};
}

}  // namespace msfl
