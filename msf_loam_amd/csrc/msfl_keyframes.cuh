// Keyframe store: the one kernel that lays stored point lists down at given poses (msfl_keyframes_compose / _insert), and gathers a
// caller's list into the store (msfl_keyframes_add).
//
//   kf_gather_kernel   member m of kind k: count points from src + rec.src .. -> TransformPoint(pose m) -> dst + rec.dst ..
//
// Launch geometry as pairs_bbox_kernel (msfl_pairs.cuh, docs/kernels/pairs.md): blockIdx.y = member, blockIdx.x = a chunk of
// kKfChunk points of it (four 16-byte points per lane, their loads issued together; a member's surplus workgroups leave at once),
// blockIdx.z = kind (corner / surf).  The member's record and its pose are wave-uniform loads from the table the host built from its
// own counts (msfl_keyframes_host.h): no wavefront searches an offset table.  The transform is msfl_transform_cloud's:
// f32 -> f64 -> q p + t -> f32, t carried over.  A streaming kernel: 16 B read and 16 B written per point, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "msfl_grid.cuh"
#include "msfl_keyframes_host.h"
#include "msfl_math.cuh"

namespace msfl {

struct KfKindView {
  const float4* src;        // the kind's pool (compose, insert) or the caller's array (add)
  const int* idx;           // add with an index list: point i of the member is src[idx[rec.src + i]]; null: src[rec.src + i]
  float4* dst;
  const KfRec* rec;         // one per member
  GridStoreDesc grid;       // kKfCheckCell: the store the points go to next
};
struct KfGatherArgs {
  KfKindView kind[2];
  const double* poses;      // 8 doubles per member
  int* bad;                 // raised (never cleared) by the two checks
  int member_base;          // blockIdx.y + member_base = member
};

__global__ void __launch_bounds__(256) kf_gather_kernel(KfGatherArgs a) {
  const bool surf = blockIdx.z != 0;
  const int m = (int)blockIdx.y + a.member_base;
  const KfRec rec = (surf ? a.kind[1].rec : a.kind[0].rec)[m];
  const int lo = (int)blockIdx.x * kKfChunk;
  if (lo >= rec.count) return;
  const float4* __restrict__ src = surf ? a.kind[1].src : a.kind[0].src;
  const int* __restrict__ idx = surf ? a.kind[1].idx : a.kind[0].idx;
  float4* __restrict__ dst = (surf ? a.kind[1].dst : a.kind[0].dst) + (size_t)rec.dst;
  float4 p[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int i = min(lo + u * 256 + (int)threadIdx.x, rec.count - 1);
    const size_t s = (size_t)rec.src + (size_t)i;
    p[u] = src[idx ? (size_t)idx[s] : s];
  }
  bool bad = false;
  if (rec.flags & kKfCheckFinite) {
#pragma unroll
    for (int u = 0; u < 4; u++) bad = bad || !(isfinite(p[u].x) && isfinite(p[u].y) && isfinite(p[u].z) && isfinite(p[u].w));
  }
  if (!(rec.flags & kKfCopy)) {
    const pose7 T = load_pose(a.poses + 8 * (size_t)m);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const float3 q = transform_point_f32(T, p[u].x, p[u].y, p[u].z);
      p[u] = make_float4(q.x, q.y, q.z, p[u].w);
    }
  }
  if (rec.flags & kKfCheckCell) {
    const GridStoreDesc d = surf ? a.kind[1].grid : a.kind[0].grid;
#pragma unroll
    for (int u = 0; u < 4; u++) bad = bad || grid_point_key(p[u], d) == kGridBadKey;
  }
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int i = lo + u * 256 + (int)threadIdx.x;
    if (i < rec.count) dst[i] = p[u];
  }
  if (bad) *a.bad = 1;      // (lanes past the end hold a copy of the member's last point: they flag nothing the others do not)
}

}  // namespace msfl
