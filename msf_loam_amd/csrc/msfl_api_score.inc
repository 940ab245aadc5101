// Exact 1-NN fitness of pose hypotheses against the resident map — C-ABI entry points msfl_score_poses and
// msfl_score_poses_batch — or against the resident pair index, scan p against pair map p — msfl_score_pairs.  Included at the
// end of msfl_api.hip (shares its handle, DevBuf, PinRing and helper macros); kernels: msfl_score.cuh.  The call stages into scratch of its own (h->sc): a matcher call after it finds the poses, records,
// neighbour lists and offset table of the handle as it left them.

#include "msfl_score.cuh"

namespace {

static_assert(sizeof(ScoreRec) == sizeof(msfl_pose_score) && sizeof(msfl_pose_score) == 32, "pose score record layout");

// pairs: scan b against pair b of the resident pair index (msfl_api_pairs.inc), else every scan against the resident single map.
// d2_out / nn_out: one row of F values per hypothesis, in hypothesis order; without `pairs` only with n_scans == 1, with it the
// rows are ragged (F(b) values in a row of scan b).
msfl_status score_impl(msfl_handle* h, const char* who, bool pairs, int n_scans, const msfl_point* corner, const int* corner_off, const msfl_point* surf,
                       const int* surf_off, const double* poses, const int* pose_off, double max_dist, msfl_pose_score* scores, float* d2_out,
                       int* nn_out, msfl_mem mem) {
  const std::string w(who);
  if (n_scans < 0 || (n_scans > 0 && (!corner_off || !surf_off || !pose_off)) || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE))
    return fail(h, MSFL_BAD_ARG, w + ": null offset array, negative count or unknown memory kind");
  // the index is exact up to the radius it was built for; d2 <= 64 keeps the fixed-point sum of < 2^24 features below 2^63
  const double thr_d = max_dist * max_dist;
  if (!(max_dist > 0.0) || !(thr_d <= (double)h->prm.map_knn_max_sq_dist) || !(thr_d <= 64.0))
    return fail(h, MSFL_BAD_ARG, w + ": max_dist must be positive, with max_dist^2 <= params.map_knn_max_sq_dist and <= 64");
  if (pairs) { const msfl_status rs = pairs_resident(h, w, n_scans); if (rs) return rs; }
  else if (!h->have_map) return fail(h, MSFL_NO_MAP, w + ": no resident single map (msfl_set_map has not been called, or msfl_match_pairs_batch replaced it)");
  if (n_scans == 0) return MSFL_OK;
  const int c0 = corner_off[0], s0 = surf_off[0], p0 = pose_off[0];
  std::vector<int> offs(3 * (size_t)(n_scans + 1) + (pairs ? 2 * (size_t)n_scans : 0));
  int* co = offs.data(); int* so = co + (n_scans + 1); int* po = so + (n_scans + 1);
  int widest = 0;                          // workgroups of the scan with the most features, among the scans that have poses
  for (int b = 0; b <= n_scans; b++) {
    co[b] = corner_off[b] - c0; so[b] = surf_off[b] - s0; po[b] = pose_off[b] - p0;
    if (b == 0) continue;
    if (co[b] < co[b - 1] || so[b] < so[b - 1] || po[b] < po[b - 1]) return fail(h, MSFL_BAD_ARG, w + ": offset arrays must be non-decreasing");
    const long long nf = (long long)(co[b] - co[b - 1]) + (so[b] - so[b - 1]);
    if (nf >= (1 << 24)) return fail(h, MSFL_CAPACITY, w + ": a scan of 2^24 features or more");
    if (po[b] > po[b - 1]) widest = std::max(widest, div_up(co[b] - co[b - 1], kScoreBlock) + div_up(so[b] - so[b - 1], kScoreBlock));
  }
  const int ncp = co[n_scans], nsp = so[n_scans], H = po[n_scans];
  if (c0 < 0 || s0 < 0 || p0 < 0 || (ncp > 0 && !corner) || (nsp > 0 && !surf) || (H > 0 && (!poses || !scores)))
    return fail(h, MSFL_BAD_ARG, w + ": negative offset or null array");
  if (H == 0) return MSFL_OK;
  size_t n_out = (size_t)H * (size_t)(ncp + nsp);           // (single scan) per-feature outputs
  std::vector<unsigned long long> out0;                     // pairs: where every pair's rows begin, and where its map clouds do
  if (pairs) {
    int* mc0 = po + (n_scans + 1); int* ms0 = mc0 + n_scans;
    out0.resize(n_scans);
    n_out = 0;
    for (int b = 0, mc = 0, ms = 0; b < n_scans; b++) {
      mc0[b] = mc; ms0[b] = ms; out0[b] = n_out;
      mc += h->pr.n_c[b]; ms += h->pr.n_s[b];
      n_out += (size_t)(po[b + 1] - po[b]) * (size_t)((co[b + 1] - co[b]) + (so[b + 1] - so[b]));
    }
  }
  hipStream_t st = h->stream;
  ScoreJob j{};
  HIPCHK(h, h->sc.off.reserve(offs.size() * sizeof(int)));
  HIPCHK(h, h->pin.upload(h->sc.off.p, offs.data(), offs.size() * sizeof(int), st));
  j.corner_off = h->sc.off.as<int>(); j.surf_off = j.corner_off + (n_scans + 1); j.pose_off = j.surf_off + (n_scans + 1);
  j.n_scans = n_scans;
  if (n_scans > 1) {
    HIPCHK(h, h->sc.scan.reserve((size_t)H * sizeof(int)));
    j.scan_of = h->sc.scan.as<int>();
  }
  j.thr = (float)thr_d;
  ScorePairsView pv{};
  if (pairs) {
    pv.cbase_c = h->pr.base_c.as<int>(); pv.cbase_s = h->pr.base_s.as<int>();
    pv.map_c0 = j.pose_off + (n_scans + 1); pv.map_s0 = pv.map_c0 + n_scans;
    if ((d2_out || nn_out) && n_out) {
      HIPCHK(h, h->sc.out0.reserve(out0.size() * sizeof(unsigned long long)));
      HIPCHK(h, h->pin.upload(h->sc.out0.p, out0.data(), out0.size() * sizeof(unsigned long long), st));
      pv.out0 = h->sc.out0.as<unsigned long long>();
    }
  }
  // (both memory kinds read from the first used element on: the offsets are relative to it)
  msfl_status s = stage_in(h, h->sc.corner, ncp ? corner + c0 : corner, (size_t)ncp, mem, st, &j.corner); if (s) return s;
  s = stage_in(h, h->sc.surf, nsp ? surf + s0 : surf, (size_t)nsp, mem, st, &j.surf); if (s) return s;
  s = stage_in(h, h->sc.poses, poses + 7 * (size_t)p0, (size_t)H * 7, mem, st, &j.poses); if (s) return s;
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(h, h->sc.rec.reserve((size_t)H * sizeof(ScoreRec)));
    if (d2_out && n_out) HIPCHK(h, h->sc.d2.reserve(n_out * sizeof(float)));
    if (nn_out && n_out) HIPCHK(h, h->sc.nn.reserve(n_out * sizeof(int)));
    j.rec = h->sc.rec.as<ScoreRec>();
    j.d2_out = d2_out && n_out ? h->sc.d2.as<float>() : nullptr;
    j.nn_out = nn_out && n_out ? h->sc.nn.as<int>() : nullptr;
  } else {
    j.rec = reinterpret_cast<ScoreRec*>(scores) + p0;
    j.d2_out = d2_out; j.nn_out = nn_out;
  }
  // (a kernel, not hipMemsetAsync: a small memset node misbehaves under graph replay, DESIGN.md §6 (v); it also sets the status and,
  // in a batch, finds every hypothesis' scan)
  hipLaunchKernelGGL(score_init_kernel, dim3(div_up(H, 256)), dim3(256), 0, st, j, H, (int)MSFL_BAD_ARG);
  if (widest > 0) {
    for (int row0 = 0; row0 < H; row0 += kScoreMaxRows) {
      const int rows = std::min(kScoreMaxRows, H - row0);
      hipLaunchKernelGGL(pairs ? score_poses_kernel<true> : score_poses_kernel<false>, dim3(widest, rows), dim3(kScoreBlock), 0, st, j, row0,
                         (const GridDesc*)h->map_c.gdesc.as<GridDesc>(), (const float4*)h->map_c.sorted.as<float4>(), (const int*)h->map_c.cell_start.as<int>(),
                         (const GridDesc*)h->map_s.gdesc.as<GridDesc>(), (const float4*)h->map_s.sorted.as<float4>(), (const int*)h->map_s.cell_start.as<int>(),
                         pv);
    }
  }
  HIPCHK(h, hipGetLastError());
  s = stage_out(h, scores + p0, j.rec, (size_t)H, mem, st); if (s) return s;
  if (j.d2_out) { s = stage_out(h, d2_out, j.d2_out, n_out, mem, st); if (s) return s; }
  if (j.nn_out) { s = stage_out(h, nn_out, j.nn_out, n_out, mem, st); if (s) return s; }
  if (mem == MSFL_MEM_HOST) HIPCHK(h, hipStreamSynchronize(st));
  return MSFL_OK;
}

}  // namespace

extern "C" {

msfl_status msfl_score_poses(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf, const double* poses,
                             int n_poses, double max_dist, msfl_pose_score* scores, float* d2_out, int* nn_out, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n_corner < 0 || n_surf < 0 || n_poses < 0) return fail(h, MSFL_BAD_ARG, "msfl_score_poses: negative count");
  const int co[2] = {0, n_corner}, so[2] = {0, n_surf}, po[2] = {0, n_poses};
  return score_impl(h, "msfl_score_poses", false, 1, corner, co, surf, so, poses, po, max_dist, scores, d2_out, nn_out, mem);
}

msfl_status msfl_score_poses_batch(msfl_handle* h, int n_scans, const msfl_point* corner, const int* corner_off, const msfl_point* surf,
                                   const int* surf_off, const double* poses, const int* pose_off, double max_dist, msfl_pose_score* scores,
                                   msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  return score_impl(h, "msfl_score_poses_batch", false, n_scans, corner, corner_off, surf, surf_off, poses, pose_off, max_dist, scores, nullptr, nullptr, mem);
}

msfl_status msfl_score_pairs(msfl_handle* h, int n_pairs, const msfl_point* corner, const int* corner_off, const msfl_point* surf,
                             const int* surf_off, const double* poses, const int* pose_off, double max_dist, msfl_pose_score* scores,
                             float* d2_out, int* nn_out, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  return score_impl(h, "msfl_score_pairs", true, n_pairs, corner, corner_off, surf, surf_off, poses, pose_off, max_dist, scores, d2_out, nn_out, mem);
}

}  // extern "C"
