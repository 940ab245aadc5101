// Batched (map, scan) PAIRS with distinct maps — C-ABI entry points msfl_match_pairs_batch and its two halves, msfl_set_pair_maps
// (the P-map index, which stays resident) and msfl_match_pairs_resident (the registrations against it).
// Included at the end of msfl_api.hip (shares its handle, DevBuf, PinRing and helper macros); kernels: msfl_pairs.cuh.
// Reference shape: one MappingScanMatcher::MatchScan2Map per (cloud_map, scan_curr), both kd-trees rebuilt inside the call
// (mapping_scan_matcher.cc:66-73; laser_mapping.cc:304-311).

#include "msfl_pairs.cuh"

namespace {

// One grid per pair over the concatenated clouds `d_pts` (device; pair p owns [off[p], off[p + 1])), into `mi`.
msfl_status build_pair_index(msfl_handle* h, const std::string& who, const float4* d_pts, const int* off, int P, MapIndex& mi, DevBuf& d_off, DevBuf& d_base) {
  ScopedTimer timer(h, T_INDEX);
  hipStream_t st = h->stream;
  const int n = off[P] - off[0];
  // cell table slices: host-known bounds (a dense 1 m grid over a LiDAR map has about one cell per point); the device grows a
  // pair's cell edge (still exact) when its bounding box needs more
  std::vector<int> base(P + 1);
  long long total = 0;
  for (int p = 0; p < P; p++) {
    base[p] = (int)total;
    const long long cap = std::min<long long>(std::max<long long>(4096, 2LL * (off[p + 1] - off[p])), h->grid_cap_cells);
    total += cap;
    if (total > 0x7fff0000LL) return fail(h, MSFL_CAPACITY, who + ": the pairs' cell tables exceed 2^31 cells together");
  }
  base[P] = (int)total;
  if (n >= (1 << 28)) return fail(h, MSFL_CAPACITY, who + ": 2^28 map points or more of one kind (the 5-NN walk addresses the sorted copy by 32-bit byte offsets)");
  HIPCHK(h, d_off.reserve((size_t)(P + 1) * sizeof(int)));
  HIPCHK(h, d_base.reserve((size_t)(P + 1) * sizeof(int)));
  HIPCHK(h, h->pin.upload(d_off.p, off, (size_t)(P + 1) * sizeof(int), st));
  HIPCHK(h, h->pin.upload(d_base.p, base.data(), (size_t)(P + 1) * sizeof(int), st));
  const size_t span = (size_t)total + 1;
  HIPCHK(h, mi.gdesc.reserve((size_t)P * sizeof(GridDesc)));
  HIPCHK(h, h->idx_cell_of.reserve(std::max<size_t>(1, (size_t)n) * sizeof(int)));
  const void* count_before = h->idx_count.p;
  HIPCHK(h, h->idx_count.reserve(span * sizeof(int)));
  if (h->idx_count.p != count_before) h->idx_count_zero = 0;
  HIPCHK(h, mi.cell_start.reserve(span * sizeof(int)));
  HIPCHK(h, mi.sorted.reserve(std::max<size_t>(1, (size_t)n) * sizeof(float4)));
  HIPCHK(h, mi.pos_of.reserve(std::max<size_t>(1, (size_t)n) * sizeof(int)));
  mi.n_input = n; mi.cap_cells = (int)std::min<long long>(total, INT32_MAX);
  const size_t zeroed = h->idx_count_zero;
  h->idx_count_zero = 0;
  if (span > zeroed) HIPCHK(h, hipMemsetAsync(h->idx_count.p, 0, span * sizeof(int), st));     // the scatter counts every cell back to zero
  const double radius = std::sqrt((double)h->prm.map_knn_max_sq_dist);
  DevBuf& bb = h->pr.bbox;                // not MapIndex::bbox: that one is the single-map build's, armed once and re-armed by its scatter kernel
  HIPCHK(h, bb.reserve((size_t)6 * P * sizeof(int)));
  hipLaunchKernelGGL(pairs_arm_kernel, dim3(div_up(6 * P, 256)), dim3(256), 0, st, bb.as<int>(), P);
  int longest = 0;
  for (int p = 0; p < P; p++) longest = std::max(longest, off[p + 1] - off[p]);
  const dim3 pgrid(std::max(1, div_up(longest, kPairChunk)), P);
  if (n > 0)
    hipLaunchKernelGGL(pairs_bbox_kernel, pgrid, dim3(256), 0, st, d_pts, (const int*)d_off.as<int>(), bb.as<int>());
  hipLaunchKernelGGL(pairs_desc_kernel, dim3(div_up(P, 256)), dim3(256), 0, st, (const int*)bb.as<int>(), P, (const int*)d_base.as<int>(), radius,
                     mi.gdesc.as<GridDesc>());
  if (n > 0)
    hipLaunchKernelGGL(pairs_count_kernel, pgrid, dim3(256), 0, st, d_pts, (const int*)d_off.as<int>(), (const int*)d_base.as<int>(),
                       (const GridDesc*)mi.gdesc.as<GridDesc>(), h->idx_cell_of.as<int>(), h->idx_count.as<int>());
  size_t tb = 0;
  HIPCHK(h, rocprim::exclusive_scan(nullptr, tb, h->idx_count.as<int>(), mi.cell_start.as<int>(), 0, span, rocprim::plus<int>(), st));
  HIPCHK(h, h->idx_cub.reserve(tb));
  HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tb, h->idx_count.as<int>(), mi.cell_start.as<int>(), 0, span, rocprim::plus<int>(), st));
  if (n > 0)
    hipLaunchKernelGGL(pairs_scatter_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, d_pts, n, (const int*)d_off.as<int>(), (const int*)h->idx_cell_of.as<int>(),
                       (const int*)mi.cell_start.as<int>(), h->idx_count.as<int>(), mi.sorted.as<float4>(), mi.pos_of.as<int>());
  HIPCHK(h, hipGetLastError());
  h->idx_count_zero = std::max(zeroed, span);
  return MSFL_OK;
}


// What both halves of a pairs call refuse before they stage or launch anything, in the order msfl_match_pairs_batch always had.  Either
// half may be absent (maps == false: msfl_match_pairs_resident; scans == false: msfl_set_pair_maps).  P == 0 passes: the caller returns.
msfl_status pairs_check(msfl_handle* h, const std::string& who, int P, bool maps, const msfl_point* map_corner, const int* map_corner_off,
                        const msfl_point* map_surf, const int* map_surf_off, bool scans, const msfl_point* corner, const int* corner_off,
                        const msfl_point* surf, const int* surf_off, const double* poses_io) {
  if (P < 0 || (P > 0 && ((maps && (!map_corner_off || !map_surf_off)) || (scans && (!corner_off || !surf_off || !poses_io)))))
    return fail(h, MSFL_BAD_ARG, who + ": null argument");
  if (P == 0) return MSFL_OK;
  // the segmented index build launches 2-D over (chunk, pair): HIP caps gridDim.y at 65 535 (ADVICE r04) — say so up front, before any staging
  if (P > 65535) return fail(h, MSFL_CAPACITY, who + ": at most 65535 pairs per call (got " + std::to_string(P) + "); split the batch");
  if (scans) { const msfl_status s = reg_check(h, P, who.c_str()); if (s) return s; }
  for (int p = 0; p < P; p++)
    if ((maps && (map_corner_off[p + 1] < map_corner_off[p] || map_surf_off[p + 1] < map_surf_off[p])) ||
        (scans && (corner_off[p + 1] < corner_off[p] || surf_off[p + 1] < surf_off[p])))
      return fail(h, MSFL_BAD_ARG, who + ": offset arrays must be non-decreasing");
  if ((maps && ((map_corner_off[P] - map_corner_off[0] > 0 && !map_corner) || (map_surf_off[P] - map_surf_off[0] > 0 && !map_surf))) ||
      (scans && ((corner_off[P] - corner_off[0] > 0 && !corner) || (surf_off[P] - surf_off[0] > 0 && !surf))))
    return fail(h, MSFL_BAD_ARG, who + ": null cloud");
  return MSFL_OK;
}

// The index half: the P maps staged (host memory) and indexed, one grid per pair; the handle then remembers the pair index on the host.
// Checked arguments (pairs_check), P > 0.  Nothing is waited for: a host-memory caller does that before it returns.
msfl_status pair_maps_build(msfl_handle* h, const std::string& who, int P, const msfl_point* map_corner, const int* map_corner_off,
                            const msfl_point* map_surf, const int* map_surf_off, msfl_mem mem) {
  hipStream_t st = h->stream;
  h->have_map = false;                                   // the handle's resident single map (msfl_set_map) is replaced by the pairs' indices
  h->pr.resident = false;                                // ... and so is an earlier pair index, also when this build fails
  const int nmc = map_corner_off[P] - map_corner_off[0], nms = map_surf_off[P] - map_surf_off[0];
  std::vector<int> mco(map_corner_off, map_corner_off + P + 1), mso(map_surf_off, map_surf_off + P + 1);
  const float4* d_mc = reinterpret_cast<const float4*>(map_corner);
  const float4* d_ms = reinterpret_cast<const float4*>(map_surf);
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(h, h->idx_stage.reserve(std::max<size_t>(1, (size_t)nmc + (size_t)nms) * sizeof(float4)));
    float4* stage = h->idx_stage.as<float4>();
    if (nmc) HIPCHK(h, hipMemcpyAsync(stage, map_corner + mco[0], (size_t)nmc * sizeof(float4), hipMemcpyHostToDevice, st));
    if (nms) HIPCHK(h, hipMemcpyAsync(stage + nmc, map_surf + mso[0], (size_t)nms * sizeof(float4), hipMemcpyHostToDevice, st));
    const int a = mco[0], b = mso[0];
    for (int p = 0; p <= P; p++) { mco[p] -= a; mso[p] -= b; }
    d_mc = stage; d_ms = stage + nmc;
  }
  msfl_status s = build_pair_index(h, who, d_mc, mco.data(), P, h->map_c, h->pr.off_c, h->pr.base_c); if (s) return s;
  s = build_pair_index(h, who, d_ms, mso.data(), P, h->map_s, h->pr.off_s, h->pr.base_s); if (s) return s;
  h->pr.n_c.resize(P); h->pr.n_s.resize(P);
  for (int p = 0; p < P; p++) { h->pr.n_c[p] = mco[p + 1] - mco[p]; h->pr.n_s[p] = mso[p + 1] - mso[p]; }
  h->pr.resident = true;
  return MSFL_OK;
}

// The registration half: scan p against pair p of the resident pair index.  Checked arguments (pairs_check), P = the index's pairs.
msfl_status pairs_register(msfl_handle* h, int P, const msfl_point* corner, const int* corner_off, const msfl_point* surf, const int* surf_off,
                           double* poses_io, int* status, msfl_match_info* info, msfl_mem mem) {
  hipStream_t st = h->stream;
  const int c0 = corner_off[0], s0 = surf_off[0];
  const int ncp = corner_off[P] - c0, nsp = surf_off[P] - s0;
  std::vector<int> co(corner_off, corner_off + P + 1), so(surf_off, surf_off + P + 1);
  const float4 *d_corner, *d_surf;
  double* d_poses;
  const bool host = mem == MSFL_MEM_HOST;          // host clouds are staged from their first used point, and the offsets follow
  msfl_status s = stage_in(h, h->in_corner, host && ncp ? corner + c0 : corner, (size_t)ncp, mem, st, &d_corner); if (s) return s;
  s = stage_in(h, h->in_surf, host && nsp ? surf + s0 : surf, (size_t)nsp, mem, st, &d_surf); if (s) return s;
  s = stage_in(h, h->poses, poses_io, (size_t)P * 7, mem, st, &d_poses); if (s) return s;
  if (host) for (int p = 0; p <= P; p++) { co[p] -= c0; so[p] -= s0; }
  // per-pair status, preset on the host: a pair whose map cloud has fewer than 5 points is not matched
  // (mapping_scan_matcher.cc:128,198 would index pointSearchSqDis[4] out of bounds; the reference's caller gates, laser_mapping.cc:284-285)
  std::vector<int> st0(P, 0);
  for (int p = 0; p < P; p++)
    if (h->pr.n_c[p] < 5 || h->pr.n_s[p] < 5) st0[p] = MSFL_MAP_TOO_SMALL;
  int* d_status = status;
  if (mem != MSFL_MEM_DEVICE || !status) { HIPCHK(h, h->status.reserve((size_t)P * sizeof(int))); d_status = h->status.as<int>(); }
  HIPCHK(h, h->pin.upload(d_status, st0.data(), (size_t)P * sizeof(int), st));
  RegSinks sinks;
  s = reg_open(h, P, st, info != nullptr, &sinks); if (s) return s;
  int n_rec = 0;
  s = upload_batch_offsets(h, P, co.data(), so.data(), &n_rec); if (s) return s;
  HIPCHK(h, h->records.reserve(record_bytes((size_t)n_rec, (size_t)(so[P] - so[0]))));
  HIPCHK(h, h->nn.reserve(std::max<size_t>(1, (size_t)n_rec) * 5 * sizeof(int)));
  const BatchView bv = batch_view(d_corner, d_surf, h->in_off.as<int>(), P + 1, P, n_rec, co[0], so[0], so[P] - so[0]);
  DeskewView dv{};
  const dim3 grid(std::max(1, div_up(n_rec, kAssocBlock))), block(kAssocBlock);
  int longest = 0;
  for (int p = 0; p < P; p++) longest = std::max(longest, (co[p + 1] - co[p]) + (so[p + 1] - so[p]));
  s = solve_outer<kLmBlock>(h, P, bv, nullptr, d_poses, d_status, sinks, solver_params(h->prm, 0), h->prm.outer_iterations, [&](int it) {
    if (n_rec <= 0) return MSFL_OK;
    {
      ScopedTimer timer(h, it > 0 ? T_ASSOC_SEEDED : T_ASSOC);
      launch_knn5(h, knn5_scan2map_kernel<false, false, true>, grid, block, bv, d_poses, d_status, dv, h->nn.as<int>(),
                  nullptr, h->pr.base_c.as<int>(), h->pr.base_s.as<int>());
    }
    ScopedTimer timer(h, T_FIT);       // nn holds positions in the concatenated sorted maps: the fit gathers as ever
    hipLaunchKernelGGL(fit_scan2map_kernel<false>, grid, block, 0, st, bv, h->map_c.sorted.as<float4>(), h->map_s.sorted.as<float4>(),
                       (const int*)h->nn.as<int>(), h->prm.line_eigen_ratio, h->prm.plane_tolerance, dv, h->records.as<double>(), (double*)nullptr);
    return MSFL_OK;
  }, longest);
  if (s) return s;
  return reg_close(h, P, mem, poses_io, d_poses, status, d_status, info, sinks);
}

// msfl_score_pairs / msfl_match_pairs_resident: is there a pair index of n_pairs pairs?
msfl_status pairs_resident(msfl_handle* h, const std::string& who, int n_pairs) {
  if (!h->pr.resident)
    return fail(h, MSFL_NO_MAP, who + ": no resident pair index (neither msfl_set_pair_maps nor msfl_match_pairs_batch has been called, or msfl_set_map replaced it)");
  if (n_pairs != (int)h->pr.n_c.size())
    return fail(h, MSFL_BAD_ARG, who + ": " + std::to_string(n_pairs) + " pairs, the resident pair index holds " + std::to_string(h->pr.n_c.size()));
  return MSFL_OK;
}

}  // namespace

extern "C" {

msfl_status msfl_set_pair_maps(msfl_handle* h, int n_pairs, const msfl_point* map_corner, const int* map_corner_off,
                               const msfl_point* map_surf, const int* map_surf_off, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  const std::string who = "msfl_set_pair_maps";
  s = pairs_check(h, who, n_pairs, true, map_corner, map_corner_off, map_surf, map_surf_off, false, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (s || n_pairs == 0) return s;
  s = pair_maps_build(h, who, n_pairs, map_corner, map_corner_off, map_surf, map_surf_off, mem); if (s) return s;
  // host arrays were staged with asynchronous copies from pageable memory: read before the caller may touch them again (msfl_set_map)
  if (mem == MSFL_MEM_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
  return MSFL_OK;
}

msfl_status msfl_match_pairs_resident(msfl_handle* h, int n_pairs, const msfl_point* corner, const int* corner_off, const msfl_point* surf,
                                      const int* surf_off, double* poses_io, int* status, msfl_match_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  const std::string who = "msfl_match_pairs_resident";
  s = pairs_resident(h, who, n_pairs); if (s) return s;
  s = pairs_check(h, who, n_pairs, false, nullptr, nullptr, nullptr, nullptr, true, corner, corner_off, surf, surf_off, poses_io); if (s) return s;
  return pairs_register(h, n_pairs, corner, corner_off, surf, surf_off, poses_io, status, info, mem);
}

msfl_status msfl_match_pairs_batch(msfl_handle* h, int n_pairs,
                                   const msfl_point* map_corner, const int* map_corner_off, const msfl_point* map_surf, const int* map_surf_off,
                                   const msfl_point* corner, const int* corner_off, const msfl_point* surf, const int* surf_off,
                                   double* poses_io, int* status, msfl_match_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  const std::string who = "msfl_match_pairs_batch";
  s = pairs_check(h, who, n_pairs, true, map_corner, map_corner_off, map_surf, map_surf_off, true, corner, corner_off, surf, surf_off, poses_io);
  if (s || n_pairs == 0) return s;
  s = pair_maps_build(h, who, n_pairs, map_corner, map_corner_off, map_surf, map_surf_off, mem); if (s) return s;   // (its index stays resident)
  return pairs_register(h, n_pairs, corner, corner_off, surf, surf_off, poses_io, status, info, mem);
}

}  // extern "C"
