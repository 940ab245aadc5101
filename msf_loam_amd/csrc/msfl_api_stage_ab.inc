// Stage A (feature extraction), stage B (scan-to-scan) and the voxel helper: C-ABI entry points.
// Included at the end of msfl_api.hip (shares its handle, DevBuf, PinRing and helper macros).

namespace {

// the smallest f32 s with (double)sqrtf(s) >= min_range: "norm() < min_range" (f32 norm, double compare) is "s < this"
float min_range_sq_threshold(double min_range) {
  if (!(min_range > 0.0)) return 0.f;                               // nothing is closer than a non-positive (or NaN) range
  if (!(min_range < 1.8e19)) return INFINITY;                       // beyond sqrt(FLT_MAX): every finite squared norm is too close
  float c = (float)(min_range * min_range);
  while ((double)sqrtf(c) >= min_range && c > 0.f) c = nextafterf(c, 0.f);
  while ((double)sqrtf(c) < min_range) c = nextafterf(c, INFINITY);
  return c;
}

ExtractParams extract_params(const msfl_params& p) {
  ExtractParams e;
  e.min_range = p.min_range;
  e.min_range_sq = min_range_sq_threshold(p.min_range);
  e.scan_period = p.scan_period;
  e.curvature_threshold = 0.1;   // the reference compares the f32 curvature with the DOUBLE literal 0.1
  e.neighbor_gap_sq = 0.05;      // ... and the f32 gap with the double literal 0.05 (:275, :293)
  if (p.curvature_threshold != 0.1f) e.curvature_threshold = (double)p.curvature_threshold;
  if (p.neighbor_gap_sq != 0.05f) e.neighbor_gap_sq = (double)p.neighbor_gap_sq;
  e.sectors = p.sectors_per_ring;
  e.max_sharp = p.max_sharp_per_sector;
  e.max_less_sharp = p.max_less_sharp_per_sector;
  e.max_flat = p.max_flat_per_sector;
  return e;
}

// All array pointers are device pointers; `h_off` is the host offset table.
msfl_status extract_device(msfl_handle* h, int B, const float4* d_pts, const uint16_t* d_ring, const int* h_off,
                           const double* d_extrinsic, ExtractView& v) {
  hipStream_t st = h->stream;
  const int o0 = h_off[0];
  const int n_total = h_off[B] - o0;
  HIPCHK(h, h->ex.off.reserve((size_t)(B + 1) * sizeof(int)));
  std::vector<int> offs(B + 1);
  for (int b = 0; b <= B; b++) {
    offs[b] = h_off[b] - o0;
    if (b > 0 && offs[b] < offs[b - 1]) return fail(h, MSFL_BAD_ARG, "extract: offsets must be non-decreasing");
  }
  HIPCHK(h, h->pin.upload(h->ex.off.p, offs.data(), offs.size() * sizeof(int), st));
  const size_t nt = std::max<size_t>(1, (size_t)n_total);
  HIPCHK(h, h->ex.gap.reserve(nt));
  HIPCHK(h, h->ex.ring_tab.reserve((size_t)B * (kMaxRings + 1) * sizeof(int)));
  HIPCHK(h, h->ex.tmp_idx.reserve(nt * 4 * sizeof(int)));
  HIPCHK(h, h->ex.ring_cnt.reserve((size_t)B * kMaxRings * 4 * sizeof(int)));
  v.in_pts = d_pts + o0; v.in_ring = d_ring + o0; v.off = h->ex.off.as<int>(); v.n_scans = B; v.n_total = n_total;
  v.gap = h->ex.gap.as<uint8_t>(); v.ring_tab = h->ex.ring_tab.as<int>();
  v.tmp_idx = h->ex.tmp_idx.as<int>(); v.ring_cnt = h->ex.ring_cnt.as<int>();
  HIPCHK(h, hipMemsetAsync(v.status, 0, (size_t)B * sizeof(int), st));
  const ExtractParams ep = extract_params(h->prm);
  ScopedTimer timer(h, T_EXTRACT);
  // few scans (the SLAM step: one): G workgroups per scan in three launches instead of one workgroup per scan, so that the
  // chip is not left to B compute units (a 64-beam sweep: 326 -> ~60 us); a batch that fills the chip by itself keeps G = 1
  int G = h->prep_split > 0 ? h->prep_split : B <= 16 ? 16 : B <= 32 ? 8 : B <= 64 ? 4 : B <= 128 ? 2 : 1;
  // a batch of 64-beam sweeps (> 65 536 points each) is still better off with two workgroups per scan: 5.01 -> 4.78 ms of extraction per
  // 1 250 scans (G = 4: 4.91, 16: 7.0); 1 024 16-beam scans: 0.81 ms with one workgroup per scan, 0.96 with two
  if (h->prep_split <= 0 && G == 1 && B > 0 && (long long)n_total / B > 65536) G = 2;
  if ((long long)B * G > 65535) G = 1;
  if (G > 1) {
    HIPCHK(h, h->ex.split.reserve(prep_split_bytes(B, G)));
    const PrepSplitView sv = prep_split_view(h->ex.split.p, B, G);
    hipLaunchKernelGGL(extract_prepare_count_kernel, dim3(G, B), dim3(1024), 0, st, v, ep, sv);
    hipLaunchKernelGGL(extract_prepare_scatter_kernel, dim3(G, B), dim3(1024), 0, st, v, ep, sv);
    hipLaunchKernelGGL(extract_prepare_finish_kernel, dim3(G, B), dim3(1024), 0, st, v, ep, sv);
  } else {
    hipLaunchKernelGGL(extract_prepare_kernel, dim3(B), dim3(1024), 0, st, v, ep);
  }
  int longest = 0;
  for (int b = 0; b < B; b++) longest = std::max(longest, offs[b + 1] - offs[b]);
  if (n_total > 0) hipLaunchKernelGGL(extract_curvature_kernel, dim3(div_up(longest, 256), B), dim3(256), 0, st, v, ep);
  hipLaunchKernelGGL(extract_pick_kernel, dim3(B, div_up(kMaxRings, kExWaves)), dim3(64 * kExWaves), 0, st, v, ep);
  hipLaunchKernelGGL(extract_compact_kernel, dim3(G, B), dim3(kCompactThreads), 0, st, v, d_extrinsic);
  HIPCHK(h, hipGetLastError());
  return MSFL_OK;
}

msfl_status extract_batch_impl(msfl_handle* h, int B, const msfl_point* pts, const uint16_t* ring, const int* off,
                               const double* extrinsic, msfl_features_batch* out, int* status, msfl_mem mem) {
  if (B < 0 || !out || (B > 0 && !off)) return fail(h, MSFL_BAD_ARG, "msfl_extract_features_batch: null argument");
  if (B == 0) return MSFL_OK;
  const int o0 = off[0], n_total = off[B] - o0;
  if (n_total < 0 || (n_total > 0 && (!pts || !ring))) return fail(h, MSFL_BAD_ARG, "msfl_extract_features_batch: bad input");
  if (!out->full_pts || !out->full_ring || !out->curvature || !out->label || !out->sharp_idx || !out->less_sharp_idx ||
      !out->flat_idx || !out->less_flat_idx || !out->n_full || !out->n_sharp || !out->n_less_sharp || !out->n_flat || !out->n_less_flat)
    return fail(h, MSFL_BAD_ARG, "msfl_extract_features_batch: null output array");
  hipStream_t st = h->stream;
  const size_t nt = std::max<size_t>(1, (size_t)n_total);
  ExtractView v{};
  const double* d_ext = nullptr;
  if (extrinsic) {
    HIPCHK(h, h->poses.reserve(7 * sizeof(double)));
    HIPCHK(h, h->pin.upload(h->poses.p, extrinsic, 7 * sizeof(double), st));
    d_ext = h->poses.as<double>();
  }
  if (mem == MSFL_MEM_DEVICE) {
    v.full_pts = reinterpret_cast<float4*>(out->full_pts) + o0; v.full_ring = out->full_ring + o0;
    v.curvature = out->curvature + o0; v.label = out->label + o0;
    v.sharp_idx = out->sharp_idx + o0; v.less_sharp_idx = out->less_sharp_idx + o0;
    v.flat_idx = out->flat_idx + o0; v.less_flat_idx = out->less_flat_idx + o0;
    v.n_full = out->n_full; v.n_sharp = out->n_sharp; v.n_less_sharp = out->n_less_sharp; v.n_flat = out->n_flat;
    v.n_less_flat = out->n_less_flat;
    if (status) v.status = status;
    else { HIPCHK(h, h->ex.status.reserve((size_t)B * sizeof(int))); v.status = h->ex.status.as<int>(); }
    return extract_device(h, B, reinterpret_cast<const float4*>(pts), ring, off, d_ext, v);
  }
  // host mode: stage in, run, stage out
  const float4* d_pts; const uint16_t* d_ring;
  msfl_status s = stage_in(h, h->ex.in_pts, n_total ? pts + o0 : pts, (size_t)n_total, mem, st, &d_pts); if (s) return s;
  s = stage_in(h, h->ex.in_ring, n_total ? ring + o0 : ring, (size_t)n_total, mem, st, &d_ring); if (s) return s;
  // All outputs live in ONE device buffer.  A small call (one scan is ~1 MB of outputs) brings them back with one copy
  // into pinned memory and hands them out with memcpy: fourteen separate transfers of 24 B .. 380 KB were 0.25 ms of a
  // single scan's 0.45.  A large batch keeps one transfer per array straight into the caller's memory.
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t o_full = 0, o_idx = o_full + up(nt * sizeof(float4)), o_curv = o_idx + up(nt * 4 * sizeof(int)),
               o_ring = o_curv + up(nt * sizeof(float)), o_label = o_ring + up(nt * sizeof(uint16_t)),
               o_cnt = o_label + up(nt), o_status = o_cnt + up((size_t)B * 5 * sizeof(int)), pack_bytes = o_status + up((size_t)B * sizeof(int));
  HIPCHK(h, h->ex.pack.reserve(pack_bytes));
  char* pack = h->ex.pack.as<char>();
  v.full_pts = reinterpret_cast<float4*>(pack + o_full); v.full_ring = reinterpret_cast<uint16_t*>(pack + o_ring);
  v.curvature = reinterpret_cast<float*>(pack + o_curv); v.label = reinterpret_cast<uint8_t*>(pack + o_label);
  int* idx = reinterpret_cast<int*>(pack + o_idx);
  v.sharp_idx = idx; v.less_sharp_idx = idx + nt; v.flat_idx = idx + 2 * nt; v.less_flat_idx = idx + 3 * nt;
  int* cnt = reinterpret_cast<int*>(pack + o_cnt);
  v.n_full = cnt; v.n_sharp = cnt + B; v.n_less_sharp = cnt + 2 * B; v.n_flat = cnt + 3 * B; v.n_less_flat = cnt + 4 * B;
  v.status = reinterpret_cast<int*>(pack + o_status);
  std::vector<int> rel_off(B + 1);
  for (int b = 0; b <= B; b++) rel_off[b] = off[b] - o0;
  s = extract_device(h, B, d_pts, d_ring, rel_off.data(), d_ext, v);
  if (s) return s;
  const size_t n = (size_t)n_total;
  int* out_cnt[5] = {out->n_full, out->n_sharp, out->n_less_sharp, out->n_flat, out->n_less_flat};
  int* lists[4] = {out->sharp_idx, out->less_sharp_idx, out->flat_idx, out->less_flat_idx};
  if (pack_bytes <= (size_t)4 << 20) {
    HIPCHK(h, h->readback.reserve(pack_bytes));
    const char* hp = h->readback.as<char>();
    HIPCHK(h, hipMemcpyAsync(h->readback.p, pack, pack_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (n) {
      std::memcpy(out->full_pts + o0, hp + o_full, n * sizeof(float4));
      std::memcpy(out->full_ring + o0, hp + o_ring, n * sizeof(uint16_t));
      std::memcpy(out->curvature + o0, hp + o_curv, n * sizeof(float));
      std::memcpy(out->label + o0, hp + o_label, n);
      for (int k = 0; k < 4; k++) std::memcpy(lists[k] + o0, hp + o_idx + (size_t)k * nt * sizeof(int), n * sizeof(int));
    }
    for (int k = 0; k < 5; k++) std::memcpy(out_cnt[k], hp + o_cnt + (size_t)k * B * sizeof(int), (size_t)B * sizeof(int));
    if (status) std::memcpy(status, hp + o_status, (size_t)B * sizeof(int));
    return MSFL_OK;
  }
  s = stage_out(h, out->full_pts + o0, v.full_pts, n, mem, st); if (s) return s;
  s = stage_out(h, out->full_ring + o0, v.full_ring, n, mem, st); if (s) return s;
  s = stage_out(h, out->curvature + o0, v.curvature, n, mem, st); if (s) return s;
  s = stage_out(h, out->label + o0, v.label, n, mem, st); if (s) return s;
  for (int k = 0; k < 4; k++) { s = stage_out(h, lists[k] + o0, idx + (size_t)k * nt, n, mem, st); if (s) return s; }
  for (int k = 0; k < 5; k++) { s = stage_out(h, out_cnt[k], cnt + (size_t)k * B, (size_t)B, mem, st); if (s) return s; }
  if (status) { s = stage_out(h, status, v.status, (size_t)B, mem, st); if (s) return s; }
  HIPCHK(h, hipStreamSynchronize(st));
  return MSFL_OK;
}

// The column index of one feature family as the association kernel takes it: a pair's queries (`longest_query` in the pair with the
// most) go `queries_per_block` to a workgroup.  use = false: no index, the family's queries stay on the brute-force kernel.  Else `b` is
// reserved for B pairs whose previous-scan clouds end at point `n_sorted` of their array.
msfl_status odom_index(msfl_handle* h, OdomIndexBufs& b, bool use, int B, size_t n_sorted, int longest_query, int queries_per_block, OdomIndex* ix) {
  *ix = OdomIndex{nullptr, nullptr, nullptr, nullptr, std::max(1, div_up(longest_query, queries_per_block))};
  if (!use) return MSFL_OK;
  HIPCHK(h, b.tab.reserve((size_t)B * kOdomTabStride * sizeof(unsigned)));
  HIPCHK(h, b.sorted.reserve(n_sorted * sizeof(float4)));
  HIPCHK(h, b.desc.reserve((size_t)B * sizeof(OdomPairDesc)));
  HIPCHK(h, b.mode.reserve((size_t)B * sizeof(int)));
  ix->tab = b.tab.as<unsigned>(); ix->sorted = b.sorted.as<float4>(); ix->desc = b.desc.as<OdomPairDesc>(); ix->mode = b.mode.as<int>();
  return MSFL_OK;
}
// The build job of that index over the family's clouds (the build writes what the queries only read).
OdomBinJob odom_bin_job(const float4* pts, const uint16_t* ring, const int* off, const OdomIndex& ix) {
  return OdomBinJob{pts, ring, off, const_cast<unsigned*>(ix.tab), const_cast<float4*>(ix.sorted), const_cast<OdomPairDesc*>(ix.desc), const_cast<int*>(ix.mode)};
}

// The index build of `jobs` clouds (n_pairs less-flat clouds, then -- jobs = 2 n_pairs -- the less-sharp ones): one workgroup per cloud,
// or, when the call holds few pairs and a cloud is long (`longest` points: a 64-beam less-flat list), 64 workgroups per cloud in four launches.
msfl_status launch_odom_bin(msfl_handle* h, hipStream_t st, const OdomBinJob& job_lf, const OdomBinJob& job_ls, int jobs, int n_pairs, long long longest) {
  const bool split = h->odom_bin_split >= 0 ? h->odom_bin_split != 0 : (n_pairs <= 4 && longest > 32768);
  if (!split || jobs > 65535) {
    hipLaunchKernelGGL(odom_bin_kernel, dim3(jobs), dim3(1024), 0, st, job_lf, job_ls, n_pairs);
    return MSFL_OK;
  }
  OdomBinSplit sp;
  sp.G = 64;
  const size_t cur_bytes = (size_t)jobs * kOdomTabStride * sizeof(unsigned);
  HIPCHK(h, h->od.split.reserve(cur_bytes + (size_t)jobs * sp.G * 8 * sizeof(int)));
  sp.cur = h->od.split.as<unsigned>();
  sp.part = reinterpret_cast<int*>(h->od.split.as<char>() + cur_bytes);
  hipLaunchKernelGGL(odom_bin_box_kernel, dim3(sp.G, jobs), dim3(kOdomSplitThreads), 0, st, job_lf, job_ls, n_pairs, sp);
  hipLaunchKernelGGL(odom_bin_count_kernel, dim3(sp.G, jobs), dim3(kOdomSplitThreads), 0, st, job_lf, job_ls, n_pairs, sp);
  hipLaunchKernelGGL(odom_bin_scan_kernel, dim3(jobs), dim3(1024), 0, st, job_lf, job_ls, n_pairs, sp);
  hipLaunchKernelGGL(odom_bin_scatter_kernel, dim3(sp.G, jobs), dim3(kOdomSplitThreads), 0, st, job_lf, job_ls, n_pairs, sp);
  return MSFL_OK;
}

msfl_status scan2scan_batch_impl(msfl_handle* h, int B, const msfl_ring_cloud_batch* c0, const msfl_ring_cloud_batch* c1,
                                 const msfl_ring_cloud_batch* c2, const msfl_ring_cloud_batch* c3, double* poses_io,
                                 int* status, msfl_match_info* info, msfl_mem mem) {
  if (B < 0 || (B > 0 && (!c0 || !c1 || !c2 || !c3 || !poses_io))) return fail(h, MSFL_BAD_ARG, "msfl_match_scan2scan_batch: null argument");
  if (B == 0) return MSFL_OK;
  { const msfl_status us = reg_check(h, B, "msfl_match_scan2scan"); if (us) return us; }
  const msfl_ring_cloud_batch* cl[4] = {c0, c1, c2, c3};
  hipStream_t st = h->stream;
  for (int k = 0; k < 4; k++) {
    if (!cl[k]->off) return fail(h, MSFL_BAD_ARG, "msfl_match_scan2scan_batch: null offsets");
    const int n = cl[k]->off[B] - cl[k]->off[0];
    if (n < 0 || (n > 0 && !cl[k]->pts) || (k < 2 && n > 0 && !cl[k]->ring))
      return fail(h, MSFL_BAD_ARG, "msfl_match_scan2scan_batch: bad cloud");
    for (int b = 0; b < B; b++) if (cl[k]->off[b + 1] < cl[k]->off[b]) return fail(h, MSFL_BAD_ARG, "offsets must be non-decreasing");
  }
  // offsets: [ls (B+1) | lf | sharp | flat | rec]
  std::vector<int> offs(5 * (size_t)(B + 1));
  const int base[4] = {cl[0]->off[0], cl[1]->off[0], cl[2]->off[0], cl[3]->off[0]};
  for (int b = 0; b <= B; b++) {
    for (int k = 0; k < 4; k++) offs[k * (B + 1) + b] = cl[k]->off[b] - (mem == MSFL_MEM_HOST ? base[k] : 0);
    offs[4 * (B + 1) + b] = (cl[2]->off[b] - base[2]) + (cl[3]->off[b] - base[3]);
  }
  const int n_rec = offs[4 * (B + 1) + B];
  HIPCHK(h, h->od.offs.reserve(offs.size() * sizeof(int)));
  HIPCHK(h, h->pin.upload(h->od.offs.p, offs.data(), offs.size() * sizeof(int), st));
  const int* d_off = h->od.offs.as<int>();
  const float4* d_pts[4]; const uint16_t* d_ring[2];
  double* d_poses; int* d_status;
  for (int k = 0; k < 4; k++) {          // a host cloud is staged from its first used point (the offsets above are relative to it)
    const size_t n = (size_t)(cl[k]->off[B] - base[k]), skip = mem == MSFL_MEM_HOST && n ? (size_t)base[k] : 0;
    msfl_status us = stage_in(h, h->od.pts[k], cl[k]->pts + skip, n, mem, st, &d_pts[k]); if (us) return us;
    if (k < 2) { us = stage_in(h, h->od.ring[k], cl[k]->ring + skip, n, mem, st, &d_ring[k]); if (us) return us; }
  }
  { const msfl_status us = stage_in(h, h->od.poses, poses_io, (size_t)B * 7, mem, st, &d_poses); if (us) return us; }
  if (mem == MSFL_MEM_DEVICE && status) d_status = status;
  else { HIPCHK(h, h->od.status.reserve((size_t)B * sizeof(int))); d_status = h->od.status.as<int>(); }
  HIPCHK(h, hipMemsetAsync(d_status, 0, (size_t)B * sizeof(int), st));
  RegSinks sinks;
  { const msfl_status us = reg_open(h, B, st, info != nullptr, &sinks); if (us) return us; }
  HIPCHK(h, h->records.reserve(record_bytes((size_t)n_rec, (size_t)(offs[3 * (B + 1) + B] - offs[3 * (B + 1)]))));
  // the current scan's sharp / flat lists are the problem's corner / surf clouds: rows 2, 3 and 4 of the table
  const BatchView bv = batch_view(d_pts[2], d_pts[3], d_off + 2 * (B + 1), B + 1, B, n_rec, offs[2 * (B + 1)], offs[3 * (B + 1)],
                                  offs[3 * (B + 1) + B] - offs[3 * (B + 1)]);
  OdomView ov;
  ov.last_ls = d_pts[0]; ov.last_ls_ring = d_ring[0]; ov.last_ls_off = d_off;
  ov.last_lf = d_pts[1]; ov.last_lf_ring = d_ring[1]; ov.last_lf_off = d_off + (B + 1);
  ov.dist_sq_threshold = h->prm.odom_distance_sq_threshold;
  ov.nearby_scan = h->prm.odom_nearby_scan;
  int max_q = 0;
  for (int b = 0; b < B; b++) max_q = std::max(max_q, offs[4 * (B + 1) + b + 1] - offs[4 * (B + 1) + b]);
  const SolverParams sp = solver_params(h->prm, h->prm.odom_min_correspondences);
  // few pairs: one wavefront per query (latency).  many pairs: edges brute-force through LDS tiles,
  // planes through a per-pair column grid of the previous scan's less-flat cloud (throughput).
  // (the wave kernel sweeps the whole previous cloud per query: with a 20 k-point less-flat cloud even ONE pair is faster
  // through the column grid — 0.40 ms of sweeps per call against 0.06 ms of binning + walks — so it only keeps the small cases)
  const long long n_targets = (long long)(offs[B] - offs[0]) + (long long)(offs[(B + 1) + B] - offs[B + 1]);
  const bool latency_path = (long long)B * max_q <= 16384 && n_targets <= (h->odom_wave_max_targets >= 0 ? h->odom_wave_max_targets : 4096LL * B);
  int max_flat = 0;
  for (int b = 0; b < B; b++) max_flat = std::max(max_flat, offs[3 * (B + 1) + b + 1] - offs[3 * (B + 1) + b]);
  const int lf_first = offs[(B + 1)], n_lf = offs[(B + 1) + B] - lf_first;
  // the column tables take kOdomTabStride words per pair: keep them below 4 GB
  // The grid walk stops at the 13 x 13 column square (kOdomMaxLevel = 6: everything outside is >= 6 m away), which is
  // only exhaustive for gates below 36 m^2: a larger odom_distance_sq_threshold keeps the brute-force kernel (exact for any gate).
  const bool gate_fits_grid = h->prm.odom_distance_sq_threshold <= 35.9;
  const bool use_grid = !latency_path && max_flat > 0 && n_lf > 0 && !h->odom_force_brute && B <= 16384 && gate_fits_grid;
  int max_sharp = 0;
  for (int b = 0; b < B; b++) max_sharp = std::max(max_sharp, offs[2 * (B + 1) + b + 1] - offs[2 * (B + 1) + b]);
  const int n_ls_end = offs[B];
  const bool use_grid_e = use_grid && max_sharp > 0 && n_ls_end > offs[0];   // the same index over the (small) less-sharp clouds for the edge queries
  OdomIndex oix, oie;
  { msfl_status is = odom_index(h, h->od.planes, use_grid, B, (size_t)lf_first + (size_t)n_lf, max_flat, kOdomBlock / kOdomLanes, &oix); if (is) return is;
    is = odom_index(h, h->od.edges, use_grid_e, B, (size_t)n_ls_end, max_sharp, kOdomBlock / kOdomLanes, &oie); if (is) return is; }
  if (use_grid) {
    ScopedTimer timer(h, T_ODOM);
    int longest = 0;
    for (int b = 0; b < B; b++) longest = std::max(longest, offs[(B + 1) + b + 1] - offs[(B + 1) + b]);
    msfl_status bs = launch_odom_bin(h, st, odom_bin_job(ov.last_lf, ov.last_lf_ring, ov.last_lf_off, oix),
                                     odom_bin_job(ov.last_ls, ov.last_ls_ring, ov.last_ls_off, oie), use_grid_e ? 2 * B : B, B, longest);     // both families in one launch
    if (bs != MSFL_OK) return bs;
  }
  const msfl_status ss = solve_outer<kOdomLmBlock>(h, B, bv, nullptr, d_poses, d_status, sinks, sp, h->prm.outer_iterations, [&](int) {
    if (max_q <= 0) return MSFL_OK;
    ScopedTimer timer(h, T_ODOM);
    if (latency_path) {
      hipLaunchKernelGGL(assoc_scan2scan_wave_kernel, dim3(div_up(max_q, 4), B), dim3(256), 0, st, bv, ov,
                         (const double*)d_poses, (const int*)d_status, h->records.as<double>());
    } else {
      hipLaunchKernelGGL(assoc_scan2scan_kernel, dim3(div_up(max_q, 256), B), dim3(256), 0, st, bv, ov,
                         (const double*)d_poses, (const int*)d_status, h->records.as<double>(), oix.mode, oie.mode);
      if (use_grid) {
        const int plane_blocks = div_up(B, 8) * 8 * oix.tiles, edge_blocks = use_grid_e ? div_up(B, 8) * 8 * oie.tiles : 0;
        hipLaunchKernelGGL((assoc_scan2scan_grid_kernel<kOdomLanes>), dim3(plane_blocks + edge_blocks), dim3(kOdomBlock), 0, st, bv, ov, oix, oie,
                           plane_blocks, (const double*)d_poses, (const int*)d_status, h->records.as<double>());
      }
    }
    return MSFL_OK;
  }, max_q);
  if (ss) return ss;
  return reg_close(h, B, mem, poses_io, d_poses, status, d_status, info, sinks);
}

}  // namespace

extern "C" {

msfl_status msfl_extract_features_batch(msfl_handle* h, int n_scans, const msfl_point* pts, const uint16_t* ring,
                                        const int* off, msfl_features_batch* out, int* status, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  // the curvature kernel launches 2-D over (tile, scan): HIP caps gridDim.y at 65 535 (ADVICE r04)
  if (n_scans > 65535) return fail(h, MSFL_CAPACITY, "msfl_extract_features_batch: at most 65535 scans per call (got " + std::to_string(n_scans) + "); split the batch");
  return extract_batch_impl(h, n_scans, pts, ring, off, nullptr, out, status, mem);
}

msfl_status msfl_extract_features(msfl_handle* h, const msfl_point* pts, const uint16_t* ring, int n,
                                  const double* extrinsic_pose7, msfl_features* out, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n < 0 || !out) return fail(h, MSFL_BAD_ARG, "msfl_extract_features: bad argument");
  if (mem != MSFL_MEM_HOST) return fail(h, MSFL_BAD_ARG, "msfl_extract_features: single-scan call takes host pointers; use the batch call for device memory");
  if (n == 0) {   // CHECK_GT(_N, 0), :200
    out->n_full = out->n_sharp = out->n_less_sharp = out->n_flat = out->n_less_flat = 0;
    return fail(h, MSFL_BAD_ARG, "msfl_extract_features: empty cloud");
  }
  const int off[2] = {0, n};
  int cnt[5] = {0, 0, 0, 0, 0};
  msfl_features_batch fb;
  fb.full_pts = out->full_pts; fb.full_ring = out->full_ring; fb.curvature = out->curvature; fb.label = out->label;
  fb.sharp_idx = out->sharp_idx; fb.less_sharp_idx = out->less_sharp_idx; fb.flat_idx = out->flat_idx;
  fb.less_flat_idx = out->less_flat_idx;
  fb.n_full = &cnt[0]; fb.n_sharp = &cnt[1]; fb.n_less_sharp = &cnt[2]; fb.n_flat = &cnt[3]; fb.n_less_flat = &cnt[4];
  int st = 0;
  s = extract_batch_impl(h, 1, pts, ring, off, extrinsic_pose7, &fb, &st, MSFL_MEM_HOST);
  if (s) return s;
  out->n_full = cnt[0]; out->n_sharp = cnt[1]; out->n_less_sharp = cnt[2]; out->n_flat = cnt[3]; out->n_less_flat = cnt[4];
  if (st) return fail(h, (msfl_status)st, st == MSFL_BAD_RING ? "ring >= 128 (msf_loam_node.cc:136)" :
                                          st == MSFL_CAPACITY ? "a ring holds more than 8192 points" : "no valid point in the cloud");
  return MSFL_OK;
}

msfl_status msfl_match_scan2scan_batch(msfl_handle* h, int n_scans, const msfl_ring_cloud_batch* last_less_sharp,
                                       const msfl_ring_cloud_batch* last_less_flat, const msfl_ring_cloud_batch* curr_sharp,
                                       const msfl_ring_cloud_batch* curr_flat, double* poses_io, int* status,
                                       msfl_match_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n_scans > 65535) return fail(h, MSFL_CAPACITY, "msfl_match_scan2scan_batch: at most 65535 pairs per call (got " + std::to_string(n_scans) + "); split the batch");
  return scan2scan_batch_impl(h, n_scans, last_less_sharp, last_less_flat, curr_sharp, curr_flat, poses_io, status, info, mem);
}

msfl_status msfl_match_scan2scan(msfl_handle* h, const msfl_ring_cloud* last_less_sharp, const msfl_ring_cloud* last_less_flat,
                                 const msfl_ring_cloud* curr_sharp, const msfl_ring_cloud* curr_flat, double pose_io[7],
                                 msfl_match_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (!last_less_sharp || !last_less_flat || !curr_sharp || !curr_flat || !pose_io)
    return fail(h, MSFL_BAD_ARG, "msfl_match_scan2scan: null argument");
  const msfl_ring_cloud* c[4] = {last_less_sharp, last_less_flat, curr_sharp, curr_flat};
  int offs[4][2];
  msfl_ring_cloud_batch cb[4];
  for (int k = 0; k < 4; k++) {
    if (c[k]->n < 0) return fail(h, MSFL_BAD_ARG, "msfl_match_scan2scan: negative size");
    offs[k][0] = 0; offs[k][1] = c[k]->n;
    cb[k].pts = c[k]->pts; cb[k].ring = c[k]->ring; cb[k].off = offs[k];
  }
  int st = 0;
  int* stp = (mem == MSFL_MEM_HOST) ? &st : nullptr;
  s = scan2scan_batch_impl(h, 1, &cb[0], &cb[1], &cb[2], &cb[3], pose_io, stp, info, mem);
  if (s) return s;
  return (msfl_status)st;
}

// One cloud = a batch of one: the per-cloud LDS form (one launch + compaction) instead of a device-wide radix sort
// with its six launches and two host synchronisations (0.45 -> see profiles: the single-scan replay).
namespace {
struct FinitePoint { __device__ bool operator()(const float4& p) const { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); } };
}
msfl_status msfl_voxel_downsample(msfl_handle* h, const msfl_point* pts, int n, float leaf, msfl_point* out, int* n_out,
                                  msfl_mem mem) {
  if (!h) return MSFL_BAD_ARG;
  if (n < 0 || !n_out || !(leaf > 0.f) || (n > 0 && (!pts || !out))) { msfl_status s = enter(h); if (s) return s; return fail(h, MSFL_BAD_ARG, "msfl_voxel_downsample: bad argument"); }
  *n_out = 0;
  if (n == 0) return enter(h);
  const int off[2] = {0, n};
  int out_off[2] = {0, 0};
  msfl_status s = msfl_voxel_downsample_batch(h, 1, pts, nullptr, off, nullptr, leaf, out, out_off, mem);
  *n_out = out_off[1];
  if (s != MSFL_BAD_ARG || h->vox_nonfinite_cloud != 0) return s;
  // pcl::VoxelGrid::applyFilter skips non-finite points of a cloud that is not dense (voxel_grid.hpp: `if (!input_->is_dense)
  // if (!pcl_isfinite(x) ...) continue;`).  Rare path, entirely on the device: stable compaction of the finite points, then the
  // same filter on what is left.  (The batch forms keep refusing such a cloud: their clouds are the extraction's outputs,
  // which cannot hold one, msf_loam_node.cc:85-111.)
  // It works in the per-point passes' scratch: pp.pts takes the finite points, pp.dq the filtered ones, pp.flag their count.
  hipStream_t st = h->stream;
  const float4* d_in = h->vox_staged_pts;                                       // where the batch call left (or found) this cloud on the device
  HIPCHK(h, h->pp.pts.reserve((size_t)n * sizeof(float4)));
  HIPCHK(h, h->pp.dq.reserve((size_t)n * sizeof(float4)));
  HIPCHK(h, h->pp.flag.reserve(sizeof(unsigned int)));
  size_t tb = 0;
  HIPCHK(h, rocprim::select(nullptr, tb, d_in, h->pp.pts.as<float4>(), h->pp.flag.as<unsigned int>(), (size_t)n, FinitePoint(), st));
  HIPCHK(h, h->idx_cub.reserve(tb));
  HIPCHK(h, rocprim::select(h->idx_cub.p, tb, d_in, h->pp.pts.as<float4>(), h->pp.flag.as<unsigned int>(), (size_t)n, FinitePoint(), st));
  unsigned int m = 0;
  HIPCHK(h, hipMemcpyAsync(&m, h->pp.flag.p, sizeof(m), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  *n_out = 0;
  h->last_error.clear();
  if (m == 0) return MSFL_OK;
  const int off2[2] = {0, (int)m};
  s = msfl_voxel_downsample_batch(h, 1, reinterpret_cast<const msfl_point*>(h->pp.pts.p), nullptr, off2, nullptr, leaf,
                                  reinterpret_cast<msfl_point*>(h->pp.dq.p), out_off, MSFL_MEM_DEVICE);
  if (s) return s;
  *n_out = out_off[1];
  HIPCHK(h, hipMemcpyAsync(out, h->pp.dq.p, (size_t)out_off[1] * sizeof(float4), mem == MSFL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return MSFL_OK;
}

msfl_status msfl_voxel_downsample_batch(msfl_handle* h, int n_clouds, const msfl_point* pts, const int* idx, const int* off,
                                        const int* count, float leaf, msfl_point* out, int* out_off, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  const int B = n_clouds;
  if (B < 0 || !(leaf > 0.f) || (B > 0 && (!off || !out_off))) return fail(h, MSFL_BAD_ARG, "msfl_voxel_downsample_batch: bad argument");
  if (B == 0) return MSFL_OK;
  for (int b = 0; b < B; b++) if (off[b + 1] < off[b]) return fail(h, MSFL_BAD_ARG, "offsets must be non-decreasing");
  const int o0 = off[0];
  const int n_total = off[B] - o0;
  for (int b = 0; b <= B; b++) out_off[b] = 0;
  h->vox_nonfinite_cloud = -1; h->vox_staged_pts = nullptr;
  if (n_total == 0) return MSFL_OK;
  if (!pts || !out) return fail(h, MSFL_BAD_ARG, "msfl_voxel_downsample_batch: null cloud");
  hipStream_t st = h->stream;
  VoxelScratch& vox = h->vox;
  const int skip = mem == MSFL_MEM_HOST ? o0 : 0;       // a host batch is staged from its first used point
  std::vector<int> offs(B + 1);
  for (int b = 0; b <= B; b++) offs[b] = off[b] - skip;
  HIPCHK(h, vox.off.reserve(offs.size() * sizeof(int)));
  HIPCHK(h, h->pin.upload(vox.off.p, offs.data(), offs.size() * sizeof(int), st));
  VoxelBatchView v;
  v.off = vox.off.as<int>(); v.n_clouds = B; v.n_total = n_total; v.inv_leaf = 1.0f / leaf;
  v.idx = nullptr; v.count = nullptr;
  s = stage_in(h, vox.pts, pts + skip, (size_t)n_total, mem, st, &v.pts); if (s) return s;
  if (idx) { s = stage_in(h, vox.idx, idx + skip, (size_t)n_total, mem, st, &v.idx); if (s) return s; }
  if (count) { s = stage_in(h, vox.cnt, count, (size_t)B, mem, st, &v.count); if (s) return s; }
  h->vox_staged_pts = v.pts;
  // ---- fast form: one workgroup per cloud, runs sorted in LDS (voxel_cloud_lds_kernel) ----
  if (!h->voxel_force_global) {
    HIPCHK(h, vox.set.staging.reserve((size_t)n_total * sizeof(float4)));
    HIPCHK(h, vox.set.run_sums.reserve((size_t)n_total * sizeof(float4)));       // per-run sums (a slice has no more runs than points)
    HIPCHK(h, vox.set.tables.reserve((size_t)(3 * B + 3) * sizeof(int)));
    int* d_m = vox.set.tables.as<int>();               // [voxels per cloud B | flags B | out_off B+1]
    int* d_flags = d_m + B;
    int* d_oo = d_flags + B;
    float4* d_out = reinterpret_cast<float4*>(out);
    if (mem == MSFL_MEM_HOST) { HIPCHK(h, vox.out.reserve((size_t)n_total * sizeof(float4))); d_out = vox.out.as<float4>(); }
    // small clouds (corner lists: the point COUNT lives on the device, so the choice is made there) are served by the
    // 256-thread instantiation at six workgroups per CU; what it escalates goes to the 1024-thread one
    hipLaunchKernelGGL((voxel_cloud_lds_kernel<4, 512>), dim3(B), dim3(256), 0, st, v, vox.set.staging.as<float4>(), vox.set.run_sums.as<float4>(), d_m, d_flags, 0);
    hipLaunchKernelGGL((voxel_cloud_lds_kernel<16, 768>), dim3(B), dim3(1024), 0, st, v, vox.set.staging.as<float4>(), vox.set.run_sums.as<float4>(), d_m, d_flags, 1);
    hipLaunchKernelGGL(voxel_batch_offsets_kernel, dim3(1), dim3(1024), 0, st, (const int*)d_m, B, d_oo);
    hipLaunchKernelGGL(voxel_batch_compact_kernel, dim3(div_up(n_total, 256)), dim3(256), 0, st, (const float4*)vox.set.staging.as<float4>(),
                       (const int*)v.off, (const int*)d_oo, B, d_out);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->readback.reserve((size_t)(2 * B + 2) * sizeof(int)));
    int* rb = h->readback.as<int>();                 // [flags B | out_off B+1]
    HIPCHK(h, hipMemcpyAsync(rb, d_flags, (size_t)(2 * B + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    bool fits = true;
    for (int b = 0; b < B; b++) fits = fits && rb[b] != 4;
    if (!fits && !h->voxel_no_big) {
      // clouds the LDS forms refused (a 64-beam less-flat list is ~100 k points): the big one-workgroup form with its records in global
      // scratch, a fixed number of persistent workgroups walking the list; then the offsets / compaction again
      std::vector<int> list;
      for (int b = 0; b < B; b++) if (rb[b] == 4) list.push_back(b);
      const int n_list = (int)list.size(), grid = std::min(n_list, 512);
      HIPCHK(h, vox.big_scratch.reserve((size_t)grid * kVoxBigScratchBytes));
      HIPCHK(h, vox.big_list.reserve((size_t)n_list * sizeof(int)));
      HIPCHK(h, h->pin.upload(vox.big_list.p, list.data(), (size_t)n_list * sizeof(int), st));
      hipLaunchKernelGGL(voxel_cloud_big_kernel, dim3(grid), dim3(1024), 0, st, v, vox.set.staging.as<float4>(), vox.set.run_sums.as<float4>(), d_m, d_flags,
                         (const int*)vox.big_list.as<int>(), n_list, reinterpret_cast<unsigned long long*>(vox.big_scratch.p),
                         reinterpret_cast<unsigned short*>(vox.big_scratch.as<char>() + (size_t)grid * 65536 * 8));   // all record areas, then all order areas
      hipLaunchKernelGGL(voxel_batch_offsets_kernel, dim3(1), dim3(1024), 0, st, (const int*)d_m, B, d_oo);
      hipLaunchKernelGGL(voxel_batch_compact_kernel, dim3(div_up(n_total, 256)), dim3(256), 0, st, (const float4*)vox.set.staging.as<float4>(),
                         (const int*)v.off, (const int*)d_oo, B, d_out);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipMemcpyAsync(rb, d_flags, (size_t)(2 * B + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
      fits = true;
      for (int b = 0; b < B; b++) fits = fits && rb[b] != 4;
    }
    if (fits) {
      std::memcpy(out_off, rb + B, (size_t)(B + 1) * sizeof(int));
      if (mem == MSFL_MEM_HOST && out_off[B] > 0) {
        HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)out_off[B] * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
      }
      for (int b = 0; b < B; b++)
        if (rb[b] == 3) { h->vox_nonfinite_cloud = b; return fail(h, MSFL_BAD_ARG, "msfl_voxel_downsample_batch: non-finite point in cloud " + std::to_string(b) + " (pcl::VoxelGrid would drop it; the clouds before it are delivered)"); }
      for (int b = 0; b < B; b++)
        if (rb[b] == 1) return fail(h, MSFL_CAPACITY, "msfl_voxel_downsample_batch: leaf size too small for a cloud's extent (PCL would skip filtering)");
      return MSFL_OK;
    }
    // a cloud does not fit the LDS form (more than 65 535 points, too many runs, coordinates beyond +-8191 voxels): device-wide form
  }
  HIPCHK(h, vox.desc.reserve((size_t)B * sizeof(VoxelCloudDesc)));
  HIPCHK(h, vox.set.tables.reserve((size_t)(3 * B + 3) * sizeof(int)));
  int* d_nvalid = vox.set.tables.as<int>();          // [n_valid B | in_off B+1 | out_off B+1 | max_cells 1]
  int* d_inoff = d_nvalid + B;
  int* d_ooff = d_inoff + (B + 1);
  int* d_maxc = d_ooff + (B + 1);
  VoxelCloudDesc* d_desc = vox.desc.as<VoxelCloudDesc>();
  HIPCHK(h, hipMemsetAsync(d_ooff, 0, (size_t)(B + 2) * sizeof(int), st));       // out_off and max_cells
  hipLaunchKernelGGL(voxel_batch_desc_kernel, dim3(B), dim3(kVoxDescThreads), 0, st, v, d_desc, d_nvalid, d_maxc);
  hipLaunchKernelGGL(voxel_batch_offsets_kernel, dim3(1), dim3(1024), 0, st, (const int*)d_nvalid, B, d_inoff);
  // read-backs land in pinned memory: [head 2 ints | out_off B+1 ints | descriptors]
  HIPCHK(h, h->readback.reserve((size_t)(B + 4) * sizeof(int) + (size_t)B * sizeof(VoxelCloudDesc)));
  int* head = h->readback.as<int>();               // valid points in the batch, largest voxel count
  int* rb_off = head + 2;
  VoxelCloudDesc* hd = reinterpret_cast<VoxelCloudDesc*>(rb_off + B + 2);
  HIPCHK(h, hipMemcpyAsync(&head[0], d_inoff + B, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(&head[1], d_maxc, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(hd, d_desc, (size_t)B * sizeof(VoxelCloudDesc), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  const int nv = head[0];
  if (nv > 0) {
    // runs of consecutive same-voxel points, numbered in arrival order
    HIPCHK(h, vox.flag.reserve((size_t)nv * 2 * sizeof(int)));
    int* flag = vox.flag.as<int>(); int* pos = flag + nv;
    const dim3 grid(div_up(nv, 256)), block(256);
    hipLaunchKernelGGL(voxel_batch_head_kernel, grid, block, 0, st, v, (const VoxelCloudDesc*)d_desc, (const int*)d_inoff, nv, flag);
    size_t tb2 = 0;
    HIPCHK(h, rocprim::inclusive_scan(nullptr, tb2, flag, pos, (size_t)(nv), rocprim::plus<int>(), st));
    HIPCHK(h, h->idx_cub.reserve(tb2));
    HIPCHK(h, rocprim::inclusive_scan(h->idx_cub.p, tb2, flag, pos, (size_t)(nv), rocprim::plus<int>(), st));
    HIPCHK(h, hipMemcpyAsync(&head[0], pos + (nv - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const int nr = head[0];                                            // runs in the batch (>= 1)
    HIPCHK(h, vox.keys[0].reserve((size_t)nr * sizeof(unsigned long long)));
    HIPCHK(h, vox.keys[1].reserve((size_t)nr * sizeof(unsigned long long)));
    HIPCHK(h, vox.vals[0].reserve((size_t)nr * sizeof(unsigned)));
    HIPCHK(h, vox.vals[1].reserve((size_t)nr * sizeof(unsigned)));
    // (this form borrows the LDS form's two large buffers for its int tables: VoxelLdsSet)
    HIPCHK(h, vox.set.run_sums.reserve(((size_t)nr + 1) * sizeof(int)));       // first slot of every run
    HIPCHK(h, vox.set.staging.reserve((size_t)nr * 3 * sizeof(int)));         // voxel-head flags, their scan, head positions
    unsigned long long *k1 = vox.keys[0].as<unsigned long long>(), *k2 = vox.keys[1].as<unsigned long long>();
    unsigned *v1 = vox.vals[0].as<unsigned>(), *v2 = vox.vals[1].as<unsigned>();
    int* run_first = vox.set.run_sums.as<int>();
    int* vflag = vox.set.staging.as<int>(); int* vpos = vflag + nr; int* head_pos = vpos + nr;
    float4* d_out = reinterpret_cast<float4*>(out);
    if (mem == MSFL_MEM_HOST) { HIPCHK(h, vox.out.reserve((size_t)nr * sizeof(float4))); d_out = vox.out.as<float4>(); }
    int cell_bits = 1, cloud_bits = 1;
    while ((1ll << cell_bits) < (long long)head[1]) cell_bits++;
    while ((1ll << cloud_bits) < (long long)B) cloud_bits++;
    // the run number rides in the low bits of its key when all three fields fit 64 bits (they do up to e.g. 1 024 clouds
    // x 16 M cells x 1 G runs): a keys-only sort over the upper bits, stable, 8 bytes per run and pass
    int rid_bits = 1;
    while ((1ll << rid_bits) < (long long)nr) rid_bits++;
    if (rid_bits + cell_bits + cloud_bits > 64) rid_bits = 0;          // fall back to (key, value) pairs
    hipLaunchKernelGGL(voxel_batch_run_kernel, grid, block, 0, st, v, (const VoxelCloudDesc*)d_desc, (const int*)d_inoff, nv, (const int*)flag,
                       (const int*)pos, cell_bits, rid_bits, k1, v1, run_first);
    size_t tb = 0;
    if (rid_bits > 0) {
      HIPCHK(h, rocprim::radix_sort_keys(nullptr, tb, k1, k2, (size_t)(nr), (unsigned)(rid_bits), (unsigned)(rid_bits + cell_bits + cloud_bits), st));
      HIPCHK(h, h->idx_cub.reserve(tb));
      HIPCHK(h, rocprim::radix_sort_keys(h->idx_cub.p, tb, k1, k2, (size_t)(nr), (unsigned)(rid_bits), (unsigned)(rid_bits + cell_bits + cloud_bits), st));
    } else {
      HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb, k1, k2, v1, v2, (size_t)nr, 0u, (unsigned)(cell_bits + cloud_bits), st));
      HIPCHK(h, h->idx_cub.reserve(tb));
      HIPCHK(h, rocprim::radix_sort_pairs(h->idx_cub.p, tb, k1, k2, v1, v2, (size_t)nr, 0u, (unsigned)(cell_bits + cloud_bits), st));
    }
    const dim3 rgrid(div_up(nr, 256));
    hipLaunchKernelGGL(voxel_batch_flag_kernel, rgrid, block, 0, st, (const unsigned long long*)k2, nr, rid_bits, vflag);
    HIPCHK(h, rocprim::inclusive_scan(nullptr, tb2, vflag, vpos, (size_t)(nr), rocprim::plus<int>(), st));
    HIPCHK(h, h->idx_cub.reserve(tb2));
    HIPCHK(h, rocprim::inclusive_scan(h->idx_cub.p, tb2, vflag, vpos, (size_t)(nr), rocprim::plus<int>(), st));
    hipLaunchKernelGGL(voxel_batch_vhead_kernel, rgrid, block, 0, st, (const int*)vflag, (const int*)vpos, nr, head_pos);
    hipLaunchKernelGGL(voxel_batch_run_centroid_kernel, rgrid, block, 0, st, v, (const int*)d_inoff, (const unsigned long long*)k2, (const unsigned*)v2,
                       (const int*)run_first, (const int*)head_pos, (const int*)vpos, nr, cell_bits, rid_bits, d_out, d_ooff);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(rb_off, d_ooff, (size_t)(B + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    std::memcpy(out_off, rb_off, (size_t)(B + 1) * sizeof(int));
    if (mem == MSFL_MEM_HOST && out_off[B] > 0) {
      HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)out_off[B] * sizeof(float4), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
    }
  }
  for (int b = 0; b < B; b++)
    if (hd[b].bad == 3) { h->vox_nonfinite_cloud = b; return fail(h, MSFL_BAD_ARG, "msfl_voxel_downsample_batch: non-finite point in cloud " + std::to_string(b) + " (pcl::VoxelGrid would drop it)"); }
  for (int b = 0; b < B; b++)
    if (hd[b].bad == 1) return fail(h, MSFL_CAPACITY, "msfl_voxel_downsample_batch: leaf size too small for a cloud's extent (PCL would skip filtering)");
  return MSFL_OK;
}

msfl_status msfl_voxel_downsample_batch_pair(msfl_handle* h, int n_clouds, const msfl_point* pts, const int* off,
                                             const int* idx_a, const int* count_a, float leaf_a, msfl_point* out_a, int* out_off_a,
                                             const int* idx_b, const int* count_b, float leaf_b, msfl_point* out_b, int* out_off_b,
                                             msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  const int B = n_clouds;
  if (B < 0 || !(leaf_a > 0.f) || !(leaf_b > 0.f) || (B > 0 && (!off || !out_off_a || !out_off_b || !idx_a || !idx_b || !count_a || !count_b)))
    return fail(h, MSFL_BAD_ARG, "msfl_voxel_downsample_batch_pair: bad argument");
  const int n_total = B > 0 ? off[B] - off[0] : 0;
  // the shared-synchronisation form serves device-resident batches whose clouds fit the LDS kernels; everything else is
  // the two plain calls
  bool plain = mem != MSFL_MEM_DEVICE || h->voxel_force_global || B == 0 || n_total <= 0 || !pts || !out_a || !out_b;
  for (int b = 0; !plain && b < B; b++) if (off[b + 1] < off[b]) plain = true;
  if (!plain) {
    hipStream_t st = h->stream;
    const int* idx[2] = {idx_a, idx_b}; const int* cnt[2] = {count_a, count_b};
    const float leaf[2] = {leaf_a, leaf_b};
    msfl_point* out[2] = {out_a, out_b}; int* out_off[2] = {out_off_a, out_off_b};
    VoxelScratch& vox = h->vox;
    std::vector<int> offs(off, off + B + 1);
    HIPCHK(h, vox.off_a.reserve(offs.size() * sizeof(int)));
    HIPCHK(h, h->pin.upload(vox.off_a.p, offs.data(), offs.size() * sizeof(int), st));
    HIPCHK(h, h->readback.reserve((size_t)2 * (2 * B + 2) * sizeof(int)));
    int* rb = h->readback.as<int>();                 // per list: [flags B | out_off B+1]
    for (int k = 0; k < 2; k++) {
      VoxelBatchView v;
      v.off = vox.off_a.as<int>(); v.n_clouds = B; v.n_total = n_total; v.inv_leaf = 1.0f / leaf[k];
      v.pts = reinterpret_cast<const float4*>(pts); v.idx = idx[k]; v.count = cnt[k];
      VoxelLdsSet& set = k == 0 ? vox.set_a : vox.set;    // list b works where the single-list call does
      DevBuf &sp = set.staging, &pc = set.run_sums;
      HIPCHK(h, sp.reserve((size_t)n_total * sizeof(float4)));
      HIPCHK(h, pc.reserve((size_t)n_total * sizeof(float4)));
      HIPCHK(h, set.tables.reserve((size_t)(3 * B + 3) * sizeof(int)));
      int* d_m = set.tables.as<int>(); int* d_flags = d_m + B; int* d_oo = d_flags + B;
      hipLaunchKernelGGL((voxel_cloud_lds_kernel<4, 512>), dim3(B), dim3(256), 0, st, v, sp.as<float4>(), pc.as<float4>(), d_m, d_flags, 0);
      hipLaunchKernelGGL((voxel_cloud_lds_kernel<16, 768>), dim3(B), dim3(1024), 0, st, v, sp.as<float4>(), pc.as<float4>(), d_m, d_flags, 1);
      hipLaunchKernelGGL(voxel_batch_offsets_kernel, dim3(1), dim3(1024), 0, st, (const int*)d_m, B, d_oo);
      hipLaunchKernelGGL(voxel_batch_compact_kernel, dim3(div_up(n_total, 256)), dim3(256), 0, st, (const float4*)sp.as<float4>(),
                         (const int*)v.off, (const int*)d_oo, B, reinterpret_cast<float4*>(out[k]));
      HIPCHK(h, hipMemcpyAsync(rb + (size_t)k * (2 * B + 2), d_flags, (size_t)(2 * B + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    // both lists' [flags | out_off] leave the pinned read-back buffer BEFORE any fallback call: the plain call below
    // reuses (and may reallocate) h->readback, which used to clobber list b's not-yet-consumed tables when list a fell back
    const std::vector<int> rb_copy(rb, rb + (size_t)2 * (2 * B + 2));
    msfl_status first_error = MSFL_OK;
    for (int k = 0; k < 2; k++) {
      const int* r = rb_copy.data() + (size_t)k * (2 * B + 2);
      bool fits = true, nonfinite = false, too_small = false;
      int first_nonfinite = -1;
      for (int b = 0; b < B; b++) {
        fits = fits && r[b] != 4; too_small = too_small || r[b] == 1;
        if (r[b] == 3) { nonfinite = true; if (first_nonfinite < 0) first_nonfinite = b; }
      }
      if (!fits) {                                   // a cloud of this list needs the device-wide form: the plain call redoes the list
        const msfl_status sk = msfl_voxel_downsample_batch(h, B, pts, idx[k], off, cnt[k], leaf[k], out[k], out_off[k], mem);
        if (sk && !first_error) first_error = sk;
        continue;
      }
      std::memcpy(out_off[k], r + B, (size_t)(B + 1) * sizeof(int));
      if (nonfinite && !first_error) first_error = fail(h, MSFL_BAD_ARG, "msfl_voxel_downsample_batch_pair: non-finite point in cloud " + std::to_string(first_nonfinite) + " of list " + (k == 0 ? "a" : "b"));
      else if (too_small && !first_error) first_error = fail(h, MSFL_CAPACITY, "msfl_voxel_downsample_batch_pair: leaf size too small for a cloud's extent (PCL would skip filtering)");
    }
    return first_error;
  }
  s = msfl_voxel_downsample_batch(h, n_clouds, pts, idx_a, off, count_a, leaf_a, out_a, out_off_a, mem);
  if (s) return s;
  return msfl_voxel_downsample_batch(h, n_clouds, pts, idx_b, off, count_b, leaf_b, out_b, out_off_b, mem);
}

}  // extern "C"
