// N3 / N2: per-point passes either side of the matchers — C-ABI entry points.
// Included at the end of msfl_api.hip (shares its handle, DevBuf, PinRing and helper macros).

namespace {

// stage the pre-integration samples as [sum_dt n | dq 4n | dp 3n] doubles
msfl_status stage_preintegration(msfl_handle* h, const msfl_preintegration* pre, PreintView& pv, const char* who) {
  if (!pre || pre->n < 2 || !pre->sum_dt || !pre->delta_q || !pre->delta_p)
    return fail(h, MSFL_BAD_ARG, std::string(who) + ": a pre-integration needs at least 2 samples");
  const size_t n = (size_t)pre->n;
  for (size_t i = 1; i < n; i++)
    if (!(pre->sum_dt[i] >= pre->sum_dt[i - 1])) return fail(h, MSFL_BAD_ARG, std::string(who) + ": sum_dt must be non-decreasing");
  std::vector<double> buf(8 * n);
  std::memcpy(buf.data(), pre->sum_dt, n * sizeof(double));
  std::memcpy(buf.data() + n, pre->delta_q, 4 * n * sizeof(double));
  std::memcpy(buf.data() + 5 * n, pre->delta_p, 3 * n * sizeof(double));
  HIPCHK(h, h->pp.pre.reserve(buf.size() * sizeof(double)));
  HIPCHK(h, h->pin.upload(h->pp.pre.p, buf.data(), buf.size() * sizeof(double), h->stream));
  const double* d = h->pp.pre.as<double>();
  pv.sum_dt = d; pv.dq = d + n; pv.dp = d + 5 * n; pv.n = pre->n;
  HIPCHK(h, h->pp.flag.reserve(sizeof(int)));
  HIPCHK(h, hipMemsetAsync(h->pp.flag.p, 0, sizeof(int), h->stream));
  return MSFL_OK;
}

// in-place cloud passes: stage host points, run `launch(d_pts)`, copy back, read the range flag
template <class Launch>
msfl_status cloud_pass(msfl_handle* h, msfl_point* pts_io, int n, msfl_mem mem, bool has_flag, const char* who, Launch&& launch) {
  hipStream_t st = h->stream;
  float4* d_pts;
  msfl_status s = stage_in(h, h->pp.pts, pts_io, (size_t)n, mem, st, &d_pts); if (s) return s;
  launch(d_pts);
  HIPCHK(h, hipGetLastError());
  int bad = 0;
  if (has_flag) HIPCHK(h, hipMemcpyAsync(&bad, h->pp.flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  if (has_flag || mem == MSFL_MEM_HOST) HIPCHK(h, hipStreamSynchronize(st));
  if (bad) return fail(h, MSFL_BAD_ARG, std::string(who) + ": a point's relative time lies outside the pre-integration span (scan_undistortion.cc:26-30)");
  s = stage_out(h, pts_io, d_pts, (size_t)n, mem, st); if (s) return s;
  if (mem == MSFL_MEM_HOST) HIPCHK(h, hipStreamSynchronize(st));
  return MSFL_OK;
}

}  // namespace

extern "C" {

msfl_status msfl_delta_qp(msfl_handle* h, const msfl_preintegration* pre, const msfl_point* pts, int n, double* dq, double* dp,
                          msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n < 0 || (n > 0 && (!pts || !dq || !dp))) return fail(h, MSFL_BAD_ARG, "msfl_delta_qp: bad argument");
  PreintView pv;
  s = stage_preintegration(h, pre, pv, "msfl_delta_qp"); if (s) return s;
  if (n == 0) return MSFL_OK;
  hipStream_t st = h->stream;
  const float4* d_pts;
  s = stage_in(h, h->pp.pts, pts, (size_t)n, mem, st, &d_pts); if (s) return s;
  double *d_dq = dq, *d_dp = dp;
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(h, h->pp.dq.reserve((size_t)n * 4 * sizeof(double)));
    HIPCHK(h, h->pp.dp.reserve((size_t)n * 3 * sizeof(double)));
    d_dq = h->pp.dq.as<double>(); d_dp = h->pp.dp.as<double>();
  }
  hipLaunchKernelGGL(delta_qp_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, pv, d_pts, n, d_dq, d_dp, h->pp.flag.as<int>());
  HIPCHK(h, hipGetLastError());
  int bad = 0;
  HIPCHK(h, hipMemcpyAsync(&bad, h->pp.flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  s = stage_out(h, dq, d_dq, (size_t)n * 4, mem, st); if (s) return s;
  s = stage_out(h, dp, d_dp, (size_t)n * 3, mem, st); if (s) return s;
  HIPCHK(h, hipStreamSynchronize(st));
  if (bad) return fail(h, MSFL_BAD_ARG, "msfl_delta_qp: a point's relative time lies outside the pre-integration span (scan_undistortion.cc:26-30)");
  return MSFL_OK;
}

msfl_status msfl_deskew_cloud(msfl_handle* h, const msfl_preintegration* pre, msfl_point* pts_io, int n, const double rot_odom_xyzw[4],
                              const double velocity[3], const double gravity[3], msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n < 0 || (n > 0 && !pts_io) || !rot_odom_xyzw || !velocity || !gravity) return fail(h, MSFL_BAD_ARG, "msfl_deskew_cloud: bad argument");
  PreintView pv;
  s = stage_preintegration(h, pre, pv, "msfl_deskew_cloud"); if (s) return s;
  if (n == 0) return MSFL_OK;
  DeskewConsts c;
  c.rot_conj.x = -rot_odom_xyzw[0]; c.rot_conj.y = -rot_odom_xyzw[1]; c.rot_conj.z = -rot_odom_xyzw[2]; c.rot_conj.w = rot_odom_xyzw[3];
  c.v.x = velocity[0]; c.v.y = velocity[1]; c.v.z = velocity[2];
  c.g.x = gravity[0]; c.g.y = gravity[1]; c.g.z = gravity[2];
  return cloud_pass(h, pts_io, n, mem, true, "msfl_deskew_cloud", [&](float4* d_pts) {
    hipLaunchKernelGGL(cloud_times_check_kernel, dim3(div_up(n, 256)), dim3(256), 0, h->stream, pv, (const float4*)d_pts, n, 0, h->pp.flag.as<int>());
    hipLaunchKernelGGL(deskew_cloud_kernel, dim3(div_up(n, 256)), dim3(256), 0, h->stream, pv, c, d_pts, n, (const int*)h->pp.flag.as<int>());
  });
}

msfl_status msfl_undistort_cloud(msfl_handle* h, const msfl_preintegration* pre, msfl_point* pts_io, int n, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n < 0 || (n > 0 && !pts_io)) return fail(h, MSFL_BAD_ARG, "msfl_undistort_cloud: bad argument");
  PreintView pv;
  s = stage_preintegration(h, pre, pv, "msfl_undistort_cloud"); if (s) return s;
  if (n == 0) return MSFL_OK;
  return cloud_pass(h, pts_io, n, mem, true, "msfl_undistort_cloud", [&](float4* d_pts) {
    hipLaunchKernelGGL(cloud_times_check_kernel, dim3(div_up(n, 256)), dim3(256), 0, h->stream, pv, (const float4*)d_pts, n, 1, h->pp.flag.as<int>());
    hipLaunchKernelGGL(undistort_cloud_kernel, dim3(div_up(n, 256)), dim3(256), 0, h->stream, pv, d_pts, n, (const int*)h->pp.flag.as<int>());
  });
}

msfl_status msfl_transform_cloud(msfl_handle* h, const msfl_point* in, int n, const double pose7[7], msfl_point* out, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n < 0 || !pose7 || (n > 0 && (!in || !out))) return fail(h, MSFL_BAD_ARG, "msfl_transform_cloud: bad argument");
  if (n == 0) return MSFL_OK;
  hipStream_t st = h->stream;
  HIPCHK(h, h->pp.pre.reserve(7 * sizeof(double)));                           // (pp.pre's second role: PointPassScratch)
  HIPCHK(h, h->pin.upload(h->pp.pre.p, pose7, 7 * sizeof(double), st));      // the pose is always a host array
  const float4* d_in;
  s = stage_in(h, h->pp.pts, in, (size_t)n, mem, st, &d_in); if (s) return s;
  float4* d_out = mem == MSFL_MEM_HOST ? h->pp.pts.as<float4>() : reinterpret_cast<float4*>(out);      // a staged cloud is transformed in place
  hipLaunchKernelGGL(transform_cloud_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, d_in, n, (const double*)h->pp.pre.as<double>(), d_out);
  HIPCHK(h, hipGetLastError());
  s = stage_out(h, out, d_out, (size_t)n, mem, st); if (s) return s;
  if (mem == MSFL_MEM_HOST) HIPCHK(h, hipStreamSynchronize(st));
  return MSFL_OK;
}

}  // extern "C"
