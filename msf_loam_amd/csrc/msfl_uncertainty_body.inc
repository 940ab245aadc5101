// Body of uncertainty_kernel (MSFL_UNC_PRIOR 0) and uncertainty_prior_kernel (MSFL_UNC_PRIOR 1), included once in each
// (msfl_uncertainty.cuh).  A textual include for the reason given in msfl_lm_solve_body.inc: the feature-off kernel stays token for
// token what it was.  With MSFL_UNC_PRIOR the solve had a pose prior (msfl_set_pose_prior): `information` is the posterior one, lidar
// J^T J + Jp^T Jp through the solve's own prior_accumulate, and n_residuals counts its six rows.  In scope: BLOCK, bv, pprime_all,
// rec_all, poses, status, info, outer_it, huber, min_correspondences, min_eigenvalue, out and, with MSFL_UNC_PRIOR, prior_all.
  static_assert(BLOCK >= 64, "36 lanes assemble the matrices");
  __shared__ LmShared<BLOCK> sh;
  __shared__ PlaneCache<BLOCK> s_cache;
  __shared__ EdgeList s_edges;
  __shared__ UncRecord s_out;
  const int b = blockIdx.x;
#if MSFL_UNC_PRIOR
  __shared__ PosePrior s_prior;
  int use_prior;
  {
    int bad;                                   // a non-finite record was refused by the solve: status[b] != 0 below
    prior_stage<BLOCK>(prior_all + b, s_prior, bad, use_prior);
  }
#endif
  unsigned long long* s_words = reinterpret_cast<unsigned long long*>(&s_out);
  for (int i = threadIdx.x; i < kUncWords; i += BLOCK) s_words[i] = 0ull;
  if (threadIdx.x < kEdgeListMax / 32) s_edges.mask[threadIdx.x] = 0;      // the first-pass form of evaluate_pass marks its edges here
  __syncthreads();
  bool valid = false;
  if (status[b] == 0) {                                                     // uniform over the workgroup
    const int nc = bv.corner_off[b + 1] - bv.corner_off[b];
    const int ns = bv.surf_off[b + 1] - bv.surf_off[b];
    const float4* corner = bv.corner + bv.corner_off[b];
    const float4* surf = bv.surf + bv.surf_off[b];
    const double* rec = rec_all + edge_rec_off(bv, bv.corner_off[b]);
    const double* recp = rec_all;
    const size_t g0 = plane_slot(bv, bv.surf_off[b]);
    const double* pprime = pprime_all ? pprime_all + 3 * (size_t)bv.rec_off[b] : nullptr;
    double acc[kAcc];
    int ne, np;
    const pose7 T = load_pose(poses + 7 * (size_t)b);
    evaluate_pass<BLOCK, true>(T, huber, corner, nc, surf, ns, pprime, rec, recp, g0, s_cache, s_edges, acc, ne, np);
    block_reduce<BLOCK>(sh, acc, ne, np);
#if MSFL_UNC_PRIOR
    if (use_prior && threadIdx.x == 0) prior_accumulate(T, &s_prior, sh.red);
#endif
    __syncthreads();
    const int n_edge = sh.cnt[0], n_plane = sh.cnt[1];
    valid = (n_edge + n_plane >= min_correspondences) && (n_edge + n_plane > 0);   // exactly when lm_solve_kernel solves
    if (valid) {
      if (threadIdx.x < 36) {
        const int i = threadIdx.x / 6, j = threadIdx.x % 6;
        const int p = min(i, j), q = max(i, j);
        s_out.information[threadIdx.x] = sh.red[7 + 6 * p - (p * (p - 1)) / 2 + (q - p)];
      }
      if (threadIdx.x == 0) {
        double a[6][6], v[6][6], g[6];
        unpack_system(sh.red, a, g);
        sym_eigen6_jacobi(a, v);
        double lmax = a[0][0];
#pragma unroll
        for (int k = 1; k < 6; k++) lmax = fmax(lmax, a[k][k]);
        const double thr = fmax(min_eigenvalue, 1e-14 * lmax);
        int n_deg = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
          // ascending position of eigenpair k (stable), then the sign convention: the largest-magnitude component
          // (lowest index on ties) is positive
          int rank = 0;
#pragma unroll
          for (int j = 0; j < 6; j++) rank += (a[j][j] < a[k][k] || (a[j][j] == a[k][k] && j < k)) ? 1 : 0;
          double big = fabs(v[0][k]), sgn = v[0][k] < 0.0 ? -1.0 : 1.0;
#pragma unroll
          for (int i = 1; i < 6; i++)
            if (fabs(v[i][k]) > big) { big = fabs(v[i][k]); sgn = v[i][k] < 0.0 ? -1.0 : 1.0; }
          s_out.eigenvalues[rank] = a[k][k];
#pragma unroll
          for (int i = 0; i < 6; i++) s_out.eigenvectors[6 * rank + i] = sgn * v[i][k];
          n_deg += a[k][k] < thr ? 1 : 0;
        }
#if MSFL_UNC_PRIOR
        const int n_res = 3 * n_edge + n_plane + (use_prior ? 6 : 0);
#else
        const int n_res = 3 * n_edge + n_plane;
#endif
        s_out.n_residuals = n_res;
        s_out.n_degenerate = n_deg;
        s_out.valid = 1;
        s_out.sigma2 = n_res > 6 ? 2.0 * (info ? info[b].final_cost[outer_it] : sh.red[0]) / (double)(n_res - 6) : 0.0;
      }
    }
  }
  __syncthreads();
  if (valid && threadIdx.x < 36) {
    // covariance = sum over the kept eigenpairs, ascending: the n_degenerate smallest are the dropped ones
    const int i = threadIdx.x / 6, j = threadIdx.x % 6;
    double c = 0.0;
    for (int k = s_out.n_degenerate; k < 6; k++) c += s_out.eigenvectors[6 * k + i] * s_out.eigenvectors[6 * k + j] / s_out.eigenvalues[k];
    s_out.covariance[threadIdx.x] = c;
  }
  __syncthreads();
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(out + b);
  for (int i = threadIdx.x; i < kUncWords; i += BLOCK) dst[i] = s_words[i];
