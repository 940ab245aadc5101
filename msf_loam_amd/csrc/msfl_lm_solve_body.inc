// Body of lm_solve_kernel (MSFL_LM_PRIOR 0), lm_solve_prior_kernel (MSFL_LM_PRIOR 1), both in msfl_kernels.cuh, and
// lm_solve_degen_kernel (MSFL_LM_DEGEN 1, msfl_degeneracy.cuh), included once in each.
// A textual include, not a shared device function: the feature-off kernel is then token for token the kernel it was before the
// pose prior existed, so its code object cannot move (docs/kernels/prior.md).  In scope: BLOCK, bv, pprime_all, rec_all, poses,
// status, info, outer_it, prm and, with MSFL_LM_PRIOR, prior_all.  With MSFL_LM_DEGEN: prior_all (may be null: the prior lines sit
// behind a run-time check, there is no sibling for "prior + degeneracy"), degen_min_eig and degen_out (may be null).
  __shared__ LmShared<BLOCK> sh;
  __shared__ PlaneCache<BLOCK> s_cache;
  __shared__ EdgeList s_edges;
#if MSFL_LM_PRIOR
  __shared__ PosePrior s_prior;
#endif
#if MSFL_LM_DEGEN
  __shared__ PosePrior s_prior;
  __shared__ DegenState s_degen;
#endif
  const int b = blockIdx.x;
  if (status[b] != 0) return;
  if (threadIdx.x < kEdgeListMax / 32) s_edges.mask[threadIdx.x] = 0;
#if MSFL_LM_PRIOR
  int use_prior;
  {
    int bad;
    prior_stage<BLOCK>(prior_all + b, s_prior, bad, use_prior);
    if (bad) {                                 // uniform: a non-finite prior is refused, the pose passes through
      if (threadIdx.x == 0) { status[b] = 3; if (info) info[b].status = 3; }   // MSFL_BAD_ARG
      return;
    }
  }
#endif
#if MSFL_LM_DEGEN
  int use_prior = 0;
  if (prior_all) {                             // uniform (a kernel argument)
    int bad;
    prior_stage<BLOCK>(prior_all + b, s_prior, bad, use_prior);
    if (bad) {
      if (threadIdx.x == 0) { status[b] = 3; if (info) info[b].status = 3; }   // MSFL_BAD_ARG
      return;
    }
  }
#endif
  __syncthreads();
  const int nc = bv.corner_off[b + 1] - bv.corner_off[b];
  const int ns = bv.surf_off[b + 1] - bv.surf_off[b];
  const float4* corner = bv.corner + bv.corner_off[b];
  const float4* surf = bv.surf + bv.surf_off[b];
  const size_t r0 = (size_t)bv.rec_off[b];
  const double* rec = rec_all + edge_rec_off(bv, bv.corner_off[b]);
  const double* recp = rec_all;
  const size_t g0 = plane_slot(bv, bv.surf_off[b]);
  const double* pprime = pprime_all ? pprime_all + 3 * r0 : nullptr;
  double* pose_g = poses + 7 * (size_t)b;
  TrState& tr = sh.tr;
  // trust-region functions inlined (msfl_kernels.cuh, lm_tr_propose): the plain 128-thread kernel only
  [[maybe_unused]] constexpr bool kTrInline = MSFL_LM_TR_INLINE && !MSFL_LM_PRIOR && !MSFL_LM_DEGEN && BLOCK < 512;
  LM_T(t_begin);
  {
    double acc[kAcc];
    int ne, np;
    const pose7 T = load_pose(pose_g);
    LM_T(t0);
    evaluate_pass<BLOCK, true>(T, prm.huber, corner, nc, surf, ns, pprime, rec, recp, g0, s_cache, s_edges, acc, ne, np);
    LM_T(t1);
    block_reduce<BLOCK>(sh, acc, ne, np);
    LM_T(t2);
    LM_ADD(0, t1 - t0); LM_ADD(1, t2 - t1); LM_ADD(4, 1);
  }
  LM_T(t_s0);
  // mask -> index list (32 lanes of wavefront 0, one mask word each; ascending index order, so the list and with it the
  // summation order of the later passes is a function of the records alone)
  if (threadIdx.x < kEdgeListMax / 32) {
    unsigned m = s_edges.mask[threadIdx.x];
    const int c = __popc(m);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) { const int v = __shfl_up(incl, o); if ((int)threadIdx.x >= o) incl += v; }
    int at = incl - c;
    while (m) { const int bit = __ffs((int)m) - 1; s_edges.idx[at++] = (unsigned short)(32 * threadIdx.x + bit); m &= m - 1; }
    if (threadIdx.x == kEdgeListMax / 32 - 1) s_edges.n = incl;
  }
  if (threadIdx.x == 0) {
    const int n_edge = sh.cnt[0], n_plane = sh.cnt[1];
    int go = 1;
    if (info) { info[b].n_edge[outer_it] = n_edge; info[b].n_plane[outer_it] = n_plane; }
    tr.cost = 0.0; tr.iteration = 0; tr.successful = 0;
    if (n_edge + n_plane < prm.min_correspondences) {
      status[b] = 1;                       // MSFL_TOO_FEW_CORRESPONDENCES (odometry_scan_matcher.cc:262-267)
      if (info) info[b].status = 1;
      go = 0;
    } else if (n_edge + n_plane == 0) {
      go = 0;                              // Ceres: empty problem, parameters untouched
    } else {
#if MSFL_LM_PRIOR
      if (use_prior) prior_accumulate(load_pose(pose_g), &s_prior, sh.red);
#endif
#if MSFL_LM_DEGEN
      if (use_prior) prior_accumulate(load_pose(pose_g), &s_prior, sh.red);
      // H0 of this solve: lidar rows + prior block.  Decomposed once; V_k is fixed for the solve, as the Jacobi scaling is.
      const int n_held = degen_decompose(sh.red, degen_min_eig, s_degen);
      if (degen_out) degen_write_record(s_degen, degen_out + b, outer_it);
      if (n_held > 0 && n_held < 6) degen_rotate(s_degen, sh.red);
#endif
#pragma unroll
      for (int k = 0; k < kAcc; k++) tr.sys[k] = sh.red[k];
#pragma unroll
      for (int i = 0; i < 7; i++) tr.x[i] = pose_g[i];
      tr.cost = sh.red[0];
      if (info) info[b].initial_cost[outer_it] = tr.cost;
      // jacobi_scaling from iteration 0: 1 / (1 + sqrt(diag(J^T J)))
      const int dg[6] = {7, 13, 18, 22, 25, 27};   // packed positions of H[i][i]
#pragma unroll
      for (int i = 0; i < 6; i++) tr.scale[i] = 1.0 / (1.0 + sqrt(sh.red[dg[i]]));
      const pose7 x = load_pose(tr.x);
#if MSFL_LM_DEGEN
      tr.gmax = n_held > 0 && n_held < 6 ? degen_gradient_max_norm(s_degen, tr.x, tr.sys + 1, prm.gtol)
                                         : gradient_max_norm_for_test(x, tr.sys + 1, prm.gtol);
#else
      tr.gmax = gradient_max_norm_for_test(x, tr.sys + 1, prm.gtol);
#endif
      tr.x_norm = pose_norm(x);
      tr.radius = prm.radius0; tr.decrease_factor = 2.0; tr.model_cost_change = 0.0;
      tr.invalid = 0; tr.reuse_diagonal = 0; tr.step_ok = 1;
#if MSFL_LM_DEGEN
      if (n_held == 6) go = 0;             // nothing observable: no step, the pose passes through, counts stay 0
      else go = n_held > 0 ? tr_propose_degen(tr, prm, s_degen) : tr_propose(tr, prm);
#else
      go = lm_tr_propose<kTrInline>(tr, prm);
#endif
    }
    sh.go = go;
  }
  __syncthreads();
  LM_T(t_s1);
  LM_ADD(2, t_s1 - t_s0);
  bool solved = (sh.cnt[0] + sh.cnt[1] >= prm.min_correspondences) && (sh.cnt[0] + sh.cnt[1] > 0);
  while (sh.go) {
    double acc[kAcc];
    int ne, np;
    const pose7 T = load_pose(tr.cand);   // lane 0 overwrites go / cand only after the reduction's barrier, which every
                                           // thread reaches after this read: no barrier of its own needed
    LM_T(t0);
    evaluate_pass<BLOCK, false>(T, prm.huber, corner, nc, surf, ns, pprime, rec, recp, g0, s_cache, s_edges, acc, ne, np);
    LM_T(t1);
    block_reduce<BLOCK>(sh, acc, ne, np);
    LM_T(t2);
#if MSFL_LM_PRIOR
    if (use_prior && threadIdx.x == 0) prior_accumulate(load_pose(tr.cand), &s_prior, sh.red);
#endif
#if MSFL_LM_DEGEN
    if (threadIdx.x == 0) {
      if (use_prior) prior_accumulate(load_pose(tr.cand), &s_prior, sh.red);
      if (s_degen.n_held > 0) {              // 0 < n_held < 6 here: the all-held solve never enters the loop
        degen_rotate(s_degen, sh.red);
        const int accepted = tr.successful;
        int cont = tr_decide(tr, sh.red, prm);
        // tr_decide took the gradient max norm of an accepted step in the pose tangent; the reduced problem's replaces it
        if (cont && tr.successful != accepted) tr.gmax = degen_gradient_max_norm(s_degen, tr.x, tr.sys + 1, prm.gtol);
        sh.go = cont ? tr_propose_degen(tr, prm, s_degen) : 0;
      } else {
        sh.go = tr_decide(tr, sh.red, prm) ? tr_propose(tr, prm) : 0;
      }
    }
#elif defined(MSFL_LM_PROFILE)
    if (threadIdx.x == 0) {
      const unsigned long long c0 = wall_clock64();
      const int cont = tr_decide(tr, sh.red, prm);
      const unsigned long long c1 = wall_clock64();
      sh.go = cont ? tr_propose(tr, prm) : 0;
      const unsigned long long c2 = wall_clock64();
      atomicAdd(&g_lm_prof[6], c1 - c0); atomicAdd(&g_lm_prof[7], c2 - c1);
    }
#else
    if (threadIdx.x == 0) sh.go = lm_tr_decide<kTrInline>(tr, sh.red, prm) ? lm_tr_propose<kTrInline>(tr, prm) : 0;
#endif
    __syncthreads();
    LM_T(t3);
    LM_ADD(0, t1 - t0); LM_ADD(1, t2 - t1); LM_ADD(2, t3 - t2); LM_ADD(4, 1);
  }
  LM_T(t_end);
  LM_ADD(3, t_end - t_begin); LM_ADD(5, 1);
  if (threadIdx.x == 0) {
    if (solved) {
#pragma unroll
      for (int i = 0; i < 7; i++) pose_g[i] = tr.x[i];
    }
    if (info) {
      info[b].lm_iterations[outer_it] = tr.iteration;
      info[b].lm_successful[outer_it] = tr.successful;
      info[b].final_cost[outer_it] = tr.cost;
    }
  }
