// Body of tr_propose (MSFL_TR_DEGEN 0, msfl_kernels.cuh) and tr_propose_degen (MSFL_TR_DEGEN 1, msfl_degeneracy.cuh), included once in
// each.  A textual include for the reason given in msfl_lm_solve_body.inc: tr_propose stays token for token what it was.  With
// MSFL_TR_DEGEN the system in tr.sys is the one degen_rotate left (eigenbasis of H0, held coordinates decoupled), and the step goes
// back to the pose tangent through degen_map_step.  In scope: tr, prm and, with MSFL_TR_DEGEN, dg.
  for (;;) {
    if (tr.iteration >= prm.max_iterations) return 0;
    if (tr.step_ok && tr.gmax <= prm.gtol) return 0;
    if (tr.radius < prm.radius_min) return 0;
    tr.iteration++;
    // A = S H S (+ LM damping); its Cholesky factor goes to L, A itself stays readable for the model cost change.
    double A[6][6], gs[6], y[6], lm2[6];
    {
      int n = 7;
#pragma unroll
      for (int p = 0; p < 6; p++)
#pragma unroll
        for (int q = p; q < 6; q++) { const double v = tr.sys[n++] * tr.scale[p] * tr.scale[q]; A[p][q] = v; A[q][p] = v; }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) gs[i] = tr.sys[1 + i] * tr.scale[i];
    if (!tr.reuse_diagonal) {
#pragma unroll
      for (int i = 0; i < 6; i++) tr.diagonal[i] = fmin(fmax(A[i][i], prm.min_diag), prm.max_diag);
    }
    double hs_diag[6];                     // undamped diagonal of S H S, for the model cost change below
    // Ceres' LM strategy appends sqrt(diagonal / radius) as extra Jacobian rows, i.e. adds diagonal / radius to the
    // normal equations: formed directly here (one division for all six), equal up to the rounding of sqrt(.)^2
    const double inv_radius = 1.0 / tr.radius;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      lm2[i] = tr.diagonal[i] * inv_radius;
      hs_diag[i] = A[i][i];
      A[i][i] += lm2[i];
    }
    // factorise, solve, then step^T Hs step from the very values A was formed from (off-diagonal entries of A and the
    // diagonal saved before damping): no second pass over the packed system in LDS.  The factor is kept as
    // L[i][j] (i > j) and the RECIPROCALS of its diagonal: one reciprocal square root per column instead of a
    // square root and 2 x (5 - j) + 2 divisions (this serial, single-lane chain is latency bound: ~200 clocks each)
    double L[6][6], dinv[6];
    bool ok = true;
#pragma unroll
    for (int jc = 0; jc < 6; jc++) {
      double s = A[jc][jc];
#pragma unroll
      for (int k = 0; k < jc; k++) s = __builtin_fma(-L[jc][k], L[jc][k], s);
      if (!(s > 0.0)) ok = false;
      dinv[jc] = fast_rsqrt(s);
#pragma unroll
      for (int i = jc + 1; i < 6; i++) {
        double v = A[i][jc];
#pragma unroll
        for (int k = 0; k < jc; k++) v = __builtin_fma(-L[i][k], L[jc][k], v);
        L[i][jc] = v * dinv[jc];
      }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
      double s = gs[i];
#pragma unroll
      for (int k = 0; k < i; k++) s = __builtin_fma(-L[i][k], y[k], s);
      y[i] = s * dinv[i];
    }
    double step[6];
#pragma unroll
    for (int i = 5; i >= 0; i--) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < 6; k++) s = __builtin_fma(-L[k][i], step[k], s);
      step[i] = s * dinv[i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) { if (!isfinite(step[i])) ok = false; step[i] = -step[i]; }
    tr.reuse_diagonal = 1;
    double mcc = 0.0;
    if (ok) {
      double gts = 0.0, shs = 0.0;
#pragma unroll
      for (int i = 0; i < 6; i++) {
        gts += gs[i] * step[i];
#pragma unroll
        for (int j = 0; j < 6; j++) {
          // Hs[i][j]: the value A was formed from (A itself off the diagonal, the saved entry on it)
          shs += step[i] * (i == j ? hs_diag[i] : A[i][j]) * step[j];
        }
      }
      mcc = -gts - 0.5 * shs;
    }
    tr.model_cost_change = mcc;
    if (!ok || !(mcc > 0.0)) {          // HandleInvalidStep
      if (++tr.invalid >= prm.max_invalid) return 0;
      tr.radius *= 0.5;
      tr.step_ok = 0;
      continue;
    }
    tr.invalid = 0;
    const pose7 x = load_pose(tr.x);
#if MSFL_TR_DEGEN
#pragma unroll
    for (int i = 0; i < 6; i++) dg.y[i] = step[i] * tr.scale[i];
    degen_map_step(dg);                  // dg.d = V_k y: no component along a held eigenvector
    const pose7 cand = pose_plus(x, mk3(dg.d[0], dg.d[1], dg.d[2]), mk3(dg.d[3], dg.d[4], dg.d[5]));
#else
    const pose7 cand = pose_plus(x, mk3(step[0] * tr.scale[0], step[1] * tr.scale[1], step[2] * tr.scale[2]),
                                 mk3(step[3] * tr.scale[3], step[4] * tr.scale[4], step[5] * tr.scale[5]));
#endif
    store_pose(tr.cand, cand);
    double sn = 0.0;
#pragma unroll
    for (int i = 0; i < 7; i++) { const double d = tr.x[i] - tr.cand[i]; sn += d * d; }
    sn = sqrt(sn);
    if (sn <= prm.ptol * (tr.x_norm + prm.ptol)) return 0;   // ParameterToleranceReached
    return 1;
  }
