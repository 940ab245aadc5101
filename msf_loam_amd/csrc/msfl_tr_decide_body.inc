// Body of tr_decide and tr_decide_inline (msfl_kernels.cuh), included once in each: a textual include for the reason given in
// msfl_lm_solve_body.inc -- the call form stays token for token what it was.  In scope: tr, red, prm.
  const double cand_cost = red[0];
  const double cost_change = tr.cost - cand_cost;
  if (fabs(cost_change) <= prm.ftol * tr.cost) return 0;
  const double rel = cost_change / tr.model_cost_change;
  if (rel > prm.min_relative_decrease) {
#pragma unroll
    for (int i = 0; i < 7; i++) tr.x[i] = tr.cand[i];
#pragma unroll
    for (int k = 0; k < kAcc; k++) tr.sys[k] = red[k];
    const pose7 x = load_pose(tr.x);
    tr.x_norm = pose_norm(x);
    tr.cost = cand_cost;
    tr.gmax = gradient_max_norm_for_test(x, tr.sys + 1, prm.gtol);
    const double t = 2.0 * rel - 1.0;
    tr.radius = fmin(tr.radius / fmax(1.0 / 3.0, 1.0 - t * t * t), prm.radius_max);
    tr.decrease_factor = 2.0;
    tr.reuse_diagonal = 0;
    tr.step_ok = 1;
    tr.successful++;
  } else {
    tr.radius = tr.radius / tr.decrease_factor;
    tr.decrease_factor *= 2.0;
    tr.reuse_diagonal = 1;
    tr.step_ok = 0;
  }
  return 1;
