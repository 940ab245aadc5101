"""Numpy model of the pose graph with a loss per factor (docs/kernels/graph.md, "A loss per factor"): the four factor kinds of
tests/graph_info_numpy.py, each factor under a LossFunction of its own as Ceres gives every residual block one.

TEST INFRASTRUCTURE.  Written from the definition in docs/kernels/graph.md and the Ceres documentation of LossFunction / Corrector, not
from the kernels.  graph_info_numpy, graph_numpy and ceres_numpy are imported, not edited, and nothing of them is patched: the losses
travel with the problem and are handed to every evaluation explicitly.

With s = |r|^2, a > 0, b = a^2 (every rho' clamped from below at DBL_MIN):

    DEFAULT        the options' huber_delta (no loss when it is 0)
    NONE           rho = s                                  rho' = 1
    HUBER          rho = s if s <= b, else 2 a sqrt(s) - b  rho' = 1, else a / sqrt(s)
    SOFT_L_ONE     rho = 2 b (sqrt(1 + s/b) - 1)            rho' = 1 / sqrt(1 + s/b)
    CAUCHY         rho = b log(1 + s/b)                     rho' = 1 / (1 + s/b)
    GEMAN_MCCLURE  rho = b s / (b + s)                      rho' = (b / (b + s))^2

All have rho'' <= 0, so the corrector scales residual and Jacobian rows by sqrt(rho') and the cost is rho / 2.  A problem is
graph_info_numpy's dict plus, per factor kind, the loss kinds and parameters: elk ela (E,), flk fla (F,), glk gla (G,), hlk hla (H,).
"""
import numpy as np

try:
    from tests import ceres_numpy as cn
    from tests import graph_info_numpy as gi
    from tests import graph_numpy as gn
except ImportError:                        # run as a script from tests/golden
    import ceres_numpy as cn
    import graph_info_numpy as gi
    import graph_numpy as gn

Options = gi.Options
DEFAULT, NONE, HUBER, SOFT_L_ONE, CAUCHY, GEMAN_MCCLURE = range(6)
NAMES = ("default", "none", "huber", "soft_l_one", "cauchy", "geman_mcclure")
LOSS_KEYS = (("elk", "ela"), ("flk", "fla"), ("glk", "gla"), ("hlk", "hla"))       # per factor kind, in the factor numbering
KEYS = gi.KEYS + tuple(k for pair in LOSS_KEYS for k in pair)


class NoLoss(Options):
    huber_delta = 0.0


def with_losses(prob):
    """A graph_info_numpy problem with every factor at DEFAULT."""
    out = {k: np.array(v) for k, v in prob.items()}
    for (lk, la), (ia, _) in zip(LOSS_KEYS, gi.KINDS):
        out[lk] = np.zeros(len(out[ia]), np.int32)
        out[la] = np.zeros(len(out[ia]))
    return out


def set_losses(prob, factor_kind, kind, a=0.0, first=0, n=None):
    """msfl_graph_set_losses on the model: factors first .. first + n of one factor kind get `kind` / `a` (scalars or n values)."""
    lk, la = LOSS_KEYS[factor_kind]
    n = len(prob[lk]) - first if n is None else n
    prob[lk][first:first + n] = kind
    prob[la][first:first + n] = np.where(np.broadcast_to(np.asarray(kind), (n,)) >= HUBER, a, 0.0)


def rho(s, kind, a, huber_delta=Options.huber_delta):
    """rho(s), rho'(s) per element; s, kind and a broadcast against each other."""
    s, kind, a = np.broadcast_arrays(np.asarray(s, np.float64), np.asarray(kind), np.asarray(a, np.float64))
    kind, a = kind.copy(), a.copy()
    dflt = kind == DEFAULT
    kind[dflt] = HUBER if huber_delta > 0.0 else NONE
    a[dflt] = huber_delta
    a = np.where(kind >= HUBER, a, 1.0)                     # NONE reads no a
    b = a * a
    out, w = s.copy(), np.ones_like(s)
    m = (kind == HUBER) & (s > b)
    n = np.sqrt(np.where(m, s, 1.0))
    out = np.where(m, 2.0 * a * n - b, out); w = np.where(m, a / n, w)
    m = kind == SOFT_L_ONE
    t = np.sqrt(1.0 + s / b)
    out = np.where(m, 2.0 * b * (t - 1.0), out); w = np.where(m, 1.0 / t, w)
    m = kind == CAUCHY
    q = 1.0 + s / b
    out = np.where(m, b * np.log(q), out); w = np.where(m, 1.0 / q, w)
    m = kind == GEMAN_MCCLURE
    q = b / (b + s)
    out = np.where(m, q * s, out); w = np.where(m, q * q, w)
    return out, np.maximum(cn.DBL_MIN, w)


def blocks(prob, x, opt, want_jacobian=True):
    """cost, and per kind (rows, Ji, Jj) after each factor's own corrector, in the factor numbering."""
    _, raw = gi.blocks(prob, x, NoLoss, want_jacobian)     # no loss: every scale is exactly 1
    cost, out = 0.0, []
    for (r, Ji, Jj), (lk, la) in zip(raw, LOSS_KEYS):
        val, w = rho((r * r).sum(-1), prob[lk], prob[la], opt.huber_delta)
        s = np.sqrt(w)
        cost += 0.5 * float(val.sum())
        if want_jacobian:
            Ji = Ji * s[:, None, None]; Jj = Jj * s[:, None, None]
        out.append((r * s[:, None], Ji, Jj))
    return cost, out


def cost(prob, x=None, opt=Options):
    return blocks(prob, prob["poses"] if x is None else x, opt, False)[0]


def weights(prob, x, opt=Options):
    """rho'(|r|^2) per factor and kind at poses x."""
    return [rho(c, prob[lk], prob[la], opt.huber_delta)[1] for c, (lk, la) in zip(gi.chi2(prob, x), LOSS_KEYS)]


def evaluate_sparse(prob, x, opt, want_jacobian=True):
    import scipy.sparse as sp
    c, blk = blocks(prob, x, opt, want_jacobian)
    r, rows, cols, vals, m = gi._triplets(prob, blk)
    _, nf = gn.free_index(prob["fixed"])
    return c, r, (sp.csr_matrix((vals, (rows, cols)), shape=(m, 6 * nf)) if want_jacobian else None)


def dense_fns(prob):
    free = ~np.asarray(prob["fixed"], bool)
    nf = int(free.sum())

    def full(xf):
        x = np.array(prob["poses"], np.float64)
        x[free] = xf.reshape(-1, 7)
        return x

    def evaluate_fn(_, xf, opt):
        c, blk = blocks(prob, full(xf), opt, True)
        r, rows, cols, vals, m = gi._triplets(prob, blk)
        J = np.zeros((m, 6 * nf))
        np.add.at(J, (rows, cols), vals)
        return c, r, J

    def plus_fn(xf, delta):
        return gn.plus_poses(xf.reshape(-1, 7), np.asarray(delta).reshape(-1, 6)).ravel()

    return evaluate_fn, plus_fn, np.array(prob["poses"], np.float64)[free].ravel(), 6 * nf, full


def solve_dense(prob, opt=Options):
    free = ~np.asarray(prob["fixed"], bool)
    if not free.any() or gi.n_factors(prob) == 0:
        tr = cn.Trace(); tr.termination = "empty"
        return np.array(prob["poses"], np.float64), tr
    ev, pl, x0, nt, full = dense_fns(prob)
    xf, tr = cn.solve(None, x0, opt, evaluate_fn=ev, plus_fn=pl, n_tangent=nt)
    return full(xf), tr


def solve_sparse(prob, opt=Options, permc_spec="COLAMD"):
    """graph_info_numpy.solve_sparse line by line, over this module's evaluate_sparse."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    free = ~np.asarray(prob["fixed"], bool)
    tr = cn.Trace()
    X = np.array(prob["poses"], np.float64)
    if not free.any() or gi.n_factors(prob) == 0:
        tr.termination = "empty"
        return X, tr
    nt = 6 * int(free.sum())

    def plus(X, delta):
        Y = X.copy()
        Y[free] = gn.plus_poses(X[free], delta.reshape(-1, 6))
        return Y

    def gmax_of(X, g):
        return np.max(np.abs(X[free] - plus(X, -g)[free]))

    cost_, r, J = evaluate_sparse(prob, X, opt)
    tr.initial_cost = tr.final_cost = cost_
    scale = 1.0 / (1.0 + np.sqrt(np.asarray(J.multiply(J).sum(0)).ravel())) if opt.jacobi_scaling else np.ones(nt)
    g = J.T @ r
    Js = J @ sp.diags(scale)
    x_norm = np.sqrt((X[free] ** 2).sum())
    gmax = gmax_of(X, g)
    if gmax <= opt.gradient_tolerance:
        tr.termination = "gradient"
        return X, tr
    radius, decrease_factor, reuse_diagonal, diagonal = opt.initial_trust_region_radius, 2.0, False, None
    invalid, step_successful = 0, True
    while True:
        if tr.iterations >= opt.max_num_iterations:
            tr.termination = "max_iterations"; break
        if step_successful and gmax <= opt.gradient_tolerance:
            tr.termination = "gradient"; break
        if radius < opt.min_trust_region_radius:
            tr.termination = "min_radius"; break
        tr.iterations += 1
        if not reuse_diagonal:
            diagonal = np.clip(np.asarray(Js.multiply(Js).sum(0)).ravel(), opt.min_lm_diagonal, opt.max_lm_diagonal)
        reuse_diagonal = True
        H = (Js.T @ Js + sp.diags(diagonal / radius)).tocsc()
        step = spl.splu(H, permc_spec=permc_spec).solve(-(Js.T @ r))
        valid = bool(np.all(np.isfinite(step)))
        used_radius = radius
        model_cost_change = 0.0
        if valid:
            m = Js @ step
            model_cost_change = -float(m @ (r + 0.5 * m))
            valid = model_cost_change > 0.0
        if not valid:
            invalid += 1
            tr.cost.append(cost_); tr.radius.append(used_radius); tr.rel_decrease.append(0.0); tr.step_norm.append(0.0); tr.accepted.append(-1)
            if invalid >= opt.max_num_consecutive_invalid_steps:
                tr.termination = "invalid_steps"; break
            radius *= 0.5
            step_successful = False
            continue
        invalid = 0
        cand = plus(X, step * scale)
        cand_cost, cand_r, cand_J = evaluate_sparse(prob, cand, opt)
        step_norm = float(np.sqrt(((X - cand)[free] ** 2).sum()))
        if step_norm <= opt.parameter_tolerance * (x_norm + opt.parameter_tolerance):
            tr.cost.append(cand_cost); tr.radius.append(used_radius); tr.rel_decrease.append(0.0); tr.step_norm.append(step_norm); tr.accepted.append(0)
            tr.termination = "parameter"; break
        cost_change = cost_ - cand_cost
        if abs(cost_change) <= opt.function_tolerance * cost_:
            tr.cost.append(cand_cost); tr.radius.append(used_radius); tr.rel_decrease.append(0.0); tr.step_norm.append(step_norm); tr.accepted.append(0)
            tr.termination = "function"; break
        rel = cost_change / model_cost_change
        ok = rel > opt.min_relative_decrease
        tr.cost.append(cand_cost); tr.radius.append(used_radius); tr.rel_decrease.append(rel); tr.step_norm.append(step_norm); tr.accepted.append(int(ok))
        if ok:
            X, cost_, r, J = cand, cand_cost, cand_r, cand_J
            Js = J @ sp.diags(scale)
            g = J.T @ r
            x_norm = np.sqrt((X[free] ** 2).sum())
            gmax = gmax_of(X, g)
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3), opt.max_trust_region_radius)
            decrease_factor, reuse_diagonal, step_successful = 2.0, False, True
            tr.successful_steps += 1
            tr.final_cost = cost_
        else:
            radius /= decrease_factor
            decrease_factor *= 2.0
            reuse_diagonal, step_successful = True, False
    return X, tr


# ---- the seeded cases of tests/test_gpu_graph_loss.py ---------------------------------------------------------------------------
CASES = ("v_gm", "four", "mixed")
WRONG_CLOSURE = 2                                          # of case (v)'s four
MIXED_SEED = 36


def without_closure(prob, k):
    """The same problem with information edge k removed (the model's reference for "the wrong closure removed by hand")."""
    out = {key: np.array(v) for key, v in prob.items()}
    for key in ("gi", "gj", "gz", "gL", "glk", "gla"):
        if key in out:
            out[key] = np.delete(out[key], k, axis=0)
    return out


def mixed(seed=MIXED_SEED):
    """130 nodes like graph_info_numpy's (iii), the six loss kinds alternating factor by factor through the whole factor numbering, so
    that neighbouring lanes take different branches.  The start poses are the odometry's with a pose noise of 3 cm / 3 mrad on top: the
    chain residuals then spread over 1e-2 .. 1e2 in |r|^2, and a = 0.5 * (1 + (k mod 4)) leaves factors of every loss kind on each
    side of s = b (make_graph_loss_golden.py asserts it)."""
    prob = with_losses(gi.make_case("iii"))
    rng = np.random.default_rng(seed)
    n = len(prob["poses"])
    noise = np.concatenate([rng.normal(0.0, 0.03, (n, 3)), gn._small_rot(rng, n, 0.003)], -1)
    prob["poses"] = gn.pose_mul(prob["poses"], noise)
    k = 0
    for lk, la in LOSS_KEYS:
        for q in range(len(prob[lk])):
            prob[lk][q] = k % 6
            prob[la][q] = 0.5 * (1 + (k // 6) % 4) if k % 6 >= HUBER else 0.0
            k += 1
    return prob


def make_case(name):
    if name == "v_gm":                                     # case (v), its four closures under Geman-McClure a = 1
        prob = with_losses(gi.make_case("v"))
        set_losses(prob, 2, GEMAN_MCCLURE, 1.0)
        return prob
    if name == "four":                                     # 3 nodes, one factor of each kind, each under a different loss
        truth, odo, poses, rng = gn.drive(3, 37)
        prob = gi.problem(poses)
        gn.add_edges(prob, 0, 1, odo[0])
        gn._gps(prob, truth, rng, [0])
        gi.add_edges_info(prob, 1, 2, odo[1], gi.draw_L(rng, 1))
        gi._gps_info(prob, truth, rng, [1], [gi._gps_cov(rng, [0.01, 0.015, 0.05])])
        prob = with_losses(prob)
        for fk, (kind, a) in enumerate(((CAUCHY, 0.7), (SOFT_L_ONE, 1.5), (GEMAN_MCCLURE, 2.0), (HUBER, 0.5))):
            set_losses(prob, fk, kind, a)
        return prob
    if name == "mixed":
        return mixed()
    raise KeyError(name)
