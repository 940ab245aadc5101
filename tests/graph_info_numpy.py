"""Numpy model of the pose graph with information-weighted factors (docs/kernels/graph.md): the two kinds of tests/graph_numpy.py
plus the two that carry a full square-root information matrix L.

TEST INFRASTRUCTURE.  Written from the definition in docs/kernels/graph.md and docs/kernels/prior.md (the residual of the pose prior,
applied to the relative pose), not from the kernels.  graph_numpy and ceres_numpy are imported, not edited.

    information edge {i, j, z, L (6 x 6)}:  qe = conj(z.q) (x) conj(q_i) (x) q_j, negated when qe.w < 0
                                            e = [R_i^T (t_j - t_i) - z.t ; 2 vec(qe)],  r = L e            (6 rows)
    information fix {i, j, t, p, L3}:       r = L3 ((1 - t) t_i + t t_j - p)                               (3 rows)

Factors are numbered edges, fixes, information edges, information fixes.  A problem is graph_numpy's dict plus
gi gj (G,), gz (G, 7), gL (G, 6, 6) and hi hj (H,), ht (H,), hp (H, 3), hL (H, 3, 3).  The dense solve is ceres_numpy.solve over the
four-kind Jacobian; the sparse one is the loop of graph_numpy.solve_sparse restated over it.
"""
import numpy as np

try:
    from tests import ceres_numpy as cn
    from tests import graph_numpy as gn
except ImportError:                        # run as a script from tests/golden
    import ceres_numpy as cn
    import graph_numpy as gn

Options = gn.Options
INFO_KEYS = ("gi", "gj", "gz", "gL", "hi", "hj", "ht", "hp", "hL")
KEYS = ("poses", "fixed", "ei", "ej", "ez", "esr", "est", "fi", "fj", "ft", "fp", "fst") + INFO_KEYS
KINDS = (("ei", "ej"), ("fi", "fj"), ("gi", "gj"), ("hi", "hj"))


def problem(poses, fixed=None):
    prob = gn.problem(poses, fixed)
    prob.update(gi=np.zeros(0, np.int32), gj=np.zeros(0, np.int32), gz=np.zeros((0, 7)), gL=np.zeros((0, 6, 6)),
                hi=np.zeros(0, np.int32), hj=np.zeros(0, np.int32), ht=np.zeros(0), hp=np.zeros((0, 3)), hL=np.zeros((0, 3, 3)))
    return prob


def with_info(prob):
    """A graph_numpy problem as a four-kind one (no information factor yet)."""
    out = problem(prob["poses"], prob["fixed"])
    out.update({k: np.array(v) for k, v in prob.items()})
    return out


def add_edges_info(prob, i, j, z, L):
    i, j = np.atleast_1d(i).astype(np.int32), np.atleast_1d(j).astype(np.int32)
    prob["gi"] = np.concatenate([prob["gi"], i]); prob["gj"] = np.concatenate([prob["gj"], j])
    prob["gz"] = np.concatenate([prob["gz"], np.asarray(z, np.float64).reshape(-1, 7)])
    prob["gL"] = np.concatenate([prob["gL"], np.asarray(L, np.float64).reshape(-1, 6, 6)])


def add_fixes_info(prob, i, j, t, p, L3):
    i, j = np.atleast_1d(i).astype(np.int32), np.atleast_1d(j).astype(np.int32)
    prob["hi"] = np.concatenate([prob["hi"], i]); prob["hj"] = np.concatenate([prob["hj"], j])
    prob["ht"] = np.concatenate([prob["ht"], np.atleast_1d(t).astype(np.float64)])
    prob["hp"] = np.concatenate([prob["hp"], np.asarray(p, np.float64).reshape(-1, 3)])
    prob["hL"] = np.concatenate([prob["hL"], np.asarray(L3, np.float64).reshape(-1, 3, 3)])


def isotropic_L(sr, st, n=1):
    """The L under which an information edge costs what the plain edge {sr, st} costs."""
    sr, st = np.broadcast_to(np.asarray(sr, float), (n,)), np.broadcast_to(np.asarray(st, float), (n,))
    L = np.zeros((n, 6, 6))
    for c in range(3):
        L[:, c, c] = 1.0 / st
        L[:, 3 + c, 3 + c] = 1.0 / (2.0 * sr)
    return L


def edges_as_info(prob):
    """The same graph with every plain edge rewritten as an information edge (in front of the ones it already has)."""
    out = with_info(prob) if "gi" not in prob else {k: np.array(v) for k, v in prob.items()}
    n = len(out["ei"])
    keep = {k: out[k] for k in ("gi", "gj", "gz", "gL")}
    out["gi"], out["gj"], out["gz"], out["gL"] = out["ei"].astype(np.int32), out["ej"].astype(np.int32), out["ez"], isotropic_L(out["esr"], out["est"], n)
    for k in ("gi", "gj", "gz", "gL"):
        out[k] = np.concatenate([out[k], keep[k]])
    out["ei"], out["ej"], out["ez"], out["esr"], out["est"] = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)), np.zeros(0), np.zeros(0)
    return out


def fix_from_covariance(cov):
    """The upper Cholesky factor of cov^-1."""
    return np.linalg.cholesky(np.linalg.inv(np.asarray(cov, np.float64))).T


def edge_from_uncertainty(pose_i, pose_j, H, n_degenerate, scale):
    """z and L^T L (not L: its rows carry the eigenvectors' signs) of the edge a registration with information H about pose_j gives."""
    lam, V = np.linalg.eigh(np.asarray(H, np.float64))
    Hk = (V[:, n_degenerate:] * lam[n_degenerate:]) @ V[:, n_degenerate:].T
    D = np.eye(6); D[:3, :3] = gn.quat_to_R(np.asarray(pose_i, np.float64)[3:])
    return gn.relative_pose(pose_i, pose_j), D.T @ Hk @ D / scale


def n_long(prob):
    fr, _ = gn.free_index(prob["fixed"])
    k = 0
    for a, b in KINDS:
        fa, fb = fr[np.asarray(prob[a], int)], fr[np.asarray(prob[b], int)]
        k += int(((fa >= 0) & (fb >= 0) & (np.abs(fa - fb) > 1)).sum())
    return k


def info_errors(prob, x, want_jacobian=True):
    """e (G, 6) of the information edges and de/d(dt_i, d_i), de/d(dt_j, d_j) (G, 6, 6) in the graph's tangent (left perturbation)."""
    gi, gj = np.asarray(prob["gi"], int), np.asarray(prob["gj"], int)
    ti, qi, tj, qj = x[gi, :3], x[gi, 3:], x[gj, :3], x[gj, 3:]
    tz, qz = prob["gz"][:, :3], prob["gz"][:, 3:]
    u = tj - ti
    A = gn.qmul(gn.qconj(qz), gn.qconj(qi))
    qe = gn.qmul(A, qj)
    s = np.where(qe[:, 3:] < 0.0, -1.0, 1.0)
    e = np.concatenate([gn.qrot(gn.qconj(qi), u) - tz, 2.0 * s * qe[:, :3]], -1)
    if not want_jacobian:
        return e, None, None
    G = len(gi)
    RiT = np.swapaxes(gn.quat_to_R(qi), -1, -2)
    M = np.empty((G, 3, 3))
    for c in range(3):
        ec = np.zeros((G, 4)); ec[:, c] = 1.0
        M[:, :, c] = 2.0 * s * gn.qmul(gn.qmul(A, ec), qj)[:, :3]
    Di = np.zeros((G, 6, 6)); Dj = np.zeros((G, 6, 6))
    Di[:, :3, :3] = -RiT; Di[:, :3, 3:] = 2.0 * RiT @ gn.skew(u); Di[:, 3:, 3:] = -M
    Dj[:, :3, :3] = RiT; Dj[:, 3:, 3:] = M
    return e, Di, Dj


def raw_residuals(prob, x):
    """Per kind the residual rows before the corrector: (E, 6), (F, 3), (G, 6), (H, 3)."""
    class NoLoss(Options):
        huber_delta = 0.0
    _, blk = gn.blocks(prob, x, NoLoss, False)
    e, _, _ = info_errors(prob, x, False)
    hi, hj = np.asarray(prob["hi"], int), np.asarray(prob["hj"], int)
    t = prob["ht"][:, None]
    eh = (1.0 - t) * x[hi, :3] + t * x[hj, :3] - prob["hp"]
    return [blk[0][0], blk[1][0], np.einsum("nij,nj->ni", prob["gL"], e), np.einsum("nij,nj->ni", prob["hL"], eh)]


def chi2(prob, x):
    """|r|^2 per factor and kind, before the loss."""
    return [(r * r).sum(-1) for r in raw_residuals(prob, x)]


def blocks(prob, x, opt, want_jacobian=True):
    """cost, and per kind (rows, Ji, Jj) after the corrector, in the factor numbering."""
    cost, out = gn.blocks(prob, x, opt, want_jacobian)
    e, Di, Dj = info_errors(prob, x, want_jacobian)
    L = prob["gL"]
    r = np.einsum("nij,nj->ni", L, e)
    rho, s = gn._huber_scale((r * r).sum(-1), opt.huber_delta)
    cost += 0.5 * float(rho.sum())
    Ji = Jj = None
    if want_jacobian:
        Ji = (L @ Di) * s[:, None, None]; Jj = (L @ Dj) * s[:, None, None]
    out.append((r * s[:, None], Ji, Jj))
    hi, hj = np.asarray(prob["hi"], int), np.asarray(prob["hj"], int)
    t = prob["ht"][:, None]
    L3 = prob["hL"]
    r = np.einsum("nij,nj->ni", L3, (1.0 - t) * x[hi, :3] + t * x[hj, :3] - prob["hp"])
    rho, s = gn._huber_scale((r * r).sum(-1), opt.huber_delta)
    cost += 0.5 * float(rho.sum())
    Ji = Jj = None
    if want_jacobian:
        H = len(hi)
        Ji = np.zeros((H, 3, 6)); Jj = np.zeros((H, 3, 6))
        Ji[:, :, :3] = (1.0 - t)[:, :, None] * L3; Jj[:, :, :3] = t[:, :, None] * L3
        Ji *= s[:, None, None]; Jj *= s[:, None, None]
    out.append((r * s[:, None], Ji, Jj))
    return cost, out


def cost(prob, x=None, opt=Options):
    return blocks(prob, prob["poses"] if x is None else x, opt, False)[0]


def _triplets(prob, blk):
    """COO triplets of the stacked Jacobian over the free nodes' tangent, rows in the factor numbering."""
    fr, _ = gn.free_index(prob["fixed"])
    rows, cols, vals, res = [], [], [], []
    row0 = 0
    for (r, Ji, Jj), (ia, ja) in zip(blk, KINDS):
        n, m = r.shape
        res.append(r.ravel())
        if Ji is not None and n:
            rr = row0 + (np.arange(n)[:, None, None] * m + np.arange(m)[None, :, None])
            for J, idx in ((Ji, prob[ia]), (Jj, prob[ja])):
                f = fr[np.asarray(idx, int)]
                keep = f >= 0
                cc = f[:, None, None] * 6 + np.arange(6)[None, None, :]
                rows.append(np.broadcast_to(rr, J.shape)[keep].ravel())
                cols.append(np.broadcast_to(cc, J.shape)[keep].ravel())
                vals.append(J[keep].ravel())
        row0 += n * m
    cat = lambda a, dt: np.concatenate(a) if a else np.zeros(0, dt)
    return np.concatenate(res), cat(rows, int), cat(cols, int), cat(vals, float), row0


def evaluate_sparse(prob, x, opt, want_jacobian=True):
    import scipy.sparse as sp
    c, blk = blocks(prob, x, opt, want_jacobian)
    r, rows, cols, vals, m = _triplets(prob, blk)
    _, nf = gn.free_index(prob["fixed"])
    return c, r, (sp.csr_matrix((vals, (rows, cols)), shape=(m, 6 * nf)) if want_jacobian else None)


def n_factors(prob):
    return sum(len(prob[a]) for a, _ in KINDS)


def dense_fns(prob):
    free = ~np.asarray(prob["fixed"], bool)
    nf = int(free.sum())

    def full(xf):
        x = np.array(prob["poses"], np.float64)
        x[free] = xf.reshape(-1, 7)
        return x

    def evaluate_fn(_, xf, opt):
        c, blk = blocks(prob, full(xf), opt, True)
        r, rows, cols, vals, m = _triplets(prob, blk)
        J = np.zeros((m, 6 * nf))
        np.add.at(J, (rows, cols), vals)
        return c, r, J

    def plus_fn(xf, delta):
        return gn.plus_poses(xf.reshape(-1, 7), np.asarray(delta).reshape(-1, 6)).ravel()

    return evaluate_fn, plus_fn, np.array(prob["poses"], np.float64)[free].ravel(), 6 * nf, full


def solve_dense(prob, opt=Options):
    free = ~np.asarray(prob["fixed"], bool)
    if not free.any() or n_factors(prob) == 0:
        tr = cn.Trace(); tr.termination = "empty"
        return np.array(prob["poses"], np.float64), tr
    ev, pl, x0, nt, full = dense_fns(prob)
    xf, tr = cn.solve(None, x0, opt, evaluate_fn=ev, plus_fn=pl, n_tangent=nt)
    return full(xf), tr


def solve_sparse(prob, opt=Options, permc_spec="COLAMD"):
    """graph_numpy.solve_sparse line by line, over the four-kind Jacobian."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    free = ~np.asarray(prob["fixed"], bool)
    tr = cn.Trace()
    X = np.array(prob["poses"], np.float64)
    if not free.any() or n_factors(prob) == 0:
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


def ate(poses, truth):
    return float(np.sqrt(np.mean(np.sum((np.asarray(poses)[:, :3] - np.asarray(truth)[:, :3]) ** 2, axis=1))))


# ---- the seeded cases of tests/test_gpu_graph_info.py ---------------------------------------------------------------------
def random_rotation(rng):
    q = rng.normal(0.0, 1.0, 4)
    return gn.quat_to_R(q / np.linalg.norm(q))


def draw_L(rng, n, rank=6):
    """diag(1 / sigma_t x 3, 1 / sigma_r x 3) blockdiag(Q, Q): sigma_t in 0.05 .. 0.2 m, sigma_r in 5 .. 20 mrad, Q a random rotation;
    a lower rank zeroes the leading rows."""
    L = np.zeros((n, 6, 6))
    for k in range(n):
        Q = random_rotation(rng)
        B = np.zeros((6, 6)); B[:3, :3] = Q; B[3:, 3:] = Q
        L[k] = np.diag(np.r_[np.full(3, 1.0 / rng.uniform(0.05, 0.2)), np.full(3, 1.0 / rng.uniform(0.005, 0.02))]) @ B
        L[k, :6 - rank] = 0.0
    return L


def _closure_z(truth, rng, i, j):
    return gn.pose_mul(gn.relative_pose(truth[i], truth[j])[None], np.concatenate([rng.normal(0, 0.01, (1, 3)), gn._small_rot(rng, 1, 0.001)], -1))[0]


def _gps_info(prob, truth, rng, at, covs):
    at = np.asarray(at, int)
    t = rng.uniform(0.1, 0.9, len(at))
    for k, cov in zip(range(len(at)), covs):
        noise = np.linalg.cholesky(cov) @ rng.normal(0.0, 1.0, 3)
        p = (1 - t[k]) * truth[at[k], :3] + t[k] * truth[at[k] + 1, :3] + noise
        add_fixes_info(prob, at[k], at[k] + 1, t[k], p, fix_from_covariance(cov))


def _gps_cov(rng, sigmas):
    Q = random_rotation(rng)
    return Q @ np.diag(np.square(sigmas)) @ Q.T


CLOSURES_D = [(0, 113), (3, 117), (7, 120), (10, 125), (15, 129), (40, 90), (55, 70), (1, 128)]      # graph_numpy's case (d)
CORRIDOR_PAIRS = [(2, 37), (5, 34), (8, 31)]
CORRIDOR_FORMS = ("plain", "isotropic", "rank5")
CASES = ("i", "ii", "iii", "v") + tuple("iv_" + f for f in CORRIDOR_FORMS)
SEEDS = dict(i=31, ii=32, iii=33, iv=34, v=35)


def corridor(form, seed=SEEDS["iv"]):
    """An out-and-back drive of 40 poses down a corridor along x (1 m steps, turned round at the far end), node 0 fixed, odometry noise
    2 cm / 4 mrad per step, and three closures whose measurement slid 2 m along the corridor axis: what a registration that is blind
    along the axis can deliver.  form: None (odometry only), "plain" (the existing edge at sr = 0.005, st = 0.05), "isotropic" (the
    same as an information edge, diag(20 x 3, 100 x 3)), "rank5" (the row of the corridor axis zeroed).  Returns (problem, truth)."""
    rng = np.random.default_rng(seed)
    n = 40
    truth = np.zeros((n, 7))
    for k in range(n):
        out = k < n // 2
        yaw = 0.0 if out else np.pi
        truth[k] = [k if out else n - 1 - k, 0.0 if out else 0.3, 0.0, 0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw)]
    rel = gn.relative_pose(truth[:-1], truth[1:])
    odo = gn.pose_mul(rel, np.concatenate([rng.normal(0.0, 0.02, (n - 1, 3)), gn._small_rot(rng, n - 1, 0.004)], -1))
    poses = np.empty((n, 7)); poses[0] = truth[0]
    for k in range(n - 1):
        poses[k + 1] = gn.pose_mul(poses[k], odo[k])
    fixed = np.zeros(n, bool); fixed[0] = True
    prob = problem(poses, fixed)
    gn._chain(prob, odo)
    for i, j in CORRIDOR_PAIRS:
        z = _closure_z(truth, rng, i, j)
        axis = gn.quat_to_R(truth[i, 3:]).T @ np.array([1.0, 0.0, 0.0])      # the corridor axis in the frame of node i, where z.t lives
        z[:3] += 2.0 * axis
        if form == "plain":
            gn.add_edges(prob, i, j, z, sr=0.005, st=0.05)
        elif form in ("isotropic", "rank5"):
            L = isotropic_L(0.005, 0.05)[0]
            if form == "rank5":
                b = np.cross(axis, [0.0, 0.0, 1.0]); b /= np.linalg.norm(b)
                Q = np.stack([axis, b, np.cross(axis, b)])
                L[:3, :3] = L[:3, :3] @ Q
                L[0] = 0.0
            add_edges_info(prob, i, j, z, L)
    return prob, truth


def make_case(name):
    """The parity shapes (i) .. (v) of tests/test_gpu_graph_info.py; the corridor (iv) comes in three forms, "iv_<form>"."""
    if name.startswith("iv_"):
        return corridor(name[3:])[0]
    n = dict(i=3, ii=37, iii=130, v=80)[name]
    truth, odo, poses, rng = gn.drive(n, SEEDS[name])
    fixed = np.zeros(n, bool)
    if name in ("ii", "v"):
        fixed[0] = True
    prob = problem(poses, fixed)
    if name == "i":                                      # information factors only, no fixed node
        add_edges_info(prob, [0, 1], [1, 2], odo, draw_L(rng, 2))
        _gps_info(prob, truth, rng, [0, 1], [_gps_cov(rng, [0.01, 0.015, 0.05]), _gps_cov(rng, [0.02, 0.008, 0.04])])
    elif name == "ii":
        gn._chain(prob, odo)
        for (i, j), rank in zip([(2, 33), (10, 36)], (6, 5)):
            add_edges_info(prob, i, j, _closure_z(truth, rng, i, j), draw_L(rng, 1, rank))
    elif name == "iii":
        k = np.arange(n - 1)
        even, odd = k[k % 2 == 0], k[k % 2 == 1]
        gn.add_edges(prob, even, even + 1, odo[even])
        add_edges_info(prob, odd, odd + 1, odo[odd], draw_L(rng, len(odd)))
        for c, (i, j) in enumerate(CLOSURES_D):
            z = _closure_z(truth, rng, i, j)
            if c < 4:
                gn.add_edges(prob, i, j, z)
            else:
                add_edges_info(prob, i, j, z, draw_L(rng, 1, 4 if c in (5, 6) else 6))
        gn._gps(prob, truth, rng, [0, 40])
        _gps_info(prob, truth, rng, [85, 128], [_gps_cov(rng, [0.01, 0.01, 0.04]), _gps_cov(rng, [0.015, 0.02, 0.06])])
    elif name == "v":                                    # one closure 5 m wrong
        gn._chain(prob, odo)
        for c, (i, j) in enumerate([(3, 70), (5, 75), (20, 60), (10, 79)]):
            z = _closure_z(truth, rng, i, j)
            if c == 2:
                z[0] += 5.0
            add_edges_info(prob, i, j, z, draw_L(rng, 1))
    return prob
