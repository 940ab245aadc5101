"""Numpy model of the pose-graph problem of msfl_graph_* (docs/kernels/graph.md), the reference's GpsFusion::Optimize
(gps_fusion.cc:27-97) with loop-closure edges on top.

TEST INFRASTRUCTURE.  Written from gps_factor.h (the two residuals), the Ceres 1.14 documentation (HuberLoss / Corrector,
EigenQuaternionParameterization, TrustRegionMinimizer) and tests/ceres_numpy.py, not from the kernels.

    relative-pose edge {i, j, z, sr, st}:  E = (T_i^-1 T_j)^-1 Z,  r = [E.t / st ; vec(E.q) / sr]      (6 rows)
    position fix {i, j, t, p, st}:         r = ((1 - t) t_i + t t_j - p) / st                           (3 rows)
    manifold per free node:                t + dt,  q <- dq (x) q,  dq = [sin|d| d/|d| ; cos|d|]        (tangent [dt ; d])

Two step solvers run the same trust-region loop:
    dense  : ceres_numpy.solve itself (lstsq on the augmented system [Js; D] s = [-r; 0]) through evaluate_fn / plus_fn;
    sparse : solve_sparse below, the loop of ceres_numpy.solve restated line by line over a scipy.sparse Jacobian with the
             step from a sparse LU of the normal equations (Js^T Js + D^2) s = -Js^T r.
A problem is a dict of arrays: poses (N, 7) [t, qx qy qz qw], fixed (N,) bool, ei ej (E,), ez (E, 7), esr est (E,),
fi fj (F,), ft (F,), fp (F, 3), fst (F,).
"""
import numpy as np

try:
    from tests import ceres_numpy as cn
except ImportError:                        # run as a script from tests/golden
    import ceres_numpy as cn


class Options(cn.Options):
    max_num_iterations = 10                # gps_fusion.cc:45
    huber_delta = 1.0                      # gps_fusion.cc:48; 0 = no loss


# ---- quaternions [x, y, z, w], batched over the leading axis -----------------------------------
def qmul(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdims=True)], -1)


def qconj(a):
    return np.concatenate([-a[..., :3], a[..., 3:]], -1)


def qrot(q, v):
    """Eigen's unit-quaternion q * v: v + 2 w (u x v) + 2 u x (u x v)."""
    u, w = q[..., :3], q[..., 3:]
    uv = np.cross(u, v)
    return v + 2.0 * (w * uv + np.cross(u, uv))


def quat_to_R(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def skew(v):
    S = np.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1] = -v[..., 2]; S[..., 0, 2] = v[..., 1]
    S[..., 1, 0] = v[..., 2]; S[..., 1, 2] = -v[..., 0]
    S[..., 2, 0] = -v[..., 1]; S[..., 2, 1] = v[..., 0]
    return S


def pose_mul(a, b):
    return np.concatenate([a[..., :3] + qrot(a[..., 3:], b[..., :3]), qmul(a[..., 3:], b[..., 3:])], -1)


def pose_inv(a):
    qi = qconj(a[..., 3:])
    return np.concatenate([-qrot(qi, a[..., :3]), qi], -1)


def relative_pose(Ti, Tj):
    """T_i^-1 T_j: the measurement an edge (i, j) carries when both poses are right."""
    return pose_mul(pose_inv(np.asarray(Ti, np.float64)), np.asarray(Tj, np.float64))


def plus_poses(x, delta):
    """(n, 7) poses, (n, 6) tangent steps: EigenQuaternionParameterization::Plus on the rotation, t + dt on the translation."""
    d = delta[:, 3:6]
    n = np.sqrt((d * d).sum(-1, keepdims=True))
    safe = np.where(n > 0.0, n, 1.0)
    dq = np.concatenate([np.sin(n) / safe * d, np.cos(n)], -1)
    q = np.where(n > 0.0, qmul(dq, x[:, 3:]), x[:, 3:])
    return np.concatenate([x[:, :3] + delta[:, :3], q], -1)


def free_index(fixed):
    fixed = np.asarray(fixed, bool)
    idx = np.cumsum(~fixed) - 1
    return np.where(fixed, -1, idx), int((~fixed).sum())


def n_long(prob):
    """Factors whose two ends are both free and more than one apart in the free numbering."""
    fr, _ = free_index(prob["fixed"])
    k = 0
    for a, b in ((prob["ei"], prob["ej"]), (prob["fi"], prob["fj"])):
        fa, fb = fr[np.asarray(a, int)], fr[np.asarray(b, int)]
        k += int(((fa >= 0) & (fb >= 0) & (np.abs(fa - fb) > 1)).sum())
    return k


def _huber_scale(sq, delta):
    """rho(s), sqrt(rho'(s)) per block; the rho'' <= 0 corrector scales residual and Jacobian by sqrt(rho')."""
    if delta <= 0.0:
        return sq, np.ones_like(sq)
    b = delta * delta
    r = np.sqrt(np.where(sq > b, sq, 1.0))
    rho1 = np.where(sq > b, np.maximum(cn.DBL_MIN, delta / r), 1.0)
    return np.where(sq > b, 2 * delta * r - b, sq), np.sqrt(rho1)


def blocks(prob, x, opt, want_jacobian=True):
    """cost, and per factor kind (rows, Ji, Jj) after the corrector: edges (E, 6), (E, 6, 6) x 2; fixes (F, 3), (F, 3, 6) x 2."""
    ei, ej, fi, fj = (np.asarray(prob[k], int) for k in ("ei", "ej", "fi", "fj"))
    cost = 0.0
    out = []
    # relative-pose edges
    ti, qi, tj, qj = x[ei, :3], x[ei, 3:], x[ej, :3], x[ej, 3:]
    tz, qz = prob["ez"][:, :3], prob["ez"][:, 3:]
    st, sr = prob["est"][:, None], prob["esr"][:, None]
    a = qrot(qi, tz)
    v = a + ti - tj
    A, B = qconj(qj), qmul(qi, qz)
    r = np.concatenate([qrot(A, v) / st, qmul(A, B)[:, :3] / sr], -1)
    rho, s = _huber_scale((r * r).sum(-1), opt.huber_delta)
    cost += 0.5 * float(rho.sum())
    Ji = Jj = None
    if want_jacobian:
        E = len(ei)
        RjT = np.swapaxes(quat_to_R(qj), -1, -2)
        M = np.empty((E, 3, 3))
        for k in range(3):
            e = np.zeros((E, 4)); e[:, k] = 1.0
            M[:, :, k] = qmul(qmul(A, e), B)[:, :3]
        Ji = np.zeros((E, 6, 6)); Jj = np.zeros((E, 6, 6))
        Ji[:, :3, :3] = RjT / st[:, :, None]
        Ji[:, :3, 3:] = RjT @ (-2.0 * skew(a)) / st[:, :, None]
        Jj[:, :3, :3] = -RjT / st[:, :, None]
        Jj[:, :3, 3:] = RjT @ (2.0 * skew(v)) / st[:, :, None]
        Ji[:, 3:, 3:] = M / sr[:, :, None]
        Jj[:, 3:, 3:] = -M / sr[:, :, None]
        Ji *= s[:, None, None]; Jj *= s[:, None, None]
    out.append((r * s[:, None], Ji, Jj))
    # position fixes
    t, st = prob["ft"][:, None], prob["fst"][:, None]
    r = ((1.0 - t) * x[fi, :3] + t * x[fj, :3] - prob["fp"]) / st
    rho, s = _huber_scale((r * r).sum(-1), opt.huber_delta)
    cost += 0.5 * float(rho.sum())
    if want_jacobian:
        F = len(fi)
        Ji = np.zeros((F, 3, 6)); Jj = np.zeros((F, 3, 6))
        for k in range(3):
            Ji[:, k, k] = ((1.0 - t) / st)[:, 0]
            Jj[:, k, k] = (t / st)[:, 0]
        Ji *= s[:, None, None]; Jj *= s[:, None, None]
    out.append((r * s[:, None], Ji, Jj))
    return cost, out


def cost(prob, x=None, opt=Options):
    return blocks(prob, prob["poses"] if x is None else x, opt, False)[0]


def _triplets(prob, blk):
    """COO triplets of the stacked Jacobian over the free nodes' tangent, rows = edges then fixes."""
    fr, _ = free_index(prob["fixed"])
    rows, cols, vals, res = [], [], [], []
    row0 = 0
    for (r, Ji, Jj), (ia, ja) in zip(blk, ((prob["ei"], prob["ej"]), (prob["fi"], prob["fj"]))):
        n, m = r.shape
        res.append(r.ravel())
        if Ji is not None and n:
            rr = row0 + (np.arange(n)[:, None, None] * m + np.arange(m)[None, :, None])
            for J, idx in ((Ji, ia), (Jj, ja)):
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
    _, nf = free_index(prob["fixed"])
    return c, r, (sp.csr_matrix((vals, (rows, cols)), shape=(m, 6 * nf)) if want_jacobian else None)


def dense_fns(prob):
    """evaluate_fn / plus_fn / x0 / n_tangent for ceres_numpy.solve: x is the stacked 7-vectors of the free nodes."""
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
        return plus_poses(xf.reshape(-1, 7), np.asarray(delta).reshape(-1, 6)).ravel()

    return evaluate_fn, plus_fn, np.array(prob["poses"], np.float64)[free].ravel(), 6 * nf, full


def solve_dense(prob, opt=Options):
    free = ~np.asarray(prob["fixed"], bool)
    if not free.any() or len(prob["ei"]) + len(prob["fi"]) == 0:
        tr = cn.Trace(); tr.termination = "empty"
        return np.array(prob["poses"], np.float64), tr
    ev, pl, x0, nt, full = dense_fns(prob)
    xf, tr = cn.solve(None, x0, opt, evaluate_fn=ev, plus_fn=pl, n_tangent=nt)
    return full(xf), tr


def solve_sparse(prob, opt=Options, permc_spec="COLAMD"):
    """ceres_numpy.solve line by line, over a sparse Jacobian; the step from a sparse LU of the damped normal equations
    (permc_spec: SuperLU's column ordering; another ordering is another summation order of the same exact solve)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    free = ~np.asarray(prob["fixed"], bool)
    tr = cn.Trace()
    X = np.array(prob["poses"], np.float64)
    if not free.any() or len(prob["ei"]) + len(prob["fi"]) == 0:
        tr.termination = "empty"
        return X, tr
    nt = 6 * int(free.sum())

    def plus(X, delta):
        Y = X.copy()
        Y[free] = plus_poses(X[free], delta.reshape(-1, 6))
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


def pose_distance(a, b):
    """Largest difference of two pose arrays: metres over the translations, radians (rotation angle of q_a^-1 q_b) over the rotations."""
    dt = float(np.max(np.sqrt(((a[:, :3] - b[:, :3]) ** 2).sum(-1)))) if len(a) else 0.0
    dq = qmul(qconj(a[:, 3:]), b[:, 3:])
    ang = 2.0 * np.arctan2(np.sqrt((dq[:, :3] ** 2).sum(-1)), np.abs(dq[:, 3]))
    return max(dt, float(np.max(ang)) if len(a) else 0.0)


# ---- the seeded synthetic drives of tests/test_gpu_graph.py ----------------------------------------
def _small_rot(rng, n, sigma):
    d = rng.normal(0.0, sigma, (n, 3)) * 0.5
    return plus_poses(np.tile([0, 0, 0, 0, 0, 0, 1.0], (n, 1)), np.concatenate([np.zeros((n, 3)), d], -1))[:, 3:]


def drive(n, seed, radius=20.0, turns=1.15):
    """Circle-like truth (a slow climb and a roll wobble on top), odometry with 2 cm / 2 mrad noise per step, and the poses the
    odometry integrates to from the true first pose."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, 2.0 * np.pi * turns, n)
    t = np.stack([radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(2 * a) + 0.02 * np.arange(n)], -1)
    yaw = a + 0.5 * np.pi
    qy = np.stack([np.zeros(n), np.zeros(n), np.sin(0.5 * yaw), np.cos(0.5 * yaw)], -1)
    roll = 0.05 * np.sin(3 * a)
    qr = np.stack([np.sin(0.5 * roll), np.zeros(n), np.zeros(n), np.cos(0.5 * roll)], -1)
    truth = np.concatenate([t, qmul(qy, qr)], -1)
    rel = relative_pose(truth[:-1], truth[1:])
    noise = np.concatenate([rng.normal(0.0, 0.02, (n - 1, 3)), _small_rot(rng, n - 1, 0.002)], -1)
    odo = pose_mul(rel, noise)
    poses = np.empty((n, 7)); poses[0] = truth[0]
    for k in range(n - 1):
        poses[k + 1] = pose_mul(poses[k], odo[k])
    return truth, odo, poses, rng


def problem(poses, fixed=None):
    n = len(poses)
    return dict(poses=np.array(poses, np.float64), fixed=np.zeros(n, bool) if fixed is None else np.asarray(fixed, bool),
                ei=np.zeros(0, np.int32), ej=np.zeros(0, np.int32), ez=np.zeros((0, 7)), esr=np.zeros(0), est=np.zeros(0),
                fi=np.zeros(0, np.int32), fj=np.zeros(0, np.int32), ft=np.zeros(0), fp=np.zeros((0, 3)), fst=np.zeros(0))


def add_edges(prob, i, j, z, sr=0.01, st=0.1):
    i, j = np.atleast_1d(i).astype(np.int32), np.atleast_1d(j).astype(np.int32)
    z = np.asarray(z, np.float64).reshape(-1, 7)
    prob["ei"] = np.concatenate([prob["ei"], i]); prob["ej"] = np.concatenate([prob["ej"], j])
    prob["ez"] = np.concatenate([prob["ez"], z])
    prob["esr"] = np.concatenate([prob["esr"], np.full(len(i), sr)]); prob["est"] = np.concatenate([prob["est"], np.full(len(i), st)])


def add_fixes(prob, i, j, t, p, st=0.01):
    i, j = np.atleast_1d(i).astype(np.int32), np.atleast_1d(j).astype(np.int32)
    prob["fi"] = np.concatenate([prob["fi"], i]); prob["fj"] = np.concatenate([prob["fj"], j])
    prob["ft"] = np.concatenate([prob["ft"], np.atleast_1d(t).astype(np.float64)])
    prob["fp"] = np.concatenate([prob["fp"], np.asarray(p, np.float64).reshape(-1, 3)])
    prob["fst"] = np.concatenate([prob["fst"], np.full(len(i), st)])


def _chain(prob, odo):
    n = len(prob["poses"])
    add_edges(prob, np.arange(n - 1), np.arange(1, n), odo)


def _closures(prob, truth, rng, pairs, wrong=None):
    for k, (i, j) in enumerate(pairs):
        z = pose_mul(relative_pose(truth[i], truth[j])[None], np.concatenate([rng.normal(0, 0.01, (1, 3)), _small_rot(rng, 1, 0.001)], -1))[0]
        if wrong is not None and k == wrong:
            z[0] += 5.0
        add_edges(prob, i, j, z)


def _gps(prob, truth, rng, at, t=None):
    at = np.asarray(at, int)
    t = rng.uniform(0.1, 0.9, len(at)) if t is None else np.asarray(t, float)
    p = (1 - t)[:, None] * truth[at, :3] + t[:, None] * truth[at + 1, :3] + rng.normal(0, 0.01, (len(at), 3))
    add_fixes(prob, at, at + 1, t, p)


CASES = ("a", "b", "c", "d", "e", "f", "g", "h")
SEEDS = dict(a=11, b=12, c=13, d=14, e=15, f=16, g=17, h=18)


def make_case(name):
    """The parity shapes (a) .. (h) of tests/test_gpu_graph.py."""
    n = dict(a=3, b=37, c=65, d=130, e=100, f=80, g=2500, h=12)[name]
    truth, odo, poses, rng = drive(n, SEEDS[name])
    fixed = np.zeros(n, bool)
    if name == "b":
        fixed[0] = True
    if name == "g":
        fixed[n // 2] = True
    prob = problem(poses, fixed)
    _chain(prob, odo)
    if name == "a":
        _gps(prob, truth, rng, [0, 1])
    elif name == "b":
        _closures(prob, truth, rng, [(2, 33), (10, 36)])
    elif name == "c":
        _gps(prob, truth, rng, [0, 12, 25, 38, 50, 63])
    elif name == "d":
        _closures(prob, truth, rng, [(0, 113), (3, 117), (7, 120), (10, 125), (15, 129), (40, 90), (55, 70), (1, 128)])
        _gps(prob, truth, rng, [0, 40, 85, 128])
    elif name == "e":
        _closures(prob, truth, rng, [(k, 50) if k < 50 else (50, k) for k in list(range(10, 45)) + list(range(56, 91))])
    elif name == "f":
        _closures(prob, truth, rng, [(0, 70), (5, 75), (20, 60), (10, 79)], wrong=2)
    elif name == "g":
        _closures(prob, truth, rng, [(0, 2170), (100, 2270), (200, 2370), (300, 2470), (900, 1600)])
        _gps(prob, truth, rng, np.arange(20) * 130 + 7)
    elif name == "h":
        extra = pose_mul(odo[4][None], np.concatenate([rng.normal(0, 0.02, (1, 3)), _small_rot(rng, 1, 0.002)], -1))[0]
        add_edges(prob, 4, 5, extra)
        _gps(prob, truth, rng, [0, 10], t=[0.0, 1.0])
    return prob
