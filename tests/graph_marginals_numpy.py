"""Numpy model of msfl_graph_marginals / msfl_graph_relative_covariance (docs/kernels/graph.md, "Marginals").

TEST INFRASTRUCTURE.  Written from the definition, not from the kernels: at given poses the stacked Jacobian of
graph_info_numpy.evaluate_sparse (Huber corrector applied), H = J^T J with no LM diagonal, Sigma = H^-1, delivered in [dt ; dtheta] with
dtheta = 2 d (world frame, left rotation vector): block (a, b) is diag(I, 2I) Sigma_d[a, b] diag(I, 2I).  graph_numpy and graph_info_numpy
are imported, not edited.

The blocks are evaluated two ways (sparse LU of H with COLAMD; LU of the Jacobi-scaled matrix in natural order, unscaled again); their
whitened difference is d_case.  cr_min_pivot restates the block cyclic reduction of the chain part in plain numpy and reports the smallest
Cholesky pivot^2 / diagonal it meets: the number the device's pivot test looks at.
"""
import numpy as np

try:
    from tests import graph_info_numpy as gi
    from tests import graph_numpy as gn
except ImportError:                        # run as a script from tests/golden
    import graph_info_numpy as gi
    import graph_numpy as gn

Options = gi.Options
TD = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])     # [dt ; d] -> [dt ; dtheta]

CASES = ("two", "free3", "free4", "b", "ii", "iii", "iv_rank5", "v", "chain1026", "g")
SINGULAR = ("h", "i")                      # anchored, yet the rotation about the line of their position fixes is free
UNANCHORED = ("e", "f")
SEEDS = dict(two=41, free3=42, free4=43, chain1026=44)


def make_case(name):
    """The parity cases of tests/test_gpu_graph_marginals.py as four-kind problems."""
    if name in gn.CASES:
        return gi.with_info(gn.make_case(name))
    if name in gi.CASES:
        return gi.make_case(name)
    n = dict(two=2, free3=4, free4=5, chain1026=1026)[name]
    truth, odo, poses, rng = gn.drive(n, SEEDS[name])
    fixed = np.zeros(n, bool); fixed[0] = True
    prob = gi.problem(poses, fixed)
    if name == "two":                                    # one free node, one information edge
        gi.add_edges_info(prob, 0, 1, odo[0], gi.draw_L(rng, 1))
        return prob
    gn._chain(prob, odo)
    if name == "free3":                                  # three free nodes and a long information edge between the outer two
        gi.add_edges_info(prob, 1, 3, gi._closure_z(truth, rng, 1, 3), gi.draw_L(rng, 1))
    elif name == "free4":                                # four free nodes, no long factor: the direct solve
        gn._gps(prob, truth, rng, [2])
    else:                                                # 1 025 free nodes: the first size with a level outside the one-workgroup tail
        gn._closures(prob, truth, rng, [(5, 1000)])
    return prob


def request(prob):
    """The pairs a parity test asks for: about 8 marginals spread over the free nodes (first and last included), 4 cross blocks and the
    reverse of one, one duplicate, and both orders of a pair with a fixed end where the graph has a fixed node."""
    fixed = np.asarray(prob["fixed"], bool)
    free = np.nonzero(~fixed)[0]
    pick = free[np.unique(np.round(np.linspace(0, len(free) - 1, 8)).astype(int))]
    pairs = [(int(k), int(k)) for k in pick]
    if len(free) >= 2:
        a, b, m = int(free[0]), int(free[-1]), int(free[len(free) // 2])
        pairs += [(a, b), (b, a), (m, int(free[len(free) // 2 - 1])), (int(pick[1]), int(pick[-2])), (m, b)]
    pairs.append(pairs[0])
    if fixed.any():
        f = int(np.nonzero(fixed)[0][0])
        pairs += [(f, int(free[-1])), (int(free[-1]), f), (f, f)]
    return np.array(pairs, np.int32)


def hessian(prob, x, opt=Options):
    """H = J^T J over the free nodes' tangent [dt ; d] at poses x."""
    _, _, J = gi.evaluate_sparse(prob, np.asarray(x, np.float64), opt)
    return (J.T @ J).tocsc()


def _columns(prob, nodes, H, scaled):
    """Sigma_d[:, node] (6 F x 6) per requested free node, by one of the two evaluations."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    fr, nf = gn.free_index(prob["fixed"])
    if scaled:
        s = 1.0 / (1.0 + np.sqrt(H.diagonal()))
        lu = spl.splu((sp.diags(s) @ H @ sp.diags(s)).tocsc(), permc_spec="NATURAL")
    else:
        s = np.ones(6 * nf)
        lu = spl.splu(H, permc_spec="COLAMD")
    out = {}
    for b in nodes:
        E = np.zeros((6 * nf, 6))
        E[6 * fr[b] + np.arange(6), np.arange(6)] = 1.0
        out[b] = s[:, None] * lu.solve(E) * s[6 * fr[b]:6 * fr[b] + 6][None, :]
    return out


def blocks(prob, x, pairs, opt=Options, scaled=False, H=None):
    """(n, 6, 6) blocks Sigma_ab in [dt ; dtheta] and sd (n, 2, 6): the standard deviations of a's and of b's coordinates (zero for a
    fixed node).  a == b is symmetrised; a fixed end gives zeros."""
    fr, nf = gn.free_index(prob["fixed"])
    H = hessian(prob, x, opt) if H is None else H
    pairs = np.asarray(pairs, int).reshape(-1, 2)
    nodes = sorted({int(k) for k in pairs.ravel() if fr[k] >= 0})
    cols = _columns(prob, nodes, H, scaled)
    sd = {k: TD * np.sqrt(np.diag(cols[k][6 * fr[k]:6 * fr[k] + 6])) for k in nodes}
    out, sds = np.zeros((len(pairs), 6, 6)), np.zeros((len(pairs), 2, 6))
    for n, (a, b) in enumerate(pairs):
        if fr[a] < 0 or fr[b] < 0:
            continue
        S = TD[:, None] * cols[b][6 * fr[a]:6 * fr[a] + 6] * TD[None, :]
        out[n] = 0.5 * (S + S.T) if a == b else S
        sds[n, 0], sds[n, 1] = sd[a], sd[b]
    return out, sds


def whitened(A, B, sd):
    """max |A_ij - B_ij| / (sd_i sd_j) over the blocks with two free ends; a block with a fixed end must be exactly zero in both."""
    worst = 0.0
    for a, b, s in zip(A, B, sd):
        if not s.all():
            assert not a.any() and not b.any(), "a block with a fixed end is not all zeros"
            continue
        worst = max(worst, float(np.max(np.abs(a - b) / np.outer(s[0], s[1]))))
    return worst


def _pivot_ratio(A):
    """Cholesky of a 6 x 6 block by hand: the smallest pivot^2 / a_jj (-1 for one that is not finite)."""
    C = np.zeros((6, 6))
    ratio = 1.0
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j] - C[j, :j] @ C[j, :j]
            q = d / A[j, j]
            ratio = min(ratio, q if np.isfinite(q) else -1.0)
            C[j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                C[i, j] = (A[i, j] - C[i, :j] @ C[j, :j]) / C[j, j]
    return ratio


def cr_min_pivot(H, nf):
    """Block cyclic reduction of the block-tridiagonal part of the Jacobi-scaled H: level by level the odd blocks are inverted and the
    even ones reduced, D' = D_k - L_k D_k-1^-1 L_k^T - L_k+1^T D_k+1^-1 L_k+1, L' = -L_k D_k-1^-1 L_k-1.  Returns the smallest pivot ratio."""
    s = 1.0 / (1.0 + np.sqrt(H.diagonal()))
    H = H.tocsr()
    D, L = [], []
    for f in range(nf):
        sl = slice(6 * f, 6 * f + 6)
        D.append(s[sl, None] * H[sl, sl].toarray() * s[None, sl])
        L.append(s[sl, None] * H[sl, 6 * f - 6:6 * f].toarray() * s[None, 6 * f - 6:6 * f] if f else np.zeros((6, 6)))
    ratio = 1.0
    with np.errstate(all="ignore"):
        while True:
            n = len(D)
            if n == 1:
                return min(ratio, _pivot_ratio(D[0]))
            inv = {}
            for k in range(1, n, 2):
                ratio = min(ratio, _pivot_ratio(D[k]))
                inv[k] = np.linalg.inv(D[k]) if np.all(np.isfinite(D[k])) and np.linalg.matrix_rank(D[k]) == 6 else np.full((6, 6), np.nan)
            Dn, Ln = [], []
            for k in range(0, n, 2):
                d, l = D[k].copy(), np.zeros((6, 6))
                if k >= 1:
                    t = L[k] @ inv[k - 1]
                    d -= t @ L[k].T
                    if k >= 2:
                        l = -t @ L[k - 1]
                if k + 1 < n:
                    d -= L[k + 1].T @ inv[k + 1] @ L[k + 1]
                Dn.append(d); Ln.append(l)
            D, L = Dn, Ln


# ---- the covariance of T_a^-1 T_b --------------------------------------------------------------------------------------------
def relative_jacobians(pose_a, pose_b):
    """d(tangent of T_ab) / d[dt_a ; dtheta_a] and / d[dt_b ; dtheta_b]: the tangent of an information edge (z.t + dt, z.q (x) dq(dtheta)),
    the nodes perturbed in the delivered coordinates (world frame, rotation on the left)."""
    pa, pb = np.asarray(pose_a, np.float64), np.asarray(pose_b, np.float64)
    Ra, Rb = gn.quat_to_R(pa[3:] / np.linalg.norm(pa[3:])), gn.quat_to_R(pb[3:] / np.linalg.norm(pb[3:]))
    u = pb[:3] - pa[:3]
    Ja, Jb = np.zeros((6, 6)), np.zeros((6, 6))
    Ja[:3, :3] = -Ra.T; Ja[:3, 3:] = Ra.T @ gn.skew(u); Ja[3:, 3:] = -Rb.T
    Jb[:3, :3] = Ra.T; Jb[3:, 3:] = Rb.T
    return Ja, Jb


def relative_jacobians_numeric(pose_a, pose_b, h=1e-6):
    """The same by central differences through plus_poses (dtheta = 2 d) and the information edge's error e = [t_ab' - t_ab ; 2 vec(qe)]."""
    pa, pb = np.asarray(pose_a, np.float64)[None], np.asarray(pose_b, np.float64)[None]
    z = gn.relative_pose(pa, pb)[0]

    def err(da, db):
        za = gn.relative_pose(gn.plus_poses(pa, (da / TD)[None]), gn.plus_poses(pb, (db / TD)[None]))[0]
        qe = gn.qmul(gn.qconj(z[3:]), za[3:])
        return np.r_[za[:3] - z[:3], 2.0 * np.sign(qe[3]) * qe[:3]]

    Ja, Jb = np.zeros((6, 6)), np.zeros((6, 6))
    zero = np.zeros(6)
    for k in range(6):
        d = np.zeros(6); d[k] = h
        Ja[:, k] = (err(d, zero) - err(-d, zero)) / (2 * h)
        Jb[:, k] = (err(zero, d) - err(zero, -d)) / (2 * h)
    return Ja, Jb


def relative_covariance(pose_a, pose_b, Saa, Sab, Sbb, jacobians=relative_jacobians):
    Ja, Jb = jacobians(pose_a, pose_b)
    J = np.hstack([Ja, Jb])
    S = np.block([[np.asarray(Saa), np.asarray(Sab)], [np.asarray(Sab).T, np.asarray(Sbb)]])
    C = J @ S @ J.T
    return 0.5 * (C + C.T)
