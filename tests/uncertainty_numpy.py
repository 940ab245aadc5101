"""Independent numpy restatement of msfl_match_uncertainty (include/msfl_c_api.h).

TEST INFRASTRUCTURE.  The reference computes no covariance (its PoseWithCovariance messages carry 36 zeros), so the
yardstick of the uncertainty output is this file, not the reference: the stacked, Huber-corrected Jacobian of
tests/ceres_numpy.evaluate (what ceres::Covariance is handed) -> H = J^T J, LAPACK's symmetric eigen-solver, the header's
sign convention, the thresholded pseudo-inverse, the a-posteriori variance factor and the change of the rotation block
from body to parent axes.  Built differently from the kernel on purpose: explicit J instead of accumulated normal
equations, eigh instead of Jacobi rotations.
"""
import numpy as np

from tests import ceres_numpy as cn


def information(corr, pose, opt=cn.Options):
    """(H = J^T J, cost, number of residual rows) of the problem `corr` at `pose`, robustified as Ceres evaluates it."""
    cost, r, J = cn.evaluate(corr, np.asarray(pose, dtype=np.float64), opt)
    return J.T @ J, cost, len(r)


def fix_signs(rows):
    """Header convention: every row's largest-magnitude component (lowest index on ties) is positive."""
    rows = np.array(rows, dtype=np.float64)
    for k in range(len(rows)):
        i = int(np.argmax(np.abs(rows[k])))          # argmax returns the first maximum
        if rows[k, i] < 0:
            rows[k] = -rows[k]
    return rows


def decompose(H, min_eigenvalue=0.0):
    """eigenvalues (ascending), eigenvectors (row k), covariance (pseudo-inverse over the kept pairs), n_degenerate."""
    w, V = np.linalg.eigh(H)
    rows = fix_signs(V.T)
    thr = max(float(min_eigenvalue), 1e-14 * w[-1])
    n_deg = int((w < thr).sum())
    cov = np.zeros((6, 6))
    for k in range(6):
        if not w[k] < thr:
            cov += np.outer(rows[k], rows[k]) / w[k]
    return w, rows, cov, n_deg


def sigma2(final_cost, n_residuals):
    return 2.0 * final_cost / (n_residuals - 6) if n_residuals > 6 else 0.0


def record(corr, pose, min_eigenvalue=0.0, opt=cn.Options):
    H, cost, m = information(corr, pose, opt)
    w, rows, cov, n_deg = decompose(H, min_eigenvalue)
    return dict(information=H, eigenvalues=w, eigenvectors=rows, covariance=cov, sigma2=sigma2(cost, m), n_residuals=m,
                n_degenerate=n_deg, valid=1)


def covariance_in_parent_frame(pose, cov, scale=1.0):
    """scale * A cov A^T, A = diag(I, R(pose)): the tangent's rotation block is body-frame (q = q * dq), a ROS
    PoseWithCovariance wants rotations about the fixed parent axes."""
    R = cn.quat_to_R(np.asarray(pose, dtype=np.float64)[3:7])
    S = np.asarray(cov, dtype=np.float64).reshape(6, 6)
    # spelled out entry by entry (the identity block costs no rounding): M = A S, out = M A^T
    M = np.zeros((6, 6))
    out = np.zeros((6, 6))
    for i in range(6):
        for j in range(6):
            M[i, j] = S[i, j] if i < 3 else R[i - 3, 0] * S[3, j] + R[i - 3, 1] * S[4, j] + R[i - 3, 2] * S[5, j]
    for i in range(6):
        for j in range(6):
            out[i, j] = scale * (M[i, j] if j < 3 else M[i, 3] * R[j - 3, 0] + M[i, 4] * R[j - 3, 1] + M[i, 5] * R[j - 3, 2])
    return out


def oracle_last_problem(orc, mc, ms, corner, surf, guess, outer_iterations=2):
    """The oracle's MatchScan2Map spelled out: (correspondences of the LAST solve, returned pose, that solve's summary)."""
    pose = np.array(guess, dtype=np.float64)
    corr = summ = None
    for _ in range(outer_iterations):
        corr = orc.associate_scan2map(mc, ms, corner, surf, pose)
        pose, summ = orc.ceres_solve(corr, pose)
    return corr, pose, summ
