"""Independent numpy restatement of the Gaussian pose prior block (msfl_pose_prior, include/msfl_c_api.h;
docs/kernels/prior.md).

TEST INFRASTRUCTURE.  The reference has no prior on its lidar problems (its IMUFactor on the scan-to-map problem is
commented out), so the yardstick is this file together with tests/ceres_numpy.solve(evaluate_fn=...).  Built differently
from the kernel on purpose: the rotation error goes through rotation MATRICES (R0^T R -> the quaternion's vector part
from the skew part, its scalar from the trace), and the Jacobian's rotation block is assembled from the matrix identity
d(skew part of Re exp(d)) instead of the quaternion form w I + skew(v).
"""
import collections

import numpy as np

from tests import ceres_numpy as cn


def rotation_error(q0, q):
    """(v, w) = vector / scalar part of conj(q0) * q with w >= 0, from Re = R(q0)^T R(q).

    For Re = I + 2 w skew(v) + 2 skew(v)^2:  skew part (Re - Re^T) / 2 = 2 w skew(v),  trace = 4 w^2 - 1.
    w = 0 (a half turn) has no skew part: the axis then comes from the symmetric part, Re + I = 2 v v^T, with the sign of
    its largest component taken from the quaternion product (any sign minimises the same cost there; tests only meet it
    through this function when they ask for it)."""
    Re = cn.quat_to_R(np.asarray(q0, dtype=np.float64)).T @ cn.quat_to_R(np.asarray(q, dtype=np.float64))
    w = 0.5 * np.sqrt(max(0.0, 1.0 + np.trace(Re)))
    a = 0.5 * np.array([Re[2, 1] - Re[1, 2], Re[0, 2] - Re[2, 0], Re[1, 0] - Re[0, 1]])   # = 2 w v
    if w > 1e-4:
        return a / (2.0 * w), w
    # near a half turn: |v_i| from the diagonal of (Re + I) / 2 - w^2 I, signs relative to the largest from the off-diagonal
    S = 0.5 * (Re + Re.T)
    d = np.sqrt(np.maximum(0.0, 0.5 * (np.diag(S) + 1.0) - w * w))
    i = int(np.argmax(d))
    v = np.array([S[i, j] / (2.0 * d[i]) if j != i else d[i] for j in range(3)])
    if w > 0.0 and a @ v < 0:
        v = -v
    return v, w


def prior_rows(x, prior):
    """(cost, r, J) of the prior block at pose x = (t, q xyzw).  prior = (pose7, L 6 x 6)."""
    x = np.asarray(x, dtype=np.float64)
    x0 = np.asarray(prior[0], dtype=np.float64)
    L = np.asarray(prior[1], dtype=np.float64).reshape(6, 6)
    v, w = rotation_error(x0[3:7], x[3:7])
    e = np.concatenate([x[:3] - x0[:3], 2.0 * v])
    r = L @ e
    # d(2 v)/d(dtheta) for R -> R exp(skew(dtheta)): Re' = Re (I + skew(d)); its skew part changes by (Re S + S Re^T) / 2 with
    # S = skew(d), which for a 3 x 3 rotation is skew(((tr Re) I - Re^T) d / 2); and 2 v = skewpart / w with
    # dw = -(v . d) / 2.  Written out with Re^T = I - 2 w skew(v) + 2 skew(v)^2 this is A = w I + skew(v).
    Re = cn.quat_to_R(x0[3:7]).T @ cn.quat_to_R(x[3:7])
    if w > 1e-4:
        B = 0.5 * (np.trace(Re) * np.eye(3) - Re.T)                  # d(2 w v)/d(dtheta)
        A = (B + np.outer(v, v)) / w                                 # 2 v = (2 w v) / w,  dw = -v^T d / 2
    else:
        A = w * np.eye(3) + cn.skew(v)
    J = L @ np.block([[np.eye(3), np.zeros((3, 3))], [np.zeros((3, 3)), A]])
    return 0.5 * float(r @ r), r, J


def is_zero(prior):
    return not np.any(np.asarray(prior[1]) != 0.0)


Problem = collections.namedtuple("Problem", "corr prior")   # what evaluate_with_prior takes as `corr`: lidar correspondences + (pose7, L) or None


def evaluate_with_prior(corr, x, opt, want_jacobian=True):
    """evaluate_fn for ceres_numpy.solve: `corr` is a Problem; the lidar blocks (Huber-corrected, ceres_numpy.evaluate) plus
    the prior rows (no loss).  An all-zero sqrt_information adds nothing, like the kernel's explicit skip."""
    cost, r, J = cn.evaluate(corr.corr, x, opt)
    if corr.prior is None or is_zero(corr.prior):
        return cost, r, J
    pc, pr, pJ = prior_rows(x, corr.prior)
    return cost + pc, np.concatenate([r, pr]), np.vstack([J.reshape(-1, 6), pJ])


def solve(corr, x0, prior, opt=cn.Options):
    """ceres_numpy.solve on lidar + prior, with the matchers' gating: the prior is not a correspondence, so a problem
    without any lidar block leaves the pose untouched (docs/kernels/prior.md: deviation from 'Ceres would solve the
    prior alone')."""
    if not any(int(c["kind"]) != 0 for c in corr):
        return np.array(x0, dtype=np.float64), None
    return cn.solve(Problem(corr, prior), x0, opt, evaluate_fn=evaluate_with_prior)


def random_spd_sqrt(rng, scale_t=20.0, scale_r=60.0):
    """A full-rank random square-root information: upper-triangular Cholesky factor of a random SPD matrix whose
    translation / rotation blocks are ~ (1 / 5 cm)^2 and (1 / 1 degree)^2."""
    A = rng.normal(size=(6, 6))
    D = np.diag([scale_t] * 3 + [scale_r] * 3)
    S = D @ (A @ A.T / 6.0 + np.eye(6)) @ D
    return np.linalg.cholesky(S).T


def translation_only_sqrt(sigma=0.05):
    """Rank 3: 1 / sigma on the three translation rows, nothing on rotation."""
    L = np.zeros((6, 6))
    L[0, 0] = L[1, 1] = L[2, 2] = 1.0 / sigma
    return L
