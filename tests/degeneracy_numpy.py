"""Independent numpy restatement of the degeneracy-aware solve (msfl_set_degeneracy, include/msfl_c_api.h;
docs/kernels/degeneracy.md), and its table of fixed cases.

TEST INFRASTRUCTURE.  Solution remapping after Zhang & Singh: the entry matrix H0 = J^T J of a solve is decomposed, the
eigen-directions below the threshold are HELD, and the solve is Ceres' trust-region LM on the reduced problem whose local
parameterisation is Plus_r(x, y) = Plus(x, V_k y), V_k the 6 x k matrix of the kept eigenvectors.  Built differently from
the kernel on purpose: the kernel rotates the accumulated 6 x 6 normal equations and decouples the held coordinates; here
the stacked Jacobian is right-multiplied by V_k and tests/ceres_numpy.solve runs a k-dimensional problem (lstsq on the
augmented m x k system).
"""
import collections
import functools

import numpy as np

from tests import ceres_numpy as cn
from tests import prior_numpy as pn

CORR_DTYPE = [("kind", np.int32), ("p", np.float64, 3), ("C", np.float64, 3), ("N", np.float64, 3)]
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def threshold(lams, min_eigenvalue):
    """The rule of msfl_match_uncertainty.n_degenerate."""
    return max(float(min_eigenvalue), 1e-14 * float(np.max(lams)))


def classify(lams, min_eigenvalue):
    """n_held: eigenvalues strictly below max(min_eigenvalue, 1e-14 * lambda_max)."""
    return int(np.sum(np.asarray(lams) < threshold(lams, min_eigenvalue)))


def margin(lams, min_eigenvalue):
    """The smallest factor between an eigenvalue and the threshold, whichever side it is on (>= 2 in every case of the table:
    the held set is then the same under any rounding)."""
    thr = threshold(lams, min_eigenvalue)
    lams = np.maximum(np.asarray(lams, dtype=np.float64), 1e-300)
    return float(np.min(np.maximum(lams / thr, thr / lams)))


def entry_matrix(corr, x, prior=None, opt=cn.Options):
    """(cost, g, H0) at pose x: the lidar rows robustified as Ceres evaluates them, plus the prior's block if one is given."""
    cost, r, J = pn.evaluate_with_prior(pn.Problem(corr, prior), np.asarray(x, dtype=np.float64), opt)
    J = J.reshape(-1, 6)
    return cost, J.T @ r, J.T @ J


def decompose(H):
    """(eigenvalues ascending, V with ROW k = eigenvector k); sign: the largest-magnitude component (lowest index on ties) positive."""
    lam, U = np.linalg.eigh(H)
    V = U.T.copy()
    for k in range(6):
        i = int(np.argmax(np.abs(V[k]) >= np.abs(V[k]).max()))
        if V[k, i] < 0:
            V[k] = -V[k]
    return lam, V


def solve(corr, x0, V, held, prior=None, opt=cn.Options, steps=None):
    """The solve of one outer iteration with the `held` weakest of the eigenvectors V (rows, ascending) held.

    held == 0: the solve is the plain one (identity basis: nothing changes).  held == 6: no step, trace None.
    Otherwise ceres_numpy.solve with evaluate_fn = the base evaluation (with the prior's rows when one is given) whose Jacobian
    is right-multiplied by V_k, plus_fn = plus(x, V_k y), n_tangent = k.  `steps`: a list that receives the 6-vector tangent step
    of every candidate."""
    x0 = np.array(x0, dtype=np.float64)
    if not any(int(c["kind"]) != 0 for c in corr):
        return x0, None                                     # the matchers' gate: nothing to solve, prior or not
    if held >= 6:
        return x0, None
    Vk = np.eye(6) if held == 0 else np.asarray(V, dtype=np.float64)[held:].T          # 6 x k
    problem = pn.Problem(corr, prior)

    def evaluate_fn(p, x, o):
        cost, r, J = pn.evaluate_with_prior(p, x, o)
        return cost, r, J.reshape(-1, 6) @ Vk

    def plus_fn(x, y):
        d = Vk @ y
        if steps is not None:
            steps.append(d)
        return cn.plus(x, d)

    return cn.solve(problem, x0, opt, evaluate_fn=evaluate_fn, plus_fn=plus_fn, n_tangent=Vk.shape[1])


def gap_threshold(lams):
    """A threshold in the widest gap of an ascending spectrum (geometric mean of its two sides) and the number of eigenvalues below it."""
    lams = np.asarray(lams, dtype=np.float64)
    k = int(np.argmax(lams[1:] / lams[:-1]))
    return float(np.sqrt(lams[k] * lams[k + 1])), k + 1


# ---- the fixed cases ---------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name block corner surf rec corr guess min_eig n_held")


def _arrays(corr, nc):
    corner = np.concatenate([corr["p"][:nc], np.zeros((nc, 1))], 1).astype(np.float32)
    surf = np.concatenate([corr["p"][nc:], np.zeros((len(corr) - nc, 1))], 1).astype(np.float32)
    rec = np.concatenate([corr["C"], corr["N"]], 1)
    return corner, surf, rec


def _axis_corr(n=60, seed=3, spread=np.pi):
    """~60 plane rows whose normals have an exactly zero x component (drawn around a pose a few centimetres / tenths of a degree
    off the identity guess), plus three weak rows with normal e_x whose points lie on the body x axis and whose residual at the
    guess is 0.05 m.  At the identity-rotation guess the x column of every strong row's Jacobian is exactly zero and the weak rows'
    Jacobian is exactly (1, 0, 0, 0, 0, 0): (e_x, 0) is an exact eigenvector of H0 with eigenvalue 3."""
    rng = np.random.default_rng(seed)
    truth = np.array([0.0, 0.06, -0.04, 0.0, 0.0, 0.0, 1.0])
    truth[3:] = cn.plus(IDENT, np.array([0, 0, 0, 0.004, -0.003, 0.005]))[3:]
    R = cn.quat_to_R(truth[3:])
    corr = np.zeros(n + 3, CORR_DTYPE)
    for i in range(n):
        p = rng.uniform(-20, 20, 3).astype(np.float32).astype(np.float64)
        a = rng.uniform(-spread, spread)
        N = np.array([0.0, np.cos(a), np.sin(a)])
        corr[i] = (2, p, R @ p + truth[:3] + 0.005 * rng.normal(size=3), N)
    for j, px in enumerate((5.0, 10.0, 15.0)):
        corr[n + j] = (2, (px, 0.0, 0.0), (px - 0.05, 0.0, 0.0), (1.0, 0.0, 0.0))
    return corr


@functools.lru_cache(maxsize=None)
def cases():
    """The table.  Every case is a fixed-record problem for msfl_solve_records with its threshold; n_held is what the numpy
    spectrum of H0 at the guess gives (the CPU test holds every eigenvalue a factor 2 away from the threshold)."""
    from tests import lm_boundary_cases as lb
    from tests.test_gpu_scan2map import _synthetic_corr
    out = []

    def add(name, block, corr, nc, guess, pick):
        corr = np.array(corr)
        lam = np.linalg.eigvalsh(entry_matrix(corr, guess)[2])
        min_eig = pick(lam)
        corner, surf, rec = _arrays(corr, nc)
        for a in (corr, corner, surf, rec):
            a.setflags(write=False)
        out.append(Case(name, block, corner, surf, rec, corr, np.array(guess, dtype=np.float64), min_eig, classify(lam, min_eig)))

    axis = _axis_corr()
    for block in lb.BLOCKS:
        add("axis", block, axis, 0, IDENT, lambda lam: float(np.sqrt(lam[0] * lam[1])))
    # two held: normals within +-0.25 rad of e_y, so z translation is weak as well (and x as in the axis case)
    two = _axis_corr(n=200, seed=4, spread=0.25)
    for block in lb.BLOCKS:
        add("two_held", block, two, 0, IDENT, lambda lam: float(np.sqrt(lam[1] * lam[2])))
    rng = np.random.default_rng(21)
    gen, truth = _synthetic_corr(rng, n_plane=300, n_edge=30, noise=0.01)
    cvt = np.zeros(len(gen), CORR_DTYPE)
    for f in ("kind", "p", "C", "N"):
        cvt[f] = gen[f]
    from msf_loam_amd import synth
    guess = synth.perturb_pose(truth, rng, 0.2, 2.0)
    add("nothing_held", 128, cvt, 30, guess, lambda lam: 0.25 * float(lam[0]))
    add("all_held", 128, cvt, 30, guess, lambda lam: 4.0 * float(lam[-1]))
    # the seams of evaluate_pass: one case on each side of the plane cache (832 / 3 072 rows) and of the edge list (1 024)
    want = [(b, lb.CACHE[b] + d, 0) for b in lb.BLOCKS for d in (-1, 1)] + [(b, 300, lb.EDGE_LIST_MAX + d) for b in lb.BLOCKS for d in (-1, 1)]
    for block, ns, nc in want:
        c = next(c for c in lb.CASES if (c.block, c.ns, c.nc, c.pattern, c.prior) == (block, ns, nc, "none", False))
        p = lb.problem(c.k)
        cvt = np.zeros(len(p.corr), CORR_DTYPE)
        for f in ("kind", "p", "C", "N"):
            cvt[f] = p.corr[f]
        add("seam-ns%d-nc%d" % (ns, nc), block, cvt, nc, p.guess, lambda lam: gap_threshold(lam)[0])
    return tuple(out)


def case_id(c):
    return "%s-b%d" % (c.name, c.block)
