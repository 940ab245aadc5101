"""CPU: the numpy model of the Gaussian pose prior (tests/prior_numpy.py) against finite differences and against the
trust-region loop of tests/ceres_numpy.py.  No GPU, no reference."""
import numpy as np

from tests import ceres_numpy as cn
from tests import prior_numpy as pn

H_FD = 1e-4
EPS = np.finfo(np.float64).eps


def _random_unit_quat(rng):
    q = rng.normal(size=4)
    return q / np.sqrt(q @ q)


def _rotated(q0, axis, angle):
    """q0 * dq(axis * angle), through ceres_numpy.plus."""
    return cn.plus(np.concatenate([np.zeros(3), q0]), np.concatenate([np.zeros(3), axis * angle]))[3:7]


def _cases():
    rng = np.random.default_rng(20240611)
    out = []
    for i in range(50):
        q0 = _random_unit_quat(rng)
        axis = rng.normal(size=3); axis /= np.sqrt(axis @ axis)
        angle = [0.0, 1e-3, 0.1, 1.0, 2.0, 3.0][i % 6] if i < 12 else rng.uniform(0.0, 3.0)   # up to 3 rad apart
        q = _rotated(q0, axis, angle)
        if i % 2:
            q = -q                                   # the same rotation from the other hemisphere: conj(q0) q has w < 0
        t0, t = rng.normal(size=3) * 10.0, rng.normal(size=3) * 10.0
        L = pn.random_spd_sqrt(rng) if i % 3 else rng.normal(size=(6, 6)) * 30.0
        if i % 7 == 0:
            L[3:] = 0.0                              # rank deficient
        out.append((np.concatenate([t, q]), (np.concatenate([t0, q0]), L), angle))
    return out


def test_jacobian_equals_central_differences():
    """J of prior_rows against central differences of r through ceres_numpy.plus, step h = 1e-4, 50 seeded (x, prior)
    pairs: rotations 0 .. 3 rad apart, every second one with q negated (the w < 0 branch), full-rank and rank-deficient L.

    Bound (absolute, per row i of J).  Along tangent axis k the rotation error is 2 (w s e_k + c v + s v x e_k) with
    s = sin(h / 2), c = cos(h / 2), so each component's third derivative in h is at most (2 / 8)(|w| + |v_i| + |v|) <=
    (1 + sqrt 2) / 4 = 0.604; the translation part is linear.  Central-difference truncation is h^2 / 6 times that, times
    the 1-norm of row i's rotation half of L; rounding adds 8 eps max|r| / h (r itself is a 6-term sum, and plus()
    normalises).  With h = 1e-4 and |L| ~ 1e2 the bound is ~1e-6 for entries of J that are ~1e2.
    Observed maximum of error / bound over the 50 cases: 0.389 (largest absolute error 4.3e-8)."""
    worst = 0.0
    worst_abs = 0.0
    n_negative_w = 0
    for x, prior, angle in _cases():
        cost, r, J = pn.prior_rows(x, prior)
        L = prior[1]
        assert r.shape == (6,) and J.shape == (6, 6) and cost == 0.5 * float(r @ r)
        # the w < 0 branch was met: the raw quaternion product has a negative scalar part for the negated q
        q0, q = prior[0][3:7], x[3:7]
        if -(-q0[:3]) @ q[:3] + q0[3] * q[3] < 0:
            n_negative_w += 1
        fd = np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6); d[k] = H_FD
            fd[:, k] = (pn.prior_rows(cn.plus(x, d), prior)[1] - pn.prior_rows(cn.plus(x, -d), prior)[1]) / (2 * H_FD)
        bound = H_FD ** 2 / 6.0 * 0.604 * np.abs(L[:, 3:]).sum(1) + 8 * EPS * max(np.abs(r).max(), 1.0) / H_FD
        err = np.abs(J - fd).max(1)
        worst = max(worst, float((err / bound).max()))
        worst_abs = max(worst_abs, float(err.max()))
        assert np.all(err <= bound), (angle, err, bound)
        # the sign fix makes q and -q the same pose
        xn = x.copy(); xn[3:7] = -xn[3:7]
        rn, Jn = pn.prior_rows(xn, prior)[1:]
        assert np.abs(rn - r).max() <= 1e-12 * max(1.0, np.abs(r).max()) and np.abs(Jn - J).max() <= 1e-12 * np.abs(J).max()
    print("central differences: worst error / bound %.3g, worst absolute error %.3g, w < 0 cases %d" % (worst, worst_abs, n_negative_w))
    assert n_negative_w >= 20


def test_jacobian_is_the_closed_form_of_the_definition():
    """The matrix-built J equals L blockdiag(I, w I + skew(v)) with (v, w) from the quaternion product of the definition."""
    for x, prior, angle in _cases():
        q0, q = prior[0][3:7], x[3:7]
        c = np.concatenate([np.zeros(3), -q0[:3], q0[3:4]])
        qe = cn.plus(c, np.zeros(6))[3:7]           # conj(q0), normalised
        ax, ay, az, aw = qe; bx, by, bz, bw = q
        v = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])
        w = aw * bw - ax * bx - ay * by - az * bz
        if w < 0:
            v, w = -v, -w
        want = prior[1] @ np.block([[np.eye(3), np.zeros((3, 3))], [np.zeros((3, 3)), w * np.eye(3) + cn.skew(v)]])
        r, J = pn.prior_rows(x, prior)[1:]
        assert np.abs(J - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), angle
        assert np.abs(r - prior[1] @ np.concatenate([x[:3] - prior[0][:3], 2 * v])).max() <= 1e-11 * max(1.0, np.abs(r).max())


def test_a_prior_alone_is_solved_to_its_mean():
    """L = I, no lidar block, start 0.3 m / 0.1 rad off: ceres_numpy.solve walks to the prior mean.

    Bar: 1e-7 m / 1e-7 rad, the pose bar every GPU parity test of this suite uses (tests/test_gpu_scan2map.py TIGHT); the
    loop's own stopping rules (gradient 1e-10, parameter 1e-8, six iterations) do not promise more on their own.
    Observed: translation 0 (the translation rows are linear: one step), rotation 2.4e-9 rad."""
    rng = np.random.default_rng(7)
    mean = np.concatenate([rng.normal(size=3), _random_unit_quat(rng)])
    d = np.concatenate([np.array([0.3, 0.0, 0.0]), np.array([0.0, 0.1, 0.0])])
    x0 = cn.plus(mean, d)
    empty = np.zeros(0, dtype=[("kind", np.int32), ("p", np.float64, 3), ("C", np.float64, 3), ("N", np.float64, 3)])
    x, tr = cn.solve(pn.Problem(empty, (mean, np.eye(6))), x0, evaluate_fn=pn.evaluate_with_prior)
    assert abs(tr.initial_cost - 0.5 * (0.3 ** 2 + (2 * np.sin(0.05)) ** 2)) <= 1e-12
    assert tr.successful_steps >= 1
    assert np.abs(x[:3] - mean[:3]).max() <= 1e-7
    v, w = pn.rotation_error(mean[3:7], x[3:7])
    assert 2 * np.sqrt(v @ v) <= 1e-7
    assert tr.final_cost <= 1e-14                    # = 1/2 (1e-7^2 + 1e-7^2)
    # and the matchers' gating on top of it (prior_numpy.solve): no correspondence, pose untouched
    x_g, _ = pn.solve(empty, x0, (mean, np.eye(6)))
    assert np.array_equal(x_g, x0)


def test_a_zero_prior_adds_nothing():
    rng = np.random.default_rng(3)
    corr = np.zeros(4, dtype=[("kind", np.int32), ("p", np.float64, 3), ("C", np.float64, 3), ("N", np.float64, 3)])
    corr["kind"] = [1, 2, 2, 0]
    corr["p"] = rng.normal(size=(4, 3)); corr["C"] = rng.normal(size=(4, 3))
    n = rng.normal(size=(4, 3)); corr["N"] = n / np.linalg.norm(n, axis=1, keepdims=True)
    x = np.concatenate([rng.normal(size=3), _random_unit_quat(rng)])
    a = cn.evaluate(corr, x, cn.Options)
    b = pn.evaluate_with_prior(pn.Problem(corr, (x, np.zeros((6, 6)))), x, cn.Options)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    c = pn.evaluate_with_prior(pn.Problem(corr, (x, np.eye(6))), x, cn.Options)
    assert len(c[1]) == len(a[1]) + 6 and c[2].shape == (len(a[1]) + 6, 6) and c[0] == a[0]      # at its mean the prior costs nothing
