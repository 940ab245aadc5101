"""Writes tests/golden/graph_loss_model_v1.npz: the parity cases of tests/test_gpu_graph_loss.py, the model's result for each
(tests/graph_loss_numpy.py) and d_case, the largest pose difference between its dense and its sparse step solver; and the table of
docs/kernels/graph.md, "A loss per factor": case (v) of graph_info_numpy with its four closures under each loss.

    python tests/golden/make_graph_loss_golden.py

Per case: the problem arrays, `x_<case>`, `tr_<case>` = [termination code, iterations, successful steps], `acc_<case>`, `cost_<case>`
= [initial, final], `d_<case>`; `pairs_v_gm`, `S_v_gm`, `sd_v_gm`, `dm_v_gm`: marginal blocks of (v) at the Geman-McClure result, their
standard deviations and the whitened difference of the model's two evaluations.  For the table: `table_kind`, `table_a` (kind -1: the
wrong closure removed by hand), `table_ate`, `table_chi2` (|r|^2 of the wrong closure at the result, NaN where it is removed),
`table_it`, and `ate_start`, `truth_v`.
The script refuses to write a case on which the two solvers disagree on the trace, or whose d_case exceeds 1e-6.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import graph_loss_numpy as gl  # noqa: E402
import graph_marginals_numpy as gm  # noqa: E402

gi, gn = gl.gi, gl.gn
TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")
TABLE = ((gl.DEFAULT, 0.0), (-1, 0.0), (gl.GEMAN_MCCLURE, 1.0), (gl.GEMAN_MCCLURE, 3.0), (gl.CAUCHY, 1.0), (gl.CAUCHY, 3.0))


def main():
    out = {}
    for name in gl.CASES:
        prob = gl.make_case(name)
        xd, td = gl.solve_dense(prob)
        xs, ts = gl.solve_sparse(prob)
        d = gn.pose_distance(xd, xs)
        print("%-8s %-14s it %2d ok %2d accepted %s cost %.6g -> %.6g  long %d  d_case %.3g" %
              (name, td.termination, td.iterations, td.successful_steps, td.accepted, td.initial_cost, td.final_cost, gi.n_long(prob), d))
        assert (td.termination, td.iterations, td.successful_steps, td.accepted) == (ts.termination, ts.iterations, ts.successful_steps, ts.accepted), \
            "case %s: the two solvers disagree on the trace; change its seed" % name
        assert d <= 1e-6, "case %s: d_case %.3g" % (name, d)
        for k in gl.KEYS:
            out["%s_%s" % (k, name)] = prob[k]
        out["x_" + name] = xd
        out["tr_" + name] = np.array([TERMINATION.index(td.termination), td.iterations, td.successful_steps], np.int32)
        out["acc_" + name] = np.array(td.accepted, np.int32)
        out["cost_" + name] = np.array([td.initial_cost, td.final_cost])
        out["d_" + name] = np.float64(d)
    # marginals of case (v) at the Geman-McClure result: H = J^T J with every factor's own corrector, by graph_marginals_numpy's two
    # evaluations (sparse LU of H; of the Jacobi-scaled H in natural order), whose whitened difference is dm
    prob = gl.make_case("v_gm")
    J = gl.evaluate_sparse(prob, out["x_v_gm"], gl.Options)[2]
    H = (J.T @ J).tocsc()
    pairs = gm.request(prob)
    S, sd = gm.blocks(prob, out["x_v_gm"], pairs, H=H)
    S2, _ = gm.blocks(prob, out["x_v_gm"], pairs, H=H, scaled=True)
    out["pairs_v_gm"], out["S_v_gm"], out["sd_v_gm"], out["dm_v_gm"] = pairs, S, sd, np.float64(gm.whitened(S, S2, sd))
    Sh, _ = gm.blocks(gi.make_case("v"), out["x_v_gm"], pairs)
    print("marginals of v_gm: %d pairs, d_case %.3g; against Huber on the closures at the same poses the blocks differ by %.3g (whitened)" %
          (len(pairs), out["dm_v_gm"], gm.whitened(S, Sh, sd)))
    assert out["dm_v_gm"] <= 1e-6
    # the mixed case: some factors of every loss kind on each side of s = b at the start poses
    prob = gl.make_case("mixed")
    s = np.concatenate(gi.chi2(prob, prob["poses"]))
    kind = np.concatenate([prob[lk] for lk, _ in gl.LOSS_KEYS]); a = np.concatenate([prob[la] for _, la in gl.LOSS_KEYS])
    for q in range(gl.HUBER, 6):
        m = kind == q
        print("mixed: %-14s %3d factors, %3d with s < b, %3d with s > b" % (gl.NAMES[q], m.sum(), (s[m] < a[m] ** 2).sum(), (s[m] > a[m] ** 2).sum()))
        assert (s[m] < a[m] ** 2).sum() >= 3 and (s[m] > a[m] ** 2).sum() >= 3
    # the table
    base = gl.with_losses(gi.make_case("v"))
    truth = gn.drive(80, gi.SEEDS["v"])[0]
    rows = []
    for kind, a in TABLE:
        prob = gl.without_closure(base, gl.WRONG_CLOSURE) if kind < 0 else {k: np.array(v) for k, v in base.items()}
        if kind > 0:
            gl.set_losses(prob, 2, kind, a)
        x, tr = gl.solve_sparse(prob)
        chi = np.nan if kind < 0 else gi.chi2(prob, x)[2][gl.WRONG_CLOSURE]
        rows.append((kind, a, gi.ate(x, truth), chi, tr.iterations))
        print("closures under %-14s a %.0f: ATE %.3f m, %2d iterations, |r|^2 of the wrong closure %.3g, weights %s" %
              ("removed" if kind < 0 else gl.NAMES[kind], a, rows[-1][2], tr.iterations, chi, np.array2string(gl.weights(prob, x)[2], precision=3)))
    out["table_kind"], out["table_a"], out["table_ate"], out["table_chi2"], out["table_it"] = (np.array(c) for c in zip(*rows))
    out["ate_start"] = np.float64(gi.ate(base["poses"], truth))
    out["truth_v"] = truth
    print("start poses: ATE %.3f m" % out["ate_start"])
    np.savez_compressed(os.path.join(HERE, "graph_loss_model_v1.npz"), **out)


if __name__ == "__main__":
    main()
