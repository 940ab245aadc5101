"""Writes tests/golden/graph_marginals_model_v1.npz: what the model (tests/graph_marginals_numpy.py) gives for the parity cases of
tests/test_gpu_graph_marginals.py.

    python tests/golden/make_graph_marginals_golden.py

The problems themselves are not stored (graph_marginals_numpy.make_case builds them from their seeds).  Per case:
`pairs_<case>` the requested pairs, `x1_<case>` the poses the model's own optimisation ends at (the start poses are the problem's),
`S0_<case>` / `S1_<case>` the blocks at the start / at those poses, `sd0_` / `sd1_` the standard deviations the whitened difference
divides by, `piv_<case>` the smallest pivot ratio of the cyclic reduction at both, and `d_<case>`, the largest whitened difference
between the two evaluations (sparse LU with COLAMD; LU of the Jacobi-scaled matrix in natural order).  For the two gauge-free cases
`piv_<case>` alone.  The script refuses a case whose d_case exceeds 1e-9.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import graph_marginals_numpy as gm  # noqa: E402


def evaluate(prob, x, pairs):
    H = gm.hessian(prob, x)
    _, nf = gm.gn.free_index(prob["fixed"])
    S, sd = gm.blocks(prob, x, pairs, H=H)
    S2, _ = gm.blocks(prob, x, pairs, scaled=True, H=H)
    return S, sd, gm.whitened(S, S2, sd), gm.cr_min_pivot(H, nf)


def main():
    out = {}
    for name in gm.CASES:
        prob = gm.make_case(name)
        pairs = gm.request(prob)
        x1, tr = gm.gi.solve_sparse(prob)
        S0, sd0, d0, p0 = evaluate(prob, prob["poses"], pairs)
        S1, sd1, d1, p1 = evaluate(prob, x1, pairs)
        d = max(d0, d1)
        print("%-10s %3d pairs  long %d  optimize: %s after %d  d_case %.3g  pivot ratio %.3g / %.3g  sd from %.3g to %.3g" %
              (name, len(pairs), gm.gi.n_long(prob), tr.termination, tr.iterations, d, p0, p1, sd0[sd0 > 0].min(), sd0.max()))
        assert d <= 1e-9, "case %s: d_case %.3g" % (name, d)
        out["pairs_" + name], out["x1_" + name] = pairs, x1
        out["S0_" + name], out["S1_" + name], out["sd0_" + name], out["sd1_" + name] = S0, S1, sd0, sd1
        out["piv_" + name], out["d_" + name] = np.array([p0, p1]), np.float64(d)
    for name in gm.SINGULAR:
        prob = gm.make_case(name)
        H = gm.hessian(prob, prob["poses"])
        ev = np.linalg.eigvalsh(H.toarray())
        out["piv_" + name] = np.float64(gm.cr_min_pivot(H, gm.gn.free_index(prob["fixed"])[1]))
        print("%-10s gauge-free: eigenvalues of H from %.3g to %.3g, pivot ratio %.3g" % (name, ev[0], ev[-1], out["piv_" + name]))
    np.savez_compressed(os.path.join(HERE, "graph_marginals_model_v1.npz"), **out)


if __name__ == "__main__":
    main()
