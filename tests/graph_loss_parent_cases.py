"""What graphs with information factors, and their marginals, returned before a loss per factor existed: the run that
tests/golden/make_graph_loss_parent_golden.py records at the parent commit and tests/test_gpu_graph_loss.py repeats on this build, on
graphs that never call msfl_graph_set_losses.  Cases (ii), (iii), (v) of tests/golden/graph_info_model_v1.npz: a fixed node with two
information closures (ranks 6 and 5), all four factor kinds with more than one workgroup of each family, Huber active on a wrong closure."""
import os

import numpy as np

from tests import graph_info_numpy as gi
from tests import graph_marginals_numpy as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("ii", "iii", "v")


def run(capi):
    """Per case: msfl_graph_cost before and after, the optimised pose bytes, the summary's bytes, the trace, |r|^2 of every factor at
    the result and the marginal blocks of graph_marginals_numpy.request with their summary's bytes."""
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_info_model_v1.npz")))
    G = capi.PoseGraph
    out = {}
    for name in CASES:
        p = {k: gold["%s_%s" % (k, name)] for k in gi.KEYS}
        g = G(0, max_nodes=len(p["poses"]), max_edges=len(p["ei"]) + len(p["gi"]), max_fixes=max(1, len(p["fi"]) + len(p["hi"])))
        g.add_nodes(p["poses"])
        for k in np.nonzero(p["fixed"])[0]:
            g.set_fixed(int(k))
        if len(p["ei"]):
            g.add_edges(G.edges(p["ei"], p["ej"], p["ez"], p["esr"], p["est"]))
        if len(p["fi"]):
            g.add_fixes(G.fixes(p["fi"], p["fj"], p["ft"], p["fp"], p["fst"]))
        g.add_edges_info(G.edges_info(p["gi"], p["gj"], p["gz"], p["gL"]))
        if len(p["hi"]):
            g.add_fixes_info(G.fixes_info(p["hi"], p["hj"], p["ht"], p["hp"], p["hL"]))
        c0 = g.cost()
        s = g.optimize()
        acc, cost = g.trace()
        out["x_" + name] = g.poses()
        out["summary_" + name] = np.frombuffer(bytes(s), np.uint8).copy()
        out["acc_" + name] = acc
        out["trace_cost_" + name] = cost
        out["cost_" + name] = np.array([c0, g.cost()])
        out["chi2_" + name] = np.concatenate([g.chi2(kind) for kind in range(4)])
        S, sm = g.marginals(gm.request(p))
        out["marginals_" + name] = S
        out["marginals_summary_" + name] = np.frombuffer(bytes(sm), np.uint8).copy()
        g.close()
    return out
