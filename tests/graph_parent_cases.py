"""What graphs without an information factor returned before information factors existed: the run that
tests/golden/make_graph_parent_golden.py records at the parent commit and tests/test_gpu_graph_info.py repeats on this build.
Cases (b), (d), (e), (h) of tests/golden/graph_model_v1.npz: a fixed node with long closures, both plain kinds with more than one
workgroup of factors, a hub of 70 long edges, a double edge with fixes at t = 0 and 1."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("b", "d", "e", "h")
KEYS = ("poses", "fixed", "ei", "ej", "ez", "esr", "est", "fi", "fj", "ft", "fp", "fst")


def run(capi):
    """Per case: the optimised pose bytes, the summary's bytes, the trace and msfl_graph_cost before and after."""
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_model_v1.npz")))
    out = {}
    for name in CASES:
        p = {k: gold["%s_%s" % (k, name)] for k in KEYS}
        g = capi.PoseGraph(0, max_nodes=len(p["poses"]), max_edges=len(p["ei"]), max_fixes=max(1, len(p["fi"])))
        g.add_nodes(p["poses"])
        for k in np.nonzero(p["fixed"])[0]:
            g.set_fixed(int(k))
        g.add_edges(g.edges(p["ei"], p["ej"], p["ez"], p["esr"], p["est"]))
        if len(p["fi"]):
            g.add_fixes(g.fixes(p["fi"], p["fj"], p["ft"], p["fp"], p["fst"]))
        c0 = g.cost()
        s = g.optimize()
        acc, cost = g.trace()
        out["x_" + name] = g.poses()
        out["summary_" + name] = np.frombuffer(bytes(s), np.uint8).copy()
        out["acc_" + name] = acc
        out["trace_cost_" + name] = cost
        out["cost_" + name] = np.array([c0, g.cost()])
        g.close()
    return out
