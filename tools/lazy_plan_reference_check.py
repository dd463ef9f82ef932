"""CPU check of the inputs of tests/test_gpu_lazy_plans.py (no GPU): for the cases of its table at n >= first_n (default 620), the
compressed oracle (the tests' reference) against the dense oracle on the uncompressed data on two sampled patterns (a full dense
enumeration at D = 1022 takes minutes), and the node reference's certificates of the nodes the node test draws.  A case whose two
oracles differ by more than 1e-11 relative, or with an uncertified node, must be reseeded before the tests mean anything.

    python tools/lazy_plan_reference_check.py [first_n [last_n]]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from bnb_reference import NodeReference                     # noqa: E402
from oracle import oracle as O                              # noqa: E402
from test_gpu_bnb_nodes import _nodes                       # noqa: E402
import test_gpu_lazy_plans as LP                            # noqa: E402


def dense_vs_compressed(X, y, P, eta, pats):
    Xo, Po = O.homogeneous(X, P)
    Xr, yr = O.regularize(Xo, y, Po, eta)
    R, z = O.compress(Xr, yr)
    comp = O.opt_patterns(R, z, Po, pats)
    dense = O.opt_patterns(Xr, yr, Po, pats)
    return float(np.max(np.abs(comp - dense) / np.maximum(1.0, np.abs(dense))))


def main():
    O.build()
    lo = int(sys.argv[1]) if len(sys.argv) > 1 else 620
    hi = int(sys.argv[2]) if len(sys.argv) > 2 else 1023
    worst = 0.0
    bad = []
    for c in LP.CASES:
        if not lo <= c["n"] <= hi:
            continue
        t0 = time.time()
        X, y, P, eta = LP._plans_problem(c)
        variants = [("faithful", X, y, P, eta)]
        if c["free_too"]:
            variants.append(("free",) + LP._plans_problem(c, D=c["n"], salt=1))
        for name, Xv, yv, Pv, ev in variants:
            pats = np.random.default_rng(c["seed"]).choice(1 << (Pv.shape[1] + 1), 2, replace=False)
            err = dense_vs_compressed(Xv, yv, Pv, ev, pats)
            worst = max(worst, err)
            if not err <= 1e-11:
                bad.append((c["id"], name, err))
            print("%-44s %-9s patterns %-8s dense vs compressed %.2e" % (c["id"], name, list(pats), err), flush=True)
        ipats, ifrees = _nodes(np.random.default_rng(c["seed"]), P.shape[1] + 1, c["nodes"])
        cert = NodeReference(*LP._plans_problem(c, planted=False)).nodes(ipats, ifrees)["certified"]      # the node test's problem
        if not cert.all():
            bad.append((c["id"], "nodes", int((~cert).sum())))
        print("%-44s nodes certified %d / %d   (%.1f s)" % (c["id"], int(cert.sum()), len(cert), time.time() - t0), flush=True)
    print("worst dense-vs-compressed difference %.3e; failures: %s" % (worst, bad or "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
