"""CPU check of the inputs of tests/test_gpu_tile_counts.py (no GPU): for every case of its table, and for the free-intercept and
batch variants, the compressed oracle (the tests' reference) against the dense oracle on the uncompressed data for every pattern, and
the node reference's certificates of the nodes the node test draws.  A case whose two oracles differ by more than 1e-11 relative, or
with an uncertified node, must be reseeded before the tests mean anything.

    python tools/tile_count_reference_check.py [first_T [last_T]]
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
import test_gpu_tile_counts as TC                           # noqa: E402


def dense_vs_compressed(X, y, P, eta):
    objs, _ = TC._oracle_all(O, X, y, P, eta)
    dense = O.fit_opt(X, y, P, eta=eta, return_all=True)["all_opt"]
    return float(np.max(np.abs(objs - dense) / np.maximum(1.0, np.abs(dense)))), float(objs.min()), float(objs.max())


def main():
    O.build()
    lo = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    hi = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    worst = 0.0
    bad = []
    for c in TC.CASES:
        if not lo <= c["T"] <= hi:
            continue
        t0 = time.time()
        X, y, P, eta = TC._problem(c)
        variants = [("faithful", X, y, P, eta)]
        if c["free_too"]:
            variants.append(("free",) + TC._problem(c, D=c["n"], salt=1))
        Xb, yb, Pb, _ = TC._problem(c, K=c["K_batch"], salt=2)
        N = Xb.shape[0]
        fp = [0, N // 3 | 1, 2 * N // 3 | 1, N]
        for f in range(4):
            tr = np.ones(N, dtype=bool)
            if f < 3:
                tr[fp[f]:fp[f + 1]] = False
            for e in (0.0, 0.3):
                variants.append(("batch f=%d eta=%g" % (f, e), np.asfortranarray(Xb[tr]), yb[tr], Pb, e))
        for name, Xv, yv, Pv, ev in variants:
            err, omin, omax = dense_vs_compressed(Xv, yv, Pv, ev)
            worst = max(worst, err)
            if not err <= 1e-11:
                bad.append((c["id"], name, err))
            print("%-34s %-18s dense vs compressed %.2e  objectives %.4g .. %.4g" % (c["id"], name, err, omin, omax), flush=True)
        ipats, ifrees = _nodes(np.random.default_rng(c["seed"]), P.shape[1] + 1, 12)
        cert = NodeReference(X, y, P, eta).nodes(ipats, ifrees)["certified"]
        if not cert.all():
            bad.append((c["id"], "nodes", int((~cert).sum())))
        print("%-34s nodes certified %d / %d   (%.1f s)" % (c["id"], int(cert.sum()), len(cert), time.time() - t0), flush=True)
    print("worst dense-vs-compressed difference %.3e; failures: %s" % (worst, bad or "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
