"""Which edges of the merged KKT scan the problems of tests/test_gpu_merged_scan.py reach: the CPU emulation of the kernel's decisions
(tools/tableau_emul.py, reference group order, leave-one-out rule) counts, per problem and chain length, the columns rejected as
dependent, the confirming scans at which a rejection still stands (and whether the next pattern's violators would then depend on
ignoring it), and the patterns solved without a pivot.  No GPU.  usage, from the repository root: python tools/merged_scan_edges.py"""
import sys, os
sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "tools")]
import numpy as np
import tableau_emul as E
import test_gpu_merged_scan as M
def run(kind, n, chain_len):
    X, y, P, dead = M.problem(kind, n)
    pr = E.prepare(X, y, P, 0.0)
    nn, T0, mask, kbits, tol = pr["n"], pr["T0"], pr["mask"], pr["kbits"], pr["tol"]
    pol = E.Policy("loo"); pop = lambda v: bin(int(v)).count("1")
    rej = conf_blocked = nopiv = wrong = 0
    npat = 1 << kbits
    for g0 in range(0, npat, chain_len):
        T = T0.copy(); basic = np.zeros(nn, bool); st = dict(T=T, T0=T0, basic=basic, n=nn, growth=1.0, log=[])
        for g in range(g0, min(g0 + chain_len, npat)):
            pat = g ^ (g >> 1)
            f = np.array([2 * pop(int(mask[v]) & pat) - pop(mask[v]) for v in range(nn)])
            blocked = np.zeros(nn, bool); progress = False; piv = 0
            while True:
                if progress: blocked[:] = False
                progress = False
                q = T[:nn, nn]; fq = np.where(f > 0, q, np.where(f < 0, -q, 0.0))
                bad = np.where(basic, (f == 0) | (fq < -tol), (fq > tol) & ~blocked)
                viol = np.nonzero(bad)[0]
                if len(viol) == 0:
                    if blocked.any():
                        conf_blocked += 1
                        # would a next-pattern predicate that honoured `blocked` differ from one that does not?
                        g2 = g + 1; p2 = g2 ^ (g2 >> 1)
                        f2 = np.array([2 * pop(int(mask[v]) & p2) - pop(mask[v]) for v in range(nn)])
                        fq2 = np.where(f2 > 0, q, np.where(f2 < 0, -q, 0.0))
                        a = np.where(basic, (f2 == 0) | (fq2 < -tol), (fq2 > tol)); b = np.where(basic, a, a & ~blocked)
                        wrong += int((a != b).any())
                    break
                for k in viol:
                    if basic[k]: E.pivot(T, k, T[k, k]); basic[k] = False; progress = True; piv += 1
                    elif pol.accept(st, k): E.pivot(T, k, T[k, k]); basic[k] = True; progress = True; piv += 1
                    else: blocked[k] = True; rej += 1
            nopiv += piv == 0
    print(kind, n, "chain", chain_len, ": rejections", rej, "| confirming scans with a blocked column", conf_blocked, "| of which the next pattern's violators depend on ignoring it", wrong, "| patterns without a pivot", nopiv)
for n in (40, 176):
    run("dup", n, 64); run("dup", n, 7); run("null", n, 64)
