"""The rescue rule of csrc/rescue.hip, stated once in numpy: Lawson-Hanson as a pivoting rule on the project's own scaled tableau
(exchange_reference.prepare's T0, its _pivot, the project's tol and PIV_EPS).  TEST INFRASTRUCTURE ONLY (imported by tests; not a
conftest.py, not collected).  Like exchange_reference it pins the RULE, not the arithmetic: one rank-1 sweep per exchanged variable.

Every pattern is solved from the fresh tableau and the empty basis.  q is the rhs column, sgn the sign of the variable's code, x the
last feasible iterate (in the pattern's signs: x >= 0):

    main pass:  candidates = non-basic, code != 0, not blocked, sgn q > tol;  none: converged
                k = the candidate of the largest sgn q (lowest index on ties)
                T[k, k] <= PIV_EPS: blocked += k, a veto, next main pass              (the sweeps' leave-one-out rule)
                pivot k in
    inner loop: s = sgn q over the basic variables
                every s > 0: x = s, blocked cleared, next main pass
                alpha = min over the wrong-signed i of x_i / (x_i - s_i);  x += alpha (s - x)
                pivot out the minimiser and every basic i with x_i <= 0

Main passes are bounded by 3 n (the oracle's itmax); every inner iteration removes a basic variable.  A pattern that runs out of main
passes is unsolved (NaN objective, the kernel's flag).  Converged means exchange_reference's kkt_violates holds for no variable.
"""
import numpy as np

import exchange_reference as E


def default_max_passes(n):
    return 3 * n


def kkt_clean(T, n, f, basic, blocked, tol):
    """csrc/sweep_rules.h kkt_violates<false> is false for every variable"""
    q = T[:n, n]
    fq = q * np.sign(f)
    bad = np.where(basic, (f == 0) | (fq < -tol), (fq > tol) & ~blocked)
    return not bad.any()


def solve_pattern(problem, f, max_passes=None):
    """one pattern from the fresh tableau: dict(solved, obj, sol [n, scaled, 0 for non-basic], passes, pivots, vetoes, clean)"""
    n, tol = problem["n"], problem["tol"]
    T = problem["T0"].copy()
    sgn = np.sign(f).astype(T.dtype)
    basic = np.zeros(n, dtype=bool)
    blocked = np.zeros(n, dtype=bool)
    x = np.zeros(n, dtype=T.dtype)
    limit = default_max_passes(n) if max_passes is None else int(max_passes)
    passes = pivots = vetoes = 0
    solved = False
    while True:
        fq = T[:n, n] * sgn
        cand = ~basic & (f != 0) & ~blocked & (fq > tol)
        if not cand.any():
            solved = True
            break
        if passes >= limit:
            break
        passes += 1
        k = int(np.argmax(np.where(cand, fq, -np.inf)))              # argmax: the first index of the maximum
        if not T[k, k] > E.PIV_EPS:
            blocked[k] = True
            vetoes += 1
            continue
        E._pivot(T, k)
        basic[k] = True
        x[k] = 0
        pivots += 1
        for _ in range(n + 1):                                       # every iteration but the last removes a basic variable
            s = T[:n, n] * sgn
            wrong = basic & ~(s > 0)
            if not wrong.any():
                x = np.where(basic, s, 0)
                blocked[:] = False
                break
            den = x - s
            ratio = np.where(wrong, np.where(den > 0, x / np.where(den > 0, den, 1), 0), np.inf)
            j = int(np.argmin(ratio))                                # the first index of the minimum
            x = np.where(basic, x + ratio[j] * (s - x), 0)
            out = basic & (x <= 0)
            out[j] = True
            for i in np.flatnonzero(out):                            # ascending
                E._pivot(T, int(i))
                basic[i] = False
                x[i] = 0
                pivots += 1
        else:
            raise AssertionError("the inner loop removed nothing")
    o2 = T[n, n]
    clean = solved and kkt_clean(T, n, f, basic, blocked, tol)
    return dict(solved=solved, obj=float(np.sqrt(o2 if o2 > 0 else 0)) if solved else float("nan"),
                sol=np.where(basic, T[:n, n], 0) if solved else np.full(n, np.nan), passes=passes, pivots=pivots, vetoes=vetoes,
                clean=clean)


def solve(problem, patterns, max_passes=None):
    """the listed reference patterns: dict(solved, obj, sol, passes, pivots, vetoes, clean), one entry per pattern"""
    res = [solve_pattern(problem, E.signs(problem, int(p)), max_passes) for p in patterns]
    out = {k: np.array([r[k] for r in res]) for k in ("solved", "obj", "passes", "pivots", "vetoes", "clean")}
    out["sol"] = np.array([r["sol"] for r in res])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The designs beyond exchange_reference's chain cases
# ---------------------------------------------------------------------------------------------------------------------------------
def correlated_throughout():
    """DESIGN.md §7 item 8 (tests/test_gpu_exchange_rule.py::test_design_correlated_throughout): n = 176, K = 5, every column from a
    shared factor; 60 of 64 patterns reach the sweeps' default pivot cap"""
    D, K = 175, 5
    rng = np.random.default_rng(20261176)
    N = 3 * D
    X = rng.standard_normal((N, (D + 1) // 2)) @ rng.standard_normal(((D + 1) // 2, D)) + 0.1 * rng.standard_normal((N, D))
    grp = rng.integers(0, K, D)
    grp[rng.choice(D, K, replace=False)] = np.arange(K)
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    y = X @ (rng.standard_normal(D) * (rng.random(D) < 0.6)) + 0.4 + rng.standard_normal(N)
    return dict(X=np.asfortranarray(X), y=y, P=np.asfortranarray(P), eta=0.0, flags=E.FAITHFUL, faithful=True, n=D + 1, K=K)


def duplicated_column():
    """c40 with a duplicated and a scaled column inside one group: of the first three features a, b, d of the largest group, column b
    becomes column a and column d becomes -2.5 column a"""
    c = dict(E.chain_case("c40"))
    X, P = c["X"].copy(), c["P"]
    grp = np.argmax(P, axis=1)
    big = int(np.argmax(np.bincount(grp)))
    a, b, d = np.flatnonzero(grp == big)[:3]
    X[:, b] = X[:, a]
    X[:, d] = -2.5 * X[:, a]
    c["X"] = np.asfortranarray(X)
    return c


def case(name):
    if name == "correlated":
        return correlated_throughout()
    if name == "c40-dup":
        return duplicated_column()
    return E.chain_case(name)


def case_patterns(name):
    """the reference patterns of a case that the tests solve: all 64, or those of the Gray indices RANGE_297 of c297"""
    if name == E.RANGE_CASE[0]:
        g = np.arange(*E.RANGE_297)
        return g ^ (g >> 1)
    return np.arange(64)


CASES = tuple(E.CHAIN_CASES) + (E.RANGE_CASE[0], "correlated", "c40-dup")
