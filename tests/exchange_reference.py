"""The DECISIONS of the tableau sweep kernels, stated once in numpy: which variables violate KKT (csrc/sweep_rules.h: sign_of_var,
kkt_violates), which of them a round exchanges (ExchangeRule: block principal pivoting, Kim & Park's backup rule after the violator
count has failed to fall for three rounds) and when a pattern gives up (the pivot cap).  TEST INFRASTRUCTURE ONLY (imported by tests;
not a conftest.py, not collected).  It pins the RULE, not the arithmetic: the tableau is a dense symmetric matrix updated by one
rank-1 sweep per exchanged variable, in ascending index order, where the kernels apply blocks of pivots through a panel; the two differ
in round-off only, and the tests that use this module first establish (on the CPU, float64 against long double) that round-off is
orders of magnitude away from every decision of their cases.

Preparation (prepare) restates csrc/prepare.hip ctx_prepare_tableau and csrc/misc.hip prep_scale_entry / prep_tableau_entry:
  augmented Gram of [X 1 y];  G[a][b] += eta * popcount(mask[a] & mask[b]) for a, b <= M (reg_entry);  faithful intercept (the
  intercept is variable M, alone in group K) or the intercept eliminated by a Schur complement, the rhs row included (base_entry);
  variables in a stable sort by the lowest group bit of their mask, 64 for a feature of no group (ctx_prepare_tableau: `key`);
  scale 1 / sqrt(d) where column_is_live(d, raw Gram diagonal), else 0 with a unit diagonal (prepare_rules.h);
  tol = tol_rel * sqrt(y'y) of the raw y (problem_tol, prepare_rules.h), tol_rel = 1e-11;  piv_eps = 1e-11 (SWEEP_PIV_EPS, ctx.h);
  default cap 20 (n + 1) (sweep_max_rounds, ctx.h).  Patterns are visited in the identity bit order: pattern = g ^ (g >> 1).

walk: chain mode.  Chain c of the range [g0, g1) covers g0 + c chain_len .. and starts from the fresh tableau and the empty basis
  (sweep_generic.hip: `T[idx] = p.T0[idx]`, s_basic = 0).  A capped pattern leaves the tableau as it stands and the next pattern of the
  chain starts from it (sweep_generic.hip: `if (step == ExchangeRule::CAPPED) { ++nunconv; break; }`, nothing is restored; the register
  kernel even takes the capped pattern's last scan for the next pattern's first round, sweep_blk.hip: `ninf_best = count2; rounds = 1`,
  which is the same scan because `nxt` has no `blocked` term and a pattern starts with no rejections).
solve: node mode, one node from the fresh tableau and the empty basis, codes -1, 0, +1 and 2 = free (kkt_violates<true>).

Rule holds the four choices a hand-written copy of ExchangeRule could get wrong; MUTANTS are used by the CPU tests to show that their
cases tell each of them from the true rule.
"""
from collections import namedtuple

import numpy as np

TOL_REL = 1e-11
PIV_EPS = 1e-11

Rule = namedtuple("Rule", "patience strict largest cap_ge")
TRUE_RULE = Rule(patience=3, strict=True, largest=True, cap_ge=False)
MUTANTS = {
    "patience 2": TRUE_RULE._replace(patience=2),
    "patience 4": TRUE_RULE._replace(patience=4),
    "<= improvement": TRUE_RULE._replace(strict=False),
    "smallest-index backup": TRUE_RULE._replace(largest=False),
    ">= at the cap": TRUE_RULE._replace(cap_ge=True),
}


def default_max_rounds(n):
    return 20 * (n + 1)


def _popcount(v):
    return bin(int(v)).count("1")


def prepare(X, y, P, eta=0.0, faithful=True, dtype=np.float64):
    """the prepared problem: dict(T0 [(n+1)^2, dtype], n, kbits, mask [n, tableau order], perm, scale, tol, faithful)"""
    X = np.asarray(X, dtype=np.float64)
    N, M = X.shape
    K = P.shape[1]
    Z = np.column_stack([X, np.ones(N), np.asarray(y, dtype=np.float64)]).astype(dtype)
    G = Z.T @ Z
    mask = [0] * (M + 2)
    for v in range(M):
        for k in range(K):
            if P[v, k]:
                mask[v] |= 1 << k
    mask[M] = 1 << K
    raw_diag = np.diag(G).copy()
    yy = G[M + 1, M + 1]
    if eta:
        for a in range(M + 1):
            for b in range(M + 1):
                c = _popcount(mask[a] & mask[b])
                if c:
                    G[a, b] += dtype(eta) * c
    n = M + 1 if faithful else M
    key = [((mask[v] & -mask[v]).bit_length() - 1) if mask[v] else 64 for v in range(n)]
    perm = sorted(range(n), key=lambda v: key[v])                      # sorted() is stable, as std::stable_sort
    idx = perm + [M + 1]
    B = G[np.ix_(idx, idx)].copy()
    if not faithful:
        gI = G[M, idx]
        B -= np.outer(gI, gI) / G[M, M]
    d = np.diag(B)[:n]
    live = (d > 0) & (d > dtype(1e-14) * np.abs(raw_diag[perm]))
    scale = np.where(live, 1 / np.sqrt(np.where(live, d, 1)), 0).astype(dtype)
    s = np.concatenate([scale, np.ones(1, dtype=dtype)])
    T0 = B * s[:, None] * s[None, :]
    for i in range(n):
        if not live[i]:
            T0[i, i] = 1
    tol = dtype(TOL_REL) * np.sqrt(yy if yy > 0 else dtype(0))
    return dict(T0=T0, n=n, kbits=K + 1 if faithful else K, mask=[mask[v] for v in perm], perm=perm, scale=scale,
                tol=tol if tol > 0 else dtype(1e-300), faithful=faithful, dtype=dtype)


def signs(problem, pattern):
    """sign_of_var for every tableau variable: f = 2 popcount(mask & pattern) - popcount(mask)"""
    return np.array([2 * _popcount(m & pattern) - _popcount(m) for m in problem["mask"]], dtype=np.int64)


def tableau_codes(problem, codes):
    """per-variable node codes over the M + 1 homogeneous variables (bnb_reference.node_codes) -> tableau order"""
    assert problem["faithful"]
    return np.asarray(codes, dtype=np.int64)[problem["perm"]]


def _pivot(T, k):
    d = T[k, k]
    inv = 1 / d
    col = T[:, k].copy()
    T -= np.outer(col, col * inv)
    T[:, k] = col * abs(inv)
    T[k, :] = col * abs(inv)
    T[k, k] = -inv
    return d


class _Run:
    """one tableau, one basis, the per-run extremes"""

    def __init__(self, problem, max_rounds, rule, keep_q):
        self.pr, self.rule = problem, rule
        self.n = problem["n"]
        self.max_rounds = default_max_rounds(self.n) if max_rounds is None else int(max_rounds)
        self.tol = problem["tol"]
        self.margin = np.inf            # smallest | |q| - tol | of any tested value
        self.min_d = np.inf             # smallest |d| pivoted on
        self.rejected = 0               # entering pivots with d <= piv_eps
        self.qs = [] if keep_q else None
        self.fresh()

    def fresh(self):
        self.T = self.pr["T0"].copy()
        self.basic = np.zeros(self.n, dtype=bool)

    def pattern(self, code, node):
        """one pattern (or node) from the tableau as it stands: dict(rounds, pivots, backups, capped, obj, viol, picks, backup_rounds)"""
        n, T, basic, tol, rule = self.n, self.T, self.basic, self.tol, self.rule
        isfree = (code == 2) if node else np.zeros(n, dtype=bool)
        f = np.where(isfree, 0, code)
        sgn = np.sign(f).astype(T.dtype)
        tested = isfree | (f != 0)
        blocked = np.zeros(n, dtype=bool)
        best, patience, rounds = n + 1, rule.patience, 0
        out = dict(rounds=0, pivots=0, backups=0, capped=False, viol=[], picks=[], backup_rounds=[])
        progress = False
        while True:
            if progress:
                blocked[:] = False
            progress = False
            q = T[:n, n]
            if self.qs is not None:
                self.qs.append(q.copy())
            fq = q * sgn
            bad = np.where(basic, (f == 0) | (fq < -tol), (fq > tol) & ~blocked)            # kkt_violates
            if node:
                bad = np.where(isfree, ~basic & ~blocked & (np.abs(q) > tol), bad)
            t = tested & ~blocked
            if t.any():
                self.margin = min(self.margin, float(np.min(np.abs(np.abs(q[t]) - tol))))
            viol = np.flatnonzero(bad)
            count = len(viol)
            if count == 0:                                                                  # ExchangeRule::next, in its order
                break
            out["viol"].append(tuple(int(v) for v in viol))
            if (count < best) if rule.strict else (count <= best):
                best, patience, allv = count, rule.patience, True
            elif patience > 0:
                patience -= 1
                allv = True
            else:
                allv = False
            rounds += 1
            if (rounds >= self.max_rounds) if rule.cap_ge else (rounds > self.max_rounds):
                out["capped"] = True
                break
            if not allv:
                viol = viol[-1:] if rule.largest else viol[:1]
                out["backups"] += 1
                out["picks"].append(int(viol[0]))
                out["backup_rounds"].append(rounds)
            out["rounds"] = rounds
            for k in viol:                                                                  # ascending
                if basic[k]:
                    self.min_d = min(self.min_d, abs(float(_pivot(T, k))))
                    basic[k] = False
                elif T[k, k] > PIV_EPS:
                    self.min_d = min(self.min_d, abs(float(_pivot(T, k))))
                    basic[k] = True
                else:
                    self.rejected += 1
                    blocked[k] = True
                    continue
                out["pivots"] += 1
                progress = True
        o2 = T[n, n]
        out["obj"] = float(np.sqrt(o2 if o2 > 0 else 0))
        return out


def _collect(run, pats, extra):
    keys = ("rounds", "pivots", "backups", "capped", "obj", "viol", "picks", "backup_rounds")
    res = {k: [p[k] for p in pats] for k in keys}
    for k in ("rounds", "pivots", "backups"):
        res[k] = np.array(res[k], dtype=np.int64)
    res["capped"] = np.array(res["capped"], dtype=bool)
    res["obj"] = np.array(res["obj"])
    res.update(extra)
    res.update(margin=run.margin, min_d=run.min_d, rejected=run.rejected, qs=run.qs, tol=float(run.tol), max_rounds=run.max_rounds)
    return res


def walk(problem, g0, g1, chain_len, max_rounds=None, dtype=None, rule=TRUE_RULE, keep_q=False):
    """chain mode over the Gray indices [g0, g1) in chains of chain_len.  Per pattern (arrays / lists in visiting order): g, pattern,
    rounds (rounds that exchanged), pivots, backups, capped, obj, viol (the violator set of every round), picks (backup steps' indices),
    backup_rounds, after_capped (the pattern started from a capped predecessor's tableau).  Per run: margin, min_d, rejected, qs."""
    assert dtype is None or dtype == problem["dtype"], "prepare the problem in the dtype of the walk"
    run = _Run(problem, max_rounds, rule, keep_q)
    pats, gs, after = [], [], []
    for c0 in range(g0, g1, chain_len):
        run.fresh()
        prev = False
        for g in range(c0, min(c0 + chain_len, g1)):
            r = run.pattern(signs(problem, g ^ (g >> 1)), node=False)
            pats.append(r)
            gs.append(g)
            after.append(prev)
            prev = r["capped"]
    gs = np.array(gs, dtype=np.int64)
    return _collect(run, pats, dict(g=gs, pattern=gs ^ (gs >> 1), after_capped=np.array(after, dtype=bool)))


def solve(problem, codes, max_rounds=None, dtype=None, rule=TRUE_RULE, keep_q=False):
    """node mode: every row of codes (tableau order: tableau_codes) from the fresh tableau and the empty basis; walk's fields"""
    assert dtype is None or dtype == problem["dtype"], "prepare the problem in the dtype of the solve"
    run = _Run(problem, max_rounds, rule, keep_q)
    pats = []
    for code in np.atleast_2d(np.asarray(codes, dtype=np.int64)):
        run.fresh()
        pats.append(run.pattern(code, node=True))
    return _collect(run, pats, {})


def same_trajectory(a, b):
    """did two runs take the same decisions: the same violator set in every round of every pattern, the same backup picks, the same caps"""
    return a["viol"] == b["viol"] and a["picks"] == b["picks"] and np.array_equal(a["capped"], b["capped"])


def drift(a, b):
    """largest |q_a - q_b| over every scan of two runs of one trajectory (both with keep_q)"""
    assert len(a["qs"]) == len(b["qs"])
    return max(float(np.max(np.abs(x.astype(np.longdouble) - y.astype(np.longdouble)))) for x, y in zip(a["qs"], b["qs"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# The cases: designs on which block principal pivoting stalls.  Independent Gaussian columns never do (0 backup steps, 4-5 rounds per
# pattern); a block of columns of low rank plus noise, embedded among them, does.  N = 3 D rows; the target has weights on the core and
# on 60 % of the rest, an offset of 0.4 and unit noise.  The seeds were picked on the CPU so that every condition of
# tests/test_exchange_reference.py holds; that file asserts them, nothing is filtered at run time.
# ---------------------------------------------------------------------------------------------------------------------------------
FAITHFUL = 1                                                 # PARTLS_OPT_FAITHFUL_INTERCEPT (include/partls.h)
CAPS = (1, 2, 3, 4, 6, 10, 40)                               # the PARTLS_MAX_ROUNDS values of the chain cases


def core_design(seed, D, K, core, rank, overlap=False):
    """(X, y, P): `core` of the D columns are Z (N x rank) @ W (rank x core) + 0.1 E; overlap: four features of two groups (|f| = 2 or
    f = 0) and one feature of no group (f = 0)"""
    rng = np.random.default_rng(seed)
    N = 3 * D
    X = rng.standard_normal((N, D))
    grp = rng.integers(0, K, D)
    grp[rng.choice(D, K, replace=False)] = np.arange(K)                # every group has a feature
    cols = rng.choice(D, core, replace=False)
    X[:, cols] = rng.standard_normal((N, rank)) @ rng.standard_normal((rank, core)) + 0.1 * rng.standard_normal((N, core))
    w = rng.standard_normal(D) * (rng.random(D) < 0.6)
    w[cols] = rng.standard_normal(core)
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    if overlap:
        for m in range(0, 12, 3):
            P[m, (grp[m] + 1) % K] = 1
        P[D - 1] = 0
    y = X @ w + 0.4 + rng.standard_normal(N)
    return np.asfortranarray(X), y, np.asfortranarray(P)


# name: (seed, D, K, flags, eta, overlap) — n = D + 1 with the faithful intercept, n = D without; 64 patterns each
CHAIN_CASES = {
    "c40": (1, 39, 5, FAITHFUL, 0.0, False),
    "c72-eta": (1, 71, 5, FAITHFUL, 0.5, False),
    "c176": (1, 175, 5, FAITHFUL, 0.0, False),
    "c40-free": (1, 40, 6, 0, 0.0, False),
    "c72-overlap": (2, 71, 5, FAITHFUL, 0.0, True),
}
CHAIN_LEN = 7                                                # the chain length the cases were picked at (the GPU tests also walk chains of 64)
GPU_CHAIN_LENS = (7, 64)                                     # the chain lengths of tests/test_gpu_exchange_rule.py
SUB_RANGE = (5, 27)                                          # ... and its sub-range with odd ends
# the deferred-update kernel at its own size: only the Gray indices RANGE_297 of this problem are walked (and emulated)
RANGE_CASE = ("c297", (2, 296, 5, FAITHFUL, 0.0, False))
RANGE_297 = (17, 25)


def chain_case(name):
    seed, D, K, flags, eta, overlap = dict([RANGE_CASE], **CHAIN_CASES)[name]
    X, y, P = core_design(seed, D, K, core=24, rank=12, overlap=overlap)
    return dict(X=X, y=y, P=P, eta=eta, flags=flags, faithful=bool(flags & FAITHFUL), n=D + (flags & FAITHFUL), K=K)


# name: (seed, D, pat, free) — K = 10 groups, a 16-variable core of rank 8, an eighth of the features in a second group (codes 0), one
# or two free groups (codes 2); one node each, solved from the empty basis
NODE_K = 10
NODE_CASES = {
    "n40": (1, 39, 0x3a2, 0x404),
    "n72": (5, 71, 0xc5, 0x10),
    "n176": (5, 175, 0x166, 0x410),
    "n297": (7, 296, 0x63a, 0x1),
    "n331": (11, 330, 0x293, 0x440),
}


def node_case(name):
    seed, D, pat, free = NODE_CASES[name]
    K = NODE_K
    X, y, P = core_design(seed, D, K, core=16, rank=8)
    rng = np.random.default_rng(seed + 5000)
    grp = np.argmax(P, axis=1)
    ex = rng.choice(D, max(2, D // 8), replace=False)
    P[ex, (grp[ex] + 1 + rng.integers(0, K - 1, len(ex))) % K] = 1
    return dict(X=X, y=y, P=np.asfortranarray(P), eta=0.0, n=D + 1, K=K, pat=pat, free=free)
