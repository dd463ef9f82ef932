"""Helpers of the tests on 32- to 40-bit pattern spaces (test_gpu_wide_patterns.py, checked on the CPU by test_wide_reference.py).
TEST INFRASTRUCTURE ONLY (imported by tests; not a conftest.py, not collected).

Index arithmetic in plain Python ints (no numpy shifts, whose width depends on the dtype), the problem generator, a cache of the
oracle's per-pattern results, and the one gate through which the GPU tests call opt_sweep / opt_models: a full sweep of 2^40 patterns
would keep a card busy for half a day and a running kernel cannot be stopped from Python, so the gate admits short ranges only."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

MAX_RANGE = 4096


def gray(g):
    """Gray index -> internal sign pattern (the pattern the sweep visits at position g)"""
    g = int(g)
    return g ^ (g >> 1)


def gray_inverse(q):
    """internal sign pattern -> its Gray index, by prefix xor: bit i of g = xor of the bits >= i of q"""
    q = int(q)
    g = 0
    while q:
        g ^= q
        q >>= 1
    return g


def reference_index(q, gbit):
    """internal pattern (group k on bit gbit[k]) -> the reference's pattern index (group k on bit k)"""
    q = int(q)
    return sum(((q >> int(gbit[k])) & 1) << k for k in range(len(gbit)))


def internal_pattern(b, gbit):
    """the inverse of reference_index"""
    b = int(b)
    return sum(((b >> k) & 1) << int(gbit[k]) for k in range(len(gbit)))


def guarded(ctx, call, g0, g1, **kw):
    """THE way the wide tests run ctx.opt_sweep / ctx.opt_models: an explicit range of at most MAX_RANGE indices inside the space"""
    assert call in ("opt_sweep", "opt_models"), call
    g0, g1 = int(g0), int(g1)
    assert 0 <= g0 < g1 <= ctx.num_patterns(), (g0, g1)
    assert g1 - g0 <= MAX_RANGE, (g0, g1)
    assert not kw.get("want_all"), "want_all allocates 2^kbits doubles on the host"
    return getattr(ctx, call)(g0, g1, **kw)


def problem(seed, D, K, empty=None):
    """(X, y, P): Gaussian X, N = 3 D + 40, one group per feature, every group used (feature k < K sits in group k) unless `empty`
    names a group that gets no feature.  The surplus features D - K all go to groups 0-7, and only those groups carry large true
    weights (x 3 against x 0.1): flipping one of them costs clearly more pivots than flipping a group >= 8, so a measured bit order
    moves groups 8 .. K - 1 to the fast bits and groups 0-7 to the slow ones.  Sparse weights (density 0.6; the first feature of
    groups 0-7 always carries one), intercept 0.4, noise 0.3."""
    rng = np.random.default_rng(seed)
    N = 3 * D + 40
    X = rng.standard_normal((N, D))
    grp = np.concatenate([np.arange(K), rng.integers(0, 8, size=D - K)])
    if empty is not None:
        assert empty >= 8
        grp[grp == empty] = empty % 8
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    keep = rng.random(D) < 0.6
    keep[:8] = True
    w = rng.standard_normal(D) * keep
    w[:8] = np.where(np.abs(w[:8]) < 0.3, 0.3 * np.where(w[:8] < 0, -1.0, 1.0), w[:8])
    w *= np.where(grp < 8, 3.0, 0.1)
    y = X @ w + 0.4 + 0.3 * rng.standard_normal(N)
    return np.asfortranarray(X), y, np.asfortranarray(P)


class OracleCache:
    """The oracle's view of one problem: oracle.homogeneous + oracle.compress once, per-pattern results (objective and nonneg_lsq's
    alpha on the QR-compressed data, Opt.jl:87-90) computed once per pattern and kept.  Patterns index the homogeneous problem:
    bit k = group k, bit K = the intercept's group (41 bits at K = 40)."""

    def __init__(self, oracle, X, y, P):
        self.oracle, self.X, self.y, self.P = oracle, X, y, P
        self.Xo, self.Po = oracle.homogeneous(X, P)
        self.R, self.z = oracle.compress(self.Xo, y)
        self.ynorm = max(1.0, float(np.linalg.norm(y)))
        self._rows = {}

    def rows(self, patterns):
        """(objectives[B], raw_alpha[B, M + 1]) of the listed patterns"""
        pats = [int(b) for b in patterns]
        todo = sorted(set(pats) - set(self._rows))
        if todo:
            parts = [todo[i::8] for i in range(8) if todo[i::8]]                 # independent solves; the oracle keeps no state
            with ThreadPoolExecutor(len(parts)) as ex:
                res = list(ex.map(lambda p: self.oracle.opt_patterns(self.R, self.z, self.Po, np.array(p, dtype=np.int64), want_alpha=True), parts))
            for p, (o, ra) in zip(parts, res):
                for i, b in enumerate(p):
                    self._rows[b] = (float(o[i]), ra[i].copy())
        return np.array([self._rows[b][0] for b in pats]), np.stack([self._rows[b][1] for b in pats])

    def data_objective(self, b):
        """the pattern's objective from the uncompressed data (what a finished model reports)"""
        return float(self.oracle.opt_patterns(self.Xo, self.y, self.Po, np.array([int(b)], dtype=np.int64))[0])


_CACHE = {}


def cached(oracle, name, seed, D, K, empty=None):
    """the OracleCache of a named problem, built once per session"""
    if name not in _CACHE:
        _CACHE[name] = OracleCache(oracle, *problem(seed, D, K, empty))
    return _CACHE[name]
