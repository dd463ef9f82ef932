"""Accuracy of the Gram form on real-valued, uncentred data at full size.

The synthetic generator of BASELINE.md §4 (gauss12) draws integers x 2^-16, so X'X of that data is exact in any summation order
(DESIGN.md §3).  The tests here use numpy Gaussian data instead (deterministic on every platform), uploaded from host memory, and
compare against references more precise than the kernels:

  * the Gram build against `gram_ref`, an error-free split of Z = [X 1 y] into fp64 GEMMs accumulated in long double;
  * the sweep's tracked objective (all_opt) against the QR-compressed oracle (oracle.compress + oracle.opt_patterns), in units of
    y'y: the near-tie window of the sweep (near_tie_rel * y'y on obj^2, ctx.h) assumes that error stays below 1e-13 y'y;
  * fit(Opt) on near ties with uncentred y, where a too narrow window would return another pattern without a word.

Why the compressed oracle is a valid yardstick on uncentred data: it computes each objective from the QR factor of [Xo y], with an
error in obj of about eps * ||y||, i.e. an error in obj^2 of about eps * obj * ||y||.  The Gram form's error in obj^2 is about
eps * y'y.  Measured in units of y'y the oracle is therefore finer by a factor of about ||y|| / obj (~1e5 at an offset of 1e3).

The first two tests run on the CPU (the references' own check); the rest need the MI355X.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from bnb_reference import ld_data_objective as _ld_data_objective

U = 2.0 ** -53                     # unit round-off of fp64
NEAR_TIE_REL = 1e-13               # ctx.h: default width of the sweep's near-tie window, in units of y'y on obj^2

# ---------------------------------------------------------------------------------------------------------------------------------
# High-precision references (host)
# ---------------------------------------------------------------------------------------------------------------------------------
_SPLIT_BITS = 18                   # bits per slice: a product of two slices has <= 36 bits, a block of 2^16 of them stays < 2^53
_SLICES = 4                        # 72 bits per element: the truncated tail is < 2^-72 of the column's largest entry
_BLOCK = 1 << 16


class AugRows:
    """Z = [X 1 y] (N x (M+2)) without materialising it: Z[i0:i1] builds one block of rows."""

    def __init__(self, X, y):
        self.X, self.y = X, y
        self.shape = (X.shape[0], X.shape[1] + 2)

    def __getitem__(self, s):
        xb = self.X[s]
        out = np.empty((xb.shape[0], self.shape[1]))
        out[:, :-2] = xb
        out[:, -2] = 1.0
        out[:, -1] = self.y[s]
        return out


def _slices(Zb):
    """Error-free split of a block: Zb[:, j] = 2^e_j * sum_s S_s[:, j] * 2^(-18 (s+1)) + tail, every S_s an integer array with
    |S_s| <= 2^18 (exact in fp64), |tail| < 2^(e_j - 73).  Returns (stacked slices [s][rows][cols], e)."""
    mx = np.abs(Zb).max(axis=0)
    e = np.frexp(mx)[1].astype(np.int64)                     # max |Zb[:, j]| < 2^e_j
    T = np.ldexp(Zb, -e[None, :])                            # exact: power-of-two scaling
    out = np.empty((_SLICES,) + Zb.shape)
    for s in range(_SLICES):
        T *= 2.0 ** _SPLIT_BITS                              # exact
        np.rint(T, out=out[s])
        T -= out[s]                                          # exact: the fractional part of a representable number
    return out, e


def gram_ref(Z, rows):
    """Rows `rows` of Z'Z, accumulated in np.longdouble (x87 extended, 64-bit mantissa).  Every product sum of one row block is
    formed EXACTLY by fp64 GEMMs on the integer slices of _slices (all partial sums are integers below 2^53, so the GEMM's
    summation order is irrelevant); only the combination of the slice pairs and the blocks rounds, in long double."""
    if np.finfo(np.longdouble).eps > 1.1e-19:
        pytest.skip("np.longdouble is not x87 extended precision on this platform: no reference finer than fp64")
    N, n = Z.shape
    rows = np.asarray(rows, dtype=np.int64)
    acc = np.zeros((len(rows), n), dtype=np.longdouble)
    for i0 in range(0, N, _BLOCK):
        Zb = np.ascontiguousarray(Z[i0:min(N, i0 + _BLOCK)], dtype=np.float64)
        S, e = _slices(Zb)
        L = S[:, :, rows]                                    # [s][rows of the block][sampled rows of G]
        for s in range(_SLICES):
            for t in range(_SLICES):
                P = L[s].T @ S[t]                            # exact integers
                scale = np.ldexp(np.longdouble(1.0), (e[rows][:, None] + e[None, :] - _SPLIT_BITS * (s + t + 2)))
                acc += P.astype(np.longdouble) * scale       # exact product (power of two), one long-double rounding
    return acc


def abs_gram(Z, rows):
    """The matching rows of |Z|'|Z| in fp64: the units of every Gram error bound (the error of a dot product scales with it)."""
    N, n = Z.shape
    rows = np.asarray(rows, dtype=np.int64)
    acc = np.zeros((len(rows), n))
    for i0 in range(0, N, _BLOCK):
        A = np.abs(np.ascontiguousarray(Z[i0:min(N, i0 + _BLOCK)], dtype=np.float64))
        acc += A[:, rows].T @ A
    return acc


def _frac(x):
    """exact rational value of a float64 or long double"""
    return Fraction(*np.longdouble(x).as_integer_ratio())


def _exact(Z, i, j):
    return sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(Z[:, i], Z[:, j])), Fraction(0))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the references' own check (no GPU marker)
# ---------------------------------------------------------------------------------------------------------------------------------
def _selftest_data():
    rng = np.random.default_rng(31)
    N, M = 3000, 12
    scales = np.logspace(-6, 6, M)                           # columns spanning 1e-6 .. 1e6
    X = np.asfortranarray(rng.standard_normal((N, M)) * scales + rng.uniform(-3, 3, M) * scales)
    y = X @ rng.standard_normal(M) + 1e3 + 0.1 * rng.standard_normal(N)
    return X, y


def test_gram_ref_agrees_with_exact_rational_sums():
    X, y = _selftest_data()
    Z = AugRows(X, y)
    Zf = Z[0:Z.shape[0]]
    rows = [0, 5, 11, 12, 13]
    ref = gram_ref(Z, rows)
    A = abs_gram(Z, rows)
    worst = 0.0
    for a, i in enumerate(rows):
        for j in (0, 3, 6, 11, 12, 13):
            ex = _exact(Zf, i, j)
            err = abs(_frac(ref[a, j]) - ex) / Fraction(float(A[a, j]))
            worst = max(worst, float(err))
    assert worst <= 1e-17, "gram_ref off the exact sum by %.3g in units of |Z|'|Z|" % worst
    # a fp64 dot product of the same data is visibly coarser (the reference resolves what the kernels get wrong)
    naive = max(abs(float(Fraction(float(Zf[:, i] @ Zf[:, 11])) - _exact(Zf, i, 11))) / A[a, 11] for a, i in enumerate(rows))
    assert naive > 10 * worst


def test_gram_ref_detects_a_one_ulp_change():
    """One ulp more in one entry of X moves G[4, 9] by ulp * x_9 and G[4, 4] by ~2 ulp * x_4: the reference sees both (centred
    columns: the entries are ~sqrt(N) products, so a one-ulp change is ~1e-18 of them, ten times the long double's resolution)."""
    rng = np.random.default_rng(32)
    X = np.asfortranarray(rng.standard_normal((3000, 12)) * np.logspace(-6, 6, 12))
    y = X @ rng.standard_normal(12) + 0.1 * rng.standard_normal(3000)
    i = int(np.argmax(np.abs(X[:, 4] * X[:, 9])))
    X2 = X.copy(order="F")
    X2[i, 4] = np.nextafter(X2[i, 4], np.inf)
    r1 = gram_ref(AugRows(X, y), [4])[0]
    r2 = gram_ref(AugRows(X2, y), [4])[0]
    for j in (9, 4):
        want = Fraction(float(X2[i, 4])) * Fraction(float(X2[i, j])) - Fraction(float(X[i, 4])) * Fraction(float(X[i, j]))
        got = _frac(r2[j]) - _frac(r1[j])
        assert got != 0 and abs(got - want) <= abs(want) / 10, (j, float(got), float(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def _features(rng, N, M, kind):
    """N x M Fortran-order X.  centred: N(0,1).  uncentred: column means U(-30, 30), scales e^U(-3, 3)."""
    A = rng.standard_normal((M, N))                          # row-major M x N == column-major N x M
    if kind == "uncentred":
        mu = rng.uniform(-30.0, 30.0, M)
        sc = np.exp(rng.uniform(-3.0, 3.0, M))
        A *= sc[:, None]
        A += mu[:, None]
    return A.T


def _target(rng, X, w, offset):
    return X @ w + offset + 0.1 * rng.standard_normal(X.shape[0])


def _problem(seed, N, M, kind, w=None):
    rng = np.random.default_rng(seed)
    X = _features(rng, N, M, kind)
    if w is None:
        w = rng.standard_normal(M)
    y = _target(rng, X, w, 1e3 if kind == "uncentred" else 0.0)
    return X, y


def _gram(partls, ctx, M):
    """the context's augmented Gram (partls_get_gram) whatever call prepared it (fit(Alt) does not record a shape in Python)"""
    G = np.zeros((M + 2, M + 2), order="F")
    assert partls.lowlevel.lib().partls_get_gram(ctx._h, G.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return G


# ---------------------------------------------------------------------------------------------------------------------------------
# §2  the Gram build on real-valued data
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_gram(partls, X, y, tag):
    N, M = X.shape
    P, _ = partls.synth_truth(7, M, 4)
    ctx = partls.Context(0)
    try:
        ctx.opt_prepare(X, y, P, 0.0, 0)
        G = _gram(partls, ctx, M)
    finally:
        ctx.close()
    rows = np.unique(np.concatenate([[0, 127, 128, M - 1, M, M + 1],
                                     np.random.default_rng(N + M).choice(M, 2, replace=False)]))
    Z = AugRows(X, y)
    ref = gram_ref(Z, rows)
    A = abs_gram(Z, rows)
    assert G[M, M] == N, "G[ones, ones] = %r, not N = %d: a row or panel was dropped or doubled" % (G[M, M], N)
    err = np.abs(G[rows, :].astype(np.longdouble) - ref).astype(np.float64)
    rig = err / (N * U * A)
    assert rig.max() <= 1.0, "%s: |G - G_ref| exceeds N u |Z|'|Z| (no summation order does that): worst %.3g at %s" % (
        tag, rig.max(), np.unravel_index(np.argmax(rig), rig.shape))
    tight = (err / A).max() / (U * math.sqrt(N))
    assert tight <= 16.0, "%s: max |G - G_ref| / |Z|'|Z| = %.3g u sqrt(N) (> 16)" % (tag, tight)
    print("[gram] %s: max |G - G_ref| / |Z|'|Z| = %.3g u sqrt(N)" % (tag, tight))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["centred", "uncentred"])
@pytest.mark.parametrize("N,M", [(100_000, 256), (100_003, 300), (1_000_000, 260)])
def test_gram_real_data(partls, N, M, kind):
    """(100k, 256): C3 plan; (100 003, 300): partial panel, partial chunk and an edge tile; (1M, 260): the C4 slice plan."""
    X, y = _problem(1000 + M + (kind == "uncentred"), N, M, kind)
    _check_gram(partls, X, y, "N=%d M=%d %s" % (N, M, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("S,CR", [(1, 16), (7, 4096), (3, 1008)])
def test_gram_real_data_forced_plans(partls, monkeypatch, S, CR):
    """Planner overrides (a Context reads them when it is created): one slice of 16-row chunks, more slices than 4096-row chunks
    leave room for ("no more slices than chunks"), and a chunk that is not a power of two."""
    monkeypatch.setenv("PARTLS_GRAM_S", str(S))
    monkeypatch.setenv("PARTLS_GRAM_CR", str(CR))
    X, y = _problem(1257, 100_000, 256, "uncentred")
    _check_gram(partls, X, y, "S=%d CR=%d" % (S, CR))


# ---------------------------------------------------------------------------------------------------------------------------------
# §3  the tracked objective against the near-tie window
# ---------------------------------------------------------------------------------------------------------------------------------
_last_compressed = {}


def _compressed_oracle(oracle, X, y, P, key=None):
    """(Xo, Po, R, z): homogeneous coordinates and the QR-compressed problem; the last one is kept for the next call with the same key"""
    if key is not None and key in _last_compressed:
        return _last_compressed[key]
    Xo, Po = oracle.homogeneous(X, P)
    R, z = oracle.compress(Xo, y)
    _last_compressed.clear()
    if key is not None:
        _last_compressed[key] = (Xo, Po, R, z)
    return Xo, Po, R, z


def _yy(y):
    return float(np.dot(y.astype(np.longdouble), y.astype(np.longdouble)))


SHAPES = {                          # name: (N, D, K, flags beyond FAITHFUL_INTERCEPT)
    "c3": (100_000, 256, 20, 0),             # 512-thread register kernel
    "d340": (20_000, 340, 10, 0),            # deferred-update kernel
    "d60_generic": (20_000, 60, 12, 2),      # PARTLS_OPT_GENERIC_KERNEL
}


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [None, 8192])
@pytest.mark.parametrize("shape,kind", [("c3", "centred"), ("c3", "uncentred"), ("d340", "uncentred"), ("d60_generic", "uncentred")])
def test_tracked_objective_vs_near_tie_window(partls, oracle, monkeypatch, shape, kind, chain):
    N, D, K, extra = SHAPES[shape]
    monkeypatch.setenv("PARTLS_BIT_ORDER", "identity")
    if chain is None:
        monkeypatch.delenv("PARTLS_CHAIN_LEN", raising=False)
    else:
        monkeypatch.setenv("PARTLS_CHAIN_LEN", str(chain))
    seed = 4000 + D + (kind == "uncentred")
    P, ws = partls.synth_truth(seed, D, K)
    X, y = _problem(seed, N, D, kind, w=ws)
    ctx = partls.Context(0)
    try:
        ctx.opt_prepare(X, y, P, 0.0, partls.lowlevel.OPT_FAITHFUL_INTERCEPT | extra)
        bo, bp, allopt, unconv = ctx.opt_sweep(0, -1, want_all=True)
        assert unconv == 0 and not np.isnan(allopt).any()
        npat = ctx.num_patterns()
        # chain c covers Gray indices [c L, (c+1) L): its last index carries the longest warm-started path.  Without an override the
        # sweep plan picks a power of two <= 2048 that divides npat / 32 on these shapes, so the ends of chains of L below are ends too
        L = chain if chain is not None else min(2048, npat // 32)
        L = min(L, npat)
        rng = np.random.default_rng(seed)
        ends = (rng.choice(npat // L, min(32, npat // L), replace=False) + 1) * L - 1
        gray = [int(ctx.opt_models(int(g), int(g) + 1)["pattern"][0]) for g in ends]
        pats = np.unique(np.concatenate([gray, rng.integers(0, npat, 32), [bp]])).astype(np.int64)
        if shape == "c3":
            a, b, t, opt, bi = ctx.opt_finish(bp)
            kkt = ctx.kkt_violation()
    finally:
        ctx.close()
    Xo, Po, R, z = _compressed_oracle(oracle, X, y, P, (shape, kind))
    ref = oracle.opt_patterns(R, z, Po, pats)
    yy = _yy(y)
    d2 = np.abs(allopt[pats] ** 2 - ref ** 2) / yy
    worst = d2.max()
    msg = "%s %s chain=%s: max |obj^2 - ref^2| = %.3g u y'y (window %.3g u y'y; pattern %d)" % (
        shape, kind, chain, worst / U, NEAR_TIE_REL / U, pats[np.argmax(d2)])
    print("[tracked] " + msg)
    assert worst <= NEAR_TIE_REL, msg
    if kind == "centred":
        np.testing.assert_allclose(allopt[pats], ref, rtol=1e-9)
    if shape == "c3":
        dense = oracle.opt_patterns(Xo, y, Po, np.array([bi], dtype=np.int64))[0]
        assert abs(opt - dense) <= 1e-9 * dense, (opt, dense)
        assert kkt <= 1e-12, kkt


# ---------------------------------------------------------------------------------------------------------------------------------
# §4  near ties with uncentred y
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def near_tie_base(partls):
    seed, N, D, K = 20260003, 100_000, 256, 20
    P, ws = partls.synth_truth(seed, D, K)
    grp = np.argmax(P, axis=1)
    beta = np.array([ws[grp == k].sum() for k in range(K)])
    rng = np.random.default_rng(seed)
    null = set(rng.choice(K, 4, replace=False).tolist()) | set(np.flatnonzero(np.abs(beta) < 0.5).tolist())
    w = ws.copy()
    for k in null:
        w[grp == k] = 0.0
    X = _features(rng, N, D, "centred")
    Xw = X @ w
    noise = 0.1 * rng.standard_normal(N)
    return dict(X=X, Xw=Xw, noise=noise, P=P, beta=beta, null=sorted(null), K=K)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0.0, 1e2, 1e4, 1e5])
def test_near_ties_uncentred_target(partls, oracle, near_tie_base, offset):
    """C3 shape with groups that carry no signal: the minimum is among the planted signs x every sign of the null groups (and of the
    intercept at offset 0).  fit(Opt) must return it (objective from the data, so a worse pattern cannot pass) in both intercept modes
    and sharded over two ranks; an uncentred y widens the near-tie window relative to obj^2 (1e-13 y'y is 1e-3 of obj^2 at offset 1e4, 0.1 at 1e5)."""
    d = near_tie_base
    X, P, K, null = d["X"], d["P"], d["K"], d["null"]
    y = d["Xw"] + offset + d["noise"]
    planted = sum(1 << k for k in range(K) if k not in null and d["beta"][k] > 0)
    icpt = [1] if offset > 0 else [0, 1]                       # a positive offset forces the intercept's sign
    cand = np.array(sorted(planted | sum(1 << null[i] for i in range(len(null)) if (m >> i) & 1) | (ib << K)
                           for m in range(1 << len(null)) for ib in icpt), dtype=np.int64)
    Xo, Po, R, z = _compressed_oracle(oracle, X, y, P)
    ref = oracle.opt_patterns(R, z, Po, cand)
    order = np.argsort(ref, kind="stable")
    best, second = ref[order[0]], ref[order[1]]
    argbest = int(cand[order[0]])
    gap = (second - best) / best
    rnd = np.random.default_rng(int(offset) + 1).integers(0, 1 << (K + 1), 64)
    ref_rnd = oracle.opt_patterns(R, z, Po, rnd)
    assert ref_rnd.min() >= best * (1 - 1e-12), "a random pattern beats the planted set: the set is not where the minimum is"
    tau = 1e-12 + 16 * U * float(np.linalg.norm(y)) / best
    kmask = (1 << K) - 1
    for label, kw in (("faithful", dict(faithful_intercept=True)), ("free", {}), ("multi[0,0]", dict(devices=[0, 0]))):
        _, _, rep = partls.fit(partls.Opt, X, y, P, on_ill_conditioned="raise", **kw)
        owner = partls.default_multi([0, 0]).context(0) if "devices" in kw else partls.default_context()
        nt = owner.near_ties_evaluated()
        msg = "offset %g %s: opt %.17g, oracle min %.17g (pattern %d), gap to 2nd %.3g, tau %.3g, best_index %d, near ties %d, null %s" % (
            offset, label, rep.opt, best, argbest, gap, tau, rep.best_index, nt, null)
        print("[near-tie] " + msg)
        assert rep.opt <= best * (1 + tau), msg
        # free intercept at offset 0: bit K comes from the sign of the fitted intercept, which may sit at zero
        mask = kmask if (offset == 0 and label != "faithful") else -1
        ok = [int(cand[order[0]]) & mask] + ([int(cand[order[1]]) & mask] if gap <= 100 * tau else [])
        assert rep.best_index & mask in ok, msg


# ---------------------------------------------------------------------------------------------------------------------------------
# §5  C4 size on real data
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_c4_alt_real_data(partls):
    """fit(Alt) at BASELINE config 4's size (N = 1M, D = 512, K = 16) on numpy Gaussian data from host memory (4.1 GB: the staged
    upload): the returned objective equals the one recomputed from the data in long double; the Gram agrees with the data."""
    seed, N, D, K = 20260004, 1_000_000, 512, 16
    P, ws = partls.synth_truth(seed, D, K)
    rng = np.random.default_rng(seed)
    X = _features(rng, N, D, "centred")
    y = _target(rng, X, ws, 1.0)
    r0 = np.random.default_rng(123)
    a0 = r0.random(D + 1); b0 = (r0.random(K + 1) - 0.5) * 10
    m, _, rep = partls.fit(partls.Alt, X, y, P, ϵ=1e-6, T=200, alpha0=a0, beta0=b0, on_ill_conditioned="raise")
    grp = np.argmax(P, axis=1)
    w = m.α * m.β[grp]
    ref = _ld_data_objective(X, y, w, m.t)
    assert abs(rep.opt - ref) <= 1e-9 * ref, (rep.opt, ref)
    assert rep.opt < 1.5 * 0.1 * np.sqrt(N)
    # the same Gram-versus-data check test_c4_full_size_alt makes, with its tolerances
    G = _gram(partls, partls.default_context(), D)
    wo = np.concatenate([w, [m.t]])
    obj = np.sqrt(wo @ G[:D + 1, :D + 1] @ wo - 2 * wo @ G[:D + 1, D + 1] + G[D + 1, D + 1])
    assert abs(obj - rep.opt) <= 1e-8 * rep.opt
    cols = [0, 1, 255, 256, 510, 511]
    np.testing.assert_allclose(G[cols, :D], X[:, cols].T @ X, rtol=1e-11, atol=1e-6)
