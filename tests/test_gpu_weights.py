"""Sample weights on the GPU: unit weights reproduce the unweighted path bit for bit (Opt on every sweep kernel, BnB,
Alt, the Gram, cross_validate); the weighted Gram against (S Z)'(S Z) in float64 over ragged shapes and panel / chunk edges; every
pattern's objective and the winner against the oracle on S-scaled data with the η rows unweighted; integer weights against row
replication; zero weights against dropped rows; BnB against the weighted Opt; the bulk model export; device weights against host
weights (bitwise) and their device-side argument errors; weighted cross-validation against single weighted fits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAITHFUL = 1


def _problem(seed, N, M, K, spread=True):
    """real-valued, uncentred data; weights over about three decades"""
    rng = np.random.default_rng(seed)
    X = rng.normal(1.0, 1.0, size=(N, M))
    grp = np.concatenate([np.arange(K), rng.integers(0, K, M - K)]) if M >= K else np.arange(M) % K
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), grp] = 1
    ws = rng.normal(0.0, 1.0, M)
    y = X @ ws + 2.0 + 0.3 * rng.normal(size=N)
    w = 10.0 ** rng.uniform(-1.5, 1.5, N) if spread else np.ones(N)
    return X, y, P, w


def _close(a, ref, tol):
    a, ref = np.asarray(a, dtype=float), np.asarray(ref, dtype=float)
    sc = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    assert np.all(np.abs(a - ref) <= tol * sc), f"max abs error {np.abs(a - ref).max():.3e} (scale {sc:.3e})"


def _same_fit(r1, r2):
    (m1, _, p1), (m2, _, p2) = r1, r2
    assert np.array_equal(m1.α, m2.α) and np.array_equal(m1.β, m2.β) and m1.t == m2.t
    for k in ("opt", "best_index", "nopen", "iters"):
        if k in p2:
            assert p1[k] == p2[k], k


def _weighted_obj(X, y, P, model, w, eta):
    """sqrt(sum_i w_i r_i^2 + the eta rows of regularizeProblem) of a cleaned model"""
    a, b, t = model.α, model.β, model.t
    r = X @ (a * (P @ b)) + t - y
    s = float(np.sum(w * r * r))
    if eta:
        wv = a * (P @ b)
        s += eta * (float(np.sum((P.T @ wv) ** 2)) + t * t)
    return np.sqrt(s)


# ---- 1. unit weights are the unweighted path, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,K,generic", [(600, 24, 4, False), (700, 300, 2, False), (500, 20, 3, True)])
def test_unit_weights_opt_bitwise(partls, N, M, K, generic):
    X, y, P, _ = _problem(11 + M, N, M, K)
    one = np.ones(N)
    for eta in (0.0, 0.7):
        _same_fit(partls.fit(partls.Opt, X, y, P, η=eta, generic_kernel=generic, weights=one),
                  partls.fit(partls.Opt, X, y, P, η=eta, generic_kernel=generic))
    if M <= 64:
        _, _, ra = partls.fit(partls.Opt, X, y, P, returnAllSolutions=True, generic_kernel=generic, weights=one)
        _, _, rb = partls.fit(partls.Opt, X, y, P, returnAllSolutions=True, generic_kernel=generic)
        assert np.array_equal(ra.solutions._all, rb.solutions._all)


def test_unit_weights_bnb_alt_gram_bitwise(partls):
    X, y, P, _ = _problem(5, 800, 30, 4)
    one = np.ones(len(y))
    _same_fit(partls.fit(partls.BnB, X, y, P, η=0.2, weights=one), partls.fit(partls.BnB, X, y, P, η=0.2))
    rng = np.random.default_rng(3)
    a0, b0 = rng.random(31), (rng.random(5) - 0.5) * 10
    _same_fit(partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0, weights=one), partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0))
    ctx = partls.Context(0)
    ctx.opt_prepare(X, y, P, 0.0, weights=one)
    G1 = ctx.gram()
    ctx.opt_prepare(X, y, P, 0.0)
    assert np.array_equal(G1, ctx.gram())
    ctx.close()


def test_unit_weights_cross_validate_bitwise(partls):
    X, y, P, _ = _problem(8, 500, 14, 3)
    kw = dict(η=[0.0, 0.3, 2.0], nfolds=4, shuffle=True, rng=5)
    a = partls.cross_validate(partls.Opt, X, y, P, weights=np.ones(len(y)), **kw)
    b = partls.cross_validate(partls.Opt, X, y, P, **kw)
    for k in ("etas", "fold_ptr", "perm", "sse", "mse", "mse_mean", "opt", "best_index", "status", "ill_conditioned"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=k not in ("perm", "fold_ptr", "best_index", "status",
                                                                                "ill_conditioned")), k
    assert a.best_eta == b.best_eta and a.best_index_eta == b.best_index_eta
    for fa, fb in zip(a.folds, b.folds):
        assert np.array_equal(fa, fb)
    for ma, mb in zip([m for row in a.models for m in row] + a.path + [a.model], [m for row in b.models for m in row] + b.path + [b.model]):
        assert np.array_equal(ma.α, mb.α) and np.array_equal(ma.β, mb.β) and ma.t == mb.t


# ---- 2. the weighted Gram against float64 --------------------------------------------------------------------------------------
def _ref_gram(X, y, w):
    s = np.sqrt(w)
    Z = np.hstack([X, np.ones((len(y), 1)), y[:, None]]) * s[:, None]
    return Z.T @ Z


def _gram_check(ctx, X, y, P, w):
    ctx.opt_prepare(X, y, P, 0.0, weights=w)
    G = ctx.gram()
    R = _ref_gram(X, y, w)
    d = np.sqrt(np.outer(np.diag(R), np.diag(R)))
    err = np.abs(G - R)
    assert np.all(err <= 1e-12 * d + 1e-300), f"N={len(y)} M={X.shape[1]}: worst {np.max(err / np.maximum(d, 1e-300)):.3e}"


def test_weighted_gram_against_float64(partls):
    ctx = partls.Context(0)
    rng = np.random.default_rng(21)
    for M in (1, 127, 128, 129, 300):
        P = np.ones((M, 1), dtype=np.int64)
        for N in (1, 15, 17, 4097):
            X = rng.normal(1.0, 1.0, (N, M))
            y = X @ rng.normal(size=M) + 1.0 + rng.normal(size=N)
            w = 10.0 ** rng.uniform(-1.5, 1.5, N)
            # zero weights on first / last rows of 16-sample panels (chunks are whole panels): the edges of both
            edge = np.flatnonzero((np.arange(N) % 16 == 0) | (np.arange(N) % 16 == 15))
            w[edge[rng.random(len(edge)) < 0.6]] = 0.0
            w[0] = 0.0 if N > 1 else 2.5
            if N > 1:
                w[-1] = 0.0
            _gram_check(ctx, X, y, P, w)
            if N == 4097:
                ctx.opt_prepare(X, y, P, 0.0, weights=np.full(N, 4.0))
                G4 = ctx.gram()
                ctx.opt_prepare(X, y, P, 0.0)
                assert np.array_equal(G4, 4.0 * ctx.gram()), f"M={M}: constant weights 4 are not exactly 4 G"
    N, M = 200_000, 129
    X = rng.normal(1.0, 1.0, (N, M))
    y = X @ rng.normal(size=M) + 1.0 + rng.normal(size=N)
    w = 10.0 ** rng.uniform(-1.5, 1.5, N)
    w[rng.random(N) < 0.05] = 0.0
    _gram_check(ctx, X, y, np.ones((M, 1), dtype=np.int64), w)
    ctx.close()


# ---- 3. against the oracle, with no oracle change: S-scaled homogeneous data, η rows unweighted ----------------------------------
def _oracle_weighted(oracle, X, y, P, w, eta):
    Xo, Po = oracle.homogeneous(X, P)
    s = np.sqrt(w)
    Xn, yn = oracle.regularize(np.asfortranarray(Xo * s[:, None]), y * s, Po, eta)
    return Xn, yn, Po


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("eta", [0.0, 0.8])
def test_every_pattern_against_the_oracle(partls, oracle, seed, eta):
    X, y, P, w = _problem(100 + seed, 400, 11, 3)
    Xn, yn, Po = _oracle_weighted(oracle, X, y, P, w, eta)
    npat = 1 << (P.shape[1] + 1)
    objs = oracle.opt_patterns(Xn, yn, Po, np.arange(npat))
    _, _, rep = partls.fit(partls.Opt, X, y, P, η=eta, weights=w, returnAllSolutions=True)
    allopt = np.asarray(rep.solutions._all)
    yw = np.sqrt(float(np.sum(w * y * y)))
    assert np.all(np.abs(allopt - objs) <= 1e-9 * objs + 1e-13 * yw), np.max(np.abs(allopt - objs) / objs)
    order = np.argsort(objs)
    model, _, r = partls.fit(partls.Opt, X, y, P, η=eta, weights=w, faithful_intercept=True)
    if objs[order[1]] - objs[order[0]] > 1e-6 * objs[order[0]]:        # clearly separated: the winner is determined
        assert r.best_index == order[0]
    assert abs(r.opt - objs[order[0]]) <= 1e-9 * objs[order[0]]
    assert abs(_weighted_obj(X, y, P, model, w, eta) - r.opt) <= 1e-9 * r.opt


# ---- 4 / 5. integer weights = replicated rows, zero weights = dropped rows ------------------------------------------------------------
def _agree(partls, X, y, P, w, Xr, yr, eta):
    for alg in (partls.Opt, partls.BnB):
        m1, _, r1 = partls.fit(alg, X, y, P, η=eta, weights=w)
        m2, _, r2 = partls.fit(alg, Xr, yr, P, η=eta)
        sc = max(1.0, np.abs(m2.α).max(), np.abs(m2.β).max(), abs(m2.t))
        _close(m1.α, m2.α, 1e-9 * sc); _close(m1.β, m2.β, 1e-9 * sc)
        assert abs(m1.t - m2.t) <= 1e-9 * sc
        assert abs(r1.opt - r2.opt) <= 1e-10 * r2.opt, (alg, r1.opt, r2.opt)
        if alg is partls.Opt:
            assert r1.best_index == r2.best_index
    rng = np.random.default_rng(9)
    a0, b0 = rng.random(X.shape[1] + 1), (rng.random(P.shape[1] + 1) - 0.5) * 10
    _, _, r1 = partls.fit(partls.Alt, X, y, P, η=eta, alpha0=a0, beta0=b0, weights=w)
    _, _, r2 = partls.fit(partls.Alt, Xr, yr, P, η=eta, alpha0=a0, beta0=b0)
    assert abs(r1.opt - r2.opt) <= 1e-8 * r2.opt, (r1.opt, r2.opt)


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_integer_weights_are_replicated_rows(partls, eta):
    X, y, P, _ = _problem(41, 500, 16, 3)
    w = np.random.default_rng(42).integers(0, 4, len(y))
    _agree(partls, X, y, P, w.astype(np.float64), np.repeat(X, w, axis=0), np.repeat(y, w), eta)


def test_zero_weights_drop_rows(partls):
    X, y, P, _ = _problem(43, 600, 16, 3)
    keep = np.random.default_rng(44).random(len(y)) < 0.7
    _agree(partls, X, y, P, keep.astype(np.float64), X[keep], y[keep], 0.3)


# ---- 6. BnB reaches the weighted Opt optimum ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [51, 52])
def test_bnb_reaches_the_weighted_opt(partls, seed):
    X, y, P, w = _problem(seed, 700, 20, 4)
    mo, _, ro = partls.fit(partls.Opt, X, y, P, η=0.1, weights=w)
    mb, _, rb = partls.fit(partls.BnB, X, y, P, η=0.1, weights=w)
    assert abs(rb.opt - ro.opt) <= 1e-10 * ro.opt
    sc = max(1.0, np.abs(mo.α).max(), np.abs(mo.β).max(), abs(mo.t))
    assert abs(mb.t - mo.t) <= 1e-9 * sc
    _close(mb.α, mo.α, 1e-9 * sc); _close(mb.β, mo.β, 1e-9 * sc)


# ---- 7. the bulk model export is weighted ------------------------------------------------------------------------------------------
def test_bulk_export_is_weighted(partls, oracle):
    X, y, P, w = _problem(61, 500, 12, 3)
    eta = 0.4
    Xn, yn, Po = _oracle_weighted(oracle, X, y, P, w, eta)
    _, _, rep = partls.fit(partls.Opt, X, y, P, η=eta, weights=w, returnAllSolutions=True)
    opt, alpha, beta, t = rep.solutions.arrays()
    npat = len(opt)
    objs, ra = oracle.opt_patterns(Xn, yn, Po, np.arange(npat), want_alpha=True)
    M, K = P.shape
    assert np.all(np.abs(opt - objs) <= 1e-9 * objs)
    for b in range(npat):
        a_r = ra[b][:M]
        s = np.array([1.0 if (b >> k) & 1 else -1.0 for k in range(K)])
        sums = P.T @ a_r
        beta_r = s * sums
        A = np.where(sums == 0.0, 1.0, sums)
        alpha_r = (P * (a_r[:, None] / A[None, :])).sum(axis=1)
        t_r = (1.0 if (b >> K) & 1 else -1.0) * ra[b][M]
        sc = max(1.0, np.abs(beta_r).max(), abs(t_r))
        assert np.all(np.abs(beta[b] - beta_r) <= 1e-9 * sc), (b, beta[b], beta_r)
        assert abs(t[b] - t_r) <= 1e-9 * sc, (b, t[b], t_r)
        assert np.all(np.abs(alpha[b] - alpha_r) <= 1e-9 * max(1.0, np.abs(alpha_r).max())), (b, alpha[b], alpha_r)


# ---- 8. device weights ------------------------------------------------------------------------------------------------------------
def test_device_weights_bitwise_and_errors(partls):
    import torch
    X, y, P, w = _problem(71, 900, 18, 3)
    N, M = X.shape
    ldX = N + 37
    dX = torch.zeros((M, ldX), dtype=torch.float64, device="cuda")       # column-major, padded leading dimension
    dX[:, :N] = torch.from_numpy(np.ascontiguousarray(X.T))
    dy = torch.from_numpy(y.copy()).cuda()
    dw = torch.from_numpy(w.copy()).cuda()
    torch.cuda.synchronize()
    for eta, flags in ((0.0, 0), (0.6, FAITHFUL)):
        h = partls.Context(0)
        h.opt_prepare(X, y, P, eta, flags, weights=w)
        rh = h.opt_sweep(0, -1, want_all=bool(flags))
        fh = h.opt_finish(rh[1])
        d = partls.Context(0)
        d.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, M, ldX, P, eta, flags, dw_ptr=dw.data_ptr())
        rd = d.opt_sweep(0, -1, want_all=bool(flags))
        fd = d.opt_finish(rd[1])
        assert np.array_equal(h.gram(), d.gram())
        assert rh[0] == rd[0] and rh[1] == rd[1] and (not flags or np.array_equal(rh[2], rd[2]))
        for u, v in zip(fh, fd):
            assert np.array_equal(np.asarray(u), np.asarray(v))
        h.close()
        # device-side argument errors: nothing prepared afterwards
        for bad, status in ((-1.0, partls.lowlevel.ERR_BAD_ARG), (float("nan"), partls.lowlevel.ERR_NONFINITE), (None, partls.lowlevel.ERR_BAD_ARG)):
            e = dw.clone()
            if bad is None:
                e.zero_()
            else:
                e[N // 2] = bad
            torch.cuda.synchronize()
            with pytest.raises(partls.PartlsError) as ei:
                d.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, M, ldX, P, eta, flags, dw_ptr=e.data_ptr())
            assert ei.value.status == status
            with pytest.raises(partls.PartlsError) as ei:
                d.opt_sweep(0, -1)
            assert ei.value.status == partls.lowlevel.ERR_STATE
        d.close()


# ---- 9. weighted cross-validation -------------------------------------------------------------------------------------------------
def test_weighted_cross_validation_against_single_fits(partls, oracle):
    X, y, P, w = _problem(81, 600, 12, 3)
    etas = [0.0, 0.5]
    cv = partls.cross_validate(partls.Opt, X, y, P, η=etas, nfolds=3, weights=w)
    fp = cv.fold_ptr
    F, E = len(fp) - 1, len(etas)
    for f in range(F):
        tr = np.ones(len(y), dtype=bool)
        tr[fp[f]:fp[f + 1]] = False
        rows = slice(fp[f], fp[f + 1])
        for e, eta in enumerate(etas):
            model, _, rep = partls.fit(partls.Opt, X[tr], y[tr], P, η=eta, weights=w[tr])
            mc = cv.models[f][e]
            assert cv.status[f, e] == 0
            yy = float(np.sum(w[tr] * y[tr] ** 2))
            if cv.best_index[f, e] == rep.best_index:
                sc = max(1.0, np.abs(model.α).max(), np.abs(model.β).max())
                _close(mc.α, model.α, 1e-9 * sc); _close(mc.β, model.β, 1e-9 * sc)
                assert abs(mc.t - model.t) <= 1e-9 * max(1.0, abs(model.t), np.abs(model.β).max())
                assert abs(cv.opt[f, e] - rep.opt) <= 1e-10 * rep.opt + 1e-15 * np.sqrt(yy)
            else:                                                      # a near tie of the training problem (1e-13 y'Wy on obj^2)
                assert abs(cv.opt[f, e] ** 2 - rep.opt ** 2) <= 1e-12 * yy
            r = partls.predict(mc, X[rows]) - y[rows]
            want = float(np.sum(w[rows] * r * r))
            assert abs(cv.sse[f, e] - want) <= 1e-12 * want, (cv.sse[f, e], want)
            assert cv.mse[f, e] == cv.sse[f, e] / w[rows].sum()
    assert np.allclose(cv.mse_mean, cv.sse.sum(axis=0) / w.sum(), rtol=1e-15, atol=0)


def test_solutions_of_a_weighted_fit_survive_a_later_fit(partls):
    """returnAllSolutions keeps its problem: after another fit took the context over, solutions[b] re-prepares the WEIGHTED problem"""
    X, y, P, w = _problem(91, 400, 10, 3)
    _, _, rep = partls.fit(partls.Opt, X, y, P, η=0.2, weights=w, returnAllSolutions=True)
    sols = rep.solutions
    before = [sols[b] for b in (0, 5, len(sols) - 1)]
    partls.fit(partls.Opt, X, y, P, η=0.2)                               # unweighted, on the same shared context
    for (o1, m1), b in zip(before, (0, 5, len(sols) - 1)):
        o2, m2 = sols[b]
        assert o1 == o2 and np.array_equal(m1.α, m2.α) and np.array_equal(m1.β, m2.β) and m1.t == m2.t
