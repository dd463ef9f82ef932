"""GPU tests of partls_diagnostics.

Data: X ~ N(mean, 1), y = X truth + 0.7 + 0.3 noise with a sparse truth (zero outside the wanted support, one sign per group), weights
10^U(-1, 1) with exact zeros, eta in {0, 0.5}.  The model is fit(Opt) on the columns of the support, embedded in all M features, so
that the size p of the support is the case's and the active columns are gathered through the index list.
Reference (numpy, independent of the Gram form): Z = [sqrt(W) Xo_A ; sqrt(eta) Po_A'], Householder QR, h = the squared row norms of the
first N rows of Q.  kappa = the 2-norm condition number of Z with unit columns; every case asserts kappa <= 50.
Bounds, with u = 2^-53 and delta = 8 p kappa^2 u (the perturbation bound of the normal equations): |h - h_ref| <= delta, and the same
delta propagated to first order through the formulas of the other outputs (see _bounds).
mean = 1 gives kappa ~ M (the ones column is the mean of the feature columns up to N(0, 1 / M) noise per row): 255 at p = 300, N = 1200
and 840 at p = 1023, N = 4092, against 25 - 32 at p = 33, N = 200.  The two large shapes therefore draw X ~ N(0, 1); N, p, the guard
kappa <= 50 and the bound are unchanged."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROWS = ("leverage", "loo", "studentized", "cooks", "residual")


# ---- data, models, reference ------------------------------------------------------------------------------------------------------------
def make_data(N, M, K, p, seed, mean=1.0, weighted=False):
    """X, y, P (feature m in group m mod K), w (None: unweighted) and the p - 1 features of the support (sorted, a random subset)"""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.normal(mean, 1.0, size=(N, M)))
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), np.arange(M) % K] = 1
    S = np.sort(rng.permutation(M)[:p - 1]) if p - 1 < M else np.arange(M)
    truth = np.zeros(M)
    truth[S] = np.where((S % K) % 2 == 0, 1.0, -1.0) * rng.uniform(0.5, 1.5, size=len(S))
    y = X @ truth + 0.7 + 0.3 * rng.normal(size=N)
    w = None
    if weighted:
        w = 10.0 ** rng.uniform(-1.0, 1.0, size=N)
        w[rng.permutation(N)[:N // 8]] = 0.0                          # exact zeros (none below N = 8)
    return X, y, P, w, S


def fit_on_support(partls, X, y, P, w, S, eta):
    """fit(Opt) on the columns S, embedded in all features; the fit keeps every column of S (asserted: the case's p)"""
    import warnings
    if len(S) == 0:
        return partls.PartLSFitResult(np.zeros(X.shape[1]), np.zeros(P.shape[1]), 0.0, P), None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sub, _, rep = partls.fit(partls.Opt, np.asfortranarray(X[:, S]), y, P[S], η=eta, weights=w)
    a = np.zeros(X.shape[1])
    a[S] = sub.α
    model = partls.PartLSFitResult(a, sub.β.copy(), float(sub.t), P)
    assert np.count_nonzero(a * (P @ sub.β)) == len(S), "the fit dropped a column of the wanted support"
    return model, rep


def reference(X, y, w, P, eta, S):
    """h_ref [N], R (the triangular factor of Z), kappa and the smallest singular value of Z with unit columns, the column norms of Z"""
    N, M = X.shape
    K = P.shape[1]
    wv = np.ones(N) if w is None else w
    XoA = np.hstack([X[:, S], np.ones((N, 1))])
    Z = np.sqrt(wv)[:, None] * XoA
    if eta:
        Po = np.zeros((M + 1, K + 1))
        Po[:M, :K] = P
        Po[M, K] = 1.0
        Z = np.vstack([Z, np.sqrt(eta) * Po[list(S) + [M]].T])
    Q, R = np.linalg.qr(Z)
    norms = np.linalg.norm(Z, axis=0)
    sv = np.linalg.svd(Z / norms, compute_uv=False)
    return (Q[:N] ** 2).sum(1), R, sv[0] / sv[-1], sv[-1], norms


def _bounds(delta, N, e, h, w, dof, nplus, sigma2):
    """delta = the bound on |h - h_ref|, propagated to first order, each with a few u of the value for the roundings of its own formula:
    loo = e / (1 - h):                 delta max|e| / min(1 - h)^2
    dof = sum h, sigma2 = rss / (n+ - dof): |d dof| <= N delta, |d sigma2| / sigma2 <= N delta / (n+ - dof) =: rs
    studentized s = sqrt(w) e / sqrt(sigma2 (1 - h)):  |s| (delta / (2 (1 - h)) + rs / 2)
    cooks c = s^2 h / (dof (1 - h)):   c (2 |ds| / |s| + N delta / dof + delta / (1 - h)) + s^2 delta / (dof (1 - h))"""
    om = 1.0 - h
    rs = N * delta / (nplus - dof)
    s = np.sqrt(w) * e / np.sqrt(sigma2 * om)
    c = s * s * h / (dof * om)
    rel_s = delta / (2 * om) + rs / 2
    return dict(loo=delta * np.max(np.abs(e)) / np.min(om) ** 2 + 4 * U * np.abs(e / om),
                studentized=2 * np.abs(s) * rel_s + 8 * U * np.abs(s),
                cooks=2 * (c * (2 * rel_s + N * delta / dof + delta / om) + s * s * delta / (dof * om)) + 16 * U * c), s, c


class DeviceProblem:
    """(X, y, w) in HBM with a padded leading dimension (ldX = N + 3, the padding NaN) and the context prepared on them"""

    def __init__(self, partls, X, y, P, w, eta, dtype=np.float64, ctx=None):
        import torch
        self.torch = torch
        N, M = X.shape
        self.N, self.ld = N, N + 3
        buf = np.full((M, self.ld), np.nan, dtype=dtype)
        buf[:, :N] = X.T
        self.dX = torch.from_numpy(buf).cuda()
        self.dy = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).cuda()
        self.dw = None if w is None else torch.from_numpy(np.ascontiguousarray(w)).cuda()
        torch.cuda.synchronize()
        self.ctx = ctx or partls.Context(0)
        self.ctx.opt_prepare_device(self.dX.data_ptr(), self.dy.data_ptr(), N, M, self.ld, P, eta,
                                    dw_ptr=None if self.dw is None else self.dw.data_ptr(), dtype=dtype)

    def diagnostics(self, model, rows=ROWS):
        torch = self.torch
        out = {r: torch.full((self.N,), -7.5, dtype=torch.float64, device="cuda") for r in rows}
        torch.cuda.synchronize()
        res = self.ctx.diagnostics_device(model.α, model.β, model.t, **{"d%s_ptr" % r: t.data_ptr() for r, t in out.items()})
        torch.cuda.synchronize()
        res.update({r: t.cpu().numpy() for r, t in out.items()})
        return res


def check_case(partls, N, M, K, p, seed, mean, eta, weighted, want_se=True):
    X, y, P, w, S = make_data(N, M, K, p, seed, mean, weighted)
    return check_problem(partls, X, y, P, w, S, eta, want_se)[0]


def check_problem(partls, X, y, P, w, S, eta, want_se=True):
    """every check of a case on given data (the support S has p - 1 features) -> (the outputs of the float64 device call, the model)"""
    N, M = X.shape
    p, weighted = len(S) + 1, w is not None
    model, _ = fit_on_support(partls, X, y, P, w, S, eta)
    href, R, kappa, smin, norms = reference(X, y, w, P, eta, S)
    assert kappa <= 50.0, kappa
    delta = 8 * p * kappa ** 2 * U
    d = DeviceProblem(partls, X, y, P, w, eta).diagnostics(model)
    s = d["summary"]
    L = partls.lowlevel
    wv = np.ones(N) if w is None else w
    h, e = d["leverage"], d["residual"]
    tag = (N, M, p, eta, weighted)
    print("case", tag, "kappa %.1f delta %.2e max|h - href| %.2e" % (kappa, delta, np.max(np.abs(h - href))))
    assert np.all(h >= 0.0) and np.all(h[wv == 0.0] == 0.0)
    assert np.max(np.abs(h - href)) <= delta, tag
    assert np.array_equal(e, y - partls.predict(model, X)), tag                       # bit for bit
    assert s[L.DIAG_P] == p and np.array_equal(np.flatnonzero(d["active"]), list(S) + [M])
    assert s[L.DIAG_NPLUS] == np.count_nonzero(wv > 0)
    # the derived per-row outputs against their formulas at h_ref, dof_ref, sigma2_ref
    dof_ref = float(np.sum(href.astype(np.longdouble)))
    rss_ref = float(np.sum(wv.astype(np.longdouble) * e.astype(np.longdouble) ** 2))
    sigma2_ref = rss_ref / (s[L.DIAG_NPLUS] - dof_ref)
    bnd, s_ref, c_ref = _bounds(delta, N, e, href, wv, dof_ref, s[L.DIAG_NPLUS], sigma2_ref)
    loo_ref = e / (1.0 - href)
    for name, ref in (("loo", loo_ref), ("studentized", s_ref), ("cooks", c_ref)):
        err = np.abs(d[name] - ref)
        print("   ", name, "max err %.2e, max err / bound %.2e" % (np.max(err), np.max(err[bnd[name] > 0] / bnd[name][bnd[name] > 0])))
        assert np.all(err <= bnd[name]), (tag, name)
    assert np.array_equal(d["loo"][wv == 0.0], e[wv == 0.0])                          # a row of weight 0: h = 0, loo = e
    # the sums: dof against p at eta = 0 and against the reference's; rss, press against longdouble sums of the returned terms
    assert abs(s[L.DIAG_DOF] - dof_ref) <= N * delta
    if eta == 0:
        assert abs(s[L.DIAG_DOF] - p) <= N * delta, (tag, s[L.DIAG_DOF])
    for key, v in ((L.DIAG_RSS, e), (L.DIAG_PRESS, d["loo"])):
        terms = wv.astype(np.longdouble) * v.astype(np.longdouble) ** 2
        assert abs(s[key] - float(np.sum(terms))) <= (N + 2) * U * float(np.sum(np.abs(terms))), (tag, key)
    assert s[L.DIAG_SIGMA2] == s[L.DIAG_RSS] / (s[L.DIAG_NPLUS] - s[L.DIAG_DOF])
    ybar = float(np.sum(wv * y) / np.sum(wv))
    tss = float(np.sum(wv * (y - ybar) ** 2))
    # tss = yy - sy^2 / sw from the Gram corner: each of the three sums carries at most N u of sum w y^2 (Cauchy-Schwarz for sy^2 / sw)
    assert abs(s[L.DIAG_TSS] - tss) <= 4 * (N + 4) * U * float(np.sum(wv * y * y)), tag
    assert s[L.DIAG_R2] == 1.0 - s[L.DIAG_RSS] / s[L.DIAG_TSS] and s[L.DIAG_R2_LOO] == 1.0 - s[L.DIAG_PRESS] / s[L.DIAG_TSS]
    assert s[L.DIAG_STATIONARITY] <= 1e-12, (tag, s[L.DIAG_STATIONARITY])             # a fit(Opt) model is stationary on its support
    if want_se:
        check_standard_errors(d, X, y, w, P, eta, S, R, kappa, smin, norms, s[L.DIAG_SIGMA2], delta, s, L, tag)
    return d, model


def _inverse_longdouble(H):
    """Gauss-Jordan without pivoting (H is SPD), in longdouble"""
    p = H.shape[0]
    A = np.hstack([H.astype(np.longdouble), np.eye(p, dtype=np.longdouble)])
    for i in range(p):
        A[i] /= A[i, i]
        f = A[:, i].copy()
        f[i] = 0
        A -= f[:, None] * A[i][None, :]
    return A[:, p:]


def check_standard_errors(d, X, y, w, P, eta, S, R, kappa, smin, norms, sigma2, delta, s, L, tag):
    """eta = 0: Cov = sigma2 (R'R)^-1 from the QR; eta > 0: the sandwich sigma2 S B S with S = (B + eta Q_A)^-1, formed in longdouble.
    Bound on a variance: the inverse of the normal matrix in the unit-column scale has norm 1 / smin^2, and a perturbation of relative
    size delta / kappa^2 = 8 p u of the normal matrix moves the inverse by delta / smin^2 in norm; unscaling entry (a, b) divides by
    norms[a] norms[b].  sigma2 itself carries N delta / (n+ - dof) relative."""
    N, M = X.shape
    K = P.shape[1]
    A = list(S) + [M]
    p = len(A)
    wv = np.ones(N) if w is None else w
    XoA = np.hstack([X[:, S], np.ones((N, 1))]).astype(np.longdouble)
    Bm = XoA.T @ (wv.astype(np.longdouble)[:, None] * XoA)
    Po = np.zeros((M + 1, K + 1))
    Po[:M, :K] = P
    Po[M, K] = 1.0
    G = Po[A]                                                                          # [p, K + 1]: the groups over the support
    if eta == 0:
        Rinv = np.linalg.solve(R, np.eye(p))
        cov = (Rinv @ Rinv.T).astype(np.longdouble)
    else:
        Sm = _inverse_longdouble(Bm + eta * (G @ G.T).astype(np.longdouble))
        cov = Sm @ Bm @ Sm
    rel_sigma = N * delta / (s[L.DIAG_NPLUS] - s[L.DIAG_DOF])
    var_w = np.array([float(cov[j, j]) for j in range(p)])
    tol_w = 2 * delta / smin ** 2 / norms ** 2 + (rel_sigma + 8 * U) * var_w
    got_w = d["se_w"][A] ** 2 / sigma2
    print("    se_w: max |var err| / bound %.2e" % np.max(np.abs(got_w - var_w) / tol_w))
    assert np.all(np.abs(got_w - var_w) <= tol_w), tag
    assert np.all(d["se_w"][np.setdiff1d(np.arange(M + 1), A)] == 0.0)
    for k in range(K):
        g = G[:, k]
        var_b = float(g.astype(np.longdouble) @ cov @ g.astype(np.longdouble))
        tol_b = 2 * delta / smin ** 2 * float(np.sum(g / norms)) ** 2 + (rel_sigma + 8 * U) * var_b
        assert abs(d["se_beta"][k] ** 2 / sigma2 - var_b) <= tol_b, (tag, k)


# ---- against the QR reference: every tile shape of T ------------------------------------------------------------------------------------
SHAPES = [  # (N, M, K, p, mean): p = 5, 16, 17, 33 (a tile less, a tile, a tile and one, two tiles and one), p = M + 1, and the row counts
    (64, 9, 2, 5, 1.0), (100, 24, 3, 16, 1.0), (100, 24, 3, 17, 1.0), (200, 40, 3, 33, 1.0), (100, 12, 3, 13, 1.0),
    (15, 6, 2, 5, 1.0), (17, 6, 2, 5, 1.0), (255, 9, 2, 5, 1.0), (257, 9, 2, 5, 1.0)]


@pytest.mark.parametrize("N,M,K,p,mean", SHAPES)
def test_outputs_within_the_normal_equations_bound_of_qr(partls, N, M, K, p, mean):
    for eta in (0.0, 0.5):
        for weighted in (False, True):
            check_case(partls, N, M, K, p, 1000 * p + N, mean, eta, weighted)


def test_support_of_300_spans_several_tile_rows(partls):
    check_case(partls, 1200, 320, 3, 300, 300, 0.0, 0.0, True, want_se=False)
    check_case(partls, 1200, 320, 3, 300, 301, 0.0, 0.5, False, want_se=False)


def test_support_of_1023_at_the_largest_model(partls):
    check_case(partls, 4092, 1022, 2, 1023, 1023, 0.0, 0.0, True, want_se=False)


@pytest.mark.parametrize("N", [1, 15, 17, 255, 257])
def test_all_zero_model_has_leverage_w_over_sum_w(partls, N):
    """p = 1: only the intercept is active, H = sum w, and h_i must equal w_i / sum w to 4 u; e = y and loo = y / (1 - h) (inf or NaN at
    N = 1, where h = 1: plain IEEE)"""
    for weighted in (False, True):
        X, y, P, w, _ = make_data(N, 3, 2, 1, N, 1.0, weighted)
        if w is not None and not w.any():
            w[0] = 1.0
        model = partls.PartLSFitResult(np.zeros(3), np.zeros(2), 0.0, P)
        d = DeviceProblem(partls, X, y, P, w, 0.0).diagnostics(model)
        wv = np.ones(N) if w is None else w
        ref = (wv.astype(np.longdouble) / np.sum(wv.astype(np.longdouble))).astype(np.float64)
        assert np.max(np.abs(d["leverage"] - ref)) <= 4 * U, (N, weighted)
        assert d["summary"][partls.lowlevel.DIAG_P] == 1 and np.array_equal(d["active"], [False, False, False, True])
        assert np.array_equal(d["residual"], y)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(d["loo"], y / (1.0 - d["leverage"]), equal_nan=True)
        assert abs(d["summary"][partls.lowlevel.DIAG_DOF] - 1.0) <= 4 * N * U
        if N == 1:
            assert d["leverage"][0] == 1.0 and not np.isfinite(d["loo"][0]) and np.isnan(d["summary"][partls.lowlevel.DIAG_SIGMA2])
    # eta = 0.5 on the same shape: the general reference (H = sum w + eta)
    if N > 1:
        X, y, P, w, S = make_data(N, 3, 2, 1, N, 1.0, True)
        href, _, kappa, _, _ = reference(X, y, w, P, 0.5, S)
        d = DeviceProblem(partls, X, y, P, w, 0.5).diagnostics(model, rows=("leverage",))
        assert kappa <= 50.0 and np.max(np.abs(d["leverage"] - href)) <= 8 * kappa ** 2 * U


# ---- against real refits ----------------------------------------------------------------------------------------------------------------
REFITS = [(60, 6, 2, 17), (120, 12, 3, 14)]       # (N, M, K, seed); the CPU oracle keeps pattern and support on 57 - 59 of 60 and 107 - 115 of 120 rows


def refit_problem(N, M, K, seed, weighted):
    X, y, P, w, _ = make_data(N, M, K, M // 2 + 1, seed, 1.0, weighted)       # half of the features carry signal: the support matters
    if w is not None:
        w[w == 0.0] = 1.0                                                 # the jackknife sets its own zero
    return X, y, P, w


@pytest.mark.parametrize("N,M,K,seed", REFITS)
def test_loo_is_the_residual_of_the_refit_without_the_row(partls, N, M, K, seed):
    """resample with W = w (1 - I): on every replicate that keeps best_index and the support, loo_i = y_i - predict(model_i, x_i) to the
    project's parity level, 1e-8 max|e|; at least 3/4 of the rows qualify"""
    for weighted in (False, True):
        for eta in (0.0, 0.5):
            X, y, P, w = refit_problem(N, M, K, seed, weighted)
            model, _, rep = partls.fit(partls.Opt, X, y, P, η=eta, weights=w)
            d = partls.diagnostics(model, X, y, η=eta, weights=w)
            W = (np.ones(N) if w is None else w)[:, None] * (1.0 - np.eye(N))
            jk = partls.resample(partls.Opt, X, y, P, W, η=eta)
            v = model.α * (P @ model.β)
            vj = np.asarray(jk.alpha) * (np.asarray(jk.beta) @ P.T)               # [N, M]
            keeps = (np.asarray(jk.status) == 0) & (np.asarray(jk.best_index) == rep.best_index) & np.all((vj != 0) == (v != 0)[None, :], axis=1)
            refit = y - (np.einsum("im,im->i", X, vj) + np.asarray(jk.t))
            err = np.abs(d.loo - refit)[keeps]
            print("refits", (N, M, K, weighted, eta), "qualify %d / %d, max err %.2e of max|e| %.2e" % (keeps.sum(), N, err.max(), np.max(np.abs(d.residual))))
            assert keeps.sum() >= 0.75 * N, (weighted, eta, int(keeps.sum()))
            assert np.all(err <= 1e-8 * np.max(np.abs(d.residual))), (weighted, eta)
            assert d.stationarity <= 1e-12 and d.p == np.count_nonzero(v) + 1


# ---- bitwise ----------------------------------------------------------------------------------------------------------------------------
def test_repeated_host_device_and_float32_calls_are_bit_equal(partls):
    N, M, K, p = 257, 24, 3, 17
    X, y, P, w, S = make_data(N, M, K, p, 5, 1.0, True)
    X = np.asfortranarray(X.astype(np.float32).astype(np.float64))        # representable in float32
    model, _ = fit_on_support(partls, X, y, P, w, S, 0.5)
    dev = DeviceProblem(partls, X, y, P, w, 0.5)
    a, b = dev.diagnostics(model), dev.diagnostics(model)
    ctx = partls.Context(0)
    ctx.opt_prepare(X, y, P, 0.5, partls.lowlevel.OPT_FAITHFUL_INTERCEPT, weights=w)     # (the flag: the sweep can return every objective)
    ctx.opt_sweep()                                                       # (the first sweep of a prepare also calibrates its visiting order)
    before = ctx.opt_sweep(want_all=True)
    host = ctx.diagnostics(model.α, model.β, model.t)
    after = ctx.opt_sweep(want_all=True)                                  # the prepared problem is untouched
    assert before[0] == after[0] and before[1] == after[1] and before[3] == after[3] and np.array_equal(before[2], after[2])
    ctx.opt_prepare(X.astype(np.float32), y, P, 0.5, weights=w)
    host32 = ctx.diagnostics(model.α, model.β, model.t)
    dev32 = DeviceProblem(partls, X, y, P, w, 0.5, dtype=np.float32).diagnostics(model)
    for other in (b, host, host32, dev32):
        for k in ROWS + ("se_w", "se_beta", "active", "summary"):
            assert np.array_equal(a[k], other[k], equal_nan=True), k
    assert ctx.diagnostics_timing()[2] > 0.0
    ctx.close()


# ---- errors: each leaves its outputs unwritten ------------------------------------------------------------------------------------------
def _raw_call(partls, ctx, alpha, beta, t, N, M, K):
    """partls_diagnostics itself, with host outputs filled with a sentinel -> (status, the outputs)"""
    out = [np.full(N, -7.5) for _ in ROWS] + [np.full(M + 1, -7.5), np.full(K, -7.5)]
    act, summ = np.full(M + 1, -7, dtype=np.int32), np.full(partls.lowlevel.DIAG_NSUM, -7.5)
    a, b = np.ascontiguousarray(alpha, dtype=np.float64), np.ascontiguousarray(beta, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    st = partls.lowlevel.lib().partls_diagnostics(ctx._h, a.ctypes.data_as(dp), b.ctypes.data_as(dp), float(t), *(o.ctypes.data for o in out[:5]),
                                                  out[5].ctypes.data_as(dp), out[6].ctypes.data_as(dp),
                                                  act.ctypes.data_as(C.POINTER(C.c_int32)), summ.ctypes.data_as(dp))
    return st, out + [act, summ]


def _unwritten(outs):
    return all(np.all(o == -7.5) for o in outs[:7]) and np.all(outs[7] == -7) and np.all(outs[8] == -7.5)


def test_refused_calls_write_nothing(partls):
    L = partls.lowlevel
    N, M, K = 40, 6, 2
    X, y, P, w, S = make_data(N, M, K, M + 1, 9, 1.0, False)
    model, _ = fit_on_support(partls, X, y, P, w, S, 0.0)
    ctx = partls.Context(0)
    st, outs = _raw_call(partls, ctx, model.α, model.β, model.t, N, M, K)             # not prepared
    assert st == L.ERR_STATE and _unwritten(outs)
    nz = np.nonzero(X)
    ctx.opt_prepare_csr(partls.CSR(np.concatenate([[0], np.cumsum(np.bincount(nz[0], minlength=N))]), nz[1], X[nz], (N, M)), y, P)
    st, outs = _raw_call(partls, ctx, model.α, model.β, model.t, N, M, K)             # a CSR problem
    assert st == L.ERR_UNSUPPORTED and _unwritten(outs)
    with pytest.raises(partls.PartlsError):
        ctx.diagnostics(model.α, model.β, model.t)
    ctx.opt_prepare(X, y, P)
    bad = model.α.copy()
    bad[2] = np.nan
    for args in ((bad, model.β, model.t), (model.α, model.β, np.inf)):                  # NaN / Inf in the model
        st, outs = _raw_call(partls, ctx, *args, N, M, K)
        assert st == L.ERR_BAD_ARG and _unwritten(outs)
    X2 = X.copy(order="F")
    X2[:, 3] = X2[:, 1]                                                                # two identical active columns
    ctx.opt_prepare(X2, y, P)
    a = np.full(M, 0.25)
    st, outs = _raw_call(partls, ctx, a, np.array([1.0, -1.0]), 0.5, N, M, K)
    assert st == L.ERR_ILL_CONDITIONED and _unwritten(outs)
    a[3] = 0.0                                                                         # ... one of them inactive: fine, and the context still works
    st, outs = _raw_call(partls, ctx, a, np.array([1.0, -1.0]), 0.5, N, M, K)
    assert st == L.OK and not _unwritten(outs) and outs[7].tolist() == [1, 1, 1, 0, 1, 1, 1] and np.all(outs[0] >= 0.0)
    ctx.close()
