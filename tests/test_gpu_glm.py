"""Generalised linear fits on the GPU.  The yardsticks are numpy in np.longdouble (tests/glm_reference.py restates the
header's formulas), the library's own weighted prepares and fits, and an IRLS around the CPU oracle — never the code under test:
  1. partls_glm_working against the longdouble rows within the bound DERIVED in include/partls_glm.h (its constants are read from the
     header): both families, the start and the model mode, N at the edges of the 1024-row block with odd and even tails, eta on both
     sides of 0 and of the clamp; the deviance equal in bits across two calls and within N times the per-row bound of the longdouble
     sum; n_clamped and max |eta| exact; partls_glm_mean; a response array that is only 8-byte aligned;
  2. partls_opt_rework against a fresh weighted prepare on the response z, bit for bit (Gram, every pattern's objective, finish, Alt,
     BnB) for float64, float32 and CSR storage from host arrays and device tensors; w alone is opt_reweight; the response of the first
     prepare is remembered across reworks and forgotten by every other prepare;
  3. fit_glm against the same loop written around Context.glm_working and fit(alg, X, z, P, weights=W), bit for bit at every iterate;
  4. fit_glm against the independent IRLS (numpy rows + the oracle's enumeration) on the committed problems, at 1e-8;
  5. a separable binomial problem ends, clamped;
  6. the domain check of the response on the device names the first offending row and leaves the prepared problem alone."""
import ctypes as C
import warnings

import numpy as np
import pytest

import glm_reference as G
from context_reuse import FAITHFUL, OnDevice, diff, flat, sparsify, to_csr

pytestmark = pytest.mark.gpu

K_ = G.constants()
U = K_["U"]


@pytest.fixture(scope="module")
def ctx(partls):
    c = partls.Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _partition(M, K):
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), np.arange(M) % K] = 1
    return P


# ---- 1. the row kernel ------------------------------------------------------------------------------------------------------------------
ROW_P = np.ones((2, 1), dtype=np.int64)
ROW_MODEL = (np.array([0.75, 0.25]), np.array([1.5]), 0.25)
EDGES = np.array([0.0, -0.0, 30.0, -30.0, 30.000001, -30.000001, 700.0, -700.0, 5e-324, 29.999999, -29.999999, 1e-3, -1e-3])


def _row_problem(seed, N, family):
    """X (N x 2), y: the linear predictor of ROW_MODEL lands near a target that lies on both sides of 0 and of the clamp (N >= 2)"""
    rng = np.random.default_rng(seed)
    target = np.concatenate([rng.normal(0.0, 3.0, N // 2), rng.uniform(-45.0, 45.0, N - N // 2)])
    n = min(N, len(EDGES))
    target[:n] = EDGES[:n] if N > 2 else np.array([-31.0, 2.0])[:n]
    X = np.zeros((N, 2), order="F")
    X[:, 0] = (target - 0.25) / (0.75 * 1.5)
    X[:, 1] = rng.normal(0.0, 1e-3, N)
    if family == "binomial":
        y = rng.choice([0.0, 1.0, 0.5, 0.25, 1e-20, 1.0 - 2.0 ** -53], size=N, p=[0.35, 0.35, 0.1, 0.1, 0.05, 0.05])
        y[rng.random(N) < 0.2] = rng.random()
    else:
        y = rng.poisson(np.exp(np.clip(target, -3.0, 6.0))).astype(np.float64)
        y[::7] = 0.0
        if N > 4:
            y[1], y[3] = 2e13, 1e-300                         # the start beyond the clamp (log 2e13 = 30.6), and next to log 0.1
    return X, y


def _check_call(got, eta, y, family, start, where):
    """one working call against the longdouble rows; returns the reference rows"""
    N = len(y)
    ref, b = G.check_rows(dict(W=got["weights"], z=got["working_response"], mu=got["mu"]), eta, y, family, start, where)
    exact = np.sum(ref["d"])
    err, tol = abs(np.longdouble(got["deviance"]) - exact), N * np.max(b["d"])
    print("[glm]%s deviance %r, longdouble %r, error %.3g, bound %.3g; max|eta| %r, clamped %d" % (
        where, got["deviance"], float(exact), float(err), float(tol), got["max_abs_eta"], got["n_clamped"]))
    assert err <= tol, (where, got["deviance"], float(exact))
    assert got["n_clamped"] == int(np.sum(ref["clamped"])), where
    return ref


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025, 3001])
def test_working_rows_against_longdouble(partls, ctx, N, family):
    X, y = _row_problem(100 + N, N, family)
    ctx.opt_prepare(X, y, ROW_P)
    before = flat(ctx.opt_sweep())
    # the start
    g0 = ctx.glm_working(None, family)
    ref = _check_call(g0, None, y, family, True, " start N=%d" % N)
    eta0 = G.start_eta(np.asarray(y, dtype=np.longdouble), family, np.longdouble)
    want = np.max(np.abs(eta0))
    assert abs(np.longdouble(g0["max_abs_eta"]) - want) <= (K_["START_ETA_ULPS"] + 2 * want) * U
    # a model: eta is predict's, bit for bit
    eta = ctx.predict(X, ROW_P, *ROW_MODEL)
    if N > 2:
        assert np.sum(eta > 30) and np.sum(eta < -30) and np.sum((eta > 0) & (eta < 30)) and np.sum((eta < 0) & (eta > -30))
    g1 = ctx.glm_working(ROW_MODEL, family)
    ref = _check_call(g1, eta, y, family, False, " model N=%d" % N)
    assert g1["max_abs_eta"] == float(np.max(np.abs(eta)))
    g2 = ctx.glm_working(ROW_MODEL, family)                   # the same input: the same bits
    assert all(_same_bits(g2[k], g1[k]) for k in ("deviance", "max_abs_eta", "n_clamped", "weights", "working_response", "mu"))
    assert _same_bits(ctx.glm_working(None, family)["deviance"], g0["deviance"])
    assert ctx.glm_working(ROW_MODEL, family, want_rows=False)["weights"] is None
    assert np.all(g1["weights"] >= 9.3e-14) and np.all(np.isfinite(g1["working_response"]))
    assert _same_bits(ctx.glm_mean(family, eta), g1["mu"])    # the inverse link alone: the same device function
    assert not diff(flat(ctx.opt_sweep()), before)            # the prepared problem is untouched


@pytest.mark.parametrize("family", G.FAMILIES)
def test_device_rows_and_a_response_that_is_only_8_byte_aligned(partls, ctx, family):
    import torch
    N = 1025
    X, y = _row_problem(7, N, family)
    ctx.opt_prepare(X, y, ROW_P)
    host = ctx.glm_working(ROW_MODEL, family)
    host0 = ctx.glm_working(None, family)
    dev = OnDevice(X)
    ybuf = torch.from_numpy(np.r_[-7.0, y]).cuda()            # y starts 8 bytes into an allocation
    out = torch.full((3, N + 2), -7.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert (ybuf.data_ptr() + 8) % 16 == 8
    ctx.opt_prepare_device(dev.ptr("X"), ybuf.data_ptr() + 8, N, 2, dev.ld, ROW_P)
    with pytest.raises(ValueError):
        ctx.glm_working(ROW_MODEL, family)                    # prepared from device pointers
    for model, want in ((ROW_MODEL, host), (None, host0)):
        got = ctx.glm_working_device(model, family, dw_ptr=out[0].data_ptr(), dz_ptr=out[1].data_ptr(), dmu_ptr=out[2].data_ptr())
        torch.cuda.synchronize()
        rows = out.cpu().numpy()
        assert np.all(rows[:, N:] == -7.5)                    # N doubles each and no more
        assert all(_same_bits(got[k], want[k]) for k in ("deviance", "max_abs_eta", "n_clamped"))
        assert _same_bits(rows[0, :N], want["weights"]) and _same_bits(rows[1, :N], want["working_response"]) and _same_bits(rows[2, :N], want["mu"])
    assert ctx.glm_working_device(ROW_MODEL, family)["deviance"] == host["deviance"]      # no rows wanted
    ctx.opt_prepare(X, y, ROW_P)
    with pytest.raises(ValueError):
        ctx.glm_working_device(ROW_MODEL, family)             # prepared from host arrays


@pytest.mark.parametrize("family", G.FAMILIES)
def test_the_inverse_link_at_the_edges(partls, ctx, family):
    """partls_glm_mean on exact values of eta: 0, -0, the clamp and beyond it, a denormal — needs no prepared problem"""
    c = partls.Context(0)
    mu = c.glm_mean(family, EDGES)
    c.close()
    ref = G.rows(EDGES.astype(np.longdouble), np.zeros(len(EDGES), dtype=np.longdouble), family, np.longdouble)["mu"]
    assert np.all(np.abs(mu.astype(np.longdouble) - ref) <= K_["MU_ULPS"] * U * ref)
    assert mu[4] == mu[6] == mu[2] and mu[5] == mu[7] == mu[3] and mu[0] == mu[1] == mu[8] == (0.5 if family == "binomial" else 1.0)
    assert np.all(np.diff(mu[np.argsort(EDGES, kind="stable")]) >= 0) and np.all(mu > 0) and np.all(np.isfinite(mu))
    assert len(ctx.glm_mean(family, np.zeros(0))) == 0


def test_refusals_of_glm_working(partls):
    L = partls.lowlevel
    lib = L.lib()
    X, y = _row_problem(8, 300, "binomial")
    c = partls.Context(0)
    DP = C.POINTER(C.c_double)

    def raw(h, alpha=ROW_MODEL[0], beta=ROW_MODEL[1], t=0.25, family=0):
        a = None if alpha is None else np.ascontiguousarray(alpha).ctypes.data_as(DP)
        b = None if beta is None else np.ascontiguousarray(beta).ctypes.data_as(DP)
        d = C.c_double(-7.5)
        st = lib.partls_glm_working(h, a, b, float(t), family, C.byref(d), None, None, None, None, None)
        assert st == 0 or d.value == -7.5                     # a refusal writes nothing
        return st

    assert raw(c._h) == L.ERR_BAD_ARG                         # no prepared problem
    with pytest.raises(ValueError):
        c.glm_working(ROW_MODEL, "binomial")
    c.opt_prepare(X, y, ROW_P)
    assert raw(c._h) == L.OK and raw(c._h, None, None) == L.OK
    for kw in (dict(alpha=None), dict(beta=None), dict(alpha=np.array([np.nan, 1.0])), dict(beta=np.array([np.inf])), dict(t=np.nan),
               dict(family=2), dict(family=-1)):
        assert raw(c._h, **kw) == L.ERR_BAD_ARG, kw
        assert lib.partls_last_error().decode().startswith("partls_glm_working"), kw
    with pytest.raises(ValueError):
        c.glm_working(ROW_MODEL, "gaussian")
    with pytest.raises(ValueError):
        c.glm_working((np.ones(3), ROW_MODEL[1], 0.0), "binomial")
    c.close()
    mc = partls.MultiContext([0, 0])
    c0 = mc.context(0)
    assert raw(c0._h) == L.ERR_UNSUPPORTED
    assert lib.partls_opt_rework(c0._h, None, None, 0) == L.ERR_UNSUPPORTED
    mc.close()


# ---- 2. the re-prepare ---------------------------------------------------------------------------------------------------------------------
def _data(seed, N, M, K):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.normal(0.5, 1.0, (N, M)))
    P = _partition(M, K)
    alpha, beta = rng.uniform(0.2, 1.0, M), rng.normal(0.0, 2.0, K)
    y = X @ (alpha * (P @ beta)) + 0.75 + 0.1 * rng.normal(size=N)
    return X, y, P


def _staged(ctx, M, K, seed, T=6):
    """everything a prepared faithful problem answers: Gram, every pattern's objective, finish, Alt, BnB"""
    rng = np.random.default_rng(seed)
    a0, b0 = rng.random(M + 1), (rng.random(K + 1) - 0.5) * 10
    ctx.tolerate_ill = True
    Gm = ctx.gram()
    bo, bp, allopt, unconv = ctx.opt_sweep(0, -1, want_all=True)
    return dict(gram=Gm, sweep=(bo, bp, allopt, unconv), finish=ctx.opt_finish(bp), alt=ctx.alt_prepared(a0, b0, 1e-6, T),
                bnb=ctx.bnb_prepared(), again=ctx.opt_sweep(0, -1, want_all=True))


def _prepare(partls, ctx, storage, on_device, X, y, P, eta, flags, w):
    """one prepare of the given storage kind, from host arrays or adopted device pointers; returns what must stay alive"""
    if storage == "csr":
        csr = to_csr(partls, X)
        if not on_device:
            return ctx.opt_prepare_csr(csr, y, P, eta, flags, weights=w)
        dev = OnDevice(y=y, w=w, csr=csr)
        ctx.opt_prepare_csr_device(dev.ptr("indptr"), dev.ptr("indices"), dev.ptr("data"), dev.ptr("y"), dev.N, dev.M, P, eta, flags,
                                   dw_ptr=dev.ptr("w"))
        return dev
    dtype = np.float32 if storage == "f32" else np.float64
    Xs = np.asfortranarray(X.astype(dtype))
    if not on_device:
        return ctx.opt_prepare(Xs, y, P, eta, flags, weights=w)
    dev = OnDevice(Xs, y, w, dtype=dtype)
    ctx.opt_prepare_device(dev.ptr("X"), dev.ptr("y"), dev.N, dev.M, dev.ld, P, eta, flags, dw_ptr=dev.ptr("w"), dtype=dtype)
    return dev


@pytest.mark.parametrize("M,K", [(12, 3), (40, 4)])
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("storage", ["f64", "f32", "csr"])
def test_rework_equals_a_fresh_weighted_prepare(partls, storage, on_device, M, K):
    N, seed, eta = 1025, 200 + M, 0.3
    X, y, P = _data(seed, N, M, K)
    if storage == "csr":
        X = sparsify(X, seed, keep=0.5)
    X = X.astype(np.float32).astype(np.float64) if storage == "f32" else X
    rng = np.random.default_rng(seed + 1)
    w, z = rng.uniform(0.25, 4.0, N), rng.normal(1.0, 3.0, N)        # arbitrary rows, not a GLM's
    used, fresh = partls.Context(0), partls.Context(0)
    try:
        keep = _prepare(partls, used, storage, on_device, X, y, P, eta, FAITHFUL, None)
        used.opt_sweep()                                     # the problem has been in use
        if on_device:
            rows = OnDevice(y=z, w=w)
            used.opt_rework_device(rows.ptr("w"), rows.ptr("y"))
        else:
            used.opt_rework(w, z)
        assert used.upload() == (0.0, 0.0)
        keep2 = _prepare(partls, fresh, storage, on_device, X, z, P, eta, FAITHFUL, w)
        bad = diff(flat(_staged(used, M, K, seed)), flat(_staged(fresh, M, K, seed)))
        assert not bad, (storage, on_device, bad)
        del keep, keep2
    finally:
        used.close()
        fresh.close()


def test_rework_with_weights_alone_is_reweight(partls):
    X, y, P = _data(210, 1025, 12, 3)
    w = np.random.default_rng(211).uniform(0.25, 4.0, 1025)
    a, b = partls.Context(0), partls.Context(0)
    a.opt_prepare(X, y, P, 0.3, FAITHFUL)
    b.opt_prepare(X, y, P, 0.3, FAITHFUL)
    a.opt_rework(w)
    b.opt_reweight(w)
    assert not diff(flat(_staged(a, 12, 3, 5)), flat(_staged(b, 12, 3, 5)))
    with pytest.raises(ValueError):
        a.opt_rework(None, y)                                 # a response without weights
    a.close()
    b.close()


def test_the_first_response_is_remembered_across_reworks(partls):
    L = partls.lowlevel
    N, M, K = 1025, 12, 3
    X, _, P = _data(220, N, M, K)
    rng = np.random.default_rng(221)
    y = (rng.random(N) < 0.4).astype(np.float64)
    model = (rng.uniform(0.2, 1.0, M), rng.normal(0.0, 0.3, K), -0.2)
    used, fresh = partls.Context(0), partls.Context(0)
    used.opt_prepare(X, y, P, 0.0, 0)
    with pytest.raises(partls.PartlsError) as e:
        used.opt_rework()                                     # no glm_working since the prepare
    assert e.value.status == L.ERR_STATE and used.opt_sweep()[3] == 0
    r1 = used.glm_working(model, "binomial")
    used.opt_rework()                                         # the rows of the last call, as copies the problem owns
    assert used.upload() == (0.0, 0.0)
    fresh.opt_prepare(X, r1["working_response"], P, 0.0, 0, weights=r1["weights"])
    assert _same_bits(used.gram(), fresh.gram())
    r2 = used.glm_working(model, "binomial")                  # z is installed, the rows still come from y
    assert all(_same_bits(r2[k], r1[k]) for k in ("deviance", "weights", "working_response", "mu"))
    r3 = used.glm_working(None, "binomial")                   # overwrites the kept rows; the problem has its own
    assert not _same_bits(r3["weights"], r1["weights"]) and _same_bits(used.gram(), fresh.gram())
    su, sf = used.opt_sweep(), fresh.opt_sweep()
    assert not diff(flat(su), flat(sf)) and not diff(flat(used.opt_finish(su[1])), flat(fresh.opt_finish(sf[1])))
    used.opt_rework(np.ones(N), r1["working_response"])       # a second rework, from host rows
    assert _same_bits(used.glm_working(model, "binomial")["deviance"], r1["deviance"])
    used.opt_reweight(r1["weights"])                          # ... and a reweight keep the record too
    assert _same_bits(used.gram(), fresh.gram())
    assert _same_bits(used.glm_working(model, "binomial")["working_response"], r1["working_response"])
    used.opt_prepare(X, r1["working_response"], P)            # every other prepare forgets: the response is now z, outside [0, 1]
    with pytest.raises(partls.PartlsError) as e:
        used.opt_rework()
    assert e.value.status == L.ERR_STATE
    with pytest.raises(partls.PartlsError) as e:
        used.glm_working(model, "binomial")
    assert e.value.status == L.ERR_BAD_ARG
    used.close()
    fresh.close()


# ---- 3. fit_glm against the host loop ------------------------------------------------------------------------------------------------------
def _glm_data(seed, N, M, K, family):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.normal(0.0, 1.0, (N, M)))
    P = _partition(M, K)
    alpha = rng.uniform(0.3, 1.0, M)
    alpha /= P @ (P.T @ alpha)
    beta = np.array([1.1, -0.8, 0.6, 0.9][:K])
    eta = X @ (alpha * (P @ beta)) + (0.2 if family == "binomial" else 0.7)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64) if family == "binomial" else rng.poisson(np.exp(eta)).astype(np.float64)
    return X, y, P, rng.random(M + 1), (rng.random(K + 1) - 0.5) * 10


def _fit_glm(partls, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", partls.GLMConvergenceWarning)
        warnings.simplefilter("ignore", partls.IllConditionedWarning)
        return partls.fit_glm(*args, **kw)


def _against_host_loop(partls, ctx, alg, X, y, P, family, **kw):
    host = G.host_loop(partls, ctx, alg, X, y, P, family=family, max_iter=8, **kw)
    n = host["iterations"]
    print("[glm] %s %s: iterations %d, deviance %r" % (alg.__name__, family, n, host["deviance"]))
    assert n >= 3                                             # the loop has something to agree on
    for j in range(1, n + 1):                                 # every iterate: the fit cut off after j re-weighted fits
        model, _, rep = _fit_glm(partls, alg, X, y, P, family=family, max_iter=j if j < n else 8, **kw)
        m, r = host["models"][j - 1], host["reports"][j - 1]
        assert _same_bits(model.α, m.α) and _same_bits(model.β, m.β) and _same_bits(model.t, m.t) and _same_bits(rep.opt, r.opt), j
        assert _same_bits(rep.glm.deviance, host["deviance"][:j + 1]) and rep.glm.iterations == j, j
        for k in ("best_index", "iters", "nopen"):
            assert (k in rep) == (k in r) and (k not in r or rep[k] == r[k]), k
    gl, last = rep.glm, host["last"]
    assert (gl.converged, gl.family) == (host["converged"], family)
    assert _same_bits(gl.weights, last["weights"]) and _same_bits(gl.working_response, last["working_response"])
    assert (gl.max_abs_eta, gl.n_clamped) == (last["max_abs_eta"], last["n_clamped"])
    assert _same_bits(partls.predict_mean(model, X, family), last["mu"])
    assert abs(gl.null_deviance - G.null_deviance(y, family)) <= 1e-12 * gl.null_deviance


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("alg", ["Opt", "Alt", "BnB"])
def test_fit_glm_against_the_host_loop(partls, ctx, alg, family, eta):
    X, y, P, a0, b0 = _glm_data(300, 300, 10, 3, family)
    kw = dict(alpha0=a0, beta0=b0) if alg == "Alt" else {}
    _against_host_loop(partls, ctx, getattr(partls, alg), X, y, P, family, η=eta, **kw)


def test_fit_glm_float32_and_csr_against_the_host_loop(partls, ctx):
    X, y, P, a0, b0 = _glm_data(301, 300, 10, 3, "binomial")
    _against_host_loop(partls, ctx, partls.Opt, np.asfortranarray(X.astype(np.float32)), y, P, "binomial")
    Xs = sparsify(X, 301, keep=0.6)
    yp = np.random.default_rng(302).poisson(np.exp(np.clip(Xs @ np.full(10, 0.2) + 0.5, -3, 3))).astype(np.float64)
    _against_host_loop(partls, ctx, partls.Opt, to_csr(partls, Xs), yp, P, "poisson", η=0.5)


def test_running_out_of_iterations_warns(partls):
    X, y, P, _, _ = _glm_data(303, 300, 10, 3, "poisson")
    with pytest.warns(partls.GLMConvergenceWarning):
        _, _, rep = partls.fit_glm(partls.Opt, X, y, P, family="poisson", max_iter=1)
    assert not rep.glm.converged and rep.glm.iterations == 1 and len(rep.glm.deviance) == 2


# ---- 4. against the independent reference -------------------------------------------------------------------------------------------------
def _fixture_fit(partls, family):
    X, y, P, rec = G.fixture(family)
    with warnings.catch_warnings():
        warnings.simplefilter("error", partls.GLMConvergenceWarning)
        warnings.simplefilter("error", partls.IllConditionedWarning)
        model, _, rep = partls.fit_glm(partls.Opt, X, y, P, family=family)
    return X, y, P, rec, model, rep


@pytest.mark.parametrize("family", G.FAMILIES)
def test_fit_glm_against_the_reference_irls(partls, family):
    X, y, P, rec, model, rep = _fixture_fit(partls, family)
    gl = rep.glm
    print("[glm] fixture %s: deviance %r (reference %r), null %r" % (family, gl.deviance, list(rec["deviance"]), gl.null_deviance))
    assert gl.converged and gl.iterations == len(rec["deviance"]) - 1
    tol = 1e-8                                                # the project's parity tolerance (tests/test_gpu_fuzz.py)
    assert np.all(np.abs(model.α - rec["alpha"]) <= tol * max(1.0, np.abs(rec["alpha"]).max()))
    assert np.all(np.abs(model.β - rec["beta"]) <= tol * max(1.0, np.abs(rec["beta"]).max()))
    assert abs(model.t - rec["t"]) <= tol * max(1.0, abs(rec["t"]))
    assert np.all(np.abs(np.array(gl.deviance) - rec["deviance"]) <= tol * np.maximum(1.0, rec["deviance"]))
    assert gl.deviance[-1] < gl.null_deviance and gl.deviance[-1] < gl.deviance[0]        # below the null deviance and below dev_0
    assert abs(gl.null_deviance - G.null_deviance(y, family)) <= 1e-12 * gl.null_deviance


# ---- 5. a separable binomial problem --------------------------------------------------------------------------------------------------------
def test_a_separable_binomial_problem_ends_clamped(partls):
    N = 64
    x = np.linspace(-2.0, 2.0, N)                             # no 0 among them
    X = np.asfortranarray(x[:, None])
    y = (x > 0).astype(np.float64)
    P = np.ones((1, 1), dtype=np.int64)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        model, _, rep = partls.fit_glm(partls.Opt, X, y, P, family="binomial")        # no PartlsError: every status was OK
    assert all(issubclass(w.category, partls.GLMConvergenceWarning) for w in seen), [str(w.message) for w in seen]
    gl = rep.glm
    print("[glm] separable: iterations %d, converged %s, clamped %d, max|eta| %r, deviance %r" % (gl.iterations, gl.converged, gl.n_clamped,
                                                                                                  gl.max_abs_eta, gl.deviance))
    assert 1 <= gl.iterations <= 25 and len(gl.deviance) == gl.iterations + 1
    assert gl.n_clamped > 0 and gl.max_abs_eta > 30.0 and np.all(np.isfinite(gl.deviance))
    assert np.all(np.isfinite(np.r_[model.α, model.β, model.t])) and model.β[0] > 0
    mu = partls.predict_mean(model, X, "binomial")
    assert np.all((mu > 0.5) == (y == 1.0))


# ---- 6. the domain check on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,value", [("binomial", np.nan), ("binomial", 1.5), ("poisson", -1.0)])
def test_the_response_is_checked_on_the_device(partls, family, value):
    import torch
    L = partls.lowlevel
    N, row = 2049, 1030
    X, _, P = _data(600, N, 5, 2)
    rng = np.random.default_rng(601)
    y = (rng.random(N) < 0.5).astype(np.float64)
    model = (rng.uniform(0.2, 1.0, 5), rng.normal(0.0, 0.3, 2), 0.1)
    c = partls.Context(0)
    if np.isnan(value):                                       # no prepare takes a NaN: it arrives in the caller's device array afterwards
        dev = OnDevice(X, y)
        c.opt_prepare_device(dev.ptr("X"), dev.ptr("y"), N, 5, dev.ld, P)
        before = flat(c.opt_sweep())
        dev.keep["y"][row] = float("nan")
        dev.keep["y"][row + 7] = float("nan")
        torch.cuda.synchronize()
        call = lambda m: c.glm_working_device(m, family)
    else:
        y[row] = value
        y[row + 7] = value
        c.opt_prepare(X, y, P)
        before = flat(c.opt_sweep())
        call = lambda m: c.glm_working(m, family)
    for m in (None, model):
        with pytest.raises(partls.PartlsError) as e:
            call(m)
        msg = L.lib().partls_last_error().decode()
        assert e.value.status == L.ERR_BAD_ARG and msg.startswith("partls_glm_working") and msg.endswith("row %d" % row), msg
    with pytest.raises(partls.PartlsError) as e:
        c.opt_rework()                                        # nothing was written: no rows to rework with
    assert e.value.status == L.ERR_STATE
    assert not diff(flat(c.opt_sweep()), before)              # the prepared problem still sweeps to the same bits
    if family == "binomial" and not np.isnan(value):
        assert c.glm_working(model, "poisson")["deviance"] > 0.0      # 1.5 is a fine Poisson response: the check is the family's
    c.close()
