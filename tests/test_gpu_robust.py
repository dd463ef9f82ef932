"""Robust fits on the GPU.  The yardsticks are numpy (tests/robust_reference.py restates the header's rules operation
for operation) and the library's own weighted fits, never the code under test:
  1. partls_robust_weights against numpy applied to predict's yhat, bit for bit (weights, scale, max_dw, n_down, n_zero; rho_sum
     within its summation bound), over row counts around every block edge, both losses, estimated and fixed scales, a second call
     against the first call's weights, a repeated call, exact fits (scale 0), ties, 1e300 and a denormal, float32 and CSR storage,
     device-resident problems with a padded leading dimension, and its refusals;
  2. partls_opt_reweight against a fresh weighted prepare, bit for bit (Gram, every pattern's objective, finish, Alt, BnB), with no
     upload, the statuses of a weighted prepare for bad weights, and its refusals;
  3. fit_robust against the same loop written around fit(..., weights=) with numpy weights, bit for bit; c = 1e300; the descent of
     the loss under a fixed scale; planted outliers; running out of iterations; the default context afterwards;
  4. the selection on residuals planted exactly (a one-column X, an all-zero model): thresholds that part in pass 0 and in pass 1, zero
     and the smallest denormal under a normal value, an exact tie at the median, and N beyond one trip of the histogram's grid."""
import warnings

import numpy as np
import pytest

import robust_reference as R
from context_reuse import FAITHFUL, GENERIC, OnDevice, diff, flat, sparsify, to_csr, weights_with_zeros

pytestmark = pytest.mark.gpu

LOSSES = ("huber", "bisquare")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx(partls):
    c = partls.Context(0)
    yield c
    c.close()


def _partition(M, K):
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), np.arange(M) % K] = 1
    return P


def _data(seed, N, M, K=None, outliers=0.1):
    """X, y, P and two models (alpha, beta, t) near the truth; a share of the rows of y is shifted"""
    rng = np.random.default_rng(seed)
    K = min(M, 3) if K is None else K
    X = np.asfortranarray(rng.normal(0.5, 1.0, (N, M)))
    P = _partition(M, K)
    alpha, beta, t = rng.uniform(0.2, 1.0, M), rng.normal(0.0, 2.0, K), 0.75
    y = X @ (alpha * (P @ beta)) + t + 0.1 * rng.normal(size=N)
    y[rng.random(N) < outliers] += 5.0
    model_b = (alpha * rng.uniform(0.9, 1.1, M), beta + 0.05 * rng.normal(size=K), t - 0.02)
    return X, y, P, (alpha, beta, t), model_b


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(got, a, loss, c=None, scale=None, w_prev=None, where=""):
    """one call's results against numpy on the absolute residuals a; returns the reference"""
    ref = R.robust_info(a, loss, c, scale, w_prev)
    print("[robust]%s N=%d %s scale=%r max_dw=%r n_down=%d n_zero=%d rho_sum=%r" % (where, len(a), loss, got["scale"], got["max_dw"],
                                                                                    got["n_down"], got["n_zero"], got["rho_sum"]))
    assert _same_bits(got["scale"], ref["scale"]), (where, got["scale"], ref["scale"])
    if ref["scale"] == 0.0:
        assert got["weights"] is None and (got["rho_sum"], got["max_dw"], got["n_down"], got["n_zero"]) == (0.0, 0.0, 0, 0), where
        return ref
    if got["weights"] is not None:
        assert _same_bits(got["weights"], ref["weights"]), (where, int(np.sum(got["weights"] != ref["weights"])))
    assert _same_bits(got["max_dw"], ref["max_dw"]), (where, got["max_dw"], ref["max_dw"])
    assert (got["n_down"], got["n_zero"]) == (ref["n_down"], ref["n_zero"]), where
    exact = np.sum(ref["rho"].astype(np.longdouble))
    assert abs(np.longdouble(got["rho_sum"]) - exact) <= (len(a) + 8) * U * exact, (where, got["rho_sum"], float(exact))
    return ref


def _abs_res(ctx, X, y, P, model):
    return np.abs(ctx.predict(X, P, *model) - y)


# ---- 1. the weights pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 17])
@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 1000, 4097, 70001])
def test_weights_against_numpy(partls, ctx, N, M):
    X, y, P, ma, mb = _data(1000 * M + N, N, M)
    aa, ab = _abs_res(ctx, X, y, P, ma), _abs_res(ctx, X, y, P, mb)
    for loss in LOSSES:
        ctx.opt_prepare(X, y, P)                             # a prepare: the record of the previous weights starts again (all ones)
        before = flat(ctx.opt_sweep())
        r1 = _check(ctx.robust_weights(*ma, loss=loss), aa, loss, where=" first")
        w1 = r1["weights"]
        c2 = 1.1 if loss == "huber" else 3.9
        g2 = ctx.robust_weights(*mb, loss=loss, c=c2, scale=0.23)
        _check(g2, ab, loss, c2, 0.23, w1, where=" second")   # a fixed scale; max_dw against the first call's weights
        g3 = ctx.robust_weights(*mb, loss=loss, c=c2, scale=0.23)
        assert _same_bits(g3["weights"], g2["weights"]) and g3["max_dw"] == 0.0          # the same input: the same bits
        assert all(_same_bits(g3[k], g2[k]) for k in ("scale", "rho_sum", "n_down", "n_zero"))
        assert ctx.robust_weights(*ma, loss=loss, want_weights=False)["weights"] is None
        assert not diff(flat(ctx.opt_sweep()), before)       # the prepared problem is untouched


def test_exact_fits_ties_and_extreme_values(partls, ctx):
    # (a) more than half of the rows fitted exactly: scale 0, no weights written, the record of the previous weights stays
    X, y, P, ma, _ = _data(7, 1001, 5)
    yh = ctx.predict(X, P, *ma)
    y2 = y.copy()
    y2[:501] = yh[:501]
    ctx.opt_prepare(X, y2, P)
    a = np.abs(yh - y2)
    assert np.sum(a == 0.0) == 501
    for loss in LOSSES:
        _check(ctx.robust_weights(*ma, loss=loss), a, loss, where=" exact")
    r1 = _check(ctx.robust_weights(*ma, scale=1.5), a, "huber", None, 1.5, None, where=" exact, fixed scale")    # against all ones
    _check(ctx.robust_weights(*ma), a, "huber", where=" exact again")
    _check(ctx.robust_weights(*ma, loss="bisquare", scale=0.4), a, "bisquare", None, 0.4, r1["weights"], where=" exact, after")
    # (b) integer data: massive ties at every rank
    rng = np.random.default_rng(8)
    N = 4097
    X = np.asfortranarray(rng.integers(-3, 4, (N, 3)).astype(np.float64))
    P = np.ones((3, 1), dtype=np.int64)
    model = (np.array([1.0, 2.0, 3.0]), np.array([1.0]), -1.0)
    y = np.round(X @ model[0] - 1.0 + rng.integers(-2, 3, N) * (rng.random(N) < 0.7))
    ctx.opt_prepare(X, y, P)
    a = _abs_res(ctx, X, y, P, model)
    assert len(np.unique(a)) <= 5 and np.array_equal(a, np.round(a))
    for loss in LOSSES:
        _check(ctx.robust_weights(*model, loss=loss), a, loss, where=" ties")
        ctx.opt_prepare(X, y, P)
    # (c) one residual of 1e300 and one denormal: ordinary values of the selection and of the weights
    X, y, P, ma, _ = _data(9, 1000, 5)
    X[:, 0] = 0.0
    X[0, 0] = 1e150                                           # column 0 lives in row 0 alone: yhat_0 ~ 1e300, (X'X)_00 = 1e300 is finite
    X[1, :] = 0.0
    alpha, beta = ma[0].copy(), ma[1].copy()
    alpha[0], beta[0] = 1e150, 1.0
    model = (alpha, beta, 0.0)
    y[0], y[1] = 0.0, 5e-324                                  # yhat_1 = 0 exactly
    ctx.opt_prepare(X, y, P)
    a = _abs_res(ctx, X, y, P, model)
    assert a[0] > 9e299 and a[1] == 5e-324
    for loss in LOSSES:
        _check(ctx.robust_weights(*model, loss=loss), a, loss, where=" extreme")
        ctx.opt_prepare(X, y, P)
        _check(ctx.robust_weights(*model, loss=loss, scale=0.75), a, loss, None, 0.75, where=" extreme, fixed scale")
        ctx.opt_prepare(X, y, P)


def test_float32_and_csr_storage(partls, ctx):
    X, y, P, ma, mb = _data(21, 4097, 17)
    X32 = np.asfortranarray(X.astype(np.float32))
    wide = X32.astype(np.float64)
    a, b = _abs_res(ctx, wide, y, P, ma), _abs_res(ctx, wide, y, P, mb)
    assert _same_bits(a, _abs_res(ctx, X32, y, P, ma))
    for loss in LOSSES:
        res = []
        for Xin in (X32, wide):                               # the float32 problem against its widened copy, both against numpy
            ctx.opt_prepare(Xin, y, P)
            r1 = _check(ctx.robust_weights(*ma, loss=loss), a, loss, where=" %s" % Xin.dtype)
            g2 = ctx.robust_weights(*mb, loss=loss)
            _check(g2, b, loss, w_prev=r1["weights"], where=" %s second" % Xin.dtype)
            res.append(g2)
        assert not diff(flat(res[0]), flat(res[1]))
    # CSR: allowed to differ from the dense problem through yhat alone, so numpy is applied to predict of the CSR matrix
    Xs = sparsify(X, 5)
    csr = to_csr(partls, Xs)
    a, b = np.abs(ctx.predict_csr(csr, P, *ma) - y), np.abs(ctx.predict_csr(csr, P, *mb) - y)
    for loss in LOSSES:
        ctx.opt_prepare_csr(csr, y, P)
        r1 = _check(ctx.robust_weights(*ma, loss=loss), a, loss, where=" csr")
        _check(ctx.robust_weights(*mb, loss=loss, scale=0.3), b, loss, None, 0.3, r1["weights"], where=" csr second")


@pytest.mark.parametrize("kind", ["f64", "f32", "csr"])
def test_device_resident_problems(partls, ctx, kind):
    """adopted device pointers (X with ldX = N + 3, the padding NaN) and the weights written to a device address"""
    import torch
    X, y, P, ma, mb = _data(31, 4097, 5)
    if kind == "csr":
        X = sparsify(X, 6)
        csr = to_csr(partls, X)
        dev = OnDevice(y=y, csr=csr)
        ctx.opt_prepare_csr_device(dev.ptr("indptr"), dev.ptr("indices"), dev.ptr("data"), dev.ptr("y"), dev.N, dev.M, P)
        a, b = np.abs(ctx.predict_csr(csr, P, *ma) - y), np.abs(ctx.predict_csr(csr, P, *mb) - y)
    else:
        dtype = np.float32 if kind == "f32" else np.float64
        X = np.asfortranarray(X.astype(dtype))
        dev = OnDevice(X, y, dtype=dtype)
        ctx.opt_prepare_device(dev.ptr("X"), dev.ptr("y"), dev.N, dev.M, dev.ld, P, dtype=dtype)
        a, b = _abs_res(ctx, X, y, P, ma), _abs_res(ctx, X, y, P, mb)
    with pytest.raises(ValueError):
        ctx.robust_weights(*ma)                               # prepared from device pointers
    dw = torch.full((dev.N + 2,), -7.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g1 = ctx.robust_weights_device(*ma, loss="bisquare", dw_ptr=dw.data_ptr())
    torch.cuda.synchronize()
    host = dw.cpu().numpy()
    assert np.all(host[dev.N:] == -7.5)                       # N doubles and no more
    g1["weights"] = host[:dev.N].copy()
    r1 = _check(g1, a, "bisquare", where=" device " + kind)
    g2 = ctx.robust_weights_device(*mb, loss="huber", scale=0.2)       # no weights wanted
    g2["weights"] = None
    _check(g2, b, "huber", None, 0.2, r1["weights"], where=" device second " + kind)
    # ... and the weights go back in as a device array: the Gram of a fresh prepare with the same weights
    ctx.opt_reweight_device(dw.data_ptr())
    G = ctx.gram()
    assert ctx.upload() == (0.0, 0.0)
    fresh = partls.Context(0)
    if kind == "csr":
        fresh.opt_prepare_csr(csr, y, P, weights=r1["weights"])
    else:
        fresh.opt_prepare(X, y, P, weights=r1["weights"])
    assert _same_bits(G, fresh.gram())
    fresh.close()
    ctx.opt_prepare(np.asfortranarray(X.astype(np.float64)), y, P)
    with pytest.raises(ValueError):
        ctx.robust_weights_device(*ma)                        # prepared from host arrays


def test_refusals_of_robust_weights(partls):
    L = partls.lowlevel
    lib = L.lib()
    X, y, P, ma, _ = _data(41, 300, 5)
    c = partls.Context(0)

    def raw(h, alpha=ma[0], beta=ma[1], t=ma[2], loss=0, cc=1.345, scale=0.0):
        import ctypes as C
        a, b = np.ascontiguousarray(alpha), np.ascontiguousarray(beta)
        s = C.c_double(-7.5)
        st = lib.partls_robust_weights(h, a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double)), float(t), loss,
                                       cc, scale, C.byref(s), None, None, None, None, None)
        assert st == 0 or s.value == -7.5                     # a refusal writes nothing
        return st

    assert raw(c._h) == L.ERR_BAD_ARG                         # no prepared problem
    with pytest.raises(ValueError):
        c.robust_weights(*ma)
    c.opt_prepare(X, y, P)
    assert raw(c._h) == L.OK
    nan_a = ma[0].copy()
    nan_a[2] = np.nan
    for kw in (dict(alpha=nan_a), dict(beta=np.array([1.0, np.inf, 0.0])), dict(t=np.nan), dict(cc=0.0), dict(cc=-1.0), dict(cc=np.nan),
               dict(cc=np.inf), dict(loss=2), dict(loss=-1), dict(scale=np.nan), dict(scale=np.inf), dict(scale=-np.inf)):
        assert raw(c._h, **kw) == L.ERR_BAD_ARG, kw
        assert lib.partls_last_error().decode().startswith("partls_robust_weights"), kw
    assert raw(c._h, scale=-3.0) == L.OK                      # not positive: the scale is estimated
    for bad in (dict(loss="cauchy"), dict(c=0.0), dict(scale=-1.0)):
        with pytest.raises(ValueError):
            c.robust_weights(*ma, **bad)
    with pytest.raises(ValueError):
        c.robust_weights(ma[0][:3], ma[1], ma[2])
    c.close()
    mc = partls.MultiContext([0, 0])
    c0 = mc.context(0)
    assert raw(c0._h) == L.ERR_UNSUPPORTED
    assert lib.partls_opt_reweight(c0._h, None, 0) == L.ERR_UNSUPPORTED
    mc.close()


# ---- 2. the re-prepare -------------------------------------------------------------------------------------------------------------------
def _staged(ctx, M, K, seed, T=6):
    """everything a prepared faithful problem answers: Gram, every pattern's objective, finish, Alt, BnB, the upload statistics"""
    rng = np.random.default_rng(seed)
    a0, b0 = rng.random(M + 1), (rng.random(K + 1) - 0.5) * 10
    ctx.tolerate_ill = True
    G = ctx.gram()
    bo, bp, allopt, unconv = ctx.opt_sweep(0, -1, want_all=True)
    return dict(gram=G, sweep=(bo, bp, allopt, unconv), finish=ctx.opt_finish(bp), alt=ctx.alt_prepared(a0, b0, 1e-6, T),
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


def _reweight_case(partls, storage, on_device, N, M, K, flags, zeros, seed, eta=0.3):
    X, y, P, _, _ = _data(seed, N, M, K)
    if storage == "csr":
        X = sparsify(X, seed)
    X = X.astype(np.float32).astype(np.float64) if storage == "f32" else X
    w = weights_with_zeros(N, seed) if zeros else np.random.default_rng(seed).uniform(0.25, 4.0, N)
    used, fresh = partls.Context(0), partls.Context(0)
    try:
        keep = _prepare(partls, used, storage, on_device, X, y, P, eta, flags, None)
        used.opt_sweep()                                     # the problem has been in use
        if on_device:
            dw = OnDevice(w=w)
            used.opt_reweight_device(dw.ptr("w"))
        else:
            used.opt_reweight(w)
        assert used.upload() == (0.0, 0.0)
        keep2 = _prepare(partls, fresh, storage, on_device, X, y, P, eta, flags, w)
        bad = diff(flat(_staged(used, M, K, seed)), flat(_staged(fresh, M, K, seed)))
        assert not bad, (storage, on_device, bad)
        del keep, keep2
    finally:
        used.close()
        fresh.close()


@pytest.mark.parametrize("zeros", [False, True], ids=["weighted", "zeros"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("storage", ["f64", "f32", "csr"])
def test_reweight_equals_a_fresh_weighted_prepare(partls, storage, on_device, zeros):
    _reweight_case(partls, storage, on_device, 300, 11, 3, FAITHFUL, zeros, 51)        # n = 12: the 256-thread register kernel


@pytest.mark.parametrize("M,K,flags", [(39, 3, FAITHFUL | GENERIC), (300, 2, FAITHFUL)], ids=["n40-generic", "n301"])
def test_reweight_on_the_other_sweep_routes(partls, M, K, flags):
    _reweight_case(partls, "f64", False, 700, M, K, flags, True, 52)
    if M == 300:
        _reweight_case(partls, "csr", False, 700, M, K, flags, False, 53)


def test_reweight_by_the_last_robust_weights(partls):
    """w == NULL: the weights of the last partls_robust_weights call, also after a later call has moved on; and a free intercept"""
    X, y, P, ma, mb = _data(54, 300, 11)
    used, fresh = partls.Context(0), partls.Context(0)
    used.opt_prepare(X, y, P, 0.0, 0)
    with pytest.raises(partls.PartlsError) as e:
        used.opt_reweight()                                   # no robust_weights since the prepare
    assert e.value.status == partls.lowlevel.ERR_STATE and used.opt_sweep()[3] == 0          # (refused before anything was touched)
    w1 = used.robust_weights(*ma, loss="bisquare")["weights"]
    used.opt_reweight()
    assert used.upload() == (0.0, 0.0)
    info2 = used.robust_weights(*mb, loss="bisquare")        # moves the kept weights on; the prepared problem keeps its own copy
    assert info2["max_dw"] == float(np.max(np.abs(info2["weights"] - w1)))               # the record survived the re-prepare
    fresh.opt_prepare(X, y, P, 0.0, 0, weights=w1)
    assert _same_bits(used.gram(), fresh.gram())
    su, sf = used.opt_sweep(), fresh.opt_sweep()
    assert not diff(flat(su), flat(sf)) and not diff(flat(used.opt_finish(su[1])), flat(fresh.opt_finish(sf[1])))
    used.opt_prepare(X, y, P)                                 # every other prepare clears the record
    with pytest.raises(partls.PartlsError):
        used.opt_reweight()
    used.close()
    fresh.close()


@pytest.mark.parametrize("storage", ["f64", "f32", "csr"])
def test_reweight_refuses_what_a_weighted_prepare_refuses(partls, storage):
    L = partls.lowlevel
    X, y, P, _, _ = _data(55, 300, 5)
    if storage == "csr":
        X = sparsify(X, 55)
    one = np.ones(300)
    bads = {"negative": np.r_[one[:-1], -1.0], "nan": np.r_[one[:-1], np.nan], "inf": np.r_[np.inf, one[:-1]], "zero sum": np.zeros(300)}
    used, fresh = partls.Context(0), partls.Context(0)
    for name, w in bads.items():
        _prepare(partls, used, storage, False, X, y, P, 0.0, 0, None)
        with pytest.raises(partls.PartlsError) as e1:
            used.opt_reweight(w)
        msg = L.lib().partls_last_error().decode()
        with pytest.raises(partls.PartlsError) as e2:
            _prepare(partls, fresh, storage, False, X, y, P, 0.0, 0, w)
        assert e1.value.status == e2.value.status == (L.ERR_NONFINITE if name in ("nan", "inf") else L.ERR_BAD_ARG), name
        assert msg == L.lib().partls_last_error().decode() and "weight" in msg, name
        for c in (used, fresh):                               # unprepared, as after a refused prepare
            with pytest.raises(partls.PartlsError) as e3:
                c.opt_sweep()
            assert e3.value.status == L.ERR_STATE, name
        with pytest.raises(partls.PartlsError) as e4:
            used.opt_reweight(one)
        assert e4.value.status == L.ERR_STATE, name
    used.close()
    fresh.close()


# ---- 3. fit_robust -------------------------------------------------------------------------------------------------------------------------
def _fit_case(seed=61, N=300, M=10, K=3):
    X, y, P, _, _ = _data(seed, N, M, K, outliers=0.1)
    rng = np.random.default_rng(seed)
    return X, y, P, rng.random(M + 1), (rng.random(K + 1) - 0.5) * 10


def _robust(partls, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", partls.RobustConvergenceWarning)
        warnings.simplefilter("ignore", partls.IllConditionedWarning)
        return partls.fit_robust(*args, **kw)


def _against_host_loop(partls, alg, X, y, P, loss, **kw):
    host = R.host_loop(partls, alg, X, y, P, loss=loss, max_iter=8, **kw)
    model, _, rep = _robust(partls, alg, X, y, P, loss=loss, max_iter=8, **kw)
    rb = rep.robust
    print("[robust] %s %s: iterations %d, scales %r, max_dw %r" % (alg.__name__, loss, rb.iterations, rb.scales, rb.max_dw))
    assert host["iterations"] >= 2                            # the loop has something to agree on
    assert (rb.iterations, rb.converged, rb.exact) == (host["iterations"], host["converged"], host["exact"])
    assert _same_bits(rb.scales, host["scales"]) and _same_bits(rb.max_dw, host["max_dw"])
    assert _same_bits(rb.weights, host["weights"]) and rb.scale == host["scales"][-1] and rb.loss == loss
    m, r = host["models"][-1], host["reports"][-1]
    assert _same_bits(model.α, m.α) and _same_bits(model.β, m.β) and _same_bits(model.t, m.t) and _same_bits(rep.opt, r.opt)
    for k in ("best_index", "iters", "nopen"):
        assert (k in rep) == (k in r) and (k not in r or rep[k] == r[k]), k
    assert len(rb.rho_sum) == len(rb.max_dw) == len(rb.scales) == len(host["scales"])
    for got, want in zip(rb.rho_sum, host["rho_sum"]):
        assert abs(got - want) <= (len(y) + 8) * U * want
    assert (rb.n_down, rb.n_zero) == (int(np.sum(rb.weights < 1.0)), int(np.sum(rb.weights == 0.0)))


@pytest.mark.parametrize("faithful,eta,loss", [(False, 0.0, "huber"), (False, 0.5, "bisquare"), (True, 0.0, "bisquare"), (True, 0.5, "huber")])
def test_fit_robust_opt_against_the_host_loop(partls, faithful, eta, loss):
    X, y, P, _, _ = _fit_case()
    _against_host_loop(partls, partls.Opt, X, y, P, loss, η=eta, faithful_intercept=faithful)


@pytest.mark.parametrize("loss", LOSSES)
def test_fit_robust_alt_and_bnb_against_the_host_loop(partls, loss):
    X, y, P, a0, b0 = _fit_case(62)
    _against_host_loop(partls, partls.Alt, X, y, P, loss, alpha0=a0, beta0=b0, η=0.5 if loss == "huber" else 0.0)
    _against_host_loop(partls, partls.BnB, X, y, P, loss, η=0.0 if loss == "huber" else 0.5)


def test_fit_robust_float32_and_csr_against_the_host_loop(partls):
    X, y, P, a0, b0 = _fit_case(63)
    X32 = np.asfortranarray(X.astype(np.float32))
    _against_host_loop(partls, partls.Opt, X32, y, P, "huber")
    _against_host_loop(partls, partls.Alt, X32, y, P, "bisquare", alpha0=a0, beta0=b0)
    csr = to_csr(partls, sparsify(X, 63, keep=0.6))
    _against_host_loop(partls, partls.Opt, csr, y, P, "bisquare", η=0.5)
    _against_host_loop(partls, partls.BnB, csr, y, P, "huber")


def test_a_huge_tuning_constant_is_the_plain_fit(partls):
    X, y, P, a0, b0 = _fit_case(64)
    for alg, kw in ((partls.Opt, {}), (partls.Opt, dict(faithful_intercept=True, η=0.5)), (partls.Alt, dict(alpha0=a0, beta0=b0)),
                    (partls.BnB, {})):
        model, _, rep = partls.fit_robust(alg, X, y, P, loss="huber", c=1e300, **kw)
        plain, _, prep = partls.fit(alg, X, y, P, **kw)
        rb = rep.robust
        assert np.array_equal(rb.weights, np.ones(len(y))) and rb.iterations == 0 and rb.converged and not rb.exact
        assert rb.max_dw == [0.0] and (rb.n_down, rb.n_zero) == (0, 0) and len(rb.scales) == 1 and rb.c == 1e300
        assert _same_bits(model.α, plain.α) and _same_bits(model.β, plain.β) and _same_bits(model.t, plain.t)
        assert _same_bits(rep.opt, prep.opt)


@pytest.mark.parametrize("loss", LOSSES)
def test_the_loss_descends_under_a_fixed_scale(partls, loss):
    """MM: the weighted least-squares objective majorises the loss at the current residuals and fit(Opt) minimises it exactly over all
    sign patterns, so rho_sum cannot rise.  Margin: the summation bound on both sides, and ten times the sweep's near-tie window (1e-13
    of y'Wy <= y'y, DESIGN.md §4.7, within which the finish may re-rank the winner), in units of the scale"""
    X, y, P, _, _ = _fit_case(65)
    s = 0.2
    _, _, rep = _robust(partls, partls.Opt, X, y, P, loss=loss, scale=s, max_iter=12, tol=1e-9)
    rho = rep.robust.rho_sum
    print("[robust] descent %s: %r" % (loss, rho))
    assert len(rho) >= 4 and rep.robust.scales == [s] * len(rho)
    for j in range(len(rho) - 1):
        assert rho[j + 1] <= rho[j] + 4 * (len(y) + 8) * U * rho[j] + 1e-12 * float(y @ y) / (s * s), (j, rho[j], rho[j + 1])
    assert rho[-1] < rho[0]


PLANTED_SEED = 0


def planted(seed, N=300, sigma=0.1):
    """y = X w* + t* + noise(sigma) with the planted signs (+, +, -) of three groups; the tenth of the rows where group 1's features are
    lowest is shifted by +50 sigma, which drags group 1's slope below zero in a plain fit"""
    rng = np.random.default_rng(seed)
    M, K = 9, 3
    X = np.asfortranarray(rng.normal(0.0, 1.0, (N, M)))
    P = _partition(M, K)
    alpha = rng.uniform(0.5, 1.0, M)
    for k in range(K):
        alpha[P[:, k] == 1] /= alpha[P[:, k] == 1].sum()
    beta = np.array([2.0, 0.6, -1.5])
    w = alpha * (P @ beta)
    z = X[:, P[:, 1] == 1] @ alpha[P[:, 1] == 1]
    shifted = np.zeros(N, dtype=bool)
    shifted[np.argsort(z)[:N // 10]] = True
    y = X @ w + 1.0 + sigma * rng.normal(size=N)
    y[shifted] += 50 * sigma
    return X, y, P, w, np.sign(beta), shifted


def test_planted_outliers(partls):
    """PLANTED_SEED is a seed for which the host loop of weighted fits (tests/robust_reference.py: host_loop, bisquare, 9 re-weighted
    fits) shows all three properties, with these margins: the plain fit's signs are (+, -, -) against the planted (+, +, -) and its
    largest coefficient error is 0.6809; the loop's last model has the planted signs and an error of 0.0123; the largest weight of a
    shifted row is 0 against a median weight of 0.96873 over the clean rows.  (The seeds 1 to 5 show the same picture.)"""
    X, y, P, w, signs, shifted = planted(PLANTED_SEED)
    plain, _, _ = partls.fit(partls.Opt, X, y, P)
    model, _, rep = _robust(partls, partls.Opt, X, y, P, loss="bisquare")
    err = lambda m: float(np.max(np.abs(m.α * (P @ m.β) - w)))           # noqa: E731
    wt = rep.robust.weights
    print("[robust] planted: plain signs %r err %.4f; robust signs %r err %.4f; shifted max w %.4f, clean median w %.4f, iterations %d"
          % (np.sign(plain.β), err(plain), np.sign(model.β), err(model), wt[shifted].max(), np.median(wt[~shifted]), rep.robust.iterations))
    assert not np.array_equal(np.sign(plain.β), signs)       # the plain fit's winning sign pattern is not the planted one ...
    assert np.array_equal(np.sign(model.β), signs)           # ... the robust fit's is
    assert err(model) < err(plain)
    assert wt[shifted].max() < np.median(wt[~shifted])


def test_running_out_of_iterations(partls):
    X, y, P, _, _ = _fit_case(66)
    host = R.host_loop(partls, partls.Opt, X, y, P, loss="huber", max_iter=1, tol=0.0)
    with pytest.warns(partls.RobustConvergenceWarning):
        model, _, rep = partls.fit_robust(partls.Opt, X, y, P, loss="huber", max_iter=1, tol=0.0)
    assert not rep.robust.converged and not rep.robust.exact and rep.robust.iterations == 1 and len(rep.robust.max_dw) == 1
    assert len(host["models"]) == 2 and not host["converged"]
    m1 = host["models"][1]
    assert _same_bits(model.α, m1.α) and _same_bits(model.β, m1.β) and _same_bits(model.t, m1.t)
    assert _same_bits(rep.robust.weights, host["weights"])


def test_the_default_context_afterwards(partls, monkeypatch):
    """after fit_robust a plain fit on the same default context returns what a fresh context returns"""
    X, y, P, a0, b0 = _fit_case(67)
    X2, y2, P2, _, _ = _fit_case(68, N=257, M=7, K=2)
    _robust(partls, partls.Opt, X, y, P, loss="bisquare", max_iter=3)
    used = [partls.fit(partls.Opt, X2, y2, P2, η=0.5), partls.fit(partls.Opt, X, y, P, weights=weights_with_zeros(len(y), 1)),
            partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0), partls.fit(partls.BnB, X2, y2, P2)]
    fresh = partls.Context(0)
    monkeypatch.setattr(partls.api, "default_context", lambda device=0: fresh)
    want = [partls.fit(partls.Opt, X2, y2, P2, η=0.5), partls.fit(partls.Opt, X, y, P, weights=weights_with_zeros(len(y), 1)),
            partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0), partls.fit(partls.BnB, X2, y2, P2)]
    monkeypatch.undo()
    fresh.close()
    for (mu, _, ru), (mf, _, rf) in zip(used, want):
        assert _same_bits(mu.α, mf.α) and _same_bits(mu.β, mf.β) and _same_bits(mu.t, mf.t) and not diff(flat(dict(ru)), flat(dict(rf)))


# ---- 4. the selection on planted residuals: thresholds that part early, and more than one trip of the histogram loop ---------------------
def _planted_residuals(a, seed):
    """a problem whose absolute residuals at an all-zero model are exactly a: one column, beta = 0 and t = 0 predict 0, y = +-a"""
    rng = np.random.default_rng(seed)
    N = len(a)
    X = np.asfortranarray(rng.normal(0.5, 1.0, (N, 1)))
    y = a * rng.choice([-1.0, 1.0], N)
    P = np.ones((1, 1), dtype=np.int64)
    model = (np.ones(1), np.zeros(1), 0.0)
    return X, y, P, model


def _check_planted(ctx, a, seed, where):
    """both losses on the planted residuals a, through _check: scale and weights bit for bit, counts exact, the loss within its bound"""
    a = np.asarray(a, dtype=np.float64)
    X, y, P, model = _planted_residuals(a, seed)
    for loss in LOSSES:
        ctx.opt_prepare(X, y, P)
        if loss == LOSSES[0]:
            assert _same_bits(_abs_res(ctx, X, y, P, model), a), where            # the residuals are the planted values
        _check(ctx.robust_weights(*model, loss=loss), a, loss, where=" %s N=%d" % (where, len(a)))


def _two_clusters(rng, N, lo, hi):
    """N / 2 values in [lo, 2 lo] and N / 2 in [hi, 2 hi], shuffled: a_(lo) is the largest of the first cluster, a_(hi) the smallest
    of the second"""
    assert N % 2 == 0
    a = np.concatenate([rng.uniform(lo, 2 * lo, N // 2), rng.uniform(hi, 2 * hi, N // 2)])
    rng.shuffle(a)
    return a


def _middle_keys(a):
    s = np.sort(a)
    N = len(s)
    return int(s[(N - 1) // 2:(N - 1) // 2 + 1].view(np.uint64)[0]), int(s[N // 2:N // 2 + 1].view(np.uint64)[0])


@pytest.mark.parametrize("N", [2, 256, 4098])
def test_thresholds_that_part_in_the_first_passes(partls, ctx, N):
    """the two order statistics of an even N ride the same eight passes, each with its own prefix filter and its own rank inside its
    own bucket from the pass in which their digits differ: pass 0 (another exponent byte) and pass 1 (the same top byte, another
    second byte) here, against the last bytes on continuous residuals.  Then a_(lo) = 0 and a_(lo) = the smallest denormal under a
    normal a_(hi) (keys 0 and 1 against 0x3f..), and an exact tie of the two inside a cluster of neighbours one ulp apart, where the
    thresholds never part and both ranks fall into one bucket of the last pass"""
    rng = np.random.default_rng(7000 + N)
    a = _two_clusters(rng, N, 1e-3, 1e3)
    klo, khi = _middle_keys(a)
    assert klo >> 56 != khi >> 56
    _check_planted(ctx, a, N, "split in pass 0")
    a = _two_clusters(rng, N, 1e-2, 1.0)
    klo, khi = _middle_keys(a)
    assert klo >> 56 == khi >> 56 and klo >> 48 != khi >> 48
    _check_planted(ctx, a, N + 1, "split in pass 1")
    for tiny, name in ((0.0, "zero"), (5e-324, "denormal")):
        a = np.concatenate([np.full(N // 2, tiny), rng.uniform(0.5, 4.0, N // 2)])
        rng.shuffle(a)
        klo, khi = _middle_keys(a)
        assert klo == (0 if tiny == 0.0 else 1) and khi >> 56 in (0x3f, 0x40)
        ref = R.robust_info(a, "huber")
        assert ref["scale"] > 0.0
        _check_planted(ctx, a, N + 2, name + " meets a normal")
    # the tie: keys base + offset, offsets within the last byte; N / 2 - 1 below 0 (one of them -1), two zeros, N / 2 - 1 above (one +1)
    base = int(np.array([1.5]).view(np.uint64)[0]) + 128
    half = N // 2 - 1
    off = np.concatenate([rng.integers(-100, 0, half), [0, 0], rng.integers(1, 101, half)])
    if half:
        off[0], off[-1] = -1, 1
    a = (np.uint64(base) + off.astype(np.int64).astype(np.uint64)).view(np.float64)
    rng.shuffle(a)
    klo, khi = _middle_keys(a)
    assert klo == khi == base and np.all(a.view(np.uint64) >> np.uint64(8) == np.uint64(base >> 8))
    _check_planted(ctx, a, N + 3, "tie at the median")


@pytest.mark.parametrize("N,split", [(262145, False), (262146, False), (262146, True), (600001, False)])
def test_more_than_one_trip_of_the_histogram_loop(partls, ctx, N, split):
    """the histogram grid is capped at 1024 workgroups of 256 rows: at N = 262 145 (odd: one statistic) and 262 146 (even: two)
    workgroup 0 makes a second trip of one and of two rows, at N = 600 001 the workgroups make three trips, the last one by 296 of
    them and ragged; continuous residuals, and at N = 262 146 also the two clusters that part the thresholds in pass 0"""
    assert N > 1024 * 256
    rng = np.random.default_rng(N + split)
    a = _two_clusters(rng, N, 1e-3, 1e3) if split else np.abs(rng.standard_normal(N)) * 10.0 ** rng.uniform(-2.0, 2.0, N)
    _check_planted(ctx, a, N, "split, second trip" if split else "trips")
