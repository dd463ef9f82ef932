"""float32 design matrices on the GPU.  The contract is equality: a float32 X is uploaded, kept and read as float32,
every kernel that reads it widens each element to double as it loads it (exact), and all arithmetic stays fp64 in the order of the fp64
path — so every output of the float32 path equals the fp64 path on X.astype(float64) bit for bit.  Every comparison below is
np.array_equal / ==, never a tolerance.  Covered: the Gram over ragged shapes, tile edges, chunk / slice splits, odd leading dimensions
on device tensors, weights, subnormal and huge entries; the three fits on every sweep route; returnAllSolutions after the context was
taken over; predict from host and device; the bytes the upload moved; the error rules; the paths that keep widening on the host."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAITHFUL = 1


def _problem(seed, N, M, K):
    """real-valued, uncentred float32 data (y and the weights are float64, as the ABI takes them)"""
    rng = np.random.default_rng(seed)
    X = rng.normal(1.0, 1.0, size=(N, M)).astype(np.float32)
    grp = np.concatenate([np.arange(K), rng.integers(0, K, M - K)]) if M >= K else np.arange(M) % K
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), grp] = 1
    y = X.astype(np.float64) @ rng.normal(0.0, 1.0, M) + 2.0 + 0.3 * rng.normal(size=N)
    w = 10.0 ** rng.uniform(-1.5, 1.5, N)
    return X, y, P, w


def _same_fit(r32, r64):
    (m1, _, p1), (m2, _, p2) = r32, r64
    assert np.array_equal(m1.α, m2.α) and np.array_equal(m1.β, m2.β) and m1.t == m2.t
    assert set(p1) == set(p2)
    for k in ("opt", "best_index", "nopen", "iters"):
        if k in p2:
            assert p1[k] == p2[k], k


# ---- 1. the Gram ----------------------------------------------------------------------------------------------------------------------
def _device_f32(X):
    """X (N x M float32) column-major in HBM the awkward way: an ODD leading dimension > N (every second column starts on a 4-byte
    boundary only) and a base address one float past an aligned allocation; the padding holds NaN, which nothing may read as data.
    Returns (tensor that owns the memory, address of X[0, 0], ldX)."""
    import torch
    N, M = X.shape
    ldX = N + (3 if N % 2 == 0 else 2)
    host = np.full(1 + M * ldX, np.nan, dtype=np.float32)
    host[1:].reshape(M, ldX)[:, :N] = X.T
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + 4, ldX


def _gram_pair(ctx, X32, y, P, w, device):
    """(Gram after the float32 prepare, Gram after the fp64 prepare of the widened data)"""
    N, M = X32.shape
    if device:
        import torch
        keep, dX_ptr, ldX = _device_f32(X32)
        assert ldX % 2 == 1 and ldX > N and dX_ptr % 8 == 4
        dy = torch.from_numpy(y).cuda()
        dw = torch.from_numpy(w).cuda() if w is not None else None
        ctx.opt_prepare_device(dX_ptr, dy.data_ptr(), N, M, ldX, P, 0.0, 0, dw_ptr=None if dw is None else dw.data_ptr(),
                               dtype=np.float32)
        assert ctx.upload() == (0.0, 0.0)
    else:
        ctx.opt_prepare(X32, y, P, 0.0, weights=w)
    G32 = ctx.gram()
    if device:
        torch.cuda.synchronize()
        del keep, dy, dw
    ctx.opt_prepare(X32.astype(np.float64), y, P, 0.0, weights=w)
    return G32, ctx.gram()


GRAM_SHAPES = [(5, 3), (37, 5), (1000, 130), (2051, 257)]    # < one 16-sample panel; a row tail; two tiles, 2-column edge; three, edge of 1


def _gram_data(N, M):
    X, y, _, w = _problem(100 + N, N, M, 1)
    if (N, M) == (37, 5):                                   # the values a narrower conversion would lose
        X[:, 4] = 0.0
        X[2, 4] = np.float32(1e-42)                         # subnormal floats: a flushed conversion leaves column 4 empty
        X[7, 4] = np.float32(-3e-45)
        X[3, 1] = np.float32(3e38)                          # near FLT_MAX: the square needs the double range
        X[2, 1] = np.float32(-2.5e38)                       # ... and shares a row with a subnormal (cross term 1e-42 * 2.5e38)
    return X, y, np.ones((M, 1), dtype=np.int64), w


@pytest.mark.parametrize("N,M", GRAM_SHAPES)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_gram_equals_the_widened_fp64_gram(partls, N, M, device):
    X, y, P, w = _gram_data(N, M)
    ctx = partls.Context(0)
    for wt in (None, w):
        G32, G64 = _gram_pair(ctx, X, y, P, wt, device)
        assert np.array_equal(G32, G64), f"weights={wt is not None}: {np.count_nonzero(G32 != G64)} entries differ"
        assert np.all(np.isfinite(G32))
        if (N, M) == (37, 5):
            assert G32[4, 4] > 0.0 and G32[1, 4] != 0.0       # the subnormals arrived
    ctx.close()


def test_gram_over_several_chunks_and_slices(partls, monkeypatch):
    """2051 rows in 64-row chunks over 3 slices per XCD group: partial tiles of many workgroups, a ragged last chunk"""
    monkeypatch.setenv("PARTLS_GRAM_CR", "64")
    monkeypatch.setenv("PARTLS_GRAM_S", "3")
    ctx = partls.Context(0)                                  # the knobs are read at creation
    monkeypatch.delenv("PARTLS_GRAM_CR")
    monkeypatch.delenv("PARTLS_GRAM_S")
    X, y, P, w = _gram_data(2051, 257)
    for device in (False, True):
        for wt in (None, w):
            G32, G64 = _gram_pair(ctx, X, y, P, wt, device)
            assert np.array_equal(G32, G64), (device, wt is not None)
    # the knobs took effect: the default plan sums the same products in another order, so its Gram agrees to the rounding of a sum of
    # N products, |error| <= N u sum_i |a_i b_i| <= N u sqrt(G_aa G_bb) per order (u = 2^-53), but not in every bit
    ref = partls.Context(0)
    ref.opt_prepare(X.astype(np.float64), y, P, 0.0, weights=w)
    R = ref.gram()
    d = np.sqrt(np.outer(np.diag(R), np.diag(R)))
    assert np.all(np.abs(R - G64) <= 2051 * 2.0 ** -52 * d)
    assert np.any(R != G64), "PARTLS_GRAM_CR / PARTLS_GRAM_S were ignored: the Gram equals the default plan's in every bit"
    ref.close()
    ctx.close()


# ---- 2. the fits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_fits_equal_the_widened_fp64_fits(partls, eta, weighted):
    X, y, P, w = _problem(7, 300, 12, 3)
    X64 = X.astype(np.float64)
    kw = dict(η=eta, weights=w if weighted else None)
    for faithful in (False, True):
        for generic in (False, True):
            o = dict(faithful_intercept=faithful, generic_kernel=generic, **kw)
            _same_fit(partls.fit(partls.Opt, X, y, P, **o), partls.fit(partls.Opt, X64, y, P, **o))
    rng = np.random.default_rng(3)
    a0, b0 = rng.random(13), (rng.random(4) - 0.5) * 10
    r32 = partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0, **kw)
    _same_fit(r32, partls.fit(partls.Alt, X64, y, P, alpha0=a0, beta0=b0, **kw))
    assert r32[2].iters >= 1
    r32 = partls.fit(partls.BnB, X, y, P, **kw)
    _same_fit(r32, partls.fit(partls.BnB, X64, y, P, **kw))
    assert r32[2].nopen >= 1


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_fits_on_the_deferred_update_route(partls, weighted):
    """n > 288: the global-memory tableau kernels, the cooperative single solves and their data passes.
    The weighted fit(BnB) is held to what the fp64 path itself repeats from run to run: report.opt and nopen.  Its α, β, t come from a
    leaf solved by the cooperative kernel (sweep_coop.hip), which on this problem returns one of two last-bit patterns for identical
    inputs whatever the element type — a defect of that kernel, older than the float32 path ("Known defect")."""
    X, y, P, w = _problem(9, 400, 300, 4)
    X64 = X.astype(np.float64)
    kw = dict(η=0.5, weights=w if weighted else None)
    for faithful in (False, True):
        _same_fit(partls.fit(partls.Opt, X, y, P, faithful_intercept=faithful, **kw),
                  partls.fit(partls.Opt, X64, y, P, faithful_intercept=faithful, **kw))
    assert partls.default_context().sweep_route()[0] == partls.lowlevel.ROUTE_DEFERRED
    rng = np.random.default_rng(4)
    a0, b0 = rng.random(301), (rng.random(5) - 0.5) * 10
    _same_fit(partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0, T=4, **kw),
              partls.fit(partls.Alt, X64, y, P, alpha0=a0, beta0=b0, T=4, **kw))
    r32, r64 = partls.fit(partls.BnB, X, y, P, **kw), partls.fit(partls.BnB, X64, y, P, **kw)
    if not weighted:
        _same_fit(r32, r64)
    else:
        assert set(r32[2]) == set(r64[2]) and r32[2].opt == r64[2].opt and r32[2].nopen == r64[2].nopen
        assert r32[0].α.shape == r64[0].α.shape and np.all(np.isfinite(r32[0].α)) and np.isfinite(r32[0].t)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_return_all_solutions_survives_a_later_fit(partls, weighted):
    X, y, P, w = _problem(12, 300, 12, 3)
    X64 = X.astype(np.float64)
    kw = dict(η=0.5, returnAllSolutions=True, weights=w if weighted else None)
    _, _, r32 = partls.fit(partls.Opt, X, y, P, **kw)
    s32 = r32.solutions
    assert s32._problem[0].dtype == np.float32 and s32._problem[0].flags.f_contiguous
    arr32 = s32.arrays()
    first32 = [s32[b] for b in (0, 5, 15)]
    _, _, r64 = partls.fit(partls.Opt, X64, y, P, **kw)       # takes the shared context over
    s64 = r64.solutions
    for a, b in zip(arr32, s64.arrays()):
        assert np.array_equal(a, b)
    again32 = [s32[b] for b in (0, 5, 15)]                   # re-prepared on a private context, through the float32 path
    assert s32._ctx is not partls.default_context()
    assert s32._ctx.upload()[1] == 4.0 * X.size
    for (o1, m1), (o2, m2), b in zip(first32, again32, (0, 5, 15)):
        o3, m3 = s64[b]
        assert o1 == o2 == o3
        for m in (m2, m3):
            assert np.array_equal(m1.α, m.α) and np.array_equal(m1.β, m.β) and m1.t == m.t


# ---- 3. predict -----------------------------------------------------------------------------------------------------------------------
def test_predict_host_and_device(partls):
    import torch
    X, y, P, _ = _problem(13, 1500, 21, 3)
    model, _, _ = partls.fit(partls.Opt, X, y, P)
    ref = partls.predict(model, X.astype(np.float64))
    assert np.array_equal(partls.predict(model, X), ref)
    assert np.array_equal(partls.predict(model, np.ascontiguousarray(X)), ref)           # C order: copied to F order, not widened
    assert np.array_equal(partls.predict(model.α, model.β, model.t, model.P, X[::2]), ref[::2])
    keep, dX_ptr, ldX = _device_f32(X)
    dyh = torch.zeros(X.shape[0], dtype=torch.float64, device="cuda")
    partls.predict_device(model, dX_ptr, X.shape[0], ldX, dyh.data_ptr(), dtype=np.float32)
    torch.cuda.synchronize()
    assert np.array_equal(dyh.cpu().numpy(), ref)


# ---- 4. nothing was widened on the way ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(37, 5), (70001, 31)], ids=["plain-copy", "staged"])
def test_upload_moves_four_bytes_per_element(partls, N, M):
    """(70001, 31): 8.7 MB of floats — above the 8 MB switch to the staged, page-locked upload, whose column batches end mid-buffer"""
    X, y, P, _ = _problem(14, N, M, 1)
    ctx = partls.Context(0)
    ctx.opt_prepare(X, y, P, 0.0)
    assert ctx.upload()[1] == 4.0 * N * M
    assert (4 * N * M > (8 << 20)) == (N > 1000)             # the large case takes the staged path, the small one the plain copy
    G32 = ctx.gram()
    ctx.opt_prepare(X.astype(np.float64), y, P, 0.0)
    assert ctx.upload()[1] == 8.0 * N * M
    assert np.array_equal(G32, ctx.gram())
    ctx.close()


# ---- 5. errors and the paths that keep widening ----------------------------------------------------------------------------------------
def test_nonfinite_and_leading_dimension_errors(partls):
    L = partls.lowlevel
    X, y, P, _ = _problem(15, 200, 6, 2)
    ctx = partls.Context(0)
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[17, 3] = bad
        with pytest.raises(partls.PartlsError) as e:
            ctx.opt_prepare(Xb, y, P, 0.0)
        assert e.value.status == L.ERR_NONFINITE
        with pytest.raises(partls.PartlsError) as e:
            partls.fit(partls.Opt, Xb, y, P)
        assert e.value.status == L.ERR_NONFINITE
    Xf = np.asfortranarray(X)
    Pf = np.asfortranarray(P)
    N, M = X.shape
    st = L.lib().partls_opt_prepare_f32(ctx._h, Xf.ctypes.data, N, M, N - 1, y.ctypes.data, None, 0, Pf.ctypes.data, 2, M, 0.0, 0)
    assert st == L.ERR_BAD_ARG
    yh = np.zeros(N)
    dp = C.POINTER(C.c_double)
    st = L.lib().partls_predict_f32(ctx._h, Xf.ctypes.data, N, M, N - 1, Pf.ctypes.data, 2, M, np.ones(M).ctypes.data_as(dp),
                                    np.ones(2).ctypes.data_as(dp), 0.0, yh.ctypes.data_as(dp))
    assert st == L.ERR_BAD_ARG
    ctx.opt_prepare(X, y, P, 0.0)                            # the context is usable afterwards
    assert np.all(np.isfinite(ctx.gram()))
    ctx.close()


def test_multi_contexts_refuse_float32_and_stay_usable(partls):
    L = partls.lowlevel
    X, y, P, _ = _problem(16, 200, 6, 2)
    mc = partls.MultiContext([0, 0])
    c0 = mc.context(0)
    with pytest.raises(partls.PartlsError) as e:
        c0.opt_prepare(X, y, P, 0.0)
    assert e.value.status == L.ERR_UNSUPPORTED
    c0.opt_prepare(X.astype(np.float64), y, P, 0.0)          # a plain fp64 prepare on the same context works ...
    fresh = partls.Context(0)
    fresh.opt_prepare(X.astype(np.float64), y, P, 0.0)
    assert np.array_equal(c0.gram(), fresh.gram())          # ... and matches a fresh context
    bo, bp, _, un = c0.opt_sweep()
    assert (bo, bp, un) == fresh.opt_sweep()[:2] + (0,)
    fresh.close()
    mc.close()


def test_devices_and_cross_validate_keep_widening(partls):
    X, y, P, _ = _problem(17, 300, 12, 3)
    X64 = X.astype(np.float64)
    _same_fit(partls.fit(partls.Opt, X, y, P, devices=[0, 0]), partls.fit(partls.Opt, X64, y, P, devices=[0, 0]))
    (m1, _, p1), (m2, _, p2) = partls.fit(partls.BnB, X, y, P, devices=[0, 0]), partls.fit(partls.BnB, X64, y, P, devices=[0, 0])
    assert np.array_equal(m1.α, m2.α) and np.array_equal(m1.β, m2.β) and m1.t == m2.t and p1.opt == p2.opt
    kw = dict(η=[0.0, 0.3], nfolds=3)
    a = partls.cross_validate(partls.Opt, X, y, P, **kw)
    b = partls.cross_validate(partls.Opt, X64, y, P, **kw)
    for k in ("sse", "mse", "mse_mean", "opt", "best_index", "status"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for ma, mb in zip(a.path, b.path):
        assert np.array_equal(ma.α, mb.α) and np.array_equal(ma.β, mb.β) and ma.t == mb.t
    # a float32 fit right after the cross-validation (which leaves a double upload behind) still goes through the float32 path
    _same_fit(partls.fit(partls.Opt, X, y, P), partls.fit(partls.Opt, X64, y, P))
