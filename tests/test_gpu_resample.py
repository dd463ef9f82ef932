"""partls_opt_weightings / bootstrap / resample on the GPU: every column of one batched call against the single
weighted fit(Opt) of that column and against the weighted oracle (S-scaled data, η rows unweighted); the all-ones column against the
unweighted fit bit for bit; independence of the position in the batch, the serial route, every sweep route; the out-of-bag error
against numpy; argument errors that write nothing; per-problem status; host against device inputs; bootstrap end to end."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAITHFUL = 1
GENERIC = 2
NEAR_TIE_REL = 1e-12          # on obj^2 in units of y'Wy: the documented window (1e-13) with room for two summation orders (test_gpu_cv.py)


def _shape(seed, N, D, K):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    grp = np.arange(D) % K
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    y = X @ (rng.random(D) * ((rng.random(K) - 0.5) * 10)[grp]) + 0.7 + 0.5 * rng.standard_normal(N)
    return X, y, P


def _columns(seed, N):
    """the six weightings of test 1: all ones; multinomial counts; a 0/1 mask; real-valued positive; counts with a block of zero rows at
    the start; counts with a block of zero rows at the end"""
    rng = np.random.default_rng(seed)
    counts = lambda: rng.multinomial(N, np.full(N, 1 / N)).astype(np.float64)      # noqa: E731
    head, tail = counts(), counts()
    head[:N // 5] = 0.0
    tail[-(N // 7):] = 0.0
    return np.asfortranarray(np.stack([np.ones(N), counts(), (rng.random(N) < 0.7).astype(np.float64), 10.0 ** rng.uniform(-1.5, 1.5, N),
                                       head, tail], axis=1))


def _oracle_objs(oracle, X, y, P, w, eta):
    """objective of every pattern of the weighted problem from the oracle (tests/test_gpu_weights.py: S-scaled homogeneous data, the η
    rows unweighted), indexed as best_index is with and without FAITHFUL: the reference's 2^(K+1) patterns"""
    Xo, Po = oracle.homogeneous(X, P)
    s = np.sqrt(w)
    Xn, yn = oracle.regularize(np.asfortranarray(Xo * s[:, None]), y * s, Po, eta)
    K = P.shape[1]
    return np.asarray(oracle.opt_patterns(Xn, yn, Po, np.arange(1 << (K + 1))))


def _close_models(a, b, t, o, bi, ra, rb, rt, ro, rbi, yy, what, objs=None):
    """test_gpu_cv.py::_check's tolerances: alpha 1e-9 scale, beta rtol 1e-9, opt 1e-10 relative; another winner only inside the near-tie window"""
    if bi == rbi:
        sc = max(1.0, np.abs(ra).max(), np.abs(rb).max())
        assert np.allclose(a, ra, rtol=0, atol=1e-9 * sc), f"{what}: alpha {np.abs(a - ra).max()}"
        assert np.allclose(b, rb, rtol=1e-9, atol=1e-9 * sc), f"{what}: beta {np.abs(b - rb).max()}"
        assert abs(t - rt) <= 1e-9 * max(1.0, abs(rt), np.abs(rb).max()), f"{what}: t {t} vs {rt}"
        assert abs(o - ro) <= 1e-10 * max(ro, 1e-300) + 1e-15 * np.sqrt(yy), f"{what}: opt {o} vs {ro}"
        return 0
    lim = NEAR_TIE_REL * yy
    if objs is not None:
        assert abs(objs[bi] ** 2 - objs[rbi] ** 2) <= lim, f"{what}: winners {bi} / {rbi} are not a near tie"
    assert abs(o ** 2 - ro ** 2) <= lim, f"{what}: opt {o} vs {ro}"
    return 1


def _col(r, b):
    return r["alpha"][:, b], r["beta"][:, b], r["t"][b], r["opt"][b], r["best_index"][b]


def _check_columns(partls, oracle, X, y, P, W, eta, flags, r, tag):
    faithful = bool(flags & FAITHFUL)
    for b in range(W.shape[1]):
        w = W[:, b]
        what = f"{tag} column {b}"
        model, _, rep = partls.fit(partls.Opt, X, y, P, η=float(eta), faithful_intercept=faithful, generic_kernel=bool(flags & GENERIC),
                                   weights=w, on_ill_conditioned="warn")
        ill = bool(rep.get("ill_conditioned", False))
        assert r["status"][b] == (9 if ill else 0), f"{what}: status {r['status'][b]}, single fit ill={ill}"
        if ill:
            continue
        yy = float(np.sum(w * y * y))
        a, bt, t, o, bi = _col(r, b)
        objs = _oracle_objs(oracle, X, y, P, w, eta) if oracle is not None else None
        _close_models(a, bt, t, o, bi, model.α, model.β, model.t, rep.opt, rep.best_index, yy, what, objs)
        if objs is not None:
            best = float(objs.min())
            assert abs(o - best) <= 1e-9 * best + 1e-13 * np.sqrt(yy), f"{what}: opt {o} vs oracle {best}"
            assert abs(objs[bi] ** 2 - best ** 2) <= NEAR_TIE_REL * yy, f"{what}: winner {bi} is not the oracle's"


def _same(a, b, keys=("alpha", "beta", "t", "opt", "best_index", "status", "oob_sse", "oob_rows")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=k in ("alpha", "beta", "t", "opt", "oob_sse")), k


@pytest.fixture(scope="module")
def ctx(partls):
    return partls.Context(0)


@pytest.fixture(scope="module")
def ctx_serial(partls):
    old = os.environ.get("PARTLS_RESAMPLE_SERIAL")
    os.environ["PARTLS_RESAMPLE_SERIAL"] = "1"
    try:
        c = partls.Context(0)
    finally:
        if old is None:
            del os.environ["PARTLS_RESAMPLE_SERIAL"]
        else:
            os.environ["PARTLS_RESAMPLE_SERIAL"] = old
    return c


SHAPES = [(120, 12, 3), (400, 36, 6)]


@pytest.fixture(scope="module")
def small():
    """the two shapes of test 1 with their six weightings: computed once, never written to"""
    out = {}
    for N, M, K in SHAPES:
        X, y, P = _shape(700 + M, N, M, K)
        out[(N, M, K)] = (X, y, P, _columns(800 + M, N))
    return out


# ---- 1. columns are single weighted fits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("flags", [0, FAITHFUL])
def test_columns_are_single_weighted_fits(partls, oracle, ctx, small, shape, eta, flags):
    X, y, P, W = small[shape]
    r = ctx.opt_weightings(X, y, P, W, eta, flags)
    _check_columns(partls, oracle, X, y, P, W, eta, flags, r, f"{shape} eta={eta} flags={flags}")


# ---- 2. the all-ones column is the unweighted fit, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("eta,flags", [(0.0, 0), (0.5, FAITHFUL)])
@pytest.mark.parametrize("pos", [0, 5])
def test_all_ones_column_is_the_unweighted_fit_bitwise(partls, ctx, small, shape, eta, flags, pos):
    """wherever it stands in the batch (pos 5: the last of six, behind five other weightings in the Gram, prepare and sweep launches)"""
    X, y, P, W = small[shape]
    assert np.all(W[:, 0] == 1.0)
    order = np.roll(np.arange(W.shape[1]), pos)
    r = ctx.opt_weightings(X, y, P, np.asfortranarray(W[:, order]), eta, flags)
    model, _, rep = partls.fit(partls.Opt, X, y, P, η=eta, faithful_intercept=bool(flags & FAITHFUL))
    a, b, t, o, bi = _col(r, pos)
    assert np.array_equal(a, model.α) and np.array_equal(b, model.β) and t == model.t and o == rep.opt and bi == rep.best_index
    assert r["status"][pos] == 0 and r["oob_rows"][pos] == 0


# ---- 3. position in the batch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_position_in_the_batch(partls, ctx, ctx_serial, small, shape):
    X, y, P, W = small[shape]
    B = W.shape[1]
    eta = 0.5
    r = ctx.opt_weightings(X, y, P, W, eta)
    _same(r, ctx.opt_weightings(X, y, P, W, eta))                     # the same call twice: bitwise
    assert np.all(r["status"] == 0)
    rev = ctx.opt_weightings(X, y, P, np.asfortranarray(W[:, ::-1]), eta)
    ser = ctx_serial.opt_weightings(X, y, P, W, eta)
    assert np.array_equal(ser["status"], r["status"]) and np.array_equal(ser["oob_rows"], r["oob_rows"])
    for b in range(B):
        yy = float(np.sum(W[:, b] * y * y))
        one = ctx.opt_weightings(X, y, P, W[:, b:b + 1], eta)
        for other, j, name in ((rev, B - 1 - b, "reversed"), (one, 0, "alone"), (ser, b, "serial")):
            assert other["status"][j] == 0 and other["oob_rows"][j] == r["oob_rows"][b]
            _close_models(*_col(other, j), *_col(r, b), yy, f"{shape} column {b} {name}")


# ---- 3b. pieces of the batch ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_pieces(partls):
    """contexts whose batched route takes PARTLS_BATCH_PIECE problems per piece (read at partls_create)"""
    made = {}
    old = os.environ.get("PARTLS_BATCH_PIECE")
    try:
        for piece in (3, 1):
            os.environ["PARTLS_BATCH_PIECE"] = str(piece)
            made[piece] = partls.Context(0)
    finally:
        if old is None:
            del os.environ["PARTLS_BATCH_PIECE"]
        else:
            os.environ["PARTLS_BATCH_PIECE"] = old
    return made


@pytest.fixture(scope="module")
def piece_refs(partls, ctx, ctx_serial):
    """per shape, computed once: the problem, its seven bootstrap weightings and the unpieced and serial results"""
    refs = {}

    def get(D, K):
        if D not in refs:
            X, y, P = _shape(99 + D, 700, D, K)
            W = np.asfortranarray(np.random.default_rng(5).multinomial(700, np.full(700, 1 / 700), size=7).T.astype(np.float64))
            refs[D] = (X, y, P, W, ctx.opt_weightings(X, y, P, W, 0.5), ctx_serial.opt_weightings(X, y, P, W, 0.5))
        return refs[D]
    return get


# the 256-thread kernel and the 512-thread kernel with winner export; B = 7 in pieces of 3, 3, 1 and of 1.  The best and the
# second-best pattern of every column are at least 6.8e-4 and 1.9e-4 y'Wy apart on obj^2 (oracle on the row-replicated data), far
# from the near-tie window: the winners must be equal.
@pytest.mark.parametrize("piece", [3, 1])
@pytest.mark.parametrize("D,K", [(24, 5), (200, 3)])
def test_pieces_of_the_batch(partls, ctx_pieces, piece_refs, D, K, piece):
    X, y, P, W, whole, serial = piece_refs(D, K)
    assert W.shape == (700, 7) and np.all((W > 0).sum(0) >= 430)
    r = ctx_pieces[piece].opt_weightings(X, y, P, W, 0.5)
    _same(r, ctx_pieces[piece].opt_weightings(X, y, P, W, 0.5))
    for other, name in ((whole, "unpieced"), (serial, "serial")):
        assert np.array_equal(r["status"], other["status"]) and np.array_equal(r["oob_rows"], other["oob_rows"])
        assert np.array_equal(r["best_index"], other["best_index"]), name
        for b in range(7):
            yy = float(np.sum(W[:, b] * y * y))
            assert _close_models(*_col(r, b), *_col(other, b), yy, f"D={D} pieces of {piece} column {b} {name}") == 0


# ---- 4. every sweep route -----------------------------------------------------------------------------------------------------------
# the shapes of test_gpu_cv.py::test_every_sweep_route: 512-thread kernel with winner export (T = 13), T = 18 without export, beyond the
# register kernel (serial on the deferred-update kernel), the generic kernel by flag, several chains per problem (K = 12)
@pytest.mark.parametrize("N,D,K,flags,route", [(500, 200, 3, 0, ("REG_512", 13)), (600, 280, 3, 0, ("REG_512", 18)),
                                               (640, 300, 3, 0, ("DEFERRED", 0)), (600, 40, 4, GENERIC, ("DEFERRED", 0)),
                                               (900, 48, 12, 0, ("REG_256", 3))])
def test_every_sweep_route(partls, ctx, N, D, K, flags, route):
    X, y, P = _shape(1234 + D, N, D, K)
    rng = np.random.default_rng(D)
    W = np.asfortranarray(np.stack([np.ones(N), rng.multinomial(N, np.full(N, 1 / N)).astype(np.float64),
                                    (rng.random(N) < 0.8).astype(np.float64)], axis=1))
    r = ctx.opt_weightings(X, y, P, W, 0.0, flags)
    L = partls.lowlevel
    assert ctx.sweep_route() == (getattr(L, "ROUTE_" + route[0]), route[1])
    _check_columns(partls, None, X, y, P, W, 0.0, flags, r, f"route N={N} D={D} K={K} flags={flags}")
    assert np.array_equal(r["oob_rows"], (W == 0).sum(0))


# ---- 5. out of bag ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_out_of_bag(partls, ctx, small, shape):
    X, y, P, W = small[shape]
    r = ctx.opt_weightings(X, y, P, W, 0.0)
    assert np.array_equal(r["oob_rows"], (W == 0).sum(0)) and r["oob_rows"].dtype == np.int64
    assert r["oob_rows"][0] == 0 and np.isnan(r["oob_sse"][0])        # the all-ones column leaves nothing out
    yy = float(y @ y)
    assert sum(bool((W[:, b] == 0).any()) for b in range(W.shape[1])) == 4
    for b in range(1, W.shape[1]):
        a, bt, t, _, _ = _col(r, b)
        out = W[:, b] == 0
        if not out.any():                                                # the real-valued positive column
            assert np.isnan(r["oob_sse"][b]) and r["oob_rows"][b] == 0
            continue
        res = X[out] @ (a * (P @ bt)) + t - y[out]
        want = float(res @ res)
        print(f"{shape} column {b}: oob_sse {r['oob_sse'][b]!r} numpy {want!r}")
        assert abs(r["oob_sse"][b] - want) <= 1e-12 * want + 1e-14 * yy, f"column {b}: {r['oob_sse'][b]} vs {want}"
        one = ctx.opt_weightings(X, y, P, W[:, b:b + 1], 0.0)
        assert one["oob_sse"][0] == r["oob_sse"][b], f"column {b}: alone {one['oob_sse'][0]!r}, in the batch {r['oob_sse'][b]!r}"
    skipped = ctx.opt_weightings(X, y, P, W, 0.0, oob=False)
    assert np.all(np.isnan(skipped["oob_sse"])) and np.array_equal(skipped["oob_rows"], r["oob_rows"])
    _same(skipped, r, keys=("alpha", "beta", "t", "opt", "best_index", "status"))


# ---- 6. errors write nothing ----------------------------------------------------------------------------------------------------------
def _raw_call(partls, handle, X, y, P, W, outs, B=None, ldW=None):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))       # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))        # noqa: E731
    N, M = X.shape
    K = P.shape[1]
    return partls.lowlevel.lib().partls_opt_weightings(
        handle, X.ctypes.data, N, M, N, y.ctypes.data, 0, P.ctypes.data, K, M, W.ctypes.data, N if ldW is None else ldW,
        W.shape[1] if B is None else B, 0.0, 0, dp(outs[0]), M, dp(outs[1]), K, dp(outs[2]), dp(outs[3]), ip(outs[4]), dp(outs[5]),
        ip(outs[6]), outs[7].ctypes.data_as(C.POINTER(C.c_int32)))


def _sentinels(M, K, B):
    return [np.full((M, B), 7.0, order="F"), np.full((K, B), 7.0, order="F"), np.full(B, 7.0), np.full(B, 7.0), np.full(B, 7, dtype=np.int64),
            np.full(B, 7.0), np.full(B, 7, dtype=np.int64), np.full(B, 7, dtype=np.int32)]


@pytest.mark.parametrize("what,status", [("nan", 3), ("inf", 3), ("negative", 1), ("zero_column", 1), ("B0", 1), ("ldW", 1)])
def test_errors_write_nothing(partls, ctx, what, status):
    X, y, P = _shape(3, 50, 6, 2)
    Xf, Pf = np.asfortranarray(X), np.asfortranarray(P)
    W = np.asfortranarray(np.ones((50, 4)))
    kw = {}
    if what == "nan":
        W[17, 2] = np.nan
    elif what == "inf":
        W[49, 3] = np.inf
    elif what == "negative":
        W[0, 1] = -1e-300
    elif what == "zero_column":
        W[:, 3] = 0.0
    elif what == "B0":
        kw["B"] = 0
    else:
        kw["ldW"] = 49
    outs = _sentinels(6, 2, 4)
    assert _raw_call(partls, ctx._h, Xf, y, Pf, W, outs, **kw) == status
    for o in outs:
        assert np.all(o == 7)
    r = ctx.opt_weightings(X, y, P, np.ones((50, 2)), 0.0)           # the context works afterwards
    assert np.all(r["status"] == 0)


def test_null_outputs_and_multi_rank_views_are_refused(partls):
    X, y, P = _shape(3, 50, 6, 2)
    Xf, Pf = np.asfortranarray(X), np.asfortranarray(P)
    W = np.asfortranarray(np.ones((50, 2)))
    mc = partls.MultiContext([0])
    outs = _sentinels(6, 2, 2)
    assert _raw_call(partls, mc.context(0)._h, Xf, y, Pf, W, outs) == partls.lowlevel.ERR_UNSUPPORTED
    for o in outs:
        assert np.all(o == 7)
    with pytest.raises(partls.PartlsError) as ei:
        mc.context(0).opt_weightings(X, y, P, W)
    assert ei.value.status == 7
    mc.close()
    c = partls.Context(0)
    L = partls.lowlevel
    none = C.POINTER(C.c_double)()
    st = L.lib().partls_opt_weightings(c._h, Xf.ctypes.data, 50, 6, 50, y.ctypes.data, 0, Pf.ctypes.data, 2, 6, W.ctypes.data, 50, 2, 0.0, 0,
                                       none, 6, none, 2, none, none, None, none, None, None)
    assert st == L.ERR_BAD_ARG
    c.close()


# ---- 7. an ill-conditioned column only flags itself ---------------------------------------------------------------------------------
def test_ill_conditioned_column_only_flags_itself(partls, ctx):
    # the recipe of test_gpu_cv.py::test_ill_conditioned_fold_only_flags_its_problem: rows 0..499 resolve the near-dependent columns
    rng = np.random.default_rng(42)
    N, D, K = 1500, 24, 4
    Z = rng.standard_normal((N, 6))
    A = rng.standard_normal((6, D))
    noise = np.full((N, 1), 1e-7)
    noise[:500] = 1e-2
    X = Z @ A + noise * rng.standard_normal((N, D))
    grp = np.arange(D) % K
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    y = X @ (rng.random(D) * np.array([1., -2, 3, -1])[grp]) + 0.3 + 0.05 * rng.standard_normal(N)
    W = np.ones((N, 3), order="F")
    W[:500, 1] = 0.0                           # weighting 1 drops the rows that resolve the columns
    W[500:1000, 2] = 0.0
    r = ctx.opt_weightings(X, y, P, W, 0.0)
    assert list(r["status"]) == [0, 9, 0], r["status"]
    _check_columns(partls, None, X, y, P, W, 0.0, 0, r, "ill-conditioned column")
    with pytest.warns(partls.IllConditionedWarning):
        res = partls.resample(partls.Opt, X, y, P, W)
    assert list(res.ill_conditioned) == [False, True, False] and all(m is not None for m in res.models)
    with pytest.raises(partls.PartlsError) as ei:
        partls.resample(partls.Opt, X, y, P, W, on_ill_conditioned="raise")
    assert ei.value.status == 9


# ---- 8. host and device inputs agree bitwise ----------------------------------------------------------------------------------------
def test_host_and_device_inputs_agree_bitwise(partls, ctx, small):
    import torch
    X, y, P, W = small[SHAPES[1]]
    N, M = X.shape
    B = W.shape[1]
    a = ctx.opt_weightings(X, y, P, W, 0.5, FAITHFUL)
    ldX, ldW = N + 5, N + 3                                                     # padded leading dimensions
    dX = torch.zeros((M, ldX), dtype=torch.float64, device="cuda")              # (M, ldX) row-major = X column-major
    dX[:, :N] = torch.from_numpy(np.ascontiguousarray(X.T))
    dW = torch.full((B, ldW), -1.0, dtype=torch.float64, device="cuda")          # the padding must never be read
    dW[:, :N] = torch.from_numpy(np.ascontiguousarray(W.T))
    dy = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    torch.cuda.synchronize()
    b = ctx.opt_weightings(None, None, P, None, 0.5, FAITHFUL, device_ptrs=(dX.data_ptr(), dy.data_ptr(), N, ldX, dW.data_ptr(), ldW, B))
    _same(a, b)


# ---- 9. bootstrap end to end ---------------------------------------------------------------------------------------------------------
def test_bootstrap_end_to_end(partls):
    X, y, P = _shape(11, 300, 12, 3)
    res = partls.bootstrap(partls.Opt, X, y, P, B=16, rng=7)
    assert res.counts.shape == (300, 16) and np.all(res.counts.sum(0) == 300)
    assert np.array_equal(res.counts, np.random.default_rng(7).multinomial(300, np.full(300, 1 / 300), size=16).T)
    assert res.alpha.shape == (16, 12) and res.beta.shape == (16, 3) and np.all(res.status == 0)
    w5 = res.counts[:, 5].astype(float)
    model, _, rep = partls.fit(partls.Opt, X, y, P, weights=w5)
    _close_models(res.alpha[5], res.beta[5], res.t[5], res.opt[5], res.best_index[5], model.α, model.β, model.t, rep.opt, rep.best_index,
                  float(np.sum(w5 * y * y)), "replicate 5")
    assert np.array_equal(res.models[5].α, res.alpha[5]) and res.models[5].t == res.t[5]
    assert np.allclose(res.sign_frequency.sum(1), 1.0) and res.sign_frequency.shape == (3, 3)
    assert abs(sum(res.pattern_frequency.values()) - 1.0) < 1e-12
    iv = res.interval()
    for k in ("alpha", "beta"):
        med = np.median(getattr(res, k), axis=0)
        assert np.all(iv[k][0] <= med) and np.all(med <= iv[k][1])
    assert iv["t"][0] <= np.median(res.t) <= iv["t"][1]
    assert np.array_equal(res.oob_rows, (res.counts == 0).sum(0)) and np.all(res.oob_rows > 0)
    assert res.oob_mse == res.oob_sse.sum() / res.oob_rows.sum()
    out = res.counts[:, 5] == 0
    r5 = partls.predict(res.models[5], X[out]) - y[out]
    assert abs(res.oob_sse[5] - float(r5 @ r5)) <= 1e-12 * float(r5 @ r5) + 1e-14 * float(y @ y)
    # the result holds arrays, not context state: a later fit on the default context works and changes nothing in it
    keep = (res.alpha.copy(), res.beta.copy(), res.oob_sse.copy())
    full, _, frep = partls.fit(partls.Opt, X, y, P)
    assert np.isfinite(frep.opt)
    assert np.array_equal(keep[0], res.alpha) and np.array_equal(keep[1], res.beta) and np.array_equal(keep[2], res.oob_sse)
    # weights scale the counts: unit weights change nothing, bit for bit
    again = partls.bootstrap(partls.Opt, X, y, P, B=16, rng=7, weights=np.ones(300))
    assert np.array_equal(again.alpha, res.alpha) and np.array_equal(again.oob_sse, res.oob_sse)
