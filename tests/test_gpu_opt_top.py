"""GPU tests of the k best patterns selected on the device (partls_opt_top, partls_opt_top_select).

The reference of every comparison is the export itself: opt_top(k) must be, bit for bit, the first k rows of opt_models of the same
pieces, NaN rows removed, ordered by np.lexsort((pattern, opt + 0.0)) — (objective with -0 = +0, reference index).  The selection
kernels alone are driven through opt_top_select with crafted objectives against the same lexsort, with the pattern of every Gray index
computed in Python (wide_reference.gray / reference_index)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from models_reference import _close
from wide_reference import MAX_RANGE, gray, problem as wide_problem, reference_index

pytestmark = pytest.mark.gpu

FAITHFUL = 1
KEYS = ("pattern", "opt", "alpha", "beta", "t", "raw_alpha")
KNOBS = ("PARTLS_TOP_PIECE", "PARTLS_BIT_ORDER", "PARTLS_EAGER_GENERIC", "PARTLS_REG_MAXT", "PARTLS_CHAIN_LEN", "PARTLS_GRID")


def _ctx(partls, monkeypatch, env=None):
    """a Context with the given knobs (read once, at partls_create)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    ctx = partls.Context(0)
    for k in env or {}:
        monkeypatch.delenv(k)
    return ctx


def _pieces(g0, g1, cap):
    """the piece boundaries of partls_opt_top for the range [g0, g1) under a cap of `cap` patterns (include/partls.h)"""
    total = g1 - g0
    if total <= 0:
        return []
    npieces = -(-total // cap)
    piece = -(-total // npieces)
    return [(p0, min(g1, p0 + piece)) for p0 in range(g0, g1, piece)]


def _export(ctx, bounds):
    """opt_models(raw=True) over the given pieces, concatenated"""
    parts = [ctx.opt_models(a, b, raw=True) for a, b in bounds]
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS}


def _first(full, k):
    """rows of an export in the order of partls_opt_top, NaN rows removed, the first k"""
    ok = np.flatnonzero(~np.isnan(full["opt"]))
    return ok[np.lexsort((full["pattern"][ok], full["opt"][ok] + 0.0))][:k]


def _same(r, full, k):
    rows = _first(full, k)
    assert r["count"] == len(rows) == len(r["pattern"])
    for key in KEYS:
        assert np.array_equal(r[key], full[key][rows]), key
    return rows


def _perm_problem():
    """the problem of test_gpu_models.py whose measured bit order is a true permutation"""
    rng = np.random.default_rng(11)
    N, M, K = 400, 45, 9
    X = np.asfortranarray(rng.standard_normal((N, M)))
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), rng.integers(0, K, size=M)] = 1
    w = rng.standard_normal(M) * (rng.random(M) < 0.6)
    return X, X @ w + 0.5 + 0.3 * rng.standard_normal(N), P, 0.0


def _named(name):
    if name == "perm":
        return _perm_problem()
    g = load_golden(name)
    return g["X"], g["y"], g["P"], float(g.get("eta", 0.0))


# ---- 1. a subset of the export, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["identity", "calibrate"])
@pytest.mark.parametrize("name", ["toy", "synth_a", "synth_b", "synth_c", "synth_eta", "corr", "perm"])
def test_first_rows_of_the_export(partls, monkeypatch, name, order):
    X, y, P, eta = _named(name)
    ctx = _ctx(partls, monkeypatch, {"PARTLS_BIT_ORDER": order})
    ctx.opt_prepare(X, y, P, eta, FAITHFUL)
    npat = ctx.num_patterns()
    full = ctx.opt_models(raw=True)
    assert full["n_unconverged"] == 0
    if name == "perm" and order == "calibrate":
        assert list(ctx.bit_order()[0]) != list(range(P.shape[1] + 1))
    for k in sorted({1, 2, 7, npat - 1, npat, min(npat + 5, 4096)}):
        r = ctx.opt_top(k, raw=True)
        assert r["count"] == min(k, npat) and r["n_unconverged"] == 0 and r["n_vetoes"] == full["n_vetoes"]
        _same(r, full, k)
        assert "raw_alpha" not in ctx.opt_top(k)
    again = ctx.opt_top(7, raw=True)
    for key in KEYS:
        assert np.array_equal(again[key], ctx.opt_top(7, raw=True)[key])         # the same arguments, the same bits
    ctx.close()


def test_against_the_oracle(partls, oracle, monkeypatch):
    X, y, P, eta = _named("synth_a")
    ctx = _ctx(partls, monkeypatch)
    ctx.opt_prepare(X, y, P, eta, FAITHFUL)
    k = 7
    r = ctx.opt_top(k)
    ref = oracle.fit_opt(X, y, P, eta, all_models=True)
    pat = r["pattern"]
    assert r["count"] == k and len(set(pat.tolist())) == k
    _close(r["opt"], np.sort(ref["all_opt"])[:k])                               # the k smallest objectives ...
    _close(r["opt"], ref["all_opt"][pat])                                       # ... of the patterns named, with their models
    _close(r["alpha"], ref["all_alpha"][pat]); _close(r["beta"], ref["all_beta"][pat]); _close(r["t"], ref["all_t"][pat])
    ctx.close()


# ---- 2. ranges and pieces ---------------------------------------------------------------------------------------------------------------
def test_ranges_pieces_and_errors(partls, monkeypatch):
    X, y, P, eta = _named("synth_b")
    # 64 patterns.  A cap of 37 gives two equal pieces of 32 (equal pieces: ceil(total / npieces)); a cap of 7 ten pieces, the last one short
    for cap, npieces, last in ((7, 10, 1), (37, 2, 32)):
        ctx = _ctx(partls, monkeypatch, {"PARTLS_TOP_PIECE": cap})
        ctx.opt_prepare(X, y, P, eta, FAITHFUL)
        npat = ctx.num_patterns()
        bounds = _pieces(0, npat, cap)
        assert npat == 64 and len(bounds) == npieces and bounds[-1][1] - bounds[-1][0] == last
        for g0, g1 in ((0, npat), (3, 37), (0, 1), (npat - 5, npat), (5, 62)):
            full = _export(ctx, _pieces(g0, g1, cap))
            for k in (1, 10, 50, 4096):
                r = ctx.opt_top(k, g0, g1, raw=True)
                assert r["count"] == min(k, g1 - g0)
                _same(r, full, k)
        if cap == 7:
            ctx.close()
    r = ctx.opt_top(10, 0, -1, raw=True)                                        # g_end = -1: to the end
    _same(r, _export(ctx, bounds), 10)
    e = ctx.opt_top(3, 7, 7, raw=True)
    assert e["count"] == 0 and len(e["pattern"]) == 0 and e["alpha"].shape == (0, P.shape[0]) and e["n_unconverged"] == 0
    L = partls.lowlevel
    for args in ((0,), (4097,), (-3,), (3, 9, 5), (3, 0, npat + 1), (3, -1, 5)):
        with pytest.raises(partls.PartlsError) as ei:
            ctx.opt_top(*args)
        assert ei.value.status == L.ERR_BAD_ARG, args
    lib = L.lib()
    pat = np.zeros(4, dtype=np.int64); opt = np.zeros(4); cnt = C.c_int64(-1)
    ip, dp = pat.ctypes.data_as(C.POINTER(C.c_int64)), opt.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.partls_opt_top(ctx._h, 0, 4, 4, None, dp, None, 0, None, 0, None, 0, None, C.byref(cnt), None, None) == L.ERR_BAD_ARG
    assert lib.partls_opt_top(ctx._h, 0, 4, 4, ip, dp, None, 0, None, 0, None, 0, None, None, None, None) == L.ERR_BAD_ARG
    assert lib.partls_opt_top(ctx._h, 0, 4, 4, ip, dp, None, 0, None, 0, None, 0, None, C.byref(cnt), None, None) == L.OK and cnt.value == 4
    assert np.array_equal(opt, ctx.opt_top(4, 0, 4)["opt"])                     # models are optional
    ctx.close()
    fresh = partls.Context(0)
    assert lib.partls_opt_top(fresh._h, 0, 4, 4, ip, dp, None, 0, None, 0, None, 0, None, C.byref(cnt), None, None) == L.ERR_STATE
    obj = np.zeros(4)
    assert lib.partls_opt_top_select(fresh._h, dp, 4, 0, 2, ip, ip, obj.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cnt)) == L.ERR_STATE
    fresh.opt_prepare(X, y, P, eta, 0)                                          # free intercept: no reference models
    with pytest.raises(partls.PartlsError) as ei:
        fresh.opt_top(3)
    assert ei.value.status == L.ERR_STATE
    fresh.close()


# ---- 3. the selection kernels on crafted keys -------------------------------------------------------------------------------------------
def _select_context(partls, monkeypatch, order):
    """K = 12 groups, faithful: 8192 patterns; a tiny N.  (ctx, reference patterns of the Gray indices 0 .. 8191)"""
    X, y, P = wide_problem(1200, 20, 12)
    ctx = _ctx(partls, monkeypatch, {"PARTLS_BIT_ORDER": order})
    ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
    assert ctx.num_patterns() == 8192
    gbit = [int(v) for v in ctx.bit_order()[0]]
    assert sorted(gbit) == list(range(13))
    if order == "identity":
        assert gbit == list(range(13))
    return ctx, np.array([reference_index(gray(g), gbit) for g in range(8192)], dtype=np.int64)


def _check_select(ctx, pats, obj, g0, k, tag):
    obj = np.asarray(obj, dtype=np.float64)
    pat = pats[g0:g0 + len(obj)]
    ok = np.flatnonzero(~np.isnan(obj))
    want = ok[np.lexsort((pat[ok], obj[ok] + 0.0))][:k]
    idx, p, val = ctx.opt_top_select(obj, g0, k)
    assert len(idx) == len(want) == min(k, len(ok)), tag
    assert np.array_equal(idx, want), tag
    assert np.array_equal(p, pat[want]), tag
    assert np.array_equal(val.view(np.int64), obj[want].view(np.int64)), tag       # the entry's own bits (-0.0 stays -0.0)


@pytest.mark.parametrize("order", ["identity", "calibrate"])
def test_selection_on_crafted_keys(partls, monkeypatch, order):
    ctx, pats = _select_context(partls, monkeypatch, order)
    rng = np.random.default_rng(5)
    n = 8192
    tiny = np.nextafter(0.0, 1.0)
    # all keys equal: the tie-break alone decides
    for v in (3.25, 0.0, -0.0, np.inf):
        _check_select(ctx, pats, np.full(n, v), 0, 100, "all equal %r" % v)
    # blocks of exact ties straddling the k-th place
    base = rng.integers(0, 40, size=n).astype(np.float64)
    counts = np.cumsum(np.bincount(base.astype(int)))
    for k in (int(counts[0]) - 1, int(counts[0]), int(counts[0]) + 1, int(counts[3]) - 7, 100, 4096):
        _check_select(ctx, pats, base, 0, k, "tie blocks k=%d" % k)
    # NaNs scattered, and a NaN majority with count < k
    some = rng.standard_normal(n)
    some[rng.random(n) < 0.1] = np.nan
    some[[0, 1, n - 1]] = np.nan
    _check_select(ctx, pats, some, 0, 500, "scattered NaN")
    most = np.full(n, np.nan)
    keep = rng.choice(n, 57, replace=False)
    most[keep] = rng.integers(0, 5, size=57) * 0.5
    most[keep[:3]] = -np.nan
    _check_select(ctx, pats, most, 0, 100, "NaN majority")
    _check_select(ctx, pats, np.full(300, np.nan), 5, 10, "all NaN")
    neg_nan = np.full(64, -np.nan)                                              # sign bit set: still never selected
    neg_nan[7] = 1.0
    _check_select(ctx, pats, neg_nan, 0, 5, "negative NaN")
    # +-0.0, denormals, +inf, negative values, huge values
    special = rng.choice(np.array([0.0, -0.0, tiny, -tiny, 5e-324 * 3, np.inf, -np.inf, 1.0, -1.0, 1e308, -1e308, 2.5e-310, np.nan]), size=n)
    for k in (1, 64, 1000, 4096):
        _check_select(ctx, pats, special, 0, k, "special values k=%d" % k)
    # strictly descending and strictly ascending
    asc = np.sort(rng.standard_normal(n) * 1e3)
    asc = asc[np.concatenate([[True], np.diff(asc) > 0])]
    for k in (1, 100, 4096):
        _check_select(ctx, pats, asc, 0, k, "ascending")
        _check_select(ctx, pats, asc[::-1].copy(), 0, k, "descending")
    # objectives as a sweep leaves them: positive, close together
    near = 10.0 + rng.random(n) * 1e-9
    _check_select(ctx, pats, near, 0, 4096, "close positive values")
    # sizes around the wave, the workgroup and the sort width; k at its ends; a range that does not start at 0
    for cnt in (1, 63, 64, 65, 255, 257, 4095, 4097, 8192):
        vals = rng.integers(0, max(2, cnt // 3), size=cnt).astype(np.float64) - 3.0
        vals[rng.random(cnt) < 0.05] = np.nan
        for g0 in (0, 5):
            if g0 + cnt > n:
                continue
            for k in (1, cnt, 4096):
                _check_select(ctx, pats, vals, g0, min(k, 4096), "cnt=%d g0=%d k=%d" % (cnt, g0, k))
    vals = rng.integers(0, 9, size=n - 5).astype(np.float64)
    _check_select(ctx, pats, vals, 5, 4096, "to the end of the space")
    L = partls.lowlevel
    for args in ((np.zeros(4), 0, 0), (np.zeros(4), 0, 4097), (np.zeros(4), n - 3, 2), (np.zeros(4), -1, 2)):
        with pytest.raises(partls.PartlsError) as ei:
            ctx.opt_top_select(*args)
        assert ei.value.status == L.ERR_BAD_ARG
    assert [len(v) for v in ctx.opt_top_select(np.zeros(0), 3, 2)] == [0, 0, 0]
    ctx.close()


# ---- 4. more than one workgroup per pass, k at its maximum ------------------------------------------------------------------------------
def test_many_workgroups_and_the_largest_k(partls, monkeypatch):
    X, y, P = wide_problem(1400, 14, 14)                                        # M = K = 14, N = 82
    X, y = np.asfortranarray(X[:64]), y[:64]
    for cap in (None, 5000):
        ctx = _ctx(partls, monkeypatch, {"PARTLS_TOP_PIECE": cap} if cap else None)
        ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
        npat = ctx.num_patterns()
        assert npat == 32768
        bounds = _pieces(0, npat, cap) if cap else [(0, npat)]
        assert len(bounds) == (7 if cap else 1)
        full = _export(ctx, bounds)
        r = ctx.opt_top(4096, raw=True)
        assert r["count"] == 4096 and r["n_unconverged"] == int(np.isnan(full["opt"]).sum()) == 0
        _same(r, full, 4096)
        _same(ctx.opt_top(100, 1000, 30001, raw=True), _export(ctx, _pieces(1000, 30001, cap) if cap else [(1000, 30001)]), 100)
        ctx.close()


# ---- 5. each sweep kernel feeds it ------------------------------------------------------------------------------------------------------
def _route_cases():
    from test_gpu_tile_counts import BY_ID, CASES
    small = next(c for c in CASES if c["T"] == 2)                               # the 256-thread register kernel
    large = next(c for c in CASES if c["T"] == 11)                              # the 512-thread register kernel
    assert BY_ID[small["id"]]["route"][0] == 1 and BY_ID[large["id"]]["route"][0] == 2
    return small, large


@pytest.mark.parametrize("which", ["reg256", "reg512", "deferred", "eager"])
def test_every_sweep_kernel_feeds_it(partls, monkeypatch, which):
    L = partls.lowlevel
    if which in ("reg256", "reg512"):
        from test_gpu_tile_counts import _problem
        case = _route_cases()[which == "reg512"]
        X, y, P, eta = _problem(case, K=min(case["K"], 5))
        env, route = dict(case["env"]), case["route"]
    else:
        from test_gpu_lazy import _problem
        X, y, P = _problem(1330, 2 * 330 + 50, 330, 4)
        eta = 0.0
        env = {"PARTLS_EAGER_GENERIC": "1"} if which == "eager" else {}
        route = (L.ROUTE_EAGER if which == "eager" else L.ROUTE_DEFERRED, 0)
    ctx = _ctx(partls, monkeypatch, env)
    ctx.opt_prepare(X, y, P, eta, FAITHFUL)
    assert ctx.sweep_route() == route
    npat = ctx.num_patterns()
    full = ctx.opt_models(raw=True)
    _same(ctx.opt_top(5, raw=True), full, 5)
    _same(ctx.opt_top(3, 2, npat - 3, raw=True), ctx.opt_models(2, npat - 3, raw=True), 3)
    ctx.close()


# ---- 6. wide spaces ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["identity", "calibrate"])
def test_forty_bit_space(partls, monkeypatch, order):
    X, y, P = wide_problem(4401, 44, 39)                                        # test_gpu_wide_patterns.py: "small"
    ctx = _ctx(partls, monkeypatch, {"PARTLS_BIT_ORDER": order})
    ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
    top = 1 << 40
    assert ctx.num_patterns() == top
    gbit = [int(v) for v in ctx.bit_order()[0]]
    if order == "calibrate":
        assert gbit != list(range(40))
    for g0, g1 in (((1 << 32) - 150, (1 << 32) + 150), (top - 300, top)):
        assert 0 <= g0 < g1 <= top and g1 - g0 <= MAX_RANGE                     # never more than a short range of this space
        full = ctx.opt_models(g0, g1, raw=True)
        assert [int(v) for v in full["pattern"]] == [reference_index(gray(g), gbit) for g in range(g0, g1)]
        r = ctx.opt_top(16, g0, g1, raw=True)
        rows = _same(r, full, 16)
        assert [int(v) for v in r["pattern"]] == [int(full["pattern"][i]) for i in rows]
        assert max(int(v) for v in full["pattern"]) >= 1 << 32
    ctx.close()


# ---- 7. the state of the last sweep -----------------------------------------------------------------------------------------------------
def test_the_sweep_state_is_left_alone(partls, monkeypatch):
    X, y, P, eta = _named("synth_c")
    out = []
    for top in (False, True):
        ctx = _ctx(partls, monkeypatch)
        ctx.opt_prepare(X, y, P, eta, FAITHFUL)
        bo, bp, _, _ = ctx.opt_sweep()
        piv, vet = ctx.pivots(), ctx.vetoes()
        if top:
            assert ctx.opt_top(50, raw=True)["count"] == 50
        out.append((bo, bp, piv, vet, ctx.pivots(), ctx.vetoes(), ctx.opt_candidates(), ctx.opt_finish(bp), ctx.near_ties_evaluated()))
        ctx.close()
    a, b = out
    assert a[:6] == b[:6] and a[8] == b[8]
    for u, v in zip(a[6] + tuple(a[7]), b[6] + tuple(b[7])):
        assert np.array_equal(u, v)


# ---- 8. fit(Opt, ..., top=k) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "synth_a"])
def test_fit_with_top(partls, name):
    X, y, P, eta = _named(name)
    k = 6
    model, _, rep = partls.fit(partls.Opt, X, y, P, η=eta, top=k, returnAllSolutions=True)
    ctx = partls.default_context(0)
    near = ctx.near_ties_evaluated()
    top = rep.top
    assert isinstance(top, partls.TopPatterns) and len(top) == k == len(top.models) and top.n_vetoes == 0
    assert np.all(np.diff(top.opt) >= 0)
    for i, b in enumerate(top.pattern):
        o, m = rep.solutions[int(b)]
        _close(top.models[i].α, m.α); _close(top.models[i].β, m.β); _close(top.models[i].t, m.t)
        assert np.array_equal(top.models[i].α, top.alpha[i]) and np.array_equal(top.models[i].β, top.beta[i]) and top.models[i].t == top.t[i]
        np.testing.assert_allclose(top.opt[i], o, rtol=0, atol=2e-7 * max(1.0, float(np.linalg.norm(y))))   # Gram form against the data (test_gpu_opt.py)
    _, _, plain = partls.fit(partls.Opt, X, y, P, η=eta, faithful_intercept=True, top=k)
    assert plain.best_index in [int(b) for b in top.pattern[:1 + near]]
    assert np.array_equal(plain.top.pattern, top.pattern) and np.array_equal(plain.top.opt, top.opt)
    assert np.array_equal(top.gap, top.opt[1:] - top.opt[0])
    b = top.beta
    assert np.array_equal(top.sign_agreement, np.stack([(b < 0).mean(0), (b == 0).mean(0), (b > 0).mean(0)], axis=1))
    K = P.shape[1]
    gp = top.group_patterns()
    seen, rows = set(), []
    for i, p in enumerate(top.pattern):
        if int(p) & ((1 << K) - 1) not in seen:
            seen.add(int(p) & ((1 << K) - 1))
            rows.append(i)
    assert gp.pattern.tolist() == [int(top.pattern[i]) & ((1 << K) - 1) for i in rows]
    assert np.array_equal(gp.opt, top.opt[rows]) and np.array_equal(gp.beta, top.beta[rows]) and len(gp.models) == len(rows)


def test_fit_with_top_weights_and_float32(partls):
    X, y, P, eta = _named("synth_a")
    N = len(y)
    w = 0.5 + np.random.default_rng(3).random(N)
    wm, _, wrep = partls.fit(partls.Opt, X, y, P, η=eta, weights=w, faithful_intercept=True)
    tm, _, trep = partls.fit(partls.Opt, X, y, P, η=eta, weights=w, top=4)
    assert trep.best_index == wrep.best_index and np.array_equal(tm.α, wm.α) and np.array_equal(tm.β, wm.β) and tm.t == wm.t
    i = [int(b) for b in trep.top.pattern].index(wrep.best_index)
    _close(trep.top.models[i].α, wm.α); _close(trep.top.models[i].β, wm.β); _close(trep.top.models[i].t, wm.t)
    _, _, unweighted = partls.fit(partls.Opt, X, y, P, η=eta, top=4)
    assert not np.array_equal(unweighted.top.opt, trep.top.opt)                 # the weights reach the ranking
    X32 = X.astype(np.float32)
    m32, _, r32 = partls.fit(partls.Opt, X32, y, P, η=eta, top=4)
    m64, _, r64 = partls.fit(partls.Opt, X32.astype(np.float64), y, P, η=eta, top=4)
    assert r32.best_index == r64.best_index and np.array_equal(m32.α, m64.α)
    for key in ("pattern", "opt", "alpha", "beta", "t"):
        assert np.array_equal(getattr(r32.top, key), getattr(r64.top, key)), key  # float32 X: the results of X.astype(float64), bit for bit


# ---- 9. more entries than one trip of the capped grids --------------------------------------------------------------------------------
def _wide_select_context(partls, monkeypatch, order):
    """as _select_context with K = 18 groups, faithful: 2^19 patterns, twice the 1024 x 256 entries that the histogram and the
    compaction grids cover in one trip.  The reference patterns of all Gray indices by numpy shifts on int64 (19 bits), checked against
    wide_reference on a sample"""
    X, y, P = wide_problem(1800, 26, 18)
    ctx = _ctx(partls, monkeypatch, {"PARTLS_BIT_ORDER": order})
    ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
    n = 1 << 19
    assert ctx.num_patterns() == n
    gbit = [int(v) for v in ctx.bit_order()[0]]
    assert sorted(gbit) == list(range(19))
    if order == "identity":
        assert gbit == list(range(19))
    g = np.arange(n, dtype=np.int64)
    q = g ^ (g >> 1)
    pats = np.zeros(n, dtype=np.int64)
    for k in range(19):
        pats |= ((q >> gbit[k]) & 1) << k
    for i in [0, 1, 2, 255, 256, 262143, 262144, 300000, n - 1] + [int(v) for v in np.random.default_rng(1).integers(0, n, 50)]:
        assert pats[i] == reference_index(gray(i), gbit)
    return ctx, pats


@pytest.mark.parametrize("cnt", [300001, 524288])
@pytest.mark.parametrize("order", ["identity", "calibrate"])
def test_selection_beyond_one_trip_of_the_grid(partls, monkeypatch, order, cnt):
    """cnt = 300 001: workgroups 0 .. 147 of topk_hist_kernel and topk_compact_kernel make a second trip, workgroup 147 a ragged one;
    cnt = 524 288 = 2 x 1024 x 256: every workgroup makes two full trips.  Keys: blocks of about 750 exact ties, so that k = 1 and 100
    end inside the first block and k = 4096 inside the sixth, decided by the reference index in the passes over lo; +-0.0 among a few
    negative values and many ties; continuous values; 5 % NaN in each"""
    ctx, pats = _wide_select_context(partls, monkeypatch, order)
    rng = np.random.default_rng(cnt)
    nan = rng.random(cnt) < 0.05
    ties = rng.integers(0, cnt // 750, size=cnt).astype(np.float64)
    zeros = rng.integers(0, 3, size=cnt).astype(np.float64)
    zeros[(zeros == 0.0) & (rng.random(cnt) < 0.5)] = -0.0
    zeros[rng.choice(cnt, 50, replace=False)] = -1.0
    assert np.signbit(zeros[zeros == 0.0]).any() and not np.signbit(zeros[zeros == 0.0]).all()
    smooth = rng.standard_normal(cnt)
    for name, keys in (("tie blocks", ties), ("signed zeros", zeros), ("continuous", smooth)):
        keys[nan] = np.nan
        keys[0], keys[cnt - 1] = np.nan, -5.0                                   # the last entry of the last trip is the best of all
        for g0 in (0, 5):
            if g0 + cnt > len(pats):
                continue
            for k in (1, 100, 4096):
                _check_select(ctx, pats, keys, g0, k, "%s cnt=%d g0=%d k=%d" % (name, cnt, g0, k))
    ctx.close()
