"""GPU tests of the bulk model export (partls_opt_models): every pattern's model straight from the sweep kernels, as
fit(Opt, ...; returnAllSolutions=true) returns them (Opt.jl:87-101), instead of one solve per pattern.

References: the golden models of the reference (toy), the oracle's per-pattern NNLS (dense Lawson-Hanson, QR-compressed data for the
large tableaus), a plain sweep's all_opt (bitwise) and the per-pattern path of the library (opt_finish / opt_pattern)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from models_reference import _cleanup, _close, _scatter

pytestmark = pytest.mark.gpu

FAITHFUL = 1


def _ctx(partls, X, y, P, eta=0.0, flags=FAITHFUL, monkeypatch=None, env=None):
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    ctx = partls.Context(0)
    if env:
        for k in env:
            monkeypatch.delenv(k)
    ctx.opt_prepare(X, y, P, eta, flags)
    return ctx


def test_toy_every_pattern_matches_the_golden_models(partls, monkeypatch):
    g = load_golden("toy")
    for env, flags in ((None, FAITHFUL), ({"PARTLS_EAGER_GENERIC": "1"}, FAITHFUL | 2), (None, FAITHFUL | 2)):
        ctx = _ctx(partls, g["X"], g["y"], g["P"], flags=flags, monkeypatch=monkeypatch, env=env)
        r = ctx.opt_models()
        assert r["n_unconverged"] == 0 and len(r["pattern"]) == 8
        s = _scatter(r, 8)
        _close(s["alpha"], g["opt_all_alpha"]); _close(s["beta"], g["opt_all_beta"]); _close(s["t"], g["opt_all_t"])
        _close(s["opt"], g["opt_all_opt"])
        ctx.close()


@pytest.mark.parametrize("name", ["synth_a", "synth_b", "synth_c", "synth_eta", "corr"])
def test_every_pattern_against_the_oracle(partls, oracle, name):
    g = load_golden(name)
    eta = float(g.get("eta", 0.0))
    X, y, P = g["X"], g["y"], g["P"]
    ctx = _ctx(partls, X, y, P, eta)
    npat = ctx.num_patterns()
    bo, bp, allopt, _ = ctx.opt_sweep(0, -1, want_all=True)
    r = ctx.opt_models(raw=True)
    assert r["n_unconverged"] == 0 and r["n_vetoes"] == 0
    # one piece on the plain sweep's chain plan: the objectives are all_opt's, bit for bit
    assert np.array_equal(r["opt"], allopt[r["pattern"]])
    s = _scatter(r, npat)
    ref = oracle.fit_opt(X, y, P, eta, all_models=True)
    _close(s["alpha"], ref["all_alpha"]); _close(s["beta"], ref["all_beta"]); _close(s["t"], ref["all_t"])
    _close(s["opt"], ref["all_opt"])
    Xo, Po = oracle.homogeneous(X, P)
    Xr, yr = oracle.regularize(Xo, y, Po, eta)
    _, ra = oracle.opt_patterns(Xr, yr, Po, np.arange(npat), want_alpha=True)
    _close(s["raw_alpha"], ra)
    ctx.close()


def test_ranges_errors_and_calibrated_order(partls, monkeypatch):
    g = load_golden("synth_b")
    X, y, P = g["X"], g["y"], g["P"]
    ctx = _ctx(partls, X, y, P)
    npat = ctx.num_patterns()
    full = ctx.opt_models(raw=True)
    cuts = [0, 3, 37, npat - 5, npat]
    parts = [ctx.opt_models(a, b, raw=True) for a, b in zip(cuts[:-1], cuts[1:])]
    for (a, b), p in zip(zip(cuts[:-1], cuts[1:]), parts):
        assert len(p["pattern"]) == b - a
        assert np.array_equal(p["pattern"], full["pattern"][a:b])          # row i = Gray index g_begin + i
    joined = {k: np.concatenate([p[k] for p in parts]) for k in ("pattern", "opt", "alpha", "beta", "t", "raw_alpha")}
    s, f = _scatter(joined, npat), _scatter(full, npat)
    for k in ("opt", "alpha", "beta", "t", "raw_alpha"):
        _close(s[k], f[k], 1e-10)
    e = ctx.opt_models(7, 7)
    assert len(e["pattern"]) == 0 and e["n_unconverged"] == 0
    lib = partls.lowlevel.lib()
    for a, b in ((9, 5), (0, npat + 1), (-1, 5)):
        with pytest.raises(partls.PartlsError) as ei:
            ctx.opt_models(a, b)
        assert ei.value.status == partls.lowlevel.ERR_BAD_ARG
    st = lib.partls_opt_models(ctx._h, 0, 4, None, None, None, 0, None, 0, None, 0, None, None, None)
    assert st == partls.lowlevel.ERR_BAD_ARG
    ctx.close()
    pat = np.zeros(4, dtype=np.int64)
    fresh = partls.Context(0)
    st = lib.partls_opt_models(fresh._h, 0, 4, pat.ctypes.data_as(C.POINTER(C.c_int64)), None, None, 0, None, 0, None, 0, None, None, None)
    assert st == partls.lowlevel.ERR_STATE
    fresh.opt_prepare(X, y, P, 0.0, 0)                                       # free intercept: 2^K patterns, no reference models
    with pytest.raises(partls.PartlsError) as ei:
        fresh.opt_models()
    assert ei.value.status == partls.lowlevel.ERR_STATE
    fresh.close()

    # a calibrated (non-identity) visiting order: the same models under the reference's pattern index
    X, y, P = _perm_problem()
    K = P.shape[1]
    res = {}
    for mode in ("identity", "calibrate"):
        c = _ctx(partls, X, y, P, monkeypatch=monkeypatch, env={"PARTLS_BIT_ORDER": mode})
        r = c.opt_models()
        res[mode] = (c.bit_order()[0], _scatter(r, c.num_patterns()))
        c.close()
    assert list(res["calibrate"][0]) != list(range(K + 1))
    for k in ("opt", "alpha", "beta", "t"):
        _close(res["calibrate"][1][k], res["identity"][1][k], 1e-9)


def _pieces(g0, g1, cap):
    """the piece boundaries of the export walk for [g0, g1) under a cap of `cap` patterns (test_gpu_opt_top.py: _pieces)"""
    total = g1 - g0
    npieces = -(-total // cap)
    piece = -(-total // npieces)
    return [(p0, min(g1, p0 + piece)) for p0 in range(g0, g1, piece)]


def _perm_problem():
    """the calibrated-order problem of test_ranges_errors_and_calibrated_order: N = 400, M = 45, K = 9, 1024 patterns"""
    rng = np.random.default_rng(11)
    N, M, K = 400, 45, 9
    X = np.asfortranarray(rng.standard_normal((N, M)))
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), rng.integers(0, K, size=M)] = 1
    w = rng.standard_normal(M) * (rng.random(M) < 0.6)
    return X, X @ w + 0.5 + 0.3 * rng.standard_normal(N), P


_EXPORT_KEYS = ("pattern", "opt", "alpha", "beta", "t", "raw_alpha")


@pytest.mark.parametrize("name,env,caps,ranges", [
    ("synth_b", {}, (7, 37), ((0, 64), (3, 37), (5, 62), (63, 64))),
    ("perm", {"PARTLS_BIT_ORDER": "calibrate"}, (100,), ((0, 1024), (17, 900))),
])
def test_one_call_in_pieces(partls, monkeypatch, name, env, caps, ranges):
    """PARTLS_TOP_PIECE caps the pieces of partls_opt_models: one call over several pieces is, bit for bit, the calls over its pieces
    one by one, and its counters are their sums; against a context without the knob (other pieces, other chains) round-off apart"""
    if name == "perm":
        X, y, P = _perm_problem()
    else:
        g = load_golden(name)
        X, y, P = g["X"], g["y"], g["P"]
    plain = _ctx(partls, X, y, P, monkeypatch=monkeypatch, env=env or None)
    npat = plain.num_patterns()
    if name == "perm":
        assert npat == 1024 and list(plain.bit_order()[0]) != list(range(P.shape[1] + 1))
    whole = _scatter(plain.opt_models(raw=True), npat)
    plain.close()
    for cap in caps:
        ctx = _ctx(partls, X, y, P, monkeypatch=monkeypatch, env=dict(env, PARTLS_TOP_PIECE=str(cap)))
        for g0, g1 in ranges:
            bounds = _pieces(g0, g1, cap)
            assert all(b - a <= cap for a, b in bounds) and bounds[0][0] == g0 and bounds[-1][1] == g1
            assert len(bounds) == -(-(g1 - g0) // cap)                     # several pieces wherever the range is longer than the cap
            r = ctx.opt_models(g0, g1, raw=True)
            parts = [ctx.opt_models(a, b, raw=True) for a, b in bounds]
            for key in _EXPORT_KEYS:
                assert np.array_equal(r[key], np.concatenate([p[key] for p in parts])), (cap, g0, g1, key)
            assert r["n_unconverged"] == sum(p["n_unconverged"] for p in parts)
            assert r["n_vetoes"] == sum(p["n_vetoes"] for p in parts)
            for key in ("opt", "alpha", "beta", "t", "raw_alpha"):   # `whole` is indexed by the reference pattern
                _close(r[key], whole[key][r["pattern"]], 1e-10)
        ctx.close()


def _big_problem(seed, N, D, K):
    """overlapping groups (f = +-2 and 0), a feature in no group, an empty group"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), rng.integers(0, K - 1, size=D)] = 1                      # group K-1 stays empty
    for m in range(0, 12, 3):
        P[m, (np.argmax(P[m]) + 1) % (K - 1)] = 1                           # features in two groups
    P[D - 1] = 0                                                             # a feature in no group
    w = rng.standard_normal(D) * (rng.random(D) < 0.6)
    y = X @ w + 0.4 + 0.3 * rng.standard_normal(N)
    return np.asfortranarray(X), y, np.asfortranarray(P)


@pytest.mark.parametrize("D,eta", [(271, 0.0), (287, 0.5), (296, 0.0), (340, 0.3)])
def test_large_tableau_kernels_against_the_oracle(partls, oracle, D, eta):
    """T = 17 / 18 of the 512-thread register kernel (n = D + 1 <= 288) and the deferred-update kernel beyond (QR-compressed oracle)"""
    K = 6
    X, y, P = _big_problem(D, 1500, D, K)
    ctx = _ctx(partls, X, y, P, eta)
    npat = ctx.num_patterns()
    r = ctx.opt_models(raw=True)
    assert r["n_unconverged"] == 0 and r["n_vetoes"] == 0
    s = _scatter(r, npat)
    pats = np.random.default_rng(D).choice(npat, 8, replace=False)
    Xo, Po = oracle.homogeneous(X, P)
    Xr, yr = oracle.regularize(Xo, y, Po, eta)
    R, z = oracle.compress(Xr, yr)
    objs, ra = oracle.opt_patterns(R, z, Po, pats, want_alpha=True)
    _close(s["raw_alpha"][pats], ra)
    _close(s["opt"][pats], objs)
    for i, b in enumerate(pats):
        a, bt, t = _cleanup(ra[i], P, int(b))
        _close(s["alpha"][b], a); _close(s["beta"][b], bt); _close(s["t"][b], t)
    ctx.close()


def test_export_leaves_the_sweep_state_alone(partls):
    g = load_golden("synth_c")
    X, y, P = g["X"], g["y"], g["P"]
    out = []
    for export in (False, True):
        ctx = _ctx(partls, X, y, P)
        bo, bp, _, _ = ctx.opt_sweep()
        piv, vet = ctx.pivots(), ctx.vetoes()
        if export:
            ctx.opt_models(raw=True)
        out.append((bo, bp, piv, vet, ctx.pivots(), ctx.vetoes(), ctx.opt_candidates(), ctx.opt_finish(bp), ctx.near_ties_evaluated()))
        ctx.close()
    a, b = out
    assert a[:6] == b[:6]
    for u, v in zip(a[6], b[6]):
        assert np.array_equal(u, v)
    for u, v in zip(a[7], b[7]):
        assert np.array_equal(u, v)
    assert a[8] == b[8]


def test_solutions_arrays_and_blocks(partls):
    g = load_golden("synth_b")
    X, y, P = g["X"], g["y"], g["P"]
    for devices in (None, [0, 0]):
        _, _, rep = partls.fit(partls.Opt, X, y, P, returnAllSolutions=True, devices=devices)
        sols = rep.solutions
        opt, alpha, beta, t = sols.arrays()
        ref = [sols[b] for b in range(len(sols))]
        _close(opt, [o for o, _ in ref])
        _close(alpha, np.stack([m.α for _, m in ref])); _close(beta, np.stack([m.β for _, m in ref])); _close(t, [m.t for _, m in ref])
        blk = list(sols.blocks(7))
        assert all(len(b[0]) <= 7 for b in blk)
        bb = np.concatenate([b[0] for b in blk])
        assert np.array_equal(np.sort(bb), np.arange(len(sols)))
        for i, a in enumerate((opt, alpha, beta, t)):
            _close(np.concatenate([b[i + 1] for b in blk]), a[bb], 1e-10)        # other pieces, other chains: round-off apart
        # another fit takes the shared context over: the solutions are still those of this problem
        h = load_golden("synth_a")
        partls.fit(partls.Opt, h["X"], h["y"], h["P"], devices=devices)
        o2, a2, b2, t2 = sols.arrays()
        _close(o2, opt); _close(a2, alpha); _close(b2, beta); _close(t2, t)


def test_c3_size_piece_against_opt_pattern_and_the_oracle(partls, oracle):
    """N = 100k, D = 256, K = 20, faithful (2^21 patterns): one Gray piece of 2^17, 32 sampled rows"""
    rng = np.random.default_rng(2026)
    N, D, K = 100_000, 256, 20
    X = np.asfortranarray(rng.standard_normal((N, D)))
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), rng.integers(0, K, size=D)] = 1
    w = rng.standard_normal(D) * (rng.random(D) < 0.5)
    y = X @ w + 0.7 + 0.5 * rng.standard_normal(N)
    ctx = _ctx(partls, X, y, P)
    r = ctx.opt_models(0, 1 << 17, raw=True)
    assert r["n_unconverged"] == 0 and len(r["pattern"]) == 1 << 17
    rows = np.random.default_rng(7).choice(1 << 17, 32, replace=False)
    pats = r["pattern"][rows]
    Xo = np.hstack([X, np.ones((N, 1))])
    Po = np.zeros((D + 1, K + 1), dtype=np.int64)
    Po[:D, :K] = P
    Po[D, K] = 1
    Rf = np.linalg.qr(np.hstack([Xo, y[:, None]]), mode="r")
    objs, ra = oracle.opt_patterns(np.asfortranarray(Rf[:, :-1]), np.ascontiguousarray(Rf[:, -1]), Po, pats, want_alpha=True)
    for i, b in enumerate(pats):
        mine = r["raw_alpha"][rows[i]]
        tol = 1e-8 * max(1.0, np.abs(ra[i]).max())
        np.testing.assert_allclose(mine, ra[i], rtol=1e-8, atol=tol)
        pa, po = ctx.opt_pattern(int(b))
        np.testing.assert_allclose(mine, pa, rtol=1e-8, atol=tol)
        np.testing.assert_allclose(r["opt"][rows[i]], po, rtol=1e-8)
        a, bt, t = _cleanup(ra[i], P, int(b))
        np.testing.assert_allclose(r["alpha"][rows[i]], a, rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(r["beta"][rows[i]], bt, rtol=1e-8, atol=tol)
    ctx.close()
