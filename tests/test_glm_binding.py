"""CPU checks of the generalised linear fits: the entry points are declared (include/partls_glm.h, which
include/partls.h includes), exported and bound in a table of their own with the same argument types; fit_glm refuses what it does not
support before any device work; the formulas of the header, restated in numpy (tests/glm_reference.py, the yardstick of the GPU tests),
give the hand-computed values on hand-made vectors and — in float64 — meet the header's own error bound against np.longdouble; and
the committed problems of tests/golden meet the conditions they were chosen by, at every iteration of the reference's own loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import check_julia_binding as CJ  # noqa: E402
import glm_reference as G  # noqa: E402

SYMS = ("partls_glm_working", "partls_opt_rework", "partls_glm_mean", "partls_get_glm_timing")
WANT = {"partls_glm_working": ["partls_ctx*", "double*", "double*", "double", "int", "double*", "double*", "int64_t*", "double*", "double*",
                               "double*"],
        "partls_opt_rework": ["partls_ctx*", "double*", "double*", "int"],
        "partls_glm_mean": ["partls_ctx*", "int", "double*", "int64_t", "int", "double*"],
        "partls_get_glm_timing": ["partls_ctx*", "double*", "double*"]}
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int64)
# the ctypes forms a C parameter type may be bound as (an array that lives on the host or in HBM goes as an address)
CTYPES_FOR_C = {"partls_ctx*": (C.c_void_p,), "double*": (DP, C.c_void_p), "int64_t*": (IP,), "double": (C.c_double,), "int": (C.c_int,),
                "int64_t": (C.c_int64,)}


def test_symbols_in_header_library_and_table(partls):
    protos = CJ.parse_header(CJ.GLM_HEADER)
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS_GLM}
    assert set(protos) == set(table) == set(SYMS)
    assert not set(SYMS) & set(CJ.parse_header())                        # not in the main header's own list ...
    assert '#include "partls_glm.h"' in open(os.path.join(ROOT, "include", "partls.h")).read()      # ... which includes theirs
    assert set(SYMS) <= set(CJ.parse_headers())
    partls.lowlevel.lib()                      # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    for name in SYMS:
        assert hasattr(lib, name), name
        ret, params = protos[name]
        res, args = table[name]
        assert ret == "partls_status" and res is C.c_int and params == WANT[name] and len(args) == len(params), name
        for k, (ct, at) in enumerate(zip(params, args)):
            assert at in CTYPES_FOR_C[ct], (name, k, ct, at)
    text = open(os.path.join(ROOT, "include", "partls_glm.h")).read()
    assert "#define PARTLS_GLM_BINOMIAL 0" in text and "#define PARTLS_GLM_POISSON 1" in text
    assert (partls.lowlevel.GLM_BINOMIAL, partls.lowlevel.GLM_POISSON) == (0, 1)
    k = G.constants()
    assert k["U"] == 2.0 ** -53 and k["CLAMP"] == G.CLAMP == 30.0
    assert partls.api.GLM_FAMILIES == G.FAMILIES
    for name in ("fit_glm", "predict_mean", "GLMConvergenceWarning"):
        assert name in partls.__all__ and getattr(partls, name) is getattr(partls.api, name)
    assert issubclass(partls.GLMConvergenceWarning, UserWarning)
    for method in ("glm_working", "glm_working_device", "opt_rework", "opt_rework_device", "glm_mean"):
        assert callable(getattr(partls.Context, method))
    done = {sym for sym, _ in CJ.check()}
    assert set(SYMS) <= done                   # INTEGRATION.md has a ccall shim for each of them


# ---- refusals of fit_glm, before any device work --------------------------------------------------------------------------------------
def _problem():
    rng = np.random.default_rng(0)
    return rng.normal(size=(12, 3)), (rng.random(12) < 0.5).astype(np.float64), np.array([[1, 0], [1, 0], [0, 1]])


def _no_device(*a, **k):
    raise AssertionError("device work started before the options were checked")


UNSUPPORTED = [("weights", dict(weights=np.ones(12))), ("restarts", dict(restarts=2)), ("top", dict(top=3)),
               ("returnAllSolutions", dict(returnAllSolutions=True))]
BAD = [dict(family="gaussian"), dict(family=None), dict(family=0), dict(family=["binomial"]),
       dict(max_iter=0), dict(max_iter=-3), dict(max_iter=2.5), dict(max_iter=True), dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf),
       dict(tol="1e-8")]


@pytest.fixture
def no_device(partls, monkeypatch):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)


@pytest.mark.parametrize("name,kw", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_unsupported_options_are_named(partls, no_device, name, kw):
    X, y, P = _problem()
    for alg in (partls.Opt, partls.Alt, partls.BnB):
        for family in G.FAMILIES:
            with pytest.raises(ValueError) as e:
                partls.fit_glm(alg, X, y, P, family=family, **kw)
            assert name in str(e.value)


def test_devices_is_not_implemented(partls, no_device):
    X, y, P = _problem()
    for alg in (partls.Opt, partls.Alt, partls.BnB):
        for devices in (2, [0, 1]):
            with pytest.raises(NotImplementedError):
                partls.fit_glm(alg, X, y, P, devices=devices)


@pytest.mark.parametrize("kw", BAD, ids=["%s=%r" % next(iter(b.items())) for b in BAD])
def test_bad_options_raise_before_device_work(partls, no_device, kw):
    X, y, P = _problem()
    for alg in (partls.Opt, partls.Alt, partls.BnB):
        with pytest.raises(ValueError):
            partls.fit_glm(alg, X, y, P, **kw)


@pytest.mark.parametrize("family,value", [("binomial", np.nan), ("binomial", np.inf), ("binomial", 1.5), ("binomial", -0.25),
                                          ("poisson", np.nan), ("poisson", np.inf), ("poisson", -1.0)])
def test_a_response_outside_the_domain_raises_before_device_work(partls, no_device, family, value):
    X, y, P = _problem()
    y[7] = value
    for alg in (partls.Opt, partls.Alt, partls.BnB):
        with pytest.raises(ValueError) as e:
            partls.fit_glm(alg, X, y, P, family=family)
        assert "fit_glm" in str(e.value)


def test_argument_errors_of_fit_come_first(partls, no_device):
    X, y, P = _problem()
    with pytest.raises(TypeError):
        partls.fit_glm(object, X, y, P)
    with pytest.raises(TypeError):
        partls.fit_glm(partls.Opt, X.astype(np.int64), y, P)
    with pytest.raises(ValueError):
        partls.fit_glm(partls.Opt, X, y[:5], P)
    with pytest.raises(ValueError):
        partls.fit_glm(partls.BnB, X, y, P, rescue=True)
    with pytest.raises(ValueError):
        partls.fit_glm(partls.Alt, X, y, P, alpha0=np.ones((2, 4)), beta0=np.ones((2, 3)))
    with pytest.raises(ValueError):
        partls.predict_mean(None, X, "gaussian")


# ---- the formulas of the header on hand-made vectors --------------------------------------------------------------------------------------
ETAS = np.array([0.0, -0.0, 30.0, -30.0, 30.000001, -30.000001, 700.0, -700.0, 5e-324, -5e-324])


def _f(fn, x, n=len(ETAS)):
    """fn(x) as numpy's array loop of n elements computes it (its scalar and array paths may differ in the last bit)"""
    return float(fn(np.full(n, x))[0])


LOG2, E30 = _f(np.log1p, 1.0), _f(np.exp, -30.0)


def test_binomial_rows_by_hand():
    for y, z0, d0 in ((0.0, -2.0, 2.0 * LOG2), (1.0, 2.0, 2.0 * LOG2), (0.5, 0.0, None)):
        r = G.rows(ETAS, np.full(len(ETAS), y), "binomial")
        assert np.all(np.isfinite(np.r_[r["W"], r["z"], r["mu"], r["d"]]))
        assert list(r["clamped"]) == [False, False, False, False, True, True, True, True, False, False]
        for i in (0, 1, 8, 9):                                # eta = 0, -0 and the denormals: e = 1, q = p = 1/2
            assert (r["mu"][i], r["W"][i], r["z"][i]) == (0.5, 0.25, ETAS[i] + z0)     # (a denormal vanishes beside 2)
            assert r["d"][i] == d0 if d0 is not None else abs(r["d"][i]) <= 4 * 2.0 ** -53 * 2 * LOG2
        # +-30 and everything beyond it give the rows of +-30
        for base, same in ((2, (4, 6)), (3, (5, 7))):
            for i in same:
                assert all(r[k][i] == r[k][base] for k in ("W", "z", "mu", "d", "ec"))
        q = 1.0 / (1.0 + E30)
        p = E30 * q
        assert (r["mu"][2], r["mu"][3]) == (q, p) and r["W"][2] == r["W"][3] == p * q > 9.3e-14
        assert r["z"][2] == 30.0 + (y - q) / (p * q) and r["z"][3] == -30.0 + (y - p) / (p * q)
        l = _f(np.log1p, E30)
        if y == 1.0:
            assert r["d"][2] == 2.0 * l and r["d"][3] == 2.0 * (30.0 + l)        # -2 log mu
        if y == 0.0:
            assert r["d"][2] == 2.0 * (30.0 + l) and r["d"][3] == 2.0 * l        # -2 log (1 - mu), without cancellation
    m = G.rows(np.array([-0.0]), np.array([1.0]), "binomial")
    assert m["ec"][0] == 0.0 and np.signbit(m["ec"][0]) and m["mu"][0] == 0.5     # -0 counts as >= 0 and stays unclamped


def test_poisson_rows_by_hand():
    r = G.rows(ETAS, np.zeros(len(ETAS)), "poisson")          # y = 0: xlogy is 0, not NaN
    assert np.all(np.isfinite(np.r_[r["W"], r["z"], r["mu"], r["d"]]))
    assert list(r["clamped"]) == [False, False, False, False, True, True, True, True, False, False]
    for i in (0, 1, 8, 9):
        assert (r["mu"][i], r["W"][i], r["z"][i], r["d"][i]) == (1.0, 1.0, -1.0, 2.0)
    assert r["mu"][6] == r["mu"][4] == r["mu"][2] == _f(np.exp, 30.0) and r["mu"][7] == r["mu"][5] == r["mu"][3] == E30
    assert r["d"][3] == 2.0 * E30 and r["z"][3] == -30.0 + (0.0 - E30) / E30 == -31.0
    log3 = _f(np.log, 3.0, 2)
    r = G.rows(np.array([0.0, log3]), np.array([3.0, 3.0]), "poisson")
    assert (r["mu"][0], r["z"][0]) == (1.0, 2.0) and r["d"][0] == 2.0 * ((3.0 * log3 - 0.0) - 2.0)
    assert abs(r["d"][1]) <= 16 * 2.0 ** -53 * 3.0 * log3                       # the saturated row: deviance 0 up to rounding


def test_the_start_by_hand():
    e = G.start_eta(np.array([0.0, 1.0, 0.5]), "binomial")
    assert e[2] == 0.0 and e[0] == _f(np.log, 0.25 / 0.75, 3) and e[1] == _f(np.log, 0.75 / 0.25, 3)
    e = G.start_eta(np.array([0.0, 2.0]), "poisson")
    assert e[0] == _f(np.log, 0.1, 2) and e[1] == _f(np.log, 2.1, 2)
    assert G.null_deviance(np.array([0.0, 1.0]), "binomial") == pytest.approx(4.0 * LOG2, rel=1e-15)
    assert G.null_deviance(np.array([2.0, 2.0]), "poisson") == 0.0


# ---- the float64 restatement meets the header's bound against longdouble: the yardstick's own yardstick ------------------------
def _mixed(seed, N, family):
    """eta on both sides of 0 and of the clamp, with exact hits of 0, -0 and +-30; y over the family's domain with its edges"""
    rng = np.random.default_rng(seed)
    eta = np.concatenate([rng.normal(0.0, 3.0, N // 2), rng.uniform(-40.0, 40.0, N - N // 2 - 8), ETAS[:8]])
    if family == "binomial":
        y = rng.choice([0.0, 1.0, 0.5, 0.25, 1e-20, 1.0 - 2.0 ** -53], size=N, p=[0.35, 0.35, 0.1, 0.1, 0.05, 0.05])
        y[rng.random(N) < 0.2] = rng.random()
    else:
        y = rng.poisson(np.exp(np.clip(eta, -3.0, 6.0))).astype(np.float64)
        y[::7] = 0.0
    return eta, y


@pytest.mark.parametrize("family", G.FAMILIES)
def test_numpy_float64_rows_meet_the_bound(family):
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than double here: no reference"
    eta, y = _mixed(5, 20000, family)
    got = G.rows(eta, y, family)
    G.check_rows(got, eta, y, family, start=False, where=" numpy")
    ys = y if family == "binomial" else np.r_[y, 1e13, 2e13, 1e-300, 5e-324]     # the start beyond the clamp, and tiny counts
    got = G.rows(G.start_eta(ys, family), ys, family)
    G.check_rows(got, None, ys, family, start=True, where=" numpy")


# ---- the committed problems ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", G.FAMILIES)
def test_fixtures_meet_their_conditions(oracle, family):
    X, y, P, rec = G.fixture(family)
    assert X.shape == (G.FIX_N, G.FIX_M) and P.shape == (G.FIX_M, G.FIX_K)
    Xm, ym, Pm = G.make_problem(family, G.FIXTURES[family][1])
    assert np.array_equal(X, Xm) and np.array_equal(y, ym) and np.array_equal(P, Pm)
    ref = G.irls(oracle, X, y, P, family)
    print("[glm] fixture %s: iterations %d, gaps %r, margins %r, deviance %r" % (family, ref["iterations"], ref["gaps"], ref["margins"],
                                                                                  ref["deviance"]))
    assert ref["converged"] and ref["iterations"] <= 25
    assert min(ref["gaps"]) > 1e-6                            # best and second-best sign pattern apart, at every iteration
    assert G.fixture_ok(ref)
    assert np.allclose(ref["alpha"], rec["alpha"], rtol=0, atol=1e-10) and np.allclose(ref["beta"], rec["beta"], rtol=0, atol=1e-10)
    assert abs(ref["t"] - rec["t"]) <= 1e-10 and np.allclose(ref["deviance"], rec["deviance"], rtol=1e-12)
    assert ref["deviance"][-1] < G.null_deviance(y, family) and ref["deviance"][-1] < ref["deviance"][0]
