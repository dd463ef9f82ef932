"""CPU checks of the robust fits: the entry points are declared (include/partls_robust.h, which include/partls.h
includes), exported and bound in a table of their own with the same argument types; fit_robust refuses what it does not support before
any device work; and the weight and scale rules of the header, restated in numpy (tests/robust_reference.py, the yardstick of the GPU
tests), give the hand-computed values on hand-made vectors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import check_julia_binding as CJ  # noqa: E402
import robust_reference as R  # noqa: E402

SYMS = ("partls_robust_weights", "partls_opt_reweight", "partls_get_robust_timing")
WANT = {"partls_robust_weights": ["partls_ctx*", "double*", "double*", "double", "int", "double", "double", "double*", "double*", "double*",
                                  "int64_t*", "int64_t*", "double*"],
        "partls_opt_reweight": ["partls_ctx*", "double*", "int"],
        "partls_get_robust_timing": ["partls_ctx*", "double*", "double*", "double*"]}
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int64)
# the ctypes forms a C parameter type may be bound as (an array that lives on the host or in HBM goes as an address)
CTYPES_FOR_C = {"partls_ctx*": (C.c_void_p,), "double*": (DP, C.c_void_p), "int64_t*": (IP,), "double": (C.c_double,), "int": (C.c_int,)}


def test_symbols_in_header_library_and_table(partls):
    protos = CJ.parse_header(CJ.ROBUST_HEADER)
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS_ROBUST}
    assert set(protos) == set(table) == set(SYMS)
    assert not set(SYMS) & set(CJ.parse_header())                        # not in the main header's own list ...
    assert '#include "partls_robust.h"' in open(os.path.join(ROOT, "include", "partls.h")).read()      # ... which includes theirs
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
    text = open(os.path.join(ROOT, "include", "partls_robust.h")).read()
    assert "#define PARTLS_ROBUST_HUBER 0" in text and "#define PARTLS_ROBUST_BISQUARE 1" in text
    assert (partls.lowlevel.ROBUST_HUBER, partls.lowlevel.ROBUST_BISQUARE) == (0, 1)
    assert partls.api.ROBUST_C == R.C_DEFAULT == {"huber": 1.345, "bisquare": 4.685}
    for name in ("fit_robust", "RobustConvergenceWarning"):
        assert name in partls.__all__ and getattr(partls, name) is getattr(partls.api, name)
    assert issubclass(partls.RobustConvergenceWarning, UserWarning)
    for method in ("robust_weights", "robust_weights_device", "opt_reweight", "opt_reweight_device"):
        assert callable(getattr(partls.Context, method))


# ---- refusals of fit_robust, before any device work -------------------------------------------------------------------------------
def _problem():
    rng = np.random.default_rng(0)
    return rng.normal(size=(12, 3)), rng.normal(size=12), np.array([[1, 0], [1, 0], [0, 1]])


def _no_device(*a, **k):
    raise AssertionError("device work started before the options were checked")


UNSUPPORTED = [("weights", dict(weights=np.ones(12))), ("restarts", dict(restarts=2)), ("top", dict(top=3)),
               ("returnAllSolutions", dict(returnAllSolutions=True))]
BAD = [dict(loss="cauchy"), dict(loss=None), dict(loss=0), dict(c=0.0), dict(c=-1.0), dict(c=np.nan), dict(c=np.inf), dict(c="1.345"),
       dict(scale=0.0), dict(scale=-2.0), dict(scale=np.nan), dict(scale=np.inf), dict(scale="iqr"), dict(scale=True),
       dict(max_iter=0), dict(max_iter=-3), dict(max_iter=2.5), dict(max_iter=True), dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf),
       dict(tol="1e-6")]


@pytest.mark.parametrize("name,kw", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_unsupported_options_are_named(partls, monkeypatch, name, kw):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    X, y, P = _problem()
    for alg in (partls.Opt, partls.Alt, partls.BnB):
        with pytest.raises(ValueError) as e:
            partls.fit_robust(alg, X, y, P, **kw)
        assert name in str(e.value)


def test_devices_is_not_implemented(partls, monkeypatch):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    X, y, P = _problem()
    for alg in (partls.Opt, partls.Alt, partls.BnB):
        for devices in (2, [0, 1]):
            with pytest.raises(NotImplementedError):
                partls.fit_robust(alg, X, y, P, devices=devices)


@pytest.mark.parametrize("kw", BAD, ids=["%s=%r" % next(iter(b.items())) for b in BAD])
def test_bad_options_raise_before_device_work(partls, monkeypatch, kw):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    X, y, P = _problem()
    for alg in (partls.Opt, partls.Alt, partls.BnB):
        with pytest.raises(ValueError):
            partls.fit_robust(alg, X, y, P, **kw)


def test_argument_errors_of_fit_come_first(partls, monkeypatch):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    X, y, P = _problem()
    with pytest.raises(TypeError):
        partls.fit_robust(object, X, y, P)
    with pytest.raises(TypeError):
        partls.fit_robust(partls.Opt, X.astype(np.int64), y, P)
    with pytest.raises(ValueError):
        partls.fit_robust(partls.Opt, X, y[:5], P)
    with pytest.raises(ValueError):
        partls.fit_robust(partls.BnB, X, y, P, rescue=True)
    with pytest.raises(ValueError):
        partls.fit_robust(partls.Alt, X, y, P, alpha0=np.ones((2, 4)), beta0=np.ones((2, 3)))
    with pytest.raises(ValueError):
        partls.fit_robust(partls.Alt, X, y, P, alpha0=np.ones(3), beta0=np.ones(3))


# ---- the rules of §1 on hand-made vectors -----------------------------------------------------------------------------------------
S = 0.6745


def test_scale_of_one_two_and_three_rows():
    assert R.mad_scale([3.0]) == (0.5 * 3.0 + 0.5 * 3.0) / S == 3.0 / S                      # N = 1: lo = hi = 0
    assert R.mad_scale([4.0, 1.0]) == (0.5 * 1.0 + 0.5 * 4.0) / S == 2.5 / S                 # N = 2: lo = 0, hi = 1
    assert R.mad_scale([9.0, 1.0, 2.0]) == 2.0 / S                                            # N = 3: lo = hi = 1
    assert R.mad_scale([5.0, 1.0, 2.0, 8.0]) == 3.5 / S                                       # N = 4: the ranks 1 and 2
    # the two halves are rounded before they are added: 0.5 * 5e-324 is 0, so two denormals of the smallest kind have median 0
    assert R.mad_scale([5e-324, 5e-324]) == 0.0 and R.mad_scale([1e300, 1e300]) == 1e300 / S


def test_all_equal_and_ties_at_the_middle_ranks():
    r = R.robust_info(np.full(5, 2.0), "huber")
    assert r["scale"] == 2.0 / S                          # k = 1.345 * 2 / 0.6745 > 2: every row inside
    assert np.array_equal(r["weights"], np.ones(5)) and r["max_dw"] == 0.0 and r["n_down"] == 0 and r["n_zero"] == 0
    u = 2.0 / (2.0 / S)
    assert np.array_equal(r["rho"], np.full(5, 0.5 * u * u))
    r = R.robust_info(np.array([0.0, 1.0, 1.0, 7.0]), "huber")            # a tie at the two middle ranks
    assert r["scale"] == 1.0 / S
    k = 1.345 * (1.0 / S)
    assert np.array_equal(r["weights"], np.array([1.0, 1.0, 1.0, k / 7.0])) and r["n_down"] == 1 and r["max_dw"] == 1.0 - k / 7.0
    r = R.robust_info(np.array([0.0, 1.0, 1.0, 7.0]), "bisquare")
    k = 4.685 * (1.0 / S)
    v = 1.0 - (1.0 / k) * (1.0 / k)
    assert np.array_equal(r["weights"], np.array([1.0, v * v, v * v, 0.0])) and r["n_down"] == 3 and r["n_zero"] == 1 and r["max_dw"] == 1.0
    assert r["rho"][3] == 4.685 * 4.685 / 6.0 and r["rho"][0] == 0.0


def test_more_than_half_zeros_gives_scale_zero():
    for a in ([0.0, 0.0, 5.0], [0.0, 0.0, 0.0, 1.0, 2.0], [0.0], [0.0, 0.0]):
        r = R.robust_info(np.array(a), "bisquare")
        assert r["scale"] == 0.0 and r["weights"] is None and (r["max_dw"], r["n_down"], r["n_zero"]) == (0.0, 0, 0)
    assert R.robust_info(np.array([0.0, 0.0, 1.0, 2.0]), "huber")["scale"] == 0.5 / S        # exactly half: the median is not 0
    assert R.robust_info(np.array([0.0, 0.0, 5.0]), "huber", scale=2.0)["scale"] == 2.0      # a fixed scale is taken as it is


def test_values_exactly_at_k():
    # scale 2, c = 1.5: k = 3.  Huber: a == k is inside (w = 1, rho = 0.5 u^2 = c u - 0.5 c^2 = 1.125 there); bisquare: u == 1 is out
    a = np.array([3.0, np.nextafter(3.0, 4.0), np.nextafter(3.0, 0.0), 6.0, 0.0])
    r = R.robust_info(a, "huber", c=1.5, scale=2.0)
    assert np.array_equal(r["weights"], np.array([1.0, 3.0 / a[1], 1.0, 0.5, 1.0])) and r["weights"][1] < 1.0
    assert r["rho"][0] == 1.125 and r["rho"][3] == 1.5 * 3.0 - 1.125 and r["rho"][4] == 0.0 and r["n_down"] == 2 and r["max_dw"] == 0.5
    r = R.robust_info(a, "bisquare", c=1.5, scale=2.0)
    assert r["weights"][0] == 0.0 and r["weights"][1] == 0.0 and r["weights"][3] == 0.0 and r["weights"][4] == 1.0
    u = a[2] / 3.0
    v = 1.0 - u * u
    assert 0.0 < r["weights"][2] == v * v < 1e-30 and r["n_zero"] == 3 and r["n_down"] == 4
    assert r["rho"][0] == 1.5 * 1.5 / 6.0 == 0.375 and r["rho"][4] == 0.0
    # against the previous weights, not against ones
    r2 = R.robust_info(a, "huber", c=1.5, scale=2.0, w_prev=np.array([1.0, 1.0, 0.25, 0.5, 1.0]))
    assert r2["max_dw"] == 0.75
