"""CPU checks of the regression diagnostics against the fake library of tools/api_call_trace.py: the entry points are
declared (include/partls_diag.h, which include/partls.h includes), exported, bound in a table of their own with the same argument
types and called by the Julia patch; diagnostics() makes exactly one prepare and one call, hands a float32 X on as float32, warns when
the model is not stationary on its support, and refuses a sparse X and bad arguments before any call."""
import ctypes as C
import hashlib
import os
import re
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import api_call_trace as T  # noqa: E402
import check_julia_binding as CJ  # noqa: E402

NAMES = ("h", "alpha", "beta", "t", "leverage", "loo", "studentized", "cooks", "residual", "se_w", "se_beta", "active", "summary")
SYMS = ("partls_diagnostics", "partls_get_diagnostics_timing")
SUMMARY = ("NPLUS", "P", "DOF", "RSS", "PRESS", "SIGMA2", "TSS", "R2", "R2_LOO", "STATIONARITY", "NSUM")


def test_symbols_in_header_library_table_and_julia(partls):
    protos = CJ.parse_header(CJ.DIAG_HEADER)
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS_DIAG}
    assert set(protos) == set(table) == set(SYMS)
    assert not set(SYMS) & set(CJ.parse_header())                        # not in the main header's own list ...
    assert '#include "partls_diag.h"' in open(os.path.join(ROOT, "include", "partls.h")).read()        # ... which includes theirs
    assert set(SYMS) <= set(CJ.parse_headers())
    partls.lowlevel.lib()                      # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    want = {"partls_diagnostics": ["partls_ctx*", "double*", "double*", "double"] + ["double*"] * 7 + ["int32_t*", "double*"],
            "partls_get_diagnostics_timing": ["partls_ctx*", "double*", "double*", "double*"]}
    assert len(want[SYMS[0]]) == len(NAMES)
    for name in SYMS:
        assert hasattr(lib, name), name
        ret, params = protos[name]
        assert ret == "partls_status" and params == want[name] and len(table[name][1]) == len(params), name
        assert table[name][0] is C.c_int
    assert partls.lowlevel.lib().partls_version() >= 109
    calls = {c[0] for c in CJ.parse_ccalls()}
    checked = {s for s, _ in CJ.check()}
    assert "partls_diagnostics" in calls and "partls_diagnostics" in checked
    for name in ("diagnostics", "Diagnostics"):
        assert name in partls.__all__ and getattr(partls, name) is getattr(partls.api, name)
    text = open(os.path.join(ROOT, "include", "partls_diag.h")).read()
    for i, name in enumerate(SUMMARY):                                   # the indices of the summary, header and binding alike
        assert re.search(r"#define PARTLS_DIAG_%s %d\b" % (name, i), text), name
        assert getattr(partls.lowlevel, "DIAG_" + name) == i


# ---- a fake device: records what the call was handed and writes what a device would ----------------------------------------------------
class _Device:
    """wraps the fake library's partls_diagnostics: every call is recorded (the model as copies, the addresses of the outputs) and the
    host outputs are written: row output number o gets o + 1 + i / 1024 in row i, se_w = 0.5, se_beta = 0.25, active all set, the summary
    from self.summary"""

    def __init__(self, fake, N, M, K, stationarity=1e-16):
        self.calls, self.N, self.M, self.K = [], N, M, K
        self.summary = np.array([N, M + 1, 3.0, 2.0, 2.5, 0.125, 8.0, 0.75, 0.6875, stationarity])
        self.inner = fake.partls_diagnostics
        fake.partls_diagnostics = self._call

    def _call(self, *args):
        assert len(args) == len(NAMES)
        status = self.inner(*args)
        a = dict(zip(NAMES, args))
        rec = {k: T._addr(a[k]) for k in NAMES[4:]}
        rec["alpha"] = np.ctypeslib.as_array((C.c_double * self.M).from_address(T._addr(a["alpha"]))).copy()
        rec["beta"] = np.ctypeslib.as_array((C.c_double * self.K).from_address(T._addr(a["beta"]))).copy()
        rec["t"] = float(a["t"])
        self.calls.append(rec)
        if status == 0 and not getattr(self, "on_device", False):
            for o, k in enumerate(NAMES[4:9]):
                if rec[k]:
                    np.ctypeslib.as_array((C.c_double * self.N).from_address(rec[k]))[:] = o + 1 + np.arange(self.N) / 1024
            if rec["se_w"]:
                np.ctypeslib.as_array((C.c_double * (self.M + 1)).from_address(rec["se_w"]))[:] = 0.5
            if rec["se_beta"]:
                np.ctypeslib.as_array((C.c_double * self.K).from_address(rec["se_beta"]))[:] = 0.25
            np.ctypeslib.as_array((C.c_int32 * (self.M + 1)).from_address(rec["active"]))[:] = 1
            np.ctypeslib.as_array((C.c_double * len(self.summary)).from_address(rec["summary"]))[:] = self.summary
        return status


@pytest.fixture
def fake(partls):
    with T.fake_library(partls.api) as f:
        yield f


P3 = np.array([[1, 0], [1, 0], [0, 1]])


def _problem(partls, N=6, seed=0):
    rng = np.random.default_rng(seed)
    X, y = rng.normal(size=(N, 3)), rng.normal(size=N)
    return X, y, partls.PartLSFitResult(np.array([0.5, 0.5, 1.0]), np.array([2.0, -1.0]), 0.25, P3)


def _lines(fake, prefix):
    return [ln for ln in fake.lines if ln.startswith(prefix)]


def test_one_prepare_and_one_call(partls, fake):
    X, y, model = _problem(partls)
    dev = _Device(fake, 6, 3, 2)
    d = partls.diagnostics(model, X, y)                                   # C-ordered float64
    assert len(_lines(fake, "partls_opt_prepare")) == 1 and len(_lines(fake, "partls_diagnostics(")) == 1 and len(dev.calls) == 1
    assert _lines(fake, "partls_opt_prepare")[0].startswith("partls_opt_prepare(") and "eta=0.0" in _lines(fake, "partls_opt_prepare")[0]
    c = dev.calls[-1]
    assert np.array_equal(c["alpha"], model.α) and np.array_equal(c["beta"], model.β) and c["t"] == 0.25
    assert all(c[k] for k in NAMES[4:])                                   # every output wanted
    assert isinstance(d, partls.Diagnostics)
    for o, k in enumerate(NAMES[4:9]):
        assert np.array_equal(getattr(d, k), o + 1 + np.arange(6) / 1024), k
    assert np.array_equal(d.se_w, np.full(4, 0.5)) and np.array_equal(d.se_beta, np.full(2, 0.25)) and d.se_t == 0.5
    assert d.active.dtype == bool and d.active.all()
    assert (d.n_pos, d.p, d.dof, d.rss, d.press, d.sigma2, d.tss, d.r2, d.r2_loo) == (6, 4, 3.0, 2.0, 2.5, 0.125, 8.0, 0.75, 0.6875)
    assert d.stationarity == 1e-16 and d.loo_mse == 2.5 / 6
    # eta and weights reach the prepare; loo_mse divides by the sum of the weights
    w = np.arange(1.0, 7.0)
    d = partls.diagnostics(model, X, y, η=0.5, weights=w)
    assert len(_lines(fake, "partls_opt_prepare")) == 2 and len(dev.calls) == 2
    ln = _lines(fake, "partls_opt_prepare")[-1]
    assert ln.startswith("partls_opt_prepare_weighted(") and "eta=0.5" in ln
    assert "w[6]=%s" % hashlib.sha1(w.tobytes()).hexdigest()[:8] in ln
    assert d.loo_mse == 2.5 / 21.0
    assert partls.diagnostics(model, X, y, eta=0.25).p == 4 and "eta=0.25" in _lines(fake, "partls_opt_prepare")[-1]


def test_float32_x_is_handed_on_as_float32(partls, fake):
    X, y, model = _problem(partls)
    _Device(fake, 6, 3, 2)
    X32 = X.astype(np.float32)
    for Xin in (X32, np.asfortranarray(X32), np.ascontiguousarray(X32.T).T):
        partls.diagnostics(model, Xin, y.astype(np.float32))
        ln = _lines(fake, "partls_opt_prepare")[-1]
        assert ln.startswith("partls_opt_prepare_f32(")
        assert "X[18]=%s" % hashlib.sha1(np.asfortranarray(X32).tobytes(order="F")).hexdigest()[:8] in ln        # 18 floats: not widened
        assert "y[6]=%s" % hashlib.sha1(y.astype(np.float32).astype(np.float64).tobytes()).hexdigest()[:8] in ln
    partls.diagnostics(model, X32, y, weights=np.ones(6))
    assert _lines(fake, "partls_opt_prepare")[-1].startswith("partls_opt_prepare_f32(")
    assert len(_lines(fake, "partls_opt_prepare")) == len(_lines(fake, "partls_diagnostics(")) == 4


def test_warns_when_the_model_is_not_stationary(partls, fake):
    X, y, model = _problem(partls)
    _Device(fake, 6, 3, 2, stationarity=1e-9)
    with pytest.warns(partls.IllConditionedWarning, match="stationarity"):
        d = partls.diagnostics(model, X, y)
    assert d.stationarity == 1e-9
    _Device(fake, 6, 3, 2, stationarity=1e-13)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        partls.diagnostics(model, X, y)


def test_context_methods_pass_host_arrays_or_device_addresses(partls, fake):
    X, y, model = _problem(partls)
    dev = _Device(fake, 6, 3, 2)
    ctx = partls.Context(0)
    with pytest.raises(ValueError):
        ctx.diagnostics(model.α, model.β, model.t)                        # nothing prepared
    ctx.opt_prepare(X, y, P3)
    out = ctx.diagnostics(model.α, model.β, model.t, rows=("loo", "residual"), want_se=False)
    c = dev.calls[-1]
    assert set(out) == {"loo", "residual", "se_w", "se_beta", "active", "summary"} and out["se_w"] is None and out["se_beta"] is None
    assert (c["leverage"], c["studentized"], c["cooks"], c["se_w"], c["se_beta"]) == (0, 0, 0, 0, 0)
    assert c["loo"] == out["loo"].ctypes.data and c["residual"] == out["residual"].ctypes.data and c["active"] and c["summary"]
    with pytest.raises(ValueError):
        ctx.diagnostics(model.α, model.β, model.t, rows=("hat",))
    with pytest.raises(ValueError):
        ctx.diagnostics_device(model.α, model.β, model.t, dloo_ptr=0x7f0000005000)        # prepared from host arrays
    with pytest.raises(ValueError):
        ctx.diagnostics(model.α[:2], model.β, model.t)
    with pytest.raises(ValueError):
        ctx.diagnostics(model.α, np.array([np.nan, 1.0]), model.t)
    n = len(dev.calls)
    ctx.opt_prepare_device(0x7f0000001000, 0x7f0000002000, 6, 3, 8, P3, 0.5)
    dev.on_device = True
    out = ctx.diagnostics_device(model.α, model.β, model.t, dleverage_ptr=0x7f0000005000, dcooks_ptr=0x7f0000006000)
    c = dev.calls[-1]
    assert (c["leverage"], c["loo"], c["studentized"], c["cooks"], c["residual"]) == (0x7f0000005000, 0, 0, 0x7f0000006000, 0)
    assert c["se_w"] == out["se_w"].ctypes.data and c["se_beta"] == out["se_beta"].ctypes.data and set(out) == {"se_w", "se_beta", "active", "summary"}
    with pytest.raises(ValueError):
        ctx.diagnostics(model.α, model.β, model.t)                        # prepared from device pointers
    assert len(dev.calls) == n + 1
    assert ctx.diagnostics_timing() == (0.0, 0.0, 0.0)
    ctx.close()


def test_bad_arguments_are_refused_before_any_call(partls, fake):
    X, y, model = _problem(partls)
    mk = partls.PartLSFitResult

    class Sparse:                                                          # anything with .tocsr() counts as sparse
        def tocsr(self):
            raise AssertionError("a refused matrix is not converted")

    with pytest.raises(NotImplementedError) as e:
        partls.diagnostics(model, Sparse(), y)
    assert "diagnostics" in str(e.value) and "densify" in str(e.value)
    with pytest.raises(NotImplementedError):
        partls.diagnostics(model, partls.CSR(np.zeros(7, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (6, 3)), y)
    with pytest.raises(TypeError):
        partls.diagnostics((model.α, model.β, model.t, P3), X, y)         # not a PartLSFitResult
    with pytest.raises(TypeError):
        partls.diagnostics(model, X.astype(np.int64), y)
    with pytest.raises(TypeError):
        partls.diagnostics(model, X, y.astype(np.int64))
    with pytest.raises(TypeError):
        partls.diagnostics(model, X[0], y)
    for bad in ((model, X[:, :2], y), (model, X, y[:5]), (mk(model.α[:2], model.β, 0.0, P3), X, y), (mk(model.α, model.β[:1], 0.0, P3), X, y),
                (mk(model.α, np.array([1.0, np.inf]), 0.0, P3), X, y), (mk(model.α, model.β, np.nan, P3), X, y)):
        with pytest.raises(ValueError):
            partls.diagnostics(*bad)
    for kw in (dict(η=-1.0), dict(eta=np.nan), dict(weights=np.ones(5)), dict(weights=-np.ones(6)), dict(weights=np.zeros(6)),
               dict(weights=np.full(6, np.nan))):
        with pytest.raises(ValueError):
            partls.diagnostics(model, X, y, **kw)
    assert not _lines(fake, "partls_opt_prepare") and not _lines(fake, "partls_diagnostics")
