"""CPU checks of the float32 design-matrix path: the three entry points are declared by the header
(include/partls_f32.h, which include/partls.h includes), exported by the library, bound by the ctypes table (SYMBOLS_F32) with the
same argument counts, and called by the Julia drop-in (tools/check_julia_binding.py); and fit / predict hand a
float32 X over as an F-contiguous float32 array — copied when it is C-ordered or strided, never widened — while every other dtype,
devices= and cross_validate keep getting float64."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_julia_binding as CJ  # noqa: E402

NEW = {"partls_opt_prepare_f32": 13, "partls_predict_f32": 12, "partls_predict_device_f32": 12}


def test_symbols_in_header_library_and_table(partls):
    protos = CJ.parse_header(CJ.F32_HEADER)
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS_F32}
    assert set(protos) == set(table) == set(NEW)
    assert '#include "partls_f32.h"' in open(os.path.join(ROOT, "include", "partls.h")).read()
    partls.lowlevel.lib()              # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    for s, n in NEW.items():
        assert s in protos and s in table and hasattr(lib, s), s
        assert len(protos[s][1]) == len(table[s][1]) == n, s
        assert protos[s][0] == "partls_status" and protos[s][1][1] == "float*", s       # X is the second parameter, a float pointer
    assert protos["partls_opt_prepare_f32"][1][5:7] == ["double*", "double*"]            # y and w stay double
    assert partls.lowlevel.lib().partls_version() >= 102


def test_integration_calls_the_entry_points_with_float32_pointers():
    calls = {c[0]: c for c in CJ.parse_ccalls()}
    checked = {s for s, _ in CJ.check()}
    for s in NEW:
        assert s in calls and s in checked, s
        assert calls[s][2][1] in ("Ptr{Float32}", "Ptr{Cfloat}"), s
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 7. `Matrix{Float32}`"):text.index("## Notes for the maintainer")]
    assert "X::Matrix{Float32}" in sec and "Matrix{Float64}(X)" not in sec.split("```julia", 1)[1]


def test_checker_rejects_a_double_pointer_for_a_float_parameter(tmp_path):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    i = text.index("ccall((:partls_predict_f32")
    j = text.index("Ptr{Float32}", i)
    bad = tmp_path / "INTEGRATION.md"
    bad.write_text(text[:j] + "Ptr{Float64}" + text[j + len("Ptr{Float32}"):])
    with pytest.raises(AssertionError):
        CJ.check(integration=str(bad))


# ---- what fit / predict hand to the context ---------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the default context (and the default multi-context): records the arrays it is given, computes nothing"""

    def __init__(self):
        self.seen = []
        self.tolerate_ill = False
        self.last_ill = False
        self.generation = 0
        self.devices = [0, 0]
        self._h = None

    def _note(self, what, X):
        assert isinstance(X, np.ndarray)
        self.seen.append((what, X))
        self._M = X.shape[1]

    def opt_prepare(self, X, y, P, eta=0.0, flags=0, weights=None):
        self._note("prepare", X)
        assert y.dtype == np.float64 and (weights is None or weights.dtype == np.float64)
        self._K = P.shape[1]

    def opt_sweep(self, g_begin=0, g_end=-1, want_all=False):
        return 0.0, 0, None, 0

    def opt_finish(self, pattern):
        return np.zeros(self._M), np.zeros(self._K), 0.0, 0.0, 0

    def alt_prepared(self, a0, b0, eps=1e-6, T=100):
        return np.zeros(self._M), np.zeros(self._K), 0.0, 0.0, 1

    def bnb_prepared(self):
        return np.zeros(self._M), np.zeros(self._K), 0.0, 0.0, 1

    def fit_opt(self, X, y, P, eta=0.0, flags=0, want_all=False):
        self._note("multi", X)
        return np.zeros(X.shape[1]), np.zeros(P.shape[1]), 0.0, 0.0, 0, None

    def cv_opt(self, X, y, P, fold_ptr, etas, flags=0, device_ptrs=None, weights=None):
        self._note("cv", X)
        raise _Stop()

    def predict(self, X, P, alpha, beta, t):
        self._note("predict", X)
        return np.zeros(X.shape[0])


class _Stop(Exception):
    pass


@pytest.fixture
def recorder(partls, monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(partls.api, "default_context", lambda device=0: r)
    monkeypatch.setattr(partls.api, "default_multi", lambda devices=None: r)
    return r


def _inputs():
    rng = np.random.default_rng(0)
    big = rng.normal(size=(24, 6)).astype(np.float32)
    layouts = {"F": np.asfortranarray(big[:12, :3]), "C": np.ascontiguousarray(big[:12, :3]), "strided": big[::2, ::2]}
    assert layouts["F"].flags.f_contiguous and layouts["C"].flags.c_contiguous and not layouts["C"].flags.f_contiguous
    assert not layouts["strided"].flags.f_contiguous and not layouts["strided"].flags.c_contiguous
    y = rng.normal(size=12).astype(np.float32)
    P = np.array([[1, 0], [1, 0], [0, 1]])
    return layouts, y, P


@pytest.mark.parametrize("layout", ["F", "C", "strided"])
def test_float32_input_reaches_the_context_as_float32(partls, recorder, layout):
    layouts, y, P = _inputs()
    X = layouts[layout]
    keep = X.copy()
    a0, b0 = np.ones(4), np.ones(3)
    partls.fit(partls.Opt, X, y, P)
    partls.fit(partls.Opt, X, y, P, weights=np.ones(12), returnAllSolutions=True)
    partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0)
    partls.fit(partls.BnB, X, y, P)
    model = partls.PartLSFitResult(np.ones(3), np.ones(2), 0.5, P)
    partls.predict(model, X)
    partls.predict(model.α, model.β, model.t, P, X)
    assert [w for w, _ in recorder.seen] == ["prepare"] * 4 + ["predict"] * 2
    for what, got in recorder.seen:
        assert got.dtype == np.float32 and got.flags.f_contiguous, what
        assert np.array_equal(got, keep), what
    assert np.array_equal(X, keep)


def test_returned_solutions_carry_the_float32_matrix(partls, recorder):
    layouts, y, P = _inputs()
    _, _, rep = partls.fit(partls.Opt, layouts["C"], y, P, returnAllSolutions=True)
    Xf = rep.solutions._problem[0]
    assert Xf.dtype == np.float32 and Xf.flags.f_contiguous and np.array_equal(Xf, layouts["C"])


@pytest.mark.parametrize("dtype", [np.float64, np.float16])
def test_other_float_dtypes_are_widened_as_before(partls, recorder, dtype):
    layouts, y, P = _inputs()
    X = layouts["C"].astype(dtype)
    partls.fit(partls.Opt, X, y, P)
    partls.predict(partls.PartLSFitResult(np.ones(3), np.ones(2), 0.5, P), X)
    assert [w for w, _ in recorder.seen] == ["prepare", "predict"]
    for what, got in recorder.seen:
        assert got.dtype == np.float64 and got.flags.f_contiguous and np.array_equal(got, X.astype(np.float64)), what


def test_devices_and_cross_validate_widen_float32_on_the_host(partls, recorder):
    layouts, y, P = _inputs()
    X = layouts["F"]
    partls.fit(partls.Opt, X, y, P, devices=[0, 0])
    with pytest.raises(_Stop):
        partls.cross_validate(partls.Opt, X, y, P, nfolds=3)
    assert [w for w, _ in recorder.seen] == ["multi", "cv"]
    for what, got in recorder.seen:
        assert got.dtype == np.float64 and got.flags.f_contiguous and np.array_equal(got, X.astype(np.float64)), what


def test_device_entry_points_reject_other_dtypes(partls):
    ctx = partls.Context.__new__(partls.Context)          # no device: the dtype is checked before anything is called
    ctx._h, ctx.generation = C.c_void_p(), 0
    P = np.ones((3, 1), dtype=np.int64)
    with pytest.raises(TypeError):
        ctx.opt_prepare_device(0, 0, 4, 3, 4, P, dtype=np.float16)
    with pytest.raises(TypeError):
        ctx.predict_device(0, 4, 3, 4, P, np.ones(3), np.ones(1), 0.0, 0, dtype=np.int32)
