"""CPU checks of the multistart fit(Alt): partls_alt_multistart is declared by the header, exported by the library,
bound by the ctypes table with the same parameter count and called by the Julia drop-in (INTEGRATION.md,
tools/check_julia_binding.py); fit(Alt, restarts=...) rejects every misuse with ValueError before any device work, and hands the
context R successive draws of the generator — row 0 is the start of the single fit with the same seed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_julia_binding as CJ  # noqa: E402

SYM = "partls_alt_multistart"


def test_symbol_in_header_library_and_table(partls):
    protos = CJ.parse_header()
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS}
    partls.lowlevel.lib()              # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    assert SYM in protos and SYM in table and hasattr(lib, SYM)
    assert protos[SYM][0] == "partls_status"
    assert len(protos[SYM][1]) == len(table[SYM][1]) == 22
    assert protos[SYM][1][-1] == "int32_t*" and protos[SYM][1][12:14] == ["int64_t*", "int64_t*"]      # status_all; iters, best_start
    assert partls.lowlevel.lib().partls_version() >= 103


def test_integration_calls_the_entry_point():
    calls = {c[0]: c for c in CJ.parse_ccalls()}
    checked = {s for s, _ in CJ.check()}
    assert SYM in calls and SYM in checked
    assert len(calls[SYM][2]) == 22
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "restarts" in text[text.index("ccall((:" + SYM) - 4000:text.index("ccall((:" + SYM)]


def _problem():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(12, 3))
    y = rng.normal(size=12)
    P = np.array([[1, 0], [1, 0], [0, 1]])
    return X, y, P


def _no_device(*a, **k):
    raise AssertionError("device work started before the arguments were checked")


M, K = 3, 2
BAD = [
    ("restarts_with_1d_starts", dict(restarts=2, alpha0=np.ones(M + 1), beta0=np.ones(K + 1))),
    ("restarts_zero", dict(restarts=0)),
    ("restarts_negative", dict(restarts=-3)),
    ("restarts_not_an_integer", dict(restarts=2.5)),
    ("restarts_disagrees_with_the_rows", dict(restarts=3, alpha0=np.ones((2, M + 1)), beta0=np.ones((2, K + 1)))),
    ("row_counts_differ", dict(alpha0=np.ones((2, M + 1)), beta0=np.ones((3, K + 1)))),
    ("alpha0_too_narrow", dict(alpha0=np.ones((2, M)), beta0=np.ones((2, K + 1)))),
    ("beta0_too_wide", dict(alpha0=np.ones((2, M + 1)), beta0=np.ones((2, K + 2)))),
    ("only_alpha0", dict(alpha0=np.ones((2, M + 1)))),
    ("matrix_with_vector", dict(alpha0=np.ones((2, M + 1)), beta0=np.ones(K + 1))),
    ("no_rows", dict(alpha0=np.ones((0, M + 1)), beta0=np.ones((0, K + 1)))),
    ("nan_start", dict(alpha0=np.ones((2, M + 1)), beta0=np.array([[1.0, np.nan, 1.0], [1.0, 1.0, 1.0]]))),
    ("inf_start", dict(alpha0=np.array([[1.0, 1.0, np.inf, 1.0], [1.0] * 4]), beta0=np.ones((2, K + 1)))),
]


@pytest.mark.parametrize("name,kw", BAD, ids=[b[0] for b in BAD])
def test_misuse_raises_before_device_work(partls, monkeypatch, name, kw):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    X, y, P = _problem()
    with pytest.raises(ValueError):
        partls.fit(partls.Alt, X, y, P, **kw)


@pytest.mark.parametrize("alg", ["Opt", "BnB"])
def test_restarts_is_an_option_of_alt_only(partls, monkeypatch, alg):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    X, y, P = _problem()
    with pytest.raises(ValueError):
        partls.fit(getattr(partls, alg), X, y, P, restarts=4)


class _Recorder:
    """stands in for the default context: records what it is given, computes nothing"""

    def __init__(self):
        self.calls = []
        self.tolerate_ill = False
        self.last_ill = False
        self.generation = 0
        self._h = None

    def opt_prepare(self, X, y, P, eta=0.0, flags=0, weights=None):
        self.calls.append(("opt_prepare", X, flags, weights))
        self._M, self._K = X.shape[1], P.shape[1]

    def alt_prepared(self, a0, b0, eps=1e-6, T=100):
        self.calls.append(("alt_prepared", a0, b0))
        return np.zeros(self._M), np.zeros(self._K), 0.0, 0.0, 1

    def alt_multistart(self, a0, b0, eps=1e-6, T=100):
        self.calls.append(("alt_multistart", a0, b0, eps, T))
        R = len(a0)
        per = dict(opt=np.arange(R, dtype=float), iters=np.ones(R, dtype=np.int64), status=np.zeros(R, dtype=np.int32),
                   alpha=np.zeros((R, self._M)), beta=np.zeros((R, self._K)), t=np.zeros(R))
        return np.zeros(self._M), np.zeros(self._K), 0.0, 0.0, 1, 0, per


@pytest.fixture
def recorder(partls, monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(partls.api, "default_context", lambda device=0: r)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    return r


def test_restarts_draws_successive_single_starts(partls, recorder):
    X, y, P = _problem()
    seed, R = 41, 5
    model, _, rep = partls.fit(partls.Alt, X, y, P, restarts=R, rng=seed, ϵ=1e-4, T=7)
    assert [c[0] for c in recorder.calls] == ["opt_prepare", "alt_multistart"]
    assert recorder.calls[0][2] == partls.lowlevel.OPT_FAITHFUL_INTERCEPT
    _, a0, b0, eps, T = recorder.calls[1]
    assert (eps, T) == (1e-4, 7) and a0.shape == (R, M + 1) and b0.shape == (R, K + 1)
    gen = np.random.default_rng(seed)
    for r in range(R):
        assert np.array_equal(a0[r], gen.random(M + 1))
        assert np.array_equal(b0[r], (gen.random(K + 1) - 0.5) * 10)
    assert rep.best_start == 0 and rep.iters == 1 and rep.opt == 0.0
    assert set(rep.starts) == {"opt", "iters", "status", "alpha", "beta", "t"} and len(rep.starts.opt) == R
    assert model.α.shape == (M,) and model.β.shape == (K,)
    # a Generator is consumed in the same way
    recorder.calls.clear()
    partls.fit(partls.Alt, X, y, P, restarts=2, rng=np.random.default_rng(seed))
    assert np.array_equal(recorder.calls[1][1], a0[:2]) and np.array_equal(recorder.calls[1][2], b0[:2])


def test_start_zero_is_the_start_of_the_single_fit(partls, recorder):
    X, y, P = _problem()
    X32 = X.astype(np.float32)                     # a staged single fit: prepare + alt_prepared on the context
    partls.fit(partls.Alt, X32, y, P, rng=9)
    partls.fit(partls.Alt, X32, y, P, rng=9, restarts=3)
    assert [c[0] for c in recorder.calls] == ["opt_prepare", "alt_prepared", "opt_prepare", "alt_multistart"]
    assert np.array_equal(recorder.calls[3][1][0], recorder.calls[1][1])
    assert np.array_equal(recorder.calls[3][2][0], recorder.calls[1][2])


def test_explicit_starts_reach_the_context_unchanged(partls, recorder):
    X, y, P = _problem()
    a0 = np.random.default_rng(1).random((3, M + 1))
    b0 = np.random.default_rng(2).random((3, K + 1)) - 0.5
    for restarts in (None, 3):
        recorder.calls.clear()
        partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0, restarts=restarts)
        assert [c[0] for c in recorder.calls] == ["opt_prepare", "alt_multistart"]
        assert np.array_equal(recorder.calls[1][1], a0) and np.array_equal(recorder.calls[1][2], b0)
    # restarts=1 is a batch of one, not the single path
    recorder.calls.clear()
    partls.fit(partls.Alt, X, y, P, restarts=1, rng=3)
    assert recorder.calls[1][0] == "alt_multistart" and recorder.calls[1][1].shape == (1, M + 1)


def test_float32_matrix_and_weights_reach_the_prepare(partls, recorder):
    X, y, P = _problem()
    w = np.arange(1, 13, dtype=np.float32)
    partls.fit(partls.Alt, X.astype(np.float32), y, P, restarts=2, rng=0, weights=w)
    what, Xg, flags, wg = recorder.calls[0]
    assert what == "opt_prepare" and Xg.dtype == np.float32 and Xg.flags.f_contiguous
    assert wg.dtype == np.float64 and np.array_equal(wg, w.astype(np.float64))
    recorder.calls.clear()
    partls.fit(partls.Alt, X, y, P, restarts=2, rng=0)
    assert recorder.calls[0][1].dtype == np.float64 and recorder.calls[0][3] is None


def test_context_checks_the_shapes_of_its_starts(partls):
    ctx = partls.Context.__new__(partls.Context)          # no device: the shapes are checked before anything is called
    ctx._h, ctx.generation, ctx._shape = C.c_void_p(), 0, (12, M, K)
    for a0, b0 in ((np.ones(M + 1), np.ones(K + 1)), (np.ones((2, M)), np.ones((2, K + 1))), (np.ones((2, M + 1)), np.ones((3, K + 1))),
                   (np.ones((0, M + 1)), np.ones((0, K + 1)))):
        with pytest.raises(ValueError):
            ctx.alt_multistart(a0, b0)
