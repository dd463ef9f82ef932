"""CPU checks of the cross-validated multistart fit(Alt): partls_cv_alt is declared by the header, exported by the
library, bound by the ctypes table with the same parameter count and called by the Julia drop-in; cross_validate(Alt, ...) rejects
every misuse before any device work, draws its starts after the fold permutation from the one generator, and hands the context
the same starts whatever the η grid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_julia_binding as CJ  # noqa: E402

SYM = "partls_cv_alt"
NPARAM = 36


def test_symbol_in_header_library_and_table(partls):
    protos = CJ.parse_header()
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS}
    partls.lowlevel.lib()              # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    assert SYM in protos and SYM in table and hasattr(lib, SYM)
    assert protos[SYM][0] == "partls_status"
    assert len(protos[SYM][1]) == len(table[SYM][1]) == NPARAM
    assert protos[SYM][1][-3:] == ["double*", "int64_t*", "int32_t*"]                  # opt_all, iters_all, status_all
    assert partls.lowlevel.lib().partls_version() >= 105


def test_integration_calls_the_entry_point():
    calls = {c[0]: c for c in CJ.parse_ccalls()}
    checked = {s for s, _ in CJ.check()}
    assert SYM in calls and SYM in checked
    assert len(calls[SYM][2]) == NPARAM
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "_fit_alt_julia" in text[text.index("## 3b."):text.index("ccall((:" + SYM)]     # the stock-Julia fallback


M, K, N = 3, 2, 12


def _problem():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(N, M))
    y = rng.normal(size=N)
    P = np.array([[1, 0], [1, 0], [0, 1]])
    return X, y, P


def _no_device(*a, **k):
    raise AssertionError("device work started before the arguments were checked")


BAD = [
    ("restarts_with_1d_starts", dict(restarts=2, alpha0=np.ones(M + 1), beta0=np.ones(K + 1))),
    ("single_start", dict(alpha0=np.ones(M + 1), beta0=np.ones(K + 1))),
    ("restarts_zero", dict(restarts=0)),
    ("restarts_not_an_integer", dict(restarts=2.5)),
    ("restarts_disagrees_with_the_rows", dict(restarts=3, alpha0=np.ones((2, M + 1)), beta0=np.ones((2, K + 1)))),
    ("row_counts_differ", dict(alpha0=np.ones((2, M + 1)), beta0=np.ones((3, K + 1)))),
    ("alpha0_too_narrow", dict(alpha0=np.ones((2, M)), beta0=np.ones((2, K + 1)))),
    ("only_alpha0", dict(alpha0=np.ones((2, M + 1)))),
    ("nan_start", dict(alpha0=np.ones((2, M + 1)), beta0=np.array([[1.0, np.nan, 1.0], [1.0, 1.0, 1.0]]))),
    ("one_fold", dict(restarts=2, nfolds=1)),
    ("more_folds_than_rows", dict(restarts=2, nfolds=N + 1)),
    ("negative_weight", dict(restarts=2, weights=-np.ones(N))),
]


@pytest.mark.parametrize("name,kw", BAD, ids=[b[0] for b in BAD])
def test_misuse_raises_before_device_work(partls, monkeypatch, name, kw):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    X, y, P = _problem()
    with pytest.raises(ValueError):
        partls.cross_validate(partls.Alt, X, y, P, η=[0.0, 1.0], **kw)


@pytest.mark.parametrize("kw", [dict(restarts=4), dict(alpha0=np.ones((2, M + 1)), beta0=np.ones((2, K + 1)))], ids=["restarts", "starts"])
def test_starts_are_an_option_of_alt_only(partls, monkeypatch, kw):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    X, y, P = _problem()
    with pytest.raises(ValueError):
        partls.cross_validate(partls.Opt, X, y, P, **kw)
    with pytest.raises(TypeError):
        partls.cross_validate(partls.BnB, X, y, P, **kw)


class _Recorder:
    """stands in for the default context: records what cv_alt is given, computes nothing"""

    def __init__(self):
        self.calls = []

    def cv_alt(self, X, y, P, fold_ptr, etas, a0, b0, eps=1e-6, T=100, device_ptrs=None, weights=None, flags=0):
        self.calls.append(dict(X=X, y=y, fold_ptr=fold_ptr, etas=etas, a0=a0, b0=b0, eps=eps, T=T, weights=weights, flags=flags))
        F = 0 if fold_ptr is None else len(fold_ptr) - 1
        E, R, Mm, Kk = len(etas), len(a0), P.shape[0], P.shape[1]
        B = (F + 1) * E
        sse = np.tile(np.arange(E, 0, -1, dtype=float), F + 1)           # the last η has the smallest held-out error
        return dict(alpha=np.zeros((Mm, B), order="F"), beta=np.zeros((Kk, B), order="F"), t=np.zeros(B), opt=np.ones(B),
                    iters=np.full(B, 3, dtype=np.int64), best_start=np.ones(B, dtype=np.int64), heldout_sse=sse,
                    status=np.zeros(B, dtype=np.int32), F=F, E=E,
                    starts=dict(opt=np.ones((B, R)), iters=np.ones((B, R), dtype=np.int64), status=np.zeros((B, R), dtype=np.int32)))


@pytest.fixture
def recorder(partls, monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(partls.api, "default_context", lambda device=0: r)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    return r


def test_starts_are_drawn_after_the_permutation(partls, recorder):
    X, y, P = _problem()
    seed, R = 41, 5
    res = partls.cross_validate(partls.Alt, X, y, P, η=[0.0, 0.5, 2.0], nfolds=3, shuffle=True, rng=seed, restarts=R, ϵ=1e-4, T=7)
    call = recorder.calls[0]
    gen = np.random.default_rng(seed)
    perm = gen.permutation(N)
    assert np.array_equal(res.perm, perm) and np.array_equal(call["X"], X[perm]) and np.array_equal(call["y"], y[perm])
    assert call["a0"].shape == (R, M + 1) and call["b0"].shape == (R, K + 1) and (call["eps"], call["T"]) == (1e-4, 7)
    for r in range(R):
        assert np.array_equal(call["a0"][r], gen.random(M + 1))
        assert np.array_equal(call["b0"][r], (gen.random(K + 1) - 0.5) * 10)
    # a Generator is consumed in the same way; without shuffle the draws are the generator's first
    recorder.calls.clear()
    partls.cross_validate(partls.Alt, X, y, P, nfolds=3, shuffle=True, rng=np.random.default_rng(seed), restarts=2)
    assert np.array_equal(recorder.calls[0]["a0"], call["a0"][:2]) and np.array_equal(recorder.calls[0]["b0"], call["b0"][:2])
    recorder.calls.clear()
    partls.cross_validate(partls.Alt, X, y, P, nfolds=3, rng=seed, restarts=1)
    assert np.array_equal(recorder.calls[0]["a0"][0], np.random.default_rng(seed).random(M + 1))


def test_the_same_starts_whatever_the_grid(partls, recorder):
    X, y, P = _problem()
    for grid in ([0.0], [0.0, 1.0, 10.0], None):
        partls.cross_validate(partls.Alt, X, y, P, η=grid, nfolds=2, rng=9, restarts=4)
    a, b, c = recorder.calls
    assert np.array_equal(a["a0"], b["a0"]) and np.array_equal(a["b0"], b["b0"])
    assert np.array_equal(a["a0"], c["a0"]) and np.array_equal(a["b0"], c["b0"])
    assert list(b["etas"]) == [0.0, 1.0, 10.0] and list(c["etas"]) == [0.0]


def test_default_is_32_starts_and_explicit_starts_pass_unchanged(partls, recorder):
    X, y, P = _problem()
    partls.cross_validate(partls.Alt, X, y, P, nfolds=2, rng=1)
    assert recorder.calls[0]["a0"].shape == (32, M + 1)
    a0 = np.random.default_rng(1).random((3, M + 1))
    b0 = np.random.default_rng(2).random((3, K + 1)) - 0.5
    for restarts in (None, 3):
        recorder.calls.clear()
        partls.cross_validate(partls.Alt, X, y, P, nfolds=2, alpha0=a0, beta0=b0, restarts=restarts)
        assert np.array_equal(recorder.calls[0]["a0"], a0) and np.array_equal(recorder.calls[0]["b0"], b0)


def test_result_fields(partls, recorder):
    X, y, P = _problem()
    w = np.arange(1, N + 1, dtype=np.float64)
    res = partls.cross_validate(partls.Alt, X.astype(np.float32), y, P, η=[0.0, 1.0], nfolds=3, restarts=4, rng=0, weights=w)
    call = recorder.calls[0]
    assert call["X"].dtype == np.float64 and np.array_equal(call["weights"], w)       # a float32 X is widened on the host, as for Opt
    assert res.best_index is None and res.best_index_eta == 1 and res.model is res.path[1]
    assert res.iters.shape == res.best_start.shape == res.opt.shape == (4, 2)
    assert set(res.starts) == {"opt", "iters", "status"} and res.starts.opt.shape == (4, 2, 4)
    assert res.mse_mean.shape == (2,) and np.allclose(res.mse_mean, np.array([6.0, 3.0]) / w.sum())


def test_opt_result_has_no_alt_fields(partls, monkeypatch):
    class Ctx:
        def cv_opt(self, X, y, P, fold_ptr, etas, flags=0, device_ptrs=None, weights=None):
            B = len(fold_ptr) * len(etas)
            return dict(alpha=np.zeros((M, B), order="F"), beta=np.zeros((K, B), order="F"), t=np.zeros(B), opt=np.ones(B),
                        best_index=np.zeros(B, dtype=np.int64), heldout_sse=np.ones(B), status=np.zeros(B, dtype=np.int32))
    monkeypatch.setattr(partls.api, "default_context", lambda device=0: Ctx())
    X, y, P = _problem()
    res = partls.cross_validate(partls.Opt, X, y, P, η=[0.0, 1.0], nfolds=2)
    assert res.best_index.shape == (3, 2) and res.iters is None and res.best_start is None and res.starts is None


def test_context_checks_the_shapes_of_its_starts(partls):
    ctx = partls.Context.__new__(partls.Context)          # no device: the shapes are checked before anything is called
    ctx._h, ctx.generation = C.c_void_p(), 0
    X, y, P = _problem()
    for a0, b0 in ((np.ones(M + 1), np.ones(K + 1)), (np.ones((2, M)), np.ones((2, K + 1))), (np.ones((2, M + 1)), np.ones((3, K + 1)))):
        with pytest.raises(ValueError):
            ctx.cv_alt(X, y, P, [0, 6, 12], [0.0], a0, b0)
