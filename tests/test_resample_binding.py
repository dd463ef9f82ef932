"""CPU checks of bootstrap / resample: partls_opt_weightings is declared by the header, exported by the library and
bound by the ctypes table; every TypeError / ValueError of bootstrap and resample is raised before any device work; bootstrap's counts
are the documented draw; the binding makes one library call with W column-major (against the fake library of tools/api_call_trace.py);
the statistics of a BootstrapResult on a hand-made table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import api_call_trace as T  # noqa: E402
import check_julia_binding as CJ  # noqa: E402


def _problem(N=12):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(N, 3))
    y = rng.normal(size=N)
    P = np.array([[1, 0], [1, 0], [0, 1]])
    return X, y, P


def _no_device(*a, **k):
    raise AssertionError("device work started before the arguments were checked")


def test_symbol_in_header_library_and_table(partls):
    protos = CJ.parse_header()
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS}
    partls.lowlevel.lib()              # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    s = "partls_opt_weightings"
    assert s in protos and s in table and hasattr(lib, s)
    assert len(protos[s][1]) == len(table[s][1]) == 25
    assert protos[s][1][10:15] == ["double*", "int64_t", "int64_t", "double", "uint32_t"]       # W, ldW, B, eta, flags
    assert partls.lowlevel.T_OOB == 5
    assert partls.lowlevel.lib().partls_version() >= 104
    for name in ("bootstrap", "resample", "BootstrapResult"):
        assert hasattr(partls, name) and name in partls.__all__
    assert hasattr(partls.Context, "opt_weightings")


BAD_WEIGHTS = [
    ("negative", lambda N: np.r_[np.ones(N - 1), -1.0]),
    ("nan", lambda N: np.r_[np.ones(N - 1), np.nan]),
    ("inf", lambda N: np.r_[np.ones(N - 1), np.inf]),
    ("short", lambda N: np.ones(N - 1)),
    ("matrix", lambda N: np.ones((N, 1))),
    ("all_zero", lambda N: np.zeros(N)),
    ("integer", lambda N: np.ones(N, dtype=np.int64)),
]


@pytest.mark.parametrize("name,make", BAD_WEIGHTS, ids=[b[0] for b in BAD_WEIGHTS])
def test_bootstrap_bad_weights_raise_before_device_work(partls, monkeypatch, name, make):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    X, y, P = _problem()
    with pytest.raises(ValueError):
        partls.bootstrap(partls.Opt, X, y, P, B=4, rng=1, weights=make(len(y)))


@pytest.mark.parametrize("B", [0, -3, 2.0, 2.5, "4", None, True])
def test_bootstrap_bad_B_raises_before_device_work(partls, monkeypatch, B):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    X, y, P = _problem()
    with pytest.raises(ValueError):
        partls.bootstrap(partls.Opt, X, y, P, B=B, rng=1)


def test_other_algorithms_and_arguments_raise_before_device_work(partls, monkeypatch):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    X, y, P = _problem()
    W = np.ones((len(y), 2))
    for alg in (partls.Alt, partls.BnB, object):
        with pytest.raises(TypeError):
            partls.bootstrap(alg, X, y, P, B=2)
        with pytest.raises(TypeError):
            partls.resample(alg, X, y, P, W)
    with pytest.raises(TypeError):
        partls.bootstrap(partls.Opt, X, y, P, B=2, devices=2)            # devices= is not an argument
    with pytest.raises(TypeError):
        partls.resample(partls.Opt, X, y, P, W, devices=2)
    with pytest.raises(ValueError):
        partls.bootstrap(partls.Opt, X, y, P, B=2, on_ill_conditioned="ignore")
    with pytest.raises(TypeError):
        partls.bootstrap(partls.Opt, X.astype(int), y, P, B=2)
    with pytest.raises(ValueError):
        partls.bootstrap(partls.Opt, X, y[:-1], P, B=2)


BAD_W = [
    ("negative", lambda N: np.c_[np.ones(N), np.r_[np.ones(N - 1), -1.0]]),
    ("nan", lambda N: np.c_[np.ones(N), np.r_[np.ones(N - 1), np.nan]]),
    ("inf", lambda N: np.c_[np.r_[np.inf, np.ones(N - 1)], np.ones(N)]),
    ("zero_column", lambda N: np.c_[np.ones(N), np.zeros(N)]),
    ("short", lambda N: np.ones((N - 1, 2))),
    ("vector", lambda N: np.ones(N)),
    ("no_columns", lambda N: np.ones((N, 0))),
    ("integer", lambda N: np.ones((N, 2), dtype=np.int64)),
]


@pytest.mark.parametrize("name,make", BAD_W, ids=[b[0] for b in BAD_W])
def test_resample_bad_W_raises_before_device_work(partls, monkeypatch, name, make):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    X, y, P = _problem()
    with pytest.raises(ValueError):
        partls.resample(partls.Opt, X, y, P, make(len(y)))


def test_the_binding_marshals_one_library_call(partls):
    """against the fake library of tools/api_call_trace.py: one partls_opt_weightings call per Python call, W column-major with ldW = N,
    a float32 X widened on the host, oob=False as a NULL oob_sse, bootstrap / resample through the default context"""
    X, y, P = _problem()
    N = len(y)
    W = np.arange(1.0, 3 * N + 1).reshape(N, 3)                          # C-ordered: copied column-major
    calls = lambda f: [ln for ln in f.lines if ln.startswith("partls_opt_weightings(")]      # noqa: E731
    with T.fake_library(partls.api) as fake:
        ctx = partls.Context(0)
        r = ctx.opt_weightings(X, y, P, W, 0.25, 1)
        line, = calls(fake)
        for part in ("N=12", "M=3", "ldX=12", "dev=0", "K=2", "ldP=3", "ldW=12", "B=3", "eta=0.25", "flags=1", "ld_alpha=3", "ld_beta=2"):
            assert part in line.replace(", ", " ").split(), (part, line)
        assert "NULL" not in line and line.endswith("-> 0")
        assert r["alpha"].shape == (3, 3) and r["beta"].shape == (2, 3) and r["oob_rows"].dtype == np.int64 and r["status"].dtype == np.int32
        ctx.opt_weightings(X.astype(np.float32).astype(np.float64), y, P, np.asfortranarray(W), 0.25, 1)
        ctx.opt_weightings(X.astype(np.float32), y, P, W, 0.25, 1)
        a, b, c = calls(fake)
        assert a != b and "X[36]=" in c                                 # another X (rounded through float32), 36 doubles
        assert b == c                                                   # the float32 X went up as float64, W in the same layout
        skipped = ctx.opt_weightings(X, y, P, W, oob=False)
        assert calls(fake)[-1].count("NULL") == 1 and np.all(np.isnan(skipped["oob_sse"]))
        with pytest.raises(ValueError):
            ctx.opt_weightings(X, y, P, W[:-1])
        with pytest.raises(ValueError):
            ctx.opt_weightings(X, y, P[:2], W)
        n = len(calls(fake))
        res = partls.bootstrap(partls.Opt, X, y, P, B=5, rng=1, generic_kernel=True)
        assert len(calls(fake)) == n + 1 and "B=5" in calls(fake)[-1] and "flags=2" in calls(fake)[-1]
        assert res.counts.shape == (N, 5) and res.alpha.shape == (5, 3) and len(res.models) == 5
        with fake.scripted(partls_opt_weightings=1):
            with pytest.raises(partls.PartlsError) as ei:
                partls.resample(partls.Opt, X, y, P, np.ones((N, 2)))
            assert ei.value.status == 1


class _Recorder:
    """stands in for the default context: keeps the W it is handed and returns a table of the right shapes"""

    def __init__(self):
        self.W = None

    def opt_weightings(self, X, y, P, W, eta, flags):
        self.W, self.eta, self.flags = np.array(W), eta, flags
        B, (M, K) = W.shape[1], P.shape
        return dict(alpha=np.ones((M, B), order="F"), beta=np.ones((K, B), order="F"), t=np.zeros(B), opt=np.ones(B),
                    best_index=np.zeros(B, dtype=np.int64), status=np.zeros(B, dtype=np.int32), oob_sse=np.ones(B),
                    oob_rows=(self.W == 0).sum(0).astype(np.int64))


def test_bootstrap_counts_are_the_documented_draw(partls, monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(partls.api, "default_context", lambda device=0: rec)
    N, B = 40, 7
    X, y, P = _problem(N)
    res = partls.bootstrap(partls.Opt, X, y, P, B=B, rng=123, η=0.25, faithful_intercept=True)
    want = np.random.default_rng(123).multinomial(N, np.full(N, 1 / N), size=B).T
    assert res.counts.dtype == np.int64 and res.counts.shape == (N, B)
    assert np.array_equal(res.counts, want) and np.all(res.counts.sum(0) == N)
    assert np.array_equal(rec.W, want.astype(float)) and rec.W.dtype == np.float64
    assert rec.eta == 0.25 and rec.flags == partls.lowlevel.OPT_FAITHFUL_INTERCEPT
    # a Generator is used as it is; weights scale the counts row by row
    w = np.linspace(0.5, 2.0, N)
    res2 = partls.bootstrap(partls.Opt, X, y, P, B=B, rng=np.random.default_rng(123), weights=w)
    assert np.array_equal(res2.counts, want) and np.array_equal(rec.W, want * w[:, None])
    assert res2.alpha.shape == (B, 3) and res2.beta.shape == (B, 2) and len(res2.models) == B
    res3 = partls.resample(partls.Opt, X, y, P, want.astype(float))
    assert res3.counts is None and np.array_equal(rec.W, want.astype(float))
    assert np.array_equal(res3.oob_rows, (want == 0).sum(0))


def test_bootstrap_result_statistics_on_a_hand_made_table(partls):
    #           beta_0  beta_1        status
    beta = np.array([[1.0, -2.0],   # 0
                     [2.0, 0.0],    # 0
                     [3.0, 1.0],    # 9: counts
                     [np.nan, np.nan],  # 6: does not count
                     [-1.0, -4.0]])  # 0
    alpha = np.array([[0.1, 0.9], [0.2, 0.8], [0.3, 0.7], [np.nan, np.nan], [0.4, 0.6]])
    t = np.array([1.0, 2.0, 3.0, np.nan, 4.0])
    res = partls.BootstrapResult(counts=None, alpha=alpha, beta=beta, t=t, opt=np.array([1.0, 1, 1, np.nan, 1]),
                                 best_index=np.array([2, 0, 2, -1, 3]), models=[object()] * 3 + [None, object()],
                                 status=np.array([0, 0, 9, 6, 0], dtype=np.int32),
                                 oob_sse=np.array([4.0, np.nan, 6.0, np.nan, 2.0]), oob_rows=np.array([2, 0, 3, 5, 1]))
    assert np.array_equal(res.ok, [True, True, True, False, True])
    assert np.array_equal(res.ill_conditioned, [False, False, True, False, False])
    assert np.array_equal(res.sign_frequency, [[0.25, 0.0, 0.75], [0.5, 0.25, 0.25]])
    assert np.allclose(res.sign_frequency.sum(1), 1.0)
    assert res.pattern_frequency == {2: 0.5, 0: 0.25, 3: 0.25}
    assert res.oob_mse == (4.0 + 6.0 + 2.0) / (2 + 3 + 1)
    iv = res.interval(0.5)
    ok = res.ok
    for k, v in (("alpha", alpha), ("beta", beta)):
        lo, hi = iv[k]
        assert np.allclose(lo, np.percentile(v[ok], 25, axis=0)) and np.allclose(hi, np.percentile(v[ok], 75, axis=0))
        assert np.all(lo <= np.median(v[ok], axis=0)) and np.all(np.median(v[ok], axis=0) <= hi)
    assert iv["t"] == (1.75, 3.25)
    full = res.interval()
    assert np.allclose(full["beta"][0], np.percentile(beta[ok], 2.5, axis=0)) and np.allclose(full["beta"][1], np.percentile(beta[ok], 97.5, axis=0))
    for bad in (0.0, 1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            res.interval(bad)
    none = partls.BootstrapResult(counts=None, alpha=alpha[3:4], beta=beta[3:4], t=t[3:4], opt=t[3:4], best_index=np.array([-1]), models=[None],
                                  status=np.array([6], dtype=np.int32), oob_sse=np.array([np.nan]), oob_rows=np.array([4]))
    assert np.isnan(none.oob_mse) and none.pattern_frequency == {} and np.all(np.isnan(none.sign_frequency))
    with pytest.raises(ValueError):
        none.interval()
