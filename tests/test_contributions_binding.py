"""CPU checks of the group contributions against the fake library of tools/api_call_trace.py: the two entry points are
declared (include/partls_contrib.h, which include/partls.h includes), exported, bound in a table of their own with the same argument
types and called by the Julia patch; every public function makes the one call it should and keeps float32 as float32;
group_importance asks for the sums alone and BootstrapResult.contributions for at most four ranks and the mean; bad arguments are
refused before any call; and BootstrapResult.predict returns what it returned before its band helper was shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import api_call_trace as T  # noqa: E402
import check_julia_binding as CJ  # noqa: E402

NAMES = ("h", "X", "N", "M", "ldX", "dev", "P", "K", "ldP", "B", "alpha", "lda", "beta", "ldb", "contrib", "ldC", "nr", "ranks", "stats",
         "mean", "sums")
NARGS = 21
SYMS = ("partls_contributions", "partls_contributions_f32")


def test_symbols_in_header_library_table_and_julia(partls):
    protos = CJ.parse_header(CJ.CONTRIB_HEADER)
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS_CONTRIB}
    assert set(protos) == set(table) == set(SYMS)
    assert not set(SYMS) & set(CJ.parse_header())                        # not in the main header's own list ...
    assert '#include "partls_contrib.h"' in open(os.path.join(ROOT, "include", "partls.h")).read()     # ... which includes theirs
    assert set(SYMS) <= set(CJ.parse_headers())
    partls.lowlevel.lib()                      # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    want = ["partls_ctx*", "double*", "int64_t", "int64_t", "int64_t", "int", "int64_t*", "int64_t", "int64_t", "int64_t", "double*",
            "int64_t", "double*", "int64_t", "double*", "int64_t", "int64_t", "int64_t*", "double*", "double*", "double*"]
    assert len(want) == len(NAMES) == NARGS
    for name in SYMS:
        assert hasattr(lib, name), name
        ret, params = protos[name]
        assert ret == "partls_status" and len(params) == len(table[name][1]) == NARGS, name
        assert params == want[:1] + ["float*" if name.endswith("f32") else "double*"] + want[2:], name
        assert table[name][0] is C.c_int
    assert table[SYMS[0]][1] == table[SYMS[1]][1]
    assert partls.lowlevel.lib().partls_version() >= 108
    calls = {c[0] for c in CJ.parse_ccalls()}
    checked = {s for s, _ in CJ.check()}
    assert "partls_contributions" in calls and "partls_contributions" in checked
    for name in ("contributions", "contributions_many", "group_importance"):
        assert name in partls.__all__ and getattr(partls, name) is getattr(partls.api, name)
    text = open(os.path.join(ROOT, "include", "partls_contrib.h")).read()
    assert "#define PARTLS_CONTRIB_CHUNK %d" % partls.lowlevel.CONTRIB_CHUNK in text


# ---- a fake device: records what a call was handed and writes what a device would -------------------------------------------------------
def _doubles(arg, n):
    return np.ctypeslib.as_array((C.c_double * n).from_address(T._addr(arg)))


class _Device:
    """wraps the fake library's two contributions symbols: every call is recorded (scalars by value, the model arrays as copies, the
    addresses of X and of the outputs) and the host outputs are written from Cube[N, K, B], the contributions this 'device' computes"""

    def __init__(self, fake, cube=None):
        self.calls, self.cube = [], cube
        for name in SYMS:
            setattr(fake, name, self._wrap(name, getattr(fake, name)))

    def _wrap(self, name, inner):
        def call(*args):
            assert len(args) == NARGS
            status = inner(*args)
            a = dict(zip(NAMES, args))
            N, M, K, B, nr, lda, ldb = (int(a[k]) for k in ("N", "M", "K", "B", "nr", "lda", "ldb"))
            rec = dict(symbol=name, N=N, M=M, K=K, B=B, nr=nr, lda=lda, ldb=ldb, ldX=int(a["ldX"]), ldP=int(a["ldP"]), ldC=int(a["ldC"]),
                       dev=int(a["dev"]), alpha=_doubles(a["alpha"], lda * B).copy(), beta=_doubles(a["beta"], ldb * B).copy(),
                       ranks=None if not T._addr(a["ranks"]) else np.ctypeslib.as_array((C.c_int64 * nr).from_address(T._addr(a["ranks"]))).copy(),
                       **{k: T._addr(a[k]) for k in ("X", "contrib", "stats", "mean", "sums")})
            if not rec["dev"]:
                xt = C.c_float if name.endswith("f32") else C.c_double
                rec["Xvalues"] = np.ctypeslib.as_array((xt * (rec["ldX"] * M)).from_address(rec["X"])).copy()
            self.calls.append(rec)
            if self.cube is not None and not rec["dev"]:
                cube = np.asarray(self.cube, dtype=np.float64)
                assert cube.shape == (N, K, B)
                if rec["contrib"]:
                    _doubles(a["contrib"], rec["ldC"] * K * B).reshape(B, K, rec["ldC"])[:, :, :N] = cube.transpose(2, 1, 0)
                if rec["stats"]:
                    _doubles(a["stats"], N * K * nr).reshape(nr, K, N)[:] = np.sort(cube, axis=2)[:, :, rec["ranks"]].transpose(2, 1, 0)
                if rec["mean"]:
                    mu = np.array([[sum(cell) / B for cell in row] for row in cube.tolist()])
                    _doubles(a["mean"], N * K).reshape(K, N)[:] = mu.T
                if rec["sums"]:
                    s = np.stack([cube.sum(0), np.abs(cube).sum(0), (cube * cube).sum(0)])          # [3, K, B]
                    _doubles(a["sums"], 3 * K * B).reshape(B, K, 3)[:] = s.transpose(2, 1, 0)
            return status
        return call


@pytest.fixture
def fake(partls):
    with T.fake_library(partls.api) as f:
        yield f


P3 = np.array([[1, 0], [1, 0], [0, 1]])


def _models(B, M=3, K=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(B, M)), rng.normal(size=(B, K)), rng.normal(size=B), P3


def _result(partls, B, bad=(), seed=0):
    """a BootstrapResult of B replicates over M = 3, K = 2; the replicates in `bad` hit the pivot cap (status 6, NaN rows)"""
    a, b, t, P = _models(B, seed=seed)
    status = np.zeros(B, dtype=np.int32)
    for j in bad:
        status[j] = partls.lowlevel.ERR_NOT_CONVERGED
        a[j] = b[j] = t[j] = np.nan
    models = [None if status[j] else partls.PartLSFitResult(a[j], b[j], float(t[j]), P) for j in range(B)]
    return partls.BootstrapResult(counts=None, alpha=a, beta=b, t=t, opt=np.zeros(B), best_index=np.zeros(B, dtype=np.int64), models=models,
                                  status=status, oob_sse=np.zeros(B), oob_rows=np.zeros(B, dtype=np.int64), P=P)


def test_context_hands_over_the_layouts_of_the_abi(partls, fake):
    dev = _Device(fake)
    a, b, _, P = _models(4)
    X = np.random.default_rng(1).normal(size=(5, 3))                      # C-ordered: goes over as a column-major copy
    ctx = partls.Context(0)
    out = ctx.contributions(X, P, a, b)
    c = dev.calls[-1]
    assert c["symbol"] == "partls_contributions" and (c["N"], c["M"], c["K"], c["B"], c["dev"]) == (5, 3, 2, 4, 0)
    assert (c["ldX"], c["ldP"], c["lda"], c["ldb"], c["ldC"], c["nr"]) == (5, 3, 3, 2, 5, 0)
    assert np.array_equal(c["Xvalues"], X.T.ravel())
    assert np.array_equal(c["alpha"], a.ravel()) and np.array_equal(c["beta"], b.ravel())          # M x B, K x B: model b = column b
    assert c["contrib"] and not c["stats"] and not c["mean"] and not c["sums"] and c["ranks"] is None
    assert out["contrib"].shape == (5, 2, 4) and out["contrib"].flags.f_contiguous
    assert out["stats"] is None and out["mean"] is None and out["sums"] is None
    # statistics only, float32 stays float32
    out = ctx.contributions(X.astype(np.float32), P, a, b, ranks=[3, 0], want_contrib=False, want_mean=True, want_sums=True)
    c = dev.calls[-1]
    assert c["symbol"] == "partls_contributions_f32" and np.array_equal(c["Xvalues"], X.astype(np.float32).T.ravel())
    assert not c["contrib"] and c["stats"] and c["mean"] and c["sums"] and c["nr"] == 2 and c["ranks"].tolist() == [3, 0]
    assert out["contrib"] is None and out["stats"].shape == (5, 2, 2) and out["mean"].shape == (5, 2) and out["sums"].shape == (3, 2, 4)
    assert all(out[k].flags.f_contiguous for k in ("stats", "mean", "sums"))
    # device pointers pass through as they are; the sums come back on the host
    got = ctx.contributions_device(0x7f0000001000, 5, 3, 8, P, a, b, dcontrib_ptr=0x7f0000002000, ldC=6, dtype=np.float32)
    c = dev.calls[-1]
    assert got is None and c["symbol"] == "partls_contributions_f32"
    assert (c["X"], c["contrib"], c["stats"], c["mean"], c["sums"]) == (0x7f0000001000, 0x7f0000002000, 0, 0, 0)
    assert (c["dev"], c["ldX"], c["ldC"], c["nr"]) == (1, 8, 6, 0)
    got = ctx.contributions_device(0x7f0000001000, 5, 3, 8, P, a, b, ranks=[1], dstats_ptr=0x7f0000003000, dmean_ptr=0x7f0000004000, want_sums=True)
    c = dev.calls[-1]
    assert c["symbol"] == "partls_contributions" and (c["contrib"], c["stats"], c["mean"], c["nr"]) == (0, 0x7f0000003000, 0x7f0000004000, 1)
    assert got.shape == (3, 2, 4) and c["sums"] == got.ctypes.data
    ctx.close()


def test_public_functions_take_models_or_arrays(partls, fake):
    a, b, t, P = _models(5)
    X = np.random.default_rng(2).normal(size=(6, 3))
    cube = np.random.default_rng(3).normal(size=(6, 2, 5))
    dev = _Device(fake, cube)
    models = [partls.PartLSFitResult(a[j], b[j], float(t[j]), P.copy()) for j in range(5)]
    for arg in (models, tuple(models), (a, b, t, P)):
        got = partls.contributions_many(arg, X)
        assert got.dtype == np.float64 and got.shape == (6, 2, 5) and np.array_equal(got, cube)
        c = dev.calls[-1]
        assert np.array_equal(c["alpha"], a.ravel()) and np.array_equal(c["beta"], b.ravel())
        assert c["symbol"] == "partls_contributions" and c["contrib"] and not c["stats"] and not c["mean"] and not c["sums"]
    partls.contributions_many(models, X.astype(np.float32))
    assert dev.calls[-1]["symbol"] == "partls_contributions_f32"
    dev.cube = cube[:, :, :1]
    one = partls.contributions(models[0], X)
    c = dev.calls[-1]
    assert one.shape == (6, 2) and one.dtype == np.float64 and np.array_equal(one, cube[:, :, 0]) and c["B"] == 1
    assert np.array_equal(c["alpha"], a[0]) and np.array_equal(c["beta"], b[0])
    partls.contributions(models[0], X.astype(np.float32))
    assert dev.calls[-1]["symbol"] == "partls_contributions_f32"


def test_group_importance_asks_for_the_sums_alone(partls, fake):
    a, b, t, P = _models(5)
    X = np.random.default_rng(4).normal(size=(7, 3))
    cube = np.random.default_rng(5).normal(size=(7, 2, 5))
    cube[:, 1, 2] = 0.0                                                    # model 2: group 1 contributes nothing
    cube[:, :, 3] = 0.0                                                    # model 3: nothing at all -> its shares are NaN
    dev = _Device(fake, cube)
    n0 = len(dev.calls)
    rep = partls.group_importance((a, b, t, P), X)
    assert len(dev.calls) == n0 + 1
    c = dev.calls[-1]
    assert c["sums"] and not c["contrib"] and not c["stats"] and not c["mean"] and c["nr"] == 0 and c["B"] == 5
    assert set(rep) == {"mean", "mean_abs", "rms", "share"} and all(rep[k].shape == (5, 2) for k in rep)
    assert np.allclose(rep.mean, cube.mean(0).T, rtol=1e-14, atol=0) and np.allclose(rep.mean_abs, np.abs(cube).mean(0).T, rtol=1e-14, atol=0)
    assert np.allclose(rep.rms, np.sqrt((cube ** 2).mean(0)).T, rtol=1e-14, atol=0)
    ok = [0, 1, 2, 4]
    assert np.allclose(rep.share[ok].sum(1), 1.0, rtol=1e-14) and rep.share[2, 1] == 0.0 and rep.share[2, 0] == 1.0
    assert np.all(np.isnan(rep.share[3]))
    # one model: vectors of K; float32 stays float32
    dev.cube = cube[:, :, :1]
    rep1 = partls.group_importance(partls.PartLSFitResult(a[0], b[0], 0.0, P), X.astype(np.float32))
    c = dev.calls[-1]
    assert c["symbol"] == "partls_contributions_f32" and c["B"] == 1 and c["sums"] and not c["contrib"]
    assert all(rep1[k].shape == (2,) for k in rep1) and np.array_equal(rep1.mean_abs, rep.mean_abs[0])
    # a bootstrap result: its successful replicates
    dev.cube = cube[:, :, :3]
    rep2 = partls.group_importance(_result(partls, 5, bad=(1, 3)), X)
    c = dev.calls[-1]
    assert c["B"] == 3 and np.all(np.isfinite(c["alpha"])) and rep2.share.shape == (3, 2)


def test_bootstrap_band_asks_for_four_ranks_and_the_mean(partls, fake):
    dev = _Device(fake, None)
    X = np.zeros((4, 3))
    _result(partls, 100).contributions(X, level=0.95)
    c = dev.calls[-1]
    assert c["ranks"].tolist() == [2, 3, 96, 97] and c["B"] == 100 and not c["contrib"] and c["stats"] and c["mean"] and not c["sums"]
    _result(partls, 5).contributions(X, level=0.5)
    assert dev.calls[-1]["ranks"].tolist() == [1, 3]
    _result(partls, 1).contributions(X, level=0.9)
    assert dev.calls[-1]["ranks"].tolist() == [0]
    res = _result(partls, 7, bad=(1, 4))
    cube = np.random.default_rng(6).normal(size=(4, 2, 5))
    dev.cube = cube
    out = res.contributions(X, level=0.8, return_all=True)
    c = dev.calls[-1]
    ok = [0, 2, 3, 5, 6]
    assert c["B"] == 5 and np.array_equal(c["alpha"], res.alpha[ok].ravel()) and c["contrib"] and len(c["ranks"]) <= 4
    assert set(out) == {"mean", "lo", "hi", "all"} and np.array_equal(out["all"], cube)
    lo, hi = np.percentile(cube, [10, 90], axis=2)
    assert out["lo"].shape == (4, 2) and np.array_equal(out["lo"], lo) and np.array_equal(out["hi"], hi)
    assert np.array_equal(out["mean"], [[sum(cell) / 5 for cell in row] for row in cube.tolist()])
    assert set(res.contributions(X, level=0.8)) == {"mean", "lo", "hi"}


@pytest.mark.parametrize("B,level", [(5, 0.5), (8, 0.95), (21, 0.9), (100, 0.99), (2, 0.5), (1, 0.9)])
def test_band_interpolation_is_numpys(partls, fake, B, level):
    rng = np.random.default_rng(B)
    cube = rng.normal(size=(6, 2, B)) * 10.0 ** rng.integers(-3, 4, size=(6, 2, 1))
    cube[0] = 1.25                                                         # ties
    _Device(fake, cube)
    out = _result(partls, B).contributions(np.zeros((6, 3)), level=level)
    lo, hi = np.percentile(cube, [50.0 - 50.0 * level, 50.0 + 50.0 * level], axis=2)
    assert np.array_equal(out["lo"], lo) and np.array_equal(out["hi"], hi)


def test_bad_arguments_are_refused_before_any_call(partls, fake):
    a, b, t, P = _models(4)
    X = np.zeros((5, 3))
    mk = partls.PartLSFitResult
    model = mk(a[0], b[0], 0.0, P)

    class Sparse:                                                          # anything with .tocsr() counts as sparse
        def tocsr(self):
            raise AssertionError("a refused matrix is not converted")

    ctx = partls.Context(0)
    res = _result(partls, 6)
    for name, fn in (("contributions", lambda: partls.contributions(model, Sparse())),
                     ("contributions_many", lambda: partls.contributions_many([model], Sparse())),
                     ("group_importance", lambda: partls.group_importance(model, Sparse())),
                     ("contributions", lambda: ctx.contributions(Sparse(), P, a, b)),
                     ("contributions", lambda: res.contributions(Sparse()))):
        with pytest.raises(NotImplementedError) as e:
            fn()
        assert name in str(e.value) and "densify" in str(e.value)
    for fn in (partls.contributions_many, partls.group_importance):
        with pytest.raises(TypeError):
            fn((a, b, t, P), np.zeros((5, 3), dtype=np.int64))            # an integer X
        with pytest.raises(ValueError):
            fn((a, b, t, P), np.zeros((5, 4)))                            # X has another M
        with pytest.raises(ValueError):
            fn([], X)                                                     # no model
        with pytest.raises(ValueError):
            fn((a[:, :2], b, t, P), X)                                    # alpha is not (B, M)
        with pytest.raises(ValueError):
            fn((a, b[:3], t[:3], P), X)                                   # beta has another B
        with pytest.raises(ValueError):
            fn([mk(a[0], b[0], 0.0, P), mk(a[1], b[1], 0.0, np.array([[1, 0], [0, 1], [0, 1]]))], X)
    with pytest.raises(TypeError):
        partls.contributions(model, X.astype(np.int32))
    with pytest.raises(TypeError):
        partls.contributions([model], X)                                  # many models go to contributions_many
    with pytest.raises(ValueError):
        ctx.contributions(X, P, a, b, ranks=[4])                          # a rank outside [0, B)
    with pytest.raises(ValueError):
        ctx.contributions(X, P, a, b[:3])
    with pytest.raises(ValueError):
        ctx.contributions_device(0x1000, 5, 3, 5, P, a, b, ranks=[1])     # ranks without a place for stats
    with pytest.raises(TypeError):
        ctx.contributions_device(0x1000, 5, 3, 5, P, a, b, dcontrib_ptr=0x2000, ldC=5, dtype=np.float16)
    for level in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            res.contributions(X, level=level)
    with pytest.raises(ValueError):
        _result(partls, 3, bad=(0, 1, 2)).contributions(X)
    with pytest.raises(TypeError):
        res.contributions(X.astype(np.int32))
    with pytest.raises(ValueError):
        res.contributions(np.zeros((5, 4)))
    assert not [ln for ln in fake.lines if ln.startswith("partls_contributions")]
    ctx.close()


class _PredictDevice:
    """the predict_many twin of _Device, for the unchanged-band check: writes stats and mean from Y[N, B]"""

    def __init__(self, fake, Y):
        self.ranks = None
        for name in ("partls_predict_many", "partls_predict_many_f32"):
            setattr(fake, name, self._wrap(getattr(fake, name), Y))

    def _wrap(self, inner, Y):
        def call(*args):
            status = inner(*args)
            N, B, nr = int(args[2]), int(args[9]), int(args[15])
            assert Y.shape == (N, B) and not T._addr(args[13])
            self.ranks = np.ctypeslib.as_array((C.c_int64 * nr).from_address(T._addr(args[16]))).copy()
            _doubles(args[17], N * nr).reshape(nr, N)[:] = np.sort(Y, axis=1)[:, self.ranks].T
            _doubles(args[18], N)[:] = [sum(row) / B for row in Y.tolist()]
            return status
        return call


@pytest.mark.parametrize("B,level", [(5, 0.5), (8, 0.95), (21, 0.9), (100, 0.95), (3, 0.1), (1, 0.9)])
def test_bootstrap_predict_is_unchanged_by_the_shared_helper(partls, fake, B, level):
    rng = np.random.default_rng(B)
    Y = rng.normal(size=(9, B)) * 10.0 ** rng.integers(-3, 4, size=(9, 1))
    Y[0] = 1.25
    dev = _PredictDevice(fake, Y)
    out = _result(partls, B).predict(np.zeros((9, 3)), level=level)
    q = [50.0 - 50.0 * level, 50.0 + 50.0 * level]
    lo, hi = np.percentile(Y, q, axis=1)
    assert set(out) == {"mean", "lo", "hi"} and len(dev.ranks) <= 4
    assert np.array_equal(out["lo"], lo) and np.array_equal(out["hi"], hi)
    assert np.array_equal(out["mean"], [sum(r) / B for r in Y.tolist()])
