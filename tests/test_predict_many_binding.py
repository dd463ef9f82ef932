"""CPU checks of predict_many against the fake library of tools/api_call_trace.py: the two entry points are declared
(include/partls.h, include/partls_f32_more.h), exported, bound with the same argument types and called by the Julia patch; the binding
hands the models over in the layouts of the ABI, leaves unwanted outputs NULL and derives the ranks of a band from its level;
bad arguments are refused before any call; failed replicates take no part; and the interpolation between the order statistics the
device returns is np.percentile's, to the last bit."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import api_call_trace as T  # noqa: E402
import check_julia_binding as CJ  # noqa: E402

NARGS = 19
NAMES = ("h", "X", "N", "M", "ldX", "dev", "P", "K", "ldP", "B", "alpha", "beta", "t", "yhat", "ldY", "nr", "ranks", "stats", "mean")


def test_symbols_in_headers_library_and_tables(partls):
    protos = CJ.parse_header()
    more = CJ.parse_header(CJ.F32_MORE_HEADER)
    table = {name: args for name, _, args in partls.lowlevel.SYMBOLS}
    table_more = {name: args for name, _, args in partls.lowlevel.SYMBOLS_F32_MORE}
    assert set(more) == set(table_more) == {"partls_predict_many_f32"}
    assert '#include "partls_f32_more.h"' in open(os.path.join(ROOT, "include", "partls.h")).read()
    partls.lowlevel.lib()                      # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    want = ["partls_ctx*", "double*", "int64_t", "int64_t", "int64_t", "int", "int64_t*", "int64_t", "int64_t", "int64_t", "double*",
            "double*", "double*", "double*", "int64_t", "int64_t", "int64_t*", "double*", "double*"]
    for name, proto, args in (("partls_predict_many", protos["partls_predict_many"], table["partls_predict_many"]),
                              ("partls_predict_many_f32", more["partls_predict_many_f32"], table_more["partls_predict_many_f32"])):
        assert hasattr(lib, name), name
        assert proto[0] == "partls_status" and len(proto[1]) == len(args) == NARGS, name
        assert proto[1] == want[:1] + ["float*" if name.endswith("f32") else "double*"] + want[2:], name
    assert table["partls_predict_many"] == table_more["partls_predict_many_f32"]
    calls = {c[0] for c in CJ.parse_ccalls()}
    checked = {s for s, _ in CJ.check()}
    for name in ("partls_predict_many", "partls_predict_many_f32"):
        assert name in calls and name in checked, name


def test_constants_are_the_headers(partls):
    text = open(os.path.join(ROOT, "include", "partls.h")).read()
    L = partls.lowlevel
    assert int(re.search(r"#define PARTLS_PREDICT_MANY_CHUNK (\d+)", text).group(1)) == L.PREDICT_MANY_CHUNK
    assert int(re.search(r"#define PARTLS_PREDICT_MANY_MAX_B (\d+)", text).group(1)) == L.PREDICT_MANY_MAX_B >= 4096
    m = re.search(r"#define PARTLS_PREDICT_MANY_BYTES \((\d+)ULL << (\d+)\)", text)
    assert int(m.group(1)) << int(m.group(2)) == L.PREDICT_MANY_BYTES
    assert "predict_many" in partls.__all__ and partls.predict_many is partls.api.predict_many


# ---- a fake device: records what a call was handed and writes what a device would -------------------------------------------------------
def _doubles(arg, n):
    return np.ctypeslib.as_array((C.c_double * n).from_address(T._addr(arg)))


class _Device:
    """wraps the fake library's two predict_many symbols: every call is recorded (scalars by value, the model arrays as copies, the
    addresses of X and of the outputs) and the outputs are written from Y[N, B], the predictions this 'device' computes"""

    def __init__(self, fake, Y=None):
        self.calls, self.Y = [], Y
        for name in ("partls_predict_many", "partls_predict_many_f32"):
            setattr(fake, name, self._wrap(name, getattr(fake, name)))

    def _wrap(self, name, inner):
        def call(*args):
            assert len(args) == NARGS
            status = inner(*args)
            a = dict(zip(NAMES, args))
            N, M, K, B, nr = (int(a[k]) for k in ("N", "M", "K", "B", "nr"))
            rec = dict(symbol=name, N=N, M=M, K=K, B=B, nr=nr, ldX=int(a["ldX"]), ldP=int(a["ldP"]), ldY=int(a["ldY"]), dev=int(a["dev"]),
                       alpha=_doubles(a["alpha"], M * B).copy(), beta=_doubles(a["beta"], K * B).copy(), t=_doubles(a["t"], B).copy(),
                       ranks=None if not T._addr(a["ranks"]) else np.ctypeslib.as_array((C.c_int64 * nr).from_address(T._addr(a["ranks"]))).copy(),
                       **{k: T._addr(a[k]) for k in ("X", "yhat", "stats", "mean")})
            if not rec["dev"]:
                xt = C.c_float if name.endswith("f32") else C.c_double
                rec["Xvalues"] = np.ctypeslib.as_array((xt * (rec["ldX"] * M)).from_address(rec["X"])).copy()
            self.calls.append(rec)
            if self.Y is not None and not rec["dev"]:
                Y = np.asarray(self.Y, dtype=np.float64)
                assert Y.shape == (N, B)
                if rec["yhat"]:
                    _doubles(a["yhat"], rec["ldY"] * B).reshape(B, rec["ldY"])[:, :N] = Y.T
                if rec["stats"]:
                    _doubles(a["stats"], N * nr).reshape(nr, N)[:] = np.sort(Y, axis=1)[:, rec["ranks"]].T
                if rec["mean"]:
                    _doubles(a["mean"], N)[:] = [sum(row) / B for row in Y.tolist()]
            return status
        return call


@pytest.fixture
def fake(partls):
    with T.fake_library(partls.api) as f:
        yield f


def _models(B, M=3, K=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(B, M)), rng.normal(size=(B, K)), rng.normal(size=B), np.array([[1, 0], [1, 0], [0, 1]])


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
    a, b, t, P = _models(4)
    X = np.random.default_rng(1).normal(size=(5, 3))                      # C-ordered: goes over as a column-major copy
    ctx = partls.Context(0)
    out = ctx.predict_many(X, P, a, b, t)
    c = dev.calls[-1]
    assert c["symbol"] == "partls_predict_many" and (c["N"], c["M"], c["K"], c["B"], c["dev"]) == (5, 3, 2, 4, 0)
    assert (c["ldX"], c["ldP"], c["ldY"], c["nr"]) == (5, 3, 5, 0)
    assert np.array_equal(c["Xvalues"], X.T.ravel())                      # column-major N x M
    assert np.array_equal(c["alpha"], a.ravel()) and np.array_equal(c["beta"], b.ravel()) and np.array_equal(c["t"], t)   # M x B, K x B: model b = column b
    assert c["yhat"] and not c["stats"] and not c["mean"] and c["ranks"] is None
    assert out["yhat"].shape == (5, 4) and out["yhat"].flags.f_contiguous and out["stats"] is None and out["mean"] is None
    # statistics only: yhat is NULL, the ranks go over as int64, stats is N x nr
    out = ctx.predict_many(X.astype(np.float32), P, a, b, t, ranks=[3, 0], want_yhat=False, want_mean=True)
    c = dev.calls[-1]
    assert c["symbol"] == "partls_predict_many_f32" and np.array_equal(c["Xvalues"], X.astype(np.float32).T.ravel())
    assert not c["yhat"] and c["stats"] and c["mean"] and c["nr"] == 2 and c["ranks"].tolist() == [3, 0]
    assert out["yhat"] is None and out["stats"].shape == (5, 2) and out["mean"].shape == (5,)
    # device pointers pass through as they are
    ctx.predict_many_device(0x7f0000001000, 5, 3, 8, P, a, b, t, dyhat_ptr=0x7f0000002000, ldY=6, dtype=np.float32)
    c = dev.calls[-1]
    assert c["symbol"] == "partls_predict_many_f32" and (c["X"], c["yhat"], c["stats"], c["mean"]) == (0x7f0000001000, 0x7f0000002000, 0, 0)
    assert (c["dev"], c["ldX"], c["ldY"], c["nr"]) == (1, 8, 6, 0)
    ctx.predict_many_device(0x7f0000001000, 5, 3, 8, P, a, b, t, ranks=[1], dstats_ptr=0x7f0000003000, dmean_ptr=0x7f0000004000)
    c = dev.calls[-1]
    assert c["symbol"] == "partls_predict_many" and (c["yhat"], c["stats"], c["mean"], c["nr"]) == (0, 0x7f0000003000, 0x7f0000004000, 1)
    ctx.close()


def test_predict_many_takes_models_or_arrays(partls, fake):
    a, b, t, P = _models(5)
    X = np.random.default_rng(2).normal(size=(6, 3))
    Y = np.random.default_rng(3).normal(size=(6, 5))
    dev = _Device(fake, Y)
    models = [partls.PartLSFitResult(a[j], b[j], float(t[j]), P.copy()) for j in range(5)]          # equal partitions, not one object
    for arg in (models, tuple(models), (a, b, t, P)):
        got = partls.predict_many(arg, X)
        assert got.dtype == np.float64 and np.array_equal(got, Y)
        c = dev.calls[-1]
        assert np.array_equal(c["alpha"], a.ravel()) and np.array_equal(c["beta"], b.ravel()) and np.array_equal(c["t"], t)
        assert c["symbol"] == "partls_predict_many" and not c["stats"] and not c["mean"]
    partls.predict_many(models, X.astype(np.float32))
    assert dev.calls[-1]["symbol"] == "partls_predict_many_f32"


def test_band_ranks_follow_the_level(partls, fake):
    dev = _Device(fake, None)
    X = np.zeros((4, 3))
    _result(partls, 100).predict(X, level=0.95)
    c = dev.calls[-1]
    assert c["ranks"].tolist() == [2, 3, 96, 97] and c["B"] == 100 and not c["yhat"] and c["stats"] and c["mean"]
    _result(partls, 5).predict(X, level=0.5)               # the 25th and 75th percentiles of 5 values are values 1 and 3 themselves
    assert dev.calls[-1]["ranks"].tolist() == [1, 3]
    _result(partls, 1).predict(X, level=0.9)
    assert dev.calls[-1]["ranks"].tolist() == [0]
    _result(partls, 2).predict(X, level=0.9)
    assert dev.calls[-1]["ranks"].tolist() == [0, 1]


def test_bad_arguments_are_refused_before_any_call(partls, fake):
    a, b, t, P = _models(4)
    X = np.zeros((5, 3))
    P2 = np.array([[1, 0], [0, 1], [0, 1]])
    mk = partls.PartLSFitResult
    with pytest.raises(ValueError):
        partls.predict_many([mk(a[0], b[0], 0.0, P), mk(a[1], b[1], 0.0, P2)], X)            # two partitions
    with pytest.raises(ValueError):
        partls.predict_many([], X)
    with pytest.raises(ValueError):
        partls.predict_many([mk(a[0], b[0], 0.0, P), mk(a[1][:2], b[1], 0.0, P)], X)         # models of two shapes
    with pytest.raises(ValueError):
        partls.predict_many((a[:, :2], b, t, P), X)                                          # alpha is not (B, M)
    with pytest.raises(ValueError):
        partls.predict_many((a, b, t[:3], P), X)                                             # t is not (B,)
    with pytest.raises(ValueError):
        partls.predict_many((a, b, t, P), np.zeros((5, 4)))                                  # X has another M
    with pytest.raises(TypeError):
        partls.predict_many((a, b, t, P), np.zeros((5, 3), dtype=np.int64))                  # an integer X
    ctx = partls.Context(0)
    with pytest.raises(ValueError):
        ctx.predict_many(X, P, a, b, t, ranks=[4])                                           # a rank outside [0, B)
    with pytest.raises(ValueError):
        ctx.predict_many_device(0x1000, 5, 3, 5, P, a, b, t, ranks=[1])                      # ranks without a place for stats
    with pytest.raises(TypeError):
        ctx.predict_many_device(0x1000, 5, 3, 5, P, a, b, t, dyhat_ptr=0x2000, ldY=5, dtype=np.float16)
    res = _result(partls, 6)
    for level in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            res.predict(X, level=level)
    with pytest.raises(ValueError):
        _result(partls, 3, bad=(0, 1, 2)).predict(X)                                         # no successful replicate
    with pytest.raises(TypeError):
        res.predict(X.astype(np.int32))
    with pytest.raises(ValueError):
        res.predict(np.zeros((5, 4)))
    assert not [ln for ln in fake.lines if ln.startswith("partls_predict_many")]
    ctx.close()


def test_failed_replicates_take_no_part(partls, fake):
    res = _result(partls, 7, bad=(1, 4))
    ok = [0, 2, 3, 5, 6]
    Y = np.random.default_rng(4).normal(size=(3, 5))
    dev = _Device(fake, Y)
    out = res.predict(np.zeros((3, 3)), level=0.8, return_all=True)
    c = dev.calls[-1]
    assert c["B"] == 5 and np.array_equal(c["alpha"], res.alpha[ok].ravel()) and np.array_equal(c["t"], res.t[ok])
    assert np.all(np.isfinite(c["alpha"])) and np.all(np.isfinite(c["beta"]))
    assert out["yhat"].shape == (3, 5) and np.array_equal(out["yhat"], Y)
    assert set(out) == {"mean", "lo", "hi", "yhat"}
    assert set(res.predict(np.zeros((3, 3)), level=0.8)) == {"mean", "lo", "hi"}


@pytest.mark.parametrize("B,level", [(5, 0.5), (5, 0.9), (8, 0.95), (8, 0.3), (21, 0.9), (100, 0.95), (100, 0.99), (3, 0.1), (2, 0.5), (1, 0.9)])
def test_interpolation_is_numpys(partls, fake, B, level):
    """lo and hi equal np.percentile on the full matrix exactly: the two neighbours are the order statistics either side of numpy's virtual
    index, and _lerp is numpy's formula with its switch at gamma = 0.5 (both sides of it occur in these cases)"""
    rng = np.random.default_rng(B)
    Y = rng.normal(size=(9, B)) * 10.0 ** rng.integers(-3, 4, size=(9, 1))
    Y[0] = 1.25                                                        # a row of ties
    if B > 2:
        Y[1, 1:] = Y[1, 0]
        Y[2] = np.arange(B)[::-1]                                      # hand-made: the percentiles of 0 .. B-1 are the virtual indices
    _Device(fake, Y)
    out = _result(partls, B).predict(np.zeros((9, 3)), level=level)
    q = [50.0 - 50.0 * level, 50.0 + 50.0 * level]
    lo, hi = np.percentile(Y, q, axis=1)
    assert np.array_equal(out["lo"], lo) and np.array_equal(out["hi"], hi)
    assert np.array_equal(out["mean"], [sum(r) / B for r in Y.tolist()])


def test_the_usual_levels_give_round_percentiles(partls, fake):
    """level 0.9 asks for the 5th and 95th percentile exactly (50 (1 - 0.9) in floating point is not 5)"""
    Y = np.random.default_rng(7).normal(size=(6, 40))
    _Device(fake, Y)
    for level, q in ((0.9, [5, 95]), (0.95, [2.5, 97.5]), (0.5, [25, 75]), (0.8, [10, 90])):
        out = _result(partls, 40).predict(np.zeros((6, 3)), level=level)
        lo, hi = np.percentile(Y, q, axis=1)
        assert np.array_equal(out["lo"], lo) and np.array_equal(out["hi"], hi), level
