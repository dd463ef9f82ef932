"""CPU checks of the rescue option at the binding (no GPU): the flag of include/partls.h is the Python constant and the getter is
exported; fit(Opt, ..., rescue=True) hands flags | 4 to the prepare and reads partls_get_rescue_stats — and only then, so that the
committed call trace of the default fit stays what it is; the combinations that are out of scope raise before any call is made."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import api_call_trace as T  # noqa: E402


def _header():
    return open(os.path.join(ROOT, "include", "partls.h")).read()


def test_the_flag_is_the_header_constant(partls):
    m = re.search(r"#define\s+PARTLS_OPT_RESCUE_CAPPED\s+(\d+)u", _header())
    assert m and int(m.group(1)) == partls.lowlevel.OPT_RESCUE_CAPPED == 4
    flags = {int(v) for v in re.findall(r"#define\s+PARTLS_OPT_[A-Z_]+\s+(\d+)u", _header())}
    assert flags == {1, 2, 4}, "the prepare flags are distinct bits"
    m = re.search(r"PARTLS_T_RESCUE\s*=\s*(\d+)", _header())
    assert m and int(m.group(1)) == partls.lowlevel.T_RESCUE


def test_the_getter_is_declared_bound_and_exported(partls):
    assert re.search(r"partls_status\s+partls_get_rescue_stats\(const partls_ctx \*ctx, int64_t \*rescued, int64_t \*pivots, int64_t \*failed\);",
                     _header())
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS}
    res, args = table["partls_get_rescue_stats"]
    assert res is C.c_int and len(args) == 4 and args[0] is C.c_void_p
    partls.lowlevel.lib()
    lib = C.CDLL(partls.library_path())
    assert hasattr(lib, "partls_get_rescue_stats")
    # no context: a status, no crash
    fn = lib.partls_get_rescue_stats
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] + [C.POINTER(C.c_int64)] * 3
    assert fn(None, None, None, None) == partls.lowlevel.ERR_BAD_ARG


@pytest.fixture
def fake(partls):
    with T.fake_library(partls.api) as f:
        yield f


def _data():
    Xs, y, P, w = T.problem()
    return Xs[np.float64, "F"], y, P


def _calls(fake, symbol):
    return [ln for ln in fake.lines if ln.startswith(symbol + "(")]


@pytest.mark.parametrize("kw,base", [({}, 0), (dict(faithful_intercept=True), 1), (dict(generic_kernel=True), 2),
                                      (dict(returnAllSolutions=True), 1), (dict(top=2), 1)])
def test_fit_sets_the_flag_and_reads_the_stats(partls, fake, kw, base):
    X, y, P = _data()
    _, _, rep = partls.fit(partls.Opt, X, y, P, rescue=True, **kw)
    prep = _calls(fake, "partls_opt_prepare")
    assert len(prep) == 1 and "flags=%d)" % (base | 4) in prep[0], prep
    assert len(_calls(fake, "partls_get_rescue_stats")) == 1
    assert rep.rescued == 0                                   # the fake writes nothing
    order = [ln.split("(")[0] for ln in fake.lines]
    assert order.index("partls_opt_finish") < order.index("partls_get_rescue_stats")
    if "top" in kw:
        assert order.index("partls_get_rescue_stats") < order.index("partls_opt_top")


def test_the_default_fit_neither_sets_the_flag_nor_calls_the_getter(partls, fake):
    X, y, P = _data()
    _, _, rep = partls.fit(partls.Opt, X, y, P)
    prep = _calls(fake, "partls_opt_prepare")
    assert len(prep) == 1 and "flags=0)" in prep[0]
    assert not _calls(fake, "partls_get_rescue_stats") and "rescued" not in rep
    _, _, rep = partls.fit(partls.Opt, X, y, P, rescue=False, faithful_intercept=True)
    assert "flags=1)" in _calls(fake, "partls_opt_prepare")[1] and not _calls(fake, "partls_get_rescue_stats")


def test_rescue_stats_reads_the_three_counters(partls, fake):
    X, y, P = _data()
    ctx = partls.Context(0)
    ctx.opt_prepare(X, y, P, 0.0, partls.lowlevel.OPT_FAITHFUL_INTERCEPT | partls.lowlevel.OPT_RESCUE_CAPPED)
    st = ctx.rescue_stats()
    assert dict(st) == dict(rescued=0, pivots=0, failed=0) and st.failed == 0
    assert _calls(fake, "partls_get_rescue_stats") == ["partls_get_rescue_stats(c1, out, out, out) -> 0"]
    with fake.scripted(partls_get_rescue_stats=1):
        with pytest.raises(partls.PartlsError):
            ctx.rescue_stats()


def test_the_refused_combinations_raise_before_any_call(partls, fake):
    X, y, P = _data()
    with pytest.raises(NotImplementedError):
        partls.fit(partls.Opt, X, y, P, rescue=True, devices=[0, 0])
    for alg in (partls.Alt, partls.BnB):
        with pytest.raises(ValueError):
            partls.fit(alg, X, y, P, rescue=True)
    assert not [ln for ln in fake.lines if "prepare" in ln or "fit" in ln]
    for fn in (partls.cross_validate, partls.bootstrap):
        with pytest.raises(TypeError):
            fn(partls.Opt, X, y, P, rescue=True)
    with pytest.raises(TypeError):
        partls.resample(partls.Opt, X, y, P, np.ones((len(y), 2)), rescue=True)
