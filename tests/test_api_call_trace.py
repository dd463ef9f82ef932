"""CPU checks of the Python binding against a fake library (tools/api_call_trace.py): the calls it makes into libpartls_hip.so for a
fixed list of cases are the committed ones (tests/golden/api_call_trace.txt, identical to the trace of the binding before its
marshalling was gathered into one path per entry family), and the tolerance of status 9 (PARTLS_ERR_ILL_CONDITIONED) belongs to the call
that asked for it: fit() leaves the shared default objects as it found them, a returnAllSolutions result keeps the on_ill_conditioned of
its own fit, a view of a MultiContext follows its owner."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import api_call_trace as T  # noqa: E402

ILL = 9


def test_the_trace_is_the_committed_one(partls):
    with open(os.path.join(GOLDEN, "api_call_trace.txt")) as f:
        want = f.read().splitlines()
    got = T.generate()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    assert len(got) == len(want)


@pytest.fixture
def fake(partls):
    with T.fake_library(partls.api) as f, warnings.catch_warnings():
        warnings.simplefilter("ignore", partls.IllConditionedWarning)
        yield f


def _data():
    Xs, y, P, w = T.problem()
    return Xs[np.float64, "F"], y, P


def _raises_ill(partls, fn, *a):
    with pytest.raises(partls.PartlsError) as e:
        fn(*a)
    assert e.value.status == ILL


def test_fit_leaves_the_default_context_as_it_found_it(partls, fake):
    X, y, P = _data()
    ctx = partls.default_context()
    assert ctx.tolerate_ill is False
    with fake.scripted(partls_opt_finish=ILL):
        _, _, rep = partls.fit(partls.Opt, X, y, P)                      # "warn" is the default
        assert rep.ill_conditioned and ctx.last_ill
        assert partls.default_context() is ctx and ctx.tolerate_ill is False
        _raises_ill(partls, ctx.opt_finish, 0)
    with fake.scripted(partls_fit_opt_multi=ILL):
        mc = partls.default_multi([0, 0])
        partls.fit(partls.Opt, X, y, P, devices=[0, 0])
        assert mc.tolerate_ill is False and ctx.tolerate_ill is False
        _raises_ill(partls, mc.fit_opt, X, y, P)


def test_a_fit_that_raises_restores_the_tolerance_too(partls, fake):
    X, y, P = _data()
    ctx = partls.default_context()
    with fake.scripted(partls_opt_sweep=6):
        with pytest.raises(partls.PartlsError) as e:
            partls.fit(partls.Opt, X, y, P)
    assert e.value.status == 6 and ctx.tolerate_ill is False
    with fake.scripted(partls_opt_finish=ILL):
        _raises_ill(partls, ctx.opt_finish, 0)


def test_a_users_own_setting_survives_a_fit(partls, fake):
    X, y, P = _data()
    own = partls.Context(0)
    own.tolerate_ill = True
    shared = partls.default_context()
    shared.tolerate_ill = True                                            # the shared object is the user's to set as well
    partls.fit(partls.Opt, X, y, P, on_ill_conditioned="raise")
    with fake.scripted(partls_opt_finish=ILL):
        _raises_ill(partls, lambda: partls.fit(partls.Opt, X, y, P, on_ill_conditioned="raise"))
        assert own.tolerate_ill is True and shared.tolerate_ill is True
        own.opt_prepare(X, y, P)
        own.opt_finish(0)
        assert own.last_ill


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["single", "multi"])
def test_solutions_keep_the_choice_of_their_own_fit(partls, fake, devices):
    X, y, P = _data()
    kw = dict(returnAllSolutions=True, devices=devices)
    warned = partls.fit(partls.Opt, X, y, P, **kw)[2].solutions
    with fake.scripted(partls_opt_finish=ILL):
        assert warned[1][1].α.shape == (3,)                              # on the shared context
    raising = partls.fit(partls.Opt, X, y, P, on_ill_conditioned="raise", **kw)[2].solutions     # takes the shared context over
    with fake.scripted(partls_opt_finish=ILL):
        _raises_ill(partls, raising.__getitem__, 1)                       # on the shared context
        assert warned[1][1].α.shape == (3,)                              # on a private context, prepared again
        assert warned._ctx is not partls.default_context() and warned._ctx.tolerate_ill is False
    partls.fit(partls.Opt, X, y, P, **kw)
    with fake.scripted(partls_opt_finish=ILL):
        _raises_ill(partls, raising.__getitem__, 1)                       # on its private context, after a "warn" fit


def test_a_view_follows_its_owner(partls, fake):
    X, y, P = _data()
    mc = partls.MultiContext([0, 0])
    mc.fit_opt(X, y, P)
    view = mc.context(0)
    view._shape = (12, 3, 2)
    with fake.scripted(partls_opt_finish=ILL):
        _raises_ill(partls, view.opt_finish, 0)
        mc.tolerate_ill = True
        view.opt_finish(0)
        assert view.last_ill and view.tolerate_ill is True
        mc.tolerate_ill = False
        _raises_ill(partls, view.opt_finish, 0)
