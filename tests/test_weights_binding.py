"""CPU checks of sample weights: fit and cross_validate reject bad weights with ValueError (and weights on several
devices with NotImplementedError) before any device work; the two weighted entry points are declared by the header, exported by the
library, bound by the ctypes table, and called by the Julia drop-in (tools/check_julia_binding.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_julia_binding as CJ  # noqa: E402

NEW = ("partls_opt_prepare_weighted", "partls_cv_opt_weighted")


def _problem():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(12, 3))
    y = rng.normal(size=12)
    P = np.array([[1, 0], [1, 0], [0, 1]])
    return X, y, P


def _no_device(*a, **k):
    raise AssertionError("device work started before the weights were checked")


BAD = [
    ("negative", lambda N: np.r_[np.ones(N - 1), -1.0]),
    ("nan", lambda N: np.r_[np.ones(N - 1), np.nan]),
    ("inf", lambda N: np.r_[np.ones(N - 1), np.inf]),
    ("short", lambda N: np.ones(N - 1)),
    ("long", lambda N: np.ones(N + 1)),
    ("matrix", lambda N: np.ones((N, 1))),
    ("all_zero", lambda N: np.zeros(N)),
    ("integer", lambda N: np.ones(N, dtype=np.int64)),
]


@pytest.mark.parametrize("name,make", BAD, ids=[b[0] for b in BAD])
def test_bad_weights_raise_before_device_work(partls, monkeypatch, name, make):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    X, y, P = _problem()
    w = make(len(y))
    for alg in (partls.Opt, partls.Alt, partls.BnB):
        with pytest.raises(ValueError):
            partls.fit(alg, X, y, P, weights=w)
    with pytest.raises(ValueError):
        partls.cross_validate(partls.Opt, X, y, P, nfolds=3, weights=w)


def test_weights_with_devices_is_not_implemented(partls, monkeypatch):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    monkeypatch.setattr(partls.api, "default_multi", _no_device)
    X, y, P = _problem()
    for alg in (partls.Opt, partls.BnB):
        with pytest.raises(NotImplementedError):
            partls.fit(alg, X, y, P, weights=np.ones(len(y)), devices=2)


def test_cross_validate_rejects_a_fold_without_training_weight(partls, monkeypatch):
    monkeypatch.setattr(partls.api, "default_context", _no_device)
    X, y, P = _problem()
    w = np.zeros(len(y))
    w[:4] = 1.0                        # only fold 0 (rows 0..3 of 3 folds) carries weight: its training rows weigh nothing
    with pytest.raises(ValueError):
        partls.cross_validate(partls.Opt, X, y, P, nfolds=3, weights=w)


def test_symbols_in_header_library_and_table(partls):
    protos = CJ.parse_header()
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS}
    partls.lowlevel.lib()              # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    for s in NEW:
        assert s in protos and s in table and hasattr(lib, s), s
    assert len(protos["partls_opt_prepare_weighted"][1]) == len(table["partls_opt_prepare_weighted"][1]) == 13
    assert len(protos["partls_cv_opt_weighted"][1]) == len(table["partls_cv_opt_weighted"][1]) == 25
    assert partls.lowlevel.lib().partls_version() >= 101


def test_integration_calls_both_entry_points():
    calls = {c[0] for c in CJ.parse_ccalls()}
    checked = {s for s, _ in CJ.check()}
    for s in NEW:
        assert s in calls and s in checked, s
