"""CPU checks of the cross-validation entry point: partls_cv_opt's prototype, the ctypes table and the Julia drop-in's ccall (INTEGRATION.md,
tools/check_julia_binding.py) describe one ABI, and the folds helper of cross_validate behaves as documented."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_julia_binding as CJ  # noqa: E402


def test_prototype_ctypes_and_julia_agree(partls):
    protos = CJ.parse_header()
    assert "partls_cv_opt" in protos
    ret, params = protos["partls_cv_opt"]
    assert ret == "partls_status" and len(params) == 24
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS}
    res, args = table["partls_cv_opt"]
    assert res is C.c_int and len(args) == 24
    assert args[6] is C.c_int and args[14] is C.c_uint32 and args[23] is C.POINTER(C.c_int32)
    calls = [c for c in CJ.parse_ccalls() if c[0] == "partls_cv_opt"]
    assert len(calls) == 1
    sym, _, types, nactual, _ = calls[0]
    assert len(types) == nactual == 24
    assert any(s == "partls_cv_opt" for s, _ in CJ.check())


def test_julia_dropin_has_a_stock_fallback():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "function cv_opt" in text and "_cv_opt_julia" in text


def test_batch_piece_knob_is_read_once_at_create():
    """PARTLS_BATCH_PIECE (problems per piece of the batched routes; the GPU tests of the pieces rest on it) is parsed in partls_create
    with the other knobs and nowhere else: the compute entries never call getenv"""
    csrc = os.path.join(ROOT, "partitionedls.jl_amd", "csrc")
    hits = {n: open(os.path.join(csrc, n)).read().count('getenv("PARTLS_BATCH_PIECE")') for n in sorted(os.listdir(csrc))
            if n.endswith((".hip", ".h"))}
    assert {n: k for n, k in hits.items() if k} == {"api.hip": 1}
    api = open(os.path.join(csrc, "api.hip")).read()
    create = api[api.index("partls_status partls_create("):api.index("void partls_destroy(")]
    assert 'getenv("PARTLS_BATCH_PIECE")) c->knobs.batch_piece = atoi(e);' in create


def test_cv_folds_uneven_sizes(partls):
    fp, perm = partls.cv_folds(11, 3)
    assert list(fp) == [0, 4, 8, 11]
    assert np.array_equal(perm, np.arange(11))
    sizes = np.diff(fp)
    assert list(sizes) == [len(a) for a in np.array_split(np.arange(11), 3)]


def test_cv_folds_shuffle_is_seeded(partls):
    fp1, p1 = partls.cv_folds(20, 4, shuffle=True, rng=7)
    fp2, p2 = partls.cv_folds(20, 4, shuffle=True, rng=np.random.default_rng(7))
    fp3, p3 = partls.cv_folds(20, 4, shuffle=True, rng=8)
    assert np.array_equal(p1, p2) and np.array_equal(fp1, fp2)
    assert not np.array_equal(p1, p3)
    assert sorted(p1) == list(range(20))


def test_cv_folds_counts(partls):
    fp, perm = partls.cv_folds(9, 0)
    assert list(fp) == [0] and len(perm) == 9
    fp, _ = partls.cv_folds(5, 5)
    assert list(fp) == [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError):
        partls.cv_folds(9, 1)
    with pytest.raises(ValueError):
        partls.cv_folds(4, 5)
    with pytest.raises(ValueError):
        partls.cv_folds(4, -2)


def test_cross_validate_rejects_other_algorithms(partls):
    X = np.ones((6, 2)); y = np.ones(6); P = np.array([[1], [1]])
    with pytest.raises(TypeError):
        partls.cross_validate(partls.BnB, X, y, P)
