"""CPU checks of the sparse design-matrix path: the two entry points are declared by include/partls_csr.h (which
include/partls.h includes), exported by the library, bound by the ctypes table (SYMBOLS_CSR) with the same argument counts, and called
by the Julia drop-in (tools/check_julia_binding.py); fit / predict hand a sparse X over as canonical CSR — int64 row
pointers, int32 column indices, float64 values — without ever building an N x M array; and the entry points that read a dense X only
refuse a sparse one instead of densifying it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_julia_binding as CJ  # noqa: E402

NEW = {"partls_opt_prepare_csr": 14, "partls_predict_csr": 14}


def test_symbols_in_header_library_and_table(partls):
    protos = CJ.parse_header(CJ.CSR_HEADER)
    table = {name: (res, args) for name, res, args in partls.lowlevel.SYMBOLS_CSR}
    assert set(protos) == set(table) == set(NEW)
    assert '#include "partls_csr.h"' in open(os.path.join(ROOT, "include", "partls.h")).read()
    assert set(NEW) <= set(CJ.parse_headers())
    partls.lowlevel.lib()              # the package's loader first (it puts torch's HIP runtime in place)
    lib = C.CDLL(partls.library_path())
    for s, n in NEW.items():
        assert hasattr(lib, s), s
        assert len(protos[s][1]) == len(table[s][1]) == n, s
        assert protos[s][0] == "partls_status", s
        assert protos[s][1][1:4] == ["int64_t*", "int32_t*", "double*"], s         # indptr, indices, values
    assert protos["partls_opt_prepare_csr"][1][6:8] == ["double*", "double*"]       # y and w
    assert partls.lowlevel.lib().partls_version() >= 107


def test_integration_calls_both_with_csr_pointers():
    calls = {c[0]: c for c in CJ.parse_ccalls()}
    checked = {s for s, _ in CJ.check()}
    for s in NEW:
        assert s in calls and s in checked, s
        assert calls[s][2][1:4] == ["Ptr{Int64}", "Ptr{Int32}", "Ptr{Float64}"], s
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 8. `X::SparseMatrixCSC`"):text.index("## Notes for the maintainer")]
    assert "sparse(X')" in sec and "Matrix(X)" not in sec and "Array(X)" not in sec


# ---- what fit / predict hand to the context ---------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the default context (and the default multi-context): records what it is given, computes nothing; every entry that
    must not be reached with a sparse X fails the test"""

    def __init__(self):
        self.seen = []
        self.tolerate_ill = False
        self.last_ill = False
        self.generation = 0
        self.devices = [0, 0]
        self._h = None

    def opt_prepare(self, X, y, P, eta=0.0, flags=0, weights=None):
        self.seen.append(("prepare", X))
        assert y.dtype == np.float64 and (weights is None or weights.dtype == np.float64)
        self._M, self._K = X.shape[1], P.shape[1]

    def opt_sweep(self, g_begin=0, g_end=-1, want_all=False):
        return 0.0, 0, (np.zeros(2 ** (self._K + 1)) if want_all else None), 0

    def opt_finish(self, pattern):
        return np.zeros(self._M), np.zeros(self._K), 0.0, 0.0, 0

    def alt_prepared(self, a0, b0, eps=1e-6, T=100):
        return np.zeros(self._M), np.zeros(self._K), 0.0, 0.0, 1

    def bnb_prepared(self):
        return np.zeros(self._M), np.zeros(self._K), 0.0, 0.0, 1

    def predict(self, X, P, alpha, beta, t):
        self.seen.append(("predict", X))
        return np.zeros(X.shape[0])

    def _never(self, *a, **k):
        raise AssertionError("a sparse X reached the context through an entry point that reads a dense X")

    fit_opt = fit_bnb = cv_opt = cv_alt = opt_weightings = predict_many = _never


@pytest.fixture
def recorder(partls, monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(partls.api, "default_context", lambda device=0: r)
    monkeypatch.setattr(partls.api, "default_multi", lambda devices=None: r)
    return r


def csr_of(D, dtype=np.float64):
    """canonical CSR of a dense array with numpy alone: np.nonzero walks it in row-major order"""
    r, c = np.nonzero(D)
    indptr = np.zeros(D.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=D.shape[0]), out=indptr[1:])
    return indptr, c.astype(np.int32), D[r, c].astype(dtype)


def _data():
    rng = np.random.default_rng(3)
    D = rng.normal(size=(12, 5)) * (rng.random((12, 5)) < 0.4)
    D[4] = 0.0
    D[:, 2] = 0.0
    return D, rng.normal(size=12), np.array([[1, 0], [1, 0], [0, 1], [0, 1], [0, 1]])


def _assert_canonical(got, D):
    indptr, indices, data = csr_of(D)
    assert type(got).__name__ == "CSR" and tuple(got.shape) == D.shape
    assert got.indptr.dtype == np.int64 and got.indices.dtype == np.int32 and got.data.dtype == np.float64
    assert all(a.flags.c_contiguous for a in (got.indptr, got.indices, got.data))
    assert np.array_equal(got.indptr, indptr) and np.array_equal(got.indices, indices) and np.array_equal(got.data, data)


def _fit_and_predict_everything(partls, X, y, P):
    partls.fit(partls.Opt, X, y, P)
    partls.fit(partls.Opt, X, y, P, weights=np.ones(len(y)), returnAllSolutions=True, top=None)
    partls.fit(partls.Alt, X, y, P, alpha0=np.ones(P.shape[0] + 1), beta0=np.ones(P.shape[1] + 1))
    partls.fit(partls.BnB, X, y, P, eta=0.5)
    model = partls.PartLSFitResult(np.ones(P.shape[0]), np.ones(P.shape[1]), 0.5, P)
    partls.predict(model, X)
    partls.predict(model.α, model.β, model.t, P, X)


@pytest.mark.parametrize("vdtype", [np.float64, np.float32])
def test_numpy_built_triple_arrives_as_canonical_csr(partls, recorder, vdtype):
    D, y, P = _data()
    D = D.astype(vdtype).astype(np.float64)                                   # values a float32 holds exactly
    indptr, indices, data = csr_of(D, vdtype)
    X = partls.CSR(indptr.astype(np.int32), indices.astype(np.int64), data, D.shape)     # other integer widths are converted
    _fit_and_predict_everything(partls, X, y, P)
    assert [w for w, _ in recorder.seen] == ["prepare"] * 4 + ["predict"] * 2
    for _, got in recorder.seen:
        _assert_canonical(got, D)                                             # float32 values arrive widened


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo", "csr_unsorted", "coo_duplicates", "csr_f32"])
def test_scipy_inputs_arrive_as_canonical_csr(partls, recorder, fmt):
    sp = pytest.importorskip("scipy.sparse")
    D, y, P = _data()
    r, c = np.nonzero(D)
    v = D[r, c]
    if fmt == "csr_unsorted":                                                  # every row's entries in descending column order
        indptr, indices, data = csr_of(D)
        idx2, dat2 = indices.copy(), data.copy()
        for i in range(D.shape[0]):
            a, b = indptr[i], indptr[i + 1]
            idx2[a:b], dat2[a:b] = indices[a:b][::-1], data[a:b][::-1]
        X = sp.csr_matrix((dat2, idx2, indptr), shape=D.shape)
        assert not X.has_sorted_indices or D.shape[0] == 0
        keep = (X.indices.copy(), X.data.copy())
    elif fmt == "coo_duplicates":                                              # every entry split into two halves, shuffled
        order = np.random.default_rng(1).permutation(2 * len(v))
        X = sp.coo_matrix((np.concatenate([v, v])[order] / 2, (np.concatenate([r, r])[order], np.concatenate([c, c])[order])), shape=D.shape)
    elif fmt == "csr_f32":
        D = D.astype(np.float32).astype(np.float64)
        X = sp.csr_matrix(D.astype(np.float32))
    else:
        X = getattr(sp, fmt + "_matrix")(D)
    _fit_and_predict_everything(partls, X, y, P)
    assert [w for w, _ in recorder.seen] == ["prepare"] * 4 + ["predict"] * 2
    for _, got in recorder.seen:
        _assert_canonical(got, D)
    if fmt == "csr_unsorted":                                                  # the caller's matrix is not reordered in place
        assert np.array_equal(X.indices, keep[0]) and np.array_equal(X.data, keep[1])


def test_solutions_keep_the_csr_triple(partls, recorder):
    D, y, P = _data()
    _, _, rep = partls.fit(partls.Opt, partls.CSR(*csr_of(D), D.shape), y, P, returnAllSolutions=True)
    _assert_canonical(rep.solutions._problem[0], D)


def test_nothing_of_size_n_times_m_is_allocated(partls, recorder):
    """N = 10^6, M = 1000, 10 nonzeros: the dense matrix would be 8 GB — a path that built it could not finish within this test"""
    N, M = 10 ** 6, 1000
    rows = np.arange(10, dtype=np.int64) * 99991
    indptr = np.zeros(N + 1, dtype=np.int64)
    indptr[rows + 1] = 1
    np.cumsum(indptr, out=indptr)
    X = partls.CSR(indptr, (np.arange(10) * 97).astype(np.int32), np.ones(10), (N, M))
    P = np.zeros((M, 2), dtype=np.int64)
    P[: M // 2, 0] = 1
    P[M // 2:, 1] = 1
    y = np.zeros(N)
    partls.fit(partls.Opt, X, y, P)
    partls.predict(partls.PartLSFitResult(np.ones(M), np.ones(2), 0.0, P), X)
    for _, got in recorder.seen:
        assert got.shape == (N, M) and len(got.data) == 10 and got.indptr[-1] == 10
    sp = pytest.importorskip("scipy.sparse")
    partls.fit(partls.BnB, sp.csr_matrix((np.ones(10), (rows, np.arange(10) * 97)), shape=(N, M)), y, P)
    assert len(recorder.seen[-1][1].data) == 10


def test_dimension_and_dtype_errors_match_the_dense_path(partls, recorder):
    D, y, P = _data()
    indptr, indices, data = csr_of(D)
    X = partls.CSR(indptr, indices, data, D.shape)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        partls.fit(partls.Opt, X, y[:-1], P)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        partls.fit(partls.Opt, X, y, P[:-1])
    with pytest.raises(TypeError, match="floating point"):
        partls.fit(partls.Opt, partls.CSR(indptr, indices, data.astype(np.int64), D.shape), y, P)
    with pytest.raises(TypeError, match="integer matrix"):
        partls.fit(partls.Opt, X, y, P.astype(np.float64))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        partls.predict(partls.PartLSFitResult(np.ones(4), np.ones(2), 0.0, P[:-1]), X)
    with pytest.raises(ValueError):
        partls.fit(partls.Opt, partls.CSR(indptr[:-1], indices, data, D.shape), y, P)
    assert recorder.seen == []


def test_dense_only_entry_points_refuse_a_sparse_x(partls, recorder):
    D, y, P = _data()
    X = partls.CSR(*csr_of(D), D.shape)
    model = partls.PartLSFitResult(np.ones(5), np.ones(2), 0.5, P)
    boot = partls.BootstrapResult(counts=None, alpha=np.ones((3, 5)), beta=np.ones((3, 2)), t=np.zeros(3), opt=np.zeros(3),
                                  best_index=np.zeros(3, dtype=np.int64), models=[model] * 3, status=np.zeros(3, dtype=np.int32),
                                  oob_sse=np.zeros(3), oob_rows=np.zeros(3), P=P)
    calls = {
        "cross_validate": lambda: partls.cross_validate(partls.Opt, X, y, P, nfolds=3),
        "bootstrap": lambda: partls.bootstrap(partls.Opt, X, y, P, B=4, rng=0),
        "resample": lambda: partls.resample(partls.Opt, X, y, P, np.ones((12, 2))),
        "predict_many": lambda: partls.predict_many([model, model], X),
        "BootstrapResult.predict": lambda: boot.predict(X),
        "devices=": lambda: partls.fit(partls.Opt, X, y, P, devices=[0, 0]),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError) as e:
            call()
        assert name in str(e.value) and "densify" in str(e.value), (name, str(e.value))
    assert recorder.seen == []


def test_the_package_never_densifies():
    pkg = os.path.join(ROOT, "partitionedls.jl_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert "toarray" not in src and "todense" not in src and "scipy" not in "".join(
                ln for ln in src.splitlines() if ln.lstrip().startswith(("import ", "from "))), f
