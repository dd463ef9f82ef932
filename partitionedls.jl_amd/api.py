"""Host-side mirror of the reference's operator interface for the hot path (PartitionedLS.jl:3 exports).

fit(Opt|Alt|BnB, X, y, P; η, ...) / predict keep the reference's names, argument meaning, result tuple
`(PartLSFitResult, nothing, report)` and error behaviour; the arithmetic runs on the MI355X through the C ABI
(include/partls.h).  Nothing here computes on the CPU beyond argument marshalling.
"""
import atexit
import ctypes as C
import os
import warnings
import weakref
from contextlib import contextmanager
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _lib as L


class PartlsError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"partls status {status}: {msg}")
        self.status = status


class Opt:      # Opt.jl:1
    """Optimal algorithm: complete enumeration of the sign patterns."""


class Alt:      # Alt.jl:3
    """Alternating optimisation."""


class BnB:      # BnB.jl:1
    """Branch and bound."""


@dataclass
class PartLSFitResult:          # PartitionedLS.jl:29-49
    α: np.ndarray
    β: np.ndarray
    t: float
    P: np.ndarray

    @property
    def alpha(self):
        return self.α

    @property
    def beta(self):
        return self.β


class Report(dict):
    """The NamedTuple third element of fit's result: .opt (all), .nopen (BnB), .solutions (Opt, returnAllSolutions)."""
    __getattr__ = dict.__getitem__


def library_path():
    return L.SO_PATH


def build_library(force=False):
    return L.build(force)


def _check(st, tolerate=()):
    """Raise on a non-zero status, except one the caller handles itself (it gets the status back)."""
    if st != L.OK and st not in tolerate:
        raise PartlsError(st, L.lib().partls_last_error().decode())
    return st


class IllConditionedWarning(UserWarning):
    """The returned model failed the data-space KKT check (PARTLS_ERR_ILL_CONDITIONED): the fp64 Gram form cannot resolve this X."""


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _inputs(X, y, P, f32=True):
    """host X, y (or None), P as the library takes them — the ONE place that decides dtype and layout.  X: a float32 array stays float32
    where the entry has a float32 form (f32), every other dtype becomes float64; F-contiguous either way (a C-ordered or
    strided input is copied, never widened; an array already in that form is returned as it is).  y: float64.  P: F-contiguous int64.
    A sparse X never gets here on a supported path (_csr marshals it): an entry that takes a dense X only refuses it."""
    _no_sparse("this entry point takes a dense X", X, "use fit / predict / Context.opt_prepare_csr / Context.predict_csr, or densify X yourself")
    xt = np.float32 if f32 and getattr(X, "dtype", None) == np.float32 else np.float64
    return (np.asfortranarray(X, dtype=xt), None if y is None else np.ascontiguousarray(y, dtype=np.float64),
            np.asfortranarray(P, dtype=np.int64))


class CSR(NamedTuple):
    """A sparse design matrix in CSR, for callers without scipy: row i holds data[indptr[i]:indptr[i+1]] in the columns
    indices[indptr[i]:indptr[i+1]], which strictly increase within a row (0-based, no duplicates); shape = (N, M).  Any object with
    .tocsr() (every scipy.sparse matrix and array) is accepted wherever this is.  DESIGN.md §4.15."""
    indptr: np.ndarray
    indices: np.ndarray
    data: np.ndarray
    shape: tuple


def _is_sparse(X):
    return isinstance(X, CSR) or hasattr(X, "tocsr")


def _no_sparse(who, X, instead):
    """the entry points that read a dense X only: a sparse X is refused, never densified behind the caller's back"""
    if _is_sparse(X):
        raise NotImplementedError("%s: a sparse X is not supported here; %s (the library never densifies a sparse matrix itself)"
                                  % (who, instead))


def _csr(X, who="fit"):
    """A sparse X as the library takes it — the ONE place that marshals one: canonical CSR (indices sorted within a row, duplicates
    summed: scipy's sum_duplicates; the arrays of a CSR tuple must be canonical already, the library's validation says so otherwise),
    indptr int64, indices int32, data float64, all contiguous.  float32 values are widened here: nnz numbers, never N x M.  TypeError /
    ValueError as the dense path's for a matrix that is not 2-D or not floating point."""
    if not isinstance(X, CSR):
        A = X.tocsr()
        if A is X:
            A = A.copy()                                     # the caller's matrix is not reordered in place
        A.sum_duplicates()
        X = CSR(A.indptr, A.indices, A.data, tuple(A.shape))
    if len(X.shape) != 2:
        raise TypeError("%s: X must be a matrix and y a vector (MethodError in the reference)" % who)
    N, M = int(X.shape[0]), int(X.shape[1])
    data = np.asarray(X.data)
    if not np.issubdtype(data.dtype, np.floating):
        raise TypeError("%s: X and y must be floating point (X::Array{<:AbstractFloat,2}, Opt.jl:73)" % who)
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(X.indices, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.float64)
    if indptr.shape != (N + 1,) or indices.ndim != 1 or indices.shape != data.shape:
        raise ValueError("%s: a CSR matrix of shape %s needs indptr of length %d and indices / data of one length, got %s, %s, %s"
                         % (who, (N, M), N + 1, indptr.shape, indices.shape, data.shape))
    if int(indptr[-1]) != len(data):                         # the library reads indptr[N] entries of indices and data
        raise ValueError("%s: indptr[N] = %d, but indices / data hold %d entries" % (who, int(indptr[-1]), len(data)))
    return CSR(indptr, indices, data, (N, M))


def _weights(weights, N, who=None):
    """per-row sample weights as the library takes them: a contiguous float64 vector of length N, or None.  who ("fit",
    "cross_validate"): checked in full on the host before any device work — floating, finite, >= 0, sum > 0 (ValueError otherwise)."""
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (N,):
        raise ValueError("weights: expected shape (%d,), got %s" % (N, w.shape))
    if who:
        if not np.issubdtype(np.asarray(weights).dtype, np.floating):
            raise ValueError("%s: weights must be floating point, got %s" % (who, np.asarray(weights).dtype))
        if not np.all(np.isfinite(w)):
            raise ValueError("%s: weights must be finite" % who)
        if np.any(w < 0):
            raise ValueError("%s: weights must be >= 0" % who)
        if not w.sum() > 0:
            raise ValueError("%s: the weights sum to 0" % who)
    return w


def _f32(dtype, who):
    """element type of a device-resident X, declared by the caller: True for float32, False for float64 (or None)"""
    dtype = np.dtype(np.float64 if dtype is None else dtype)
    if dtype not in (np.float64, np.float32):
        raise TypeError("%s: dtype must be float64 or float32, got %s" % (who, dtype))
    return dtype == np.float32


def _many_models(alpha, beta, t, M, K, ranks, who="predict_many"):
    """B models as partls_predict_many takes them: alpha[B, M], beta[B, K], t[B] C-contiguous float64 (row b = model b) and the ranks as
    an int64 vector (None: no order statistics).  ValueError for shapes that do not fit each other, M and K; a rank outside [0, B).
    partls_contributions takes the same models without t (its callers pass zeros); who: the caller's name in the messages."""
    a = np.ascontiguousarray(alpha, dtype=np.float64)
    b = np.ascontiguousarray(beta, dtype=np.float64)
    tv = np.ascontiguousarray(t, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2 or tv.ndim != 1 or a.shape[0] < 1 or a.shape != (tv.shape[0], M) or b.shape != (tv.shape[0], K):
        raise ValueError("%s: expected alpha (B, %d), beta (B, %d) and t (B,) with B >= 1, got %s, %s and %s"
                         % (who, M, K, a.shape, b.shape, tv.shape))
    if ranks is None:
        return a, b, tv, None
    r = np.ascontiguousarray(ranks, dtype=np.int64)
    if r.ndim != 1 or len(r) < 1 or r.min() < 0 or r.max() >= a.shape[0]:
        raise ValueError("%s: ranks must be a non-empty vector of positions in [0, %d)" % (who, a.shape[0]))
    return a, b, tv, r


class _Model:
    """The output set of a call that returns one model: alpha[M], beta[K], t, opt and one int64 (best_index / iters / nopen)."""

    def __init__(self, M, K):
        self.a, self.b = np.zeros(M), np.zeros(K)
        self.t, self.o, self.n = C.c_double(), C.c_double(), C.c_int64()
        self.ptrs = (_dp(self.a), _dp(self.b), C.byref(self.t), C.byref(self.o), C.byref(self.n))     # in the order of the C ABI

    def result(self):
        return self.a, self.b, self.t.value, self.o.value, self.n.value


def _ill(obj, st):
    """status of a call on obj (Context / MultiContext) whose outputs are filled even when it reports PARTLS_ERR_ILL_CONDITIONED
    (include/partls.h): raised, or with obj.tolerate_ill recorded in obj.last_ill"""
    _check(st, (L.ERR_ILL_CONDITIONED,) if obj.tolerate_ill else ())
    obj.last_ill = st == L.ERR_ILL_CONDITIONED


@contextmanager
def _tolerating(on_ill_conditioned, *objs):
    """fit's on_ill_conditioned ("warn": tolerate status 9) holds on objs (Context / MultiContext, or None) inside the block only: what
    their user set comes back on every way out"""
    saved = [(o, o.tolerate_ill) for o in objs if o is not None]
    try:
        for o, _ in saved:
            o.tolerate_ill = on_ill_conditioned == "warn"
        yield
    finally:
        for o, was in saved:
            o.tolerate_ill = was


def _host_fit(obj, entry, X, y, P, eta, *options, all_opt=()):
    """One-call fit of marshalled host float64 inputs on obj (Context / MultiContext): partls_fit_alt, partls_fit_bnb, partls_fit_opt_multi
    and partls_fit_bnb_multi share the argument list up to η, take their options next, write one model (_Model) and, Opt, all_opt last"""
    N, M = X.shape
    K = P.shape[1]
    out = _Model(M, K)
    obj.generation += 1
    _ill(obj, entry(obj._h, X.ctypes.data, N, M, N, y.ctypes.data, P.ctypes.data, K, M, float(eta), *options, *out.ptrs, *all_opt))
    obj._shape = (N, M, K)
    return out.result()


class Context:
    """Thin owner of a partls_ctx (one per device)."""

    def __init__(self, device=0, *, _owner=None, _handle=None):
        """_owner, _handle: a non-owning view of the rank context _handle of the MultiContext _owner (MultiContext.context)"""
        self._h = C.c_void_p(_handle)
        self._owner, self._borrowed = _owner, _owner is not None
        if not self._borrowed:
            _check(L.lib().partls_create(int(device), C.byref(self._h)))
            _live_contexts.add(self)
        self.device = None if self._borrowed else device
        self.generation = 0          # bumped by every prepare: lazily rebuilt results check it (see _Solutions)
        self._tolerate_ill = False
        self.last_ill = False

    @property
    def tolerate_ill(self):
        """True: status 9 (outputs hold the best Gram-form model) is recorded in last_ill instead of raised.  A view has no setting of
        its own: it reads its MultiContext's at every call."""
        return self._tolerate_ill if self._owner is None else self._owner.tolerate_ill

    @tolerate_ill.setter
    def tolerate_ill(self, value):
        if self._owner is not None:
            raise AttributeError("a view takes tolerate_ill from its MultiContext: set it there")
        self._tolerate_ill = bool(value)

    def close(self):
        """Release the device objects now.  Also run for every live context by an atexit hook, i.e. BEFORE interpreter
        finalisation and before the HIP runtime (or a profiler layered on it) tears itself down — a context destroyed later,
        from a module-global's __del__ during exit(), made HIP calls into a dead runtime (round-1 rocprofv3 crash)."""
        if self._h and not self._borrowed:      # a view of a MultiContext's rank does not own the handle
            L.lib().partls_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- staged Opt path -------------------------------------------------------------------------------------------
    def opt_prepare(self, X, y, P, eta=0.0, flags=0, weights=None):
        """X, y: host arrays (any layout; copied F-contiguous).  weights: optional per-row sample weights (host, length N):
        partls_opt_prepare_weighted, after which every staged call on the problem is weighted.
        A float32 X stays float32 — uploaded and read as such through partls_opt_prepare_f32, with or without weights; the results are
        those of X.astype(float64) bit for bit.  Every other dtype is converted to float64; y always is.
        A sparse X (CSR tuple, or anything with .tocsr()) goes through opt_prepare_csr."""
        if _is_sparse(X):
            return self.opt_prepare_csr(X, y, P, eta, flags, weights=weights)
        X, y, P = _inputs(X, y, P)
        N, M = X.shape
        w = _weights(weights, N)
        self._prepare(X.ctypes.data, y.ctypes.data, None if w is None else w.ctypes.data, 0, X.dtype == np.float32, N, M, N, P, eta,
                      flags)

    def opt_prepare_device(self, dX_ptr, dy_ptr, N, M, ldX, P, eta=0.0, flags=0, dw_ptr=None, dtype=np.float64):
        """dX_ptr, dy_ptr (and dw_ptr, optional per-row sample weights, N doubles): raw device addresses (e.g. torch tensor
        .data_ptr()) that stay owned by the caller.  dtype: element type of X — float64, or float32 (a float32 tensor; ldX counts
        elements; y and the weights stay float64): partls_opt_prepare_f32."""
        f32 = _f32(dtype, "opt_prepare_device")
        self._prepare(C.c_void_p(dX_ptr), C.c_void_p(dy_ptr), None if dw_ptr is None else C.c_void_p(dw_ptr), 1, f32, N, M, ldX,
                      np.asfortranarray(P, dtype=np.int64), eta, flags)

    def _prepare(self, xp, yp, wp, on_device, f32, N, M, ldX, P, eta, flags):
        """The one prepare behind opt_prepare and opt_prepare_device.  xp, yp, wp (or None): addresses, on the host or (on_device) in
        HBM; f32: X holds float32 (partls_opt_prepare_f32, weighted or not); P: F-contiguous int64."""
        lib = L.lib()
        head = (self._h, xp, N, M, ldX, yp)
        tail = (on_device, P.ctypes.data, P.shape[1], P.shape[0], float(eta), int(flags))
        self.generation += 1
        if f32:
            _check(lib.partls_opt_prepare_f32(*head, wp, *tail))
        elif wp is None:
            _check(lib.partls_opt_prepare(*head, *tail))
        else:
            _check(lib.partls_opt_prepare_weighted(*head, wp, *tail))
        self._prepared_as(N, M, P.shape[1], on_device)

    def _prepared_as(self, N, M, K, on_device):
        """What the staged calls size their outputs by, recorded once a prepare has SUCCEEDED: a prepare refused by the argument checks
        leaves the library's problem untouched (csrc/prepare.hip: prepare_begin), so it must leave the shape of that problem here too."""
        self._shape = (N, M, K)
        self._on_device = bool(on_device)                    # where the per-row outputs of diagnostics live

    def opt_prepare_csr(self, csr, y, P, eta=0.0, flags=0, weights=None):
        """opt_prepare for a sparse X (a CSR tuple or anything with .tocsr(); host arrays): partls_opt_prepare_csr — X goes up as
        8 (N + 1) + 12 nnz bytes and is never densified; every staged call then works as after a dense prepare."""
        A = _csr(csr, "opt_prepare_csr")
        N, M = A.shape
        y, P = np.ascontiguousarray(y, dtype=np.float64), np.asfortranarray(P, dtype=np.int64)
        if y.shape != (N,) or P.ndim != 2 or P.shape[0] != M:
            raise ValueError("DimensionMismatch: X is %s, y is %s, P is %s" % ((N, M), y.shape, P.shape))
        w = _weights(weights, N)
        self._prepare_csr(A.indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data, y.ctypes.data,
                          None if w is None else w.ctypes.data, 0, N, M, P, eta, flags)

    def opt_prepare_csr_device(self, indptr_ptr, indices_ptr, data_ptr, dy_ptr, N, M, P, eta=0.0, flags=0, dw_ptr=None):
        """the same with the CSR arrays (int64 indptr[N + 1], int32 indices, float64 data), y and the optional weights in HBM: raw device
        addresses that stay owned by the caller and must stay valid while the context holds the problem"""
        self._prepare_csr(C.c_void_p(indptr_ptr), C.c_void_p(indices_ptr), C.c_void_p(data_ptr), C.c_void_p(dy_ptr),
                          None if dw_ptr is None else C.c_void_p(dw_ptr), 1, int(N), int(M), np.asfortranarray(P, dtype=np.int64), eta, flags)

    def _prepare_csr(self, pp, ip, vp, yp, wp, on_device, N, M, P, eta, flags):
        self.generation += 1
        _check(L.lib().partls_opt_prepare_csr(self._h, pp, ip, vp, N, M, yp, wp, on_device, P.ctypes.data, P.shape[1], P.shape[0],
                                              float(eta), int(flags)))
        self._prepared_as(N, M, P.shape[1], on_device)

    def predict_csr(self, csr, P, alpha, beta, t):
        """predict for a sparse X (a CSR tuple or anything with .tocsr(); host arrays): partls_predict_csr.  An empty row gives t."""
        A = _csr(csr, "predict_csr")
        N, M = A.shape
        yh = np.zeros(N)
        self._predict_csr(A.indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data, 0, N, M, np.asfortranarray(P, dtype=np.int64),
                          alpha, beta, t, yh.ctypes.data)
        return yh

    def predict_csr_device(self, indptr_ptr, indices_ptr, data_ptr, N, M, P, alpha, beta, t, dyhat_ptr):
        """the same with the CSR arrays and yhat (N doubles) in HBM: raw device addresses"""
        self._predict_csr(C.c_void_p(indptr_ptr), C.c_void_p(indices_ptr), C.c_void_p(data_ptr), 1, int(N), int(M),
                          np.asfortranarray(P, dtype=np.int64), alpha, beta, t, C.c_void_p(dyhat_ptr))

    def _predict_csr(self, pp, ip, vp, on_device, N, M, P, alpha, beta, t, yhat):
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        b = np.ascontiguousarray(beta, dtype=np.float64)
        _check(L.lib().partls_predict_csr(self._h, pp, ip, vp, N, M, on_device, P.ctypes.data, P.shape[1], P.shape[0], _dp(a), _dp(b),
                                          float(t), yhat))

    def num_patterns(self):
        return int(L.lib().partls_opt_num_patterns(self._h))

    def bit_order(self):
        """(gbit, flip_cost): gbit[k] = Gray-index bit that carries group k in this context's sweeps; flip_cost[k] = measured
        pivots per flip of group k (-1 where the calibration did not run).  Runs the calibration if no sweep has yet."""
        kb = max(self.num_patterns().bit_length() - 1, 0)   # beyond 40 sign bits num_patterns() is 0: the library raises ERR_UNSUPPORTED
        g = np.zeros(kb, dtype=np.int64)
        fc = np.zeros(kb)
        _check(L.lib().partls_opt_bit_order(self._h, _ip(g), _dp(fc)))
        return g, fc

    def opt_sweep(self, g_begin=0, g_end=-1, want_all=False):
        bo = C.c_double()
        bp = C.c_int64()
        nu = C.c_int64()
        allopt = np.full(self.num_patterns(), np.nan) if want_all else None
        _check(L.lib().partls_opt_sweep(self._h, int(g_begin), int(g_end), C.byref(bo), C.byref(bp),
                                        _dp(allopt) if want_all else None, C.byref(nu)))
        return bo.value, bp.value, allopt, nu.value

    def opt_finish(self, pattern):
        out = _Model(*self._shape[1:])
        _ill(self, L.lib().partls_opt_finish(self._h, int(pattern), *out.ptrs))
        return out.result()

    def opt_candidates(self):
        """(obj, pattern) arrays: this context's winner of the last sweep and its near ties (tracked objectives), best first."""
        o = np.zeros(4); p = np.zeros(4, dtype=np.int64); n = C.c_int64()
        _check(L.lib().partls_opt_candidates(self._h, 4, _dp(o), _ip(p), C.byref(n)))
        return o[:n.value].copy(), p[:n.value].copy()

    def opt_merge_candidates(self, objs, pats):
        """Install the merged candidate lists of ALL ranks (same list on every rank): returns the global (objective, pattern) winner;
        the next opt_finish(pattern) re-ranks it against its near ties on the data objective, as a single context would."""
        o = np.ascontiguousarray(objs, dtype=np.float64); p = np.ascontiguousarray(pats, dtype=np.int64)
        wo = C.c_double(); wp = C.c_int64()
        _check(L.lib().partls_opt_merge_candidates(self._h, len(o), _dp(o), _ip(p), C.byref(wo), C.byref(wp)))
        return wo.value, wp.value

    def near_ties_evaluated(self):
        return self._count(L.lib().partls_get_near_ties)

    def opt_pattern(self, pattern):
        N, M, K = self._shape
        ra = np.zeros(M + 1)
        o = C.c_double()
        _check(L.lib().partls_opt_pattern(self._h, int(pattern), _dp(ra), C.byref(o)))
        return ra, o.value

    def opt_models(self, g_begin=0, g_end=-1, raw=False):
        """Models of the Gray-index range [g_begin, g_end) straight from the sweep (partls_opt_models), rows in visiting order:
        dict of numpy arrays pattern[B] (reference index b), opt[B], alpha[B, M], beta[B, K], t[B] (cleanupResult), raw_alpha[B, M+1]
        when raw=True, and the counts n_unconverged (those rows are NaN) and n_vetoes.  Gram-form models (not refined in data space)."""
        N, M, K = self._shape
        B = max(0, (self.num_patterns() if g_end < 0 else int(g_end)) - int(g_begin))
        pat = np.zeros(B, dtype=np.int64)
        opt = np.zeros(B)
        a = np.zeros((B, M))
        b = np.zeros((B, K))
        t = np.zeros(B)
        ra = np.zeros((B, M + 1)) if raw else None
        nu = C.c_int64()
        nv = C.c_int64()
        _check(L.lib().partls_opt_models(self._h, int(g_begin), int(g_end), _ip(pat), _dp(opt), _dp(ra) if raw else None, M + 1,
                                         _dp(a), M, _dp(b), K, _dp(t), C.byref(nu), C.byref(nv)))
        out = dict(pattern=pat, opt=opt, alpha=a, beta=b, t=t, n_unconverged=nu.value, n_vetoes=nv.value)
        if raw:
            out["raw_alpha"] = ra
        return out

    def opt_top(self, k, g_begin=0, g_end=-1, raw=False):
        """The k best patterns of the Gray-index range [g_begin, g_end) and their models, selected on the device (partls_opt_top):
        dict of pattern[c], opt[c], alpha[c, M], beta[c, K], t[c] (raw_alpha[c, M+1] when raw=True), best first — by (opt, pattern),
        -0.0 equal to +0.0, a pattern that hit the pivot cap never listed — with count = c = min(k, converged patterns of the range),
        n_unconverged and n_vetoes.  The rows are opt_models' rows of those patterns (Gram form, not refined in data space)."""
        N, M, K = self._shape
        k = int(k)
        B = max(k, 0)
        pat = np.zeros(B, dtype=np.int64)
        opt = np.zeros(B)
        a = np.zeros((B, M))
        b = np.zeros((B, K))
        t = np.zeros(B)
        ra = np.zeros((B, M + 1)) if raw else None
        cn = C.c_int64()
        nu = C.c_int64()
        nv = C.c_int64()
        _check(L.lib().partls_opt_top(self._h, int(g_begin), int(g_end), k, _ip(pat), _dp(opt), _dp(ra) if raw else None, M + 1,
                                      _dp(a), M, _dp(b), K, _dp(t), C.byref(cn), C.byref(nu), C.byref(nv)))
        c = cn.value
        out = dict(pattern=pat[:c], opt=opt[:c], alpha=a[:c], beta=b[:c], t=t[:c], count=c, n_unconverged=nu.value, n_vetoes=nv.value)
        if raw:
            out["raw_alpha"] = ra[:c]
        return out

    def opt_top_select(self, obj, g0, k):
        """The selection stage of opt_top alone (partls_opt_top_select): obj = objectives of Gray indices g0 .. g0 + len(obj) - 1 of the
        prepared problem -> (index, pattern, opt) of the min(k, non-NaN) best entries in opt_top's order; index = positions in obj."""
        o = np.ascontiguousarray(obj, dtype=np.float64)
        k = int(k)
        B = max(k, 0)
        idx = np.zeros(B, dtype=np.int64)
        pat = np.zeros(B, dtype=np.int64)
        val = np.zeros(B)
        cn = C.c_int64()
        _check(L.lib().partls_opt_top_select(self._h, _dp(o), len(o), int(g0), k, _ip(idx), _ip(pat), _dp(val), C.byref(cn)))
        c = cn.value
        return idx[:c], pat[:c], val[:c]

    def cv_opt(self, X, y, P, fold_ptr, etas, flags=0, device_ptrs=None, weights=None):
        """partls_cv_opt: fit(Opt) on every (fold, η) training set and on all rows, in one call.  X, y: host arrays, or
        device_ptrs=(dX_ptr, dy_ptr, N, ldX[, dw_ptr]) for device-resident inputs (X then ignored; pass X=None).  fold_ptr: F+1 boundaries
        (None or [] for the path only).  weights (host inputs) / dw_ptr (device inputs): optional per-row sample weights
        (partls_cv_opt_weighted).  Returns a dict of column-major results, one problem per column, q = f * E + e: alpha (M x B), beta (K x B),
        t, opt, best_index, heldout_sse, status (all length B)."""
        keep, xp, yp, wp, on_dev, N, ldX, P, fp, F, et, E, B = self._cv_inputs("cv_opt", X, y, P, fold_ptr, etas, device_ptrs, weights)
        M, K = P.shape
        alpha = np.zeros((M, B), order="F")
        beta = np.zeros((K, B), order="F")
        t = np.zeros(B); opt = np.zeros(B); sse = np.zeros(B)
        bi = np.zeros(B, dtype=np.int64)
        stat = np.zeros(B, dtype=np.int32)
        self.generation += 1
        head = (self._h, xp, int(N), int(M), int(ldX), yp)
        tail = (on_dev, P.ctypes.data, K, M, _ip(fp) if F else None, F, _dp(et), E, int(flags), _dp(alpha), M, _dp(beta), K, _dp(t), _dp(opt),
                _ip(bi), _dp(sse), _i32p(stat))
        if wp is None:
            _check(L.lib().partls_cv_opt(*head, *tail))
        else:
            _check(L.lib().partls_cv_opt_weighted(*head, wp, *tail))
        return dict(alpha=alpha, beta=beta, t=t, opt=opt, best_index=bi, heldout_sse=sse, status=stat, F=F, E=E)

    @staticmethod
    def _cv_inputs(who, X, y, P, fold_ptr, etas, device_ptrs, weights):
        """the marshalling cv_opt and cv_alt share: (arrays to keep alive, X / y / w pointers, x_on_device, N, ldX, P, fold_ptr, F, etas, E, B)"""
        wp = None
        keep = None
        if device_ptrs is None:
            X, y, P = _inputs(X, y, P, f32=False)
            N, ldX, on_dev = X.shape[0], X.shape[0], 0
            if X.shape[1] != P.shape[0]:
                raise ValueError("DimensionMismatch: X is %s, P is %s" % (X.shape, P.shape))
            w = _weights(weights, N)
            keep = (X, y, w)
            xp, yp, wp = X.ctypes.data, y.ctypes.data, None if w is None else w.ctypes.data
        else:
            if weights is not None:
                raise ValueError("%s: device inputs take their weights as the fifth entry of device_ptrs" % who)
            P = np.asfortranarray(P, dtype=np.int64)
            dX, dy, N, ldX = device_ptrs[:4]
            xp, yp, on_dev = C.c_void_p(dX), C.c_void_p(dy), 1
            if len(device_ptrs) > 4 and device_ptrs[4] is not None:
                wp = C.c_void_p(device_ptrs[4])
        fp = np.ascontiguousarray([] if fold_ptr is None else fold_ptr, dtype=np.int64)
        F = max(len(fp) - 1, 0)
        et = np.ascontiguousarray(np.atleast_1d(etas), dtype=np.float64)
        E = len(et)
        return keep, xp, yp, wp, on_dev, N, ldX, P, fp, F, et, E, (F + 1) * max(E, 1)

    def cv_alt(self, X, y, P, fold_ptr, etas, alpha0s, beta0s, eps=1e-6, T=100, device_ptrs=None, weights=None, flags=0):
        """partls_cv_alt: the multistart fit(Alt) on every (fold, η) training set and on all rows, in one call; inputs as
        cv_opt, starts as alt_multistart — alpha0s (R, M+1), beta0s (R, K+1), the same R starts for every problem.  Returns cv_opt's dict
        with best_start in place of best_index, plus iters (B) and starts = dict(opt, iters, status), each (B, R): row q = f * E + e,
        column r = start r (meanings: alt_multistart)."""
        keep, xp, yp, wp, on_dev, N, ldX, P, fp, F, et, E, B = self._cv_inputs("cv_alt", X, y, P, fold_ptr, etas, device_ptrs, weights)
        M, K = P.shape
        a0 = np.ascontiguousarray(alpha0s, dtype=np.float64); b0 = np.ascontiguousarray(beta0s, dtype=np.float64)
        if a0.ndim != 2 or b0.ndim != 2 or a0.shape[1] != M + 1 or b0.shape[1] != K + 1 or a0.shape[0] != b0.shape[0]:
            raise ValueError("cv_alt: alpha0s must be (R, %d) and beta0s (R, %d), got %s and %s" % (M + 1, K + 1, a0.shape, b0.shape))
        R = a0.shape[0]
        nR = max(R, 1)
        alpha = np.zeros((M, B), order="F")
        beta = np.zeros((K, B), order="F")
        t = np.zeros(B); opt = np.zeros(B); sse = np.zeros(B)
        it = np.zeros(B, dtype=np.int64); bs = np.zeros(B, dtype=np.int64)
        stat = np.zeros(B, dtype=np.int32)
        oa = np.zeros((B, nR)); ia = np.zeros((B, nR), dtype=np.int64); sa = np.zeros((B, nR), dtype=np.int32)
        self.generation += 1
        _check(L.lib().partls_cv_alt(self._h, xp, int(N), int(M), int(ldX), yp, wp, on_dev, P.ctypes.data, K, M, _ip(fp) if F else None, F,
                                     _dp(et), E, int(flags), float(eps), int(T), R, _dp(a0), M + 1, _dp(b0), K + 1,
                                     _dp(alpha), M, _dp(beta), K, _dp(t), _dp(opt), _ip(it), _ip(bs), _dp(sse), _i32p(stat),
                                     _dp(oa), _ip(ia), _i32p(sa)))
        return dict(alpha=alpha, beta=beta, t=t, opt=opt, iters=it, best_start=bs, heldout_sse=sse, status=stat, F=F, E=E,
                    starts=dict(opt=oa, iters=ia, status=sa))

    def opt_weightings(self, X, y, P, W, eta=0.0, flags=0, device_ptrs=None, oob=True):
        """partls_opt_weightings: fit(Opt) under every column of W (N x B row weightings: bootstrap counts, 0/1 masks, any weights
        that are finite, >= 0 and sum to more than 0 per column) in one call.  X, y, W: host arrays, or
        device_ptrs=(dX_ptr, dy_ptr, N, ldX, dW_ptr, ldW, B) for device-resident float64 inputs (X, y, W then ignored; pass None).
        A float32 X is widened to float64 on the host (this entry has no float32 form).  oob=False skips the out-of-bag pass.
        Returns a dict of column-major results, one problem per column: alpha (M x B), beta (K x B), t, opt, best_index, status,
        oob_sse (NaN where a column has no zero-weight row, the problem failed, or oob=False) and oob_rows (all length B)."""
        if device_ptrs is None:
            X, y, P = _inputs(X, y, P, f32=False)
            N, ldX, on_dev = X.shape[0], X.shape[0], 0
            if X.shape[1] != P.shape[0]:
                raise ValueError("DimensionMismatch: X is %s, P is %s" % (X.shape, P.shape))
            Wf = np.asfortranarray(W, dtype=np.float64)
            if Wf.ndim != 2 or Wf.shape[0] != N or Wf.shape[1] < 1:
                raise ValueError("opt_weightings: W must be (%d, B) with B >= 1, got %s" % (N, Wf.shape))
            B, ldW = Wf.shape[1], N
            xp, yp, wp = X.ctypes.data, y.ctypes.data, Wf.ctypes.data
        else:
            P = np.asfortranarray(P, dtype=np.int64)
            dX, dy, N, ldX, dW, ldW, B = device_ptrs
            xp, yp, wp, on_dev = C.c_void_p(dX), C.c_void_p(dy), C.c_void_p(dW), 1
        M, K = P.shape
        nB = max(int(B), 1)
        alpha = np.zeros((M, nB), order="F")
        beta = np.zeros((K, nB), order="F")
        t = np.zeros(nB); opt = np.zeros(nB); sse = np.full(nB, np.nan)
        bi = np.zeros(nB, dtype=np.int64)
        rows = np.zeros(nB, dtype=np.int64)
        stat = np.zeros(nB, dtype=np.int32)
        self.generation += 1
        _check(L.lib().partls_opt_weightings(self._h, xp, int(N), int(M), int(ldX), yp, on_dev, P.ctypes.data, K, M, wp, int(ldW), int(B),
                                             float(eta), int(flags), _dp(alpha), M, _dp(beta), K, _dp(t), _dp(opt), _ip(bi),
                                             _dp(sse) if oob else None, _ip(rows), _i32p(stat)))
        return dict(alpha=alpha, beta=beta, t=t, opt=opt, best_index=bi, status=stat, oob_sse=sse, oob_rows=rows)

    def alt_prepared(self, alpha0, beta0, eps=1e-6, T=100):
        """Alt on a context prepared with OPT_FAITHFUL_INTERCEPT (e.g. device-resident inputs)."""
        N, M, K = self._shape
        a0 = np.ascontiguousarray(alpha0, dtype=np.float64); b0 = np.ascontiguousarray(beta0, dtype=np.float64)
        out = _Model(M, K)
        _ill(self, L.lib().partls_alt_prepared(self._h, float(eps), int(T), _dp(a0), _dp(b0), *out.ptrs))
        return out.result()

    def alt_multistart(self, alpha0s, beta0s, eps=1e-6, T=100, raise_if_none=True):
        """Alt from R starting points in one batched device call (partls_alt_multistart) on a context prepared with
        OPT_FAITHFUL_INTERCEPT.  alpha0s: (R, M+1), beta0s: (R, K+1), row r = start r.  Returns (alpha, beta, t, opt, iters, best_start,
        starts): the winner as alt_prepared returns a fit, and starts = dict of per-start arrays in start order — opt[R] (Gram-form loss
        of the last iteration), iters[R], status[R] (OK, ERR_NONFINITE for a non-finite starting point, ERR_NOT_CONVERGED), alpha[R, M],
        beta[R, K], t[R]; rows of a failed start are NaN.  When no start finished: PartlsError(ERR_NOT_CONVERGED), or with
        raise_if_none=False the same tuple with NaN for the winner and best_start = -1."""
        N, M, K = self._shape
        a0 = np.ascontiguousarray(alpha0s, dtype=np.float64); b0 = np.ascontiguousarray(beta0s, dtype=np.float64)
        if a0.ndim != 2 or b0.ndim != 2 or a0.shape[1] != M + 1 or b0.shape[1] != K + 1 or a0.shape[0] != b0.shape[0] or a0.shape[0] < 1:
            raise ValueError("alt_multistart: alpha0s must be (R, %d) and beta0s (R, %d) with R >= 1, got %s and %s"
                             % (M + 1, K + 1, a0.shape, b0.shape))
        R = a0.shape[0]
        out = _Model(M, K)
        best = C.c_int64()
        aa = np.zeros((R, M)); ba = np.zeros((R, K)); ta = np.zeros(R); oa = np.zeros(R)
        ia = np.zeros(R, dtype=np.int64); sa = np.zeros(R, dtype=np.int32)
        st = L.lib().partls_alt_multistart(self._h, float(eps), int(T), R, _dp(a0), M + 1, _dp(b0), K + 1, *out.ptrs, C.byref(best),
                                           _dp(aa), M, _dp(ba), K, _dp(ta), _dp(oa), _ip(ia), _i32p(sa))
        if st == L.ERR_NOT_CONVERGED and not raise_if_none:
            self.last_ill = False
        else:
            _ill(self, st)
        return out.result() + (best.value, dict(opt=oa, iters=ia, status=sa, alpha=aa, beta=ba, t=ta))

    def bnb_prepared(self):
        out = _Model(*self._shape[1:])
        _ill(self, L.lib().partls_bnb_prepared(self._h, *out.ptrs))
        return out.result()

    def bnb_bound(self, pats, frees):
        """Bound a batch of BnB nodes (pat[i], free[i]) on a prepared faithful context: (lb[count], branch[count])."""
        pats = np.ascontiguousarray(pats, dtype=np.uint64)
        frees = np.ascontiguousarray(frees, dtype=np.uint64)
        n = len(pats)
        lb = np.zeros(n)
        br = np.zeros(n, dtype=np.int32)
        if n:
            _check(L.lib().partls_bnb_bound(self._h, n, _u64p(pats), _u64p(frees), _dp(lb), _i32p(br)))
        return lb, br

    def bnb_snap_begin(self):
        _check(L.lib().partls_bnb_snap_begin(self._h))

    def bnb_bound_snap(self, pats, frees, src_slots):
        """bnb_bound with tableau snapshots: node i starts from slot src_slots[i] (-1: fresh tableau); returns (lb, branch, dst_slots)."""
        pats = np.ascontiguousarray(pats, dtype=np.uint64)
        frees = np.ascontiguousarray(frees, dtype=np.uint64)
        src = np.ascontiguousarray(src_slots, dtype=np.int32)
        n = len(pats)
        lb = np.zeros(n); br = np.zeros(n, dtype=np.int32); dst = np.full(n, -1, dtype=np.int32)
        if n:
            _check(L.lib().partls_bnb_bound_snap(self._h, n, _u64p(pats), _u64p(frees), _i32p(src), _i32p(dst), _dp(lb), _i32p(br)))
        return lb, br, dst

    def bnb_snap_release(self, slots):
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        if len(sl):
            _check(L.lib().partls_bnb_snap_release(self._h, len(sl), _i32p(sl)))

    def bnb_search(self, max_nodes=0):
        """The BnB search on a prepared faithful context (warm-started node bounds): (mu, pat, free, nodes_bounded)."""
        mu = C.c_double(); pat = C.c_uint64(); fr = C.c_uint64(); nn = C.c_int64()
        _check(L.lib().partls_bnb_search(self._h, int(max_nodes), C.byref(mu), C.byref(pat), C.byref(fr), C.byref(nn)))
        return mu.value, pat.value, fr.value, nn.value

    def bnb_leaf(self, pat, free):
        out = _Model(*self._shape[1:])
        _ill(self, L.lib().partls_bnb_leaf(self._h, C.c_uint64(int(pat)), C.c_uint64(int(free)), *out.ptrs[:4]))
        return out.result()[:4]

    def predict(self, X, P, alpha, beta, t):
        """yhat = X (P .* alpha) beta .+ t for a host X of any layout (partls_predict).  A float32 X stays float32 — copied F-contiguous
        when it is C-ordered or strided, never widened — and is uploaded and read as such (partls_predict_f32); every
        other dtype is converted to float64.  A sparse X goes through predict_csr."""
        if _is_sparse(X):
            return self.predict_csr(X, P, alpha, beta, t)
        X, _, P = _inputs(X, None, P)
        N, M = X.shape
        yh = np.zeros(N)
        self._predict(X.ctypes.data, 0, X.dtype == np.float32, N, M, N, P, alpha, beta, t, _dp(yh))
        return yh

    def predict_device(self, dX_ptr, N, M, ldX, P, alpha, beta, t, dyhat_ptr, dtype=np.float64):
        """the same with X (N x M, ldX, elements of `dtype`: float64 or float32) and yhat (N doubles) in HBM: raw device addresses"""
        self._predict(C.c_void_p(dX_ptr), 1, _f32(dtype, "predict_device"), int(N), int(M), int(ldX), np.asfortranarray(P, dtype=np.int64),
                      alpha, beta, t, C.c_void_p(dyhat_ptr))

    def _predict(self, xp, on_device, f32, N, M, ldX, P, alpha, beta, t, yhat):
        """The one predict behind predict and predict_device: xp and yhat are addresses on the host or (on_device) in HBM"""
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        b = np.ascontiguousarray(beta, dtype=np.float64)
        lib = L.lib()
        if on_device:
            fn = lib.partls_predict_device_f32 if f32 else lib.partls_predict_device
        else:
            fn = lib.partls_predict_f32 if f32 else lib.partls_predict
        _check(fn(self._h, xp, N, M, ldX, P.ctypes.data, P.shape[1], M, _dp(a), _dp(b), float(t), yhat))

    def predict_many(self, X, P, alpha, beta, t, *, ranks=None, want_yhat=True, want_mean=False):
        """The predictions of B models over one partition P in one upload of a host X (partls_predict_many).
        alpha[B, M], beta[B, K], t[B]: row b = model b.  Returns dict(yhat, stats, mean): yhat[N, B] (None unless want_yhat), column b
        = predict with model b bit for bit; stats[N, len(ranks)] (None without ranks), column q = the value at 0-based position
        ranks[q] of each row's ascending sort of its B predictions; mean[N] (None unless want_mean), summed over b = 0 .. B-1 in that
        order.  Without want_yhat no N x B array exists on the host.  X as in predict: float32 stays float32."""
        X, _, P = _inputs(X, None, P)
        N, M = X.shape
        a, b, tv, r = _many_models(alpha, beta, t, M, P.shape[1], ranks)
        B = a.shape[0]
        yh = np.zeros((N, B), order="F") if want_yhat else None
        st = None if r is None else np.zeros((N, len(r)), order="F")
        mu = np.zeros(N) if want_mean else None
        self._predict_many(X.ctypes.data, 0, X.dtype == np.float32, N, M, N, P, a, b, tv, None if yh is None else yh.ctypes.data, N, r,
                           None if st is None else st.ctypes.data, None if mu is None else mu.ctypes.data)
        return dict(yhat=yh, stats=st, mean=mu)

    def predict_many_device(self, dX_ptr, N, M, ldX, P, alpha, beta, t, *, dyhat_ptr=None, ldY=0, ranks=None, dstats_ptr=None,
                            dmean_ptr=None, dtype=np.float64):
        """the same with X (N x M, ldX, elements of `dtype`: float64 or float32) and every wanted output in HBM, as raw device
        addresses: dyhat_ptr (N x B doubles, column-major, leading dimension ldY >= N; rows N .. ldY are not written), dstats_ptr
        (N x len(ranks), leading dimension N; wanted exactly when ranks is given), dmean_ptr (N)"""
        f32 = _f32(dtype, "predict_many_device")
        P = np.asfortranarray(P, dtype=np.int64)
        a, b, tv, r = _many_models(alpha, beta, t, int(M), P.shape[1], ranks)
        if (r is None) != (dstats_ptr is None):
            raise ValueError("predict_many_device: dstats_ptr goes with ranks")
        self._predict_many(C.c_void_p(dX_ptr), 1, f32, int(N), int(M), int(ldX), P, a, b, tv,
                           None if dyhat_ptr is None else C.c_void_p(dyhat_ptr), int(ldY), r,
                           None if dstats_ptr is None else C.c_void_p(dstats_ptr), None if dmean_ptr is None else C.c_void_p(dmean_ptr))

    def _predict_many(self, xp, on_device, f32, N, M, ldX, P, a, b, tv, yhat, ldY, ranks, stats, mean):
        """The one call behind predict_many and predict_many_device: xp and the outputs (or None) are addresses on the host or
        (on_device) in HBM; a[B, M], b[B, K], tv[B] C-contiguous float64 (the M x B / K x B column-major layouts of the ABI); ranks:
        int64 vector or None"""
        lib = L.lib()
        fn = lib.partls_predict_many_f32 if f32 else lib.partls_predict_many
        _check(fn(self._h, xp, N, M, ldX, on_device, P.ctypes.data, P.shape[1], M, a.shape[0], _dp(a), _dp(b), _dp(tv), yhat, ldY,
                  0 if ranks is None else len(ranks), None if ranks is None else _ip(ranks), stats, mean))

    def contributions(self, X, P, alpha, beta, *, ranks=None, want_contrib=True, want_mean=False, want_sums=False):
        """The group contributions c[i, k, b] = beta[b, k] sum over the features m of group k of alpha[b, m] X[i, m] of B models over one
        partition P, in one upload of a host X (partls_contributions): one fma chain per (row, group, model) over
        the group's features in ascending m; the intercept is part of no contribution.  alpha[B, M], beta[B, K]: row b = model b.
        Returns dict(contrib, stats, mean, sums), all F-ordered: contrib[N, K, B] (None unless want_contrib), slab b = the call with
        model b alone bit for bit; stats[N, K, len(ranks)] (None without ranks), [i, k, q] = the value at 0-based position ranks[q] of
        the ascending sort of c[i, k, :]; mean[N, K] (None unless want_mean), summed over b in index order; sums[3, K, B] (None unless
        want_sums): over the rows, the sums of c, |c| and c^2, in an order that depends on N alone.  Without want_contrib no N x K x B
        array exists on the host.  X as in predict: float32 stays float32; a sparse X is refused (NotImplementedError)."""
        _no_sparse("Context.contributions", X, "densify X yourself")
        X, _, P = _inputs(X, None, P)
        N, M = X.shape
        K = P.shape[1]
        a, b, _, r = _many_models(alpha, beta, np.zeros(np.shape(alpha)[:1]), M, K, ranks, "contributions")
        B = a.shape[0]
        ct = np.zeros((N, K, B), order="F") if want_contrib else None
        st = None if r is None else np.zeros((N, K, len(r)), order="F")
        mu = np.zeros((N, K), order="F") if want_mean else None
        sm = np.zeros((3, K, B), order="F") if want_sums else None
        self._contributions(X.ctypes.data, 0, X.dtype == np.float32, N, M, N, P, a, b, None if ct is None else ct.ctypes.data, N, r,
                            None if st is None else st.ctypes.data, None if mu is None else mu.ctypes.data, sm)
        return dict(contrib=ct, stats=st, mean=mu, sums=sm)

    def contributions_device(self, dX_ptr, N, M, ldX, P, alpha, beta, *, dcontrib_ptr=None, ldC=0, ranks=None, dstats_ptr=None,
                             dmean_ptr=None, want_sums=False, dtype=np.float64):
        """the same with X (N x M, ldX, elements of `dtype`: float64 or float32) and every wanted array output in HBM, as raw device
        addresses: dcontrib_ptr (N x K x B doubles, element (i, k, b) at i + ldC (k + K b), ldC >= N; rows N .. ldC are not
        written), dstats_ptr (N x K x len(ranks), leading dimension N; wanted exactly when ranks is given), dmean_ptr (N x K).
        Returns sums[3, K, B] on the host when want_sums, else None."""
        f32 = _f32(dtype, "contributions_device")
        P = np.asfortranarray(P, dtype=np.int64)
        a, b, _, r = _many_models(alpha, beta, np.zeros(np.shape(alpha)[:1]), int(M), P.shape[1], ranks, "contributions_device")
        if (r is None) != (dstats_ptr is None):
            raise ValueError("contributions_device: dstats_ptr goes with ranks")
        sm = np.zeros((3, P.shape[1], a.shape[0]), order="F") if want_sums else None
        self._contributions(C.c_void_p(dX_ptr), 1, f32, int(N), int(M), int(ldX), P, a, b,
                            None if dcontrib_ptr is None else C.c_void_p(dcontrib_ptr), int(ldC), r,
                            None if dstats_ptr is None else C.c_void_p(dstats_ptr), None if dmean_ptr is None else C.c_void_p(dmean_ptr), sm)
        return sm

    def _contributions(self, xp, on_device, f32, N, M, ldX, P, a, b, contrib, ldC, ranks, stats, mean, sums):
        """The one call behind contributions and contributions_device: xp, contrib, stats and mean (or None) are addresses on the host
        or (on_device) in HBM; a[B, M], b[B, K] C-contiguous float64 (the M x B / K x B column-major layouts of the ABI, leading
        dimensions M and K); ranks: int64 vector or None; sums: a host float64 array of 3 K B elements or None"""
        lib = L.lib()
        fn = lib.partls_contributions_f32 if f32 else lib.partls_contributions
        K = P.shape[1]
        _check(fn(self._h, xp, N, M, ldX, on_device, P.ctypes.data, K, M, a.shape[0], _dp(a), M, _dp(b), K, contrib, ldC,
                  0 if ranks is None else len(ranks), None if ranks is None else _ip(ranks), stats, mean, None if sums is None else _dp(sums)))

    _DIAG_ROWS = ("leverage", "loo", "studentized", "cooks", "residual")

    def diagnostics(self, alpha, beta, t, *, rows=_DIAG_ROWS, want_se=True):
        """Regression diagnostics of the model (alpha[M], beta[K], t) on the problem this context is prepared for, from HOST arrays
        (opt_prepare): partls_diagnostics, DESIGN.md §4.17.  Returns a dict: the per-row arrays named in `rows` (of leverage, loo,
        studentized, cooks, residual; N doubles each), se_w[M + 1] and se_beta[K] (unless want_se is False), active[M + 1] (bool) and
        summary[lowlevel.DIAG_NSUM] (indices lowlevel.DIAG_*).  The prepared problem is untouched."""
        if getattr(self, "_on_device", False):
            raise ValueError("Context.diagnostics: the problem was prepared from device pointers; its per-row outputs are device "
                             "arrays (diagnostics_device)")
        bad = [r for r in rows if r not in self._DIAG_ROWS]
        if bad:
            raise ValueError("Context.diagnostics: unknown per-row output %r (known: %s)" % (bad[0], ", ".join(self._DIAG_ROWS)))
        N = self._diag_shape("Context.diagnostics")[0]
        out = {r: np.zeros(N) for r in rows}
        out.update(self._diagnostics(alpha, beta, t, {r: a.ctypes.data for r, a in out.items()}, want_se))
        return out

    def diagnostics_device(self, alpha, beta, t, *, dleverage_ptr=None, dloo_ptr=None, dstudentized_ptr=None, dcooks_ptr=None,
                           dresidual_ptr=None, want_se=True):
        """the same on a problem prepared from DEVICE pointers (opt_prepare_device): the per-row outputs that are wanted are raw device
        addresses of N doubles each; returns dict(se_w, se_beta, active, summary) on the host"""
        if not getattr(self, "_on_device", True):
            raise ValueError("Context.diagnostics_device: the problem was prepared from host arrays; its per-row outputs are host "
                             "arrays (diagnostics)")
        self._diag_shape("Context.diagnostics_device")
        ptrs = dict(zip(self._DIAG_ROWS, (dleverage_ptr, dloo_ptr, dstudentized_ptr, dcooks_ptr, dresidual_ptr)))
        return self._diagnostics(alpha, beta, t, {r: int(a) for r, a in ptrs.items() if a is not None}, want_se)

    def _diag_shape(self, who):
        shape = getattr(self, "_shape", None)
        if shape is None:
            raise ValueError("%s: no prepared problem on this context" % who)
        return shape

    def _diagnostics(self, alpha, beta, t, rows, want_se):
        """The one call behind diagnostics and diagnostics_device: rows maps the names of the wanted per-row outputs to addresses, on the
        host or in HBM as the prepare was"""
        _, M, K = self._shape
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        b = np.ascontiguousarray(beta, dtype=np.float64)
        if a.shape != (M,) or b.shape != (K,):
            raise ValueError("diagnostics: expected alpha (%d,) and beta (%d,), got %s and %s" % (M, K, a.shape, b.shape))
        if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.isfinite(t)):
            raise ValueError("diagnostics: the model has a NaN / Inf in alpha, beta or t")
        se_w, se_b = (np.zeros(M + 1), np.zeros(K)) if want_se else (None, None)
        active, summary = np.zeros(M + 1, dtype=np.int32), np.zeros(L.DIAG_NSUM)
        _check(L.lib().partls_diagnostics(self._h, _dp(a), _dp(b), float(t), *(rows.get(r) for r in self._DIAG_ROWS),
                                          None if se_w is None else _dp(se_w), None if se_b is None else _dp(se_b), _i32p(active),
                                          _dp(summary)))
        return dict(se_w=se_w, se_beta=se_b, active=active.astype(bool), summary=summary)

    def diagnostics_timing(self):
        """(leverage kernel, host factorisation, whole call) of the last diagnostics call on this context, in ms"""
        ms = [C.c_double() for _ in range(3)]
        _check(L.lib().partls_get_diagnostics_timing(self._h, *(C.byref(m) for m in ms)))
        return tuple(m.value for m in ms)

    # ---- robust fits ----------------------------------------------------------------------------------
    def robust_weights(self, alpha, beta, t, *, loss="huber", c=None, scale=None, want_weights=True):
        """The row weights of a Huber or bisquare loss at the model (alpha[M], beta[K], t) on the problem this context is prepared for,
        from HOST arrays (opt_prepare): partls_robust_weights, DESIGN.md §4.18.  c: the tuning constant (None: 1.345 / 4.685);
        scale: a positive float holds the residual scale fixed, None (or "mad") estimates it as median |residual| / 0.6745.
        Returns a dict: weights[N] (None unless want_weights, or when scale is 0), scale, rho_sum, max_dw (against the previous
        call's weights since the last prepare; all ones when there was none), n_down, n_zero.  scale == 0 (at least half of the rows
        are fitted exactly): no weights were formed.  The prepared problem is untouched."""
        if getattr(self, "_on_device", False):
            raise ValueError("Context.robust_weights: the problem was prepared from device pointers; its weights are a device "
                             "array (robust_weights_device)")
        N = self._diag_shape("Context.robust_weights")[0]
        w = np.zeros(N) if want_weights else None
        out = self._robust_weights(alpha, beta, t, loss, c, scale, None if w is None else w.ctypes.data)
        out["weights"] = w if out["scale"] != 0.0 else None
        return out

    def robust_weights_device(self, alpha, beta, t, *, loss="huber", c=None, scale=None, dw_ptr=None):
        """the same on a problem prepared from DEVICE pointers (opt_prepare_device): dw_ptr (optional) is the raw device address of N
        doubles that receive the weights; returns the dict without weights"""
        if not getattr(self, "_on_device", True):
            raise ValueError("Context.robust_weights_device: the problem was prepared from host arrays; its weights are a host "
                             "array (robust_weights)")
        self._diag_shape("Context.robust_weights_device")
        return self._robust_weights(alpha, beta, t, loss, c, scale, None if dw_ptr is None else C.c_void_p(dw_ptr))

    def _robust_weights(self, alpha, beta, t, loss, c, scale, w_out):
        """The one call behind robust_weights and robust_weights_device: w_out (or None) is an address on the host or in HBM, as the
        prepare was"""
        _, M, K = self._shape
        code, cv, sv = _robust_options(loss, c, scale, "robust_weights")
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        b = np.ascontiguousarray(beta, dtype=np.float64)
        if a.shape != (M,) or b.shape != (K,):
            raise ValueError("robust_weights: expected alpha (%d,) and beta (%d,), got %s and %s" % (M, K, a.shape, b.shape))
        s, rho, dw = C.c_double(), C.c_double(), C.c_double()
        nd, nz = C.c_int64(), C.c_int64()
        _check(L.lib().partls_robust_weights(self._h, _dp(a), _dp(b), float(t), code, cv, sv, C.byref(s), C.byref(rho), C.byref(dw),
                                             C.byref(nd), C.byref(nz), w_out))
        return dict(scale=s.value, rho_sum=rho.value, max_dw=dw.value, n_down=nd.value, n_zero=nz.value)

    def opt_reweight(self, weights=None):
        """New sample weights for the prepared problem, X untouched (partls_opt_reweight): weights[N] (host; the rules
        of opt_prepare's weights), or None for the weights of the last robust_weights call on this context.  Afterwards the context
        is in the state opt_prepare(..., weights=weights) would leave it in, bit for bit; nothing but a host weights vector is
        uploaded.  A refusal leaves the context unprepared."""
        N = self._diag_shape("Context.opt_reweight")[0]
        w = _weights(weights, N)
        self.generation += 1
        _check(L.lib().partls_opt_reweight(self._h, None if w is None else w.ctypes.data, 0))

    def opt_reweight_device(self, dw_ptr):
        """the same with the weights in HBM: the raw device address of N doubles, which stay owned by the caller and must stay valid
        while the context holds the problem"""
        self._diag_shape("Context.opt_reweight_device")
        self.generation += 1
        _check(L.lib().partls_opt_reweight(self._h, C.c_void_p(dw_ptr), 1))

    def robust_timing(self):
        """(residual pass, selection of the median, weight kernel) of the last robust_weights call on this context, in ms of device time"""
        ms = [C.c_double() for _ in range(3)]
        _check(L.lib().partls_get_robust_timing(self._h, *(C.byref(m) for m in ms)))
        return tuple(m.value for m in ms)

    # ---- generalised linear fits ----------------------------------------------------------------------
    def glm_working(self, model=None, family="binomial", *, want_rows=True):
        """The working rows of a family ("binomial": logit link; "poisson": log link) at a model on the problem this context is prepared
        for, from HOST arrays (opt_prepare): partls_glm_working, DESIGN.md §4.19.  model: None for the start (eta from y alone, as
        R's glm.fit), a (alpha[M], beta[K], t) triple or a fit result.  The response is the one the problem was prepared with, whatever
        opt_rework installed since.  Returns a dict: deviance, max_abs_eta (before the clamp at +-30), n_clamped and (unless
        want_rows is False) weights[N], working_response[N], mu[N].  The prepared problem is untouched."""
        if getattr(self, "_on_device", False):
            raise ValueError("Context.glm_working: the problem was prepared from device pointers; its rows are device arrays "
                             "(glm_working_device)")
        N = self._diag_shape("Context.glm_working")[0]
        rows = [np.zeros(N) for _ in range(3)] if want_rows else [None] * 3
        out = self._glm_working(model, family, *(None if r is None else r.ctypes.data for r in rows))
        out.update(weights=rows[0], working_response=rows[1], mu=rows[2])
        return out

    def glm_working_device(self, model=None, family="binomial", *, dw_ptr=None, dz_ptr=None, dmu_ptr=None):
        """the same on a problem prepared from DEVICE pointers (opt_prepare_device): dw_ptr, dz_ptr, dmu_ptr (each optional) are raw
        device addresses of N doubles that receive the rows; returns the dict without rows"""
        if not getattr(self, "_on_device", True):
            raise ValueError("Context.glm_working_device: the problem was prepared from host arrays; its rows are host arrays "
                             "(glm_working)")
        self._diag_shape("Context.glm_working_device")
        return self._glm_working(model, family, *(None if q is None else C.c_void_p(q) for q in (dw_ptr, dz_ptr, dmu_ptr)))

    def _glm_working(self, model, family, w_out, z_out, mu_out):
        """The one call behind glm_working and glm_working_device: the row outputs (or None) are addresses on the host or in HBM, as the
        prepare was"""
        _, M, K = self._shape
        code = _glm_family(family, "glm_working")
        a = b = None
        t = 0.0
        if model is not None:
            alpha, beta, t = (model.α, model.β, model.t) if hasattr(model, "α") else model
            a = np.ascontiguousarray(alpha, dtype=np.float64)
            b = np.ascontiguousarray(beta, dtype=np.float64)
            if a.shape != (M,) or b.shape != (K,):
                raise ValueError("glm_working: expected alpha (%d,) and beta (%d,), got %s and %s" % (M, K, a.shape, b.shape))
        dev, em, nc = C.c_double(), C.c_double(), C.c_int64()
        _check(L.lib().partls_glm_working(self._h, None if a is None else _dp(a), None if b is None else _dp(b), float(t), code,
                                          C.byref(dev), C.byref(em), C.byref(nc), w_out, z_out, mu_out))
        return dict(deviance=dev.value, max_abs_eta=em.value, n_clamped=nc.value)

    def opt_rework(self, w=None, z=None):
        """New sample weights AND a new response for the prepared problem, X untouched (partls_opt_rework): w[N], z[N]
        (host), or neither for the rows of the last glm_working call on this context; w alone is opt_reweight(w).  Afterwards the
        context is in the state opt_prepare(X, z, ..., weights=w) would leave it in, bit for bit, except that glm_working still reads
        the response of the first prepare; nothing but host w / z is uploaded.  A refusal leaves the context unprepared."""
        N = self._diag_shape("Context.opt_rework")[0]
        if w is None and z is not None:
            raise ValueError("Context.opt_rework: z is given without w")
        wv = _weights(w, N)
        zv = None
        if z is not None:
            zv = np.ascontiguousarray(z, dtype=np.float64)
            if zv.shape != (N,):
                raise ValueError("Context.opt_rework: z must have %d entries, got %s" % (N, zv.shape))
        self.generation += 1
        _check(L.lib().partls_opt_rework(self._h, None if wv is None else wv.ctypes.data, None if zv is None else zv.ctypes.data, 0))

    def opt_rework_device(self, dw_ptr, dz_ptr=None):
        """the same with the rows in HBM: raw device addresses of N doubles each, which stay owned by the caller and must stay valid
        while the context holds the problem"""
        self._diag_shape("Context.opt_rework_device")
        self.generation += 1
        _check(L.lib().partls_opt_rework(self._h, C.c_void_p(dw_ptr), None if dz_ptr is None else C.c_void_p(dz_ptr), 1))

    def glm_mean(self, family, eta):
        """mu = the inverse link of the family at eta (host array), by the device function of the working rows, clamp included
        (partls_glm_mean)"""
        code = _glm_family(family, "glm_mean")
        e = np.ascontiguousarray(eta, dtype=np.float64).reshape(-1)
        mu = np.zeros(e.shape[0])
        if e.shape[0]:
            _check(L.lib().partls_glm_mean(self._h, code, e.ctypes.data, e.shape[0], 0, mu.ctypes.data))
        return mu

    def glm_mean_device(self, family, deta_ptr, N, dmu_ptr):
        """the same with eta and mu (N doubles each) in HBM: raw device addresses"""
        _check(L.lib().partls_glm_mean(self._h, _glm_family(family, "glm_mean_device"), C.c_void_p(deta_ptr), int(N), 1, C.c_void_p(dmu_ptr)))

    def glm_timing(self):
        """(residual pass, row kernel) of the last glm_working call on this context, in ms of device time"""
        ms = [C.c_double() for _ in range(2)]
        _check(L.lib().partls_get_glm_timing(self._h, *(C.byref(m) for m in ms)))
        return tuple(m.value for m in ms)

    def _count(self, getter):
        n = C.c_int64()
        _check(getter(self._h, C.byref(n)))
        return n.value

    def timing(self, which):
        ms = C.c_double()
        _check(L.lib().partls_get_timing(self._h, int(which), C.byref(ms)))
        return ms.value

    def upload(self):
        """(ms, bytes) of the host -> device upload of X inside the last prepare / fit (0, 0: device-resident inputs)"""
        ms = C.c_double(); b = C.c_double()
        _check(L.lib().partls_get_upload(self._h, C.byref(ms), C.byref(b)))
        return ms.value, b.value

    def pivots(self):
        return self._count(L.lib().partls_get_pivots)

    def vetoes(self):
        return self._count(L.lib().partls_get_vetoes)

    def rescue_stats(self):
        """lowlevel.OPT_RESCUE_CAPPED: Report(rescued, pivots, failed) of the rescue kernel in the last opt_sweep, opt_models or opt_top
        and the opt_finish / opt_pattern calls since (include/partls.h: partls_get_rescue_stats)"""
        r = C.c_int64(); p = C.c_int64(); f = C.c_int64()
        _check(L.lib().partls_get_rescue_stats(self._h, C.byref(r), C.byref(p), C.byref(f)))
        return Report(rescued=r.value, pivots=p.value, failed=f.value)

    def blocks(self):
        """pivot blocks of the cooperative kernel in the last single-node solve (0: the solve ran on another kernel)"""
        return self._count(L.lib().partls_get_blocks)

    def sweep_route(self):
        """(kernel, T): the sweep kernel of the prepared problem (or of the last cv_opt's problems) — L.ROUTE_REG_256, ROUTE_REG_512,
        ROUTE_DEFERRED or ROUTE_EAGER — and its tile count on the register kernels, 0 otherwise (include/partls.h: partls_get_sweep_route)"""
        k = C.c_int(); t = C.c_int()
        _check(L.lib().partls_get_sweep_route(self._h, C.byref(k), C.byref(t)))
        return k.value, t.value

    def kkt_violation(self):
        """data-space KKT violation of the last finished winner (include/partls.h: partls_get_kkt_violation)"""
        v = C.c_double()
        _check(L.lib().partls_get_kkt_violation(self._h, C.byref(v), None))
        return v.value

    def min_pivot(self):
        """smallest leave-one-out pivot of the last finished model's basis (lower bound of 1 / cond of its Gram block)"""
        v = C.c_double(); mp = C.c_double()
        _check(L.lib().partls_get_kkt_violation(self._h, C.byref(v), C.byref(mp)))
        return mp.value

    def gram(self):
        N, M, K = self._shape
        G = np.zeros((M + 2, M + 2), order="F")
        _check(L.lib().partls_get_gram(self._h, _dp(G)))
        return G

    def synth_device(self, seed, N, D, wstar, dX_ptr, dy_ptr):
        ws = np.ascontiguousarray(wstar, dtype=np.float64)
        _check(L.lib().partls_synth_device(self._h, C.c_uint64(seed), N, D, _dp(ws), C.c_void_p(dX_ptr), C.c_void_p(dy_ptr)))


class Frontier:
    """The frontier of the BnB search as a native object (include/partls.h: partls_frontier_*): pops and deals rounds of nodes,
    ingests the ranks' (bound, branch, snapshot slot) triples, keeps the snapshot reference counts.  dist.bnb_search_warm drives it."""

    def __init__(self, n_groups, rank=0, world=1, batch=1024):
        self._h = C.c_void_p()
        _check(L.lib().partls_frontier_create(int(n_groups), int(rank), int(world), int(batch), C.byref(self._h)))
        self.world, self.batch = int(world), int(batch)
        self._pat = np.zeros(self.batch, dtype=np.uint64); self._free = np.zeros(self.batch, dtype=np.uint64)
        self._src = np.zeros(self.batch, dtype=np.int32); self._per = np.zeros(self.world, dtype=np.int32)
        self._dead = np.zeros(4 * self.batch * self.world + 64, dtype=np.int32)

    def close(self):
        if self._h:
            L.lib().partls_frontier_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def next(self):
        """(total, pats, frees, src_slots, per_rank): this rank's share of the next round (views valid until the next call)"""
        tot = C.c_int64(); mine = C.c_int64()
        _check(L.lib().partls_frontier_next(self._h, C.byref(tot), C.byref(mine), _u64p(self._pat), _u64p(self._free), _i32p(self._src),
                                            _i32p(self._per)))
        m = mine.value
        return tot.value, self._pat[:m], self._free[:m], self._src[:m], self._per.copy()

    def ingest(self, lb, branch, dst):
        """results of the whole round in rank-major order; returns this rank's dead snapshot slots"""
        lb = np.ascontiguousarray(lb, dtype=np.float64); br = np.ascontiguousarray(branch, dtype=np.int32)
        ds = np.ascontiguousarray(dst, dtype=np.int32)
        nd = C.c_int64()
        _check(L.lib().partls_frontier_ingest(self._h, _dp(lb), _i32p(br), _i32p(ds), _i32p(self._dead), len(self._dead), C.byref(nd)))
        return self._dead[:nd.value].copy()

    def result(self):
        mu = C.c_double(); pat = C.c_uint64(); fr = C.c_uint64(); nn = C.c_int64()
        _check(L.lib().partls_frontier_result(self._h, C.byref(mu), C.byref(pat), C.byref(fr), C.byref(nn)))
        return mu.value, pat.value, fr.value, nn.value


class MultiContext:
    """Owner of a partls_multi: fit(Opt) and fit(BnB) sharded over several GPUs of one node inside the library (one host thread and
    one context per device; include/partls.h: partls_fit_opt_multi, partls_fit_bnb_multi).  devices: None = every visible device, an
    int n = devices 0..n-1, or a list of device indices (a list naming a device twice rehearses the R-rank control flow on one GPU:
    the Gram sum of its row blocks then runs through the host instead of RCCL)."""

    def __init__(self, devices=None):
        self._h = C.c_void_p()
        if devices is None:
            arr, n = None, 0
        elif isinstance(devices, (int, np.integer)):
            arr, n = None, int(devices)
        else:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            n = len(devices)
        _check(L.lib().partls_multi_create(arr, n, C.byref(self._h)))
        self.generation = 0          # bumped by every fit (see _Solutions)
        self.devices = [int(d) for d in devices] if arr is not None else list(range(self.size))
        self.tolerate_ill = False
        self.last_ill = False
        self._views = weakref.WeakSet()
        _live_contexts.add(self)

    def close(self):
        if self._h:
            # the rank contexts die with the handle: views of them must not keep the raw pointers (a _Solutions object built on one
            # notices the generation change and prepares its problem again on a context of its own)
            self.generation += 1
            for v in list(self._views):
                v._h = C.c_void_p()
            L.lib().partls_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return int(L.lib().partls_multi_size(self._h))

    @property
    def uses_rccl(self):
        return bool(L.lib().partls_multi_uses_rccl(self._h))

    def context(self, rank=0):
        """Non-owning view of rank r's context (rank 0 holds the fitted problem: opt_finish / opt_pattern work on it)."""
        h = L.lib().partls_multi_context(self._h, int(rank))
        if not h:
            raise IndexError("rank out of range")
        view = Context(_owner=self, _handle=h)
        self._views.add(view)
        return view

    def fit_opt(self, X, y, P, eta=0.0, flags=0, want_all=False):
        X, y, P = _inputs(X, y, P, f32=False)
        allopt = np.full(1 << (P.shape[1] + 1), np.nan) if want_all else None
        return _host_fit(self, L.lib().partls_fit_opt_multi, X, y, P, eta, int(flags),
                         all_opt=(_dp(allopt) if want_all else None,)) + (allopt,)

    def fit_bnb(self, X, y, P, eta=0.0):
        """fit(BnB) with the frontier search sharded over the ranks (include/partls.h: partls_fit_bnb_multi): (alpha, beta, t, opt, nopen)"""
        return _host_fit(self, L.lib().partls_fit_bnb_multi, *_inputs(X, y, P, f32=False), eta)

    def timing(self, rank, which):
        ms = C.c_double()
        _check(L.lib().partls_multi_get_timing(self._h, int(rank), int(which), C.byref(ms)))
        return ms.value


def synth_truth(seed, D, K):
    """Partition matrix and true weights of the BASELINE.md §4 synthetic problem (host side, tiny)."""
    P = np.zeros((D, K), dtype=np.int64, order="F")
    ws = np.zeros(D)
    _check(L.lib().partls_synth_truth(C.c_uint64(seed), D, K, _ip(P), _dp(ws)))
    return P, ws


_default_ctx = {}
_default_multi = {}
_live_contexts = weakref.WeakSet()


@atexit.register
def _close_all_contexts():
    for ctx in list(_live_contexts):
        try:
            ctx.close()
        except Exception:
            pass
    _default_ctx.clear()
    _default_multi.clear()


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def default_multi(devices=None):
    key = devices if devices is None or isinstance(devices, (int, np.integer)) else tuple(int(d) for d in devices)
    if key not in _default_multi:
        _default_multi[key] = MultiContext(devices)
    return _default_multi[key]


# ---------------------------------------------------------------------------------------------------------------------
# L2 helpers the reference exports (PartitionedLS.jl:76-81, :108-123) — shape bookkeeping only, kept for API parity
# ---------------------------------------------------------------------------------------------------------------------
def homogeneousCoords(X, P):
    X = np.asarray(X)
    P = np.asarray(P, dtype=np.int64)
    Xo = np.hstack([X, np.ones((X.shape[0], 1), dtype=X.dtype)])
    Po = np.zeros((P.shape[0] + 1, P.shape[1] + 1), dtype=np.int64)
    Po[:-1, :-1] = P
    Po[-1, -1] = 1
    return Xo, Po


def regularizeProblem(X, y, P, η):
    if η == 0:
        return X, y
    X = np.asarray(X)
    rows = [np.sqrt(η) * (np.asarray(P)[:, k] == 1).astype(X.dtype)[None, :] for k in range(np.asarray(P).shape[1])]
    return np.vstack([X] + rows), np.concatenate([np.asarray(y), np.zeros(len(rows), dtype=X.dtype)])


# ---------------------------------------------------------------------------------------------------------------------
# fit / predict
# ---------------------------------------------------------------------------------------------------------------------
def _fit_inputs(X, y, P, f32=False):
    """fit's and cross_validate's argument checks (the reference's method signatures), then _inputs.  Float32 inputs
    (test/runtests.jl:123-146): y is widened (N numbers), X only where the device path has no float32 form (f32 False); result fields
    are abstract floats in the reference.  A sparse X (fit only) comes back as the marshalled CSR tuple (_csr), under the same checks."""
    y = np.asarray(y)
    P = np.asarray(P)
    sparse = _is_sparse(X)
    X = _csr(X, "fit") if sparse else np.asarray(X)          # (_csr: 2-D and floating, the same two errors)
    if (not sparse and X.ndim != 2) or y.ndim != 1:
        raise TypeError("fit: X must be a matrix and y a vector (MethodError in the reference)")
    if not ((sparse or np.issubdtype(X.dtype, np.floating)) and np.issubdtype(y.dtype, np.floating)):
        raise TypeError("fit: X and y must be floating point (X::Array{<:AbstractFloat,2}, Opt.jl:73)")
    if not np.issubdtype(P.dtype, np.integer) or P.ndim != 2:
        raise TypeError("fit: P must be an integer matrix (P::Array{Int,2})")
    if X.shape[0] != y.shape[0] or P.shape[0] != X.shape[1]:
        raise ValueError("DimensionMismatch: X is %s, y is %s, P is %s" % (tuple(X.shape), y.shape, P.shape))
    if sparse:
        return X, np.ascontiguousarray(y, dtype=np.float64), np.asfortranarray(P, dtype=np.int64)
    return _inputs(X, y, P, f32)


def _generator(rng):
    """rng as fit, cross_validate and cv_folds take it: None (fresh entropy), an int seed, or a numpy Generator (used as it is)"""
    if rng is None or isinstance(rng, (int, np.integer)):
        return np.random.default_rng(None if rng is None else int(rng))
    return rng


def _draw_start(gen, M, K):
    """one starting point of Alt, (alpha0[M+1], beta0[K+1]), as the reference draws it"""
    alpha0 = gen.random(M + 1)                                # Alt.jl:65
    return alpha0, (gen.random(K + 1) - 0.5) * 10             # Alt.jl:66


def _alt_starts(alg, M, K, restarts, alpha0, beta0, rng):
    """The starting points of a multistart fit(Alt) — (alpha0s[R, M+1], beta0s[R, K+1]) — or None for a single fit; every misuse is a
    ValueError here, before any device work.  Drawn starts are R successive single draws (Alt.jl:65-66), so start 0 is the start of the
    single fit with the same rng."""
    nd = [np.ndim(v) for v in (alpha0, beta0) if v is not None]
    if restarts is None and 2 not in nd:
        return None
    if alg is not Alt:
        if restarts is not None:
            raise ValueError("fit: restarts is an option of Alt")
        return None                                           # Opt / BnB ignore alpha0 / beta0, as before
    if restarts is not None:
        if isinstance(restarts, bool) or not isinstance(restarts, (int, np.integer)) or int(restarts) < 1:
            raise ValueError("fit: restarts must be an integer >= 1, got %r" % (restarts,))
        if 1 in nd:
            raise ValueError("fit: restarts with a single starting point (1-D alpha0 / beta0); pass (R, M+1) and (R, K+1) arrays")
    if nd:
        if alpha0 is None or beta0 is None or nd != [2, 2]:
            raise ValueError("fit: explicit starts need alpha0 of shape (R, M+1) and beta0 of shape (R, K+1)")
        a0 = np.ascontiguousarray(alpha0, dtype=np.float64)
        b0 = np.ascontiguousarray(beta0, dtype=np.float64)
        if a0.shape[0] < 1 or a0.shape != (a0.shape[0], M + 1) or b0.shape != (a0.shape[0], K + 1):
            raise ValueError("fit: alpha0 must be (R, %d) and beta0 (R, %d), got %s and %s" % (M + 1, K + 1, a0.shape, b0.shape))
        if restarts is not None and int(restarts) != a0.shape[0]:
            raise ValueError("fit: restarts = %d but %d explicit starts" % (int(restarts), a0.shape[0]))
        if not (np.all(np.isfinite(a0)) and np.all(np.isfinite(b0))):
            raise ValueError("fit: the starting points must be finite")
        return a0, b0
    gen = _generator(rng)
    a0, b0 = zip(*[_draw_start(gen, M, K) for _ in range(int(restarts))])
    return np.array(a0), np.array(b0)


class _Problem(NamedTuple):
    """What a _Solutions object keeps of its fit, to prepare the problem again: the marshalled inputs and the options"""
    X: np.ndarray
    y: np.ndarray
    P: np.ndarray
    eta: float
    flags: int
    device: int
    weights: object = None                 # sample weights of a weighted fit
    on_ill_conditioned: str = "raise"      # of the fit; the default is what a Context does on its own


class _Solutions:
    """returnAllSolutions (Opt.jl:99-101): element b is (opt_b, PartLSFitResult_b); models are rebuilt on demand from the context
    that holds the fitted problem.  They stay valid whatever is fitted afterwards, as in the reference: when a later fit has taken
    the shared context over, the problem is prepared once more on a private context owned by this object."""

    def __init__(self, ctx, all_opt, P, problem):
        self._ctx, self._all, self._P, self._problem = ctx, all_opt, P, _Problem(*problem)
        # a view of a MultiContext's rank 0: the owner counts the fits and holds the tolerance
        self._owner = getattr(ctx, "_owner", None) or ctx
        self._gen = self._owner.generation

    def __len__(self):
        return len(self._all)

    def _context(self):
        if self._owner.generation != self._gen:        # the shared context now holds another problem
            p = self._problem
            self._ctx = self._owner = Context(p.device)
            self._ctx.opt_prepare(p.X, p.y, p.P, p.eta, p.flags, weights=p.weights)
            self._gen = self._ctx.generation
        return self._ctx

    def __getitem__(self, b):
        if b < 0:
            b += len(self)
        ctx = self._context()
        with _tolerating(self._problem.on_ill_conditioned, self._owner):     # of the fit that made this object, whatever was fitted since
            a, bt, t, opt, _ = ctx.opt_finish(b)
        return float(self._all[b]), PartLSFitResult(a, bt, t, self._P)

    def __iter__(self):
        return (self[b] for b in range(len(self)))

    def blocks(self, chunk=1 << 18):
        """Every pattern's model in bulk, in the sweep's visiting order: a generator of (b, opt, alpha, beta, t) blocks of at most `chunk`
        patterns (b: reference indices; alpha[len(b), M], beta[len(b), K]).  The models come straight from the sweep kernels
        (partls_opt_models): the Gram-form solutions that rank opt, not refined in data space as self[b]'s are.  A pattern that hit the
        pivot cap is solved once more on its own (opt_finish).  With refused dependent columns (n_vetoes > 0) the Gram form carries no
        guarantee: the block is rebuilt pattern by pattern through self[b] instead, with a warning."""
        ctx = self._context()
        npat = len(self)
        warned = False
        for g0 in range(0, npat, int(chunk)):
            r = ctx.opt_models(g0, min(npat, g0 + int(chunk)))
            b, opt, a, bt, t = r["pattern"], r["opt"], r["alpha"], r["beta"], r["t"]
            if r["n_vetoes"] > 0:
                if not warned:
                    warnings.warn("partitionedls: the sweep refused dependent columns (%d leave-one-out vetoes): the Gram-form models carry no "
                                  "guarantee, every model is rebuilt on its own (slow)" % r["n_vetoes"], IllConditionedWarning, stacklevel=2)
                    warned = True
                redo = np.arange(len(b))
            else:
                redo = np.flatnonzero(np.isnan(opt))
            for i in redo:
                o, model = self[int(b[i])]
                opt[i], a[i], bt[i], t[i] = o, model.α, model.β, model.t
            yield b, opt, a, bt, t

    def arrays(self, chunk=1 << 18):
        """(opt[2^(K+1)], alpha[2^(K+1), M], beta[2^(K+1), K], t[2^(K+1)]) indexed by the reference pattern b — every model at once,
        from blocks(chunk) (see there for accuracy and fallbacks)."""
        _, M, K = self._context()._shape
        npat = len(self)
        opt = np.empty(npat)
        alpha = np.empty((npat, M))
        beta = np.empty((npat, K))
        t = np.empty(npat)
        for b, o, a, bt, tt in self.blocks(chunk):
            opt[b] = o
            alpha[b] = a
            beta[b] = bt
            t[b] = tt
        return opt, alpha, beta, t


@dataclass
class TopPatterns:
    """report.top of fit(Opt, ..., top=k): the k best sign patterns of the enumeration and their models, best first (partls_opt_top;
    DESIGN.md §4.13).  pattern[k] (reference index b over the K groups and, bit K, the intercept), opt[k], alpha[k, M], beta[k, K], t[k];
    models: the same as a list of PartLSFitResult; n_vetoes: the sweep's leave-one-out refusals (> 0: the models were rebuilt one by
    one through opt_finish).  The order is that of the Gram-form objectives: (opt, pattern), -0.0 equal to +0.0.  fit's own winner is
    re-ranked among its near ties in data space, so report.best_index is among the first entries of pattern, not necessarily the first."""
    pattern: np.ndarray
    opt: np.ndarray
    alpha: np.ndarray
    beta: np.ndarray
    t: np.ndarray
    models: list
    n_vetoes: int = 0

    def __len__(self):
        return len(self.pattern)

    @property
    def gap(self):
        """opt[1:] - opt[0]: how far behind the winner each runner-up is"""
        return self.opt[1:] - self.opt[:1]

    @property
    def sign_agreement(self):
        """[K, 3]: share of the listed models with beta_k < 0, = 0, > 0 (the layout of BootstrapResult.sign_frequency)"""
        b = np.asarray(self.beta)
        if len(b) == 0:
            return np.full((b.shape[1], 3), np.nan)
        return np.stack([(b < 0).mean(0), (b == 0).mean(0), (b > 0).mean(0)], axis=1)

    def group_patterns(self):
        """The list over the 2^K group patterns: the intercept's bit (bit K) dropped from every pattern, of the entries that then
        coincide the better (earlier) one kept, the order preserved.  A TopPatterns whose pattern holds the group patterns."""
        K = np.asarray(self.beta).shape[1]
        gp = np.asarray(self.pattern, dtype=np.int64) & ((1 << K) - 1)
        _, first = np.unique(gp, return_index=True)
        keep = np.sort(first)
        return TopPatterns(gp[keep], self.opt[keep], self.alpha[keep], self.beta[keep], self.t[keep], [self.models[i] for i in keep],
                           self.n_vetoes)


def _top_patterns(ctx, k, Pout):
    """fit(Opt, ..., top=k) after the fit: opt_top(k) on the prepared context -> TopPatterns"""
    r = ctx.opt_top(k)
    if r["n_unconverged"] > 0:
        raise PartlsError(L.ERR_NOT_CONVERGED, "%d subproblems hit the pivot cap" % r["n_unconverged"])
    pat, opt, a, b, t = r["pattern"], r["opt"], r["alpha"], r["beta"], r["t"]
    if r["n_vetoes"] > 0:
        warnings.warn("partitionedls: the sweep refused dependent columns (%d leave-one-out vetoes): the Gram-form models carry no "
                      "guarantee, the %d listed models are rebuilt on their own (the ranking is kept)" % (r["n_vetoes"], len(pat)),
                      IllConditionedWarning, stacklevel=3)
        for i in range(len(pat)):                              # (status 9 of a rebuilt model: as fit's on_ill_conditioned says)
            a[i], b[i], t[i] = ctx.opt_finish(int(pat[i]))[:3]
    models = [PartLSFitResult(a[i].copy(), b[i].copy(), float(t[i]), Pout) for i in range(len(pat))]
    return TopPatterns(pat, opt, a, b, t, models, int(r["n_vetoes"]))


def fit(alg, X, y, P, *, η=None, eta=None, ϵ=None, eps=None, T=100, nnlsalg="nnls", returnAllSolutions=False, rng=None,
        alpha0=None, beta0=None, device=0, devices=None, faithful_intercept=False, generic_kernel=False, on_ill_conditioned="warn",
        weights=None, restarts=None, top=None, rescue=False):
    """fit(::Type{Opt|Alt|BnB}, X, y, P; η, ...) -> (PartLSFitResult, None, Report)   [Opt.jl:73, Alt.jl:50, BnB.jl:30]

    η/eta: regularisation (default 0.0);  Alt: ϵ/eps (1e-6), T (100), rng (None | int seed | numpy Generator) or an
    explicit starting point alpha0[M+1], beta0[K+1];  Opt: returnAllSolutions.
    faithful_intercept=True enumerates the reference's 2^(K+1) patterns instead of 2^K with a free intercept
    (same optimum).  Opt / BnB, devices=... (None | count | list of device indices): the enumeration / the frontier search is sharded
    over those GPUs inside the library (partls_fit_opt_multi, partls_fit_bnb_multi: the ranks' results meet in host memory), as the
    Julia drop-in does on a multi-GPU node.  nnlsalg is accepted for signature parity; the device solver is an exact active-set method.
    on_ill_conditioned: what to do when the returned model fails the data-space KKT check (status 9: X beyond the fp64 Gram form;
    the reference's QR-based NNLS still returns a model there, and the Julia patch reroutes to it): "warn" (default) returns the best
    Gram-form model with report.ill_conditioned = True and report.kkt_violation set, and emits IllConditionedWarning; "raise" raises
    PartlsError(status 9).
    weights: optional per-row sample weights w[N] (floating, finite, >= 0, sum > 0): the data term becomes sum_i w_i r_i^2 (the η rows
    stay unweighted) and report.opt its square root with the η rows; a row of weight 0 acts as an absent row.  Single device only
    (NotImplementedError with devices=).  DESIGN.md §4.7.
    A float32 X is uploaded and read as float32 (half the transfer and half the device memory of float64); all arithmetic stays fp64
    and every result equals the fit of X.astype(float64) bit for bit.  With devices= it is widened on the host.  DESIGN.md §4.8.
    A sparse X — any object with .tocsr() (every scipy.sparse matrix or array) or a CSR(indptr, indices, data, shape) tuple — is
    uploaded as CSR and never densified: every option of Opt (returnAllSolutions, top=, rescue=, faithful_intercept, generic_kernel),
    Alt (restarts= too), BnB, weights=, η and on_ill_conditioned works as for a dense X; NotImplementedError with devices=.
    DESIGN.md §4.15.
    Alt, restarts=R (int >= 1): Alt is a local method — R starting points run in one batched device call on one Gram matrix
    (partls_alt_multistart) and the best one is returned.  The starts are R successive single draws from rng (start 0
    is the start of fit(Alt, rng=seed)), or explicit: alpha0 of shape (R, M+1) with beta0 of shape (R, K+1) (restarts then None or R).
    report.opt / .iters are the winner's, report.best_start its index, report.starts = Report(opt, iters, status, alpha, beta, t) with
    one row per start (opt: the Gram-form loss of its last iteration; NaN rows where status != 0).  ValueError: 1-D starts together
    with restarts, mismatched shapes, non-finite starts, restarts < 1, restarts with Opt / BnB.  PartlsError(ERR_NOT_CONVERGED) when
    every start failed.
    Opt, top=k (int in 1 .. lowlevel.OPT_TOP_MAX_K): report.top = TopPatterns, the k best sign patterns and their models, selected on
    the device after the fit (partls_opt_top).  It forces the faithful enumeration, as returnAllSolutions does, and
    combines with it, with weights= and with a float32 X.  The ranking is the Gram-form one: report.best_index, re-ranked among near
    ties in data space, is among the first entries of top.pattern, not necessarily the first.  ValueError: top outside that range, or
    with Alt / BnB; NotImplementedError with devices= (merge per-shard Context.opt_top lists with dist.merge_top).
    Opt, rescue=True: a sign pattern that hits the pivot cap of the sweep (designs that are correlated throughout; otherwise
    PartlsError(ERR_NOT_CONVERGED)) is solved again on the device by Lawson-Hanson (lowlevel.OPT_RESCUE_CAPPED);
    report.rescued counts them.  Nothing extra runs when no pattern caps.  ValueError with Alt / BnB; NotImplementedError with devices=.
    """
    if alg not in (Opt, Alt, BnB):
        raise TypeError("fit: first argument must be Opt, Alt or BnB")
    if rescue:
        if alg is not Opt:
            raise ValueError("fit: rescue= is an option of Opt (the enumeration), not of %s" % alg.__name__)
        if devices is not None:
            raise NotImplementedError("fit: rescue= is not supported on several devices (devices=)")
    if top is not None:
        if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= int(top) <= L.OPT_TOP_MAX_K:
            raise ValueError("fit: top must be an int in 1 .. %d, got %r" % (L.OPT_TOP_MAX_K, top))
        if alg is not Opt:
            raise ValueError("fit: top= is an option of Opt (the enumeration), not of %s" % alg.__name__)
        if devices is not None:
            raise NotImplementedError("fit: top= is not supported on several devices (devices=); merge per-shard Context.opt_top lists "
                                      "with dist.merge_top")
    eta_v = 0.0 if (η is None and eta is None) else float(η if η is not None else eta)
    eps_v = 1e-6 if (ϵ is None and eps is None) else float(ϵ if ϵ is not None else eps)
    if nnlsalg not in ("nnls", "pivot", "fnnls"):
        raise ValueError("nnlsalg must be one of :nnls, :pivot, :fnnls")
    if on_ill_conditioned not in ("warn", "raise"):
        raise ValueError('on_ill_conditioned must be "warn" or "raise"')
    if devices is not None:
        _no_sparse("fit(devices=)", X, "fit on one device, or densify X yourself")
    Xf, yf, Pf = _fit_inputs(X, y, P, f32=devices is None)
    N, M = Xf.shape
    K = Pf.shape[1]
    wf = _weights(weights, N, "fit")
    # fits that exist as prepare + a staged call only (a sparse Xf is the marshalled CSR tuple: Context.opt_prepare takes it as it is)
    staged = wf is not None or isinstance(Xf, CSR) or Xf.dtype == np.float32
    starts = _alt_starts(alg, M, K, restarts, alpha0, beta0, rng)     # None: a single fit, today's path
    if wf is not None and devices is not None:
        raise NotImplementedError("fit: sample weights are not supported on several devices (devices=)")
    ctx = default_context(device)
    mc = default_multi(devices) if devices is not None and alg is not Alt else None
    ctx.last_ill = False
    Pout = np.array(Pf, dtype=np.int64, order="C")
    faithful = L.OPT_FAITHFUL_INTERCEPT

    def result(owner, a, b, t, **kw):
        """the reference's result tuple: the NamedTuple third element carries what the data-space check said as well"""
        if owner.last_ill:
            kkt = ctx.kkt_violation() if owner is ctx else float("nan")
            warnings.warn("partitionedls: the model's KKT conditions do not hold in data space (X is too ill-conditioned for the fp64 "
                          "Gram form); the returned model is the best Gram-form one — " + L.lib().partls_last_error().decode(),
                          IllConditionedWarning, stacklevel=3)
            kw.update(ill_conditioned=True, kkt_violation=kkt)
        return PartLSFitResult(a, b, t, Pout), None, Report(**kw)

    def solutions(c, allopt, flags, dev):
        return _Solutions(c, allopt, Pout, _Problem(Xf, yf, Pf, eta_v, flags, dev, wf, on_ill_conditioned))

    # on_ill_conditioned holds on the shared objects for the span of this call only
    with _tolerating(on_ill_conditioned, ctx, mc):
        if alg is Opt:
            flags = (faithful if (faithful_intercept or returnAllSolutions or top is not None) else 0) | (L.OPT_GENERIC_KERNEL if generic_kernel else 0)
            if rescue:
                flags |= L.OPT_RESCUE_CAPPED
            if mc is not None:
                a, b, t, opt, bi, allopt = mc.fit_opt(Xf, yf, Pf, eta_v, flags, want_all=returnAllSolutions)
                if returnAllSolutions:
                    c0 = mc.context(0)
                    c0._shape = (N, M, K)
                    return result(mc, a, b, t, solutions=solutions(c0, allopt, flags, mc.devices[0]))
                return result(mc, a, b, t, opt=opt, best_index=bi)
            ctx.opt_prepare(Xf, yf, Pf, eta_v, flags, weights=wf)
            bobj, bpat, allopt, unconv = ctx.opt_sweep(0, -1, want_all=returnAllSolutions)
            if unconv:
                raise PartlsError(L.ERR_NOT_CONVERGED, f"{unconv} subproblems hit the pivot cap")
            a, b, t, opt, bi = ctx.opt_finish(bpat)
            rescued = ctx.rescue_stats().rescued if rescue else 0
            extra = {} if top is None else dict(top=_top_patterns(ctx, int(top), Pout))
            if rescue:                                        # (after the sweep and the finish, before opt_top starts its own count)
                extra.update(rescued=rescued)
            if returnAllSolutions:
                return result(ctx, a, b, t, solutions=solutions(ctx, allopt, flags, device), **extra)
            return result(ctx, a, b, t, opt=opt, best_index=bi, **extra)
        if alg is Alt and starts is not None:
            ctx.opt_prepare(Xf, yf, Pf, eta_v, faithful, weights=wf)
            a, b, t, o, it, best, per = ctx.alt_multistart(starts[0], starts[1], eps_v, int(T))
            return result(ctx, a, b, t, opt=o, iters=it, best_start=best, starts=Report(**per))
        if alg is Alt:
            if alpha0 is None or beta0 is None:
                alpha0, beta0 = _draw_start(_generator(rng), M, K)
            a0 = np.ascontiguousarray(alpha0, dtype=np.float64)
            b0 = np.ascontiguousarray(beta0, dtype=np.float64)
            if a0.shape != (M + 1,) or b0.shape != (K + 1,):
                raise ValueError("alpha0 must have M+1 and beta0 K+1 entries")
            if staged:                                        # partls_fit_alt = prepare (faithful) + partls_alt_prepared
                ctx.opt_prepare(Xf, yf, Pf, eta_v, faithful, weights=wf)
                a, b, t, o, it = ctx.alt_prepared(a0, b0, eps_v, int(T))
            else:
                a, b, t, o, it = _host_fit(ctx, L.lib().partls_fit_alt, Xf, yf, Pf, eta_v, eps_v, int(T), _dp(a0), _dp(b0))
            return result(ctx, a, b, t, opt=o, iters=it)
        if mc is not None:
            a, b, t, o, no = mc.fit_bnb(Xf, yf, Pf, eta_v)
            return result(mc, a, b, t, opt=o, nopen=no)
        if staged:                                            # partls_fit_bnb = prepare (faithful) + partls_bnb_prepared
            ctx.opt_prepare(Xf, yf, Pf, eta_v, faithful, weights=wf)
            a, b, t, o, no = ctx.bnb_prepared()
        else:
            a, b, t, o, no = _host_fit(ctx, L.lib().partls_fit_bnb, Xf, yf, Pf, eta_v)
        return result(ctx, a, b, t, opt=o, nopen=no)


def _irls_problem(who, what, alg, X, y, P, η, eta, ϵ, eps, T, rng, alpha0, beta0, faithful_intercept, generic_kernel, rescue, device,
                  on_ill_conditioned):
    """What the re-weighted fits (fit_robust, fit_glm) share from the option checks on: the marshalled inputs, the flags of the staged
    prepare and staged(), the staged call of alg on whatever problem the context is prepared for.  Returns (ctx, Xf, yf, Pf, eta, flags,
    staged, Pout); no device work but default_context.  who / what: the caller's name and its subject in the messages."""
    if rescue and alg is not Opt:
        raise ValueError("%s: rescue= is an option of Opt (the enumeration), not of %s" % (who, alg.__name__))
    if on_ill_conditioned not in ("warn", "raise"):
        raise ValueError('on_ill_conditioned must be "warn" or "raise"')
    eta_v = _eta(η, eta)
    eps_v = 1e-6 if (ϵ is None and eps is None) else float(ϵ if ϵ is not None else eps)
    Xf, yf, Pf = _fit_inputs(X, y, P, f32=True)
    N, M = Xf.shape
    K = Pf.shape[1]
    flags = L.OPT_FAITHFUL_INTERCEPT
    if alg is Opt:
        flags = (L.OPT_FAITHFUL_INTERCEPT if faithful_intercept else 0) | (L.OPT_GENERIC_KERNEL if generic_kernel else 0) | (L.OPT_RESCUE_CAPPED if rescue else 0)
    if alg is Alt:
        if np.ndim(alpha0) == 2 or np.ndim(beta0) == 2:
            raise ValueError("%s: several starting points (restarts) are not supported together with %s" % (who, what))
        if alpha0 is None or beta0 is None:
            alpha0, beta0 = _draw_start(_generator(rng), M, K)
        a0 = np.ascontiguousarray(alpha0, dtype=np.float64)
        b0 = np.ascontiguousarray(beta0, dtype=np.float64)
        if a0.shape != (M + 1,) or b0.shape != (K + 1,):
            raise ValueError("alpha0 must have M+1 and beta0 K+1 entries")
    ctx = default_context(device)
    ctx.last_ill = False
    Pout = np.array(Pf, dtype=np.int64, order="C")

    def staged():
        """the staged call of alg on the prepared problem -> (alpha, beta, t, the Report fields of this fit)"""
        if alg is Opt:
            _, bpat, _, unconv = ctx.opt_sweep(0, -1)
            if unconv:
                raise PartlsError(L.ERR_NOT_CONVERGED, f"{unconv} subproblems hit the pivot cap")
            a, b, t, opt, bi = ctx.opt_finish(bpat)
            kw = dict(opt=opt, best_index=bi)
            if rescue:
                kw.update(rescued=ctx.rescue_stats().rescued)
            return a, b, t, kw
        if alg is Alt:
            a, b, t, o, it = ctx.alt_prepared(a0, b0, eps_v, int(T))
            return a, b, t, dict(opt=o, iters=it)
        a, b, t, o, no = ctx.bnb_prepared()
        return a, b, t, dict(opt=o, nopen=no)

    return ctx, Xf, yf, Pf, eta_v, flags, staged, Pout


def _irls_ill(ctx, kw):
    """the ill-conditioned ending of a re-weighted fit: fit's warning and report fields for the last staged fit"""
    if ctx.last_ill:
        warnings.warn("partitionedls: the model's KKT conditions do not hold in data space (X is too ill-conditioned for the fp64 "
                      "Gram form); the returned model is the best Gram-form one — " + L.lib().partls_last_error().decode(),
                      IllConditionedWarning, stacklevel=3)
        kw.update(ill_conditioned=True, kkt_violation=ctx.kkt_violation())


class RobustConvergenceWarning(UserWarning):
    """fit_robust ran out of iterations (max_iter) before the row weights settled within tol"""


ROBUST_C = {"huber": 1.345, "bisquare": 4.685}     # the usual 95 %-efficiency tuning constants


def _robust_options(loss, c, scale, who):
    """(loss code, c, scale_in) as partls_robust_weights takes them; ValueError for anything else.  scale: None or "mad" (0.0: the
    library estimates it) or a positive finite float"""
    if loss not in ROBUST_C:
        raise ValueError('%s: loss must be "huber" or "bisquare", got %r' % (who, loss))
    if c is None:
        c = ROBUST_C[loss]
    if isinstance(c, (bool, str)) or not isinstance(c, (int, float, np.integer, np.floating)) or not np.isfinite(c) or not c > 0:
        raise ValueError("%s: c must be a finite number > 0, got %r" % (who, c))
    if scale is None or (isinstance(scale, str) and scale == "mad"):
        s = 0.0
    elif isinstance(scale, (bool, str)) or not isinstance(scale, (int, float, np.integer, np.floating)) or not np.isfinite(scale) or not scale > 0:
        raise ValueError('%s: scale must be "mad" or a finite number > 0, got %r' % (who, scale))
    else:
        s = float(scale)
    return (L.ROBUST_HUBER if loss == "huber" else L.ROBUST_BISQUARE), float(c), s


def fit_robust(alg, X, y, P, *, loss="huber", c=None, scale="mad", max_iter=50, tol=1e-6, η=None, eta=None, ϵ=None, eps=None, T=100,
               rng=None, alpha0=None, beta0=None, faithful_intercept=False, generic_kernel=False, rescue=False, device=0,
               on_ill_conditioned="warn", weights=None, restarts=None, top=None, returnAllSolutions=False, devices=None):
    """fit_robust(Opt|Alt|BnB, X, y, P; loss, c, scale, ...) -> (PartLSFitResult, None, Report): an M-estimator of the partitioned
    model by iteratively reweighted least squares.  X is uploaded once; every iteration forms the row weights of the
    loss at the current model on the device (Context.robust_weights), swaps them into the prepared problem (Context.opt_reweight)
    and runs the staged fit of alg again.  The loop, exactly:
      1. prepare as fit does for a staged fit, unweighted (float32 stays float32, sparse stays CSR) and fit model_0 (Opt: sweep +
         finish, PartlsError(ERR_NOT_CONVERGED) on capped patterns as in fit; Alt: alt_prepared; BnB: bnb_prepared);
      2. for j = 1 .. max_iter: info = robust_weights(model_{j-1}); info.scale == 0 (at least half of the rows fitted exactly): stop,
         exact and converged; info.max_dw <= tol: stop, converged; else opt_reweight() and the staged fit again -> model_j.
    Alt starts every iteration from the one starting point fit(Alt, rng=, alpha0=, beta0=) would use.
    loss: "huber" or "bisquare"; c: its tuning constant (None: 1.345 / 4.685); scale: "mad" (median |residual| / 0.6745 of every
    iteration's residuals) or a positive float that holds it fixed — then, with Opt, each step minimises a majoriser of the loss
    exactly and report.robust.rho_sum does not increase (up to rounding).  The other options are fit's.
    Returns the last model; the report carries the last fit's fields (opt, best_index / iters / nopen, ill_conditioned ...) and
    report.robust = Report(loss, c, scale, iterations (re-weighted fits run), converged, exact, weights[N] (the last ones formed; all
    ones when none were), rho_sum, max_dw, scales (lists, one entry per robust_weights call), n_down, n_zero).  Out of iterations:
    converged = False and a RobustConvergenceWarning.
    ValueError before any device work: weights=, restarts=, top=, returnAllSolutions= (not combined with a robust loss), a bad loss,
    c, scale, max_iter or tol; NotImplementedError: devices=."""
    if alg not in (Opt, Alt, BnB):
        raise TypeError("fit_robust: first argument must be Opt, Alt or BnB")
    for name, given in (("weights", weights is not None), ("restarts", restarts is not None), ("top", top is not None),
                        ("returnAllSolutions", bool(returnAllSolutions))):
        if given:
            raise ValueError("fit_robust: %s= is not supported together with a robust loss" % name)
    if devices is not None:
        raise NotImplementedError("fit_robust: several devices (devices=) are not supported")
    code, cv, sv = _robust_options(loss, c, scale, "fit_robust")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or int(max_iter) < 1:
        raise ValueError("fit_robust: max_iter must be an integer >= 1, got %r" % (max_iter,))
    if isinstance(tol, (bool, str)) or not isinstance(tol, (int, float, np.integer, np.floating)) or not np.isfinite(tol) or tol < 0:
        raise ValueError("fit_robust: tol must be a finite number >= 0, got %r" % (tol,))
    ctx, Xf, yf, Pf, eta_v, flags, staged, Pout = _irls_problem(
        "fit_robust", "a robust loss", alg, X, y, P, η, eta, ϵ, eps, T, rng, alpha0, beta0, faithful_intercept, generic_kernel, rescue,
        device, on_ill_conditioned)
    N = Xf.shape[0]
    rho_sums, max_dws, scales = [], [], []
    w_last = np.ones(N)                                       # the library writes the weights of every call that forms some into it
    iterations, converged, exact = 0, False, False
    with _tolerating(on_ill_conditioned, ctx):
        ctx.opt_prepare(Xf, yf, Pf, eta_v, flags)
        a, b, t, kw = staged()
        for _ in range(int(max_iter)):
            info = ctx._robust_weights(a, b, t, loss, cv, sv if sv > 0 else None, w_last.ctypes.data)
            rho_sums.append(info["rho_sum"]); max_dws.append(info["max_dw"]); scales.append(info["scale"])
            if info["scale"] == 0.0:
                converged = exact = True
                break
            if info["max_dw"] <= tol:
                converged = True
                break
            ctx.opt_reweight()
            a, b, t, kw = staged()
            iterations += 1
        _irls_ill(ctx, kw)
    if not converged:
        warnings.warn("partitionedls: fit_robust stopped after max_iter = %d re-weighted fits with the weights still moving "
                      "(max |dw| = %.3g > tol = %.3g)" % (int(max_iter), max_dws[-1], tol), RobustConvergenceWarning, stacklevel=2)
    kw["robust"] = Report(loss=loss, c=cv, scale=info["scale"], iterations=iterations, converged=converged, exact=exact, weights=w_last,
                          rho_sum=rho_sums, max_dw=max_dws, scales=scales, n_down=info["n_down"], n_zero=info["n_zero"])
    return PartLSFitResult(a, b, t, Pout), None, Report(**kw)


class GLMConvergenceWarning(UserWarning):
    """fit_glm ran out of iterations (max_iter) before the deviance settled within tol"""


GLM_FAMILIES = ("binomial", "poisson")


def _glm_family(family, who):
    """the family code as partls_glm_working takes it; ValueError for anything else"""
    if not isinstance(family, str) or family not in GLM_FAMILIES:
        raise ValueError('%s: family must be "binomial" or "poisson", got %r' % (who, family))
    return L.GLM_BINOMIAL if family == "binomial" else L.GLM_POISSON


def _glm_null_deviance(y, family):
    """the deviance of the intercept-only model (mu = mean(y) under both canonical links), in numpy"""
    y = np.asarray(y, dtype=np.float64)
    m = float(np.mean(y))
    with np.errstate(divide="ignore", invalid="ignore"):
        xlogy = lambda a: np.where(a == 0.0, 0.0, a * np.log(np.where(a == 0.0, 1.0, a)))
        if family == "binomial":
            if m <= 0.0 or m >= 1.0:
                return 0.0
            d = (xlogy(y) + xlogy(1.0 - y)) - (y * np.log(m) + (1.0 - y) * np.log1p(-m))
        else:
            if m <= 0.0:
                return 0.0
            d = (xlogy(y) - y * np.log(m)) - (y - m)
    return float(2.0 * np.sum(d))


def fit_glm(alg, X, y, P, *, family="binomial", max_iter=25, tol=1e-8, η=None, eta=None, ϵ=None, eps=None, T=100, rng=None,
            alpha0=None, beta0=None, faithful_intercept=False, generic_kernel=False, rescue=False, device=0,
            on_ill_conditioned="warn", weights=None, restarts=None, top=None, returnAllSolutions=False, devices=None):
    """fit_glm(Opt|Alt|BnB, X, y, P; family, ...) -> (PartLSFitResult, None, Report): the partitioned model under a logistic
    (family="binomial", logit link, y in [0, 1]) or Poisson (family="poisson", log link, y >= 0) likelihood, by iteratively reweighted
    least squares.  X is uploaded once; every iteration swaps the working weights and the working response into the
    prepared problem on the device (Context.opt_rework), runs the staged fit of alg and forms the next working rows at its model
    (Context.glm_working).  The loop, exactly:
      1. prepare as fit_robust does: unweighted, on y (float32 stays float32, sparse stays CSR);
      2. glm_working(None) -> dev_0 (the start: eta from y alone, as R's glm.fit);
      3. for j = 1 .. max_iter: opt_rework(); the staged fit of alg (fit_robust's) -> model_j; glm_working(model_j) -> dev_j; stop,
         converged, when |dev_j - dev_{j-1}| <= tol (|dev_j| + 0.1) (R's rule).
    The model is on the link scale: predict(model, X) is eta; predict_mean(model, X, family) is the mean.  The linear predictor is
    clamped to [-30, 30] inside the working rows, so a separable binomial problem ends (report.glm.n_clamped > 0).  IRLS without step
    control need not be monotone: report.glm.deviance shows every iterate's.
    Returns the last model; the report carries the last fit's fields (opt, best_index / iters / nopen, ill_conditioned ...) and
    report.glm = Report(family, iterations, converged, deviance (list: dev_0 .. dev_iterations), null_deviance (the intercept-only
    model's, in numpy), max_abs_eta, n_clamped (of the last working call), weights[N], working_response[N] (the last rows formed)).
    Out of iterations: converged = False and a GLMConvergenceWarning.
    ValueError before any device work: weights=, restarts=, top=, returnAllSolutions= (prior weights are not supported), a bad
    family, max_iter or tol, a y with NaN / Inf or outside the family's domain; NotImplementedError: devices=."""
    if alg not in (Opt, Alt, BnB):
        raise TypeError("fit_glm: first argument must be Opt, Alt or BnB")
    for name, given in (("weights", weights is not None), ("restarts", restarts is not None), ("top", top is not None),
                        ("returnAllSolutions", bool(returnAllSolutions))):
        if given:
            raise ValueError("fit_glm: %s= is not supported together with a family" % name)
    if devices is not None:
        raise NotImplementedError("fit_glm: several devices (devices=) are not supported")
    _glm_family(family, "fit_glm")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or int(max_iter) < 1:
        raise ValueError("fit_glm: max_iter must be an integer >= 1, got %r" % (max_iter,))
    if isinstance(tol, (bool, str)) or not isinstance(tol, (int, float, np.integer, np.floating)) or not np.isfinite(tol) or tol < 0:
        raise ValueError("fit_glm: tol must be a finite number >= 0, got %r" % (tol,))
    yv = np.asarray(y)
    if yv.ndim == 1 and np.issubdtype(yv.dtype, np.floating) and yv.size:
        if not np.all(np.isfinite(yv)):
            raise ValueError("fit_glm: y contains NaN / Inf")
        if family == "binomial" and (yv.min() < 0 or yv.max() > 1):
            raise ValueError("fit_glm: the binomial family needs 0 <= y <= 1")
        if family == "poisson" and yv.min() < 0:
            raise ValueError("fit_glm: the Poisson family needs y >= 0")
    ctx, Xf, yf, Pf, eta_v, flags, staged, Pout = _irls_problem(
        "fit_glm", "a family", alg, X, y, P, η, eta, ϵ, eps, T, rng, alpha0, beta0, faithful_intercept, generic_kernel, rescue, device,
        on_ill_conditioned)
    N = Xf.shape[0]
    w_last, z_last = np.zeros(N), np.zeros(N)                 # the library writes the rows of every working call into them
    devs = []
    iterations, converged = 0, False
    with _tolerating(on_ill_conditioned, ctx):
        ctx.opt_prepare(Xf, yf, Pf, eta_v, flags)
        info = ctx._glm_working(None, family, w_last.ctypes.data, z_last.ctypes.data, None)
        devs.append(info["deviance"])
        for _ in range(int(max_iter)):
            ctx.opt_rework()
            a, b, t, kw = staged()
            iterations += 1
            info = ctx._glm_working((a, b, t), family, w_last.ctypes.data, z_last.ctypes.data, None)
            devs.append(info["deviance"])
            if abs(devs[-1] - devs[-2]) <= tol * (abs(devs[-1]) + 0.1):
                converged = True
                break
        _irls_ill(ctx, kw)
    if not converged:
        warnings.warn("partitionedls: fit_glm stopped after max_iter = %d re-weighted fits with the deviance still moving "
                      "(|change| = %.3g)" % (int(max_iter), abs(devs[-1] - devs[-2])), GLMConvergenceWarning, stacklevel=2)
    kw["glm"] = Report(family=family, iterations=iterations, converged=converged, deviance=devs,
                       null_deviance=_glm_null_deviance(yf, family), max_abs_eta=info["max_abs_eta"], n_clamped=info["n_clamped"],
                       weights=w_last, working_response=z_last)
    return PartLSFitResult(a, b, t, Pout), None, Report(**kw)


def predict_mean(model, X, family, *, device=0):
    """predict_mean(model, X, family) -> the mean of a fit_glm model on the rows of X: predict(model, X), then the inverse link of the
    family on the device, clamp included (partls_glm_mean) — on the training X, the mu of the fit's last working call bit for bit."""
    _glm_family(family, "predict_mean")
    return default_context(device).glm_mean(family, predict(model, X, device=device))


def cv_folds(N, nfolds=5, shuffle=False, rng=None):
    """Folds of cross_validate: (fold_ptr[F+1], perm[N]).  Fold sizes are numpy.array_split's (the first N % F folds one row longer);
    fold f is rows fold_ptr[f]:fold_ptr[f+1] of the data permuted by perm (the identity without shuffle; with shuffle, a permutation drawn
    from rng: None, an int seed or a numpy Generator).  nfolds = 0 or None: no folds (fold_ptr = [0]).  nfolds = 1, a negative count and
    nfolds > N are errors (ValueError)."""
    N = int(N)
    if N < 1:
        raise ValueError("cv_folds: need N >= 1 rows")
    if nfolds is None or int(nfolds) == 0:
        return np.array([0], dtype=np.int64), np.arange(N, dtype=np.int64)
    F = int(nfolds)
    if F == 1 or F < 0:
        raise ValueError("cv_folds: nfolds must be 0 (no folds) or >= 2, got %d" % F)
    if F > N:
        raise ValueError("cv_folds: %d folds for %d rows" % (F, N))
    sizes = np.array([len(a) for a in np.array_split(np.arange(N), F)], dtype=np.int64)
    fold_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if shuffle:
        perm = _generator(rng).permutation(N).astype(np.int64)
    else:
        perm = np.arange(N, dtype=np.int64)
    return fold_ptr, perm


@dataclass
class CVResult:
    """What cross_validate returns.  sse / mse: F x E held-out sums / means of squared errors; mse_mean[e] = sum_f sse[f, e] / N (pooled);
    with sample weights, sse is weighted and the means divide by the weight of the fold / of all rows instead of the row counts;
    best_eta: argmin of mse_mean over the η values whose problems all succeeded (first on ties); models[f][e] the training fits, path[e]
    the full-data fits, model = path at best_eta; status[f][e] (F+1 rows: the last is the path) and ill_conditioned (status 9).
    best_index: the winning patterns of Opt (None for Alt); iters, best_start, starts: cross_validate(Alt) only (see there)."""
    etas: np.ndarray
    folds: list
    fold_ptr: np.ndarray
    perm: np.ndarray
    sse: np.ndarray
    mse: np.ndarray
    mse_mean: np.ndarray
    best_eta: float
    best_index_eta: int
    models: list
    path: list
    model: object
    opt: np.ndarray
    best_index: np.ndarray
    status: np.ndarray
    ill_conditioned: np.ndarray
    iters: np.ndarray = None               # Alt: completed iterations of every problem's winner
    best_start: np.ndarray = None          # Alt: every problem's winning start (-1: none finished)
    starts: object = None                  # Alt: Report(opt, iters, status), each [F+1, E, R]


def cross_validate(alg, X, y, P, *, η=None, eta=None, nfolds=5, shuffle=False, rng=None, faithful_intercept=False, device=0,
                   on_ill_conditioned="warn", generic_kernel=False, weights=None, restarts=None, alpha0=None, beta0=None, ϵ=None, eps=None,
                   T=100):
    """K-fold cross-validation of fit(Opt) — or of the multistart fit(Alt) — over an η grid, plus the full-data path, in one device
    call (partls_cv_opt, partls_cv_alt).

    η/eta: the grid (default [0.0]); nfolds: F (0: the path only); shuffle / rng: rows permuted on the host first (CVResult.perm).
    Problem (f, e) is fit(Opt, X[train_f], y[train_f], P; η = η[e]) with train_f every row outside fold f in order.
    on_ill_conditioned: "warn" (default) keeps status-9 models and warns once, "raise" raises PartlsError(9).
    weights: optional per-row sample weights (as fit; permuted with the rows by shuffle): problem (f, e) is the weighted fit on train_f,
    sse[f, e] = sum over fold f of w_i r_i^2, mse[f, e] = sse[f, e] / (weight of fold f), mse_mean[e] = sum_f sse[f, e] / sum_i w_i.
    Alt (the tool beyond K = 39 groups): problem (f, e) is fit(Alt, X[train_f], y[train_f], P; η = η[e], restarts=R, ϵ, T)
    from the SAME R starts for every problem — restarts=R draws them (default 32), alpha0 (R, M+1) with beta0 (R, K+1) gives them; rules
    and ValueErrors of fit.  One generator made from rng is consumed first by the shuffle permutation and then by R successive single
    draws.  CVResult then carries iters, best_start ([F+1, E]) and starts = Report(opt, iters, status), each [F+1, E, R]; best_index is
    None.  restarts or starts with Opt: ValueError."""
    if alg not in (Opt, Alt):
        raise TypeError("cross_validate: only Opt and Alt are supported")
    if alg is Opt and (restarts is not None or alpha0 is not None or beta0 is not None):
        raise ValueError("cross_validate: restarts, alpha0 and beta0 are options of Alt")
    if on_ill_conditioned not in ("warn", "raise"):
        raise ValueError('on_ill_conditioned must be "warn" or "raise"')
    _no_sparse("cross_validate", X, "densify X yourself, or call fit per fold and η")
    grid = [0.0] if (η is None and eta is None) else (η if η is not None else eta)
    etas = np.ascontiguousarray(np.atleast_1d(np.asarray(grid, dtype=np.float64)))
    Xf, yf, Pf = _fit_inputs(X, y, P)
    N, M = Xf.shape
    K = Pf.shape[1]
    wf = _weights(weights, N, "cross_validate")
    if alg is Alt:
        rng = _generator(rng)                                # one generator: the permutation first, then the starts
    fold_ptr, perm = cv_folds(N, nfolds, shuffle, rng)
    starts = None
    if alg is Alt:
        if restarts is None and 2 not in [np.ndim(v) for v in (alpha0, beta0) if v is not None]:
            restarts = 32
        starts = _alt_starts(Alt, M, K, restarts, alpha0, beta0, rng)
        eps_v = 1e-6 if (ϵ is None and eps is None) else float(ϵ if ϵ is not None else eps)
    if shuffle:
        Xf = np.asfortranarray(Xf[perm])
        yf = np.ascontiguousarray(yf[perm])
        if wf is not None:
            wf = np.ascontiguousarray(wf[perm])
    if wf is not None and len(fold_ptr) > 1:
        pos = np.add.reduceat((wf > 0).astype(np.int64), fold_ptr[:-1])
        if np.any(pos == pos.sum()):
            raise ValueError("cross_validate: the training rows of some fold have zero total weight")
    F = len(fold_ptr) - 1
    E = len(etas)
    flags = (L.OPT_FAITHFUL_INTERCEPT if faithful_intercept else 0) | (L.OPT_GENERIC_KERNEL if generic_kernel else 0)
    ctx = default_context(device)
    if alg is Opt:
        r = ctx.cv_opt(Xf, yf, Pf, fold_ptr if F else None, etas, flags, weights=wf)
        extra = dict(best_index=r["best_index"].reshape(F + 1, E).copy())
    else:
        r = ctx.cv_alt(Xf, yf, Pf, fold_ptr if F else None, etas, starts[0], starts[1], eps_v, int(T), weights=wf,
                       flags=L.OPT_GENERIC_KERNEL if generic_kernel else 0)
        per = {k: np.asarray(v).reshape(F + 1, E, -1).copy() for k, v in r["starts"].items()}
        extra = dict(best_index=None, iters=r["iters"].reshape(F + 1, E).copy(), best_start=r["best_start"].reshape(F + 1, E).copy(),
                     starts=Report(**per))
    st = r["status"].reshape(F + 1, E)
    if on_ill_conditioned == "raise" and np.any(st == L.ERR_ILL_CONDITIONED):
        raise PartlsError(L.ERR_ILL_CONDITIONED, "a cross-validation problem failed its data-space KKT check")
    if np.any(st == L.ERR_ILL_CONDITIONED):
        warnings.warn("partitionedls: %d cross-validation problem(s) failed the data-space KKT check (X too ill-conditioned for the fp64 "
                      "Gram form); their models are the best Gram-form ones" % int(np.sum(st == L.ERR_ILL_CONDITIONED)),
                      IllConditionedWarning, stacklevel=2)
    Pout = np.array(Pf, dtype=np.int64, order="C")

    def model(q):
        if r["status"][q] == L.ERR_NOT_CONVERGED:
            return None
        return PartLSFitResult(r["alpha"][:, q].copy(), r["beta"][:, q].copy(), float(r["t"][q]), Pout)

    models = [[model(f * E + e) for e in range(E)] for f in range(F)]
    path = [model(F * E + e) for e in range(E)]
    sse = r["heldout_sse"].reshape(F + 1, E)[:F].copy()
    if wf is None:
        sizes, total = np.diff(fold_ptr).astype(np.float64), N
    else:
        sizes = np.array([wf[fold_ptr[f]:fold_ptr[f + 1]].sum() for f in range(F)])
        total = wf.sum()
    with np.errstate(divide="ignore", invalid="ignore"):          # a held-out fold of weight 0 has no mean (NaN)
        mse = sse / sizes[:, None] if F else sse
    mse_mean = sse.sum(axis=0) / total if F else np.full(E, np.nan)
    failed = np.any(st == L.ERR_NOT_CONVERGED, axis=0)
    cand = np.where(failed | np.isnan(mse_mean), np.inf, mse_mean)
    if F and np.isfinite(cand).any():
        be = int(np.argmin(cand))
    else:
        be = 0 if not failed[0] else -1
    best_eta = float(etas[be]) if be >= 0 else float("nan")
    folds = [perm[fold_ptr[f]:fold_ptr[f + 1]] for f in range(F)]
    return CVResult(etas=etas, folds=folds, fold_ptr=fold_ptr, perm=perm, sse=sse, mse=mse, mse_mean=mse_mean, best_eta=best_eta,
                    best_index_eta=be, models=models, path=path, model=path[be] if be >= 0 else None,
                    opt=r["opt"].reshape(F + 1, E).copy(), status=st.copy(), ill_conditioned=(st == L.ERR_ILL_CONDITIONED), **extra)


@dataclass
class BootstrapResult:
    """What bootstrap and resample return: one fit(Opt) per weighting (replicate) b, as arrays — nothing here refers to a context.
    counts: the N x B int64 multinomial draws of bootstrap (None from resample); alpha[B, M], beta[B, K], t[B], opt[B], best_index[B];
    models[b]: PartLSFitResult, or None where status[b] is 6 (pivot cap: NaN rows); status[B] (0 / 9 / 6); oob_sse[b] / oob_rows[b]:
    squared error and number of the rows replicate b left out (weight 0); P: the partition the replicates share.  The statistics below go
    over the successful replicates (status 0 or 9) and are plain numpy on B rows; predict runs on the device."""
    counts: object
    alpha: np.ndarray
    beta: np.ndarray
    t: np.ndarray
    opt: np.ndarray
    best_index: np.ndarray
    models: list
    status: np.ndarray
    oob_sse: np.ndarray
    oob_rows: np.ndarray
    P: object = None            # the partition of every replicate (predict needs no model object)

    @property
    def ok(self):
        """replicates that returned a model"""
        return np.asarray(self.status) != L.ERR_NOT_CONVERGED

    @property
    def ill_conditioned(self):
        return np.asarray(self.status) == L.ERR_ILL_CONDITIONED

    @property
    def oob_mse(self):
        """pooled out-of-bag error: sum of oob_sse over sum of oob_rows, over the successful replicates that left rows out"""
        use = self.ok & (np.asarray(self.oob_rows) > 0) & np.isfinite(self.oob_sse)
        return float(np.sum(self.oob_sse[use]) / np.sum(self.oob_rows[use])) if use.any() else float("nan")

    @property
    def sign_frequency(self):
        """[K, 3]: share of the successful replicates with β_k < 0, = 0, > 0"""
        b = np.asarray(self.beta)[self.ok]
        if not len(b):
            return np.full((np.asarray(self.beta).shape[1], 3), np.nan)
        return np.stack([(b < 0).mean(0), (b == 0).mean(0), (b > 0).mean(0)], axis=1)

    @property
    def pattern_frequency(self):
        """{best_index: share of the successful replicates whose winner it is}"""
        bi = np.asarray(self.best_index)[self.ok]
        v, c = np.unique(bi, return_counts=True)
        return {int(p): float(n) / len(bi) for p, n in zip(v, c)}

    def interval(self, level=0.95):
        """percentile bounds over the successful replicates: dict(alpha=(lo[M], hi[M]), beta=(lo[K], hi[K]), t=(lo, hi))"""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError("interval: level must lie in (0, 1), got %r" % level)
        ok = self.ok
        if not ok.any():
            raise ValueError("interval: no successful replicate")
        q = [50.0 * (1.0 - level), 100.0 - 50.0 * (1.0 - level)]
        out = {}
        for k in ("alpha", "beta", "t"):
            lo, hi = np.percentile(np.asarray(getattr(self, k))[ok], q, axis=0)
            out[k] = (float(lo), float(hi)) if k == "t" else (lo, hi)
        return out

    def predict(self, X, level=0.95, *, return_all=False, device=0):
        """Percentile band of the successful replicates' predictions for the rows of X, in one pass over X (partls_predict_many,
        DESIGN.md §4.12): dict(mean[N], lo[N], hi[N]) — the mean over the replicates and the 50 (1 - level) and 100 - 50 (1 - level)
        percentiles of each row's B_ok predictions as np.percentile defines them (linear interpolation), computed as 50 - 50 level
        and 50 + 50 level: exactly 5 and 95 for level 0.9, 2.5 and 97.5 for 0.95.  The device returns the order
        statistics either side of each percentile (at most four per row) and the mean; the interpolation between two neighbours
        happens here, by np.percentile's own formula.  return_all=True adds yhat[N, B_ok], column j = predict with the j-th successful
        replicate; without it no N x B array exists on the host.  X as in predict.  ValueError: level outside (0, 1), no
        successful replicate, a result without its partition (P)."""
        X, a, b, t = self._band_inputs("predict", X, level)
        r, lo, hi = _percentile_band(level, len(t), lambda ranks: default_context(device).predict_many(
            X, self.P, a, b, t, ranks=ranks, want_yhat=return_all, want_mean=True))
        out = dict(mean=r["mean"], lo=lo, hi=hi)
        if return_all:
            out["yhat"] = r["yhat"]
        return out

    def contributions(self, X, level=0.95, return_all=False, *, device=0):
        """Percentile band of the successful replicates' group contributions for the rows of X, in one pass over X
        (partls_contributions): dict(mean, lo, hi), each [N, K] — per (row, group) the mean over the replicates and
        the percentiles 50 - 50 level and 50 + 50 level of its B_ok contributions, np.percentile(all, q, axis=2) to the last bit (the
        device returns the order statistics either side of each percentile and the mean, the interpolation happens here, as in
        predict).  return_all=True adds all[N, K, B_ok], slab j = contributions of the j-th successful replicate; without it no
        N x K x B array exists on the host.  X and the errors as in predict; a sparse X raises NotImplementedError."""
        X, a, b, t = self._band_inputs("contributions", X, level)
        r, lo, hi = _percentile_band(level, len(t), lambda ranks: default_context(device).contributions(
            X, self.P, a, b, ranks=ranks, want_contrib=return_all, want_mean=True))
        out = dict(mean=r["mean"], lo=lo, hi=hi)
        if return_all:
            out["all"] = r["contrib"]
        return out

    def _band_inputs(self, who, X, level):
        """the checks predict and contributions share, before any device work -> X as an array and the successful replicates' alpha, beta, t"""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError("%s: level must lie in (0, 1), got %r" % (who, level))
        ok = self.ok
        if not ok.any():
            raise ValueError("%s: no successful replicate" % who)
        if self.P is None:
            raise ValueError("%s: this result does not carry its partition P" % who)
        _no_sparse("BootstrapResult.%s" % who, X, "densify X yourself, or call %s per model" % who)
        X = np.asarray(X)
        if not np.issubdtype(X.dtype, np.floating) or X.ndim != 2:
            raise TypeError("%s: X must be a floating-point matrix" % who)
        a, b, t = np.asarray(self.alpha)[ok], np.asarray(self.beta)[ok], np.asarray(self.t)[ok]
        if X.shape[1] != a.shape[1]:
            raise ValueError("DimensionMismatch in %s" % who)
        return X, a, b, t


def _percentile_band(level, n, call):
    """The band of BootstrapResult.predict and .contributions over n values per cell: the ranks either side of the percentiles
    50 - 50 level and 50 + 50 level (_percentile_ranks: at most four), call(ranks) -> a result dict whose "stats" holds those order
    statistics along its last axis, and numpy's interpolation between the neighbours (_lerp) -> (the result dict, lo, hi)"""
    ranks, parts = _percentile_ranks(n, [50.0 - 50.0 * float(level), 50.0 + 50.0 * float(level)])
    r = call(ranks)
    lo, hi = (_lerp(r["stats"][..., i], r["stats"][..., j], g) for i, j, g in parts)
    return r, lo, hi


def _percentile_ranks(n, q):
    """np.percentile(v, q) of n values by its default (linear) method, in two steps: the positions of the sorted values it reads —
    (ranks, parts) with ranks the distinct positions in ascending order (int64) and parts[j] = (index into ranks of the lower
    neighbour, of the upper one, weight gamma) for percentile q[j] — and _lerp below.  The virtual index is (n - 1) (q / 100), its
    floor and ceiling the two neighbours (one position, gamma 0, when it is whole)."""
    virtual = (n - 1) * np.true_divide(np.asarray(q, dtype=np.float64), 100)
    lower = np.clip(np.floor(virtual), 0, n - 1)
    upper = np.clip(np.ceil(virtual), 0, n - 1)
    ranks = np.unique(np.concatenate([lower, upper])).astype(np.int64)
    parts = [(int(np.searchsorted(ranks, lo)), int(np.searchsorted(ranks, up)), float(v - lo)) for lo, up, v in zip(lower, upper, virtual)]
    return ranks, parts


def _lerp(a, b, gamma):
    """numpy's interpolation between neighbours a and b (numpy/lib/_function_base_impl.py, _lerp): a + (b - a) gamma, and from the upper
    end, b - (b - a) (1 - gamma), when gamma >= 0.5"""
    d = b - a
    return b - d * (1 - gamma) if gamma >= 0.5 else a + d * gamma


def _resample(who, alg, X, y, P, make_W, eta, faithful_intercept, generic_kernel, device, on_ill_conditioned):
    """bootstrap and resample after their own argument checks.  make_W(N) -> (counts or None, W[N, B] float64) runs after the checks
    of X, y, P and before any device work."""
    if alg is not Opt:
        raise TypeError("%s: only Opt is supported" % who)
    if on_ill_conditioned not in ("warn", "raise"):
        raise ValueError('on_ill_conditioned must be "warn" or "raise"')
    _no_sparse(who, X, "densify X yourself, or call fit(weights=...) per weighting")
    Xf, yf, Pf = _fit_inputs(X, y, P)
    N, M = Xf.shape
    counts, W = make_W(N)
    if not np.all(W.sum(axis=0) > 0):
        raise ValueError("%s: a weighting sums to 0" % who)
    B = W.shape[1]
    flags = (L.OPT_FAITHFUL_INTERCEPT if faithful_intercept else 0) | (L.OPT_GENERIC_KERNEL if generic_kernel else 0)
    r = default_context(device).opt_weightings(Xf, yf, Pf, W, eta, flags)
    st = r["status"]
    n_ill = int(np.sum(st == L.ERR_ILL_CONDITIONED))
    if n_ill and on_ill_conditioned == "raise":
        raise PartlsError(L.ERR_ILL_CONDITIONED, "%d replicate(s) failed the data-space KKT check" % n_ill)
    if n_ill:
        warnings.warn("partitionedls: %d replicate(s) failed the data-space KKT check (X too ill-conditioned for the fp64 Gram form under "
                      "their weights); their models are the best Gram-form ones" % n_ill, IllConditionedWarning, stacklevel=3)
    Pout = np.array(Pf, dtype=np.int64, order="C")
    alpha, beta = np.ascontiguousarray(r["alpha"].T), np.ascontiguousarray(r["beta"].T)
    models = [None if st[b] == L.ERR_NOT_CONVERGED else PartLSFitResult(alpha[b].copy(), beta[b].copy(), float(r["t"][b]), Pout)
              for b in range(B)]
    return BootstrapResult(counts=counts, alpha=alpha, beta=beta, t=r["t"], opt=r["opt"], best_index=r["best_index"], models=models,
                           status=st, oob_sse=r["oob_sse"], oob_rows=r["oob_rows"], P=Pout)


def _eta(η, eta):
    return 0.0 if (η is None and eta is None) else float(η if η is not None else eta)


def bootstrap(alg, X, y, P, *, B=100, rng=None, η=None, eta=None, weights=None, faithful_intercept=False, generic_kernel=False, device=0,
              on_ill_conditioned="warn"):
    """Nonparametric bootstrap of fit(Opt): B replicates in one device call (partls_opt_weightings) -> BootstrapResult.

    Replicate b is fit(Opt, X, y, P; η, weights=counts[:, b]) with counts = _generator(rng).multinomial(N, np.full(N, 1/N), size=B).T
    (int64, N x B; rng: None, an int seed or a numpy Generator) — returned as result.counts, so any replicate can be reproduced with
    fit(..., weights=result.counts[:, b].astype(float)).  weights (as fit): the replicate's weights are counts[:, b] * weights.
    The rows a replicate did not draw are its out-of-bag rows: result.oob_sse, oob_rows, oob_mse.  on_ill_conditioned as
    cross_validate.  Only Opt (TypeError otherwise); single device.  A float32 X is widened to float64 on the host.
    ValueError before any device work: B not an integer >= 1, bad weights (floating, finite, >= 0, sum > 0)."""
    if alg is not Opt:
        raise TypeError("bootstrap: only Opt is supported")
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or int(B) < 1:
        raise ValueError("bootstrap: B must be an integer >= 1, got %r" % (B,))

    def make_W(N):
        wf = _weights(weights, N, "bootstrap")
        counts = _generator(rng).multinomial(N, np.full(N, 1.0 / N), size=int(B)).T.astype(np.int64)
        W = np.asfortranarray(counts, dtype=np.float64)
        return counts, W if wf is None else np.asfortranarray(W * wf[:, None])

    return _resample("bootstrap", alg, X, y, P, make_W, _eta(η, eta), faithful_intercept, generic_kernel, device, on_ill_conditioned)


def resample(alg, X, y, P, W, *, η=None, eta=None, faithful_intercept=False, generic_kernel=False, device=0, on_ill_conditioned="warn"):
    """fit(Opt) under the caller's own row weightings W (N x B: jackknife or repeated train / validation splits as 0/1 columns, any
    reweighting) in one device call -> BootstrapResult with counts=None.  W: floating, finite, >= 0, every column sum > 0 (ValueError
    otherwise, before any device work).  Otherwise as bootstrap; a column's zero-weight rows are its out-of-bag rows."""
    if alg is not Opt:
        raise TypeError("resample: only Opt is supported")

    def make_W(N):
        Wa = np.asarray(W)
        if not np.issubdtype(Wa.dtype, np.floating):
            raise ValueError("resample: W must be floating point, got %s" % Wa.dtype)
        if Wa.ndim != 2 or Wa.shape[0] != N or Wa.shape[1] < 1:
            raise ValueError("resample: W must have shape (%d, B) with B >= 1, got %s" % (N, Wa.shape))
        Wf = np.asfortranarray(Wa, dtype=np.float64)
        if not np.all(np.isfinite(Wf)):
            raise ValueError("resample: W must be finite")
        if np.any(Wf < 0):
            raise ValueError("resample: W must be >= 0")
        return None, Wf

    return _resample("resample", alg, X, y, P, make_W, _eta(η, eta), faithful_intercept, generic_kernel, device, on_ill_conditioned)


def predict(*args, device=0):
    """predict(model, X) or predict(α, β, t, P, X)  ->  X * (P .* α) * β .+ t     [PartitionedLS.jl:132-134,152-155]
    X: a floating-point matrix, or sparse (anything with .tocsr(), or a CSR tuple): predicted from CSR, never densified."""
    if len(args) == 2:
        model, X = args
        α, β, t, P = model.α, model.β, model.t, model.P
    elif len(args) == 5:
        α, β, t, P, X = args
    else:
        raise TypeError("predict(model, X) or predict(α, β, t, P, X)")
    if _is_sparse(X):                                   # marshalled here once (TypeError as below); Context.predict takes the tuple as it is
        Xf, Pf = _csr(X, "predict"), np.asfortranarray(P, dtype=np.int64)
    else:
        X = np.asarray(X)
        if not np.issubdtype(X.dtype, np.floating) or X.ndim != 2:
            raise TypeError("predict: X must be a floating-point matrix")
        Xf, _, Pf = _inputs(X, None, P)                 # what the context is handed is what goes up (Context.predict takes it as it is)
    a = np.ascontiguousarray(α, dtype=np.float64)
    b = np.ascontiguousarray(β, dtype=np.float64)
    M = Xf.shape[1]
    if Pf.shape[0] != M or a.shape != (M,) or b.shape != (Pf.shape[1],):
        raise ValueError("DimensionMismatch in predict")
    return default_context(device).predict(Xf, Pf, a, b, t)


def _model_arrays(who, models):
    """models as predict_many, contributions_many and group_importance accept them -> (alpha[B, M], beta[B, K], t[B], P): a sequence of
    PartLSFitResult over one common partition, or a tuple (alpha, beta, t, P) of arrays, passed on as it is"""
    if isinstance(models, tuple) and len(models) == 4 and not isinstance(models[0], PartLSFitResult):
        a, b, t, P = models
    else:
        ms = list(models)
        if not ms or not all(isinstance(m, PartLSFitResult) for m in ms):
            raise ValueError("%s: models must be a non-empty sequence of PartLSFitResult or a tuple (alpha, beta, t, P)" % who)
        P = np.asarray(ms[0].P)
        if not all(m.P is ms[0].P or np.array_equal(np.asarray(m.P), P) for m in ms[1:]):
            raise ValueError("%s: the models must share one partition P" % who)
        if len({np.shape(m.α) for m in ms}) != 1 or len({np.shape(m.β) for m in ms}) != 1:
            raise ValueError("%s: the models differ in shape" % who)
        a, b, t = np.stack([m.α for m in ms]), np.stack([m.β for m in ms]), np.array([m.t for m in ms], dtype=np.float64)
    return a, b, t, P


def predict_many(models, X, *, device=0):
    """The predictions of many models for the rows of X in one upload of X (partls_predict_many)  ->  [N, B] float64,
    column b = predict(models[b], X) bit for bit.  models: a sequence of PartLSFitResult over one common partition (bootstrap's
    models, a cross-validation path, the starts of fit(Alt), solutions), or a tuple (alpha[B, M], beta[B, K], t[B], P) of arrays
    (BootstrapResult's alpha, beta, t, P; solutions.arrays()).  X as in predict: float32 goes up as float32.  More than
    lowlevel.PREDICT_MANY_MAX_B models are predicted in slices of that many columns (one upload of X per slice).
    ValueError: an empty sequence, models over different partitions, shapes that do not fit; TypeError: X not a floating matrix."""
    a, b, t, P = _model_arrays("predict_many", models)
    _no_sparse("predict_many", X, "densify X yourself, or call predict per model")
    X = np.asarray(X)
    if not np.issubdtype(X.dtype, np.floating) or X.ndim != 2:
        raise TypeError("predict_many: X must be a floating-point matrix")
    Xf, _, Pf = _inputs(X, None, P)
    if Pf.ndim != 2 or Pf.shape[0] != Xf.shape[1]:
        raise ValueError("DimensionMismatch in predict_many")
    a, b, t, _ = _many_models(a, b, t, Xf.shape[1], Pf.shape[1], None)
    ctx, cap = default_context(device), L.PREDICT_MANY_MAX_B
    parts = [ctx.predict_many(Xf, Pf, a[s:s + cap], b[s:s + cap], t[s:s + cap])["yhat"] for s in range(0, len(t), cap)]
    return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=1)


def _contrib_inputs(who, models, X):
    """what contributions_many and group_importance share, before any device work: the models (t is ignored), X and P as the library
    takes them"""
    a, b, t, P = _model_arrays(who, models)
    _no_sparse(who, X, "densify X yourself (contributions from CSR are not implemented)")
    X = np.asarray(X)
    if not np.issubdtype(X.dtype, np.floating) or X.ndim != 2:
        raise TypeError("%s: X must be a floating-point matrix" % who)
    Xf, _, Pf = _inputs(X, None, P)
    if Pf.ndim != 2 or Pf.shape[0] != Xf.shape[1]:
        raise ValueError("DimensionMismatch in %s" % who)
    a, b, _, _ = _many_models(a, b, np.zeros(np.shape(a)[:1]) if t is None else t, Xf.shape[1], Pf.shape[1], None, who)
    return a, b, Xf, Pf


def contributions_many(models, X, *, device=0):
    """The group contributions of many models for the rows of X in one upload of X (partls_contributions)  ->
    [N, K, B] float64: [i, k, b] = β_k Σ_{m in group k} α_m X[i, m] of model b, one fma chain over the group's features in ascending m.
    For a partition, contributions.sum(1) + t is predict up to summation order.  models as in predict_many (t is ignored); slab b equals
    contributions(models[b], X) bit for bit.  More than lowlevel.PREDICT_MANY_MAX_B models go in slices of that many (one upload of X
    per slice).  ValueError / TypeError as predict_many; NotImplementedError for a sparse X (the library never densifies)."""
    a, b, Xf, Pf = _contrib_inputs("contributions_many", models, X)
    ctx, cap = default_context(device), L.PREDICT_MANY_MAX_B
    parts = [ctx.contributions(Xf, Pf, a[s:s + cap], b[s:s + cap])["contrib"] for s in range(0, len(a), cap)]
    return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=2)


def contributions(model, X, *, device=0):
    """How much each group contributes to each prediction  ->  [N, K] float64: [i, k] = β_k Σ_{m in group k} α_m X[i, m]; for a partition
    the row sums plus t are predict(model, X) up to summation order.  See contributions_many."""
    if not isinstance(model, PartLSFitResult):
        raise TypeError("contributions: model must be a PartLSFitResult (many models: contributions_many)")
    return np.ascontiguousarray(contributions_many([model], X, device=device)[:, :, 0])


def group_importance(model_or_models, X, *, device=0):
    """Per-group summaries of the contributions over the rows of X  ->  Report(mean, mean_abs, rms, share), each [K] for one
    PartLSFitResult and [B, K] for many models (as predict_many accepts them, or a BootstrapResult: its successful replicates):
    the mean of c, of |c|, the root mean square of c, and share[k] = mean_abs[k] / Σ_k mean_abs (NaN where that sum is 0).  All four
    are derived here from the 3 K B sums the device returns (partls_contributions' sums): no N x K array crosses PCIe."""
    who = "group_importance"
    one = isinstance(model_or_models, PartLSFitResult)
    if isinstance(model_or_models, BootstrapResult):
        res = model_or_models
        if not res.ok.any():
            raise ValueError("%s: no successful replicate" % who)
        if res.P is None:
            raise ValueError("%s: this result does not carry its partition P" % who)
        ok = res.ok
        models = (np.asarray(res.alpha)[ok], np.asarray(res.beta)[ok], np.asarray(res.t)[ok], res.P)
    else:
        models = [model_or_models] if one else model_or_models
    a, b, Xf, Pf = _contrib_inputs(who, models, X)
    ctx, cap, N = default_context(device), L.PREDICT_MANY_MAX_B, Xf.shape[0]
    parts = [ctx.contributions(Xf, Pf, a[s:s + cap], b[s:s + cap], want_contrib=False, want_sums=True)["sums"] for s in range(0, len(a), cap)]
    sums = parts[0] if len(parts) == 1 else np.concatenate(parts, axis=2)
    mean, mean_abs, rms = sums[0].T / N, sums[1].T / N, np.sqrt(sums[2].T / N)           # [B, K]
    total = mean_abs.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(total > 0, mean_abs / total, np.nan)
    pick = (lambda v: np.ascontiguousarray(v[0])) if one else np.ascontiguousarray
    return Report(mean=pick(mean), mean_abs=pick(mean_abs), rms=pick(rms), share=pick(share))


@dataclass
class Diagnostics:
    """Row-by-row diagnostics of one model on (X, y, weights, η) — see diagnostics().  Per row [N]: leverage, loo, studentized, cooks,
    residual.  Per weight / group: se_w[M + 1] (0 outside the support; the intercept's last), se_beta[K], se_t, active[M + 1].
    Scalars: n_pos (rows of positive weight), p (size of the support), dof, rss, press, sigma2, tss, r2, r2_loo, stationarity and
    loo_mse = press / Σw."""
    leverage: np.ndarray
    loo: np.ndarray
    studentized: np.ndarray
    cooks: np.ndarray
    residual: np.ndarray
    se_w: np.ndarray
    se_beta: np.ndarray
    se_t: float
    active: np.ndarray
    n_pos: int
    p: int
    dof: float
    rss: float
    press: float
    sigma2: float
    tss: float
    r2: float
    r2_loo: float
    stationarity: float
    loo_mse: float


def _kkt_tol():
    """the data-space KKT tolerance a context is created with (PARTLS_KKT_TOL, read at partls_create; 1e-12)"""
    try:
        return float(os.environ.get("PARTLS_KKT_TOL", "1e-12"))
    except ValueError:
        return 1e-12


def diagnostics(model, X, y, *, η=None, eta=None, weights=None, device=0):
    """Judge one fit row by row  ->  Diagnostics.  model: a PartLSFitResult fitted to (X, y) with the same η and weights.

    Conditional on the model's sign pattern and support A (the weights v_m = α_m Σ_k P[m,k] β_k that are not 0, and the intercept) the
    fit is a linear smoother with H = Xo_A' W Xo_A + η Q_A, and the device returns: leverage h_i = w_i x_iA' H^-1 x_iA; residual
    e_i = y_i − predict(model, X)_i, bit for bit; loo_i = e_i / (1 − h_i), by Sherman–Morrison the residual of row i had it been left out
    (what resample with a jackknife weighting gives whenever the refit keeps pattern and support — without N Grams and N sweeps);
    studentized and Cook's distances; dof = Σ h, rss, press = Σ w loo², sigma2 = rss / (n_pos − dof), r2, r2_loo; and the standard
    errors of the weights, of β and of t from Cov = sigma2 H^-1 B H^-1 (partls_diagnostics).  One prepare (upload of X
    and Gram products) and one call; a float32 X stays float32.

    Caveats.  Everything is conditional on the selected pattern and support: there is no selection adjustment, so the standard errors
    are those of the least-squares problem the selection ended on.  Weights are precision weights (w_i ∝ 1 / variance_i), not
    frequencies: n_pos counts rows, not Σw.  stationarity tells whether the model really is the penalised least-squares solution on its
    support (it is for fit(Opt) / fit(BnB)); where it exceeds the context's KKT tolerance an IllConditionedWarning is given, and loo,
    sigma2 and the standard errors do not mean what their names say.  A sparse X is refused (NotImplementedError)."""
    who = "diagnostics"
    if not isinstance(model, PartLSFitResult):
        raise TypeError("%s: model must be a PartLSFitResult" % who)
    _no_sparse(who, X, "densify X yourself (diagnostics from CSR are not implemented)")
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1 or not np.issubdtype(X.dtype, np.floating) or not np.issubdtype(y.dtype, np.floating):
        raise TypeError("%s: X must be a floating-point matrix and y a floating-point vector" % who)
    Xf, yf, Pf = _inputs(X, y, model.P)
    N, M = Xf.shape
    a, b = np.ascontiguousarray(model.α, dtype=np.float64), np.ascontiguousarray(model.β, dtype=np.float64)
    if yf.shape != (N,) or Pf.ndim != 2 or Pf.shape[0] != M or a.shape != (M,) or b.shape != (Pf.shape[1],):
        raise ValueError("DimensionMismatch in %s" % who)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.isfinite(model.t)):
        raise ValueError("%s: the model has a NaN / Inf in α, β or t" % who)
    η = _eta(η, eta)
    if not (η >= 0 and np.isfinite(η)):
        raise ValueError("%s: η must be finite and >= 0" % who)
    w = _weights(weights, N, who)
    ctx = default_context(device)
    ctx.opt_prepare(Xf, yf, Pf, η, 0, weights=w)
    out = ctx.diagnostics(a, b, float(model.t))
    s = out["summary"]
    if s[L.DIAG_STATIONARITY] > _kkt_tol():
        warnings.warn("diagnostics: the model is not the least-squares solution on its support for this (X, y, η, weights) "
                      "(stationarity %.3g): loo, sigma2 and the standard errors are not those of a refit" % s[L.DIAG_STATIONARITY],
                      IllConditionedWarning, stacklevel=2)
    return Diagnostics(leverage=out["leverage"], loo=out["loo"], studentized=out["studentized"], cooks=out["cooks"],
                       residual=out["residual"], se_w=out["se_w"], se_beta=out["se_beta"], se_t=float(out["se_w"][M]),
                       active=out["active"], n_pos=int(s[L.DIAG_NPLUS]), p=int(s[L.DIAG_P]), dof=float(s[L.DIAG_DOF]),
                       rss=float(s[L.DIAG_RSS]), press=float(s[L.DIAG_PRESS]), sigma2=float(s[L.DIAG_SIGMA2]), tss=float(s[L.DIAG_TSS]),
                       r2=float(s[L.DIAG_R2]), r2_loo=float(s[L.DIAG_R2_LOO]), stationarity=float(s[L.DIAG_STATIONARITY]),
                       loo_mse=float(s[L.DIAG_PRESS] / (N if w is None else w.sum())))


def predict_device(model, dX_ptr, N, ldX, dyhat_ptr, device=0, dtype=np.float64):
    """predict with X (N x M, column-major, leading dimension ldX) and yhat (N) resident in HBM: raw device addresses (e.g.
    torch tensor .data_ptr()) that stay owned by the caller.  PartitionedLS.jl:132-134 without the PCIe copy of X.
    dtype: element type of X, float64 or float32 (ldX counts elements); yhat is float64 either way."""
    Pf = np.asfortranarray(model.P, dtype=np.int64)
    default_context(device).predict_device(dX_ptr, N, Pf.shape[0], ldX, Pf, model.α, model.β, model.t, dyhat_ptr, dtype=dtype)
