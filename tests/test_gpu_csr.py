"""Sparse design matrices on the GPU: partls_opt_prepare_csr / partls_predict_csr against the dense path on the
densified matrix, against extended-precision references and against the oracle.  Every CSR triple is built with numpy from a dense
array (np.nonzero walks it in row-major order), so nothing here needs scipy.

Data: a Bernoulli(d) mask (d = 0.15 for M < 100, 0.1 otherwise) times values.  Integer case: values +-{1, 2, 3}, integer y, weights
from {0, 1, 4} — every Gram entry, weighted or not, is an integer far below 2^53 and exact in any summation order, so the sparse and
the dense Gram must agree in every bit.  Real case: values N(1, 1), real y, weights 10 ** uniform(-1.5, 1.5).  No complete one-hot
blocks (their columns sum to the ones column).  The fit and data-pass problems are checked here, on the CPU, to be well conditioned
(unit-column [X, 1] between 1.5 and 20), so neither path meets vetoes or status 9; the Gram-only matrices carry a forced empty column,
for which that number does not exist, and need no conditioning.

Bounds: a sum of n products accumulated in fp64 in any order lies within (n + 2) 2^-53 sum |terms| of the exact value (n - 1 additions
and at most two roundings per product, to first order with one unit of slack); the fits use the project's parity level 1e-8.
The oracle has no sample weights: a weighted Opt is checked against it through its per-pattern objectives on the row-scaled homogeneous
problem (opt, best_index); weighted models, and weighted Alt / BnB, are checked against the dense path."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FAITHFUL = 1
KKT_TOL = 1e-12                      # PARTLS_KKT_TOL's default (ctx.h)
ERR_BAD_ARG, ERR_NONFINITE, ERR_UNSUPPORTED, ERR_STATE = 1, 3, 7, 8


# ---- data --------------------------------------------------------------------------------------------------------------------------------
def csr_of(D, S=None):
    """canonical CSR of the dense array D over the structure S (default: its nonzeros)"""
    r, c = np.nonzero(D if S is None else S)
    indptr = np.zeros(D.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=D.shape[0]), out=indptr[1:])
    return indptr, c.astype(np.int32), np.ascontiguousarray(D[r, c], dtype=np.float64)


def _density(M):
    return 0.15 if M < 100 else 0.1


def _partition(rng, M, K):
    grp = np.concatenate([np.arange(K), rng.integers(0, K, M - K)]) if M >= K else np.arange(M) % K
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), grp] = 1
    return P


def _matrix(rng, N, M, integer, d=None):
    S = rng.random((N, M)) < (_density(M) if d is None else d)
    V = rng.integers(1, 4, (N, M)) * rng.choice([-1.0, 1.0], (N, M)) if integer else rng.normal(1.0, 1.0, (N, M))
    return np.where(S, V, 0.0), S


def _response(rng, D, integer):
    y = D @ rng.normal(0.0, 1.0, D.shape[1]) + 2.0 + 0.3 * rng.normal(size=D.shape[0])
    return np.round(3 * y) if integer else y


def _weights(rng, N, integer):
    return rng.choice([0.0, 1.0, 4.0], N) if integer else 10.0 ** rng.uniform(-1.5, 1.5, N)


def _cond_unit_columns(D):
    Z = np.hstack([D, np.ones((D.shape[0], 1))])
    return np.linalg.cond(Z / np.linalg.norm(Z, axis=0))


@functools.lru_cache(maxsize=None)
def gram_case(N, M, integer, special=""):
    """(D, S, y, w): the Gram matrices — an empty row, an empty column, one fully dense row and one stored zero forced in"""
    rng = np.random.default_rng(1000 * N + M + (7 if integer else 0))
    D, S = _matrix(rng, N, M, integer, d=0.5 if special == "slices" else None)
    if special == "long":
        S[:, 1] = rng.random(N) < 0.93                      # one column holds >= 90 % of the rows: split into ranges
        D[:, 1] = np.where(S[:, 1], 2.0 if integer else 1.5, 0.0)
        assert S[:, 1].mean() >= 0.9
    D[N // 2], S[N // 2] = 0.0, False                       # an empty row
    D[:, M - 1], S[:, M - 1] = 0.0, False                   # an empty column
    S[N - 1, : M - 1] = True                                # a fully dense row (but for the empty column)
    D[N - 1, : M - 1] = np.arange(1, M) % 3 + 1.0 if integer else rng.normal(1.0, 1.0, M - 1)
    i, j = (0, 0) if N // 2 != 0 else (1, 0)
    S[i, j], D[i, j] = True, 0.0                            # a stored zero
    return D, S, _response(rng, D, integer), _weights(rng, N, integer)


def _device(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _prepare_csr(ctx, D, S, y, P, w, device, eta=0.0, flags=0):
    indptr, indices, data = csr_of(D, S)
    if device:
        import torch
        t = _device(indptr, indices, data, y, w)
        ctx.opt_prepare_csr_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), D.shape[0], D.shape[1], P, eta,
                                   flags, dw_ptr=None if w is None else t[4].data_ptr())
        assert ctx.upload() == (0.0, 0.0)
        return t                                            # keeps the tensors alive while the context holds the problem
    ctx.opt_prepare_csr(ctx_csr(indptr, indices, data, D.shape), y, P, eta, flags, weights=w)
    up = ctx.upload()
    assert up[1] == 8 * (D.shape[0] + 1) + 12 * len(data) and up[0] >= 0.0
    return None


def ctx_csr(indptr, indices, data, shape):
    import partls_amd
    return partls_amd.package().CSR(indptr, indices, data, shape)


GRAM_SHAPES = [(5, 3), (37, 5), (1000, 130), (2051, 257)]
GRAM_CASES = [(N, M, "") for N, M in GRAM_SHAPES] + [(1000, 130, "long"), (70000, 8, "slices")]


# ---- 1. Gram, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,special", GRAM_CASES)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_integer_gram_equals_the_dense_gram_and_numpy(partls, N, M, special, device):
    D, S, y, w = gram_case(N, M, True, special)
    P = np.ones((M, 1), dtype=np.int64)
    Z = np.hstack([D, np.ones((N, 1)), y[:, None]]).astype(np.int64)
    ctx = partls.Context(0)
    for wt in (None, w):
        keep = _prepare_csr(ctx, D, S, y, P, wt, device)
        Gs = ctx.gram()
        del keep
        ctx.opt_prepare(D, y, P, 0.0, weights=wt)
        Gd = ctx.gram()
        exact = (Z * (np.ones(N) if wt is None else wt).astype(np.int64)[:, None]).T @ Z
        assert np.array_equal(Gs, Gd), f"weights={wt is not None}: {np.count_nonzero(Gs != Gd)} entries differ from the dense Gram"
        assert np.array_equal(Gs, exact.astype(np.float64))
    ctx.close()


def test_gram_of_a_matrix_without_nonzeros(partls):
    D, S = np.zeros((5, 3)), np.zeros((5, 3), dtype=bool)
    y, P = np.arange(5.0), np.ones((3, 1), dtype=np.int64)
    ctx = partls.Context(0)
    for device in (False, True):
        keep = _prepare_csr(ctx, D, S, y, P, None, device)
        Gs = ctx.gram()
        del keep
        Z = np.hstack([D, np.ones((5, 1)), y[:, None]])
        assert np.array_equal(Gs, Z.T @ Z)
    ctx.close()


# ---- 2. Gram, real values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,special", GRAM_CASES)
def test_real_gram_within_the_summation_bound_and_reproducible(partls, N, M, special):
    D, S, y, w = gram_case(N, M, False, special)
    P = np.ones((M, 1), dtype=np.int64)
    Z = np.hstack([D, np.ones((N, 1)), y[:, None]])
    ZL = Z.astype(np.longdouble)
    nz = (Z != 0).astype(np.float64)
    ctx = partls.Context(0)
    for wt in (None, w):
        wl = np.ones(N) if wt is None else wt
        ref = (ZL * wl.astype(np.longdouble)[:, None]).T @ ZL
        mag = (np.abs(Z) * wl[:, None]).T @ np.abs(Z)
        terms = nz.T @ nz                                    # n_pq: rows where both entries are nonzero
        for device in (False, True):
            keep = _prepare_csr(ctx, D, S, y, P, wt, device)
            G1 = ctx.gram()
            del keep
            err = np.abs(G1.astype(np.longdouble) - ref).astype(np.float64)
            bound = (terms + 2) * U * mag
            worst = float(np.max(err / np.maximum(bound, 1e-300)))
            print(f"N={N} M={M} {special} weighted={wt is not None} device={device}: max error / bound = {worst:.3f}")
            assert np.all(err <= bound), worst
            assert np.array_equal(G1, G1.T)
            keep = _prepare_csr(ctx, D, S, y, P, wt, device)
            assert np.array_equal(ctx.gram(), G1), "two prepares of one input differ"
            del keep
    ctx.close()


# ---- 3. data passes ------------------------------------------------------------------------------------------------------------------
SEEDS = {(1200, 300): 1}             # picked so that the conditioning window below holds


@functools.lru_cache(maxsize=None)
def fit_case(N, M, K, integer, seed=0):
    rng = np.random.default_rng(77 * N + M + 1000 * (seed + SEEDS.get((N, M), 0)) + (5 if integer else 0))
    D, S = _matrix(rng, N, M, integer)
    D[3], S[3] = 0.0, False                                  # an empty row
    c = _cond_unit_columns(D)
    assert 1.5 <= c <= 20.0, c
    return D, S, _response(rng, D, integer), _weights(rng, N, integer), _partition(rng, M, K)


@pytest.mark.parametrize("N,M,K", [(37, 5, 2), (2051, 257, 3)])
def test_predict_within_the_row_bound_and_reproducible(partls, N, M, K):
    D, S, _, _, P = fit_case(N, M, K, False)
    rng = np.random.default_rng(5)
    alpha, beta, t = rng.random(M), rng.normal(size=K), 0.75
    wv = (P * alpha[:, None]) @ beta
    ref = D.astype(np.longdouble) @ wv.astype(np.longdouble) + np.longdouble(t)
    bound = ((D != 0).sum(1) + 2) * U * (np.abs(D) @ np.abs(wv) + abs(t))
    indptr, indices, data = csr_of(D, S)
    ctx = partls.Context(0)
    yh = ctx.predict_csr(ctx_csr(indptr, indices, data, D.shape), P, alpha, beta, t)
    import torch
    tp, ti, tv = _device(indptr, indices, data)
    out = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.predict_csr_device(tp.data_ptr(), ti.data_ptr(), tv.data_ptr(), N, M, P, alpha, beta, t, out.data_ptr())
    yd = out.cpu().numpy()
    for got in (yh, yd):
        assert np.all(np.abs(got.astype(np.longdouble) - ref).astype(np.float64) <= bound)
        assert np.all(got[(D != 0).sum(1) == 0] == t) and ((D != 0).sum(1) == 0).any()      # empty rows give exactly t
    assert np.array_equal(yh, yd)
    assert np.array_equal(ctx.predict_csr(ctx_csr(indptr, indices, data, D.shape), P, alpha, beta, t), yh)
    model = partls.PartLSFitResult(alpha, beta, t, P)
    assert np.array_equal(partls.predict(model, ctx_csr(indptr, indices, data, D.shape)), yh)
    ctx.close()


@pytest.mark.parametrize("N,M,K", [(400, 24, 5), (70000, 8, 2)])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_kkt_violation_after_a_fit_matches_the_dense_path(partls, N, M, K, weighted):
    """the winner's data-space KKT check reads the CSR X'r in column order, ones column included (70000 rows: several row slices)"""
    D, S, y, w, P = fit_case(N, M, K, False)
    wt = w if weighted else None
    ctx = partls.default_context(0)
    partls.fit(partls.Opt, D, y, P, weights=wt, on_ill_conditioned="raise")
    dense = ctx.kkt_violation()
    partls.fit(partls.Opt, ctx_csr(*csr_of(D, S), D.shape), y, P, weights=wt, on_ill_conditioned="raise")
    sparse = ctx.kkt_violation()
    print(f"N={N} M={M} weighted={weighted}: kkt dense {dense:.3e} sparse {sparse:.3e}")
    assert sparse <= 4 * dense and sparse < KKT_TOL


# ---- 4. fits ---------------------------------------------------------------------------------------------------------------------------
FIT_SHAPES = [(400, 24, 5, 1), (1200, 200, 4, 2), (1200, 300, 4, 3)]       # route: register kernel 256 threads / 512 threads / deferred


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.all(np.abs(a - b) <= 1e-8 * max(1.0, float(np.max(np.abs(b))))), (what, float(np.max(np.abs(a - b))))


def _same_model(r1, r2, what):
    (m1, _, p1), (m2, _, p2) = r1, r2
    _close(m1.α, m2.α, what + " alpha")
    _close(m1.β, m2.β, what + " beta")
    _close(m1.t, m2.t, what + " t")
    _close(p1["opt"], p2["opt"], what + " opt")


@functools.lru_cache(maxsize=None)
def _oracle_refs(N, M, K, eta):
    from oracle import oracle as O
    O.build()
    D, _, y, _, P = fit_case(N, M, K, False)
    a0, b0 = _start(M, K)
    return O.fit_opt(D, y, P, eta, return_all=True), O.fit_alt(D, y, P, a0, b0, eta), O.fit_bnb(D, y, P, eta)


def _start(M, K):
    rng = np.random.default_rng(3)
    return rng.random(M + 1), (rng.random(K + 1) - 0.5) * 10


def _vs_oracle(res, ref, what):
    m, _, p = res
    _close(p["opt"], ref["opt"], what + " opt (oracle)")
    _close(m.α, ref["alpha"], what + " alpha (oracle)")
    _close(m.β, ref["beta"], what + " beta (oracle)")
    _close(m.t, ref["t"], what + " t (oracle)")


@pytest.mark.parametrize("N,M,K,route", FIT_SHAPES)
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_real_fits_match_the_dense_path_and_the_oracle(partls, N, M, K, route, eta, weighted):
    from oracle import oracle as O
    D, S, y, w, P = fit_case(N, M, K, False)
    X = ctx_csr(*csr_of(D, S), D.shape)
    kw = dict(η=eta, weights=w if weighted else None, on_ill_conditioned="raise")
    ctx = partls.default_context(0)
    # the runner-up is more than 1e-6 relative away in the dense enumeration: a near tie cannot excuse a mismatch
    _, _, full = partls.fit(partls.Opt, D, y, P, returnAllSolutions=True, **kw)
    allopt = np.sort(np.unique(np.asarray(full.solutions._all)))
    assert allopt[1] - allopt[0] > 1e-6 * allopt[0], allopt[:2]
    for faithful in (True, False):
        rd = partls.fit(partls.Opt, D, y, P, faithful_intercept=faithful, **kw)
        rs = partls.fit(partls.Opt, X, y, P, faithful_intercept=faithful, **kw)
        assert ctx.sweep_route()[0] == route
        assert rs[2]["best_index"] == rd[2]["best_index"]
        _same_model(rs, rd, f"Opt faithful={faithful}")
        if not weighted:
            ref = _oracle_refs(N, M, K, eta)[0]
            _vs_oracle(rs, ref, "Opt")
            if faithful:
                assert rs[2]["best_index"] == ref["best_index"]
    if weighted:                                             # the oracle's objective of every pattern on the row-scaled homogeneous problem
        Xo, Po = O.homogeneous(D, P)
        s = np.sqrt(w)
        Xn, yn = O.regularize(Xo * s[:, None], y * s, Po, eta)
        objs = O.opt_patterns(Xn, yn, Po, np.arange(2 ** (K + 1)))
        rs = partls.fit(partls.Opt, X, y, P, faithful_intercept=True, **kw)
        assert rs[2]["best_index"] == int(np.argmin(objs))
        _close(rs[2]["opt"], objs.min(), "weighted Opt opt (oracle)")
    a0, b0 = _start(M, K)
    rs = partls.fit(partls.Alt, X, y, P, alpha0=a0, beta0=b0, **kw)
    _same_model(rs, partls.fit(partls.Alt, D, y, P, alpha0=a0, beta0=b0, **kw), "Alt")
    assert rs[2]["iters"] >= 1
    if not weighted:
        _vs_oracle(rs, _oracle_refs(N, M, K, eta)[1], "Alt")
    rs = partls.fit(partls.Alt, X, y, P, restarts=4, rng=11, **kw)
    rd = partls.fit(partls.Alt, D, y, P, restarts=4, rng=11, **kw)
    assert rs[2]["best_start"] == rd[2]["best_start"]
    _same_model(rs, rd, "Alt restarts=4")
    rs = partls.fit(partls.BnB, X, y, P, **kw)
    _same_model(rs, partls.fit(partls.BnB, D, y, P, **kw), "BnB")
    if not weighted:
        _vs_oracle(rs, _oracle_refs(N, M, K, eta)[2], "BnB")


@pytest.mark.parametrize("N,M,K,route", FIT_SHAPES)
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_integer_fits_see_identical_gram_bits(partls, N, M, K, route, weighted):
    """all_opt, best_index and the top-8 list come from the Gram form alone: equal Gram bits give equal bits here"""
    D, S, y, w, P = fit_case(N, M, K, True)
    X = ctx_csr(*csr_of(D, S), D.shape)
    ctx = partls.default_context(0)
    for eta in (0.0, 0.5):
        kw = dict(η=eta, weights=w if weighted else None, returnAllSolutions=True, top=8, on_ill_conditioned="raise")
        _, _, pd_ = partls.fit(partls.Opt, D, y, P, **kw)
        md, _, ps = partls.fit(partls.Opt, X, y, P, **kw)
        assert ctx.sweep_route()[0] == route
        assert np.array_equal(ps.solutions._all, pd_.solutions._all)
        assert int(np.argmin(ps.solutions._all)) == int(np.argmin(pd_.solutions._all))
        assert np.array_equal(ps.top.pattern, pd_.top.pattern) and np.array_equal(ps.top.opt, pd_.top.opt)
        # three patterns rebuilt after a dense fit has taken the context over (the CSR triple is prepared again on a private context)
        partls.fit(partls.Opt, D[:, :3], y, P[:3, :1] * 0 + 1)
        for b in (0, len(ps.solutions) // 2, len(ps.solutions) - 1):
            (o1, m1), (o2, m2) = ps.solutions[b], pd_.solutions[b]
            assert o1 == o2
            _close(m1.α, m2.α, f"solutions[{b}] alpha")
            _close(m1.β, m2.β, f"solutions[{b}] beta")
            _close(m1.t, m2.t, f"solutions[{b}] t")


def test_rescue_on_a_problem_where_nothing_caps(partls):
    D, S, y, _, P = fit_case(400, 24, 5, False)
    X = ctx_csr(*csr_of(D, S), D.shape)
    m0, _, p0 = partls.fit(partls.Opt, X, y, P)
    m1, _, p1 = partls.fit(partls.Opt, X, y, P, rescue=True)
    assert p1["rescued"] == 0 and p1["best_index"] == p0["best_index"] and p1["opt"] == p0["opt"]
    assert np.array_equal(m1.α, m0.α) and np.array_equal(m1.β, m0.β) and m1.t == m0.t


def test_scipy_input_fits_like_the_numpy_built_triple(partls):
    sp = pytest.importorskip("scipy.sparse")
    D, S, y, _, P = fit_case(400, 24, 5, False)
    m0, _, p0 = partls.fit(partls.Opt, ctx_csr(*csr_of(D), D.shape), y, P)
    m1, _, p1 = partls.fit(partls.Opt, sp.csc_matrix(D), y, P)
    assert p1["opt"] == p0["opt"] and np.array_equal(m1.α, m0.α) and np.array_equal(m1.β, m0.β) and m1.t == m0.t
    assert np.array_equal(partls.predict(m1, sp.coo_matrix(D)), partls.predict(m0, ctx_csr(*csr_of(D), D.shape)))


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------
def _broken(kind):
    D, S, y, w, P = fit_case(400, 24, 5, False)
    indptr, indices, data = (a.copy() for a in csr_of(D, S))
    row = int(np.flatnonzero(np.diff(indptr) >= 2)[2])       # a row with at least two entries
    a = indptr[row]
    w = None
    if kind == "unsorted":
        indices[a], indices[a + 1] = indices[a + 1], indices[a]
    elif kind == "duplicate":
        indices[a + 1] = indices[a]
    elif kind == "index=M":
        indices[indptr[row + 1] - 1] = D.shape[1]
    elif kind == "negative index":
        indices[a] = -1
    elif kind == "indptr[0]=1":
        indptr[0], row = 1, 0
    elif kind == "decreasing indptr":
        indptr[row + 1] = indptr[row] - 1 if indptr[row] > 0 else indptr[row]
        assert indptr[row + 1] < indptr[row]
    elif kind == "nan":
        data[a] = np.nan
    elif kind == "inf":
        data[a + 1] = -np.inf
    elif kind == "negative weight":
        w = np.ones(D.shape[0])
        w[5] = -1.0
    return (indptr, indices, data), D, S, y, w, P, row


@pytest.mark.parametrize("kind,status", [("unsorted", ERR_BAD_ARG), ("duplicate", ERR_BAD_ARG), ("index=M", ERR_BAD_ARG),
                                         ("negative index", ERR_BAD_ARG), ("indptr[0]=1", ERR_BAD_ARG),
                                         ("decreasing indptr", ERR_BAD_ARG), ("nan", ERR_NONFINITE), ("inf", ERR_NONFINITE),
                                         ("negative weight", ERR_BAD_ARG)])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_invalid_input_is_refused_and_leaves_the_context_unprepared(partls, kind, status, device):
    (indptr, indices, data), D, S, y, w, P, row = _broken(kind)
    N, M = D.shape
    ctx = partls.Context(0)
    _prepare_csr(ctx, D, S, y, P, None, False)               # a prepared problem that the failed prepare must not leave behind
    with pytest.raises(partls.PartlsError) as e:
        if device:
            t = _device(indptr, indices, data, y, w)
            ctx.opt_prepare_csr_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), N, M, P,
                                       dw_ptr=None if w is None else t[4].data_ptr())
        else:
            ctx._prepare_csr(indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, y.ctypes.data,
                             None if w is None else w.ctypes.data, 0, N, M, np.asfortranarray(P), 0.0, 0)
    assert e.value.status == status, str(e.value)
    if kind not in ("negative weight",):
        assert "row %d" % row in str(e.value), str(e.value)  # the message names the first offending row
    with pytest.raises(partls.PartlsError) as e2:
        ctx.opt_sweep()
    assert e2.value.status == ERR_STATE
    _prepare_csr(ctx, D, S, y, P, None, device)              # a later valid prepare works
    assert ctx.opt_sweep()[3] == 0
    ctx.close()


def test_a_multicontext_member_refuses_a_sparse_prepare(partls):
    D, S, y, _, P = fit_case(37, 5, 2, False)
    mc = partls.MultiContext([0, 0])
    c0 = mc.context(0)
    with pytest.raises(partls.PartlsError) as e:
        c0.opt_prepare_csr(ctx_csr(*csr_of(D, S), D.shape), y, P)
    assert e.value.status == ERR_UNSUPPORTED
    with pytest.raises(partls.PartlsError) as e2:
        c0.opt_sweep()
    assert e2.value.status == ERR_STATE
    mc.close()


# ---- 6. upload accounting ---------------------------------------------------------------------------------------------------------
def test_upload_accounting(partls):
    D, S, y, w, P = fit_case(2051, 257, 3, False)
    nnz = int(S.sum())
    ctx = partls.Context(0)
    for wt in (None, w):
        _prepare_csr(ctx, D, S, y, P, wt, False)
        assert ctx.upload()[1] == 8 * (2051 + 1) + 12 * nnz
        keep = _prepare_csr(ctx, D, S, y, P, wt, True)
        assert ctx.upload() == (0.0, 0.0)
        del keep
    ctx.close()
