"""partls_cv_opt on the GPU: every (fold, η) problem of one batched call against the single fit(Opt) of its training rows — winner,
model, objective, held-out SSE from numpy — on the golden fixtures, seeded random problems and every sweep route (256-thread kernel,
512-thread kernel with and without winner export, the serial fallback beyond n = 288, the generic kernel, several chains per problem);
batched against PARTLS_CV_SERIAL=1, run-to-run and host-against-device identity, per-problem status, argument errors, the C2 shape."""
import os

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FAITHFUL = 1
GENERIC = 2
NEAR_TIE_REL = 1e-12          # on obj^2 in units of y'y: the documented window (1e-13) with room for the two Gram summation orders


def _fold_ptr(N, F):
    return np.concatenate([[0], np.cumsum([len(a) for a in np.array_split(np.arange(N), F)])]).astype(np.int64)


def _train(N, fold_ptr, f):
    F = len(fold_ptr) - 1
    if f == F:
        return np.ones(N, dtype=bool)
    m = np.ones(N, dtype=bool)
    m[fold_ptr[f]:fold_ptr[f + 1]] = False
    return m


def _heldout(X, y, P, a, b, t, rows):
    w = a * (P @ b)
    r = X[rows] @ w + t - y[rows]
    return float(r @ r)


def _check(partls, oracle, X, y, P, fold_ptr, etas, flags, r, tag):
    """every problem of r against its single fit; returns the number of near-tie winners that differed"""
    N = X.shape[0]
    F, E = len(fold_ptr) - 1, len(etas)
    faithful = bool(flags & FAITHFUL)
    ties = 0
    for f in range(F + 1):
        tr = _train(N, fold_ptr, f)
        for e, eta in enumerate(etas):
            q = f * E + e
            what = f"{tag} f={f} eta={eta}"
            model, _, rep = partls.fit(partls.Opt, X[tr], y[tr], P, η=float(eta), faithful_intercept=faithful,
                                       generic_kernel=bool(flags & GENERIC), on_ill_conditioned="warn")
            ill = bool(rep.get("ill_conditioned", False))
            assert r["status"][q] == (9 if ill else 0), f"{what}: status {r['status'][q]}, single fit ill={ill}"
            yy = float(y[tr] @ y[tr])
            if ill:
                continue                  # the best Gram-form model of a problem the Gram form cannot resolve: nothing to compare to 1e-9
            a, b, t, o, bi = r["alpha"][:, q], r["beta"][:, q], r["t"][q], r["opt"][q], r["best_index"][q]
            Z = np.hstack([X[tr], np.ones((int(tr.sum()), 1))])
            if np.linalg.matrix_rank(Z) < Z.shape[1]:
                # dependent columns on these rows: the minimiser is not unique, only its objective is
                assert abs(o - rep.opt) <= 1e-8 * max(rep.opt, 1e-300) + 1e-12 * np.sqrt(yy), f"{what}: opt {o} vs {rep.opt}"
            elif bi == rep.best_index:
                sc = max(1.0, np.abs(model.α).max(), np.abs(model.β).max())
                assert np.allclose(a, model.α, rtol=0, atol=1e-9 * sc), f"{what}: alpha {np.abs(a - model.α).max()}"
                assert np.allclose(b, model.β, rtol=1e-9, atol=1e-9 * sc), f"{what}: beta {np.abs(b - model.β).max()}"
                assert abs(t - model.t) <= 1e-9 * max(1.0, abs(model.t), np.abs(model.β).max()), f"{what}: t {t} vs {model.t}"
                assert abs(o - rep.opt) <= 1e-10 * max(rep.opt, 1e-300) + 1e-15 * np.sqrt(yy), f"{what}: opt {o} vs {rep.opt}"
            else:
                # both winners within the near-tie window of the training problem, per the oracle's objectives of every pattern
                ref = oracle.fit_opt(X[tr], y[tr], P, eta=float(eta), return_all=True)
                ao = np.asarray(ref["all_opt"])
                lim = NEAR_TIE_REL * yy
                assert abs(ao[bi] ** 2 - ao[rep.best_index] ** 2) <= lim, f"{what}: winners {bi} / {rep.best_index} not a near tie"
                assert abs(o ** 2 - rep.opt ** 2) <= lim, f"{what}: opt {o} vs {rep.opt}"
                ties += 1
            if f < F:
                rows = slice(fold_ptr[f], fold_ptr[f + 1])
                want = _heldout(X, y, P, a, b, t, rows)
                fy = float(y[rows] @ y[rows])
                assert abs(r["heldout_sse"][q] - want) <= 1e-12 * max(want, 1e-300) + 1e-14 * fy, f"{what}: sse {r['heldout_sse'][q]} vs {want}"
            else:
                assert np.isnan(r["heldout_sse"][q])
    return ties


def _run(partls, ctx, X, y, P, fold_ptr, etas, flags=0):
    return ctx.cv_opt(X, y, P, fold_ptr, np.asarray(etas, dtype=np.float64), flags)


@pytest.fixture(scope="module")
def ctx(partls):
    return partls.Context(0)


@pytest.fixture(scope="module")
def ctx_serial(partls):
    old = os.environ.get("PARTLS_CV_SERIAL")
    os.environ["PARTLS_CV_SERIAL"] = "1"
    try:
        c = partls.Context(0)
    finally:
        if old is None:
            del os.environ["PARTLS_CV_SERIAL"]
        else:
            os.environ["PARTLS_CV_SERIAL"] = old
    return c


@pytest.mark.parametrize("name", ["synth_a", "synth_eta", "corr", "toy"])
@pytest.mark.parametrize("flags", [0, FAITHFUL])
def test_golden_problems_match_single_fits(partls, oracle, ctx, name, flags):
    g = load_golden(name)
    X, y, P = g["X"], g["y"], g["P"].astype(np.int64)
    N = X.shape[0]
    fp = _fold_ptr(N, 2 if N < 8 else 5)
    etas = [0.0, 1e-3, 0.5]
    r = _run(partls, ctx, X, y, P, fp, etas, flags)
    _check(partls, oracle, X, y, P, fp, etas, flags, r, f"{name} flags={flags}")


def test_toy_three_folds_of_one_and_two_rows(partls, oracle, ctx):
    g = load_golden("toy")
    X, y, P = g["X"], g["y"], g["P"].astype(np.int64)
    fp = np.array([0, 1, 3, 4], dtype=np.int64)
    r = _run(partls, ctx, X, y, P, fp, [0.0, 0.5], FAITHFUL)
    _check(partls, oracle, X, y, P, fp, [0.0, 0.5], FAITHFUL, r, "toy 1-2-1")


def _random_problem(rng):
    K = int(rng.integers(1, 7))
    sizes = rng.integers(1, 9, size=K)
    D = int(sizes.sum())
    N = int(rng.integers(3 * D + 30, 6 * D + 60))
    P = np.zeros((D, K), dtype=np.int64)
    order = rng.permutation(D) if rng.random() < 0.5 else np.arange(D)     # non-contiguous groups
    c = 0
    for k, s in enumerate(sizes):
        P[order[c:c + s], k] = 1
        c += s
    if K >= 2 and rng.random() < 0.3:
        P[rng.integers(0, D), rng.integers(0, K)] = 1                        # overlapping partition
    X = rng.standard_normal((N, D))
    if rng.random() < 0.4:
        X *= np.exp(rng.uniform(-3, 3, size=D))[None, :]                    # badly scaled columns
    kind = rng.random()
    if kind < 0.15 and D >= 3:
        X[:, rng.integers(0, D)] = X[:, rng.integers(0, D)]                 # duplicate column
    elif kind < 0.3 and D >= 3:
        X[:, rng.integers(0, D)] = 0.0                                      # null column
    elif kind < 0.4 and D >= 4:
        i, j, l = rng.choice(D, 3, replace=False)
        X[:, i] = 0.5 * X[:, j] - 2.0 * X[:, l]                             # dependent triple
    grp = P.argmax(1)
    y = X @ (rng.random(D) * ((rng.random(K) - 0.5) * 10)[grp]) + rng.uniform(-2, 2) + rng.choice([1e-3, 0.3, 3.0]) * rng.standard_normal(N)
    # fold boundaries at odd rows
    # fold boundaries at odd rows; every training set keeps more rows than variables
    F = int(rng.integers(2, 5))
    while True:
        cuts = np.sort(rng.choice(np.arange(1, N // 2) * 2 - 1, F - 1, replace=False))
        fp = np.concatenate([[0], cuts, [N]]).astype(np.int64)
        if np.diff(fp).max() <= N - D - 8:
            return X, y, P, fp


@pytest.mark.parametrize("block", range(4))
def test_random_problems_match_single_fits(partls, oracle, ctx, block):
    rng = np.random.default_rng(77000 + block)
    for it in range(11):
        X, y, P, fp = _random_problem(rng)
        flags = FAITHFUL if it % 2 else 0
        etas = [0.0, 1e-3, 0.5]
        r = _run(partls, ctx, X, y, P, fp, etas, flags)
        _check(partls, oracle, X, y, P, fp, etas, flags, r, f"block {block} it {it} {X.shape} K={P.shape[1]} folds={list(fp)}")


def _shape(seed, N, D, K):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    grp = np.arange(D) % K
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    y = X @ (rng.random(D) * ((rng.random(K) - 0.5) * 10)[grp]) + 0.7 + 0.5 * rng.standard_normal(N)
    return X, y, P


# n = 200: 512-thread kernel with winner export (T = 13); n = 280: T = 18 without export; n = 300: beyond the register kernel (serial
# fallback on the deferred-update kernel); n = 40 under PARTLS_OPT_GENERIC_KERNEL; K = 12: several chains per problem
@pytest.mark.parametrize("N,D,K,flags", [(500, 200, 3, 0), (600, 280, 3, 0), (640, 300, 3, 0), (600, 40, 4, GENERIC), (900, 48, 12, 0)])
def test_every_sweep_route(partls, oracle, ctx, N, D, K, flags):
    X, y, P = _shape(1234 + D, N, D, K)
    fp = np.array([0, 101, 333, N], dtype=np.int64)
    etas = [0.0, 0.5]
    r = _run(partls, ctx, X, y, P, fp, etas, flags)
    _check(partls, oracle, X, y, P, fp, etas, flags, r, f"route N={N} D={D} K={K} flags={flags}")


def _same(a, b):
    for k in ("alpha", "beta", "t", "opt", "best_index", "heldout_sse", "status"):
        assert np.array_equal(a[k], b[k], equal_nan=k not in ("best_index", "status")), k


@pytest.mark.parametrize("D,K", [(24, 5), (200, 3)])
def test_batched_matches_serial_and_repeats_bitwise(partls, ctx, ctx_serial, D, K):
    X, y, P = _shape(99 + D, 700, D, K)
    fp = _fold_ptr(700, 5)
    etas = np.array([0.0, 1e-3, 0.5, 2.0])
    a = _run(partls, ctx, X, y, P, fp, etas)
    b = _run(partls, ctx, X, y, P, fp, etas)
    _same(a, b)
    s = _run(partls, ctx_serial, X, y, P, fp, etas)
    assert np.array_equal(a["status"], s["status"])
    for q in range(len(a["t"])):
        if a["best_index"][q] == s["best_index"][q]:
            sc = max(1.0, np.abs(s["alpha"][:, q]).max(), np.abs(s["beta"][:, q]).max())
            assert np.allclose(a["alpha"][:, q], s["alpha"][:, q], rtol=0, atol=1e-9 * sc)
            assert np.allclose(a["beta"][:, q], s["beta"][:, q], rtol=1e-9, atol=1e-9 * sc)
            assert abs(a["opt"][q] - s["opt"][q]) <= 1e-10 * s["opt"][q]
        else:
            assert abs(a["opt"][q] ** 2 - s["opt"][q] ** 2) <= NEAR_TIE_REL * float(y @ y)
    ok = ~np.isnan(s["heldout_sse"])
    assert np.allclose(a["heldout_sse"][ok], s["heldout_sse"][ok], rtol=1e-9, atol=0)


def _agree(a, s):
    """two routes of one call: the same statuses and winners, models and objectives within the tolerances of batched against serial"""
    assert np.array_equal(a["status"], s["status"])
    assert np.array_equal(a["best_index"], s["best_index"])
    for q in range(len(a["t"])):
        sc = max(1.0, np.abs(s["alpha"][:, q]).max(), np.abs(s["beta"][:, q]).max())
        assert np.allclose(a["alpha"][:, q], s["alpha"][:, q], rtol=0, atol=1e-9 * sc), q
        assert np.allclose(a["beta"][:, q], s["beta"][:, q], rtol=1e-9, atol=1e-9 * sc), q
        assert abs(a["opt"][q] - s["opt"][q]) <= 1e-10 * s["opt"][q], q
    ok = ~np.isnan(s["heldout_sse"])
    assert np.array_equal(ok, ~np.isnan(a["heldout_sse"]))
    assert np.allclose(a["heldout_sse"][ok], s["heldout_sse"][ok], rtol=1e-9, atol=0)


@pytest.fixture(scope="module")
def ctx_pieces(partls):
    """contexts whose batched route takes PARTLS_BATCH_PIECE problems per piece (read at partls_create)"""
    made = {}
    old = os.environ.get("PARTLS_BATCH_PIECE")
    try:
        for piece in (3, 1):
            os.environ["PARTLS_BATCH_PIECE"] = str(piece)
            made[piece] = partls.Context(0)
    finally:
        if old is None:
            del os.environ["PARTLS_BATCH_PIECE"]
        else:
            os.environ["PARTLS_BATCH_PIECE"] = old
    return made


# 256-thread kernel; 512-thread kernel with winner export; T = 18 without export.  B = 8 problems, E = 2: pieces of 3 begin at q0 = 3 (not
# a multiple of E) and 6, and the fold changes inside each.  The gap between the best and the second-best pattern of every problem
# (oracle, in units of y'y on obj^2) is at least 7.0e-4, 4.0e-4 and 1.5e-6, far from the near-tie window: the winners must be equal.
PIECE_SHAPES = {"n24": (99 + 24, 700, 24, 5, None), "n200": (99 + 200, 700, 200, 3, None), "n280": (1234 + 280, 600, 280, 3, [0, 101, 333, 600])}
PIECE_ETAS = [0.0, 0.5]


@pytest.fixture(scope="module")
def piece_refs(partls, ctx, ctx_serial):
    """per shape, computed once: the problem and its unpieced and serial results"""
    refs = {}

    def get(name):
        if name not in refs:
            seed, N, D, K, fp = PIECE_SHAPES[name]
            X, y, P = _shape(seed, N, D, K)
            fp = _fold_ptr(N, 3) if fp is None else np.asarray(fp, dtype=np.int64)
            refs[name] = (X, y, P, fp, _run(partls, ctx, X, y, P, fp, PIECE_ETAS), _run(partls, ctx_serial, X, y, P, fp, PIECE_ETAS))
        return refs[name]
    return get


@pytest.mark.parametrize("piece", [3, 1])
@pytest.mark.parametrize("name", list(PIECE_SHAPES))
def test_pieces_of_the_batch(partls, oracle, ctx_pieces, piece_refs, name, piece):
    X, y, P, fp, whole, serial = piece_refs(name)
    assert len(whole["t"]) == 8
    a = _run(partls, ctx_pieces[piece], X, y, P, fp, PIECE_ETAS)
    _same(a, _run(partls, ctx_pieces[piece], X, y, P, fp, PIECE_ETAS))
    assert _check(partls, oracle, X, y, P, fp, PIECE_ETAS, 0, a, f"{name} pieces of {piece}") == 0
    _agree(a, whole)
    _agree(a, serial)


def test_host_and_device_inputs_agree_bitwise(partls, ctx):
    import torch
    X, y, P = _shape(5, 800, 30, 4)
    fp = np.array([0, 3, 257, 511, 800], dtype=np.int64)
    etas = [0.0, 0.1]
    a = _run(partls, ctx, X, y, P, fp, etas, FAITHFUL)
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()                   # (D, N) row-major = X column-major, ld N
    dy = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    torch.cuda.synchronize()
    b = ctx.cv_opt(None, None, P, fp, np.asarray(etas), FAITHFUL, device_ptrs=(dX.data_ptr(), dy.data_ptr(), 800, 800))
    _same(a, b)


def test_ill_conditioned_fold_only_flags_its_problem(partls, oracle, ctx):
    rng = np.random.default_rng(42)
    N, D, K = 1500, 24, 4
    Z = rng.standard_normal((N, 6))
    A = rng.standard_normal((6, D))
    noise = np.full((N, 1), 1e-7)
    noise[:500] = 1e-2                        # fold 0 carries the rows that resolve the columns: training set 0 lacks them
    X = Z @ A + noise * rng.standard_normal((N, D))
    grp = np.arange(D) % K
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    y = X @ (rng.random(D) * np.array([1., -2, 3, -1])[grp]) + 0.3 + 0.05 * rng.standard_normal(N)
    fp = np.array([0, 500, 1000, 1500], dtype=np.int64)
    r = _run(partls, ctx, X, y, P, fp, [0.0])
    assert r["status"][0] == 9 and np.all(r["status"][1:] == 0), r["status"]
    _check(partls, oracle, X, y, P, fp, [0.0], 0, r, "ill-conditioned fold")


@pytest.mark.parametrize("fold_ptr,etas", [
    ([0, 50], [0.0]),                          # F = 1
    ([0, 30, 30, 50], [0.0]),                  # not strictly increasing
    ([0, 20, 49], [0.0]),                      # fold_ptr[F] != N
    ([0, 20, 50], []),                         # E = 0
    ([0, 20, 50], [0.0, -1.0]),                # negative eta
    ([0, 20, 50], [float("nan")]),             # NaN eta
])
def test_bad_arguments_write_nothing(partls, ctx, fold_ptr, etas):
    import ctypes as C
    L = partls.lowlevel
    X, y, P = _shape(3, 50, 6, 2)
    Xf = np.asfortranarray(X)
    fp = np.asarray(fold_ptr, dtype=np.int64)
    et = np.asarray(etas if etas else [0.0], dtype=np.float64)
    E = len(etas)
    F = len(fp) - 1
    B = (F + 1) * max(E, 1)
    outs = [np.full((6, B), 7.0, order="F"), np.full((2, B), 7.0, order="F"), np.full(B, 7.0), np.full(B, 7.0),
            np.full(B, 7, dtype=np.int64), np.full(B, 7.0), np.full(B, 7, dtype=np.int32)]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))       # noqa: E731
    st = L.lib().partls_cv_opt(ctx._h, Xf.ctypes.data, 50, 6, 50, y.ctypes.data, 0, P.ctypes.data, 2, 6,
                               fp.ctypes.data_as(C.POINTER(C.c_int64)), F, dp(et), E, 0, dp(outs[0]), 6, dp(outs[1]), 2, dp(outs[2]),
                               dp(outs[3]), outs[4].ctypes.data_as(C.POINTER(C.c_int64)), dp(outs[5]),
                               outs[6].ctypes.data_as(C.POINTER(C.c_int32)))
    assert st == L.ERR_BAD_ARG
    for o in outs:
        assert np.all(o == 7)


def test_c2_shape_matches_its_single_fits(partls, oracle, ctx):
    X, y, P, _ = oracle.synth(20260002, 10_000, 128, 12)
    fp = _fold_ptr(10_000, 5)
    etas = [0.0, 1e-3, 0.1, 1.0]
    r = _run(partls, ctx, X, y, P, fp, etas)
    _check(partls, oracle, X, y, P, fp, etas, 0, r, "C2")


def test_cross_validate_end_to_end(partls):
    X, y, P = _shape(11, 400, 12, 3)
    res = partls.cross_validate(partls.Opt, X, y, P, η=[0.0, 0.5, 5.0], nfolds=4, shuffle=True, rng=3)
    assert res.sse.shape == (4, 3) and res.mse.shape == (4, 3)
    assert np.allclose(res.mse_mean, res.sse.sum(0) / 400)
    assert res.best_eta == res.etas[int(np.argmin(res.mse_mean))]
    Xp, yp = X[res.perm], y[res.perm]
    tr = np.ones(400, dtype=bool)
    tr[res.fold_ptr[1]:res.fold_ptr[2]] = False
    m, _, rep = partls.fit(partls.Opt, Xp[tr], yp[tr], P, η=0.5)
    assert np.allclose(res.models[1][1].α, m.α, atol=1e-9) and np.allclose(res.models[1][1].β, m.β, rtol=1e-9, atol=1e-9)
    full, _, _ = partls.fit(partls.Opt, X, y, P, η=float(res.best_eta))
    assert np.allclose(res.model.α, full.α, atol=1e-9)
