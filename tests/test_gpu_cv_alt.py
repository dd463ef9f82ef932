"""GPU tests of the cross-validated multistart fit(Alt) (partls_cv_alt): every stable trajectory of every (fold, η)
problem against the dense CPU oracle's fit of the training rows, every problem's winner, the held-out SSE from numpy, the single
device fit bit for bit, the batched route against PARTLS_CV_SERIAL=1 bit for bit, independence of the grid, the chunking and the
order of the starts, more slots than one grid dimension, per-trajectory failures, weights, device-resident inputs, the end-to-end
η choice and argument errors.

Data (the recipe of test_gpu_alt_multistart.py): rng = default_rng(seed); X = standard_normal((N, D)); P[m, m % K] = 1;
y = X @ standard_normal(D) + 0.2 standard_normal(N); starts from default_rng(123); folds from cv_folds without shuffle; eps = 1e-6.

Stability mask (computed on the oracle side, asserted per fixture): a trajectory is stable when the oracle's iteration count is the
same at eps / 2, eps and 2 eps AND its opt moves by <= 1e-9 relative when X is multiplied elementwise by 1 + 1e-13 N(0, 1)
(default_rng(seed + 1)) — the stand-in for the second Gram summation order of the fold sums: Alt's beta-step can flip a sign on
less.  Unstable trajectories are left out of the comparison with the oracle, and they may be at most 1/8 of a fixture's."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 1e-6
# name: seed, N, D, K, F, etas, R, T, sweep route and tile count of the shape (None: not asserted; DEFERRED: n > 288, hence the serial
# route of partls_cv_alt), unstable trajectories (oracle side)
FIXTURES = {
    "A5": dict(seed=7, N=400, D=36, K=6, F=5, etas=[0.0, 1.0, 10.0, 100.0, 1000.0], R=8, T=100, route="REG_256", tiles=None, unstable=14),
    "C3": dict(seed=19, N=400, D=90, K=45, F=3, etas=[0.0, 2.0, 20.0, 200.0], R=8, T=100, route=None, tiles=None, unstable=0),
    "B":  dict(seed=11, N=120, D=11, K=3, F=4, etas=[0.0, 0.1], R=8, T=100, route="REG_256", tiles=1, unstable=4),
    "D":  dict(seed=23, N=500, D=200, K=5, F=2, etas=[0.0, 1.0], R=4, T=40, route="REG_512", tiles=None, unstable=0),
    "E":  dict(seed=17, N=600, D=300, K=4, F=2, etas=[0.0, 1.0], R=3, T=40, route="DEFERRED", tiles=None, unstable=2),
}
PER_START = ("opt", "iters", "status")
PER_PROBLEM = ("alpha", "beta", "t", "opt", "iters", "best_start", "heldout_sse", "status")


def _data(seed, N, D, K, R):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), np.arange(D) % K] = 1
    y = X @ rng.standard_normal(D) + 0.2 * rng.standard_normal(N)
    gen = np.random.default_rng(123)
    a0 = np.empty((R, D + 1))
    b0 = np.empty((R, K + 1))
    for r in range(R):
        a0[r] = gen.random(D + 1)
        b0[r] = (gen.random(K + 1) - 0.5) * 10
    for v in (X, y, P, a0, b0):
        v.setflags(write=False)
    return X, y, P, a0, b0


@functools.lru_cache(maxsize=None)
def problem(name):
    import partls_amd
    f = FIXTURES[name]
    fold_ptr, _ = partls_amd.package().cv_folds(f["N"], f["F"])
    return _data(f["seed"], f["N"], f["D"], f["K"], f["R"]) + (fold_ptr,)


def _train(N, fold_ptr, f):
    m = np.ones(N, dtype=bool)
    if f < len(fold_ptr) - 1:
        m[fold_ptr[f]:fold_ptr[f + 1]] = False
    return m


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's fit of every trajectory (computed once per fixture, shared, read-only): dict of opt, iters [F+1, E, R], alpha
    [F+1, E, R, M], beta [F+1, E, R, K], t [F+1, E, R] and the stability mask [F+1, E, R]"""
    from oracle import oracle as O
    O.build()
    f = FIXTURES[name]
    X, y, P, a0, b0, fold_ptr = problem(name)
    F, E, R, M, K = f["F"], len(f["etas"]), f["R"], f["D"], f["K"]
    Xp = X * (1.0 + 1e-13 * np.random.default_rng(f["seed"] + 1).standard_normal(X.shape))
    out = dict(opt=np.zeros((F + 1, E, R)), iters=np.zeros((F + 1, E, R), dtype=np.int64), alpha=np.zeros((F + 1, E, R, M)),
               beta=np.zeros((F + 1, E, R, K)), t=np.zeros((F + 1, E, R)), stable=np.zeros((F + 1, E, R), dtype=bool))
    for fo in range(F + 1):
        tr = _train(f["N"], fold_ptr, fo)
        Xt, yt, Xpt = np.asfortranarray(X[tr]), np.ascontiguousarray(y[tr]), np.asfortranarray(Xp[tr])
        for e, eta in enumerate(f["etas"]):
            for r in range(R):
                ref = O.fit_alt(Xt, yt, P, a0[r], b0[r], eta, eps=EPS, T=f["T"])
                its = [O.fit_alt(Xt, yt, P, a0[r], b0[r], eta, eps=ee, T=f["T"])["iters"] for ee in (2 * EPS, EPS / 2)]
                po = O.fit_alt(Xpt, yt, P, a0[r], b0[r], eta, eps=EPS, T=f["T"])["opt"]
                out["opt"][fo, e, r], out["iters"][fo, e, r], out["t"][fo, e, r] = ref["opt"], ref["iters"], ref["t"]
                out["alpha"][fo, e, r], out["beta"][fo, e, r] = ref["alpha"], ref["beta"]
                out["stable"][fo, e, r] = its[0] == ref["iters"] == its[1] and abs(po - ref["opt"]) <= 1e-9 * ref["opt"]
    for v in out.values():
        v.setflags(write=False)
    return out


def _context(partls, **env):
    """a fresh context created under the given environment knobs (they are read at partls_create)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return partls.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _cv_alt(partls, X, y, P, fold_ptr, etas, a0, b0, T, weights=None, flags=0, **env):
    ctx = _context(partls, **env)
    try:
        return ctx.cv_alt(X, y, P, fold_ptr if len(fold_ptr) > 1 else None, np.asarray(etas, dtype=np.float64), a0, b0, EPS, T,
                          weights=weights, flags=flags)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def device(name, serial=False):
    import partls_amd
    partls = partls_amd.package()
    f = FIXTURES[name]
    X, y, P, a0, b0, fold_ptr = problem(name)
    env = dict(PARTLS_CV_SERIAL=1) if serial else {}
    return _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0, b0, f["T"], **env)


def _same(a, b, cols=slice(None), cols_b=None, starts=slice(None), starts_b=None):
    cols_b = cols if cols_b is None else cols_b
    starts_b = starts if starts_b is None else starts_b
    for k in PER_PROBLEM:
        assert np.array_equal(np.asarray(a[k])[..., cols], np.asarray(b[k])[..., cols_b], equal_nan=True), k
    for k in PER_START:
        assert np.array_equal(a["starts"][k][cols][:, starts], b["starts"][k][cols_b][:, starts_b], equal_nan=True), k


def _same_trajectories(a, b, cols=slice(None), cols_b=None, starts=slice(None), starts_b=None):
    cols_b = cols if cols_b is None else cols_b
    starts_b = starts if starts_b is None else starts_b
    for k in PER_START:
        assert np.array_equal(a["starts"][k][cols][:, starts], b["starts"][k][cols_b][:, starts_b], equal_nan=True), k


def test_fixture_facts_of_the_oracle():
    """what the fixtures were chosen for, asserted on the oracle side before the device is compared"""
    ra = reference("A5")
    win = ra["opt"].argmin(axis=2)
    srt = np.sort(ra["opt"], axis=2)
    gap = (srt[..., 1] / srt[..., 0] - 1.0).min()
    print("A5: winners", np.unique(win), "smallest gap %.4f" % gap)
    assert np.all(win == 7) and 0.0024 < gap < 0.0026
    rb = reference("B")
    sb = np.sort(rb["opt"], axis=2)
    assert np.any(sb[..., 1] - sb[..., 0] <= 1e-9 * sb[..., 0])              # exact ties between starts (up to the oracle's rounding)
    rd = reference("D")
    sd = np.sort(rd["opt"], axis=2)
    gd = (sd[..., 1] / sd[..., 0] - 1.0).min()
    print("D: smallest gap %.4f" % gd)
    assert 0.175 < gd < 0.177
    for name, f in FIXTURES.items():
        st = reference(name)["stable"]
        print(name, "unstable", int((~st).sum()), "of", st.size)
        assert int((~st).sum()) == f["unstable"] and 8 * f["unstable"] <= st.size, name


def _pooled_mse(name, sse):
    f = FIXTURES[name]
    return sse.reshape(f["F"] + 1, -1)[:f["F"]].sum(axis=0) / f["N"]


def _oracle_mse(name):
    f = FIXTURES[name]
    X, y, P, _, _, fold_ptr = problem(name)
    ref = reference(name)
    E = len(f["etas"])
    sse = np.zeros((f["F"], E))
    for fo in range(f["F"]):
        rows = slice(fold_ptr[fo], fold_ptr[fo + 1])
        for e in range(E):
            r = int(ref["opt"][fo, e].argmin())
            w = ref["alpha"][fo, e, r] * (P @ ref["beta"][fo, e, r])
            res = X[rows] @ w + ref["t"][fo, e, r] - y[rows]
            sse[fo, e] = res @ res
    return sse.sum(axis=0) / f["N"]


@pytest.mark.parametrize("name,want,best,margin", [("A5", [18.821, 18.778, 18.622, 21.479, 33.718], 2, 0.008),
                                                   ("C3", [15.947, 15.855, 17.854, 39.172], 1, 0.006)])
def test_eta_choice_of_the_oracle(name, want, best, margin):
    mse = _oracle_mse(name)
    print(name, "pooled held-out MSE of the oracle", mse)
    assert np.allclose(mse, want, atol=2e-3)
    order = np.sort(mse)
    assert int(mse.argmin()) == best and order[1] / order[0] - 1.0 > 0.9 * margin


@pytest.mark.parametrize("name", list(FIXTURES))
def test_every_stable_trajectory_equals_the_oracle(partls, name):
    f = FIXTURES[name]
    ref = reference(name)
    r = device(name)
    F, E, R = f["F"], len(f["etas"]), f["R"]
    so, si, ss = (r["starts"][k].reshape(F + 1, E, R) for k in PER_START)
    assert np.all(ss == partls.lowlevel.OK) and np.all(r["status"] == 0)
    st = ref["stable"]
    err = np.abs(so - ref["opt"]) / np.maximum(1.0, ref["opt"])
    print(name, "worst opt error of a stable trajectory %.3g, iteration mismatches %d" % (err[st].max(), int((si != ref["iters"])[st].sum())))
    assert np.all(err[st] <= 1e-8)
    assert np.array_equal(si[st], ref["iters"][st])
    # every problem's winner
    for fo in range(F + 1):
        for e in range(E):
            q = fo * E + e
            oo = ref["opt"][fo, e]
            order = np.argsort(oo, kind="stable")
            assert abs(r["opt"][q] - oo[order[0]]) <= 1e-8 * max(1.0, oo[order[0]]), (fo, e)
            if R > 1 and oo[order[1]] > oo[order[0]] * (1.0 + 1e-6):
                assert r["best_start"][q] == order[0], (fo, e)
            b = int(r["best_start"][q])
            if st[fo, e, b]:
                np.testing.assert_allclose(r["alpha"][:, q], ref["alpha"][fo, e, b], atol=1e-6, err_msg=str((fo, e)))
                np.testing.assert_allclose(r["beta"][:, q], ref["beta"][fo, e, b], atol=1e-6, err_msg=str((fo, e)))
                assert abs(r["t"][q] - ref["t"][fo, e, b]) <= 1e-6, (fo, e)
            assert r["iters"][q] == si[fo, e, b]


@pytest.mark.parametrize("name", ["A5", "C3", "B"])
def test_heldout_sse_is_the_returned_models(partls, name):
    f = FIXTURES[name]
    X, y, P, _, _, fold_ptr = problem(name)
    r = device(name)
    E = len(f["etas"])
    for q in range((f["F"] + 1) * E):
        fo = q // E
        if fo == f["F"]:
            assert np.isnan(r["heldout_sse"][q])
            continue
        rows = slice(fold_ptr[fo], fold_ptr[fo + 1])
        w = r["alpha"][:, q] * (P @ r["beta"][:, q])
        res = X[rows] @ w + r["t"][q] - y[rows]
        want, fy = float(res @ res), float(y[rows] @ y[rows])
        assert abs(r["heldout_sse"][q] - want) <= 1e-12 * max(want, 1e-300) + 1e-14 * fy, q


@pytest.mark.parametrize("name", ["A5", "B", "D", "E"])
def test_no_folds_one_eta_is_the_single_fit_bit_for_bit(partls, name):
    f = FIXTURES[name]
    X, y, P, a0, b0, _ = problem(name)
    eta = f["etas"][1]
    r = _cv_alt(partls, X, y, P, [0], [eta], a0, b0, f["T"])
    model, _, rep = partls.fit(partls.Alt, X, y, P, η=eta, ϵ=EPS, T=f["T"], alpha0=a0, beta0=b0)
    route = partls.default_context(0).sweep_route()
    if f["route"] is not None:
        assert route[0] == getattr(partls.lowlevel, "ROUTE_" + f["route"]), route
    if f["tiles"] is not None:
        assert route[1] == f["tiles"], route
    for k in PER_START:
        assert np.array_equal(r["starts"][k][0], rep.starts[k], equal_nan=True), k
    assert np.array_equal(r["alpha"][:, 0], model.α) and np.array_equal(r["beta"][:, 0], model.β) and r["t"][0] == model.t
    assert r["opt"][0] == rep.opt and r["iters"][0] == rep.iters and r["best_start"][0] == rep.best_start
    assert np.isnan(r["heldout_sse"][0]) and r["status"][0] == 0


@pytest.mark.parametrize("name", ["A5", "C3", "B"])
def test_batched_equals_serial_and_repeats_bit_for_bit(partls, name):
    f = FIXTURES[name]
    X, y, P, a0, b0, fold_ptr = problem(name)
    _same(device(name), device(name, serial=True))
    _same(device(name), _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0, b0, f["T"]))


def test_a_column_does_not_depend_on_the_grid_the_chunking_or_the_start_order(partls):
    f = FIXTURES["A5"]
    X, y, P, a0, b0, fold_ptr = problem("A5")
    full = device("A5")
    E, e = len(f["etas"]), 2                                               # eta = 10
    cols = slice(e, None, E)
    alone = _cv_alt(partls, X, y, P, fold_ptr, [f["etas"][e]], a0, b0, f["T"])
    _same(full, alone, cols=cols, cols_b=slice(None))
    chunked = _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0, b0, f["T"], PARTLS_ALT_MS_CHUNK=5)    # chunks straddle problems
    _same(full, chunked)
    rev = _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0[::-1], b0[::-1], f["T"])
    _same_trajectories(full, rev, starts_b=slice(None, None, -1))
    for k in ("alpha", "beta", "t", "opt", "iters", "heldout_sse", "status"):
        assert np.array_equal(full[k], rev[k], equal_nan=True), k
    assert np.array_equal(rev["best_start"], f["R"] - 1 - full["best_start"])                # A5 has no exact ties between starts


@pytest.mark.parametrize("name,env", [("A5", dict(PARTLS_BATCH_PIECE=3)), ("A5", dict(PARTLS_BATCH_PIECE=1)),
                                      ("B", dict(PARTLS_BATCH_PIECE=3)), ("B", dict(PARTLS_BATCH_PIECE=1)),
                                      ("A5", dict(PARTLS_BATCH_PIECE=3, PARTLS_ALT_MS_CHUNK=5))])
def test_pieces_of_the_batch(partls, name, env):
    """the problems prepared and iterated a piece at a time (pieces of 3 cut through a fold's eta grid: E = 5 and 2), alone and with
    the trajectories of a piece chunked as well: a problem's trajectories do not depend on its neighbours, so everything is bitwise"""
    f = FIXTURES[name]
    X, y, P, a0, b0, fold_ptr = problem(name)
    pieced = _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0, b0, f["T"], **env)
    _same(pieced, device(name))
    _same(pieced, device(name, serial=True))


def test_more_slots_than_one_grid_dimension(partls, oracle):
    N, D, K, F, R = 40, 3, 2, 5, 1400
    etas = [0.0, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0]
    X, y, P, a0, b0 = _data(5, N, D, K, R)
    fold_ptr, _ = partls.cv_folds(N, F)
    assert (F + 1) * len(etas) * R == 67200 > 65535
    r = _cv_alt(partls, X, y, P, fold_ptr, etas, a0, b0, 100)
    s = _cv_alt(partls, X, y, P, fold_ptr, etas, a0, b0, 100, PARTLS_CV_SERIAL=1)
    _same(r, s)
    assert np.all(r["starts"]["status"] == 0)
    pick = np.random.default_rng(0).choice(67200, size=64, replace=False)
    bad = 0
    for g in pick:
        q, st = divmod(int(g), R)
        fo, e = divmod(q, len(etas))
        tr = _train(N, fold_ptr, fo)
        Xt, yt = np.asfortranarray(X[tr]), np.ascontiguousarray(y[tr])
        ref = oracle.fit_alt(Xt, yt, P, a0[st], b0[st], etas[e], eps=EPS, T=100)
        its = [oracle.fit_alt(Xt, yt, P, a0[st], b0[st], etas[e], eps=ee, T=100)["iters"] for ee in (2 * EPS, EPS / 2)]
        if not (its[0] == ref["iters"] == its[1]):
            bad += 1
            continue
        assert abs(r["starts"]["opt"][q, st] - ref["opt"]) <= 1e-8 * max(1.0, ref["opt"]), g
        assert r["starts"]["iters"][q, st] == ref["iters"], g
    assert 8 * bad <= 64


def test_a_nonfinite_start_fails_in_every_problem_and_leaves_the_others_alone(partls):
    f = FIXTURES["A5"]
    X, y, P, a0, b0, fold_ptr = problem("A5")
    full = device("A5")
    bad = b0.copy()
    bad[2, 0] = np.nan
    r = _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0, bad, f["T"])
    st = r["starts"]["status"]
    assert np.all(st[:, 2] == partls.lowlevel.ERR_NONFINITE) and np.all(np.delete(st, 2, axis=1) == 0)
    assert np.all(np.isnan(r["starts"]["opt"][:, 2])) and np.all(r["starts"]["iters"][:, 2] == 0)
    keep = np.arange(f["R"]) != 2
    _same_trajectories(full, r, starts=keep)
    _same(full, r, starts=keep)                                                  # start 7 wins every problem of A5: the models stand


def test_the_pivot_cap_fails_every_problem_and_the_call_returns(partls):
    """A5's data at eta = 0 and 1, where no alpha-step ends within one round (B's one-tile alpha-steps do; so do some of A5's at
    eta = 10).  On the whole grid the two routes attribute the cap hits to the same trajectories."""
    f = FIXTURES["A5"]
    X, y, P, a0, b0, fold_ptr = problem("A5")
    for env in (dict(), dict(PARTLS_CV_SERIAL=1)):
        r = _cv_alt(partls, X, y, P, fold_ptr, [0.0, 1.0], a0, b0, f["T"], PARTLS_ALT_MS_MAX_ROUNDS=1, **env)
        assert np.all(r["status"] == partls.lowlevel.ERR_NOT_CONVERGED) and np.all(r["best_start"] == -1) and np.all(r["iters"] == 0)
        assert np.all(np.isnan(r["alpha"])) and np.all(np.isnan(r["beta"])) and np.all(np.isnan(r["t"])) and np.all(np.isnan(r["opt"]))
        assert np.all(np.isnan(r["heldout_sse"]))
        assert np.all(r["starts"]["status"] == partls.lowlevel.ERR_NOT_CONVERGED) and np.all(np.isnan(r["starts"]["opt"]))
    capped = _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0, b0, f["T"], PARTLS_ALT_MS_MAX_ROUNDS=1)
    st = capped["starts"]["status"]
    print("pivot cap, whole grid: %d of %d trajectories finish, problems with a winner:" % (int((st == 0).sum()), st.size), np.flatnonzero(capped["status"] == 0))
    assert np.all((st == 0) | (st == partls.lowlevel.ERR_NOT_CONVERGED))
    _same(capped, _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0, b0, f["T"], PARTLS_ALT_MS_MAX_ROUNDS=1, PARTLS_CV_SERIAL=1))
    full = device("A5")
    ok = st == 0                                                                # a trajectory the cap never touched is the uncapped one
    for k in PER_START:
        assert np.array_equal(capped["starts"][k][ok], full["starts"][k][ok]), k


def test_weights(partls):
    f = FIXTURES["B"]
    X, y, P, a0, b0, fold_ptr = problem("B")
    w = np.random.default_rng(3).uniform(0.5, 2.0, size=f["N"])
    r = _cv_alt(partls, X, y, P, fold_ptr, f["etas"], a0, b0, f["T"], weights=w)
    E = len(f["etas"])
    for q in range((f["F"] + 1) * E):
        fo, e = divmod(q, E)
        tr = _train(f["N"], fold_ptr, fo)
        m, _, rep = partls.fit(partls.Alt, X[tr], y[tr], P, η=f["etas"][e], ϵ=EPS, T=f["T"], alpha0=a0, beta0=b0, weights=w[tr])
        print("weights: problem", q, "opt %.15g (single fit %.15g)" % (r["opt"][q], rep.opt))
        assert abs(r["opt"][q] - rep.opt) <= 1e-9 * max(1.0, rep.opt), q
        np.testing.assert_allclose(r["starts"]["opt"][q], rep.starts.opt, rtol=1e-9, atol=1e-9, err_msg=str(q))
        if r["best_start"][q] == rep.best_start:
            np.testing.assert_allclose(r["alpha"][:, q], m.α, rtol=0, atol=1e-9 * max(1.0, np.abs(m.α).max()), err_msg=str(q))
            np.testing.assert_allclose(r["beta"][:, q], m.β, rtol=0, atol=1e-9 * max(1.0, np.abs(m.β).max()), err_msg=str(q))
            assert abs(r["t"][q] - m.t) <= 1e-9 * max(1.0, abs(m.t)), q
        if fo < f["F"]:
            rows = slice(fold_ptr[fo], fold_ptr[fo + 1])
            res = X[rows] @ (r["alpha"][:, q] * (P @ r["beta"][:, q])) + r["t"][q] - y[rows]
            want = float((w[rows] * res) @ res)
            assert abs(r["heldout_sse"][q] - want) <= 1e-12 * want + 1e-14 * float((w[rows] * y[rows]) @ y[rows]), q


def test_host_and_device_inputs_agree_bitwise(partls):
    import torch
    f = FIXTURES["B"]
    X, y, P, a0, b0, fold_ptr = problem("B")
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()                   # (D, N) row-major = X column-major, ld N
    dy = torch.from_numpy(y.copy()).cuda()
    torch.cuda.synchronize()
    ctx = partls.Context(0)
    try:
        r = ctx.cv_alt(None, None, P, fold_ptr, np.asarray(f["etas"]), a0, b0, EPS, f["T"], device_ptrs=(dX.data_ptr(), dy.data_ptr(), f["N"], f["N"]))
    finally:
        ctx.close()
    _same(device("B"), r)


@pytest.mark.parametrize("name,best", [("C3", 1), ("A5", 2)])
def test_cross_validate_picks_the_oracles_eta(partls, name, best):
    f = FIXTURES[name]
    X, y, P, a0, b0, _ = problem(name)
    res = partls.cross_validate(partls.Alt, X, y, P, η=f["etas"], nfolds=f["F"], alpha0=a0, beta0=b0, ϵ=EPS, T=f["T"])
    print(name, "pooled held-out MSE", res.mse_mean)
    assert int(_oracle_mse(name).argmin()) == best and res.best_index_eta == best and res.best_eta == f["etas"][best]
    assert res.model is res.path[best] and res.best_index is None
    assert res.starts.opt.shape == (f["F"] + 1, len(f["etas"]), f["R"]) and res.best_start.shape == (f["F"] + 1, len(f["etas"]))
    d = device(name)
    assert np.array_equal(res.mse_mean, _pooled_mse(name, d["heldout_sse"]))
    if name == "C3":                                                            # K = 45 groups: what the feature is for
        with pytest.raises(partls.PartlsError) as ei:
            partls.fit(partls.Opt, X, y, P)
        assert ei.value.status == partls.lowlevel.ERR_UNSUPPORTED


def test_61_groups_fill_the_beta_system(partls, oracle):
    N, D, K, R = 150, 61, 61, 2
    X, y, P, a0, b0 = _data(29, N, D, K, R)
    fold_ptr, _ = partls.cv_folds(N, 2)
    etas = [0.5, 5.0]
    r = _cv_alt(partls, X, y, P, fold_ptr, etas, a0, b0, 100)
    _same(r, _cv_alt(partls, X, y, P, fold_ptr, etas, a0, b0, 100, PARTLS_CV_SERIAL=1))
    assert np.all(r["starts"]["status"] == 0) and np.all(r["status"] == 0)
    for q in range(6):
        fo, e = divmod(q, 2)
        tr = _train(N, fold_ptr, fo)
        best = min(oracle.fit_alt(np.asfortranarray(X[tr]), np.ascontiguousarray(y[tr]), P, a0[s], b0[s], etas[e], eps=EPS, T=100)["opt"]
                   for s in range(R))
        assert abs(r["opt"][q] - best) <= 1e-8 * max(1.0, best), q


def test_bad_arguments_write_nothing(partls):
    f = FIXTURES["B"]
    X, y, P, a0, b0, fold_ptr = problem("B")
    L = partls.lowlevel
    M, K, N, R = f["D"], f["K"], f["N"], f["R"]
    Xf = np.asfortranarray(X)
    Pf = np.asfortranarray(P)
    et = np.array(f["etas"])
    E, B = len(et), (f["F"] + 1) * len(et)
    ctx = partls.Context(0)
    try:
        def call(R=R, eps=EPS, lda0=M + 1, ldb0=K + 1, lda=M, ldb=K, fp=fold_ptr):
            fp = np.ascontiguousarray(fp, dtype=np.int64)
            nR = max(R, 1)
            dbl, i64, i32 = np.float64, np.int64, np.int32
            alpha, beta = np.full((M, B), 7.0, order="F"), np.full((K, B), 7.0, order="F")
            t, opt, sse, oa = np.full(B, 7.0), np.full(B, 7.0), np.full(B, 7.0), np.full((B, nR), 7.0)
            it, bs, ia = np.full(B, 7, dtype=i64), np.full(B, 7, dtype=i64), np.full((B, nR), 7, dtype=i64)
            stat, sa = np.full(B, 7, dtype=i32), np.full((B, nR), 7, dtype=i32)
            ptr = {dbl: L._dp, i64: L._ip, i32: C.POINTER(C.c_int32)}
            p = lambda a: a.ctypes.data_as(ptr[a.dtype.type])                      # noqa: E731
            st = L.lib().partls_cv_alt(ctx._h, Xf.ctypes.data, N, M, N, y.ctypes.data, None, 0, Pf.ctypes.data, K, M, p(fp), f["F"],
                                       p(et), E, 0, float(eps), f["T"], R, p(a0), lda0, p(b0), ldb0,
                                       p(alpha), lda, p(beta), ldb, p(t), p(opt), p(it), p(bs), p(sse), p(stat), p(oa), p(ia), p(sa))
            assert all(np.all(o == 7) for o in (alpha, beta, t, opt, it, bs, sse, stat, oa, ia, sa))
            return st
        assert call(R=0) == L.ERR_BAD_ARG
        assert call(eps=0.0) == L.ERR_BAD_ARG and call(eps=-1.0) == L.ERR_BAD_ARG
        assert call(lda0=M) == L.ERR_BAD_ARG and call(ldb0=K) == L.ERR_BAD_ARG
        assert call(lda=M - 1) == L.ERR_BAD_ARG and call(ldb=K - 1) == L.ERR_BAD_ARG
        unsorted = np.array(fold_ptr).copy()
        unsorted[1], unsorted[2] = unsorted[2], unsorted[1]
        assert call(fp=unsorted) == L.ERR_BAD_ARG
    finally:
        ctx.close()
