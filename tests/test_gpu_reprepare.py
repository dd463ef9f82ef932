"""One context, many problems in a row: after every step the context's result equals, byte for byte, that of a fresh context given only
that step's problem.  The steps change everything a prepared problem leaves behind (csrc/prepare.hip: forget_problem) — the route
(256-thread register kernel / deferred-update kernel), sample weights, the element type of X, the internal contexts of cv_opt and
opt_weightings — so a field the reset misses shows up as a fit that remembers its predecessor.  Every step asserts sweep_route(), so
that it cannot pass on another kernel than the one it names.
Also here: X with one NaN through the two batched entries (the single prepare's case is tests/test_gpu_opt.py::test_errors): status 3,
nothing written, and the context fits a clean problem afterwards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOLDS, ETAS = [0, 200, 400, 600], [0.0, 0.5]


@pytest.fixture(scope="module")
def problems(partls, oracle):
    L = partls.lowlevel
    XA, yA, PA, _ = oracle.synth(20260001, 600, 20, 4)
    XB, yB, PB, _ = oracle.synth(20260002, 600, 40, 6)
    rng = np.random.default_rng(20260003)
    w = rng.uniform(0.25, 4.0, 600)
    w[::37] = 0.0
    W = np.asfortranarray(np.stack([rng.multinomial(600, np.full(600, 1 / 600)).astype(np.float64), np.ones(600),
                                    (rng.random(600) < 0.7).astype(np.float64)], axis=1))
    A = (np.asfortranarray(XA), yA, PA)
    return {
        "A": dict(data=A, flags=0, route=L.ROUTE_REG_256),
        "weighted A": dict(data=A, flags=0, route=L.ROUTE_REG_256, weights=w),
        "B": dict(data=(np.asfortranarray(XB), yB, PB), flags=L.OPT_GENERIC_KERNEL, route=L.ROUTE_DEFERRED),
        "float32 A": dict(data=(np.asfortranarray(XA, dtype=np.float32), yA, PA), flags=0, route=L.ROUTE_REG_256),
        "cv A": dict(data=A, flags=0, route=L.ROUTE_REG_256, cv=True),
        "weightings A": dict(data=A, flags=0, route=L.ROUTE_REG_256, W=W),
    }


def _step(ctx, p):
    """the step's result as a tuple of byte strings"""
    X, y, P = p["data"]
    if p.get("cv"):
        r = ctx.cv_opt(X, y, P, FOLDS, ETAS, p["flags"])
        keys = ("opt", "best_index", "alpha", "beta", "t", "heldout_sse", "status")
    elif "W" in p:
        r = ctx.opt_weightings(X, y, P, p["W"], 0.0, p["flags"])
        keys = ("opt", "best_index", "alpha", "beta", "t", "oob_sse", "oob_rows", "status")
    else:
        ctx.opt_prepare(X, y, P, 0.0, p["flags"], weights=p.get("weights"))
        assert ctx.sweep_route()[0] == p["route"]
        _, bpat, _, unconv = ctx.opt_sweep()
        assert unconv == 0 and bpat >= 0
        a, b, t, opt, best = ctx.opt_finish(bpat)
        r = dict(opt=np.float64(opt), best_index=np.int64(best), alpha=a, beta=b, t=np.float64(t))
        keys = ("opt", "best_index", "alpha", "beta", "t")
    assert ctx.sweep_route()[0] == p["route"]
    return tuple(np.asarray(r[k]).tobytes() for k in keys)


@pytest.fixture(scope="module")
def fresh(partls, problems):
    """every step on a context of its own, once"""
    out = {}
    for name, p in problems.items():
        ctx = partls.Context(0)
        try:
            out[name] = _step(ctx, p)
        finally:
            ctx.close()
    return out


def test_a_reused_context_fits_like_a_fresh_one(partls, problems, fresh):
    assert fresh["A"] != fresh["weighted A"] and fresh["A"] != fresh["B"]          # the steps differ, so a remembered one would show
    ctx = partls.Context(0)
    try:
        for name in ("A", "weighted A", "B", "float32 A", "cv A", "B", "weightings A", "A", "B", "A"):
            assert _step(ctx, problems[name]) == fresh[name], name
    finally:
        ctx.close()


@pytest.mark.parametrize("entry", ["cv_opt", "opt_weightings"])
def test_nan_in_x_through_the_batched_entries(partls, oracle, entry):
    L = partls.lowlevel
    X, y, P, _ = oracle.synth(20260004, 60, 6, 2)
    X = np.asfortranarray(X)
    Xn = X.copy()
    Xn[17, 3] = np.nan

    def fit(c):
        c.opt_prepare(X, y, P)
        _, bpat, _, unconv = c.opt_sweep()
        assert unconv == 0
        return tuple(np.asarray(v).tobytes() for v in c.opt_finish(bpat))

    ref = partls.Context(0)
    ctx = partls.Context(0)
    try:
        want = fit(ref)
        with pytest.raises(partls.PartlsError) as e:
            if entry == "cv_opt":
                ctx.cv_opt(Xn, y, P, [0, 20, 40, 60], ETAS)
            else:
                ctx.opt_weightings(Xn, y, P, np.ones((60, 2)))
        assert e.value.status == L.ERR_NONFINITE == 3
        assert fit(ctx) == want
    finally:
        ref.close()
        ctx.close()
