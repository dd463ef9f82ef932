"""Context lifecycle: create -> opt_prepare -> opt_sweep -> opt_finish -> destroy, ten times over, gives bitwise the same fit every
round — on the 256-thread register route (which exports best_sol), on the global-memory route with its per-workgroup scratch, and
with contexts that ran cv_opt (internal contexts, cv* buffers) or alt_multistart (ams* buffers) before they were destroyed.  Every
device and page-locked buffer of a context is released by its own destructor (csrc/ctx.h); no memory-size assertion: the free-memory
counter of a shared device moves with other work."""
import numpy as np
import pytest

ROUNDS = 10


def _problem(oracle, seed, N, D, K):
    X, y, P, _ = oracle.synth(seed, N, D, K)
    return np.asfortranarray(X), y, P


def _round(partls, X, y, P, flags, route, extra=None):
    ctx = partls.Context(0)
    try:
        ctx.opt_prepare(X, y, P, 0.0, flags)
        assert ctx.sweep_route()[0] == route
        _, bpat, _, unconv = ctx.opt_sweep()
        assert unconv == 0 and bpat >= 0
        a, b, t, opt, best = ctx.opt_finish(bpat)
        if extra is not None:
            extra(ctx)
    finally:
        ctx.close()
    return opt, best, a, b


def _same(r0, r):
    assert np.float64(r0[0]).tobytes() == np.float64(r[0]).tobytes()
    assert r0[1] == r[1]
    assert r0[2].tobytes() == r[2].tobytes() and r0[3].tobytes() == r[3].tobytes()


@pytest.mark.gpu
def test_lifecycle_register_route(partls, oracle):
    L = partls.lowlevel
    X, y, P = _problem(oracle, 20260001, 600, 20, 4)             # the smoke problem
    first = _round(partls, X, y, P, 0, L.ROUTE_REG_256)
    for _ in range(ROUNDS - 1):
        _same(first, _round(partls, X, y, P, 0, L.ROUTE_REG_256))


@pytest.mark.gpu
def test_lifecycle_global_memory_route(partls, oracle):
    L = partls.lowlevel
    X, y, P = _problem(oracle, 20260002, 600, 40, 6)
    first = _round(partls, X, y, P, L.OPT_GENERIC_KERNEL, L.ROUTE_DEFERRED)
    for _ in range(ROUNDS - 1):
        _same(first, _round(partls, X, y, P, L.OPT_GENERIC_KERNEL, L.ROUTE_DEFERRED))


@pytest.mark.gpu
def test_lifecycle_after_cv_and_multistart(partls, oracle):
    L = partls.lowlevel
    X, y, P = _problem(oracle, 20260001, 600, 20, 4)
    M, K = P.shape
    flags = L.OPT_FAITHFUL_INTERCEPT                             # alt_multistart needs the intercept in the tableau

    def run_cv(ctx):                                             # 3 folds x 2 eta + the two full-data problems
        ctx.cv_opt(X, y, P, [0, 200, 400, 600], [0.0, 0.5], flags)

    def run_multistart(ctx):                                     # 4 starts on the problem the round prepared
        rng = np.random.default_rng(7)
        a0 = rng.uniform(0.1, 1.0, (4, M + 1))
        b0 = rng.uniform(-1.0, 1.0, (4, K + 1))
        ctx.alt_multistart(a0, b0, eps=1e-6, T=20)

    extras = {0: run_multistart, 1: run_cv}                      # once each; cv_opt prepares the context anew, so it goes last in its round
    first = _round(partls, X, y, P, flags, L.ROUTE_REG_256, extras[0])
    for i in range(1, ROUNDS):
        _same(first, _round(partls, X, y, P, flags, L.ROUTE_REG_256, extras.get(i)))
