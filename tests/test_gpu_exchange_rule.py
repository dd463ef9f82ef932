"""The backup exchange rule and the pivot cap in every sweep kernel, against tests/exchange_reference.py.

csrc/sweep_rules.h defines ExchangeRule once; only sweep_generic.hip is built from it, and sweep_blk.hip (plain and merged-scan
instantiations), sweep_lazy.hip and sweep_coop.hip hold hand-written copies.  Here every copy walks designs on which block principal
pivoting stalls (a third to two thirds of the patterns take backup steps) and is compared with the float64 emulation of the rule,
DECISION FOR DECISION: the pivot counter equals the emulation's total, and under PARTLS_MAX_ROUNDS = 1, 2, 3, 4, 6, 10, 40 the set of
capped patterns — which fixes every pattern's round count — is the emulation's, read per pattern from the NaN rows of the export.
tests/test_exchange_reference.py asserts, without a GPU, what makes that comparison sound: no pivot near piv_eps, every tested value at
least 1000 x the float64 / long-double drift and 1000 x tol away from its tolerance, and every plausible miscopy of the rule (patience
2 or 4, <= improvement, smallest-index backup, >= at the cap) changing the pivot count or the capped set of every case — for every
walk of this file (chains of 7 and 64, the whole range and the sub-range, every cap); the emulation here asserts the cheap ones again.

Chain mode (PARTLS_PAIR=0, PARTLS_BIT_ORDER=identity, PARTLS_CHAIN_LEN 7 and 64; the whole range and the Gray indices 5..26):
  256-thread register  c40, c72-eta, c40-free (free intercept: no all_opt and no export, so counters and the winner only), c72-overlap
  512-thread register  c176
  deferred-update      c40 with PARTLS_OPT_GENERIC_KERNEL; c297 (n = 297, Gray indices 17..24 only)
  eager generic        c40 with PARTLS_OPT_GENERIC_KERNEL and PARTLS_EAGER_GENERIC=1
Node mode (bnb_bound, one node per call from the fresh tableau): n40, n72 (256-thread), n176 (512-thread), n40 through the flag, n297
and n331 (deferred-update), n40 eager generic (the node twice in one call: a single node of a global-memory context goes to the
cooperative kernel), n331 on the cooperative kernel (PARTLS_EAGER_GENERIC=1, batches of one, blocks() > 0).
Every route's pivots() counts exchanges one by one and is compared exactly.

The default walk (pair walk, bit order and chain length as the library chooses) visits in another order, so only outcomes are
compared; fit(Opt) runs in a child process, because the default context reads its knobs once.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import exchange_reference as E
from bnb_reference import NodeReference, U
from test_exchange_reference import oracle_objectives
from test_gpu_bnb_nodes import C_TWO, C_UP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAITHFUL, GENERIC = 1, 2                                    # PARTLS_OPT_FAITHFUL_INTERCEPT, PARTLS_OPT_GENERIC_KERNEL (include/partls.h)
REG_256, REG_512, DEFERRED, EAGER = 1, 2, 3, 4              # partls_route (include/partls.h)
ERR_NOT_CONVERGED = 6
TOL_OBJ = 1e-9                                              # tests/test_gpu_opt.py
KNOBS = ("PARTLS_PAIR", "PARTLS_BIT_ORDER", "PARTLS_CHAIN_LEN", "PARTLS_MAX_ROUNDS", "PARTLS_EAGER_GENERIC", "PARTLS_REG_MAXT",
         "PARTLS_GRID", "PARTLS_NO_EXPORT", "PARTLS_NO_COOP", "PARTLS_COOP_ROWS")
EAGER_ENV = {"PARTLS_EAGER_GENERIC": "1"}
# route: (case, environment, flags, sweep_route())
CHAIN_ROUTES = {
    "reg256-c40": ("c40", {}, 0, (REG_256, 3)),
    "reg256-c72-eta": ("c72-eta", {}, 0, (REG_256, 5)),
    "reg512-c176": ("c176", {}, 0, (REG_512, 11)),
    "reg256-c40-free": ("c40-free", {}, 0, (REG_256, 3)),
    "reg256-c72-overlap": ("c72-overlap", {}, 0, (REG_256, 5)),
    "deferred-c40": ("c40", {}, GENERIC, (DEFERRED, 0)),
    "eager-c40": ("c40", EAGER_ENV, GENERIC, (EAGER, 0)),
    "deferred-c297": ("c297", {}, 0, (DEFERRED, 0)),
}
# route: (case, environment, flags, sweep_route(), copies of the node per call, cooperative kernel)
NODE_ROUTES = {
    "reg256-n40": ("n40", {}, 0, (REG_256, 3), 1, False),
    "reg256-n72": ("n72", {}, 0, (REG_256, 5), 1, False),
    "reg512-n176": ("n176", {}, 0, (REG_512, 11), 1, False),
    "deferred-n40": ("n40", {}, GENERIC, (DEFERRED, 0), 1, False),
    "deferred-n297": ("n297", {}, 0, (DEFERRED, 0), 1, False),
    "deferred-n331": ("n331", {}, 0, (DEFERRED, 0), 1, False),
    "eager-n40": ("n40", EAGER_ENV, GENERIC, (EAGER, 0), 2, False),
    "coop-n331": ("n331", EAGER_ENV, 0, (EAGER, 0), 1, True),
}
_CASES, _WALKS, _NODES = {}, {}, {}


def context(partls, monkeypatch, env):
    """a Context with the given knobs (read once, at partls_create)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = partls.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


def chain(oracle, name):
    """the case, its prepared reference problem and the oracle's optimum of every pattern (by pattern index): once per case"""
    if name not in _CASES:
        c = E.chain_case(name)
        pr = E.prepare(c["X"], c["y"], c["P"], c["eta"], c["faithful"])
        npat = 1 << pr["kbits"]
        _CASES[name] = dict(case=c, pr=pr, npat=npat, objs=oracle_objectives(oracle, c, np.arange(npat)))
    return _CASES[name]


def emulate(name, pr, g0, g1, chain_len, cap):
    """the float64 emulation of one walk, with the conditions it needs on itself: no rejection, every decision far from the tolerance"""
    key = (name, g0, g1, chain_len, cap)
    if key not in _WALKS:
        r = E.walk(pr, g0, g1, chain_len, cap)
        assert r["rejected"] == 0 and r["min_d"] >= 1e-6 and r["margin"] >= 1000.0 * r["tol"], (key, r["rejected"], r["min_d"], r["margin"])
        _WALKS[key] = r
    return _WALKS[key]


@pytest.mark.parametrize("cap", (None,) + E.CAPS)
@pytest.mark.parametrize("route", list(CHAIN_ROUTES))
def test_chain_walk_decision_for_decision(partls, oracle, monkeypatch, route, cap):
    name, env, flags, kernel = CHAIN_ROUTES[route]
    ref = chain(oracle, name)
    c, pr, objs = ref["case"], ref["pr"], ref["objs"]
    faithful = c["faithful"]
    ranges = [E.RANGE_297] if name == E.RANGE_CASE[0] else [(0, ref["npat"]), E.SUB_RANGE]
    for chain_len in E.GPU_CHAIN_LENS:
        knobs = dict(env, PARTLS_PAIR="0", PARTLS_BIT_ORDER="identity", PARTLS_CHAIN_LEN=str(chain_len))
        if cap is not None:
            knobs["PARTLS_MAX_ROUNDS"] = str(cap)
        ctx = context(partls, monkeypatch, knobs)
        try:
            ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], c["flags"] | flags)
            assert ctx.sweep_route() == kernel, "%s runs on %s" % (route, ctx.sweep_route())
            assert ctx.bit_order()[0].tolist() == list(range(pr["kbits"]))
            for g0, g1 in ranges:
                emu = emulate(name, pr, g0, g1, chain_len, cap)
                tag = "%s cap %s chain %d [%d, %d)" % (route, cap, chain_len, g0, g1)
                bo, bp, allo, unconv = ctx.opt_sweep(g0, g1, want_all=faithful)
                piv, vet = ctx.pivots(), ctx.vetoes()
                capped, conv = emu["capped"], ~emu["capped"]
                print("[exchange] %s: %d pivots (emulation %d), %d capped (emulation %d), %d backup steps in the emulation, %d vetoes" % (
                    tag, piv, emu["pivots"].sum(), unconv, capped.sum(), emu["backups"].sum(), vet))
                assert piv == int(emu["pivots"].sum()), "%s: %d pivots, the rule takes %d" % (tag, piv, emu["pivots"].sum())
                assert vet == 0, tag
                assert unconv == int(capped.sum()), "%s: %d patterns capped, the rule caps %d" % (tag, unconv, capped.sum())
                want = objs[emu["pattern"]]
                if faithful:
                    got = allo[emu["pattern"]]
                    assert not np.isnan(got).any() and np.isnan(allo).sum() == len(allo) - (g1 - g0), tag
                    err = np.abs(got - want)[conv] / np.maximum(1.0, want[conv]) if conv.any() else np.zeros(1)
                    assert np.all(np.abs(got - want)[conv] <= TOL_OBJ * np.maximum(1.0, want[conv])), "%s: all_opt off by %.3g" % (tag, err.max())
                if not capped.any():
                    win = int(emu["pattern"][np.lexsort((emu["pattern"], emu["obj"]))[0]])
                    assert bp == win, "%s: winner %d, the emulation's %d" % (tag, bp, win)
                    assert abs(bo - objs[win]) <= TOL_OBJ * max(1.0, objs[win]), tag
                if not faithful:
                    continue                                            # the export needs the faithful intercept
                m = ctx.opt_models(g0, g1, raw=True)
                assert m["pattern"].tolist() == emu["pattern"].tolist(), tag
                nan_opt = np.isnan(m["opt"])
                assert nan_opt.tolist() == capped.tolist(), "%s: NaN opt at Gray indices %s, the rule caps %s" % (
                    tag, (g0 + np.flatnonzero(nan_opt)).tolist(), (g0 + np.flatnonzero(capped)).tolist())
                for field in ("raw_alpha", "alpha", "beta"):
                    assert np.array_equal(np.isnan(m[field]).all(axis=1), capped) and np.array_equal(np.isnan(m[field]).any(axis=1), capped), (tag, field)
                assert np.array_equal(np.isnan(m["t"]), capped), tag
                assert m["n_unconverged"] == int(capped.sum()) and m["n_vetoes"] == 0, tag
                assert np.all(np.abs(m["opt"] - want)[conv] <= TOL_OBJ * np.maximum(1.0, want[conv])), tag
                top = ctx.opt_top(g1 - g0, g0, g1)
                assert top["n_unconverged"] == int(capped.sum()) and top["count"] == int(conv.sum()), tag
                assert set(top["pattern"].tolist()) == set(emu["pattern"][conv].tolist()), "%s: opt_top lists a capped pattern" % tag
        finally:
            ctx.close()


def node(name):
    """the node case, the exact reference of its node and of the root, and the emulation of both: once per case"""
    if name not in _NODES:
        c = E.node_case(name)
        ref = NodeReference(c["X"], c["y"], c["P"], c["eta"])
        root = (0, (1 << (c["K"] + 1)) - 1)
        exact = ref.nodes([c["pat"], root[0]], [c["free"], root[1]])
        assert exact["certified"].all()
        pr = E.prepare(c["X"], c["y"], c["P"], c["eta"])
        emu = E.solve(pr, np.array([E.tableau_codes(pr, exact["codes"][i]) for i in range(2)]))
        assert emu["rejected"] == 0 and emu["min_d"] >= 1e-6 and emu["margin"] >= 1000.0 * emu["tol"] and not emu["capped"].any()
        _NODES[name] = dict(case=c, ref=ref, exact=exact, emu=emu, root=root)
    return _NODES[name]


def bound_ok(tag, ref, lb, lb_ref):
    e2 = float((np.longdouble(lb) ** 2 - np.longdouble(lb_ref) ** 2) / (U * ref.yy))
    print("[exchange] %s: lb^2 - lb_ref^2 = %.3g u y'y" % (tag, e2))
    assert abs(e2) <= C_TWO and e2 <= C_UP, "%s: lb %.17g, reference %.17g (%.3g u y'y)" % (tag, lb, lb_ref, e2)


@pytest.mark.parametrize("route", list(NODE_ROUTES))
def test_node_solve_decision_for_decision(partls, monkeypatch, route):
    name, env, flags, kernel, copies, coop = NODE_ROUTES[route]
    nd = node(name)
    c, ref, exact, emu = nd["case"], nd["ref"], nd["exact"], nd["emu"]
    rounds, pivots = int(emu["rounds"][0]), int(emu["pivots"][0])
    assert emu["backups"][0] >= 1 and emu["rounds"][1] < rounds - 1, "the root is not the easy node"
    pats, frees = np.array([c["pat"]] * copies, np.uint64), np.array([c["free"]] * copies, np.uint64)
    rp, rf = np.array([nd["root"][0]], np.uint64), np.array([nd["root"][1]], np.uint64)
    # the default cap; a cap of exactly the node's round count (still met); one round less (ERR_NOT_CONVERGED)
    for cap in (None, rounds, rounds - 1):
        ctx = context(partls, monkeypatch, dict(env, **({} if cap is None else {"PARTLS_MAX_ROUNDS": str(cap)})))
        try:
            ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], FAITHFUL | flags)
            assert ctx.sweep_route() == kernel, "%s runs on %s" % (route, ctx.sweep_route())
            tag = "%s cap %s" % (route, cap)
            if cap == rounds - 1:
                with pytest.raises(partls.PartlsError) as err:
                    ctx.bnb_bound(pats, frees)
                assert err.value.status == ERR_NOT_CONVERGED, tag
                print("[exchange] %s: ERR_NOT_CONVERGED (the node takes %d rounds)" % (tag, rounds))
            else:
                lb, _ = ctx.bnb_bound(pats, frees)
                piv = ctx.pivots()
                print("[exchange] %s: %d pivots (emulation %d x %d), %d rounds and %d backup steps in the emulation" % (
                    tag, piv, copies, pivots, rounds, emu["backups"][0]))
                if coop:
                    assert ctx.blocks() > 0, "%s: not solved by the cooperative kernel" % tag
                assert piv == copies * pivots, "%s: %d pivots, the rule takes %d" % (tag, piv, copies * pivots)
                for v in lb:
                    bound_ok(tag, ref, v, exact["lb"][0])
            # the same context then bounds an easy node (the root: every variable free)
            lb, _ = ctx.bnb_bound(rp, rf)
            if coop:
                assert ctx.blocks() > 0, "%s: the root was not solved by the cooperative kernel" % tag
            assert ctx.pivots() == int(emu["pivots"][1]), "%s: root %d pivots, the rule takes %d" % (tag, ctx.pivots(), emu["pivots"][1])
            bound_ok(tag + " root", ref, lb[0], exact["lb"][1])
        finally:
            ctx.close()


@pytest.mark.parametrize("name", list(E.CHAIN_CASES))
def test_default_walk_outcomes(partls, oracle, monkeypatch, name):
    """pair walk, bit order and chain length as the library chooses: other trajectories, the same outcomes"""
    ref = chain(oracle, name)
    c, objs = ref["case"], ref["objs"]
    win = int(np.argmin(objs))
    ctx = context(partls, monkeypatch, {})
    try:
        ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], c["flags"])
        bo, bp, allo, unconv = ctx.opt_sweep(0, -1, want_all=c["faithful"])
        print("[exchange] default walk %s: %d pivots, %d capped, winner %d (oracle %d)" % (name, ctx.pivots(), unconv, bp, win))
        assert unconv == 0 and ctx.vetoes() == 0
        if c["faithful"]:
            assert np.all(np.abs(allo - objs) <= TOL_OBJ * np.maximum(1.0, objs)), "max error %.3g" % np.abs(allo - objs).max()
        assert bp == win and abs(bo - objs[win]) <= TOL_OBJ * max(1.0, objs[win])
    finally:
        ctx.close()
    ctx = context(partls, monkeypatch, {"PARTLS_MAX_ROUNDS": "6"})
    try:
        ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], c["flags"])
        unconv = ctx.opt_sweep(0, -1)[3]
        print("[exchange] default walk %s under a cap of 6: %d capped, %d pivots" % (name, unconv, ctx.pivots()))
        assert unconv > 0
        if c["faithful"]:
            m = ctx.opt_models(raw=True)
            nan = np.isnan(m["opt"])
            assert m["n_unconverged"] == unconv == int(nan.sum())
            assert np.array_equal(np.isnan(m["raw_alpha"]).all(axis=1), nan) and np.array_equal(np.isnan(m["raw_alpha"]).any(axis=1), nan)
            want = objs[m["pattern"]]
            assert np.all(np.abs(m["opt"] - want)[~nan] <= TOL_OBJ * np.maximum(1.0, want[~nan]))
            top = ctx.opt_top(len(nan))
            assert top["n_unconverged"] == unconv and set(top["pattern"].tolist()) == set(m["pattern"][~nan].tolist())
    finally:
        ctx.close()


FIT_CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import partls_amd, exchange_reference as E
pkg = partls_amd.package()
c = E.chain_case("c40")
try:
    model, _, rep = pkg.fit(pkg.Opt, c["X"], c["y"], c["P"], eta=c["eta"], faithful_intercept=True)
    print("RESULT " + json.dumps(dict(status=0, opt=rep.opt, best_index=int(rep.best_index), alpha=model.alpha.tolist(), beta=model.beta.tolist(), t=float(model.t))))
except pkg.PartlsError as e:
    print("RESULT " + json.dumps(dict(status=int(e.status))))
"""


def fit_in_child(env):
    full = {k: v for k, v in os.environ.items() if k not in KNOBS}
    full.update(env)
    run = subprocess.run([sys.executable, "-c", FIT_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=full, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
    assert run.returncode == 0 and len(lines) == 1, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    return json.loads(lines[0][7:])


def test_fit_reports_the_cap(oracle):
    """fit(Opt) on c40: status 6 under PARTLS_MAX_ROUNDS=6 (the default context reads its knobs once: a fresh process each), the oracle's
    model without the knob"""
    c = E.chain_case("c40")
    assert fit_in_child({"PARTLS_MAX_ROUNDS": "6"}) == {"status": ERR_NOT_CONVERGED}
    got = fit_in_child({})
    ref = oracle.fit_opt(c["X"], c["y"], c["P"], eta=c["eta"])
    assert got["status"] == 0 and got["best_index"] == ref["best_index"]
    assert abs(got["opt"] - ref["opt"]) <= TOL_OBJ * max(1.0, ref["opt"])
    np.testing.assert_allclose(got["alpha"], ref["alpha"], atol=1e-7)     # TOL_MODEL of tests/test_gpu_opt.py
    np.testing.assert_allclose(got["beta"], ref["beta"], atol=1e-7)
    assert abs(got["t"] - ref["t"]) <= 1e-7


def test_design_correlated_throughout(partls, oracle, monkeypatch):
    """n = 176, every column from Z (N x n/2) @ W + 0.1 E: the emulation predicts that 52-57 of the 64 patterns reach the default cap of
    3540 rounds (about 4e5 pivots), at a distance of only ~1e-8 from the tolerance, so nothing is compared decision for decision.
    Whatever the count turns out to be: n_unconverged is the number of NaN rows, every other row has the oracle's optimum, and fit
    raises status 6 exactly when the count is not 0.  (DESIGN.md §7 records the observation.)"""
    D, K = 175, 5
    rng = np.random.default_rng(20261176)
    N = 3 * D
    X = rng.standard_normal((N, (D + 1) // 2)) @ rng.standard_normal(((D + 1) // 2, D)) + 0.1 * rng.standard_normal((N, D))
    grp = rng.integers(0, K, D)
    grp[rng.choice(D, K, replace=False)] = np.arange(K)
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    y = X @ (rng.standard_normal(D) * (rng.random(D) < 0.6)) + 0.4 + rng.standard_normal(N)
    X, P = np.asfortranarray(X), np.asfortranarray(P)
    objs = oracle.fit_opt(X, y, P, return_all=True)["all_opt"]
    ctx = context(partls, monkeypatch, {})
    try:
        ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
        assert ctx.sweep_route() == (REG_512, 11)
        t0 = time.perf_counter()
        unconv = ctx.opt_sweep(0, -1)[3]
        dt = time.perf_counter() - t0
        piv = ctx.pivots()
        m = ctx.opt_models(raw=True)
    finally:
        ctx.close()
    nan = np.isnan(m["opt"])
    want = objs[m["pattern"]]
    err = np.abs(m["opt"] - want)[~nan] / np.maximum(1.0, want[~nan]) if (~nan).any() else np.zeros(1)
    print("[exchange] correlated throughout, n = 176: %d of 64 patterns capped at %d rounds, %d pivots, sweep %.1f ms, max error of the others %.3g" % (
        unconv, E.default_max_rounds(176), piv, 1e3 * dt, err.max()))
    assert m["n_unconverged"] == int(nan.sum()) == unconv
    assert np.array_equal(np.isnan(m["raw_alpha"]).all(axis=1), nan) and np.array_equal(np.isnan(m["raw_alpha"]).any(axis=1), nan)
    assert np.all(np.abs(m["opt"] - want)[~nan] <= TOL_OBJ * np.maximum(1.0, want[~nan])), "max error %.3g" % err.max()
    raised = None
    try:
        partls.fit(partls.Opt, X, y, P, faithful_intercept=True)
    except partls.PartlsError as e:
        raised = e.status
    assert raised == (ERR_NOT_CONVERGED if unconv else None), (raised, unconv)
