"""PARTLS_OPT_RESCUE_CAPPED on the GPU: patterns that hit the pivot cap are solved again by the rescue kernel (csrc/rescue.hip; the
rule is tests/rescue_reference.py's, checked on the CPU by tests/test_rescue_reference.py).

PARTLS_MAX_ROUNDS = 1 and 10 force the cap at small size, as in tests/test_gpu_exchange_rule.py, whose contexts, cases and routes
these tests share (PARTLS_PAIR=0, PARTLS_BIT_ORDER=identity, PARTLS_CHAIN_LEN=7):
  256-thread register  c40, c72-eta, c40-free (free intercept: no export, so winner and counters only), c72-overlap
  512-thread register  c176
  deferred-update      c40 with PARTLS_OPT_GENERIC_KERNEL; c297 (Gray indices 17..24 only)
  eager generic        c40 with PARTLS_OPT_GENERIC_KERNEL and PARTLS_EAGER_GENERIC=1
Every test first shows, on a context WITHOUT the flag and with the same knobs, that patterns cap (all of them need more than one
round; at cap 10 some but not all) and which: the NaN rows of its export.  With the flag nothing is left unconverged, every
objective is the oracle's within TOL_OBJ, the rescued rows are the models of an uncapped context, opt_top is a host sort of
opt_models bit for bit, and opt_finish / opt_pattern succeed where the plain context reports status 6.
The design that is correlated throughout is fitted at the default cap in a child process.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import exchange_reference as E
import rescue_reference as R
from test_exchange_reference import oracle_objectives
from test_gpu_exchange_rule import CHAIN_ROUTES, ERR_NOT_CONVERGED, FAITHFUL, KNOBS, ROOT, TOL_OBJ, chain, context

pytestmark = pytest.mark.gpu

RESCUE = 4                                                  # PARTLS_OPT_RESCUE_CAPPED (include/partls.h)
ERR_UNSUPPORTED = 7
TOL_MODEL = 1e-7                                            # tests/test_gpu_opt.py
WALK = dict(PARTLS_PAIR="0", PARTLS_BIT_ORDER="identity", PARTLS_CHAIN_LEN=str(E.CHAIN_LEN))
ALL_KNOBS = KNOBS + ("PARTLS_RESCUE_MAX_PASSES",)
KEYS = ("pattern", "opt", "alpha", "beta", "t", "raw_alpha")
_UNCAPPED = {}


def ctx_with(partls, monkeypatch, env):
    monkeypatch.delenv("PARTLS_RESCUE_MAX_PASSES", raising=False)
    return context(partls, monkeypatch, env)


def gray_range(name, npat):
    return E.RANGE_297 if name == E.RANGE_CASE[0] else (0, npat)


def uncapped(partls, monkeypatch, name, c, pats):
    """opt_pattern (faithful cases) and opt_finish of the listed patterns on a context with the default cap: once per case"""
    if name not in _UNCAPPED:
        ctx = ctx_with(partls, monkeypatch, {})
        try:
            ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], c["flags"])
            _UNCAPPED[name] = dict(pattern={int(b): ctx.opt_pattern(int(b)) for b in pats} if c["faithful"] else {},
                                   finish={int(b): ctx.opt_finish(int(b)) for b in (int(pats[0]), int(pats[-1]))})
        finally:
            ctx.close()
    return _UNCAPPED[name]


def close_obj(got, want):
    return np.abs(got - want) <= TOL_OBJ * np.maximum(1.0, want)


def same_as_host_sort(top, full, k):
    ok = np.flatnonzero(~np.isnan(full["opt"]))
    rows = ok[np.lexsort((full["pattern"][ok], full["opt"][ok] + 0.0))][:k]
    assert top["count"] == len(rows) == len(top["pattern"])
    for key in KEYS:
        assert np.array_equal(top[key], full[key][rows]), key


@pytest.mark.parametrize("cap", (1, 10))
@pytest.mark.parametrize("route", list(CHAIN_ROUTES))
def test_capped_patterns_are_rescued(partls, oracle, monkeypatch, route, cap):
    name, env, flags, kernel = CHAIN_ROUTES[route]
    ref = chain(oracle, name)
    c, pr, objs = ref["case"], ref["pr"], ref["objs"]
    faithful, n = c["faithful"], pr["n"]
    g0, g1 = gray_range(name, ref["npat"])
    total = g1 - g0
    gs = np.arange(g0, g1)
    pats = gs ^ (gs >> 1)
    want = objs[pats]
    knobs = dict(env, PARTLS_MAX_ROUNDS=str(cap), **WALK)
    tag = "%s cap %d" % (route, cap)

    # ---- the precondition: without the flag, patterns cap, and the export says which
    plain = ctx_with(partls, monkeypatch, knobs)
    try:
        plain.opt_prepare(c["X"], c["y"], c["P"], c["eta"], c["flags"] | flags)
        assert plain.sweep_route() == kernel, tag
        _, bp0, _, unconv0 = plain.opt_sweep(g0, g1, want_all=faithful)
        assert (0 < unconv0) if cap == 1 else (0 < unconv0 < total), "%s: %d of %d capped without the flag" % (tag, unconv0, total)
        st = plain.rescue_stats()
        assert (st.rescued, st.pivots, st.failed) == (0, 0, 0), tag
        if faithful:
            m0 = plain.opt_models(g0, g1, raw=True)
            nan0 = np.isnan(m0["opt"])
            assert m0["n_unconverged"] == int(nan0.sum()) == unconv0, tag
            assert np.array_equal(np.isnan(m0["raw_alpha"]).all(axis=1), nan0), tag
            assert plain.rescue_stats().rescued == 0, tag
        if cap == 1:                                           # (every single solve of these cases takes 4 rounds or more)
            with pytest.raises(partls.PartlsError) as err:
                plain.opt_finish(int(pats[0] if bp0 != pats[0] else pats[-1]))   # (not the sweep's winner, whose solution it left behind)
            assert err.value.status == ERR_NOT_CONVERGED, tag
        ncapped = int(nan0.sum()) if faithful else unconv0
    finally:
        plain.close()

    unc = uncapped(partls, monkeypatch, name, c, pats)
    ctx = ctx_with(partls, monkeypatch, knobs)
    try:
        ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], c["flags"] | flags | RESCUE)
        assert ctx.sweep_route() == kernel, tag
        # ---- opt_sweep: the second pass is authoritative
        t0 = time.perf_counter()
        bo, bp, allo, unconv = ctx.opt_sweep(g0, g1, want_all=faithful)
        dt = time.perf_counter() - t0
        st = ctx.rescue_stats()
        print("[rescue] %s: %d of %d capped, rescued %d with %d pivots (%.1f per pattern; rescue kernel %.3f ms, sweep call %.1f ms), failed %d" % (
            tag, ncapped, total, st.rescued, st.pivots, st.pivots / max(1, st.rescued), ctx.timing(partls.lowlevel.T_RESCUE), 1e3 * dt, st.failed))
        assert unconv == 0 and st.failed == 0, tag
        assert st.rescued == ncapped, "%s: %d rescued, the export of the plain context has %d NaN rows" % (tag, st.rescued, ncapped)
        assert st.pivots >= st.rescued and st.pivots <= st.rescued * 4 * n, tag
        if faithful:
            emu = R.solve(pr, pats[nan0])                       # the rule, pivot for pivot (tests/rescue_reference.py)
            assert emu["solved"].all() and st.pivots == int(emu["pivots"].sum()), "%s: %d pivots, the rule takes %d" % (tag, st.pivots, emu["pivots"].sum())
            got = allo[pats]
            assert not np.isnan(got).any() and np.isnan(allo).sum() == len(allo) - total, tag
            assert close_obj(got, want).all(), "%s: all_opt off by %.3g" % (tag, (np.abs(got - want) / np.maximum(1.0, want)).max())
        order = np.lexsort((pats, want))
        win = int(pats[order[0]])
        if total < 2 or want[order[1]] - want[order[0]] > TOL_OBJ * max(1.0, want[order[0]]):
            assert bp == win, "%s: winner %d, the oracle's %d" % (tag, bp, win)
        assert close_obj(bo, objs[bp]), tag
        co, cp = ctx.opt_candidates()
        assert len(cp) >= 1 and cp[0] == bp and co[0] == bo, tag
        # ---- opt_finish on the sweep's winner, and on a pattern of its own: solved where the plain context reports the cap
        a, b, t, o, bi = ctx.opt_finish(bp)
        assert close_obj(o, objs[bp]), tag
        for pat, (ua, ub, ut, uo, ubi) in unc["finish"].items():
            before = ctx.rescue_stats().rescued
            a, b, t, o, bi = ctx.opt_finish(pat)
            if cap == 1:
                assert ctx.rescue_stats().rescued > before, "%s: opt_finish(%d) did not cap" % (tag, pat)
            assert bi == ubi and close_obj(o, uo), tag
            np.testing.assert_allclose(a, ua, atol=TOL_MODEL, err_msg=tag)
            np.testing.assert_allclose(b, ub, atol=TOL_MODEL, err_msg=tag)
            assert abs(t - ut) <= TOL_MODEL, tag
        if not faithful:
            return                                             # the export needs the faithful intercept
        # ---- opt_models: no NaN row; the rescued rows are the models of an uncapped context
        m = ctx.opt_models(g0, g1, raw=True)
        st = ctx.rescue_stats()
        assert m["pattern"].tolist() == pats.tolist(), tag
        assert m["n_unconverged"] == 0 and st.failed == 0 and st.rescued == ncapped, tag
        for key in KEYS:
            assert not np.isnan(m[key]).any(), (tag, key)
        assert close_obj(m["opt"], want).all(), tag
        assert np.array_equal(m["opt"], allo[pats]), "%s: the second pass's all_opt is not its export's objective" % tag
        for i in np.flatnonzero(nan0):
            ra, ro = unc["pattern"][int(pats[i])]
            mine = m["raw_alpha"][i]
            f = E.signs(pr, int(pats[i]))[np.argsort(pr["perm"])]
            assert np.all(mine >= 0) and np.all(mine[f == 0] == 0), "%s: row %d is not sign-feasible" % (tag, i)
            tol = 1e-8 * max(1.0, np.abs(ra).max())             # tests/test_gpu_models.py
            np.testing.assert_allclose(mine, ra, rtol=1e-8, atol=tol, err_msg="%s row %d" % (tag, i))
            np.testing.assert_allclose(m["opt"][i], ro, rtol=1e-8, err_msg="%s row %d" % (tag, i))
        # ---- opt_top: a host sort of opt_models, bit for bit
        for k in (min(8, total), total):
            top = ctx.opt_top(k, g0, g1, raw=True)
            assert top["n_unconverged"] == 0 and top["count"] == k, (tag, k)
            assert ctx.rescue_stats().rescued == ncapped, (tag, k)
            same_as_host_sort(top, m, k)
        # ---- opt_pattern
        for pat in (int(pats[0]), int(pats[-1])):
            ra, ro = ctx.opt_pattern(pat)
            ua, uo = unc["pattern"][pat]
            np.testing.assert_allclose(ra, ua, rtol=1e-8, atol=1e-8 * max(1.0, np.abs(ua).max()), err_msg=tag)
            assert close_obj(ro, uo), tag
    finally:
        ctx.close()


@pytest.mark.parametrize("route", ["reg256-c40", "deferred-c40"])
def test_second_pass_in_pieces(partls, oracle, monkeypatch, route):
    """PARTLS_TOP_PIECE = 7 at a cap of 1: the second pass, opt_models and opt_top walk the 64 patterns of c40 in ten pieces, the last
    one short; the second pass and the export cut the same pieces, so all_opt is the export's objectives bit for bit"""
    name, env, flags, kernel = CHAIN_ROUTES[route]
    ref = chain(oracle, name)
    c, objs = ref["case"], ref["objs"]
    g0, g1 = 0, ref["npat"]
    assert g1 == 64
    gs = np.arange(g0, g1)
    pats = gs ^ (gs >> 1)
    want = objs[pats]
    knobs = dict(env, PARTLS_MAX_ROUNDS="1", **WALK)

    def pieced(fl):
        monkeypatch.setenv("PARTLS_TOP_PIECE", "7")
        try:
            ctx = ctx_with(partls, monkeypatch, knobs)
        finally:
            monkeypatch.delenv("PARTLS_TOP_PIECE")
        ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], c["flags"] | flags | fl)
        assert ctx.sweep_route() == kernel, route
        return ctx

    plain = pieced(0)
    try:
        m0 = plain.opt_models(g0, g1, raw=True)
        ncapped = int(np.isnan(m0["opt"]).sum())
        assert ncapped > 0 and m0["n_unconverged"] == ncapped, route
    finally:
        plain.close()
    ctx = pieced(RESCUE)
    try:
        bo, bp, allo, unconv = ctx.opt_sweep(g0, g1, want_all=True)
        st = ctx.rescue_stats()
        assert unconv == 0 and st.failed == 0, route
        assert st.rescued == ncapped, "%s: %d rescued, the export of the plain context has %d NaN rows" % (route, st.rescued, ncapped)
        got = allo[pats]
        assert np.isfinite(got).all(), route
        assert close_obj(got, want).all(), "%s: all_opt off by %.3g" % (route, (np.abs(got - want) / np.maximum(1.0, want)).max())
        order = np.lexsort((pats, want))
        if want[order[1]] - want[order[0]] > TOL_OBJ * max(1.0, want[order[0]]):
            assert bp == int(pats[order[0]]), "%s: winner %d, the oracle's %d" % (route, bp, pats[order[0]])
        assert close_obj(bo, objs[bp]), route
        co, cp = ctx.opt_candidates()
        assert len(cp) >= 1 and (co[0], cp[0]) == (bo, bp), route
        m = ctx.opt_models(g0, g1, raw=True)
        assert m["pattern"].tolist() == pats.tolist() and m["n_unconverged"] == 0, route
        assert np.array_equal(m["opt"], allo[pats]), "%s: the second pass's all_opt is not its export's objective" % route
        top = ctx.opt_top(8, g0, g1, raw=True)
        assert top["n_unconverged"] == 0 and top["count"] == 8, route
        same_as_host_sort(top, m, 8)
    finally:
        ctx.close()


@pytest.mark.parametrize("cap", (1, 10))
def test_duplicated_and_scaled_column(partls, oracle, monkeypatch, cap):
    """c40 with a duplicated and a scaled column inside one group: the oracle's objectives, no NaN"""
    c = R.case("c40-dup")
    objs = oracle_objectives(oracle, c, np.arange(64))
    ctx = ctx_with(partls, monkeypatch, dict(PARTLS_MAX_ROUNDS=str(cap), **WALK))
    try:
        ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], FAITHFUL | RESCUE)
        bo, bp, allo, unconv = ctx.opt_sweep(0, -1, want_all=True)
        st = ctx.rescue_stats()
        print("[rescue] c40-dup cap %d: rescued %d, %d pivots, %d vetoes of the sweep" % (cap, st.rescued, st.pivots, ctx.vetoes()))
        assert unconv == 0 and st.failed == 0 and st.rescued > 0
        assert not np.isnan(allo).any() and close_obj(allo, objs).all(), "max error %.3g" % np.nanmax(np.abs(allo - objs))
        assert close_obj(bo, objs.min())
        m = ctx.opt_models(raw=True)
        assert m["n_unconverged"] == 0 and not np.isnan(m["opt"]).any() and not np.isnan(m["raw_alpha"]).any()
        assert close_obj(m["opt"], objs[m["pattern"]]).all()
    finally:
        ctx.close()


def test_out_of_passes_stays_nan_and_is_counted(partls, oracle, monkeypatch):
    """PARTLS_RESCUE_MAX_PASSES = 1 at a cap of 1: every pattern needs more than one main pass, so the rescue solves none"""
    ref = chain(oracle, "c40")
    c = ref["case"]
    ctx = ctx_with(partls, monkeypatch, dict(PARTLS_MAX_ROUNDS="1", PARTLS_RESCUE_MAX_PASSES="1", **WALK))
    monkeypatch.delenv("PARTLS_RESCUE_MAX_PASSES", raising=False)
    try:
        ctx.opt_prepare(c["X"], c["y"], c["P"], c["eta"], FAITHFUL | RESCUE)
        bo, bp, allo, unconv = ctx.opt_sweep(0, -1, want_all=True)
        st = ctx.rescue_stats()
        assert unconv == 64 and (st.rescued, st.failed) == (0, 64) and st.pivots == 64
        assert bp == -1 and np.isnan(allo).all()
        m = ctx.opt_models(raw=True)
        assert m["n_unconverged"] == 64 and np.isnan(m["opt"]).all() and np.isnan(m["raw_alpha"]).all() and np.isnan(m["t"]).all()
        assert ctx.rescue_stats().failed == 64
        top = ctx.opt_top(8)
        assert top["count"] == 0 and top["n_unconverged"] == 64
        for call in (ctx.opt_pattern, ctx.opt_finish):
            with pytest.raises(partls.PartlsError) as err:
                call(5)
            assert err.value.status == ERR_NOT_CONVERGED
    finally:
        ctx.close()


def test_the_entries_out_of_scope(partls, oracle, monkeypatch):
    """partls_cv_opt, partls_opt_weightings and partls_fit_opt_multi refuse the flag; Alt and BnB calls ignore it"""
    ref = chain(oracle, "c40")
    c = ref["case"]
    X, y, P = c["X"], c["y"], c["P"]
    ctx = ctx_with(partls, monkeypatch, {})
    try:
        folds = np.array([0, len(y) // 2, len(y)], dtype=np.int64)
        for call in (lambda: ctx.cv_opt(X, y, P, folds, [0.0], flags=FAITHFUL | RESCUE),
                     lambda: ctx.opt_weightings(X, y, P, np.ones((len(y), 2), order="F"), 0.0, flags=RESCUE)):
            with pytest.raises(partls.PartlsError) as err:
                call()
            assert err.value.status == ERR_UNSUPPORTED
        mc = partls.MultiContext([0, 0])
        try:
            with pytest.raises(partls.PartlsError) as err:
                mc.fit_opt(X, y, P, 0.0, RESCUE)
            assert err.value.status == ERR_UNSUPPORTED
        finally:
            mc.close()
        ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
        plain = ctx.bnb_prepared()
        ctx.opt_prepare(X, y, P, 0.0, FAITHFUL | RESCUE)
        flagged = ctx.bnb_prepared()
        for u, v in zip(plain, flagged):
            np.testing.assert_allclose(np.asarray(u), np.asarray(v), rtol=1e-12, atol=1e-12)
        assert ctx.rescue_stats().rescued == 0
    finally:
        ctx.close()


FIT_CHILD = """
import json, sys, time
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import partls_amd, rescue_reference as R
pkg = partls_amd.package()
c = R.case(%r)
try:
    t0 = time.perf_counter()
    model, _, rep = pkg.fit(pkg.Opt, c["X"], c["y"], c["P"], eta=c["eta"], faithful_intercept=True, rescue=True, returnAllSolutions=True)
    t1 = time.perf_counter()
    ctx = pkg.default_context()
    sweep_ms, rescue_ms = ctx.timing(pkg.lowlevel.T_SWEEP), ctx.timing(pkg.lowlevel.T_RESCUE)
    st = ctx.rescue_stats()
    allo = np.array(rep.solutions._all)
    opt, alpha, beta, t = rep.solutions.arrays()
    t2 = time.perf_counter()
    print("RESULT " + json.dumps(dict(status=0, rescued=int(rep.rescued), pivots=int(st.pivots), failed=int(st.failed), all_opt=allo.tolist(),
                                      opt=opt.tolist(), fit_ms=1e3 * (t1 - t0), sweep_ms=sweep_ms, rescue_ms=rescue_ms, models_ms=1e3 * (t2 - t1),
                                      t=float(model.t))))
except pkg.PartlsError as e:
    print("RESULT " + json.dumps(dict(status=int(e.status))))
"""


def fit_in_child(case, env):
    full = {k: v for k, v in os.environ.items() if k not in ALL_KNOBS}
    full.update(env)
    run = subprocess.run([sys.executable, "-c", FIT_CHILD % (ROOT, os.path.join(ROOT, "tests"), case)], env=full, capture_output=True, text=True,
                         timeout=120)
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
    assert run.returncode == 0 and len(lines) == 1, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    return json.loads(lines[0][7:])


def test_fit_on_the_design_correlated_throughout(oracle):
    """DESIGN.md §7 item 8 at the default cap: without the flag fit reports status 6 (tests/test_gpu_exchange_rule.py); with it, the
    fit returns and every one of the 64 objectives is the oracle's"""
    c = R.case("correlated")
    objs = oracle.fit_opt(c["X"], c["y"], c["P"], return_all=True)["all_opt"]
    got = fit_in_child("correlated", {})
    assert got["status"] == 0, got
    print("[rescue] correlated throughout, n = 176: %d of 64 rescued with %d pivots; fit %.1f ms (sweep incl. second pass %.1f ms, rescue kernel "
          "%.3f ms), all models %.1f ms" % (got["rescued"], got["pivots"], got["fit_ms"], got["sweep_ms"], got["rescue_ms"], got["models_ms"]))
    assert got["rescued"] > 0 and got["failed"] == 0
    for key in ("all_opt", "opt"):
        v = np.array(got[key])
        assert len(v) == 64 and close_obj(v, objs).all(), "%s: max error %.3g" % (key, np.nanmax(np.abs(v - objs) / np.maximum(1.0, objs)))


def test_fit_reports_what_the_rescue_could_not_solve():
    """fit(Opt, rescue=True) with one main pass at a cap of 1: status 6, and the call returns"""
    assert fit_in_child("c40", {"PARTLS_MAX_ROUNDS": "1", "PARTLS_RESCUE_MAX_PASSES": "1"}) == {"status": ERR_NOT_CONVERGED}
    got = fit_in_child("c40", {"PARTLS_MAX_ROUNDS": "1"})
    assert got["status"] == 0 and got["rescued"] >= 64 and got["failed"] == 0
