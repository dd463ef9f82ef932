"""One long-lived context through every entry family: after each call its results equal, byte for byte, those of a fresh context that
ran only that call (helpers: tests/context_reuse.py).  The oracle is the library itself on a new Context(0) under the same knobs; there
is no tolerance.  Every step asserts sweep_route().

The contract per entry family, and where it is written
  prepares (partls_opt_prepare, _weighted, _f32, _csr; host or adopted device arrays)
      include/partls.h, partls_opt_prepare_weighted: "The next plain prepare (or fit) on the context is unweighted again";
      include/partls_csr.h: "The next prepare of any kind decides the storage again"; csrc/ctx.h, forget_problem: "c forgets its prepared
      problem and what its last sweep or solve left behind".  Asserted: a step (prepare, sweep with all_opt where the intercept is
      faithful, finish, gram, bit_order, num_patterns, kkt_violation, the sweep's vetoes) after ANY predecessor equals the fresh step.
  refused prepares
      include/partls.h, above partls_opt_prepare ("A refused prepare"): the argument checks leave the context as it was; the weights
      ("the context is left unprepared", partls_opt_prepare_weighted), a CSR matrix ("on failure the context is left unprepared",
      partls_csr.h), P outside {0,1} and NaN in X leave it unprepared.  The header did not say which of the two holds for ldX < N,
      eta < 0 and NaN in X; csrc/prepare.hip (prepare_begin) decides it and the header now says what the code does.
  partls_predict, _device, _f32, _csr, partls_predict_many, partls_contributions
      "The context's prepared problem, if any, is untouched" (partls.h, partls_predict_many; partls_csr.h, partls_predict_csr;
      partls_contrib.h, which adds "a refused call leaves the context as it was").
  partls_diagnostics
      partls_diag.h: "The prepared problem is untouched: a sweep after the call returns what it returned before"; a CSR problem is
      refused with PARTLS_ERR_UNSUPPORTED, "found before anything is written".
  partls_opt_models, partls_opt_top
      partls.h: "Leaves the state of the last partls_opt_sweep untouched: winner, near ties, exported winner row, candidates, pivot and
      veto counters"; partls_opt_top "as partls_opt_models does".  partls_opt_top_select, _candidates, _bit_order, partls_get_gram read.
  single solves on the prepared problem (partls_opt_pattern, partls_alt_prepared, _multistart, partls_bnb_prepared, _bound, _leaf,
  _search, the snapshot ABI)
      No header promises that they keep the sweep's exported solution.  Asserted: sweeps equal the fresh sweeps; a finish equals the
      fresh default finish or the finish of a fresh context created with PARTLS_NO_EXPORT=1, nothing else.
  partls_cv_opt, _weighted, partls_cv_alt, partls_opt_weightings
      partls.h, partls_cv_opt: "holds no prepared problem (a staged call must prepare again)"; the other two: "Context state afterwards
      as after partls_cv_opt".  Asserted: every staged call returns PARTLS_ERR_STATE with its outputs unwritten, the batched call
      itself repeats its fresh bits on a used context, and every kind of prepare then equals fresh.

Part 1.  Thirteen kinds of problem (context_reuse.make_kinds; the table of routes is asserted per step), in the order of an Eulerian
circuit of the complete digraph on the kinds (context_reuse.euler_circuit: every ordered pair adjacent exactly once, a kind after
itself included; the n = 301 tableau directly before the smallest problem), once under PARTLS_BIT_ORDER=identity and once under
calibrate, on contexts created with PARTLS_PAIR=1.  The generated order, 170 steps (0.14 s and 0.18 s on an MI355X):
  1 2 3 4 5 6 7 8 9 10 11 12 13 1 3 5 7 9 11 13 2 4 6 8 10 12 1 4 7 10 13 3 6 9 12 2 5 8 11 1 5 9 13 4 8 12 3 7 11 2 6 10 1 6 11 3 8 13 5
  10 2 7 12 4 9 1 7 13 6 12 5 11 4 10 3 9 2 8 1 8 2 9 3 10 4 11 5 12 6 13 7 1 9 4 12 7 2 10 5 13 8 3 11 6 1 10 6 2 11 7 3 12 8 4 13 9 5 1
  11 8 5 2 12 9 6 3 13 10 7 4 1 12 10 8 6 4 2 13 11 9 7 5 3 1 13 13 12 12 11 11 10 10 9 9 8 8 7 7 6 6 5 5 4 4 3 3 2 2 1 1

Part 2.  prepare, I, sweep, I, finish, I, sweep, finish for 22 intruders I on six base problems (dense, pair walk, generic kernel,
float32, weighted, CSR; all with a faithful intercept, which the exports and the single solves need), PARTLS_BIT_ORDER=identity.
Which finish reference each intruder matched, as the test prints it: on all six bases EVERY intruder — the fourteen that must
(predict, predict_device, predict_csr, predict_many, contributions, diagnostics, opt_models partial / full, opt_top partial / full,
opt_top_select, opt_candidates, gram, bit_order) and the eight single solves (opt_pattern, alt_prepared, alt_multistart, bnb_prepared,
bnb_bound, bnb_leaf, bnb_search, the snapshot ABI) — matched the DEFAULT finish, in both finishes: no single solve loses the sweep's
exported solution today, and the no-export finish differs from the default one in its bits on every base.  diagnostics on the CSR
base is the one refusal (PARTLS_ERR_UNSUPPORTED at all three stages; the fit around it equals fresh).

Left out, and why
  * partls_opt_merge_candidates, the one-call partls_fit_* entries and the partls_multi contexts: not staged calls of a single context's
    fit; the Python fit() helpers take no context.
  * pivots(), timings, upload statistics: the headers say a later solve overwrites the counters; the last two are not deterministic.
  * The cooperative kernel is never launched on purpose.  The single solves on the generic-kernel problems reach it as the library
    does; on a device so crowded that its grid barrier times out the library solves on one workgroup instead, which is a second
    kernel and need not give the same bits.
  * No fault-injection knob is set.

What it found: no stale state in the library.  One bug in the Python binding: Context._prepare recorded the shape of a prepare BEFORE
the library accepted it, so after a prepare refused by the argument checks (old problem untouched) opt_finish, opt_models and the
solves sized their outputs for the refused problem — too small whenever that one had fewer features.  The shortest sequence is kept as
test_refused_prepare_of_another_shape_keeps_the_old_problems_outputs.
"""
import time

import numpy as np
import pytest

import context_reuse as cr
from context_reuse import FAITHFUL, GENERIC, context, diff, flat, recorded

pytestmark = pytest.mark.gpu

FOLDS, ETAS = [0, 200, 400, 600], [0.0, 0.5]


def new_ctx(partls, monkeypatch, env):
    ctx = context(partls, monkeypatch, env)
    ctx.tolerate_ill = True                                  # status 9 fills the outputs: recorded in the results, not raised
    return ctx


def on_fresh(partls, monkeypatch, env, fn):
    """fn(ctx) on a context of its own"""
    ctx = new_ctx(partls, monkeypatch, env)
    try:
        return fn(ctx)
    finally:
        ctx.close()


# ---- part 1: every kind of prepare after every other ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kinds(partls, oracle):
    return cr.make_kinds(partls, oracle)


_fresh_steps = {}


def fresh_steps(partls, monkeypatch, kinds, order):
    """every kind's step on a context of its own, once per bit order"""
    if order not in _fresh_steps:
        env = {"PARTLS_PAIR": "1", "PARTLS_BIT_ORDER": order}
        res = [on_fresh(partls, monkeypatch, env, lambda ctx: cr.staged_step(ctx, k)) for k in kinds[0]]
        for i, j in cr.SHARED:                               # the kinds on shared data differ, so a remembered predecessor would show
            assert {"finish.alpha", "finish.beta", "finish.opt"} & set(diff(res[i], res[j])), (kinds[0][i].name, kinds[0][j].name)
        moved = [k.name for k, r in zip(kinds[0], res) if not np.array_equal(r["gbit"], np.arange(len(r["gbit"])))]
        print("[reuse] %s: kinds whose groups left their own Gray bits: %s" % (order, moved))
        if order == "calibrate":                             # the visiting order and the flip costs are live state there
            assert moved and sum(bool(np.all(r["flip_cost"] >= 0.0)) for r in res) >= len(res) // 2
        else:
            assert not moved and all(np.all(r["flip_cost"] == -1.0) for r in res)
        _fresh_steps[order] = res
    return _fresh_steps[order]


@pytest.mark.parametrize("order", ["identity", "calibrate"])
def test_every_prepare_after_every_other(partls, monkeypatch, kinds, order):
    K = kinds[0]
    fresh = fresh_steps(partls, monkeypatch, kinds, order)
    circuit = cr.euler_circuit(len(K))
    assert (cr.LARGEST, cr.SMALLEST) in set(zip(circuit, circuit[1:]))           # the large tableau directly before the smallest problem
    print("[reuse] order of kinds (%s): %s" % (order, " ".join(str(i + 1) for i in circuit)))
    ctx = new_ctx(partls, monkeypatch, {"PARTLS_PAIR": "1", "PARTLS_BIT_ORDER": order})
    bad = []
    t0 = time.perf_counter()
    try:
        prev = None
        for i in circuit:
            d = diff(cr.staged_step(ctx, K[i]), fresh[i])
            if d:
                bad.append("%s after %s: %s" % (K[i].name, "nothing" if prev is None else K[prev].name, d))
            prev = i
    finally:
        ctx.close()
    print("[reuse] %d steps in %.2f s, %d differ from fresh" % (len(circuit), time.perf_counter() - t0, len(bad)))
    assert not bad, "\n".join(bad)


# ---- part 2: calls between the stages of one fit --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def query(partls):
    return cr.Query(partls)


def bases(partls, kinds):
    L = partls.lowlevel
    (XA, yA, PA), (XB, yB, PB), (XP, yP, PP) = kinds[1]["A"], kinds[1]["B"], kinds[1]["pair"]
    ident = {"PARTLS_BIT_ORDER": "identity"}

    def kind(name, X, y, P, flags, route, w=None, tiles=None):
        return cr.Kind(name, lambda ctx: ctx.opt_prepare(X, y, P, 0.0, flags, weights=w), route, flags, tiles=tiles)

    return {
        "dense": cr.Base("dense", kind("dense", XA, yA, PA, FAITHFUL, L.ROUTE_REG_256), ident, 20, 4),
        "pair": cr.Base("pair", kind("pair", XP, yP, PP, FAITHFUL, L.ROUTE_REG_512, tiles=11), dict(ident, PARTLS_PAIR="1"), 175, 5),
        "generic": cr.Base("generic", kind("generic", XB, yB, PB, FAITHFUL | GENERIC, L.ROUTE_DEFERRED), ident, 40, 6),
        "float32": cr.Base("float32", kind("float32", np.asfortranarray(XA, dtype=np.float32), yA, PA, FAITHFUL, L.ROUTE_REG_256), ident, 20, 4),
        "weighted": cr.Base("weighted", kind("weighted", XA, yA, PA, FAITHFUL, L.ROUTE_REG_256, w=kinds[1]["wA"]), ident, 20, 4),
        "csr": cr.Base("csr", kind("csr", kinds[1]["csrB"], yB, PB, FAITHFUL, L.ROUTE_REG_256), ident, 40, 6),
    }


BASES = ("dense", "pair", "generic", "float32", "weighted", "csr")
REFUSED = {("diagnostics", "csr"): "ERR_UNSUPPORTED"}        # include/partls_diag.h: a problem prepared from CSR


def uninterrupted(ctx, base):
    """prepare, sweep, finish, sweep, finish -> [S1, F1, S2, F2]"""
    base.kind.prepare(ctx)
    cr.check_route(ctx, base.kind)
    out = []
    for _ in range(2):
        out.append(cr.sweep_result(ctx, base.kind))
        cr.check_route(ctx, base.kind)
        out.append(cr.finish_result(ctx, int(out[-1]["best_pattern"])))
    return out


def interrupted(partls, ctx, base, call):
    """prepare, I, sweep, I, finish, I, sweep, finish -> ([S1, F1, S2, F2], [I1, I2, I3])"""
    base.kind.prepare(ctx)
    cr.check_route(ctx, base.kind)
    fit, intr = [], []
    intr.append(recorded(partls, lambda: call(ctx, base)))
    fit.append(cr.sweep_result(ctx, base.kind))
    cr.check_route(ctx, base.kind)
    intr.append(recorded(partls, lambda: call(ctx, base)))
    fit.append(cr.finish_result(ctx, int(fit[0]["best_pattern"])))
    intr.append(recorded(partls, lambda: call(ctx, base)))
    fit.append(cr.sweep_result(ctx, base.kind))
    cr.check_route(ctx, base.kind)
    fit.append(cr.finish_result(ctx, int(fit[2]["best_pattern"])))
    return fit, intr


def intruder_alone(partls, ctx, base, call, stage):
    """prepare (, sweep (, finish)), I on a fresh context -> I's result"""
    base.kind.prepare(ctx)
    if stage >= 1:
        s = cr.sweep_result(ctx, base.kind)
    if stage >= 2:
        cr.finish_result(ctx, int(s["best_pattern"]))
    return recorded(partls, lambda: call(ctx, base))


@pytest.mark.parametrize("name", BASES)
def test_calls_between_the_stages_of_one_fit(partls, monkeypatch, kinds, query, name):
    L = partls.lowlevel
    base = bases(partls, kinds)[name]
    ref = on_fresh(partls, monkeypatch, base.env, lambda ctx: uninterrupted(ctx, base))
    ref_noexp = on_fresh(partls, monkeypatch, dict(base.env, PARTLS_NO_EXPORT="1"), lambda ctx: uninterrupted(ctx, base))
    assert int(ref[0]["n_unconverged"]) == 0
    base.winner = int(ref[0]["best_pattern"])
    base.model = (ref[1]["alpha"], ref[1]["beta"], float(ref[1]["t"]))
    bad = []
    t0 = time.perf_counter()
    for iname, (ikind, call) in cr.intruders(query).items():
        alone = [on_fresh(partls, monkeypatch, base.env, lambda ctx: intruder_alone(partls, ctx, base, call, s)) for s in range(3)]
        fit, intr = on_fresh(partls, monkeypatch, base.env, lambda ctx: interrupted(partls, ctx, base, call))
        want_status = REFUSED.get((iname, name))
        for s in range(3):
            if want_status is not None:                      # the refusal itself, with the status the header names
                if set(alone[s]) != {"status"} or int(alone[s]["status"]) != getattr(L, want_status):
                    bad.append("%s at stage %d: expected %s, got %s" % (iname, s, want_status, alone[s]))
            elif "status" in alone[s]:
                bad.append("%s at stage %d on a fresh context: status %d" % (iname, s, int(alone[s]["status"])))
            d = diff(intr[s], alone[s])
            if d:
                bad.append("%s at stage %d differs from its fresh run: %s" % (iname, s, d))
        for k in (0, 2):                                     # the sweeps: always the fresh bits
            d = diff(fit[k], ref[k])
            if d:
                bad.append("sweep %d around %s: %s" % (k // 2 + 1, iname, d))
        took = []
        for k in (1, 3):                                     # the finishes
            d, dn = diff(fit[k], ref[k]), diff(fit[k], ref_noexp[k])
            took.append("both" if not d and not dn else "default" if not d else "no-export" if not dn else "NEITHER")
            if d and (ikind == "pure" or dn):
                bad.append("finish %d around %s (%s): differs from the default finish in %s, from the no-export finish in %s"
                           % (k // 2 + 1, iname, ikind, d, dn))
        print("[reuse] %-8s %-18s %-5s finish 1: %-9s finish 2: %s" % (name, iname, ikind, took[0], took[1]))
    print("[reuse] %s: %.2f s" % (name, time.perf_counter() - t0))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("pool", ["tiny_pool", "default_pool"])
def test_solves_from_previous_state(partls, monkeypatch, pool):
    """Alt warm-starts its alpha-steps from the previous tableau (the cooperative kernel's, on the deferred route) and BnB reuses its
    snapshot pool: each solve once after ANOTHER problem's solve of the same n, on one context, equals the solve on a fresh one"""
    from test_gpu_alt_bnb import _branching_problem
    L = partls.lowlevel
    env = {"PARTLS_BIT_ORDER": "identity"}
    if pool == "tiny_pool":
        env["PARTLS_BNB_POOL_MB"] = "1"                      # as tests/test_gpu_alt_bnb.py's tiny_pool mode
    probs = [_branching_problem(seed=7), _branching_problem(seed=8)]          # n = 37 both
    rng = np.random.default_rng(20260031)
    a0, b0 = rng.uniform(0.1, 1.0, 37), rng.uniform(-1.0, 1.0, 7)

    def prepare(ctx, p):
        ctx.opt_prepare(p[0], p[1], p[2], 0.0, FAITHFUL | GENERIC)
        assert ctx.sweep_route() == (L.ROUTE_DEFERRED, 0)

    solves = {"alt_prepared": lambda ctx: ctx.alt_prepared(a0, b0, eps=1e-6, T=30), "bnb_prepared": lambda ctx: ctx.bnb_prepared(),
              "bnb_search": lambda ctx: ctx.bnb_search(0)}
    fresh = {}
    for s, fn in solves.items():
        for q in (0, 1):
            def one(ctx, s=s, fn=fn, q=q):
                prepare(ctx, probs[q])
                return recorded(partls, lambda: fn(ctx))
            fresh[s, q] = on_fresh(partls, monkeypatch, env, one)
            assert "status" not in fresh[s, q], (s, q, fresh[s, q])
        assert diff(fresh[s, 0], fresh[s, 1]), s             # the two problems differ
    assert int(fresh["bnb_search", 0]["3"]) > 20             # nodes bounded: the search branches
    bad = []
    ctx = new_ctx(partls, monkeypatch, env)
    try:
        for before in solves:
            for after in solves:
                prepare(ctx, probs[0])
                d0 = diff(recorded(partls, lambda: solves[before](ctx)), fresh[before, 0])
                prepare(ctx, probs[1])
                d1 = diff(recorded(partls, lambda: solves[after](ctx)), fresh[after, 1])
                if d0 or d1:
                    bad.append("%s on problem 0, then %s on problem 1: %s, %s" % (before, after, d0, d1))
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


# ---- part 3: batched entries and refused calls as predecessors ------------------------------------------------------------------------------
def batched_entries(kinds):
    XA, yA, PA = kinds[1]["A"]
    rng = np.random.default_rng(20260041)
    W = np.asfortranarray(np.stack([rng.multinomial(600, np.full(600, 1 / 600)).astype(np.float64), np.ones(600),
                                    (rng.random(600) < 0.7).astype(np.float64)], axis=1))
    a0, b0 = rng.uniform(0.1, 1.0, (2, 21)), rng.uniform(-1.0, 1.0, (2, 5))
    return {
        "cv_opt": lambda ctx: ctx.cv_opt(XA, yA, PA, FOLDS, ETAS, FAITHFUL),
        "cv_opt weighted": lambda ctx: ctx.cv_opt(XA, yA, PA, FOLDS, ETAS, 0, weights=kinds[1]["wA"]),
        "cv_alt": lambda ctx: ctx.cv_alt(XA, yA, PA, FOLDS, ETAS, a0, b0, eps=1e-6, T=10),
        "opt_weightings": lambda ctx: ctx.opt_weightings(XA, yA, PA, W, 0.0, FAITHFUL),
    }


ENV3 = {"PARTLS_PAIR": "1", "PARTLS_BIT_ORDER": "identity"}


def prepared_and_swept(ctx, kind):
    kind.prepare(ctx)
    cr.check_route(ctx, kind)
    return cr.sweep_result(ctx, kind)


@pytest.mark.parametrize("entry", ["cv_opt", "cv_opt weighted", "cv_alt", "opt_weightings"])
def test_batched_entry_leaves_no_prepared_problem(partls, monkeypatch, kinds, entry):
    """include/partls.h, partls_cv_opt: "holds no prepared problem (a staged call must prepare again)"; partls_opt_weightings and
    partls_cv_alt: "Context state afterwards as after partls_cv_opt\""""
    L = partls.lowlevel
    K = kinds[0]
    fresh = fresh_steps(partls, monkeypatch, kinds, "identity")
    call = batched_entries(kinds)[entry]
    held = K[8]                                              # kind 9: A, eta 0.5, faithful (N = 600, M = 20, K = 4)
    want = on_fresh(partls, monkeypatch, ENV3, lambda ctx: flat(call(ctx)))
    bad = []
    ctx = new_ctx(partls, monkeypatch, ENV3)
    try:
        for i, k in enumerate(K):
            prepared_and_swept(ctx, held if i % 2 == 0 else K[(i + 5) % len(K)])
            d = diff(flat(call(ctx)), want)
            if d:
                bad.append("%s before %s differs from its fresh run: %s" % (entry, k.name, d))
            if i < 2:
                for name, st, outs in cr.raw_staged_calls(partls, ctx, *cr.RAW_SHAPE):
                    if st != L.ERR_STATE or not cr.unwritten(outs):
                        bad.append("%s after %s: status %d, outputs %s" % (name, entry, st, "untouched" if cr.unwritten(outs) else "WRITTEN"))
            d = diff(cr.staged_step(ctx, k), fresh[i])
            if d:
                bad.append("%s after %s: %s" % (k.name, entry, d))
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


def refused_prepares(partls, kinds):
    """name -> (call(ctx), status, whether the context is left unprepared (else: untouched))"""
    L = partls.lowlevel
    XA, yA, PA = kinds[1]["A"]
    XB, yB, PB = kinds[1]["B"]
    csr = kinds[1]["csrB"]
    Xn = XA.copy(order="F")
    Xn[17, 3] = np.nan
    vals = csr.data.copy()
    vals[100] = np.nan
    ptr = csr.indptr.copy()
    ptr[300] = ptr[299] - 1
    idx = csr.indices.copy()
    idx[int(csr.indptr[200])] = 40                           # the first entry of row 200: a column index = M
    w = kinds[1]["wA"]
    wneg, wnan = w.copy(), w.copy()
    wneg[5], wnan[5] = -1.0, np.nan
    dev = kinds[1]["keep"][0]                                # (600 x 30 in HBM, ld 603)
    PC = kinds[1]["C"][2]
    Pbad = PA.copy(order="F")
    Pbad[7, 2] = 2
    return {
        "NaN in X": (lambda ctx: ctx.opt_prepare(Xn, yA, PA), L.ERR_NONFINITE, True),
        "NaN in CSR values": (lambda ctx: ctx.opt_prepare(partls.CSR(csr.indptr, csr.indices, vals, csr.shape), yB, PB), L.ERR_NONFINITE, True),
        "decreasing indptr": (lambda ctx: ctx.opt_prepare(partls.CSR(ptr, csr.indices, csr.data, csr.shape), yB, PB), L.ERR_BAD_ARG, True),
        "column index out of range": (lambda ctx: ctx.opt_prepare(partls.CSR(csr.indptr, idx, csr.data, csr.shape), yB, PB), L.ERR_BAD_ARG, True),
        "negative weight": (lambda ctx: ctx.opt_prepare(XA, yA, PA, weights=wneg), L.ERR_BAD_ARG, True),
        "NaN weight": (lambda ctx: ctx.opt_prepare(XA, yA, PA, weights=wnan), L.ERR_NONFINITE, True),
        "weights summing to 0": (lambda ctx: ctx.opt_prepare(XA, yA, PA, weights=np.zeros(600)), L.ERR_BAD_ARG, True),
        "an entry of P outside {0,1}": (lambda ctx: ctx.opt_prepare(XA, yA, Pbad), L.ERR_BAD_PARTITION, True),
        "ldX < N": (lambda ctx: ctx.opt_prepare_device(dev.ptr("X"), dev.ptr("y"), 600, 30, 599, PC), L.ERR_BAD_ARG, False),
        "eta < 0": (lambda ctx: ctx.opt_prepare(XB, yB, PB, -1.0), L.ERR_BAD_ARG, False),
    }


def test_refused_prepare_leaves_the_documented_state(partls, monkeypatch, kinds):
    """Errors of the weights and of the CSR validation: "the context is left unprepared" (include/partls.h, partls_opt_prepare_weighted;
    include/partls_csr.h).  NaN in a dense X is found in the Gram products, after the reset: unprepared as well.  ldX < N and eta < 0 are
    refused by the argument checks that precede the reset (csrc/prepare.hip: prepare_begin): the old problem is untouched."""
    L = partls.lowlevel
    K = kinds[0]
    fresh = fresh_steps(partls, monkeypatch, kinds, "identity")
    held = K[8]
    want_sweep = on_fresh(partls, monkeypatch, ENV3, lambda ctx: prepared_and_swept(ctx, held))
    want_fit = on_fresh(partls, monkeypatch, ENV3, lambda ctx: cr.finish_result(ctx, int(prepared_and_swept(ctx, held)["best_pattern"])))
    bad = []
    ctx = new_ctx(partls, monkeypatch, ENV3)
    try:
        for j, (name, (call, status, unprepared)) in enumerate(refused_prepares(partls, kinds).items()):
            prepared_and_swept(ctx, held)
            with pytest.raises(partls.PartlsError) as e:
                call(ctx)
            if e.value.status != status:
                bad.append("%s: status %d, expected %d" % (name, e.value.status, status))
            if unprepared:
                for cname, st, outs in cr.raw_staged_calls(partls, ctx, *cr.RAW_SHAPE)[:2]:
                    if st != L.ERR_STATE or not cr.unwritten(outs):
                        bad.append("%s after '%s': status %d, outputs %s" % (cname, name, st, "untouched" if cr.unwritten(outs) else "WRITTEN"))
            else:
                s = cr.sweep_result(ctx, held)
                d = diff(s, want_sweep) + diff(cr.finish_result(ctx, int(s["best_pattern"])), want_fit)
                if d:
                    bad.append("the old problem after '%s': %s" % (name, d))
            i = (3 * j + 1) % len(K)                         # the next valid prepare: another kind every time
            d = diff(cr.staged_step(ctx, K[i]), fresh[i])
            if d:
                bad.append("%s after '%s': %s" % (K[i].name, name, d))
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


def test_refused_prepare_of_another_shape_keeps_the_old_problems_outputs(partls, monkeypatch, kinds):
    """The shortest sequence of the one bug this module found: prepare(A: M = 20, K = 4), sweep, prepare(B: M = 40, K = 6, eta = -1)
    refused with the old problem untouched, finish.  Context.opt_finish sized alpha and beta for the REFUSED problem's shape."""
    L = partls.lowlevel
    held = kinds[0][8]
    XB, yB, PB = kinds[1]["B"]
    want = on_fresh(partls, monkeypatch, ENV3, lambda ctx: cr.finish_result(ctx, int(prepared_and_swept(ctx, held)["best_pattern"])))

    def run(ctx):
        s = prepared_and_swept(ctx, held)
        with pytest.raises(partls.PartlsError) as e:
            ctx.opt_prepare(XB, yB, PB, -1.0)
        assert e.value.status == L.ERR_BAD_ARG
        return cr.finish_result(ctx, int(s["best_pattern"]))

    got = on_fresh(partls, monkeypatch, ENV3, run)
    assert got["alpha"].shape == (20,) and got["beta"].shape == (4,)
    assert not diff(got, want)


def test_refused_auxiliary_calls_leave_the_fit_alone(partls, monkeypatch, kinds, query):
    L = partls.lowlevel
    q = query
    bs = bases(partls, kinds)
    nan_alpha = q.alpha[:2].copy()
    nan_alpha[1, 4] = np.nan

    def raw_many(ctx):
        st, yh = cr.raw_predict_many(partls, ctx, q.X, q.P, q.alpha, q.beta, q.t, 0)
        assert cr.unwritten([yh])
        return st

    def raising(fn):
        def call(ctx):
            with pytest.raises(partls.PartlsError) as e:
                fn(ctx)
            return e.value.status
        return call

    cases = {
        "diagnostics on a CSR problem": ("csr", raising(lambda ctx: ctx.diagnostics(np.full(40, 0.5), np.ones(6), 0.25)), L.ERR_UNSUPPORTED),
        "contributions with a NaN model": ("dense", raising(lambda ctx: ctx.contributions(q.X, q.P, nan_alpha, q.beta[:2])), L.ERR_BAD_ARG),
        "predict_many with B = 0": ("dense", raw_many, L.ERR_BAD_ARG),
        "opt_top with k beyond its limit": ("dense", raising(lambda ctx: ctx.opt_top(L.OPT_TOP_MAX_K + 1)), L.ERR_BAD_ARG),
    }
    bad = []
    for name, (bname, call, status) in cases.items():
        base = bs[bname]
        ref = on_fresh(partls, monkeypatch, base.env, lambda ctx: uninterrupted(ctx, base))

        def run(ctx):
            base.kind.prepare(ctx)
            st = [call(ctx)]
            s1 = cr.sweep_result(ctx, base.kind)
            st.append(call(ctx))
            f1 = cr.finish_result(ctx, int(s1["best_pattern"]))
            st.append(call(ctx))
            s2 = cr.sweep_result(ctx, base.kind)
            cr.check_route(ctx, base.kind)
            return st, [s1, f1, s2, cr.finish_result(ctx, int(s2["best_pattern"]))]

        st, fit = on_fresh(partls, monkeypatch, base.env, run)
        if st != [status] * 3:
            bad.append("%s: statuses %s, expected %d" % (name, st, status))
        for k in range(4):
            d = diff(fit[k], ref[k])
            if d:
                bad.append("%s: stage %d of the fit differs from fresh: %s" % (name, k, d))
    assert not bad, "\n".join(bad)
