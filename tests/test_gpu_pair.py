"""The pair walk of the 512-thread register sweep kernel (csrc/sweep_blk.hip, chain mode, PAIR): of two patterns
that differ in internal bit 0 only the tableau visits one, and the other — its twin — is priced from the columns of its violators C
(a |C| x |C| solve on one wave, |C| FMAs per row, one KKT scan) without a pivot on the tableau; a twin that pricing cannot finish is
solved by the ordinary rounds.

Shapes: n = 176 (T = 11) and n = 256 (T = 16) tableau variables, K = 6 groups, N = 2 D + 50 rows — the smallest problems that put a
pair walk with a multi-column twin on that kernel; both intercept modes (faithful: n = D + 1, 128 patterns, all_opt exists; fitted:
n = D, 64 patterns, winner and objective only).  Every case takes contexts of its own with PARTLS_PAIR=1 / 0 (and PARTLS_REG_MAXT
where the route needs it) and asserts the route.  The bit order of problems this small is the identity, so group 0 sits on bit 0:

  plain     random groups, group 0 of 12 features: twins are priced — pivots() falls strictly below the paired-off walk's;
  straddle  group 0 = 10 all-zero columns followed by 12 features: its live variables are tableau variables 10..21, two tile columns;
  wide      group 0 of 20 features that all carry signal: |C| > 16, every twin takes the ordinary path, and the walk then IS the plain
            walk (the tableau goes on from the twin), so the pivot count is not below the paired-off count by more than the chains'
            first patterns' share;
  null      group 0 of all-zero columns, group 1 without a feature: C is empty, the twin's objective is the committed member's, bit for bit;
  dup       exactly duplicated columns.  Four features of group 0 have a copy in another group: such a copy never meets the guard — while
            one of the two is basic the other's reduced cost is 0, so it is no violator and never in C.  Two features of group 0 are
            copies of EACH OTHER: where the committed member has both nonbasic and the twin's signs let them in, both are in C with the
            same reduced cost, the first enters, the second's pivot is then ~1e-16 and the guard (pair_solve: entering pivot <= 1e-4)
            sends the twin to the rounds, whose rejection rule applies (tools/pair_emul.py: `guard` > 0 on every dup problem);
  overlap   features of two groups (group 0 among them) and a feature of none;
  edges     PARTLS_CHAIN_LEN = 1, 2, 3, 7 (odd chains leave patterns without partner), sub-ranges with odd g0, odd g1 and g1 - g0 = 1;
            ranges covered piecewise equal the full enumeration.

Every case checks: all_opt against the oracle at |opt - ref| <= 1e-9 max(1, ref) (tests/test_gpu_opt.py's bound); the winner identical
to a PARTLS_PAIR=0 run of the same problem; all_opt of the two runs within rtol 1e-10 (two walks of one problem); unconverged == 0.
The winner is compared as it is, no bit cleared: null's exact ties lie inside one chain and are bit-equal, so the first-index rule
decides them the same way in both walks, and no other kind has a group whose flip changes nothing.

Every kind but wide and null also asserts pivots() strictly below the paired-off walk's — twins were priced, for straddle through the
two-tile-column gather — and every case runs the finish on the sweep's winner with PARTLS_FINISH_TRACE: best_index equals the paired-off
run's, the objective agrees within rtol 1e-10, and where the paired-off walk's best_sol was taken by the finish (it carries the
winner's signs) the pair walk's is taken too — a best_sol written from a priced twin's temporaries (qt, bt) with the committed
member's signs or basis would be refused there — where the sweep's winner is a priced twin, which these problems do not guarantee:
tests/test_gpu_pair_routes.py has the problems that do, the other tile counts and the automatic route.  tools/pair_emul.py walks these very problems on the CPU, reports the priced and the
hard twins of each and fails unless every kind has the twins it is there for."""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAITHFUL = 1                                                # PARTLS_OPT_FAITHFUL_INTERCEPT (include/partls.h)
REG_512 = 2                                                 # partls_route (include/partls.h)
K = 6
TOL_OBJ = 1e-9                                              # tests/test_gpu_opt.py
TOL_WALKS = 1e-10                                           # two walks of one problem
KINDS = ("plain", "straddle", "wide", "null", "dup", "overlap")
SIZES = (176, 256)
CASES = tuple((kind, n, flags) for kind in KINDS for n in SIZES for flags in (FAITHFUL, 0))
ENV_KNOBS = ("PARTLS_REG_MAXT", "PARTLS_CHAIN_LEN", "PARTLS_NO_EXPORT", "PARTLS_EAGER_GENERIC", "PARTLS_GRID", "PARTLS_PAIR", "PARTLS_BIT_ORDER",
             "PARTLS_FINISH_TRACE")
PRICED_KINDS = ("plain", "straddle", "dup", "overlap")       # kinds whose pair walk must save pivots (tools/pair_emul.py: easy twins on each)
COUPLING = 0.01                                             # see problem()
SEED = {"plain": 0, "straddle": 0, "wide": 0, "null": 0, "dup": 0, "overlap": 0}


def problem(kind, n, flags=FAITHFUL, K=K, coupling=COUPLING):
    """(X, y, P) of one kind; K groups, the part of group 0's columns inside the span of the others scaled to `coupling` (the defaults
    draw the problems of this file; tests/test_gpu_pair_routes.py asks for longer enumerations and other couplings)"""
    D = n - 1 if flags & FAITHFUL else n
    N = 2 * D + 50
    rng = np.random.default_rng(20262000 + 1000 * n + 100 * SEED[kind] + 17 * KINDS.index(kind) + (flags & FAITHFUL))
    X = rng.standard_normal((N, D))
    n0 = {"plain": 12, "straddle": 22, "wide": 20, "null": 2, "dup": 12, "overlap": 10}[kind]
    lo = 2 if kind == "null" else 1                                     # the first group the other features are dealt to
    hi = K
    grp = rng.integers(lo, hi, D)
    grp[rng.choice(D, hi - lo, replace=False)] = np.arange(lo, hi)      # each of those groups has a feature
    g0 = np.sort(rng.choice(np.flatnonzero(np.bincount(grp, minlength=K)[grp] > 1), n0, replace=False))
    grp[g0] = 0
    assert all((grp == k).any() for k in range(lo, hi)) and (grp == 0).sum() == n0
    w = rng.standard_normal(D) * (rng.random(D) < 0.6)
    w[g0] = rng.choice([-1.0, 1.0], n0) * (0.5 + rng.random(n0))        # every feature of group 0 carries signal
    # With N = 2 D + 50 rows the columns correlate at the 1 / sqrt(N) level, and a flip of group 0 at full coupling leaves violators in
    # the other groups after EVERY block pivot on C (tools/pair_emul.py: 64 hard twins of 64; on the flagship problem, N = 100 000, nine
    # twins in ten are easy).  The part of group 0's columns inside the span of the others is scaled to 1 %: most twins are then
    # priced, some stay hard, and the rows' |C| FMAs still decide which.
    oth = np.flatnonzero(grp != 0)
    Q, _ = np.linalg.qr(np.column_stack([X[:, oth], np.ones(N)]))
    par = Q @ (Q.T @ X[:, g0])
    X[:, g0] += (coupling - 1.0) * par
    if kind == "straddle":
        X[:, g0[:10]] = 0.0                                             # tableau variables 0..9 never move; 10..21 straddle tile columns 0 and 1
    if kind == "null":
        X[:, g0] = 0.0
    if kind == "dup":
        for a in g0[:4]:                                                # four exact duplicates of features of group 0 in other groups
            b = int(rng.choice(np.flatnonzero(grp != 0)))
            X[:, b] = X[:, a]
        X[:, g0[5]] = X[:, g0[4]]                                       # ... and two features of group 0 that are copies of each other
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    if kind == "overlap":
        for m in g0[:3]:
            P[m, 1 + int(rng.integers(0, hi - 1))] = 1                  # features of group 0 and of another group
        for m in np.flatnonzero(grp != 0)[:3]:
            P[m, grp[m] + 1 if grp[m] + 1 < hi else 1] = 1                   # ... and of two of the others
        P[np.flatnonzero(grp != 0)[-1]] = 0                             # a feature of no group
    y = X @ w + 0.4 + 0.3 * rng.standard_normal(N)
    return np.asfortranarray(X), y, np.asfortranarray(P)


def context(partls, monkeypatch, env):
    """a Context with the given knobs (read once, at partls_create)"""
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = partls.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


def sweep(partls, monkeypatch, X, y, P, flags, pair, env=None, ranges=None, capfd=None):
    """the enumeration (or the listed sub-ranges) on a context of its own: dict(obj, pat, all, pivots); with capfd also the finish on
    the sweep's winner: fin = dict(opt, index, taken: the finish took the kernel's best_sol)"""
    n = X.shape[1] + (1 if flags & FAITHFUL else 0)
    knobs = {"PARTLS_PAIR": "1" if pair else "0", "PARTLS_REG_MAXT": "18"}
    knobs.update(env or {})
    if capfd is not None:
        knobs["PARTLS_FINISH_TRACE"] = "1"
    ctx = context(partls, monkeypatch, knobs)
    try:
        ctx.opt_prepare(X, y, P, 0.0, flags)
        assert ctx.sweep_route() == (REG_512, (n + 15) // 16), ctx.sweep_route()
        assert ctx.bit_order()[0].tolist() == list(range(ctx.num_patterns().bit_length() - 1))       # group 0 on bit 0
        npat = ctx.num_patterns()
        allo = np.full(npat, np.nan)
        best, piv = [], 0
        for lo, hi in ranges or [(0, npat)]:
            bo, bp, part, unconv = ctx.opt_sweep(lo, hi, want_all=bool(flags & FAITHFUL))
            assert unconv == 0, "%d patterns hit the pivot cap in [%d, %d)" % (unconv, lo, hi)
            if part is not None:
                seen = ~np.isnan(part)
                assert seen.sum() == hi - lo and not (seen & ~np.isnan(allo)).any()
                allo[seen] = part[seen]
            best.append((bo, bp))
            piv += ctx.pivots()
        bo, bp = min(best)
        fin = None
        if capfd is not None:
            assert ranges is None
            sys.stdout.write(capfd.readouterr().out)                    # (what was printed so far stays in the report)
            ctx.tolerate_ill = True                                     # dup: the data-space verdict is not this test's subject
            _, _, _, fo, fidx = ctx.opt_finish(bp)
            err = capfd.readouterr().err
            assert "the sweep's solution of its winner" in err, err
            fin = dict(opt=fo, index=fidx, taken="): taken" in err)
        return dict(obj=bo, pat=bp, all=allo, pivots=piv, fin=fin)
    finally:
        ctx.close()


_REF = {}


def reference(oracle, partls, monkeypatch, capfd, kind, n, flags):
    """the problem, the oracle's optimum of every pattern (faithful mode) and the paired-off walk, computed once per case"""
    key = (kind, n, flags)
    if key not in _REF:
        X, y, P = problem(kind, n, flags)
        objs = None
        if flags & FAITHFUL:
            Xo, Po = oracle.homogeneous(X, P)
            R, z = oracle.compress(Xo, y)
            objs = oracle.opt_patterns(R, z, Po, np.arange(1 << (K + 1)))
        off = sweep(partls, monkeypatch, X, y, P, flags, pair=False, capfd=capfd)
        _REF[key] = dict(X=X, y=y, P=P, objs=objs, off=off, flags=flags)
    return _REF[key]


def check(tag, ref, got):
    objs, off = ref["objs"], ref["off"]
    if objs is not None:
        err = np.abs(got["all"] - objs) / np.maximum(1.0, np.abs(objs))
        dif = np.abs(got["all"] - off["all"]) / np.abs(off["all"])
        print("[pair] %s: max error %.3g relative to max(1, obj), against the paired-off walk %.3g; %d pivots (paired off: %d); winner %d (%d)" % (
            tag, err.max(), dif.max(), got["pivots"], off["pivots"], got["pat"], off["pat"]))
        assert np.all(np.abs(got["all"] - objs) <= TOL_OBJ * np.maximum(1.0, np.abs(objs))), "%s: max error %.3g" % (tag, err.max())
        np.testing.assert_allclose(got["all"], off["all"], rtol=TOL_WALKS, err_msg=tag)
        assert abs(got["obj"] - got["all"][got["pat"]]) <= TOL_WALKS * max(1.0, got["obj"]), tag
    else:
        print("[pair] %s: %d pivots (paired off: %d); winner %d (%d), objective %.17g (%.17g)" % (
            tag, got["pivots"], off["pivots"], got["pat"], off["pat"], got["obj"], off["obj"]))
    assert got["pat"] == off["pat"], "%s: winner %d, paired off %d" % (tag, got["pat"], off["pat"])
    assert abs(got["obj"] - off["obj"]) <= TOL_WALKS * max(1.0, off["obj"]), tag
    if got["fin"] is not None:
        fg, fo = got["fin"], off["fin"]
        print("[pair] %s: finish best_index %d (%d), objective %.17g (%.17g), best_sol taken %s (%s)" % (
            tag, fg["index"], fo["index"], fg["opt"], fo["opt"], fg["taken"], fo["taken"]))
        assert fg["index"] == fo["index"], tag
        assert abs(fg["opt"] - fo["opt"]) <= TOL_WALKS * max(1.0, fo["opt"]), tag
        assert fg["taken"] or not fo["taken"], "%s: the finish refused the pair walk's best_sol" % tag


@pytest.mark.parametrize("kind,n,flags", CASES)
def test_pair_walk(partls, oracle, monkeypatch, capfd, kind, n, flags):
    ref = reference(oracle, partls, monkeypatch, capfd, kind, n, flags)
    X, y, P, off = ref["X"], ref["y"], ref["P"], ref["off"]
    got = sweep(partls, monkeypatch, X, y, P, flags, pair=True, capfd=capfd)
    tag = "%s n=%d %s" % (kind, n, "faithful" if flags else "fitted")
    check(tag, ref, got)
    if kind in PRICED_KINDS:
        assert got["pivots"] < off["pivots"], (got["pivots"], off["pivots"])           # the witness that twins were priced
    if kind == "wide":
        # every twin takes the ordinary path: nothing is saved beyond (at most) the chains' first patterns.  Both walks once more on chains
        # of this test's own length, so that the chain starts are known: g0 = 0, clen, 2 clen, ...
        npat, clen, share = len(got["all"]), 8, 0
        env = {"PARTLS_CHAIN_LEN": str(clen)}
        on = sweep(partls, monkeypatch, X, y, P, flags, pair=True, env=env)
        offc = sweep(partls, monkeypatch, X, y, P, flags, pair=False, env=env)
        ctx = context(partls, monkeypatch, dict(env, PARTLS_PAIR="0", PARTLS_REG_MAXT="18"))
        try:
            ctx.opt_prepare(X, y, P, 0.0, flags)
            for g0 in range(0, npat, clen):
                assert ctx.opt_sweep(g0, g0 + 1)[3] == 0
                share += ctx.pivots()
        finally:
            ctx.close()
        print("[pair] %s: chains of %d: %d pivots (paired off: %d), first patterns' share %d" % (tag, clen, on["pivots"], offc["pivots"], share))
        assert on["pat"] == offc["pat"] == off["pat"], tag
        assert on["pivots"] >= offc["pivots"] - share, (on["pivots"], offc["pivots"], share)
    if kind == "null" and flags & FAITHFUL:
        pats = np.arange(len(got["all"]))
        assert np.array_equal(got["all"], got["all"][pats & ~1])                        # C is empty: the committed member's objective, bit for bit


@pytest.mark.parametrize("n", SIZES)
def test_pair_walk_edges(partls, oracle, monkeypatch, capfd, n):
    """chains of 1, 2, 3, 7 and sub-ranges with odd ends: patterns without partner are ordinary patterns"""
    ref = reference(oracle, partls, monkeypatch, capfd, "plain", n, FAITHFUL)
    X, y, P = ref["X"], ref["y"], ref["P"]
    base = sweep(partls, monkeypatch, X, y, P, FAITHFUL, pair=True)
    check("edges n=%d" % n, ref, base)
    npat = len(ref["objs"])
    walks = [("chain %s" % cl, dict(env={"PARTLS_CHAIN_LEN": cl})) for cl in ("1", "2", "3", "7")]
    walks.append(("odd ranges", dict(ranges=[(0, 1), (1, 22), (22, 23), (23, 47), (47, 48), (48, 101), (101, npat)])))
    walks.append(("odd ranges, chain 3", dict(env={"PARTLS_CHAIN_LEN": "3"}, ranges=[(0, 5), (5, 31), (31, npat)])))
    for name, kw in walks:
        got = sweep(partls, monkeypatch, X, y, P, FAITHFUL, pair=True, **kw)
        check("edges n=%d %s" % (n, name), ref, got)
        assert got["pat"] == base["pat"], name
        np.testing.assert_allclose(got["all"], base["all"], rtol=TOL_WALKS, err_msg=name)
