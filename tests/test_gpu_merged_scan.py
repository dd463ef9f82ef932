"""The merged KKT scan of the register sweep kernels (csrc/sweep_blk.hip, chain mode): the scan that finds pattern g solved also
publishes the violators of pattern g + 1, whose exchange starts from it without a scan of its own.

Each case is the smallest shape that reaches one edge of that transition, on the 256-thread kernel (n = 40, T = 3) and on the
512-thread kernel (n = 176, T = 11), K = 5 groups, faithful intercept (n = D + 1 variables, 2^(K+1) = 64 patterns), N = 2 D + 50 rows:

  null     a group of all-zero columns and a group with no feature, on the two lowest Gray bits: their flips change nothing, so the
           successor is optimal at the confirming scan (count2 == 0), and so is the pattern after it.  Witness: the pivot counter of a
           single chain stands still over exactly those patterns (asserted);
  dup      exactly duplicated columns in different groups: the duplicate is rejected as dependent inside a round (`blocked`) and has to
           be re-examined afterwards.  Witness (tools/merged_scan_edges.py, the CPU emulation of the kernel's decisions on these very
           problems): 3 / 13 rejections in the full walk at n = 40 / 176, 12 / 28 with chains of 7.  What is NOT reached, here or by any
           problem that keeps the 1e-9 bound: a rejection still standing at a CONFIRMING scan.  That needs a round whose only violators
           are all rejected; a rejected column is dependent on the basis, an exactly dependent column has a zero gradient there and is
           no violator, and a nearly dependent one with a gradient above the tolerance is a column whose rejection moves the objective
           far beyond 1e-9 of the oracle's.  The emulation counts 0 such scans.  That `nxt` ignores `blocked` is therefore checked by
           reading (the predicate has no `blocked` term), not by a run;
  plain    chain boundaries: PARTLS_CHAIN_LEN = 1, 2, 3, 7 and the default, and sub-ranges opt_sweep(g0, g1) with odd ends;
  overlap  n = 48: features of two groups (|f| = 2) and a feature of no group (f = 0).

Every case compares all_opt of the full enumeration with the oracle's per-pattern optimum (dense Lawson-Hanson on QR-compressed
data) at tests/test_gpu_opt.py's tolerance, |opt - ref| <= 1e-9 max(1, ref), and the winner with the reference kernel's
(sweep_generic.hip: PARTLS_OPT_GENERIC_KERNEL with PARTLS_EAGER_GENERIC=1 on a context of its own, route asserted).  Where flips change nothing the patterns that differ only in those groups are the
same problem and tie exactly in exact arithmetic; the two kernels may break such a tie differently, so winners are compared after
clearing the bits of those groups.  Two walks of one problem (other chain lengths, sub-ranges) start their chains elsewhere, take
different pivot paths — 846 against 813 pivots in the stored counts — and so agree to rounding, not bit for bit: the winner must be
identical, all_opt within rtol 1e-10, the bound test_gpu_lazy.py and test_gpu_tile_counts.py use for two walks.

Decision identity: the kernel takes the decisions of the kernel before the merged scan, pivot for pivot, so pivots(), vetoes() and
best_index of four seeded problems equal the numbers stored in tests/golden/merged_scan_counts.json (produced by
tools/merged_scan_counts.py with the library of the commit before this change)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAITHFUL, GENERIC = 1, 2                                    # PARTLS_OPT_FAITHFUL_INTERCEPT, PARTLS_OPT_GENERIC_KERNEL (include/partls.h)
REG_256, REG_512, EAGER = 1, 2, 4                           # partls_route (include/partls.h)
K = 5
TOL_OBJ = 1e-9                                              # tests/test_gpu_opt.py
TOL_WALKS = 1e-10                                           # two walks of one problem
SIZES = (40, 176)
ENV_KNOBS = ("PARTLS_REG_MAXT", "PARTLS_CHAIN_LEN", "PARTLS_NO_EXPORT", "PARTLS_EAGER_GENERIC", "PARTLS_GRID")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merged_scan_counts.json")
# (kind, n, seed, flags) of the decision-identity problems: both kernels, both intercept modes
COUNT_CASES = (("plain", 40, 1, FAITHFUL), ("dup", 40, 2, 0), ("dup", 176, 3, FAITHFUL), ("plain", 176, 4, 0))


def problem(kind, n, seed=0, flags=FAITHFUL):
    """(X, y, P, dead): dead = bit mask (pattern index bits = groups) of the groups whose flip changes nothing"""
    D = n - 1 if flags & FAITHFUL else n
    N = 2 * D + 50
    rng = np.random.default_rng(20261000 + 1000 * n + seed + 17 * ("plain", "null", "dup", "overlap").index(kind))
    X = rng.standard_normal((N, D))
    used = K - 2 if kind == "null" else (K - 1 if kind == "overlap" else K)
    grp = rng.integers(0, used, D)
    grp[rng.choice(D, used, replace=False)] = np.arange(used)          # every used group has a feature
    dead = 0
    if kind == "null":
        # groups 0 and 1 are the dead ones: they sit on the two lowest Gray bits (the bit order of a problem this small is the
        # identity; a calibrated order would put the cheapest flips there too), so three patterns of every four follow a dead flip
        grp += 2
        z = rng.choice(D, 2, replace=False)
        grp[z] = 0                                                      # group 0: two all-zero columns; group 1: no feature
        X[:, z] = 0.0
        assert all((grp == k).any() for k in range(2, K)) and not (grp == 1).any()
        dead = 0b11
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    w = rng.standard_normal(D) * (rng.random(D) < 0.6)
    if kind == "dup":
        for _ in range(4):                                              # four exact duplicates, each pair in two different groups
            a = int(rng.integers(0, D))
            b = int(rng.choice(np.flatnonzero(grp != grp[a])))
            X[:, b] = X[:, a]
    if kind == "overlap":
        for m in range(0, 12, 3):
            P[m, (grp[m] + 1) % used] = 1                               # features of two groups
        P[D - 1] = 0                                                    # a feature of no group
        dead = 1 << (K - 1)                                             # group K - 1 is empty
    y = X @ w + 0.4 + 0.3 * rng.standard_normal(N)
    return np.asfortranarray(X), y, np.asfortranarray(P), dead


def route(n):
    T = (n + 15) // 16
    return (REG_256 if T <= 10 else REG_512, T)


def context(partls, monkeypatch, env=None):
    """a Context with the given knobs (read once, at partls_create)"""
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    ctx = partls.Context(0)
    for k in env or {}:
        monkeypatch.delenv(k)
    return ctx


def sweep(partls, monkeypatch, X, y, P, flags=FAITHFUL, env=None, ranges=None, expect_route=None):
    """full enumeration (or the listed sub-ranges) on a context of its own: dict(obj, pat, all, pivots, vetoes)"""
    ctx = context(partls, monkeypatch, env)
    try:
        ctx.opt_prepare(X, y, P, 0.0, flags)
        if expect_route is not None:
            assert ctx.sweep_route() == expect_route, (ctx.sweep_route(), expect_route)
        npat = ctx.num_patterns()
        allo = np.full(npat, np.nan)
        best, piv, vet = [], 0, 0
        for lo, hi in ranges or [(0, npat)]:
            bo, bp, part, unconv = ctx.opt_sweep(lo, hi, want_all=bool(flags & FAITHFUL))      # all_opt exists in faithful mode only
            assert unconv == 0, "%d patterns hit the pivot cap in [%d, %d)" % (unconv, lo, hi)
            if part is not None:
                seen = ~np.isnan(part)
                assert seen.sum() == hi - lo and not (seen & ~np.isnan(allo)).any()
                allo[seen] = part[seen]
            best.append((bo, bp))
            piv += ctx.pivots()
            vet += ctx.vetoes()
        bo, bp = min(best)
        return dict(obj=bo, pat=bp, all=allo, pivots=piv, vetoes=vet)
    finally:
        ctx.close()


_REF = {}


def reference(oracle, partls, monkeypatch, kind, n):
    """the problem, the oracle's optimum of every faithful pattern and the reference kernel's winner, computed once per case"""
    if (kind, n) not in _REF:
        X, y, P, dead = problem(kind, n)
        Xo, Po = oracle.homogeneous(X, P)
        R, z = oracle.compress(Xo, y)
        pats = np.arange(1 << (K + 1))
        objs = oracle.opt_patterns(R, z, Po, pats)
        np.testing.assert_allclose(objs, objs[pats & ~dead], rtol=1e-12)               # the construction: those flips change nothing
        # the reference kernel (sweep_generic.hip): the flag takes the problem off the register kernels, the knob picks the eager
        # kernel among the others; the route is asserted, so that it cannot fall back to the kernel under test
        gen = sweep(partls, monkeypatch, X, y, P, flags=FAITHFUL | GENERIC, env={"PARTLS_EAGER_GENERIC": "1"}, expect_route=(EAGER, 0))
        _REF[(kind, n)] = dict(X=X, y=y, P=P, dead=dead, objs=objs, gen=gen)
    return _REF[(kind, n)]


def check(tag, ref, got):
    """all_opt against the oracle, the winner against the reference kernel's"""
    objs, gen, dead = ref["objs"], ref["gen"], ref["dead"]
    err = np.abs(got["all"] - objs) / np.maximum(1.0, np.abs(objs))
    print("[merged scan] %s: max error %.3g relative to max(1, obj); %d pivots, %d vetoes; winner %d, reference kernel %d" % (
        tag, err.max(), got["pivots"], got["vetoes"], got["pat"], gen["pat"]))
    assert np.all(np.abs(got["all"] - objs) <= TOL_OBJ * np.maximum(1.0, np.abs(objs))), "%s: max error %.3g" % (tag, err.max())
    assert got["pat"] & ~dead == gen["pat"] & ~dead, "%s: winner %d, reference kernel %d" % (tag, got["pat"], gen["pat"])
    assert abs(got["obj"] - gen["obj"]) <= TOL_WALKS * max(1.0, gen["obj"]), tag
    assert abs(got["obj"] - got["all"][got["pat"]]) <= TOL_WALKS * max(1.0, got["obj"]), tag


@pytest.mark.parametrize("n", SIZES)
def test_flip_that_changes_nothing(partls, oracle, monkeypatch, n):
    """a group of zero columns and a group without a feature: patterns that differ only in them are the same problem — the oracle and
    the sweep give them the same optimum — and the sweep solves them without a pivot"""
    ref = reference(oracle, partls, monkeypatch, "null", n)
    dead, objs = ref["dead"], ref["objs"]
    pats = np.arange(len(objs))
    got = sweep(partls, monkeypatch, ref["X"], ref["y"], ref["P"], expect_route=route(n))
    check("null n=%d" % n, ref, got)
    # witness that the edge is reached: in ONE chain the pivots of the first g patterns do not grow over a pattern that follows a dead flip
    # (Gray index g with g % 4 != 0: the flipped bit is 0 or 1), three in a row each time — count2 == 0 at the confirming scan of the pattern
    # before, and again at the scan after it — and do grow over the others
    ctx = context(partls, monkeypatch, {"PARTLS_CHAIN_LEN": "64"})
    try:
        ctx.opt_prepare(ref["X"], ref["y"], ref["P"], 0.0, FAITHFUL)
        assert ctx.bit_order()[0].tolist() == list(range(K + 1))
        upto = []
        for g in range(1, 14):
            assert ctx.opt_sweep(0, g)[3] == 0
            upto.append(ctx.pivots())
    finally:
        ctx.close()
    steps = np.diff(upto)                                               # steps[g - 1] = pivots of pattern g in that chain
    print("[merged scan] null n=%d: pivots of patterns 1..12 of one chain %s" % (n, steps.tolist()))
    for g in range(1, 13):
        assert (steps[g - 1] == 0) == (g % 4 != 0), (g, steps.tolist())
    np.testing.assert_allclose(got["all"], got["all"][pats & ~dead], rtol=TOL_WALKS)
    # chain starts dominating: the confirming scan of a chain's last pattern must not leak into the next chain
    for cl in ("1", "2", "3"):
        check("null n=%d chain %s" % (n, cl), ref, sweep(partls, monkeypatch, ref["X"], ref["y"], ref["P"], env={"PARTLS_CHAIN_LEN": cl}))


@pytest.mark.parametrize("n", SIZES)
def test_duplicated_columns_in_different_groups(partls, oracle, monkeypatch, n):
    ref = reference(oracle, partls, monkeypatch, "dup", n)
    got = sweep(partls, monkeypatch, ref["X"], ref["y"], ref["P"], expect_route=route(n))
    check("dup n=%d" % n, ref, got)
    check("dup n=%d chain 7" % n, ref, sweep(partls, monkeypatch, ref["X"], ref["y"], ref["P"], env={"PARTLS_CHAIN_LEN": "7"}))


@pytest.mark.parametrize("n", SIZES)
def test_chain_boundaries(partls, oracle, monkeypatch, n):
    """the same problem cut into chains of 1, 2, 3, 7 and the default length, and into sub-ranges with odd ends"""
    ref = reference(oracle, partls, monkeypatch, "plain", n)
    X, y, P = ref["X"], ref["y"], ref["P"]
    base = sweep(partls, monkeypatch, X, y, P, expect_route=route(n))
    check("plain n=%d" % n, ref, base)
    npat = len(ref["objs"])
    walks = [("chain %s" % cl, dict(env={"PARTLS_CHAIN_LEN": cl})) for cl in ("1", "2", "3", "7")]
    walks.append(("odd ranges", dict(ranges=[(0, 1), (1, 22), (22, 23), (23, 47), (47, npat)])))
    walks.append(("odd ranges, chain 3", dict(env={"PARTLS_CHAIN_LEN": "3"}, ranges=[(0, 5), (5, 31), (31, npat)])))
    for name, kw in walks:
        got = sweep(partls, monkeypatch, X, y, P, **kw)
        check("plain n=%d %s" % (n, name), ref, got)
        assert got["pat"] == base["pat"], name
        np.testing.assert_allclose(got["all"], base["all"], rtol=TOL_WALKS, err_msg=name)


def test_faithful_overlapping_partition(partls, oracle, monkeypatch):
    """|f| = 2 (a feature of two groups whose signs agree), f = 0 (they disagree, or a feature of no group): n = 48"""
    ref = reference(oracle, partls, monkeypatch, "overlap", 48)
    assert ref["P"].sum(axis=1).max() == 2 and ref["P"].sum(axis=1).min() == 0
    check("overlap n=48", ref, sweep(partls, monkeypatch, ref["X"], ref["y"], ref["P"], expect_route=route(48)))
    check("overlap n=48 chain 3", ref, sweep(partls, monkeypatch, ref["X"], ref["y"], ref["P"], env={"PARTLS_CHAIN_LEN": "3"}))


def counts(partls, monkeypatch):
    """the decision counters of COUNT_CASES: what tests/golden/merged_scan_counts.json stores"""
    out = []
    for kind, n, seed, flags in COUNT_CASES:
        X, y, P, _ = problem(kind, n, seed, flags)
        for cl in (None, "7"):
            got = sweep(partls, monkeypatch, X, y, P, flags=flags, env={"PARTLS_CHAIN_LEN": cl} if cl else None, expect_route=route(n))
            out.append(dict(kind=kind, n=n, seed=seed, flags=flags, chain_len=cl or "default", shape=[int(X.shape[0]), int(X.shape[1]), K],
                            pivots=got["pivots"], vetoes=got["vetoes"], best_index=got["pat"]))
    return out


def test_decisions_are_those_of_the_kernel_before(partls, monkeypatch):
    with open(GOLDEN) as fh:
        golden = json.load(fh)["counts"]
    got = counts(partls, monkeypatch)
    for g, c in zip(golden, got):
        print("[merged scan] counts %s" % json.dumps(c))
    assert got == golden
