"""The cases of tests/exchange_reference.py, checked on the reference alone (no GPU): they reach the backup rule and the pivot cap, they
are far from every tolerance, and they tell the true ExchangeRule (csrc/sweep_rules.h) from each of its plausible miscopies.
tests/test_gpu_exchange_rule.py then compares the kernels with the float64 emulation decision for decision; everything that comparison
relies on is asserted here, so that it cannot be lost silently.  No case is skipped or filtered at run time.

For every case (chain cases: all 64 patterns in chains of 7 under the default cap; c297: the Gray indices 17..24; node cases: one node):
  no rejection          no entering pivot with d <= piv_eps = 1e-11, and the smallest |d| pivoted on is at least 1e-6;
  objectives            every converged pattern's objective equals the oracle's dense NNLS optimum to 1e-12 relative (free intercept:
                        the smaller of the oracle's two intercept signs; nodes: bnb_reference.NodeReference, certified);
  one trajectory        the float64 and the long-double run have the same violator set in every round;
  decision margin       the smallest distance of a tested |q| from tol is at least 1000 x the largest |q_float64 - q_longdouble| of any
                        scan of that trajectory (the drift: between the two reference runs, never against the device) and 1000 x tol;
  coverage, discrimination   see the tests.

Measured (drift = max |q_float64 - q_longdouble|; margin = smallest | |q| - tol |; objective error relative to the oracle):
  case          patterns with backup steps  backup steps  pivots  most rounds  tol      drift    margin   smallest |d|  objective error
  c40           33 of 64                    660           5301    193          1.7e-09  3.1e-10  9.2e-05  1.2e-03       7.5e-14
  c72-eta       41 of 64                    1732          9823    238          2.7e-09  4.2e-10  8.4e-05  5.9e-04       9.2e-14
  c176          27 of 64                    1533          13838   327          3.8e-09  3.1e-10  6.1e-05  1.5e-03       9.3e-14
  c40-free      34 of 64                    877           5825    122          1.0e-09  1.8e-10  9.6e-05  9.2e-04       3.3e-14
  c72-overlap   26 of 64                    582           6477    97           2.7e-09  2.4e-10  4.2e-05  1.2e-03       4.2e-14
  c297 (8)      5 of 8                      312           2560    158          5.7e-09  2.7e-10  1.4e-05  1.1e-03       1.1e-14
  node          rounds  backup steps  pivots  tol      drift    margin   smallest |d|  objective error
  n40           25      15            74      6.4e-10  1.6e-11  1.1e-02  3.8e-03       8.0e-16
  n72           18      6             102     1.9e-09  1.2e-10  1.4e-03  1.6e-03       2.3e-15
  n176          49      27            412     2.8e-09  8.7e-11  5.9e-03  3.1e-03       1.7e-15
  n297          23      9             286     3.5e-09  2.0e-11  7.3e-04  3.0e-03       1.2e-15
  n331          36      15            542     4.5e-09  2.5e-10  5.0e-04  2.2e-03       1.9e-15
(the test prints the figures of every case; the drift is that of thousands of pivots on |d| down to 1e-3, and still five orders of
magnitude below the margin).
Patterns capped under PARTLS_MAX_ROUNDS = 1, 2, 3, 4, 6, 10, 40 (chains of 7): c40 64 64 62 58 48 32 8, c72-eta 64 64 61 58 51 42 21,
c176 64 64 64 60 47 28 18, c40-free 64 63 64 62 54 41 12, c72-overlap 64 63 63 60 45 25 10.
Smallest margin over every walk the GPU tests compare with (chains of 7 and 64, whole range and Gray indices 5..26, every cap):
c40 9.2e-05, c72-eta 3.6e-05, c176 1.6e-05, c40-free 2.3e-05, c72-overlap 5.7e-06 (1000 x tol = 2.7e-06).
"""
import numpy as np
import pytest

import exchange_reference as E
from bnb_reference import NodeReference

CHAINS = list(E.CHAIN_CASES)
NODES = list(E.NODE_CASES)
TOL_ORACLE = 1e-12
_CACHE = {}


def oracle_objectives(oracle, case, patterns):
    """the dense NNLS optimum of the listed patterns (free intercept: the better of the two intercept signs)"""
    Xo, Po = oracle.homogeneous(case["X"], case["P"])
    Xn, yn = oracle.regularize(Xo, case["y"], Po, case["eta"])
    R, z = oracle.compress(Xn, yn)
    pats = np.asarray(patterns, dtype=np.int64)
    if case["faithful"]:
        return oracle.opt_patterns(R, z, Po, pats)
    return np.minimum(oracle.opt_patterns(R, z, Po, pats), oracle.opt_patterns(R, z, Po, pats | (1 << case["K"])))


def chain_runs(name):
    """the float64 and the long-double walk of a chain case under the default cap, and the float64 walks under CAPS: once per case"""
    if name not in _CACHE:
        c = E.chain_case(name)
        g0, g1 = E.RANGE_297 if name == E.RANGE_CASE[0] else (0, 64)
        pr = E.prepare(c["X"], c["y"], c["P"], c["eta"], c["faithful"])
        prl = E.prepare(c["X"], c["y"], c["P"], c["eta"], c["faithful"], dtype=np.longdouble)
        assert pr["kbits"] == 6
        _CACHE[name] = dict(case=c, pr=pr, range=(g0, g1), f64=E.walk(pr, g0, g1, E.CHAIN_LEN, keep_q=True),
                            ld=E.walk(prl, g0, g1, E.CHAIN_LEN, keep_q=True),
                            caps={cap: E.walk(pr, g0, g1, E.CHAIN_LEN, cap) for cap in E.CAPS})
    return _CACHE[name]


def node_runs(name):
    if name not in _CACHE:
        c = E.node_case(name)
        ref = NodeReference(c["X"], c["y"], c["P"], c["eta"])
        node = ref.node(c["pat"], c["free"])
        pr = E.prepare(c["X"], c["y"], c["P"], c["eta"])
        prl = E.prepare(c["X"], c["y"], c["P"], c["eta"], dtype=np.longdouble)
        codes = E.tableau_codes(pr, node["codes"])
        _CACHE[name] = dict(case=c, pr=pr, node=node, codes=codes, f64=E.solve(pr, codes, keep_q=True), ld=E.solve(prl, codes, keep_q=True))
    return _CACHE[name]


def check_run(tag, r, rl, ref_obj):
    """the conditions every case meets; prints the figures the module docstring quotes"""
    assert E.same_trajectory(r, rl), "%s: the float64 and the long-double run part ways" % tag
    dr = E.drift(r, rl)
    conv = ~r["capped"]
    err = float(np.max(np.abs(r["obj"][conv] - ref_obj[conv]) / ref_obj[conv]))
    print("[exchange ref] %s: %d of %d patterns take backup steps, %d backup steps, %d pivots, most rounds %d, tol %.2g, drift %.2g, margin %.2g, "
          "smallest |d| %.2g, rejected %d, objective error %.2g" % (tag, int((r["backups"] > 0).sum()), len(r["backups"]), r["backups"].sum(),
                                                                    r["pivots"].sum(), r["rounds"].max(), r["tol"], dr, r["margin"], r["min_d"],
                                                                    r["rejected"], err))
    assert r["rejected"] == 0 and rl["rejected"] == 0, "%s: an entering pivot was rejected (d <= piv_eps)" % tag
    assert r["min_d"] >= 1e-6, "%s: smallest |d| %.3g" % (tag, r["min_d"])
    assert not r["capped"].any(), "%s: a pattern hits the default cap" % tag
    assert err <= TOL_ORACLE, "%s: objective off the oracle's by %.3g" % (tag, err)
    assert r["margin"] >= 1000.0 * dr, "%s: margin %.3g, drift %.3g" % (tag, r["margin"], dr)
    assert r["margin"] >= 1000.0 * r["tol"], "%s: margin %.3g, tol %.3g" % (tag, r["margin"], r["tol"])
    assert min(r["margin"], rl["margin"]) > 0.0


def differs(a, b):
    return int(a["pivots"].sum()) != int(b["pivots"].sum()) or not np.array_equal(a["capped"], b["capped"])


@pytest.mark.parametrize("name", CHAINS)
def test_chain_case(oracle, name):
    runs = chain_runs(name)
    r = runs["f64"]
    check_run(name, r, runs["ld"], oracle_objectives(oracle, runs["case"], r["pattern"]))
    assert int((r["backups"] > 0).sum()) >= 20, "%s: only %d patterns take a backup step" % (name, int((r["backups"] > 0).sum()))
    print("[exchange ref] %s: capped under %s: %s" % (name, E.CAPS, [int(runs["caps"][c]["capped"].sum()) for c in E.CAPS]))
    ref = oracle_objectives(oracle, runs["case"], r["pattern"])
    # every walk the GPU tests compare with (chains of 7 and 64, the whole range and the sub-range, every cap): no rejection, far from
    # the tolerance, and a pattern that converges under a cap has the oracle's optimum, whatever tableau it started from
    worst = np.inf
    for chain_len in E.GPU_CHAIN_LENS:
        for g0, g1 in ((0, 64), E.SUB_RANGE):
            for cap in (None,) + E.CAPS:
                whole7 = chain_len == E.CHAIN_LEN and (g0, g1) == (0, 64)
                rc = (r if cap is None else runs["caps"][cap]) if whole7 else E.walk(runs["pr"], g0, g1, chain_len, cap)
                conv = ~rc["capped"]
                worst = min(worst, rc["margin"])
                assert rc["rejected"] == 0 and rc["min_d"] >= 1e-6 and rc["margin"] >= 1000.0 * rc["tol"], (name, chain_len, g0, cap)
                assert np.all(np.abs(rc["obj"][conv] - ref[rc["g"]][conv]) <= TOL_ORACLE * ref[rc["g"]][conv]), (name, chain_len, g0, cap)
    print("[exchange ref] %s: smallest margin over chains of %s, both ranges and every cap: %.2g" % (name, E.GPU_CHAIN_LENS, worst))


def test_range_case(oracle):
    """the 8 patterns the deferred-update kernel walks at its own size (n = 297)"""
    name = E.RANGE_CASE[0]
    runs = chain_runs(name)
    r = runs["f64"]
    assert runs["pr"]["n"] == 297 and len(r["g"]) == 8
    check_run(name, r, runs["ld"], oracle_objectives(oracle, runs["case"], r["pattern"]))
    assert int((r["backups"] > 0).sum()) >= 3
    caps = [int(runs["caps"][c]["capped"].sum()) for c in E.CAPS]
    print("[exchange ref] %s: capped under %s: %s" % (name, E.CAPS, caps))
    assert 0 < min(caps) and len(set(caps)) >= 4              # the caps cut the range at different patterns


@pytest.mark.parametrize("name", CHAINS)
def test_chain_case_tells_the_rule_from_its_miscopies(name):
    """each mutant changes the total pivot count or the set of capped patterns under at least one cap"""
    runs = chain_runs(name)
    pr, (g0, g1) = runs["pr"], runs["range"]
    for mname, mutant in E.MUTANTS.items():
        found = None
        for cap in E.CAPS:
            if differs(E.walk(pr, g0, g1, E.CHAIN_LEN, cap, rule=mutant), runs["caps"][cap]):
                found = cap
                break
        print("[exchange ref] %s: '%s' differs from the rule under a cap of %s" % (name, mname, found))
        assert found is not None, "%s does not tell '%s' from the rule" % (name, mname)


@pytest.mark.parametrize("name", NODES)
def test_node_case(name):
    """one node from the empty basis: codes -1, 0, +1 and 2; at least one backup step; every mutant changes the pivot count — under the
    default cap or, for the comparison at the cap, under a cap of exactly the node's round count (which the true rule still meets)"""
    runs = node_runs(name)
    r, node, codes, pr = runs["f64"], runs["node"], runs["codes"], runs["pr"]
    assert node["certified"]
    assert set(np.unique(codes).tolist()) == {-1, 0, 1, 2}, "%s: codes %s" % (name, np.unique(codes))
    check_run(name, r, runs["ld"], np.array([node["lb"]]))
    assert r["backups"][0] >= 1, "%s takes no backup step" % name
    rounds = int(r["rounds"][0])
    at_cap = E.solve(pr, codes, rounds)
    assert not at_cap["capped"][0] and at_cap["pivots"][0] == r["pivots"][0]
    assert E.solve(pr, codes, rounds - 1)["capped"][0]
    for mname, mutant in E.MUTANTS.items():
        got = int(E.solve(pr, codes, rounds, rule=mutant)["pivots"][0])          # (a mutant may cycle up to the default cap: asked last)
        if got == int(r["pivots"][0]):
            got = int(E.solve(pr, codes, rule=mutant)["pivots"][0])
        print("[exchange ref] %s: '%s' takes %d pivots, the rule %d (%d rounds)" % (name, mname, got, r["pivots"][0], rounds))
        assert got != int(r["pivots"][0]), "%s does not tell '%s' from the rule" % (name, mname)


def test_coverage_of_the_backup_picks():
    """across the cases the backup step picks an index in tile 0, the index n - 1, an index in a partial last tile and indices on both
    sides of the mask-word boundaries 63/64 and 127/128; and under the caps a pattern that starts from a capped predecessor's tableau
    needs a backup step within its first five rounds"""
    tile0 = last = partial = False
    sides = {63: False, 64: False, 127: False, 128: False}
    after = []
    for name in CHAINS:
        runs = chain_runs(name)
        n = runs["pr"]["n"]
        for r in [runs["f64"]] + list(runs["caps"].values()):
            picks = set(k for p in r["picks"] for k in p)
            tile0 |= any(k < 16 for k in picks)
            last |= (n - 1) in picks
            partial |= n % 16 != 0 and any(k >= 16 * (n // 16) for k in picks)
            for k in sides:
                sides[k] |= k in picks
        for cap, r in runs["caps"].items():
            hits = [int(g) for g, a, br in zip(r["g"], r["after_capped"], r["backup_rounds"]) if a and br and br[0] <= 5]
            if hits:
                after.append((name, cap, hits[:4]))
    for name in NODES:
        r = node_runs(name)["f64"]
        assert r["backups"][0] >= 1
    print("[exchange ref] backup step within five rounds after a capped predecessor (case, cap, Gray indices): %s" % after)
    assert tile0 and last and partial and all(sides.values()), (tile0, last, partial, sides)
    assert after, "no pattern needs a backup step in its first five rounds after a capped predecessor"


def test_rule_order_of_tests():
    """ExchangeRule::next as written: a converged scan is no round, and the patience is spent before the cap is looked at"""
    c = E.chain_case("c40")
    pr = E.prepare(c["X"], c["y"], c["P"], c["eta"], c["faithful"])
    full = E.walk(pr, 0, 8, 8)
    for cap in (1, 2, 3):
        r = E.walk(pr, 0, 8, 8, cap)
        assert r["rounds"].max() <= cap
        # the first pattern of a chain starts from the same tableau whatever the cap: it is capped exactly when it needs more rounds
        assert bool(r["capped"][0]) == (full["rounds"][0] > cap)
    assert not E.walk(pr, 0, 8, 8, int(full["rounds"].max()))["capped"].any()


def test_fit_case_reaches_the_cap():
    """what tests/test_gpu_exchange_rule.py::test_fit_reports_the_cap relies on: c40 with the faithful intercept in the chains of 4 the
    library cuts 64 patterns of a 256-thread problem into (sweep_plan, sweep_setup.hip) caps patterns under PARTLS_MAX_ROUNDS=6"""
    pr = chain_runs("c40")["pr"]
    assert E.walk(pr, 0, 64, 4, 6)["capped"].sum() > 0 and not E.walk(pr, 0, 64, 4)["capped"].any()
