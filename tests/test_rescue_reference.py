"""The rescue rule (tests/rescue_reference.py: Lawson-Hanson on the scaled tableau) on the CPU, against the dense NNLS oracle.

On every design the rescue is built for — the chain cases of exchange_reference, the Gray indices 17..24 of c297, the design that is
correlated throughout and c40 with a duplicated and a scaled column inside a group — every pattern, solved from
the empty basis, ends with no KKT violator under the sweeps' own kkt_violates, within 3 n main passes, at the oracle's optimum within
TOL_OBJ.  A bound of one main pass leaves patterns unsolved, which is what PARTLS_RESCUE_MAX_PASSES = 1 forces in the GPU tests.
"""
import numpy as np
import pytest

import exchange_reference as E
import rescue_reference as R
from test_exchange_reference import oracle_objectives

TOL_OBJ = 1e-9                                              # tests/test_gpu_opt.py
_SOLVED = {}


def solved(name):
    if name not in _SOLVED:
        c = R.case(name)
        pr = E.prepare(c["X"], c["y"], c["P"], c["eta"], c["faithful"])
        pats = R.case_patterns(name)
        _SOLVED[name] = dict(case=c, pr=pr, pats=pats, res=R.solve(pr, pats))
    return _SOLVED[name]


@pytest.mark.parametrize("name", R.CASES)
def test_every_pattern_is_solved(oracle, name):
    s = solved(name)
    c, pr, pats, res = s["case"], s["pr"], s["pats"], s["res"]
    n = pr["n"]
    want = oracle_objectives(oracle, c, pats)
    err = np.abs(res["obj"] - want) / np.maximum(1.0, want)
    print("[rescue] %s, n = %d: %d patterns, main passes max %d (bound %d), pivots max %d, vetoes %d, objective off by at most %.3g" % (
        name, n, len(pats), res["passes"].max(), R.default_max_passes(n), res["pivots"].max(), res["vetoes"].sum(), err.max()))
    assert res["solved"].all() and res["clean"].all(), "unsolved: %s" % pats[~(res["solved"] & res["clean"])].tolist()
    assert res["passes"].max() <= R.default_max_passes(n)
    assert np.all(np.abs(res["obj"] - want) <= TOL_OBJ * np.maximum(1.0, want)), "max error %.3g" % err.max()
    # the solution row carries the pattern's signs and is 0 where the pattern asks for 0
    for p, sol in zip(pats, res["sol"]):
        f = E.signs(pr, int(p))
        assert np.all(sol * np.sign(f) >= 0) and np.all(sol[f == 0] == 0)


@pytest.mark.parametrize("name", ("c40", "c176"))
def test_one_main_pass_leaves_patterns_unsolved(name):
    s = solved(name)
    res = R.solve(s["pr"], s["pats"], max_passes=1)
    assert not res["solved"].any(), "a pattern of %s needs one main pass only" % name
    assert np.isnan(res["obj"]).all() and np.isnan(res["sol"]).all() and (res["passes"] == 1).all()


def test_a_bound_at_the_need_is_met():
    """the bound counts main passes as the kernel does: exactly the passes a pattern takes are enough, one less is not"""
    s = solved("c40")
    need = int(s["res"]["passes"][5])
    assert R.solve(s["pr"], s["pats"][5:6], max_passes=need)["solved"][0]
    assert not R.solve(s["pr"], s["pats"][5:6], max_passes=need - 1)["solved"][0]
