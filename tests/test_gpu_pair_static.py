"""The pair walk's static pricing column (csrc/sweep_blk.hip, PAIR; host: pair_relayout in csrc/sweep_setup.hip): once the bit
order is known the host moves the live variables of the group on Gray bit 0 into ONE tile column (T - 2, which is full at every n of
its tile count) and the kernel prices every twin from that column's fixed tile slots — all 16 columns gathered, the violator mask taken
from the column's 16 rhs entries.  Context.perm stays the one map from tableau index to feature, so everything behind the sweep
(best_sol and the finish, the model export, top-k) must come out right through it.

Shapes: the 512-thread kernel, T = 11 (n = 161 .. 176) and T = 16 (n = 250, 256); N = 3 D rows, K = 5 groups (64 patterns faithful, 32
fitted); PARTLS_PAIR=1 on the test's own contexts (inherited knobs cleared as tests/test_gpu_pair.py does), PARTLS_CHAIN_LEN = 16 and 7.
The bit order.  all_opt exists in faithful mode only, and there the calibration may give bit 0 to the intercept's group of ONE variable
instead (it does on the first problem below when that is calibrated; test_calibrated_order_faithful takes whichever of the two it gets).  So the faithful cases — every pattern's objective against the
oracle — run under PARTLS_BIT_ORDER=identity with the decoupled group `g` = 0 of `live` live (+ `dead` all-zero) columns on bit 0, and the
fitted cases run under PARTLS_BIT_ORDER=calibrate, where that group is the cheapest by far and takes bit 0 wherever it sits — asserted
in both.  Where it sits BEFORE the relayout is computed here from the prepare's rule (stable sort on the
lowest group): first, middle, last, straddling two tile columns.

Every case: all_opt (faithful) against the oracle at |opt - ref| <= 1e-9 max(1, ref), the winner equal to the oracle's (fitted: to the
PARTLS_PAIR=0 walk's, objective against the oracle's), the finish on the winner against oracle.fit_opt at atol 1e-7, unconverged == 0,
and pivots() strictly below the PARTLS_PAIR=0 walk's: twins were priced.  The tolerances are those of tests/test_gpu_pair.py
(TOL_OBJ, TOL_WALKS) and tests/test_gpu_pair_routes.py (ATOL_MODEL)."""
import numpy as np
import pytest

from test_gpu_pair import FAITHFUL, REG_512, TOL_OBJ, TOL_WALKS, context, problem as pair_problem

pytestmark = pytest.mark.gpu

ATOL_MODEL = 1e-7
K = 5
COUPLING = 0.01
CHAINS = ("16", "7")


def make(n, flags, g, live, dead=0, dead_inside=False, seed=0):
    """(X, y, P): K groups, group g = `live` decoupled features that all carry signal + `dead` all-zero columns (before the live ones in
    feature order, or — dead_inside — between them)"""
    D = n - 1 if flags & FAITHFUL else n
    N = 3 * D
    rng = np.random.default_rng(20263000 + 1000 * n + 100 * g + 10 * live + dead + 7 * seed + (flags & FAITHFUL))
    X = rng.standard_normal((N, D))
    others = [k for k in range(K) if k != g]
    grp = np.asarray(others)[rng.integers(0, K - 1, D)]
    grp[rng.choice(D, K - 1, replace=False)] = others                     # each of those groups has a feature
    cand = np.flatnonzero(np.bincount(grp, minlength=K)[grp] > 1)
    gs = np.sort(rng.choice(cand, live + dead, replace=False))
    grp[gs] = g
    assert all((grp == k).any() for k in range(K))
    zero = gs[1:1 + dead] if dead_inside else gs[:dead]
    lv = np.setdiff1d(gs, zero)
    w = rng.standard_normal(D) * (rng.random(D) < 0.6)
    w[lv] = rng.choice([-1.0, 1.0], live) * (0.5 + rng.random(live))
    oth = np.flatnonzero(grp != g)
    Q, _ = np.linalg.qr(np.column_stack([X[:, oth], np.ones(N)]))
    X[:, lv] += (COUPLING - 1.0) * (Q @ (Q.T @ X[:, lv]))                 # as tests/test_gpu_pair.py: most twins are then priced
    X[:, zero] = 0.0
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    y = X @ w + 0.4 + 0.3 * rng.standard_normal(N)
    return np.asfortranarray(X), y, np.asfortranarray(P)


def positions(X, P, g):
    """tableau indices, BEFORE any relayout, of the live features of group g: the prepare sorts the features stably by lowest group"""
    P = np.asarray(P)
    low = np.array([int(np.flatnonzero(r)[0]) if r.any() else 64 for r in P])
    order = np.argsort(low, kind="stable")
    return [int(i) for i, m in enumerate(order) if P[m, g] and np.asarray(X)[:, m].any()]


def bit_order_of(flags):
    """PARTLS_BIT_ORDER of a case: see the module docstring"""
    return "identity" if flags & FAITHFUL else "calibrate"


def run(partls, monkeypatch, X, y, P, flags, pair, chain="16", g=None, order=None):
    """one enumeration on a context of its own: dict(obj, pat, all, pivots, order, fin); g: the group expected on bit 0"""
    n = X.shape[1] + (1 if flags & FAITHFUL else 0)
    ctx = context(partls, monkeypatch, {"PARTLS_PAIR": "1" if pair else "0", "PARTLS_BIT_ORDER": order or bit_order_of(flags),
                                        "PARTLS_CHAIN_LEN": chain})
    try:
        ctx.opt_prepare(X, y, P, 0.0, flags)
        assert ctx.sweep_route() == (REG_512, (n + 15) // 16), ctx.sweep_route()
        order = ctx.bit_order()[0].tolist()
        if g is not None:
            assert order[g] == 0, "the calibration put group %d on bit 0, not group %d: %s" % (order.index(0), g, order)
        bo, bp, allo, unconv = ctx.opt_sweep(0, ctx.num_patterns(), want_all=bool(flags & FAITHFUL))
        assert unconv == 0
        piv = ctx.pivots()
        ctx.tolerate_ill = True
        a, b, t, fo, fidx = ctx.opt_finish(bp)
        return dict(obj=bo, pat=bp, all=allo, pivots=piv, order=order, fin=dict(alpha=a, beta=b, t=t, opt=fo, index=fidx))
    finally:
        ctx.close()


def check_case(partls, oracle, monkeypatch, tag, X, y, P, flags, g, expect_walk=True, order=None):
    ref = oracle.fit_opt(X, y, P, return_all=True)
    objs = ref["all_opt"]
    off = run(partls, monkeypatch, X, y, P, flags, pair=False, g=g, order=order)
    out = None
    for chain in CHAINS:
        got = run(partls, monkeypatch, X, y, P, flags, pair=True, chain=chain, g=g, order=order)
        print("[pair static] %s chain %s: %d pivots (PARTLS_PAIR=0, chain 16: %d); winner %d (oracle %d), objective %.17g (%.17g)" % (
            tag, chain, got["pivots"], off["pivots"], got["pat"], ref["best_index"], got["obj"], ref["opt"]))
        if flags & FAITHFUL:
            err = np.abs(got["all"] - objs) / np.maximum(1.0, np.abs(objs))
            print("[pair static] %s chain %s: max error of all_opt %.3g" % (tag, chain, err.max()))
            assert np.all(np.abs(got["all"] - objs) <= TOL_OBJ * np.maximum(1.0, np.abs(objs))), err.max()
            assert got["pat"] == ref["best_index"]
            assert got["obj"] == got["all"][got["pat"]]
        else:                                                   # fitted intercept: the smaller of the pattern's two intercept signs
            wref = min(objs[got["pat"]], objs[got["pat"] | (1 << K)])
            assert abs(got["obj"] - wref) <= TOL_OBJ * max(1.0, wref) and abs(wref - ref["opt"]) <= TOL_OBJ * max(1.0, ref["opt"])
        assert got["pat"] == off["pat"]
        assert abs(got["obj"] - off["obj"]) <= TOL_WALKS * max(1.0, off["obj"])
        fin = got["fin"]
        assert fin["index"] == off["fin"]["index"]
        if flags & FAITHFUL:
            assert fin["index"] == ref["best_index"]
        assert abs(fin["opt"] - ref["opt"]) <= TOL_OBJ * max(1.0, ref["opt"])
        np.testing.assert_allclose(fin["alpha"], ref["alpha"], atol=ATOL_MODEL)
        np.testing.assert_allclose(fin["beta"], ref["beta"], atol=ATOL_MODEL)
        np.testing.assert_allclose(fin["t"], ref["t"], atol=ATOL_MODEL)
        if chain == "16":
            if expect_walk:
                assert got["pivots"] < off["pivots"], (got["pivots"], off["pivots"])       # the witness that twins were priced
            out = got
    return off, out


# (tag, n, flags, group on bit 0, live, dead, dead inside the group, property of the live variables' positions before the relayout)
T11 = 16 * 9                                                 # first tableau index of the pair column at T = 11
CASES = (
    ("a: 12 live, first", 161, FAITHFUL, 0, 12, 0, False, lambda p, n: p[0] == 0),
    ("a: 13 live, first", 170, FAITHFUL, 0, 13, 0, False, lambda p, n: p[0] == 0),
    ("a: 13 live, middle, fitted", 170, 0, 2, 13, 0, False, lambda p, n: p[0] > 16 and p[-1] < n - 17),
    ("a: 16 live, first", 176, FAITHFUL, 0, 16, 0, False, lambda p, n: p == list(range(16))),
    ("b: 12 live, first, fitted", 176, 0, 0, 12, 0, False, lambda p, n: p[0] == 0),
    ("b: 12 live, last, fitted", 176, 0, K - 1, 12, 0, False, lambda p, n: p == list(range(n - 12, n))),
    ("b: 12 live, middle, fitted", 176, 0, 2, 12, 0, False, lambda p, n: p[0] > 16 and p[-1] < n - 17),
    ("c: 12 live behind 10 all-zero columns: two tile columns", 176, FAITHFUL, 0, 12, 10, False, lambda p, n: p == list(range(10, 22))),
    ("d: n = 256", 256, FAITHFUL, 0, 12, 0, False, lambda p, n: p[0] == 0),
    ("d: n = 250, fitted", 250, 0, 2, 12, 0, False, lambda p, n: p[0] > 16 and p[-1] < n - 17),
    ("e: an all-zero column inside the group", 176, FAITHFUL, 0, 12, 1, True, lambda p, n: p == [0] + list(range(2, 13))),
)


@pytest.mark.parametrize("tag,n,flags,g,live,dead,inside,where", CASES, ids=[c[0] for c in CASES])
def test_static_column(partls, oracle, monkeypatch, tag, n, flags, g, live, dead, inside, where):
    X, y, P = make(n, flags, g, live, dead, inside)
    pos = positions(X, P, g)
    assert len(pos) == live and where(pos, n), pos
    check_case(partls, oracle, monkeypatch, tag, X, y, P, flags, g)


def test_calibrated_order_faithful(partls, oracle, monkeypatch):
    """faithful mode under the calibrated order: bit 0 goes to the decoupled group or to the intercept's group of one variable (then the
    pair column holds the intercept and |C| <= 1) — either way a group that fits the column, every pattern's objective is checked
    under a permuted bit order, and twins are priced"""
    X, y, P = make(176, FAITHFUL, 0, 12, seed=2)
    _, got = check_case(partls, oracle, monkeypatch, "calibrated, faithful", X, y, P, FAITHFUL, None, order="calibrate")
    print("[pair static] calibrated, faithful: order %s" % got["order"])
    assert got["order"].index(0) in (0, K) and got["order"] != list(range(K + 1)), got["order"]


def test_group_of_17_keeps_the_layout(partls, oracle, monkeypatch):
    """17 live variables do not fit one tile column: the walk is off even when forced and nothing is laid out again — the sweep IS the
    PARTLS_PAIR=0 sweep: the same pivots and the same objectives bit for bit (a relayout changes the pivot order and with it last bits)"""
    X, y, P = make(176, FAITHFUL, 0, 17)
    off, got = check_case(partls, oracle, monkeypatch, "g: 17 live", X, y, P, FAITHFUL, 0, expect_walk=False)
    assert got["pivots"] == off["pivots"], (got["pivots"], off["pivots"])
    assert np.array_equal(got["all"], off["all"])
    assert got["obj"] == off["obj"]
    for k in ("alpha", "beta", "t"):
        assert np.array_equal(got["fin"][k], off["fin"][k]), k


@pytest.mark.parametrize("n", (176, 256))
def test_guarded_twins(partls, oracle, monkeypatch, n):
    """f: the `dup` problems of tests/test_gpu_pair.py (two features of group 0 are copies of each other; K = 6, group 0 on bit 0).  Every pair [g, g + 2), g even, is swept alone and
    against [g, g + 1): equal pivots — the twin was priced (or C was empty); more — it took the ordinary rounds.  Both kinds must occur
    and every objective is the oracle's."""
    X, y, P = pair_problem("dup", n, FAITHFUL)
    Xo, Po = oracle.homogeneous(X, P)
    R, z = oracle.compress(Xo, y)
    npat = 1 << (np.asarray(P).shape[1] + 1)
    objs = oracle.opt_patterns(R, z, Po, np.arange(npat))
    ctx = context(partls, monkeypatch, {"PARTLS_PAIR": "1", "PARTLS_BIT_ORDER": "identity", "PARTLS_CHAIN_LEN": "16"})
    try:
        ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
        assert ctx.sweep_route() == (REG_512, n // 16)
        assert ctx.bit_order()[0][0] == 0
        priced = rounds = 0
        worst = 0.0
        for g in range(0, npat, 2):
            _, _, part, unconv = ctx.opt_sweep(g, g + 2, want_all=True)
            both = ctx.pivots()
            assert unconv == 0
            seen = np.flatnonzero(~np.isnan(part))
            assert sorted(seen.tolist()) == sorted([g ^ (g >> 1), (g + 1) ^ ((g + 1) >> 1)])
            worst = max(worst, float(np.max(np.abs(part[seen] - objs[seen]) / np.maximum(1.0, objs[seen]))))
            assert np.all(np.abs(part[seen] - objs[seen]) <= TOL_OBJ * np.maximum(1.0, objs[seen]))
            assert ctx.opt_sweep(g, g + 1)[3] == 0
            first = ctx.pivots()
            assert both >= first
            priced += both == first
            rounds += both > first
        print("[pair static] dup n=%d: %d twins priced, %d by the ordinary rounds; max error %.3g" % (n, priced, rounds, worst))
        assert priced >= 1 and rounds >= 1, (priced, rounds)
        bo, bp, allo, unconv = ctx.opt_sweep(0, npat, want_all=True)
        assert unconv == 0 and bp == int(np.argmin(objs))
        assert np.all(np.abs(allo - objs) <= TOL_OBJ * np.maximum(1.0, objs))
    finally:
        ctx.close()


def test_perm_round_trip(partls, oracle, monkeypatch):
    """h: the model export, the k best patterns and the finish on a context that was laid out again against the same calls under PARTLS_PAIR=0"""
    X, y, P = make(176, FAITHFUL, 0, 12, seed=1)
    res = {}
    for pair in (True, False):
        ctx = context(partls, monkeypatch, {"PARTLS_PAIR": "1" if pair else "0", "PARTLS_BIT_ORDER": "identity", "PARTLS_CHAIN_LEN": "16"})
        try:
            ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
            assert ctx.bit_order()[0][0] == 0
            bo, bp, allo, unconv = ctx.opt_sweep(0, ctx.num_patterns(), want_all=True)
            assert unconv == 0
            piv = ctx.pivots()
            m = ctx.opt_models()
            top = ctx.opt_top(3)
            fin = ctx.opt_finish(bp)
            res[pair] = dict(pat=bp, all=allo, pivots=piv, m=m, top=top, fin=fin)
        finally:
            ctx.close()
    on, off = res[True], res[False]
    assert on["pivots"] < off["pivots"], (on["pivots"], off["pivots"])                       # the context was laid out again and walked in pairs
    assert on["pat"] == off["pat"]
    assert on["m"]["n_unconverged"] == 0 and off["m"]["n_unconverged"] == 0
    assert np.array_equal(on["m"]["pattern"], off["m"]["pattern"])
    np.testing.assert_allclose(on["m"]["opt"], off["m"]["opt"], rtol=TOL_WALKS)
    np.testing.assert_allclose(on["m"]["opt"], on["all"][on["m"]["pattern"]], rtol=TOL_WALKS)
    for k in ("alpha", "beta", "t"):
        np.testing.assert_allclose(on["m"][k], off["m"][k], atol=ATOL_MODEL, err_msg="opt_models " + k)
        np.testing.assert_allclose(on["top"][k], off["top"][k], atol=ATOL_MODEL, err_msg="opt_top " + k)
    assert np.array_equal(on["top"]["pattern"], off["top"]["pattern"]) and on["top"]["pattern"][0] == on["pat"]
    np.testing.assert_allclose(on["top"]["opt"], off["top"]["opt"], rtol=TOL_WALKS)
    ref = oracle.fit_opt(X, y, P)
    for got in (on["fin"], off["fin"]):
        a, b, t, fo, fidx = got
        assert fidx == ref["best_index"] and abs(fo - ref["opt"]) <= TOL_OBJ * max(1.0, ref["opt"])
        np.testing.assert_allclose(a, ref["alpha"], atol=ATOL_MODEL)
        np.testing.assert_allclose(b, ref["beta"], atol=ATOL_MODEL)
        np.testing.assert_allclose(t, ref["t"], atol=ATOL_MODEL)
