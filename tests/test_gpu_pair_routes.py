"""The pair walk (csrc/sweep_blk.hip, PAIR; host rule sweep_pairs in csrc/sweep_setup.hip) where tests/test_gpu_pair.py does
not reach: every instantiation, the route a caller gets without a knob, and what record_twin leaves behind.  The problems, the
contexts and the checks are that file's (problem, context, sweep, check, reference; TOL_OBJ against the oracle, TOL_WALKS between two
walks of one problem); the finish is held against oracle.fit_opt at atol 1e-7 as in tests/test_gpu_lazy.py.  Every case asserts its
route first.  tools/pair_emul.py walks the problems of A and B on the CPU and fails unless they have the twins they are there for.

  A  every tile count.  The pair walk is one kernel per T = 11 .. 16 (gather_tile, RS, RHSPOS, the twin's row position, pair_solve's
     wave all depend on T): kind `plain` at n = 16 (T - 1) + 1 — the last tile column holds one variable, in faithful mode the
     intercept alone — and n = 16 T, both intercept modes, less the four cases test_gpu_pair.py has.  check() as there, and pivots()
     strictly below the paired-off walk's: twins were priced in every instantiation (the emulation: 21 .. 57 priced, 2 .. 14 hard).
  B  the winner is a priced twin.  In the range [g - 1, g + 1) with g odd the tableau visits Gray index g - 1 and g is its twin; the
     problems are those whose global winner has an odd Gray index and a twin that pricing finishes (mirrored: the columns of group 0
     negated, which exchanges the members of every pair).  pivots() of [g - 1, g + 1) equals that of [g - 1, g) and the two objectives
     differ: the twin was priced with C not empty, so the winner's best_sol is the one record_twin wrote from qt and bt — the finish
     must take it and return the oracle's model.
  C  the route a caller gets: PARTLS_PAIR unset, 18-bit enumerations at n = 176 (K = 17 faithful, K = 18 fitted).  The expected verdict
     is computed here from the documented rule (length rule on K', >= 32 patterns per CU in the range, 12 .. 16 LIVE variables on bit 0,
     T <= 16) with the CU count read from the device; the witness is pivots() against a PARTLS_PAIR=0 context on the same problem:
     exactly equal where the rule says off (the same deterministic kernel), strictly lower where it says on.  Group 0 on bit 0
     (PARTLS_BIT_ORDER=identity) with 12, 16, 17 live features, with all-zero columns beside the live ones, at 17 bits and at T = 17;
     short and long ranges of one problem, the short one bit-equal to partls_opt_models' rows; the calibrated order, whatever group it
     puts on bit 0; and a small forced walk (K = 6, PARTLS_BIT_ORDER=calibrate, PARTLS_PAIR=1) on a problem whose cheapest group is
     not group 0, so that the twin's pattern and the first-reference-index rule run under a permuted order, with exact ties.
  D  near ties: partls_opt_candidates after the pair walk lists what it lists after the paired-off walk (record_twin's runner-up), on
     the two `null` problems and on their mirror images in group 2, where the two walks meet the winner's copies in different orders.
  E  three shards on one device: odd shard boundaries, merged all_opt and winner equal the single context's pair walk."""
import sys

import numpy as np
import pytest

from test_gpu_pair import COUPLING, FAITHFUL, K, REG_512, TOL_OBJ, TOL_WALKS, check, context, problem, reference, sweep

pytestmark = pytest.mark.gpu

ATOL_MODEL = 1e-7                                           # tests/test_gpu_lazy.py: the finish against oracle.fit_opt

# ---- A ---------------------------------------------------------------------------------------------------------------------------
TILE_CASES = tuple((n, flags) for T in range(11, 17) for n in (16 * (T - 1) + 1, 16 * T) for flags in (FAITHFUL, 0)
                   if n not in (176, 256))                  # (plain, 176 | 256, both modes) run in tests/test_gpu_pair.py
# ---- B: (kind, n, mirrored, coupling); winner / Gray index / |C| by oracle and emulation: 104 / 79 / 12, 26 / 19 / 12, 67 / 125 / 9,
# 112 / 95 / 12, 1 / 1 / 12.  At coupling 0.01 the winner's twin of the two plain problems has violators left after the block pivot.
TWIN_CASES = (("straddle", 176, True, COUPLING), ("straddle", 256, False, COUPLING), ("overlap", 256, True, COUPLING),
              ("plain", 176, False, 0.001), ("plain", 256, False, 0.001))


def gray(g):
    return g ^ (g >> 1)


def gray_inverse(p):
    g = 0
    while p:
        g ^= p
        p >>= 1
    return g


def twin_problem(kind, n, mirror, coupling):
    """a problem of B; mirror: the columns of group 0 negated"""
    X, y, P = problem(kind, n, FAITHFUL, coupling=coupling)
    if mirror:
        X = np.array(X, order="F")
        X[:, np.asarray(P)[:, 0] != 0] *= -1.0
    return X, y, P


def route_problem(n, flags, K, live=12, null=0):
    """problem("plain", n, flags, K=K) with group 0 rebuilt to `live` live columns and `null` all-zero ones.  Columns that join group 0
    are taken from groups that keep a feature and are decoupled from the other groups like the 12 it has; all-zero columns are first
    the joined ones, then the first of the original 12."""
    X, y, P = problem("plain", n, flags, K=K)
    X, P = np.array(X, order="F"), np.array(P, order="F")
    N, D = X.shape
    rng = np.random.default_rng(77000 + 100 * (live + null) + null)
    old = np.flatnonzero(P[:, 0])
    assert len(old) == 12
    new = []
    for _ in range(live + null - 12):
        cnt = P.sum(axis=0)
        m = int(rng.choice([m for m in range(D) if P[m, 0] == 0 and cnt[int(np.argmax(P[m]))] > 1]))
        P[m] = 0
        P[m, 0] = 1
        new.append(m)
    assert (P.sum(axis=1) == 1).all() and (P.sum(axis=0) >= 1).all() and P[:, 0].sum() == live + null
    zero = (new + old.tolist())[:len(old) + len(new) - live]
    X[:, zero] = 0.0
    if new:
        Q, _ = np.linalg.qr(np.column_stack([X[:, P[:, 0] == 0], np.ones(N)]))
        X[:, new] += (COUPLING - 1.0) * (Q @ (Q.T @ X[:, new]))
        y = y + X[:, new] @ (rng.choice([-1.0, 1.0], len(new)) * (0.5 + rng.random(len(new))))     # ... and carry signal (the live ones)
    assert sum(bool(X[:, m].any()) for m in np.flatnonzero(P[:, 0])) == live
    return np.asfortranarray(X), y, np.asfortranarray(P)


def swapped(X, y, P, k):
    """the same problem with the names of group 0 and group k exchanged: the decoupled (or all-zero) group is group k"""
    P = np.array(P, order="F")
    P[:, [0, k]] = P[:, [k, 0]]
    return X, y, np.asfortranarray(P)


def oracle_objectives(oracle, X, y, P, flags, pats):
    """optimum of the listed patterns (reference indices): Opt.jl:87-90 on QR-compressed data; with a fitted intercept the smaller of
    the pattern's two intercept signs (include/partls.h)"""
    Xo, Po = oracle.homogeneous(X, P)
    R, z = oracle.compress(Xo, y)
    pats = np.asarray(pats, dtype=np.int64)
    objs = oracle.opt_patterns(R, z, Po, pats)
    if not flags & FAITHFUL:
        objs = np.minimum(objs, oracle.opt_patterns(R, z, Po, pats | (1 << np.asarray(P).shape[1])))
    return objs


def walk(partls, monkeypatch, X, y, P, flags, env, ranges=None, capfd=None, identity=True, cands=False, models=None):
    """test_gpu_pair.sweep with the knobs, the bit order and the range left to the caller: the route asserted, then one opt_sweep per
    range on one context — dict(obj, pat, all, pivots) of the LAST range, `runs` of every range, order, and on request cand
    (opt_candidates), models (opt_models of that Gray range) and fin (the finish on the last range's winner, with its trace)"""
    n = X.shape[1] + (1 if flags & FAITHFUL else 0)
    knobs = dict(env)
    if capfd is not None:
        knobs["PARTLS_FINISH_TRACE"] = "1"
    ctx = context(partls, monkeypatch, knobs)
    try:
        ctx.opt_prepare(X, y, P, 0.0, flags)
        assert ctx.sweep_route() == (REG_512, (n + 15) // 16), ctx.sweep_route()
        order = ctx.bit_order()[0].tolist()
        if identity:
            assert order == list(range(len(order))), order
        npat = ctx.num_patterns()
        runs = []
        for lo, hi in ranges or [(0, npat)]:
            bo, bp, part, unconv = ctx.opt_sweep(lo, hi, want_all=bool(flags & FAITHFUL))
            assert unconv == 0, "%d patterns hit the pivot cap in [%d, %d)" % (unconv, lo, hi)
            runs.append(dict(obj=bo, pat=bp, all=part, pivots=ctx.pivots()))
        out = dict(runs[-1], runs=runs, order=order, npat=npat, fin=None)
        if cands:
            out["cand"] = ctx.opt_candidates()
        if models is not None:
            out["models"] = ctx.opt_models(*models)
        if capfd is not None:
            sys.stdout.write(capfd.readouterr().out)
            a, b, t, fo, fidx = ctx.opt_finish(out["pat"])
            err = capfd.readouterr().err
            assert "the sweep's solution of its winner" in err, err
            out["fin"] = dict(alpha=a, beta=b, t=t, opt=fo, index=fidx, taken="): taken" in err)
        return out
    finally:
        ctx.close()


def forced(pair, **more):
    return dict({"PARTLS_PAIR": "1" if pair else "0", "PARTLS_REG_MAXT": "18"}, **more)


# ---- A: every tile count, both edge sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,flags", TILE_CASES)
def test_every_tile_count(partls, oracle, monkeypatch, capfd, n, flags):
    ref = reference(oracle, partls, monkeypatch, capfd, "plain", n, flags)
    got = sweep(partls, monkeypatch, ref["X"], ref["y"], ref["P"], flags, pair=True, capfd=capfd)      # asserts (REG_512, T)
    check("plain n=%d (T=%d) %s" % (n, (n + 15) // 16, "faithful" if flags else "fitted"), ref, got)
    assert got["pivots"] < ref["off"]["pivots"], (got["pivots"], ref["off"]["pivots"])                 # twins were priced at this T


# ---- B: the winner is a priced twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,mirror,coupling", TWIN_CASES)
def test_winner_is_a_priced_twin(partls, oracle, monkeypatch, capfd, kind, n, mirror, coupling):
    X, y, P = twin_problem(kind, n, mirror, coupling)
    ref = oracle.fit_opt(X, y, P, return_all=True)
    objs = ref["all_opt"]
    w = int(np.argmin(objs))
    g = gray_inverse(w)
    assert w == ref["best_index"] and g & 1, "the oracle's winner %d has Gray index %d: it is no twin of a two-pattern range" % (w, g)
    on = walk(partls, monkeypatch, X, y, P, FAITHFUL, forced(True), ranges=[(g - 1, g + 1)], capfd=capfd)
    first = walk(partls, monkeypatch, X, y, P, FAITHFUL, forced(True), ranges=[(g - 1, g)])
    off = walk(partls, monkeypatch, X, y, P, FAITHFUL, forced(False), ranges=[(g - 1, g + 1)], capfd=capfd)
    fin, fof = on["fin"], off["fin"]
    print("[pair routes] %s n=%d%s: winner %d = gray(%d); pivots of [g-1, g+1) %d, of [g-1, g) %d, paired off %d; objectives %.17g (twin) "
          "%.17g (visited), oracle %.17g; best_sol taken %s (paired off: %s); finish opt %.17g (paired off %.17g, oracle %.17g)" % (
              kind, n, " mirrored" if mirror else "", w, g, on["pivots"], first["pivots"], off["pivots"], on["all"][w], on["all"][gray(g - 1)],
              objs[w], fin["taken"], fof["taken"], fin["opt"], fof["opt"], ref["opt"]))
    assert first["pat"] == gray(g - 1)
    assert on["pivots"] == first["pivots"], (on["pivots"], first["pivots"])                     # nothing was pivoted for the twin ...
    assert on["all"][w] != on["all"][gray(g - 1)]                                               # ... and C was not empty
    assert np.isnan(on["all"]).sum() == len(objs) - 2
    assert on["pat"] == w
    assert abs(on["obj"] - objs[w]) <= TOL_OBJ * max(1.0, objs[w]) and on["obj"] == on["all"][w]
    assert abs(on["all"][gray(g - 1)] - objs[gray(g - 1)]) <= TOL_OBJ * max(1.0, objs[gray(g - 1)])
    assert fin["taken"], "the finish refused the best_sol record_twin wrote"
    assert fin["index"] == w
    assert abs(fin["opt"] - ref["opt"]) <= TOL_OBJ * max(1.0, ref["opt"])
    np.testing.assert_allclose(fin["alpha"], ref["alpha"], atol=ATOL_MODEL)
    np.testing.assert_allclose(fin["beta"], ref["beta"], atol=ATOL_MODEL)
    np.testing.assert_allclose(fin["t"], ref["t"], atol=ATOL_MODEL)
    assert off["pat"] == w and fof["index"] == fin["index"]
    assert abs(fin["opt"] - fof["opt"]) <= TOL_WALKS * max(1.0, fof["opt"])
    assert off["pivots"] > on["pivots"], (off["pivots"], on["pivots"])


# ---- C: the route users get --------------------------------------------------------------------------------------------------------
def cu_count():
    import torch                                            # (as tests/test_gpu_bnb_nodes.py reads it; the first import in a process takes seconds)
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def live_on_bit0(X, P, flags, order):
    """live variables of the group that `order` (gbit[k] = Gray bit of group k) puts on bit 0"""
    k = order.index(0)
    P = np.asarray(P)
    if k == P.shape[1]:
        return 1                                            # faithful mode's last group: the intercept
    return sum(bool(np.asarray(X)[:, m].any()) for m in np.flatnonzero(P[:, k]))


def rule(ncu, kbits, total, live, T):
    """sweep_pairs as documented (csrc/sweep_setup.hip), PARTLS_PAIR unset, on the 512-thread register kernel"""
    seg_len = (kbits + 1) // 2 if kbits >= 8 else kbits
    return T <= 16 and kbits >= 2 and (1 << kbits) >= ncu * 32 * (8 + seg_len) and total >= ncu * 32 and 12 <= live <= 16


def compare_routes(partls, oracle, monkeypatch, tag, X, y, P, flags, order_env, ranges=None, want=None):
    """PARTLS_PAIR unset against PARTLS_PAIR=0 on one problem; returns (walked in pairs?, the unset walk)"""
    identity = order_env.get("PARTLS_BIT_ORDER") == "identity"
    auto = walk(partls, monkeypatch, X, y, P, flags, order_env, ranges=ranges, identity=identity)
    off = walk(partls, monkeypatch, X, y, P, flags, dict(order_env, PARTLS_PAIR="0"), ranges=ranges, identity=identity)
    assert auto["order"] == off["order"]
    ncu, kbits, T = cu_count(), len(auto["order"]), (X.shape[1] + (flags & FAITHFUL) + 15) // 16
    live = live_on_bit0(X, P, flags, auto["order"])
    lo, hi = (ranges or [(0, auto["npat"])])[-1]
    expect = rule(ncu, kbits, hi - lo, live, T)
    print("[pair routes] %s: %d CUs, %d bits, T = %d, group %d with %d live variables on bit 0, range of %d: pair walk expected %s; "
          "%d pivots (PARTLS_PAIR=0: %d); winner %d (%d)" % (tag, ncu, kbits, T, auto["order"].index(0), live, hi - lo,
                                                             "on" if expect else "off", auto["pivots"], off["pivots"], auto["pat"], off["pat"]))
    if want is not None:
        assert expect == want(ncu), (tag, expect)
    if expect:
        assert auto["pivots"] < off["pivots"], (auto["pivots"], off["pivots"])
    else:
        assert auto["pivots"] == off["pivots"], (auto["pivots"], off["pivots"])
    assert auto["pat"] == off["pat"]
    assert abs(auto["obj"] - off["obj"]) <= TOL_WALKS * max(1.0, off["obj"])
    seen = np.arange(auto["npat"])
    if flags & FAITHFUL:
        seen = np.flatnonzero(~np.isnan(auto["all"]))
        assert len(seen) == hi - lo and np.array_equal(seen, np.flatnonzero(~np.isnan(off["all"])))
        np.testing.assert_allclose(auto["all"][seen], off["all"][seen], rtol=TOL_WALKS, err_msg=tag)
        assert auto["obj"] == auto["all"][auto["pat"]]
    pats = np.unique(np.concatenate([[auto["pat"]], np.random.default_rng(X.shape[1]).choice(seen, 48, replace=False)]))
    objs = oracle_objectives(oracle, X, y, P, flags, pats)
    wref = objs[pats.tolist().index(auto["pat"])]
    assert abs(auto["obj"] - wref) <= TOL_OBJ * max(1.0, wref), (auto["obj"], wref)
    if flags & FAITHFUL:
        assert np.all(np.abs(auto["all"][pats] - objs) <= TOL_OBJ * np.maximum(1.0, objs)), np.abs(auto["all"][pats] - objs).max()
    else:
        assert np.all(objs >= wref)                         # no all_opt with a fitted intercept: no sampled pattern beats the winner
    return expect, auto


IDENTITY = {"PARTLS_BIT_ORDER": "identity"}
# (tag, n, flags, K, live, null columns, the verdict given the CU count)
ROUTE_CASES = (
    ("12 live", 176, FAITHFUL, 17, 12, 0, lambda ncu: ncu <= 481),             # 2^18 >= 32 ncu (8 + 9)
    ("16 live", 176, FAITHFUL, 17, 16, 0, lambda ncu: ncu <= 481),
    ("17 live", 176, FAITHFUL, 17, 17, 0, lambda ncu: False),
    ("12 columns, 11 live", 176, FAITHFUL, 17, 11, 1, lambda ncu: False),
    ("14 columns, 10 live", 176, FAITHFUL, 17, 10, 4, lambda ncu: False),
    ("20 columns, 12 live", 176, FAITHFUL, 17, 12, 8, lambda ncu: ncu <= 481),
    ("12 live, 17 bits", 176, FAITHFUL, 16, 12, 0, lambda ncu: ncu <= 240),    # 2^17 >= 32 ncu (8 + 9): off on 256 CUs
    ("12 live, T = 17", 272, FAITHFUL, 17, 12, 0, lambda ncu: False),
    ("12 live, fitted", 176, 0, 18, 12, 0, lambda ncu: ncu <= 481),
    ("17 live, fitted", 176, 0, 18, 17, 0, lambda ncu: False),
)


@pytest.mark.parametrize("tag,n,flags,K,live,null,want", ROUTE_CASES, ids=[c[0] for c in ROUTE_CASES])
def test_automatic_route(partls, oracle, monkeypatch, tag, n, flags, K, live, null, want):
    X, y, P = route_problem(n, flags, K, live, null)
    compare_routes(partls, oracle, monkeypatch, tag, X, y, P, flags, IDENTITY, want=want)


def test_automatic_route_by_range(partls, oracle, monkeypatch):
    """a range of fewer than 32 patterns per CU keeps the plain walk, and its objectives are partls_opt_models' rows bit for bit"""
    X, y, P = route_problem(176, FAITHFUL, 17)
    ncu = cu_count()
    short, full = 32 * ncu - 2, 32 * ncu
    assert rule(ncu, 18, full, 12, 11), "the 18-bit enumeration is too short for the pair walk on %d CUs" % ncu
    on, _ = compare_routes(partls, oracle, monkeypatch, "range of 32 per CU", X, y, P, FAITHFUL, IDENTITY, ranges=[(0, full)])
    off, auto = compare_routes(partls, oracle, monkeypatch, "range of 2 less", X, y, P, FAITHFUL, IDENTITY, ranges=[(0, short)])
    assert on and not off
    m = walk(partls, monkeypatch, X, y, P, FAITHFUL, IDENTITY, ranges=[(0, short)], models=(0, short))["models"]
    assert m["n_unconverged"] == 0 and np.array_equal(m["pattern"], gray(np.arange(short)))
    assert np.array_equal(m["opt"], auto["all"][m["pattern"]])
    assert auto["obj"] in m["opt"] and m["pattern"][int(np.argmin(m["opt"]))] == auto["pat"]


def test_automatic_route_calibrated_order(partls, oracle, monkeypatch):
    """nothing set: the calibration chooses the group on bit 0 and the rule counts THAT group's live variables"""
    X, y, P = route_problem(176, FAITHFUL, 17)
    on, auto = compare_routes(partls, oracle, monkeypatch, "calibrated order", X, y, P, FAITHFUL, {})
    print("[pair routes] calibrated order %s: pair walk %s" % (auto["order"], "on" if on else "off"))


@pytest.mark.parametrize("n,flags", [(176, FAITHFUL), (256, 0)])
def test_forced_walk_under_a_permuted_order(partls, oracle, monkeypatch, capfd, n, flags):
    """K = 6: the 12 decoupled features are group 3, group 0 is a large ordinary group — the calibration puts another group than 0 on bit 0"""
    X, y, P = swapped(*problem("plain", n, flags), 3)
    env = {"PARTLS_BIT_ORDER": "calibrate"}
    off = walk(partls, monkeypatch, X, y, P, flags, forced(False, **env), capfd=capfd, identity=False)
    got = walk(partls, monkeypatch, X, y, P, flags, forced(True, **env), capfd=capfd, identity=False)
    print("[pair routes] permuted n=%d: order %s" % (n, got["order"]))
    assert got["order"] == off["order"] and got["order"][0] != 0, got["order"]
    objs = oracle_objectives(oracle, X, y, P, flags, np.arange(got["npat"])) if flags & FAITHFUL else None
    check("permuted n=%d %s" % (n, "faithful" if flags else "fitted"), dict(objs=objs, off=off), got)
    if objs is None:
        wref = oracle_objectives(oracle, X, y, P, flags, [got["pat"]])[0]
        assert abs(got["obj"] - wref) <= TOL_OBJ * max(1.0, wref)
    assert got["pivots"] < off["pivots"], (got["pivots"], off["pivots"])


@pytest.mark.parametrize("n", [176, 256])
def test_exact_ties_under_a_permuted_order(partls, oracle, monkeypatch, capfd, n):
    """`null` with group 3 as the group of all-zero columns (group 1 has no feature): flips of either change nothing, whatever bits the
    calibration gives them — every pattern equals its partners bit for bit and the first REFERENCE index wins in both walks"""
    X, y, P = swapped(*problem("null", n, FAITHFUL), 3)
    env = {"PARTLS_BIT_ORDER": "calibrate"}
    off = walk(partls, monkeypatch, X, y, P, FAITHFUL, forced(False, **env), capfd=capfd, identity=False)
    got = walk(partls, monkeypatch, X, y, P, FAITHFUL, forced(True, **env), capfd=capfd, identity=False)
    print("[pair routes] ties n=%d: order %s" % (n, got["order"]))
    assert got["order"] == off["order"] and got["order"] != list(range(K + 1)), got["order"]
    assert max(got["order"][1], got["order"][3]) < 4           # both inside every chain of 16: partners share a tableau
    objs = oracle_objectives(oracle, X, y, P, FAITHFUL, np.arange(got["npat"]))
    check("ties n=%d" % n, dict(objs=objs, off=off), got)
    pats = np.arange(got["npat"])
    for bit in (1 << 1, 1 << 3):
        assert np.array_equal(got["all"], got["all"][pats ^ bit]), bit
    assert got["pat"] & (1 << 1 | 1 << 3) == 0                 # the first reference index of the winner's four copies


# ---- D: near ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mirror", [(176, False), (256, False), (176, True), (256, True)])
def test_candidates_after_the_pair_walk(partls, oracle, monkeypatch, n, mirror):
    """The winner's four copies p, p ^ 1, p ^ 2, p ^ 3 (p: bits 0 and 1 clear) are four consecutive Gray indices 4 m .. 4 m + 3.  The plain
    walk visits them as p, p^1, p^3, p^2 (m even) or p^2, p^3, p^1, p (m odd); the pair walk, whose tableau stays on bit 0 clear here
    (C is empty: every twin is recorded, none visited), as p, p^1, p^2, p^3 or p^2, p^3, p, p^1.  The two `null` problems have m even;
    mirror: the columns of group 2 negated, which flips bit 2 of every pattern and makes m odd — there the runner-up of the winner's
    workgroup depends on the order of the visits unless exact ties among runners-up go to the first reference index as well."""
    X, y, P = problem("null", n, FAITHFUL)
    if mirror:
        X = np.array(X, order="F")
        X[:, np.asarray(P)[:, 2] != 0] *= -1.0
    off = walk(partls, monkeypatch, X, y, P, FAITHFUL, forced(False), cands=True)
    got = walk(partls, monkeypatch, X, y, P, FAITHFUL, forced(True), cands=True)
    (go, gp), (fo, fp) = got["cand"], off["cand"]
    print("[pair routes] candidates n=%d%s: %s %s (paired off: %s %s); the winner's Gray index %d" % (
        n, " mirrored" if mirror else "", gp.tolist(), go.tolist(), fp.tolist(), fo.tolist(), gray_inverse(int(gp[0]))))
    assert (gray_inverse(int(fp[0])) >> 2) & 1 == int(mirror)
    assert gp.tolist() == fp.tolist()
    np.testing.assert_allclose(go, fo, rtol=TOL_WALKS)
    assert gp[0] == got["pat"] == off["pat"] and go[0] == got["obj"]
    # group 0 is all zero and group 1 empty: the winner's copies differ from it in bits 0 and 1 only and have its objective exactly
    ties = [i for i in range(1, len(gp)) if (int(gp[i]) ^ int(gp[0])) < 4]
    assert ties and all(go[i] == go[0] for i in ties), (gp, go)
    assert all(go[i] > go[0] for i in range(1, len(gp)) if i not in ties)


# ---- E: shards ---------------------------------------------------------------------------------------------------------------------
def test_three_shards(partls, oracle, monkeypatch, capfd):
    """128 patterns over three ranks: [0, 42), [42, 85), [85, 128) — pairs cut at an odd boundary are ordinary patterns"""
    ref = reference(oracle, partls, monkeypatch, capfd, "plain", 176, FAITHFUL)
    X, y, P = ref["X"], ref["y"], ref["P"]
    one = sweep(partls, monkeypatch, X, y, P, FAITHFUL, pair=True)
    res = {}
    for pair in (True, False):
        for k, v in forced(pair).items():
            monkeypatch.setenv(k, v)
        mc = partls.MultiContext([0, 0, 0])
        for k in forced(pair):
            monkeypatch.delenv(k)
        try:
            a, b, t, opt, bi, allopt = mc.fit_opt(X, y, P, 0.0, FAITHFUL, want_all=True)
            assert mc.context(0).sweep_route() == (REG_512, 11)
            res[pair] = dict(bi=bi, all=allopt, opt=opt, pivots=sum(mc.context(r).pivots() for r in (1, 2)))
        finally:
            mc.close()
    got, off = res[True], res[False]
    print("[pair routes] three shards: winner %d (single context %d), pivots of ranks 1 and 2: %d (paired off %d)" % (
        got["bi"], one["pat"], got["pivots"], off["pivots"]))
    assert not np.isnan(got["all"]).any()
    np.testing.assert_allclose(got["all"], one["all"], rtol=TOL_WALKS)
    assert got["bi"] == one["pat"] == off["bi"]
    assert abs(got["all"][got["bi"]] - one["obj"]) <= TOL_WALKS * max(1.0, one["obj"])
    assert abs(got["opt"] - off["opt"]) <= TOL_WALKS * max(1.0, off["opt"])
    assert got["pivots"] < off["pivots"], (got["pivots"], off["pivots"])         # the ranks' contexts walked in pairs
