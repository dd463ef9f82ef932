"""Every LDS plan of the deferred-update sweep kernel (csrc/sweep_lazy.hip) in chain, models and node mode, up to the maximum n = 1023,
every pattern against the oracle.  The counterpart of test_gpu_tile_counts.py for the other sweep kernel.

The kernel's behaviour depends on the leading dimension ld = n + 1 through lazy_plan() (csrc/lazy_plan.h; restated here as lazy_plan,
held against the library's by test_lazy_plan.py): 512 threads up to ld = 512 and 1024 beyond, the block width mb and the height `rows`
of the LDS pool.  (threads, mb) classes, by ld:

  512 threads:  mb 16: 2 .. 334 (rows 64 up to ld 253, then 63 .. 48)   15: 335 .. 355   14: 356 .. 378   13: 379 .. 405
                12: 406 .. 436   11: 437 .. 471   10: 472 .. 512
  1024 threads: mb 8: 513 .. 621   7: 622 .. 694   6: 695 .. 785   5: 786 .. 903   4: 904 .. 1024 (rows 14 .. 12)

(mb, rows) decide when a block is cut short to fill the pool (never at mb <= 5), how many pending terms a flush applies (8 .. 12 at
the top, ~40 at n = 341), how far its read-ahead reaches into the rows + 4 pool, which panel runs, the flush's strip width and edge
strips (NTl mod 4 / 2, NTl = ceil(n / 16)), the materialise turn (NTl mod 3) and whether the last wave's rows end below lane 16
(ld mod 64 < 16).  A mistake confined to one class is invisible at every other, so the table holds every class, both neighbours of the
class edges 16 | 15, 512 | 1024 threads, 8 | 7, 6 | 5 and 5 | 4, n = 2 and the maximum n = 1023 (ld = 1024: every thread owns a row,
16 full mask words).  Sizes up to n = 253 run behind OPT_GENERIC_KERNEL.  test_table_covers_every_plan pins the table; every GPU test
asserts the route (ROUTE_DEFERRED) first.

Problems: those of test_gpu_tile_counts.py (its generator, N = 2 D + 50, D = n - 1 with the faithful intercept), designs rotating
plain, eta, dup, null, triple, scaled, overlap, layouts alternating contiguous / scattered; K = 7 up to n = 129 (K = 1 at n = 2), 5 up
to n = 333, 4 up to n = 693, 3 above, so that the oracle stays affordable (0.7 s per pattern at D = 1022).  The generator's dup and
triple designs alone never reach the panel's veto redo (the plain pivot test refuses their columns), so from D = 64 on those two
designs also carry the ten badly scaled triples of test_gpu_lazy.py (_plans_problem) in chain and models mode, and vetoes > 0 is
asserted on each of them: n = 289, 334, 511 on the stepwise panel, n = 620, 785, 903 on the two-phase panel.  Node mode keeps the
generator's own problem (see test_node_mode).

References: the oracle's per-pattern NNLS on QR-compressed data (tools/lazy_plan_reference_check.py: agrees with the dense oracle on
the raw data to round-off at n >= 620, and certifies the inner nodes used here), the eager kernel (sweep_generic.hip,
PARTLS_EAGER_GENERIC=1) for all patterns, tests/bnb_reference.py for nodes.  Tolerances are the suite's own, as listed in
test_gpu_tile_counts.py: objectives rtol 1e-9 on the well-posed designs, 1e-8 + 2e-7 ||y|| with planted dependence, 1e-6 ||y|| on
predictions, models _close(1e-9), lazy against eager and walk against walk rtol 1e-10 with pivot counts within 1 %, node bounds
through test_gpu_bnb_nodes._check, warm against cold node bounds rtol 1e-10.

The warm batch of the node test runs on a target that forces branching (test_gpu_lazy._branching_large) with 6 balanced groups, as
that file's own warm-start test has at D = 330, whatever the case's K: it needs no oracle, and the bound it asserts depends on the
share of the branched group.  The root (every group free) has all n variables basic.  The two children of a root branched on a
group of g variables push the g wrong-signed variables out between them and exchange up to as many again in their wake when warm,
<= 2 g pivots; cold, each child first enters the n - g variables of the free groups: >= 2 (n - g).  The ratio g / (n - g) is 1 / 5
at g = n / 6 and 1 / 2 at g = n / 3, so "a quarter of the cold pivots" is asserted with 6 groups, which is every case but n = 2
(one feature, one group: a group of one variable cannot mix signs, the root does not branch).

Measured on the MI355X: without the scaled triples every objective is within 6e-15 of the oracle (relative to max(1, obj)) and lazy
and eager within 4.7e-15 of each other, at every size up to n = 1023; with them 3.5e-11 and 5.5e-11.  No bound was set from these.
Totals: 1 table test without GPU and 3 x 28 + 1 = 85 GPU tests, 49 s for the file alone (the largest case 5 s)."""
import numpy as np
import pytest

from bnb_reference import NodeReference, U
from models_reference import _cleanup, _close, _scatter
from test_gpu_bnb_nodes import C_TWO, _check as _check_nodes, _nodes
from test_gpu_lazy import _branching_large
from test_gpu_tile_counts import DESIGNS, RANK_DEFICIENT, _bounds, _fits, _models_of, _oracle_all, _problem, _shards_ok, _winner_ok

gpu = pytest.mark.gpu

FAITHFUL, GENERIC = 1, 2                                    # OPT_FAITHFUL_INTERCEPT, OPT_GENERIC_KERNEL
ROUTE_DEFERRED, ROUTE_EAGER = 3, 4                          # partls_route (include/partls.h)
FORCED = (2, 15, 16, 17, 63, 64, 65, 129, 253)              # below the register kernel's limit: behind OPT_GENERIC_KERNEL
DEFAULT = (289, 333, 334, 368, 385, 420, 449, 511, 512, 620, 621, 640, 693, 784, 785, 902, 903, 1009, 1023)
CLASS_EDGES = (334, 512, 621, 785, 903)                     # last ld of a (threads, mb) class whose two neighbours the table must hold
KNOBS = ("PARTLS_REG_MAXT", "PARTLS_CHAIN_LEN", "PARTLS_NO_EXPORT", "PARTLS_EAGER_GENERIC", "PARTLS_GRID", "PARTLS_BNB_COLD",
         "PARTLS_BNB_BATCH", "PARTLS_PAIR", "PARTLS_BIT_ORDER")


def lazy_plan(ld):
    """(threads, mb, rows, dynamic LDS bytes) of a leading dimension, or None where no plan fits: csrc/lazy_plan.h and the choice of
    launch_sweep_lazy, restated"""
    mbmax, mt, maxr = 16, 8, 64
    budget = 151 * 1024
    fixed = ld * 8 + 4 * ld * 8 + 3 * ld + (2 * mbmax * mbmax + 8 * mbmax + 18) * 8 + 64
    row = ld * 8
    if budget < fixed + 6 * (row + 8 + mbmax * 8):
        return None
    rows = min(maxr, (budget - fixed) // (row + 8 + mbmax * 8))
    mb = min(rows // 3, mbmax)
    if ld > 512:
        mb = min(mb, mt)
    mb = max(mb, 2)
    shmem = ((rows + 4) * ld + ld + rows + mbmax + (rows + 4) * mbmax + 2 * mbmax * mbmax + 2 * mbmax + 18) * 8 + 3 * ld + 16
    return (512 if ld <= 512 else 1024), mb, rows, shmem


def snapshot_chunk_slots(n):
    """slots per chunk of the BnB snapshot pool beyond the register kernel (SnapshotPool::begin, snapshot_bytes: csrc/solvers.hip)"""
    ld = n + 1
    slot = ((ld * ld + ld) * 8 + n + 255) & ~255
    return max(8, min(512, (160 << 20) // slot))


def _table():
    out = []
    for i, n in enumerate(FORCED + DEFAULT):
        D = n - 1
        K = 1 if n == 2 else 7 if n <= 129 else 5 if n <= 333 else 4 if n <= 693 else 3
        threads, mb, rows, _ = lazy_plan(n + 1)
        design, layout = DESIGNS[i % len(DESIGNS)], ("contiguous", "scattered")[i % 2]
        out.append(dict(id="n%d-mb%d-rows%d-%s-%s" % (n, mb, rows, design, layout), n=n, D=D, K=K, design=design, layout=layout,
                        seed=7000000 + 1000 * i + n, flags=FAITHFUL | (GENERIC if n in FORCED else 0), route=(ROUTE_DEFERRED, 0),
                        threads=threads, mb=mb, rows=rows, env={},
                        free_too=n % 16 == 0,               # the chain test also runs flags without FAITHFUL, D = n
                        nodes=12 if n <= 693 else 4))
    return out


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}
IDS = list(BY_ID)


def _context(partls, monkeypatch, env=None):
    """a Context with the given knobs and no others (read once, at partls_create)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    ctx = partls.Context(0)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return ctx


def _vetoed(case, D=None):
    """does the case's problem carry the scaled dependent triples that only the leave-one-out rule refuses?"""
    return case["design"] in ("dup", "triple") and (case["D"] if D is None else D) >= 64


def _plans_problem(case, D=None, salt=0, planted=True):
    """the tile-count test's problem of the case (planted=False: as it is).  The duplicate columns and the unit-scale triple of its dup / triple designs are
    refused by the plain pivot test, which never reaches the panel's redo; from D = 64 on these two designs also get the ten badly
    scaled triples of test_gpu_lazy._problem in columns 20 .. 49 (x_i = 0.5 x_j - 2 x_l with a small x_j: its Gram-form pivot comes
    out above the threshold and only the leave-one-out rule refuses it)."""
    X, y, P, eta = _problem(case, D=D, salt=salt)
    if planted and _vetoed(case, D):
        for t in range(10):
            l, j, i = 20 + 3 * t, 21 + 3 * t, 22 + 3 * t
            X[:, j] *= 0.004
            X[:, i] = 0.5 * X[:, j] - 2.0 * X[:, l]
    return X, y, P, eta


_REF = {}


def _reference(oracle, case, planted=True):
    """the case's problem and its oracle results, computed once for the mode tests that share it"""
    key = (case["id"], planted and _vetoed(case))
    if key not in _REF:
        X, y, P, eta = _plans_problem(case, planted=planted)
        objs, ra = _oracle_all(oracle, X, y, P, eta)
        _REF[key] = dict(X=X, y=y, P=P, eta=eta, objs=objs, ra=ra, ynorm=max(1.0, float(np.linalg.norm(y))))
    return _REF[key]


def _rel(a, ref):
    return float(np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref))))


def _sweep(partls, monkeypatch, case, X, y, P, eta, flags, env, route, shards=None):
    """one full sweep, with every objective in faithful mode: dict(bo, bp, all, npat, pivots, vetoes); shards = (tag, objs, rtol, atol)
    also runs _shards_ok"""
    ctx = _context(partls, monkeypatch, env)
    try:
        ctx.opt_prepare(X, y, P, eta, flags)
        assert ctx.sweep_route() == route, "%s runs on %s" % (case["id"], ctx.sweep_route())
        bo, bp, allo, unconv = ctx.opt_sweep(0, -1, want_all=bool(flags & FAITHFUL))       # all_opt exists in faithful mode only
        assert unconv == 0, "%s %s: %d patterns hit the pivot cap" % (case["id"], env, unconv)
        out = dict(bo=bo, bp=bp, all=None if allo is None else allo.copy(), npat=ctx.num_patterns(), pivots=ctx.pivots(), vetoes=ctx.vetoes())
        if shards:
            tag, objs, rtol, atol = shards
            _shards_ok(tag, partls, ctx, objs, bo, bp, rtol, atol)
        return out
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_table_covers_every_plan():
    """the table against the restated plan: every (threads, mb) class, both neighbours of the class edges, n = 2 and n = 1023, the
    residues of ld, n and the tile count that select strips, turns and lane masks, every design on either thread plan"""
    plans = {ld: lazy_plan(ld) for ld in range(2, 1025)}
    assert all(plans.values()), "a plan is refused below ld = 1025"
    assert [c["n"] for c in CASES] == list(FORCED + DEFAULT) and len(BY_ID) == len(CASES)
    assert all(c["D"] == c["n"] - 1 and (c["threads"], c["mb"], c["rows"]) == plans[c["n"] + 1][:3] for c in CASES)
    assert all(bool(c["flags"] & GENERIC) == (c["n"] <= 288) and c["flags"] & FAITHFUL for c in CASES)
    lds = {c["n"] + 1 for c in CASES}
    classes = {p[:2] for p in plans.values()}
    assert classes == {(512, m) for m in range(10, 17)} | {(1024, m) for m in range(4, 9)}
    assert {(c["threads"], c["mb"]) for c in CASES} == classes
    for ld in CLASS_EDGES:
        assert plans[ld][:2] != plans[ld + 1][:2], ld
        assert ld in lds and ld + 1 in lds, ld
    assert plans[253][2] == 64 and plans[254][2] == 63 and 254 in lds          # the first ld whose pool is budget-bound
    assert 3 in lds and 1024 in lds and plans[1024][1:3] == (4, 12)
    assert max(p[3] for p in plans.values()) == plans[694][3] and 694 in lds   # the largest LDS request
    assert any(ld % 64 < 16 for ld in lds)
    ns = [c["n"] for c in CASES]
    assert {0, 1, 15} <= {n % 16 for n in ns}
    assert {0, 1, 3} <= {((n + 15) // 16) % 4 for n in ns} and {0, 1, 2} == {((n + 15) // 16) % 3 for n in ns}
    for threads in (512, 1024):
        assert {c["design"] for c in CASES if c["threads"] == threads} == set(DESIGNS), threads
        for d in ("dup", "triple"):
            assert any(c["design"] == d and c["threads"] == threads and _vetoed(c) for c in CASES), (threads, d)
        assert {c["layout"] for c in CASES if c["threads"] == threads} == {"contiguous", "scattered"}
    assert [c["K"] for c in CASES] == [1 if n == 2 else 7 if n <= 129 else 5 if n <= 333 else 4 if n <= 693 else 3 for n in ns]
    assert all(c["free_too"] == (c["n"] % 16 == 0) for c in CASES) and sum(c["free_too"] for c in CASES) >= 5
    assert snapshot_chunk_slots(1023) == 19


@gpu
@pytest.mark.parametrize("cid", IDS)
def test_chain_mode(partls, oracle, monkeypatch, cid):
    """opt_sweep on the lazy and on the eager kernel: every pattern's objective against the oracle, lazy against eager, the winner,
    three shards, a second lazy walk in which every workgroup walks several chains through one pool (PARTLS_CHAIN_LEN=4,
    PARTLS_GRID=2); at n mod 16 = 0 also the free-intercept problem with D = n features"""
    case = BY_ID[cid]
    ref = _reference(oracle, case)
    X, y, P, eta, objs = ref["X"], ref["y"], ref["P"], ref["eta"], ref["objs"]
    rtol, atol = _bounds(case, ref)
    lz = _sweep(partls, monkeypatch, case, X, y, P, eta, case["flags"], None, case["route"], shards=(cid, objs, rtol, atol))
    eg = _sweep(partls, monkeypatch, case, X, y, P, eta, case["flags"], {"PARTLS_EAGER_GENERIC": "1"}, (ROUTE_EAGER, 0))
    w2 = _sweep(partls, monkeypatch, case, X, y, P, eta, case["flags"], {"PARTLS_CHAIN_LEN": "4", "PARTLS_GRID": "2"}, case["route"])
    fig = dict(oracle=_rel(lz["all"], objs), eager_oracle=_rel(eg["all"], objs), gap=float(np.max(np.abs(lz["all"] - eg["all"]) / eg["all"])),
               walks=float(np.max(np.abs(w2["all"] - lz["all"]) / lz["all"])))
    print("[plans] %s chain: lazy vs oracle %.3g, eager vs oracle %.3g (relative to max(1, obj)), lazy vs eager %.3g, walks differ by "
          "%.3g; pivots %d / %d, vetoes %d / %d" % (cid, fig["oracle"], fig["eager_oracle"], fig["gap"], fig["walks"], lz["pivots"],
                                                    eg["pivots"], lz["vetoes"], eg["vetoes"]))
    np.testing.assert_allclose(lz["all"], objs, rtol=rtol, atol=atol, err_msg=cid + ": lazy kernel against the oracle")
    np.testing.assert_allclose(eg["all"], objs, rtol=rtol, atol=atol, err_msg=cid + ": eager kernel against the oracle")
    np.testing.assert_allclose(lz["all"], eg["all"], rtol=1e-10, err_msg=cid + ": lazy against eager")
    assert abs(lz["pivots"] - eg["pivots"]) <= 0.01 * eg["pivots"], (lz["pivots"], eg["pivots"])
    _winner_ok(cid, objs, lz["bo"], lz["bp"], rtol, atol)
    _winner_ok(cid + " eager", objs, eg["bo"], eg["bp"], rtol, atol)
    np.testing.assert_allclose(w2["all"], lz["all"], rtol=1e-10, err_msg=cid + ": several chains per workgroup against the default walk")
    tol = rtol * max(1.0, float(objs.min())) + atol
    assert w2["bp"] == lz["bp"] or abs(objs[w2["bp"]] - objs[lz["bp"]]) <= tol, (w2["bp"], lz["bp"])
    if _vetoed(case):
        assert lz["vetoes"] > 0, "%s: no pivot was refused by the leave-one-out rule: the panel's redo did not run" % cid
    if not case["free_too"]:
        return
    # free intercept: n = D, one pattern per sign vector of the groups; its optimum is the better of the two intercept signs
    Xf, yf, Pf, etaf = _plans_problem(case, D=case["n"], salt=1)
    fo, _ = _oracle_all(oracle, Xf, yf, Pf, etaf)
    half = len(fo) // 2
    fobjs = np.minimum(fo[:half], fo[half:])
    ynorm = max(1.0, float(np.linalg.norm(yf)))
    frtol, fatol = (1e-8, 2e-7 * ynorm) if case["design"] in RANK_DEFICIENT else (1e-9, 0.0)
    tag = cid + " free intercept"
    fr = _sweep(partls, monkeypatch, case, Xf, yf, Pf, etaf, case["flags"] & ~FAITHFUL, None, case["route"], shards=(tag, fobjs, frtol, fatol))
    assert fr["npat"] == half
    _winner_ok(tag, fobjs, fr["bo"], fr["bp"], frtol, fatol)


@gpu
@pytest.mark.parametrize("cid", IDS)
def test_models_mode(partls, oracle, monkeypatch, cid):
    """opt_models(raw=True) on the lazy kernel's MODELS instantiation: every pattern exactly once, the objectives bit-equal to the same
    context's all_opt, objective, nonneg_lsq's alpha and the cleaned alpha / beta / t of every pattern against the oracle (with planted
    dependence: objective and predictions), and a range cut inside a chain"""
    case = BY_ID[cid]
    ref = _reference(oracle, case)
    X, y, P, eta, objs, ra = ref["X"], ref["y"], ref["P"], ref["eta"], ref["objs"], ref["ra"]
    rtol, atol = _bounds(case, ref)
    ctx = _context(partls, monkeypatch)
    try:
        ctx.opt_prepare(X, y, P, eta, case["flags"])
        assert ctx.sweep_route() == case["route"]
        npat = ctx.num_patterns()
        _, _, allo, unconv = ctx.opt_sweep(0, -1, want_all=True)
        r = ctx.opt_models(raw=True)
        cut = ctx.opt_models(3, npat - 5, raw=True) if npat > 8 else None
    finally:
        ctx.close()
    assert unconv == 0 and r["n_unconverged"] == 0 and len(r["pattern"]) == npat == len(objs)
    # one piece on the plain sweep's chain plan: the objectives are all_opt's, bit for bit
    assert np.array_equal(r["opt"], allo[r["pattern"]]), cid
    s = _scatter(r, npat)
    alpha, beta, t = _models_of(ra, P)
    d = np.linalg.norm(_fits(X, P, s["alpha"], s["beta"], s["t"]) - _fits(X, P, alpha, beta, t), axis=1).max()
    print("[plans] %s models: max objective error %.3g, max raw alpha error %.3g, max prediction distance %.3g ||y||, %d vetoes" % (
        cid, _rel(s["opt"], objs), _rel(s["raw_alpha"], ra), d / ref["ynorm"], r["n_vetoes"]))
    np.testing.assert_allclose(s["opt"], objs, rtol=rtol, atol=atol, err_msg=cid)
    da, db, dt = _models_of(s["raw_alpha"], P)                                # the cleaned model is cleanupResult of the device's own raw alpha
    _close(s["alpha"], da); _close(s["beta"], db); _close(s["t"], dt)
    if case["design"] in RANK_DEFICIENT:
        assert d <= 1e-6 * ref["ynorm"], "%s: predictions %.3g ||y|| from the oracle's" % (cid, d / ref["ynorm"])
    else:
        assert r["n_vetoes"] == 0
        _close(s["raw_alpha"], ra)
        _close(s["alpha"], alpha); _close(s["beta"], beta); _close(s["t"], t)
    if cut is not None:
        assert cut["n_unconverged"] == 0 and np.array_equal(cut["pattern"], r["pattern"][3:npat - 5])
        full = {k: r[k][3:npat - 5] for k in ("opt", "alpha", "beta", "t", "raw_alpha")}
        _close(cut["opt"], full["opt"], 1e-10)
        if case["design"] in RANK_DEFICIENT:                                   # another chain start, another of the equal minimisers
            dc = np.linalg.norm(_fits(X, P, cut["alpha"], cut["beta"], cut["t"]) - _fits(X, P, full["alpha"], full["beta"], full["t"]), axis=1).max()
            assert dc <= 1e-6 * ref["ynorm"], "%s: the cut's predictions %.3g ||y|| from the full call's" % (cid, dc / ref["ynorm"])
        else:
            for k in ("alpha", "beta", "t", "raw_alpha"):
                _close(cut[k], full[k], 1e-10)


@gpu
@pytest.mark.parametrize("cid", IDS)
def test_node_mode(partls, oracle, monkeypatch, cid):
    """bnb_bound: every leaf is Opt's pattern of the same bits; the root and a few random inner nodes against the exact node reference;
    opt_finish of the winner with and without the sweep's exported solution; one warm batch (root into a snapshot slot, its two
    children from that slot) against the same batch on a PARTLS_BNB_COLD context.  On the generator's own problem, without the scaled
    triples: the bounds of test_gpu_bnb_nodes (C_TWO, C_UP in u y'y) were measured on designs whose accepted columns are well
    conditioned, and a triple's x_i = -2 x_l + 0.002 e gives the Gram block of the normalised pair the condition 2 / (0.001^2 / 2) = 4e6."""
    case = BY_ID[cid]
    ref = _reference(oracle, case, planted=False)
    X, y, P, eta, objs = ref["X"], ref["y"], ref["P"], ref["eta"], ref["objs"]
    rtol, atol = _bounds(case, ref)
    K = P.shape[1]
    Kp = K + 1
    leaves = np.arange(1 << Kp, dtype=np.uint64)
    assert len(leaves) <= 16 or case["n"] < 785               # the scratch tableau of a node batch is grid x ld^2 doubles
    ipats, ifrees = _nodes(np.random.default_rng(case["seed"]), Kp, case["nodes"])
    fin = {}
    for mode, env in (("export", None), ("resolve", {"PARTLS_NO_EXPORT": "1"})):
        ctx = _context(partls, monkeypatch, env)
        try:
            ctx.opt_prepare(X, y, P, eta, case["flags"])
            assert ctx.sweep_route() == case["route"]
            if mode == "export":
                lb, br = ctx.bnb_bound(leaves, np.zeros_like(leaves))
                ilb, ibr = ctx.bnb_bound(ipats, ifrees)
            bo, bp, allo, unconv = ctx.opt_sweep(0, -1, want_all=True)
            assert unconv == 0
            fin[mode] = ctx.opt_finish(bp)
        finally:
            ctx.close()
    nref = NodeReference(X, y, P, eta)
    assert (br == -1).all(), "a leaf has no free group to branch on"
    loose = np.flatnonzero(P.sum(axis=1) == 0)
    if len(loose) == 0:
        e2 = np.abs(lb ** 2 - allo ** 2) / (U * nref.yy)
        print("[plans] %s node: leaves against chain mode %.3g u y'y, against the oracle %.3g" % (cid, e2.max(), _rel(lb, objs)))
        assert e2.max() <= C_TWO, "%s: leaf lb vs all_opt: %.3g u y'y at pattern %d" % (cid, e2.max(), int(np.argmax(e2)))
        np.testing.assert_allclose(lb, objs, rtol=rtol, atol=atol, err_msg=cid)
    else:
        # a feature in no group is fixed at 0 by Opt and left free by BnB (test_gpu_tile_counts.test_node_mode): such a leaf is the
        # better of the two patterns that the feature's sign adds once the feature sits in a group of its own
        assert len(loose) == 1
        P2 = np.asfortranarray(np.hstack([P, np.zeros((P.shape[0], 1), dtype=np.int64)]))
        P2[loose[0], K] = 1
        o2, _ = _oracle_all(oracle, X, y, P2, eta)
        b = np.arange(1 << Kp)
        b2 = (b & ((1 << K) - 1)) | ((b >> K) << (K + 1))
        leaf = np.minimum(o2[b2], o2[b2 | (1 << K)])
        print("[plans] %s node: leaves against the oracle %.3g" % (cid, _rel(lb, leaf)))
        np.testing.assert_allclose(lb, leaf, rtol=rtol, atol=atol, err_msg=cid)
        assert np.all(lb ** 2 <= allo ** 2 + C_TWO * U * nref.yy), "%s: freeing a feature cannot raise a bound" % cid
    _check_nodes(cid, nref, nref.nodes(ipats, ifrees), ipats, ifrees, ilb, ibr, case["design"] in RANK_DEFICIENT)
    b = int(np.argmin(objs))
    m = float(objs[b])
    want = _fits(X, P, *[np.asarray(v)[None] for v in _cleanup(ref["ra"][b], P, b)])[0]
    for mode, (a, bt, t, opt, bi) in fin.items():
        assert abs(opt - m) <= 1e-9 * max(1.0, m), "%s %s: opt %.17g, oracle %.17g" % (cid, mode, opt, m)
        d = np.linalg.norm(_fits(X, P, a[None], bt[None], np.array([t]))[0] - want)
        assert d <= 1e-6 * ref["ynorm"], "%s %s: predictions %.3g ||y|| from the oracle's" % (cid, mode, d / ref["ynorm"])
    assert fin["export"][4] == fin["resolve"][4] and abs(fin["export"][3] - fin["resolve"][3]) <= 1e-12 * fin["resolve"][3]
    # the warm batch: a node with a destination slot flushes what is pending when it ends (an Rcur no chain-mode flush has), and its
    # children start from that snapshot
    D = case["D"]
    Kb = max(1, min(6, D // 2))
    Xb, yb, Pb = _branching_large(case["seed"], 2 * D + 50, D, Kb)
    full = (1 << (Kb + 1)) - 1
    res = {}
    for mode, env in (("warm", None), ("cold", {"PARTLS_BNB_COLD": "1"})):
        ctx = _context(partls, monkeypatch, env)
        try:
            ctx.opt_prepare(Xb, yb, Pb, 0.0, case["flags"])
            assert ctx.sweep_route() == case["route"]
            ctx.bnb_snap_begin()
            lb0, br0, dst0 = ctx.bnb_bound_snap(np.array([0], dtype=np.uint64), np.array([full], dtype=np.uint64), np.array([-1], dtype=np.int32))
            k = int(br0[0])
            assert k >= 0 or D < 2, "%s: the root of the branching problem does not branch" % cid
            bit = 1 << max(k, 0)                              # D = 1: a group of one variable cannot mix signs; its children are bounded all the same
            fr = full & ~bit
            lb1, br1, _ = ctx.bnb_bound_snap(np.array([bit, 0], dtype=np.uint64), np.array([fr, fr], dtype=np.uint64),
                                             np.array([dst0[0], dst0[0]], dtype=np.int32))
            res[mode] = dict(lb0=lb0[0], k=k, dst0=int(dst0[0]), lb1=lb1.copy(), br1=br1.copy(), piv=ctx.pivots())
        finally:
            ctx.close()
    w, c = res["warm"], res["cold"]
    print("[plans] %s node: warm children differ from cold by %.3g, pivots %d / %d" % (
        cid, float(np.max(np.abs(w["lb1"] - c["lb1"]) / c["lb1"])), w["piv"], c["piv"]))
    assert w["dst0"] >= 0 and c["dst0"] == -1                 # a snapshot was taken; none in cold mode
    assert w["k"] == c["k"] and abs(w["lb0"] - c["lb0"]) <= 1e-10 * c["lb0"]
    np.testing.assert_allclose(w["lb1"], c["lb1"], rtol=1e-10, err_msg=cid + ": warm against cold children")
    np.testing.assert_array_equal(w["br1"], c["br1"])
    assert np.all(w["lb1"] >= w["lb0"] * (1.0 - 1e-10)), "%s: a child's bound lies below its parent's" % cid
    if Kb == 6:                                               # see the module docstring
        assert w["piv"] * 4 < c["piv"], (w["piv"], c["piv"])


@gpu
def test_snapshot_pool_crosses_a_chunk_at_the_maximum(partls, monkeypatch):
    """n = 1023: a chunk of the snapshot pool holds 19 slots (8.4 MB each); a search that bounds more nodes than that allocates a second
    chunk.  Warm against cold: the same search node for node, and its optimum is the Opt sweep's minimum on the same data."""
    D, K = 1022, 4
    X, y, P = _branching_large(1023, 2 * D + 50, D, K)
    res = {}
    for mode, env in (("warm", {"PARTLS_BNB_BATCH": "16"}), ("cold", {"PARTLS_BNB_BATCH": "16", "PARTLS_BNB_COLD": "1"})):
        ctx = _context(partls, monkeypatch, env)
        try:
            ctx.opt_prepare(X, y, P, 0.0, FAITHFUL)
            assert ctx.sweep_route() == (ROUTE_DEFERRED, 0)
            res[mode] = ctx.bnb_search(0)
            if mode == "warm":
                bo, bp, _, unconv = ctx.opt_sweep(0, -1)
                assert unconv == 0
        finally:
            ctx.close()
    w, c = res["warm"], res["cold"]
    print("[plans] snapshot pool at n = 1023: %d nodes bounded, %d slots per chunk, mu %.17g, Opt %.17g" % (w[3], snapshot_chunk_slots(D + 1), w[0], bo))
    assert w[1:] == c[1:], (w, c)
    assert abs(w[0] - c[0]) <= 1e-10 * c[0]
    assert abs(w[0] - bo) <= 1e-9 * max(1.0, bo), "BnB optimum %.17g, Opt sweep's minimum %.17g" % (w[0], bo)
    assert w[3] > snapshot_chunk_slots(D + 1), "%d nodes bounded: the pool never needed a second chunk" % w[3]
