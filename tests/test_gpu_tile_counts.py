"""Every tile count of the register sweep kernels (csrc/sweep_blk.hip) in all four modes, every pattern against the oracle.

The register kernel is a template over the tile count T = ceil(n / 16), compiled for T = 1 .. 20, and each T exists as four
instantiations with a static register layout of their own (slots, split of the tile columns over the workgroup halves, gather / scatter
if-chains, row stride by parity of T, 256 threads up to T = 10, winner export up to T = 17):

  chain   <T, false>                 opt_sweep                         test_chain_mode
  models  <T, false, true>           opt_models                        test_models_mode
  node    <T, true>                  bnb_bound, opt_finish's re-solve  test_node_mode
  batch   <T, false, false, true>    cv_opt                            test_batch_mode

A mistake confined to one T is invisible at every other T, so the table below holds two problems per T: n = 16 T (last tile full) and
n = 16 (T - 1) + 1 (last tile: one variable and 15 padded rows and columns; n = 2 at T = 1), n = D + 1 in faithful mode.  T = 19 and 20
run behind PARTLS_REG_MAXT=20.  Every test asserts the route (Context.sweep_route()) before anything else, so a changed threshold
fails here instead of moving a case to another kernel; test_table_covers_every_instantiation pins the table itself.

Problems: K = 7 groups (256 faithful patterns; K = 1 at D = 1), N = 2 D + 50, seeds from (T, n).  The group layout alternates between
the two sizes of a T: contiguous groups of unequal size (the largest holds a quarter of the features: longer than a tile column from
D = 65 on, so a flip turns over whole tile columns: more than 8 violators in one, the two-blocks-per-column path) and scattered groups.
The design rotates over the table: plain, eta > 0, duplicate columns, null column, dependent triple, badly scaled columns, overlapping
groups with an empty group and a feature in no group; each meets the 256-thread and the 512-thread kernel at least twice.  The batch
test runs 8 problems (3 folds x eta = [0, 0.3] and the path) with K = 7 up to T = 6 and K = 4 above, which keeps the oracle's share of
the run time at that of one full enumeration per case.

Reference: the oracle's per-pattern NNLS (dense Lawson-Hanson, Opt.jl:87-90) on QR-compressed data, every pattern of every case
(tools/tile_count_reference_check.py: on these inputs it agrees with the dense oracle on the uncompressed data to 1e-11 relative and
the node reference certifies every node).  Tolerances are the suite's own: objectives rtol 1e-9 on the well-posed designs
(test_gpu_lazy.py, test_gpu_fullsize.py); rtol 1e-8 + 2e-7 ||y|| with planted dependence and 1e-6 ||y|| on predictions
(test_gpu_fuzz.py); models _close(1e-9) (test_gpu_models.py); node bounds C_TWO / C_UP / W_REL / NEAR_TIE_SHARE through
test_gpu_bnb_nodes._check; two walks of one problem rtol 1e-10 (test_gpu_lazy.py); the finished winner 1e-9 and 1e-6 ||y||
(test_gpu_edge.py); cross-validation problems through test_gpu_cv._check."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from bnb_reference import NodeReference, U
from models_reference import _cleanup, _close, _scatter
from test_gpu_bnb_nodes import C_TWO, _check as _check_nodes, _nodes
from test_gpu_cv import _check as _check_cv

pytestmark = pytest.mark.gpu

FAITHFUL = 1
REG_256, REG_512 = 1, 2                                     # partls_route (include/partls.h)
DESIGNS = ("plain", "eta", "dup", "null", "triple", "scaled", "overlap")
RANK_DEFICIENT = ("dup", "null", "triple")


def _table():
    out = []
    for T in range(1, 21):
        for j, n in enumerate((16 * T, 16 * (T - 1) + 1 if T > 1 else 2)):
            D = n - 1
            design = DESIGNS[(2 * (T - 1) + j) % len(DESIGNS)]
            layout = ("contiguous", "scattered")[(T + j) % 2]
            out.append(dict(id="T%d-n%d-%s-%s" % (T, n, design, layout), T=T, n=n, D=D, K=min(7, D), design=design, layout=layout,
                            seed=100000 * T + n, route=(REG_256 if T <= 10 else REG_512, T),
                            env={"PARTLS_REG_MAXT": "20"} if T >= 19 else {},
                            free_too=j == 0,                # the chain test also runs flags = 0 (n = D = 16 T, 2^K patterns)
                            K_batch=min(7, D) if T <= 6 else 4))
    return out


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}
IDS = list(BY_ID)


def _problem(case, D=None, K=None, salt=0):
    """(X, y, P, eta) of a case; D, K override the case's (the free-intercept and the batch variants), salt separates their seeds"""
    D = case["D"] if D is None else D
    K = case["K"] if K is None else K
    design, layout = case["design"], case["layout"]
    rng = np.random.default_rng(case["seed"] + 7919 * salt)
    N = 2 * D + 50
    X = rng.standard_normal((N, D))
    Kg = K - 1 if design == "overlap" and K >= 3 else K       # overlap: group K - 1 stays empty
    if layout == "contiguous":
        wts = rng.permutation(Kg) + 1.0
        sizes = np.maximum(1, np.floor(wts / wts.sum() * D)).astype(int)
        sizes[int(np.argmax(sizes))] += D - int(sizes.sum())
        assert sizes.min() >= 1 and sizes.sum() == D
        grp = np.repeat(np.arange(Kg), sizes)
    else:
        grp = rng.integers(0, Kg, D)
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    w = rng.standard_normal(D) * (rng.random(D) < 0.6)
    eta = 0.0
    if design == "eta":
        eta = 0.5
    elif design == "dup" and D >= 3:
        a, b = rng.choice(D, 2, replace=False)
        X[:, a] = X[:, b]
        if D >= 40:
            X[:, D - 1] = X[:, D - 2]
    elif design == "null" and D >= 3:
        X[:, rng.integers(0, D)] = 0.0
    elif design == "triple" and D >= 4:
        i, j, l = rng.choice(D, 3, replace=False)
        X[:, i] = 0.5 * X[:, j] - 2.0 * X[:, l]
    elif design == "scaled":
        sc = np.exp(rng.uniform(-3, 3, size=D))
        X *= sc[None, :]
        w /= sc
    elif design == "overlap" and K >= 3:
        for m in range(0, min(12, D - 1), 3):
            P[m, (grp[m] + 1) % Kg] = 1                       # features in two groups
        P[D - 1] = 0                                          # a feature in no group
    y = X @ w + 0.4 + 0.3 * rng.standard_normal(N)
    return np.asfortranarray(X), y, np.asfortranarray(P), eta


def _oracle_all(oracle, X, y, P, eta):
    """every faithful pattern on QR-compressed data: (objectives[2^(K+1)], nonneg_lsq's alpha[2^(K+1), M + 1]); the patterns are
    independent solves, spread over a few threads (the oracle keeps no state between calls)"""
    Xo, Po = oracle.homogeneous(X, P)
    Xr, yr = oracle.regularize(Xo, y, Po, eta)
    R, z = oracle.compress(Xr, yr)
    pats = np.arange(1 << Po.shape[1])
    with ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(lambda p: oracle.opt_patterns(R, z, Po, p, want_alpha=True), np.array_split(pats, min(8, len(pats)))))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


_REF = {}


def _reference(oracle, case):
    """the case's problem and its oracle results, computed once for the four mode tests"""
    if case["id"] not in _REF:
        X, y, P, eta = _problem(case)
        objs, ra = _oracle_all(oracle, X, y, P, eta)
        _REF[case["id"]] = dict(X=X, y=y, P=P, eta=eta, objs=objs, ra=ra, ynorm=max(1.0, float(np.linalg.norm(y))))
    return _REF[case["id"]]


def _bounds(case, ref):
    """(rtol, atol) of an objective against the oracle: see the module docstring"""
    if case["design"] in RANK_DEFICIENT:
        return 1e-8, 2e-7 * ref["ynorm"]
    return 1e-9, 0.0


def _context(partls, monkeypatch, case, env=None):
    """a Context with the case's knobs (read once, at partls_create)"""
    env = dict(case["env"], **(env or {}))
    for k in ("PARTLS_REG_MAXT", "PARTLS_CHAIN_LEN", "PARTLS_NO_EXPORT", "PARTLS_CV_SERIAL", "PARTLS_EAGER_GENERIC", "PARTLS_GRID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = partls.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


def _models_of(ra, P):
    """cleanupResult of every pattern's raw alpha: (alpha[B, M], beta[B, K], t[B])"""
    cl = [_cleanup(ra[b], P, b) for b in range(len(ra))]
    return np.stack([c[0] for c in cl]), np.stack([c[1] for c in cl]), np.array([c[2] for c in cl])


def _fits(X, P, alpha, beta, t):
    """predictions of a stack of models (PartitionedLS.jl:132): [B, N]"""
    W = alpha * (beta @ P.T.astype(np.float64))
    return W @ X.T + np.asarray(t)[:, None]


def _winner_ok(tag, objs, bo, bp, rtol, atol):
    """the reported winner attains the oracle's minimum (a tie may pick another index of equal objective, as in the fuzz)"""
    m = float(objs.min())
    tol = rtol * max(1.0, m) + atol
    assert abs(bo - m) <= tol, "%s: best objective %.17g, oracle %.17g" % (tag, bo, m)
    assert objs[bp] <= m + tol, "%s: pattern %d (oracle %.17g) does not attain the minimum %.17g" % (tag, bp, objs[bp], m)


def _shards_ok(tag, partls, ctx, objs, bo, bp, rtol, atol):
    """three Gray-index shards reproduce the full sweep's winner"""
    npat = ctx.num_patterns()
    parts = [ctx.opt_sweep(*partls.dist.shard_range(npat, r, 3)) for r in range(3)]
    assert all(p[3] == 0 for p in parts), tag
    so, sp = min((p[0], p[1]) for p in parts)
    assert abs(so - bo) <= 1e-10 * bo, "%s: shards' best %.17g, full sweep %.17g" % (tag, so, bo)
    tol = rtol * max(1.0, float(objs.min())) + atol
    assert sp == bp or abs(objs[sp] - objs[bp]) <= tol, "%s: shards' winner %d, full sweep's %d (no tie in the oracle)" % (tag, sp, bp)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_table_covers_every_instantiation():
    """both sizes of every T = 1 .. 20, 256 threads up to T = 10 and 512 beyond; every design at least twice on either kernel"""
    assert [(c["T"], c["n"]) for c in CASES] == [(T, n) for T in range(1, 21) for n in (16 * T, 16 * (T - 1) + 1 if T > 1 else 2)]
    assert all((c["n"] + 15) // 16 == c["T"] and c["D"] == c["n"] - 1 for c in CASES)
    routes = sorted(c["route"] for c in CASES)
    assert routes == sorted([(REG_256, T) for T in range(1, 11)] * 2 + [(REG_512, T) for T in range(11, 21)] * 2)
    for kernel in (REG_256, REG_512):
        for d in DESIGNS:
            assert sum(c["route"][0] == kernel and c["design"] == d for c in CASES) >= 2, (kernel, d)
    for T in range(1, 21):
        assert {c["layout"] for c in CASES if c["T"] == T} == {"contiguous", "scattered"}
    assert all(c["K"] == 7 for c in CASES if c["D"] >= 7)
    big = [c for c in CASES if c["layout"] == "contiguous" and c["D"] > 64]
    assert big and all(_problem(c)[2].sum(axis=0).max() > 16 for c in big)


@pytest.mark.parametrize("cid", IDS)
def test_chain_mode(partls, oracle, monkeypatch, cid):
    """opt_sweep: every pattern's objective, the winner, a second walk with chain starts dominating (PARTLS_CHAIN_LEN=16), three shards;
    at n = 16 T also the free-intercept problem with D = n features (flags = 0: 2^K patterns, the winner)"""
    case = BY_ID[cid]
    ref = _reference(oracle, case)
    X, y, P, eta, objs = ref["X"], ref["y"], ref["P"], ref["eta"], ref["objs"]
    rtol, atol = _bounds(case, ref)
    got = {}
    for walk, env in (("default", None), ("chain16", {"PARTLS_CHAIN_LEN": "16"})):
        ctx = _context(partls, monkeypatch, case, env)
        try:
            ctx.opt_prepare(X, y, P, eta, FAITHFUL)
            assert ctx.sweep_route() == case["route"]
            bo, bp, allo, unconv = ctx.opt_sweep(0, -1, want_all=True)
            assert unconv == 0, "%s %s: %d patterns hit the pivot cap" % (cid, walk, unconv)
            got[walk] = (bo, bp, allo.copy())
            if walk == "default":
                _shards_ok(cid, partls, ctx, objs, bo, bp, rtol, atol)
        finally:
            ctx.close()
    bo, bp, allo = got["default"]
    err = np.abs(allo - objs) / np.maximum(1.0, np.abs(objs))
    print("[tiles] %s chain: max error %.3g (relative to max(1, obj)), walks differ by %.3g" % (
        cid, err.max(), np.max(np.abs(got["chain16"][2] - allo) / allo)))
    np.testing.assert_allclose(allo, objs, rtol=rtol, atol=atol, err_msg=cid)
    _winner_ok(cid, objs, bo, bp, rtol, atol)
    np.testing.assert_allclose(got["chain16"][2], allo, rtol=1e-10, err_msg=cid + ": PARTLS_CHAIN_LEN=16 against the default walk")
    _winner_ok(cid + " chain16", objs, got["chain16"][0], got["chain16"][1], rtol, atol)
    if not case["free_too"]:
        return
    # free intercept: n = D, one pattern per sign vector of the groups; its optimum is the better of the two intercept signs
    Xf, yf, Pf, etaf = _problem(case, D=case["n"], salt=1)
    fo, _ = _oracle_all(oracle, Xf, yf, Pf, etaf)
    half = len(fo) // 2
    fobjs = np.minimum(fo[:half], fo[half:])
    ynorm = max(1.0, float(np.linalg.norm(yf)))
    frtol, fatol = (1e-8, 2e-7 * ynorm) if case["design"] in RANK_DEFICIENT else (1e-9, 0.0)
    ctx = _context(partls, monkeypatch, case)
    try:
        ctx.opt_prepare(Xf, yf, Pf, etaf, 0)
        assert ctx.sweep_route() == case["route"] and ctx.num_patterns() == half
        bo, bp, _, unconv = ctx.opt_sweep(0, -1)
        assert unconv == 0
        _winner_ok(cid + " free intercept", fobjs, bo, bp, frtol, fatol)
        _shards_ok(cid + " free intercept", partls, ctx, fobjs, bo, bp, frtol, fatol)
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", IDS)
def test_models_mode(partls, oracle, monkeypatch, cid):
    """opt_models(raw=True): every pattern exactly once; objective, nonneg_lsq's alpha and the cleaned alpha / beta / t of every pattern.
    With planted dependence the minimiser is not unique: objective and predictions instead of the coefficients."""
    case = BY_ID[cid]
    ref = _reference(oracle, case)
    X, y, P, eta, objs, ra = ref["X"], ref["y"], ref["P"], ref["eta"], ref["objs"], ref["ra"]
    rtol, atol = _bounds(case, ref)
    ctx = _context(partls, monkeypatch, case)
    try:
        ctx.opt_prepare(X, y, P, eta, FAITHFUL)
        assert ctx.sweep_route() == case["route"]
        npat = ctx.num_patterns()
        r = ctx.opt_models(raw=True)
    finally:
        ctx.close()
    assert r["n_unconverged"] == 0 and len(r["pattern"]) == npat == len(objs)
    s = _scatter(r, npat)
    alpha, beta, t = _models_of(ra, P)
    d = np.linalg.norm(_fits(X, P, s["alpha"], s["beta"], s["t"]) - _fits(X, P, alpha, beta, t), axis=1).max()
    print("[tiles] %s models: max objective error %.3g, max prediction distance %.3g ||y||, %d vetoes" % (
        cid, (np.abs(s["opt"] - objs) / np.maximum(1.0, objs)).max(), d / ref["ynorm"], r["n_vetoes"]))
    np.testing.assert_allclose(s["opt"], objs, rtol=rtol, atol=atol, err_msg=cid)
    # the cleaned model is the raw one, whatever the design: cleanupResult of the device's own raw alpha
    da, db, dt = _models_of(s["raw_alpha"], P)
    _close(s["alpha"], da); _close(s["beta"], db); _close(s["t"], dt)
    if case["design"] in RANK_DEFICIENT:
        assert d <= 1e-6 * ref["ynorm"], "%s: predictions %.3g ||y|| from the oracle's" % (cid, d / ref["ynorm"])
    else:
        assert r["n_vetoes"] == 0
        _close(s["raw_alpha"], ra)
        _close(s["alpha"], alpha); _close(s["beta"], beta); _close(s["t"], t)


@pytest.mark.parametrize("cid", IDS)
def test_node_mode(partls, oracle, monkeypatch, cid):
    """bnb_bound: every leaf (free = 0) is Opt's pattern of the same bits; the root and 12 random inner nodes against the exact node
    reference; opt_finish of the winner from the sweep's exported solution (T <= 17) and from a fresh node solve"""
    case = BY_ID[cid]
    ref = _reference(oracle, case)
    X, y, P, eta, objs = ref["X"], ref["y"], ref["P"], ref["eta"], ref["objs"]
    rtol, atol = _bounds(case, ref)
    Kp = P.shape[1] + 1
    leaves = np.arange(1 << Kp, dtype=np.uint64)
    ipats, ifrees = _nodes(np.random.default_rng(case["seed"]), Kp, 12)
    fin = {}
    for mode, env in (("export", None), ("resolve", {"PARTLS_NO_EXPORT": "1"})):
        ctx = _context(partls, monkeypatch, case, env)
        try:
            ctx.opt_prepare(X, y, P, eta, FAITHFUL)
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
        print("[tiles] %s node: leaves against chain mode %.3g u y'y" % (cid, e2.max()))
        assert e2.max() <= C_TWO, "%s: leaf lb vs all_opt: %.3g u y'y at pattern %d" % (cid, e2.max(), int(np.argmax(e2)))
        np.testing.assert_allclose(lb, objs, rtol=rtol, atol=atol, err_msg=cid)
    else:
        # A feature in no group is fixed at 0 by Opt (its multiplier sum_k P[m,k] s_k is 0, Opt.jl:28-29) and left free by BnB (no branched
        # group constrains it, BnB.jl:74-79), so such a leaf is not Opt's pattern: it is the better of the two patterns that the feature's
        # sign adds once the feature sits in a group of its own.
        assert len(loose) == 1
        K = P.shape[1]
        P2 = np.asfortranarray(np.hstack([P, np.zeros((P.shape[0], 1), dtype=np.int64)]))
        P2[loose[0], K] = 1
        o2, _ = _oracle_all(oracle, X, y, P2, eta)
        b = np.arange(1 << Kp)
        b2 = (b & ((1 << K) - 1)) | ((b >> K) << (K + 1))
        leaf = np.minimum(o2[b2], o2[b2 | (1 << K)])
        print("[tiles] %s node: leaves against the oracle %.3g" % (cid, (np.abs(lb - leaf) / np.maximum(1.0, leaf)).max()))
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


@pytest.mark.parametrize("cid", IDS)
def test_batch_mode(partls, oracle, monkeypatch, cid):
    """cv_opt: 3 folds x eta = [0, 0.3] and the path in one launch (blockIdx.y = problem); every problem against the single fit(Opt) of
    its training rows (test_gpu_cv._check: status, winner, model, objective, held-out SSE from numpy) and against the oracle on them"""
    case = BY_ID[cid]
    X, y, P, _ = _problem(case, K=case["K_batch"], salt=2)
    N = X.shape[0]
    fp = np.array([0, N // 3 | 1, 2 * N // 3 | 1, N], dtype=np.int64)         # fold boundaries at odd rows
    etas = [0.0, 0.3]
    ctx = _context(partls, monkeypatch, case)
    try:
        r = ctx.cv_opt(X, y, P, fp, np.asarray(etas), FAITHFUL)
        assert ctx.sweep_route() == case["route"]
    finally:
        ctx.close()
    assert len(r["opt"]) == 8
    _check_cv(partls, oracle, X, y, P, fp, etas, FAITHFUL, r, cid)
    deficient = case["design"] in RANK_DEFICIENT
    for f in range(4):
        tr = np.ones(N, dtype=bool)
        if f < 3:
            tr[fp[f]:fp[f + 1]] = False
        Xt, yt = np.asfortranarray(X[tr]), y[tr]
        ynorm = max(1.0, float(np.linalg.norm(yt)))
        for e, eta in enumerate(etas):
            q = f * 2 + e
            tag = "%s f=%d eta=%g" % (cid, f, eta)
            assert r["status"][q] == 0, tag
            objs, ra = _oracle_all(oracle, Xt, yt, P, eta)
            b = int(np.argmin(objs))
            m = float(objs[b])
            rtol, atol = (1e-8, 2e-7 * ynorm) if deficient else (1e-9, 0.0)
            tol = rtol * max(1.0, m) + atol
            assert abs(r["opt"][q] - m) <= tol, "%s: opt %.17g, oracle %.17g" % (tag, r["opt"][q], m)
            assert objs[r["best_index"][q]] <= m + tol, "%s: best_index %d does not attain the oracle's minimum" % (tag, r["best_index"][q])
            want = _fits(Xt, P, *[np.asarray(v)[None] for v in _cleanup(ra[b], P, b)])[0]
            have = _fits(Xt, P, r["alpha"][:, q][None], r["beta"][:, q][None], r["t"][q:q + 1])[0]
            d = np.linalg.norm(have - want)
            assert d <= 1e-6 * ynorm, "%s: predictions %.3g ||y|| from the oracle's" % (tag, d / ynorm)
