"""BnB node by node: every lower bound (BnB.jl:69-92) and branch group (BnB.jl:42-57,107,117) the device returns, against the exact
per-node reference of tests/bnb_reference.py (projected NNLS on QR-compressed data, certified, objective in long double).

Whole searches (test_gpu_alt_bnb.py, test_gpu_fullsize.py, the fuzz) only see the optimum: a bound that is too loose, an overlap
variable left free instead of fixed at 0, the last maximal nu chosen instead of the first or a wrong bound on a subtree without the
optimum leave it unchanged.  Here every node of every kernel route is checked:

  route                      how                                               problems
  256-thread register        D + 1 <= 160                                      D = 15, 16, 63, 159
  512-thread register        T = 11 .. 18                                      D = 160, 255, 287
  register at T = 19 / 20    PARTLS_REG_MAXT=20                                D = 300, 319
  deferred-update            n > 288                                           D = 288, 330, 520
  deferred-update, small n   PARTLS_OPT_GENERIC_KERNEL                         D = 40
  host: generic + host nu    PARTLS_EAGER_GENERIC=1 + PARTLS_OPT_GENERIC_KERNEL D = 40
  host: cooperative, 1 node  PARTLS_EAGER_GENERIC=1                            D = 330, batches of one node

Bound error, in units of u y'y (u = 2^-53, y'y on the regularised data), e2 = lb^2 - lb_ref^2:
  |e2| <= C_TWO (both directions) and e2 <= C_UP (the direction that prunes the optimum).
Measured on the MI355X (maxima over every node of the route, cold and warm: max |e2| / max e2, in u y'y):
  256-thread register 18.9 / 13.1, 512-thread register 25.7 / 25.7, register at T = 19 / 20 17.6 / 17.6,
  deferred-update (n > 288) 25.3 / 19.6, deferred-update at small n 15.0 / 14.2, host generic + host nu 3.7 / 1.2,
  host cooperative 29.2 / 29.2.
C_TWO = 96 and C_UP = 64 sit at 3.3 and 2.2 times the worst measurement and far below the sweep's near-tie window
(1e-13 y'y = 901 u y'y).

Branch: the device's argmax must be one the reference allows when every w_j may be off by W_REL (max_i |w_i| ||x_i||) / ||x_j||
(the Gram form's accuracy in the scaled variables): the bracket [lo_k, hi_k] of each nu_k follows, -1 is allowed only when every
lo_k is 0, group k only when hi_k > 0 and hi_k >= max lo.  Nodes where more than the reference's own choice is allowed are near ties;
they are counted and must stay few (measured: 103 of the 3000-node batch on overlapping groups, 8 of the 600-node batch, 4 of the
other 1300 nodes).  Rank-deficient designs (duplicate / null column) assert lb only: w and nu are not unique there.
"""
import numpy as np
import pytest

from bnb_reference import NodeReference, U

pytestmark = pytest.mark.gpu

FAITHFUL, GENERIC = 1, 2
C_TWO = 96.0                       # |lb^2 - lb_ref^2| <= C_TWO u y'y
C_UP = 64.0                        # lb^2 - lb_ref^2 <= C_UP u y'y
W_REL = 1e-7                       # accuracy of the device's w, relative to max_i |w_i| ||x_i|| (scaled variables)
NEAR_TIE_SHARE = 0.05              # near-tie branch decisions allowed per batch


def _ctx(partls, monkeypatch, X, y, P, eta=0.0, flags=0, env=None):
    """a context prepared with OPT_FAITHFUL_INTERCEPT; environment knobs are read when a Context is created"""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    ctx = partls.Context(0)
    for k in (env or {}):
        monkeypatch.delenv(k)
    ctx.opt_prepare(X, y, P, eta, FAITHFUL | flags)
    return ctx


def _problem(seed, N, D, K, design=()):
    """(X, y, P, eta).  Groups are drawn without regard to column order (not contiguous)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    grp = rng.permutation(np.arange(D) % K)
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    w = rng.standard_normal(D)
    noise = 0.1
    if "feasible" in design:                  # the target respects one sign per group: nodes with those signs are feasible
        s = rng.choice([-1.0, 1.0], K)
        w = s[grp] * rng.uniform(0.5, 1.5, D)
        noise = 0.01
    if "scaled" in design:                    # columns from 1e-3 to 1e3
        sc = np.logspace(-3, 3, D)[rng.permutation(D)]
        X *= sc
        w /= sc
    if "overlap" in design:                   # a quarter of the features in a second group: nodes with codes 0
        ex = rng.choice(D, max(2, D // 4), replace=False)
        P[ex, (grp[ex] + 1 + rng.integers(0, K - 1, len(ex))) % K] = 1
    if "empty" in design:                     # group K-1 empty (its features join group 0); feature 0 in no group
        P[:, 0] |= P[:, K - 1]
        P[:, K - 1] = 0
        P[0, :] = 0
    if "dup" in design:                       # a duplicate column and a null column (the dependence rule)
        X[:, 1] = X[:, 0]
        X[:, 2] = 0.0
    y = X @ w + (1e3 if "offset" in design else 0.0) + noise * rng.standard_normal(N)
    eta = 0.5 if "eta" in design else 0.0
    return np.asfortranarray(X), y, P, eta


def _nodes(rng, Kp, count, feasible_pat=None):
    """root, then `count` nodes cycling through every depth 0..Kp (random branched groups, random pattern bits)"""
    full = (1 << Kp) - 1
    pats, frees = [0], [full]
    for i in range(count):
        d = i % (Kp + 1)
        br = rng.choice(Kp, d, replace=False)
        free = full & ~int(sum(1 << int(k) for k in br))
        pat = int(sum(1 << k for k in range(Kp) if rng.integers(0, 2)))
        pats.append(pat if feasible_pat is None else (feasible_pat | (pat & free)))
        frees.append(free)
    return np.array(pats, dtype=np.uint64), np.array(frees, dtype=np.uint64)


def _allowed(ref, r, i, free):
    """branches the device may return for node i of reference result r (see the module docstring)"""
    w, codes, Po, cn = r["w"][i], r["codes"][i], ref.Po, ref.cn
    scale = np.max(np.abs(w) * cn)
    err = np.where(cn > 0.0, W_REL * scale / np.where(cn > 0.0, cn, 1.0), 0.0)
    can_pos = ((codes == 1) | (codes == 2)) & (w > -err)
    can_neg = ((codes == -1) | (codes == 2)) & (w < err)
    Kp = Po.shape[1]
    lo = np.zeros(Kp)
    hi = np.zeros(Kp)
    for k in range(Kp):
        if not (free >> k) & 1:
            continue
        m = Po[:, k] != 0
        hp = np.sum((np.maximum(w, 0.0) + err)[m & can_pos])
        hn = np.sum((np.maximum(-w, 0.0) + err)[m & can_neg])
        lp = np.sum(np.maximum(w - err, 0.0)[m])
        ln = np.sum(np.maximum(-w - err, 0.0)[m])
        lo[k], hi[k] = lp * ln, hp * hn
    out = {k for k in range(Kp) if hi[k] > 0.0 and hi[k] >= lo.max()}
    if lo.max() == 0.0:
        out.add(-1)
    return out


def _check(tag, ref, r, pats, frees, lb, br, rank_deficient=False):
    """every node against the reference; returns (max |e2|, max e2, near ties) in units of u y'y"""
    assert r["certified"].all(), "%s: the reference could not certify nodes %s" % (tag, np.flatnonzero(~r["certified"])[:8])
    e2 = (lb.astype(np.longdouble) ** 2 - r["lb"].astype(np.longdouble) ** 2).astype(np.float64) / (U * ref.yy)
    worst, up = float(np.abs(e2).max()), float(e2.max())
    print("[nodes] %s: %d nodes, max |e2| %.3g u y'y, max e2 %.3g u y'y" % (tag, len(lb), worst, up))
    i = int(np.argmax(np.abs(e2)))
    assert worst <= C_TWO, "%s: |lb^2 - lb_ref^2| = %.3g u y'y > %g at node (pat %#x, free %#x): lb %.17g, ref %.17g" % (
        tag, worst, C_TWO, int(pats[i]), int(frees[i]), lb[i], r["lb"][i])
    i = int(np.argmax(e2))
    assert up <= C_UP, "%s: lb over-estimates by %.3g u y'y > %g at node (pat %#x, free %#x): lb %.17g, ref %.17g" % (
        tag, up, C_UP, int(pats[i]), int(frees[i]), lb[i], r["lb"][i])
    if rank_deficient:
        return worst, up, 0
    ties = 0
    for i in range(len(lb)):
        ok = _allowed(ref, r, i, int(frees[i]))
        assert int(br[i]) in ok, "%s: node (pat %#x, free %#x) branches on %d, reference %d (allowed %s; nu %s)" % (
            tag, int(pats[i]), int(frees[i]), int(br[i]), int(r["branch"][i]), sorted(ok), np.array2string(r["nu"][i], precision=4))
        assert int(r["branch"][i]) in ok
        ties += len(ok) > 1
    print("[nodes] %s: %d near-tie branch decisions of %d" % (tag, ties, len(lb)))
    assert ties <= max(2, NEAR_TIE_SHARE * len(lb)), "%s: %d near-tie branch decisions of %d" % (tag, ties, len(lb))
    return worst, up, ties


# ---------------------------------------------------------------------------------------------------------------------------------
# every route: root, random nodes at every depth, a batch of one node
# ---------------------------------------------------------------------------------------------------------------------------------
ROUTES = {   # id: (D, K, design, env, flags, random nodes, sweep_route(): (partls_route, tile count))
    "reg256-d15": (15, 4, ("offset", "overlap"), None, 0, 40, (1, 1)),
    "reg256-d16": (16, 5, ("empty",), None, 0, 40, (1, 2)),
    "reg256-d63": (63, 45, ("offset",), None, 0, 60, (1, 4)),
    "reg256-d159": (159, 12, ("dup",), None, 0, 30, (1, 10)),
    "reg512-d160": (160, 61, ("feasible",), None, 0, 40, (2, 11)),
    "reg512-d255": (255, 20, ("overlap", "eta"), None, 0, 30, (2, 16)),
    "reg512-d287": (287, 16, ("scaled", "offset"), None, 0, 24, (2, 18)),
    "regT19-d300": (300, 12, ("offset",), {"PARTLS_REG_MAXT": "20"}, 0, 16, (2, 19)),
    "regT20-d319": (319, 10, ("overlap", "eta"), {"PARTLS_REG_MAXT": "20"}, 0, 16, (2, 20)),
    "lazy-d288": (288, 12, ("offset",), None, 0, 16, (3, 0)),
    "lazy-d330": (330, 10, ("dup", "eta"), None, 0, 12, (3, 0)),
    "lazy-d520": (520, 8, ("scaled",), None, 0, 8, (3, 0)),
    "lazy-generic-d40": (40, 8, ("overlap", "offset"), None, GENERIC, 40, (3, 0)),
    "host-generic-d40": (40, 8, ("scaled",), {"PARTLS_EAGER_GENERIC": "1"}, GENERIC, 40, (4, 0)),
    "host-coop-d330": (330, 10, ("offset",), {"PARTLS_EAGER_GENERIC": "1"}, 0, 5, (4, 0)),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_node_bounds_and_branches(partls, monkeypatch, route):
    D, K, design, env, flags, count, kernel = ROUTES[route]
    seed = 7100 + D + K
    X, y, P, eta = _problem(seed, max(3 * D, 400), D, K, design)
    Kp = K + 1
    rng = np.random.default_rng(seed)
    feas = None
    if "feasible" in design:
        # the target's own group signs (bit k set: group k >= 0), the intercept's bit from the root's sign
        grp = np.argmax(P, axis=1)
        w0 = np.linalg.lstsq(np.column_stack([X, np.ones(len(y))]), y, rcond=None)[0]
        feas = int(sum(1 << k for k in range(K) if w0[:-1][grp == k].sum() > 0)) | (int(w0[-1] > 0) << K)
    pats, frees = _nodes(rng, Kp, count)
    if feas is not None:
        fp, ff = _nodes(rng, Kp, count // 2, feasible_pat=feas)
        pats, frees = np.concatenate([pats, fp]), np.concatenate([frees, ff])
    ctx = _ctx(partls, monkeypatch, X, y, P, eta, flags, env)
    try:
        assert ctx.sweep_route() == kernel, "%s runs on %s" % (route, ctx.sweep_route())
        if route.startswith("host-coop"):                    # one node per call: the cooperative kernel
            out = []
            for i in range(len(pats)):
                out.append(ctx.bnb_bound(pats[i:i + 1], frees[i:i + 1]))
                # pivot blocks are counted by the cooperative kernel only: 0 would mean the solve fell back to one workgroup
                assert ctx.blocks() > 0, "node %d was not solved by the cooperative kernel" % i
            lb = np.concatenate([o[0] for o in out])
            br = np.concatenate([o[1] for o in out])
        else:
            lb, br = ctx.bnb_bound(pats, frees)
            lb1, br1 = ctx.bnb_bound(pats[:1], frees[:1])    # a batch of exactly one node (the root)
    finally:
        ctx.close()
    ref = NodeReference(X, y, P, eta)
    r = ref.nodes(pats, frees)
    rank_def = "dup" in design
    _check(route, ref, r, pats, frees, lb, br, rank_def)
    if not route.startswith("host-coop"):
        _check(route + ":single", ref, {k: v[:1] for k, v in r.items()}, pats[:1], frees[:1], lb1, br1, rank_def)
    if feas is not None:
        nf = count // 2 + 1
        assert (r["branch"][-nf:] == -1).all(), "the feasible nodes are not feasible in the reference"
        assert (br[-nf:] == -1).all(), "%s: feasible nodes branch on %s" % (route, br[-nf:][br[-nf:] != -1])
    if "overlap" in design:
        assert (r["codes"] == 0).any(), "no node fixed a variable at 0"


# ---------------------------------------------------------------------------------------------------------------------------------
# leaves: node mode against chain mode on the same NNLS
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_leaf_matches_opt(partls, monkeypatch):
    """free = 0: the node is Opt's pattern with the same bits (bit k set: group k >= 0, both Opt.jl:4-20 and BnB.jl:120-121), overlap
    features with one group of each sign fixed at 0 in both.  lb == all_opt[pat] (chain mode) == opt_pattern(pat) == the reference."""
    X, y, P, eta = _problem(7201, 400, 15, 4, ("offset", "overlap"))
    Kp = 5
    pats = np.arange(1 << Kp, dtype=np.uint64)
    frees = np.zeros_like(pats)
    ctx = _ctx(partls, monkeypatch, X, y, P, eta)
    try:
        lb, br = ctx.bnb_bound(pats, frees)
        _, _, allopt, unconv = ctx.opt_sweep(0, -1, want_all=True)
        single = np.array([ctx.opt_pattern(int(p))[1] for p in pats])
    finally:
        ctx.close()
    assert unconv == 0
    ref = NodeReference(X, y, P, eta)
    r = ref.nodes(pats, frees)
    _check("leaves-d15", ref, r, pats, frees, lb, br)
    assert (br == -1).all(), "a leaf has no free group to branch on"
    for name, v in (("all_opt", allopt), ("opt_pattern", single)):
        e2 = np.abs(lb ** 2 - v ** 2) / (U * ref.yy)
        assert e2.max() <= C_TWO, "leaf lb vs %s: %.3g u y'y at pattern %d" % (name, e2.max(), int(np.argmax(e2)))
    # the opposite pattern is a different problem: the bit convention is not flipped
    flip = (~pats.astype(np.int64)) & ((1 << Kp) - 1)
    assert np.abs(lb ** 2 - allopt[flip] ** 2).max() > 1e3 * C_TWO * U * ref.yy


# ---------------------------------------------------------------------------------------------------------------------------------
# batches larger than the grid: workgroups run several nodes
# ---------------------------------------------------------------------------------------------------------------------------------
# bnb_bound_batch (solvers.hip) launches min(count, cap) workgroups, which stride over the nodes.  The register kernel's cap is
# CUs x resident workgroups per CU x PARTLS_BNB_WG_PER_CU (default 8); with the knob at 1 it is at most CUs x 3 for the 256-thread
# kernel (52.8 KB of LDS per workgroup, 160 KB per CU) and CUs x 1 for the 512-thread kernel.  The deferred-update kernel's is 2 x CUs.
BATCHES = {   # id: (D, K, flags, env, nodes, workgroups per CU at most)
    "reg256-d15": (15, 6, 0, {"PARTLS_BNB_WG_PER_CU": "1"}, 3000, 3),
    "reg512-d160": (160, 12, 0, {"PARTLS_BNB_WG_PER_CU": "1"}, 300, 1),
    "lazy-generic-d40": (40, 8, GENERIC, None, 600, 2),
}


@pytest.mark.parametrize("batch", list(BATCHES))
def test_batch_larger_than_the_grid(partls, monkeypatch, batch):
    import torch
    D, K, flags, env, count, per_cu = BATCHES[batch]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert count > ncu * per_cu, "%d nodes do not exceed the grid cap of %d workgroups: no workgroup runs two nodes" % (count, ncu * per_cu)
    route = "batch%d-%s" % (count, batch)
    X, y, P, eta = _problem(7300 + D, max(3 * D, 400), D, K, ("offset", "overlap"))
    rng = np.random.default_rng(7300 + D)
    pats, frees = _nodes(rng, K + 1, count - 1)
    ctx = _ctx(partls, monkeypatch, X, y, P, eta, flags, env)
    try:
        lb, br = ctx.bnb_bound(pats, frees)
    finally:
        ctx.close()
    ref = NodeReference(X, y, P, eta)
    _check(route, ref, ref.nodes(pats, frees), pats, frees, lb, br)


# ---------------------------------------------------------------------------------------------------------------------------------
# snapshot chains: warm bounds from the parent's slot, against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
CHAINS = {   # id: (D, K, design, flags)
    "reg256-d63": (63, 10, ("offset", "overlap"), 0),
    "reg512-d200": (200, 12, ("offset",), 0),
    "lazy-d288": (288, 8, ("offset", "overlap"), 0),
    "lazy-generic-d40": (40, 8, ("offset", "overlap"), GENERIC),
}


@pytest.mark.parametrize("pool", ["default", "1MB"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_snapshot_chain(partls, monkeypatch, chain, pool):
    """root to a leaf along the device's own branch (the lowest free group once a node is feasible), both children of every node on
    the way bounded warm from the parent's slot; every warm bound against the reference and against a cold bound of the same node.
    PARTLS_BNB_POOL_MB=1 leaves no room for a chunk of slots: dst = -1, the children start cold."""
    D, K, design, flags = CHAINS[chain]
    X, y, P, eta = _problem(7400 + D, max(3 * D, 400), D, K, design)
    Kp = K + 1
    env = {"PARTLS_BNB_POOL_MB": "1"} if pool == "1MB" else None
    ctx = _ctx(partls, monkeypatch, X, y, P, eta, flags, env)
    pats, frees, lbs, brs, srcs = [], [], [], [], []
    try:
        ctx.bnb_snap_begin()
        pat, free = 0, (1 << Kp) - 1
        lb, br, dst = ctx.bnb_bound_snap(np.array([pat], np.uint64), np.array([free], np.uint64), np.array([-1], np.int32))
        pats.append(pat); frees.append(free); lbs.append(lb[0]); brs.append(br[0]); srcs.append(-1)
        slot, b = int(dst[0]), int(br[0])
        live = [slot] if slot >= 0 else []
        step = 0
        while free:
            k = b if b >= 0 else (free & -free).bit_length() - 1
            cf = free & ~(1 << k)
            cp = np.array([pat | (1 << k), pat & ~(1 << k)], np.uint64)
            lb, br, dst = ctx.bnb_bound_snap(cp, np.array([cf, cf], np.uint64), np.array([slot, slot], np.int32))
            for j in range(2):
                pats.append(int(cp[j])); frees.append(cf); lbs.append(lb[j]); brs.append(br[j]); srcs.append(slot)
            live += [int(s) for s in dst if s >= 0]
            j = step % 2                                            # alternate >= 0 and <= 0 children down the chain
            ctx.bnb_snap_release([s for s in ([slot] if slot >= 0 else []) + [int(dst[1 - j])] if s >= 0])
            live = [s for s in live if s not in (slot, int(dst[1 - j]))]
            pat, free, slot, b = int(cp[j]), cf, int(dst[j]), int(br[j])
            step += 1
        ctx.bnb_snap_release(live)
        cold_lb, cold_br = ctx.bnb_bound(np.array(pats, np.uint64), np.array(frees, np.uint64))
    finally:
        ctx.close()
    pats, frees = np.array(pats, np.uint64), np.array(frees, np.uint64)
    lbs, brs, srcs = np.array(lbs), np.array(brs, np.int32), np.array(srcs)
    if pool == "default":
        assert (srcs[1:] >= 0).all(), "%s: a child started cold although the pool had room" % chain
    else:
        assert (srcs[1:] == -1).any(), "%s: PARTLS_BNB_POOL_MB=1 handed out every slot" % chain
    ref = NodeReference(X, y, P, eta)
    r = ref.nodes(pats, frees)
    tag = "chain-" + chain
    _check(tag + ":warm", ref, r, pats, frees, lbs, brs)
    _check(tag + ":cold", ref, r, pats, frees, cold_lb, cold_br)
    d = np.abs(lbs.astype(np.longdouble) ** 2 - cold_lb.astype(np.longdouble) ** 2).astype(np.float64) / (U * ref.yy)
    assert d.max() <= C_TWO, "%s: warm and cold bounds of node %d differ by %.3g u y'y" % (chain, int(np.argmax(d)), d.max())

