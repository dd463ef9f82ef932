"""Helpers of tests/test_gpu_context_reuse.py: the problem kinds, the generated order of the steps, the step results as dicts of
numpy arrays that are compared byte for byte, the intruders of an interrupted fit and the raw-ABI calls with sentinel-filled outputs.
Nothing here asserts a tolerance: every comparison is `diff` (dtype, shape and tobytes)."""
import ctypes as C

import numpy as np

from test_gpu_pair import context            # a Context whose knobs are exactly the given ones (read once, at partls_create)

FAITHFUL, GENERIC = 1, 2                     # PARTLS_OPT_FAITHFUL_INTERCEPT, PARTLS_OPT_GENERIC_KERNEL (include/partls.h)
SENTINEL, ISENTINEL = -7.5, -7


# ---- results ------------------------------------------------------------------------------------------------------------------------------
def flat(obj, prefix=""):
    """any nest of tuples / dicts / arrays / scalars -> {name: numpy array}"""
    out = {}
    if isinstance(obj, dict):
        for k, v in obj.items():
            out.update(flat(v, "%s%s." % (prefix, k)))
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            out.update(flat(v, "%s%d." % (prefix, i)))
    elif obj is None:
        out[prefix.rstrip(".")] = np.zeros(0)
    else:
        out[prefix.rstrip(".")] = np.asarray(obj)
    return out


def diff(got, want):
    """the names of the fields of two flat results that are not the same bytes"""
    bad = [k for k in want if k not in got or got[k].dtype != want[k].dtype or got[k].shape != want[k].shape
           or got[k].tobytes() != want[k].tobytes()]
    return bad + [k for k in got if k not in want]


def recorded(partls, fn):
    """fn()'s flat result; a refusal by the library is a result too: {status}"""
    try:
        return flat(fn())
    except partls.PartlsError as e:
        assert e.status != partls.lowlevel.ERR_HIP, e      # a HIP error is never a result
        return {"status": np.asarray(e.status)}


# ---- the order of part 1 ------------------------------------------------------------------------------------------------------------------
def euler_circuit(n):
    """An Eulerian circuit of the complete digraph with loops on n vertices (Hierholzer; every vertex has n successors and n
    predecessors): n * n + 1 vertices from 0 back to 0 in which every ordered pair, (v, v) included, is adjacent exactly once.
    Successors of v are tried in the order v + 1, v + 2, ..., v (its loop last)."""
    used = [0] * n
    stack, order = [0], []
    while stack:
        v = stack[-1]
        if used[v] < n:
            used[v] += 1
            stack.append((v + used[v]) % n)
        else:
            order.append(stack.pop())
    order.reverse()
    pairs = set(zip(order, order[1:]))
    assert len(order) == n * n + 1 and len(pairs) == n * n
    return order


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def to_csr(partls, X):
    """the CSR tuple of the nonzeros of a dense matrix"""
    N, M = X.shape
    r, c = np.nonzero(X)                                   # row-major order: sorted by row, ascending columns within a row
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))]).astype(np.int64)
    return partls.CSR(indptr, c.astype(np.int32), np.ascontiguousarray(X[r, c]), (N, M))


def sparsify(X, seed, keep=0.3):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(X * (rng.random(X.shape) < keep))


def weights_with_zeros(N, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, N)
    w[::37] = 0.0
    return w


class OnDevice:
    """arrays in HBM that stay owned by the test (adopted pointers): X with a padded leading dimension (ld = N + 3, the padding NaN),
    y, optional weights; or the three arrays of a CSR matrix"""

    def __init__(self, X=None, y=None, w=None, dtype=np.float64, csr=None):
        import torch
        self.torch = torch
        self.keep = {}
        if X is not None:
            N, M = X.shape
            self.N, self.M, self.ld = N, M, N + 3
            buf = np.full((M, self.ld), np.nan, dtype=dtype)
            buf[:, :N] = X.T
            self.keep["X"] = torch.from_numpy(buf).cuda()
        if csr is not None:
            self.N, self.M = csr.shape
            self.keep["indptr"] = torch.from_numpy(np.ascontiguousarray(csr.indptr, dtype=np.int64)).cuda()
            self.keep["indices"] = torch.from_numpy(np.ascontiguousarray(csr.indices, dtype=np.int32)).cuda()
            self.keep["data"] = torch.from_numpy(np.ascontiguousarray(csr.data, dtype=np.float64)).cuda()
        if y is not None:
            self.keep["y"] = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).cuda()
        if w is not None:
            self.keep["w"] = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda()
        torch.cuda.synchronize()

    def ptr(self, name):
        return self.keep[name].data_ptr() if name in self.keep else None


class Kind:
    """one kind of prepared problem: prepare(ctx) and what it must run on"""

    def __init__(self, name, prepare, route, flags, tiles=None, n=None):
        self.name, self.prepare, self.route, self.flags, self.tiles, self.n = name, prepare, route, flags, tiles, n
        self.faithful = bool(flags & FAITHFUL)


def make_kinds(partls, oracle):
    """the thirteen kinds of part 1, in the order of the issue's table (index i = kind i + 1), and the data they are made of"""
    from test_gpu_pair_dense import make as make_pair
    L = partls.lowlevel
    XA, yA, PA, _ = oracle.synth(20260001, 600, 20, 4)
    XB, yB, PB, _ = oracle.synth(20260002, 600, 40, 6)
    XC, yC, PC, _ = oracle.synth(20260005, 600, 30, 5)
    XL, yL, PL, _ = oracle.synth(20260011, 640, 300, 3)
    XA, XB, XC, XL = (np.asfortranarray(v) for v in (XA, XB, XC, XL))
    wA, wB, wC = weights_with_zeros(600, 20260003), weights_with_zeros(600, 20260004), weights_with_zeros(600, 20260006)
    XC32 = np.asfortranarray(XC, dtype=np.float32)
    csrB = to_csr(partls, sparsify(XB, 20260007))
    csrC = to_csr(partls, sparsify(XC, 20260008))
    devC = OnDevice(XC, yC, wC)
    devC32 = OnDevice(XC32, yC, dtype=np.float32)
    devCsr = OnDevice(y=yC, csr=csrC)
    XP, yP, PP = make_pair("full", 176)                      # n = 176, T = 11, K = 5, faithful: tests/test_gpu_pair_dense.py
    # the same X and y under another partition: group 0 gives its 16 features to group 1 and takes 12 of group 1's, so the group on
    # Gray bit 0 still fits one tile column (csrc/sweep_setup.hip: pair_rule) and the pair column is laid with other variables
    grp = np.argmax(PP, axis=1)
    assert np.all(PP.sum(axis=1) == 1)
    g0, g1 = np.flatnonzero(grp == 0), np.flatnonzero(grp == 1)
    grp[g0], grp[g1[:12]] = 1, 0
    PP2 = np.zeros_like(PP, order="F")
    PP2[np.arange(len(grp)), grp] = 1

    def host(X, y, P, eta, flags, w=None):
        return lambda ctx: ctx.opt_prepare(X, y, P, eta, flags, weights=w)

    def dev(d, P, eta, flags, dtype):
        return lambda ctx: ctx.opt_prepare_device(d.ptr("X"), d.ptr("y"), d.N, d.M, d.ld, P, eta, flags, dw_ptr=d.ptr("w"), dtype=dtype)

    kinds = [
        Kind("1 dense fp64", host(XA, yA, PA, 0.0, 0), L.ROUTE_REG_256, 0),
        Kind("2 dense fp64 weighted", host(XA, yA, PA, 0.0, FAITHFUL, wA), L.ROUTE_REG_256, FAITHFUL),
        Kind("3 float32", host(XC32, yC, PC, 0.0, 0), L.ROUTE_REG_256, 0),
        Kind("4 CSR", host(csrB, yB, PB, 0.0, FAITHFUL), L.ROUTE_REG_256, FAITHFUL),
        Kind("5 CSR weighted", host(csrB, yB, PB, 0.0, 0, wB), L.ROUTE_REG_256, 0),
        Kind("6 device fp64 padded weighted", dev(devC, PC, 0.0, FAITHFUL, np.float64), L.ROUTE_REG_256, FAITHFUL),
        Kind("7 device float32 padded eta 0.25", dev(devC32, PC, 0.25, 0, np.float32), L.ROUTE_REG_256, 0),
        Kind("8 device CSR", lambda ctx: ctx.opt_prepare_csr_device(devCsr.ptr("indptr"), devCsr.ptr("indices"), devCsr.ptr("data"),
                                                                    devCsr.ptr("y"), devCsr.N, devCsr.M, PC, 0.0, FAITHFUL),
             L.ROUTE_REG_256, FAITHFUL),
        Kind("9 eta 0.5 faithful on 1's data", host(XA, yA, PA, 0.5, FAITHFUL), L.ROUTE_REG_256, FAITHFUL),
        Kind("10 generic kernel", host(XB, yB, PB, 0.0, GENERIC), L.ROUTE_DEFERRED, GENERIC),
        Kind("11 large tableau n 301", host(XL, yL, PL, 0.0, FAITHFUL), L.ROUTE_DEFERRED, FAITHFUL, n=301),
        Kind("12 pair walk n 176", host(XP, yP, PP, 0.0, FAITHFUL), L.ROUTE_REG_512, FAITHFUL, tiles=11),
        Kind("13 pair walk, other partition", host(XP, yP, PP2, 0.0, FAITHFUL), L.ROUTE_REG_512, FAITHFUL, tiles=11),
    ]
    data = dict(A=(XA, yA, PA), B=(XB, yB, PB), C=(XC, yC, PC), wA=wA, wB=wB, csrB=csrB, pair=(XP, yP, PP),
                keep=(devC, devC32, devCsr))
    return kinds, data


SMALLEST, LARGEST = 0, 10                    # indices of kind 1 (n = 20) and kind 11 (n = 301)
SHARED = ((0, 1), (0, 8), (1, 8), (3, 4), (2, 6), (2, 5), (11, 12))   # pairs of kinds on the same X and y: their fresh results must differ


# ---- the staged Opt step ------------------------------------------------------------------------------------------------------------------
def check_route(ctx, kind):
    route, tiles = ctx.sweep_route()
    assert route == kind.route, (kind.name, route, tiles)
    if kind.tiles is not None:
        assert tiles == kind.tiles, (kind.name, tiles)


def sweep_result(ctx, kind):
    """partls_opt_sweep(want_all where the intercept is faithful) and the sweep's veto count (a later solve overwrites it)"""
    bo, bp, allo, nu = ctx.opt_sweep(want_all=kind.faithful)
    return flat(dict(best_obj=np.float64(bo), best_pattern=np.int64(bp), all_opt=allo, n_unconverged=np.int64(nu),
                     vetoes=np.int64(ctx.vetoes())))


def finish_result(ctx, pattern):
    ctx.tolerate_ill = True                  # status 9 fills the outputs: recorded, not raised
    a, b, t, opt, best = ctx.opt_finish(pattern)
    return flat(dict(alpha=a, beta=b, t=np.float64(t), opt=np.float64(opt), best_index=np.int64(best), ill=np.bool_(ctx.last_ill),
                     kkt=np.float64(ctx.kkt_violation())))


def staged_step(ctx, kind):
    """prepare, sweep, finish and the getters: everything deterministic that the headers document for a staged Opt fit"""
    kind.prepare(ctx)
    check_route(ctx, kind)
    if kind.n is not None:
        assert ctx.gram().shape[0] == kind.n + 1             # (M + 2: the augmented Gram of n - 1 features)
    res = {"sweep." + k: v for k, v in sweep_result(ctx, kind).items()}
    bp = int(res["sweep.best_pattern"])
    assert bp >= 0, kind.name
    res.update({"finish." + k: v for k, v in finish_result(ctx, bp).items()})
    g, fc = ctx.bit_order()
    res.update(flat(dict(gram=ctx.gram(), gbit=g, flip_cost=fc, num_patterns=np.int64(ctx.num_patterns()))))
    check_route(ctx, kind)
    return res


# ---- raw ABI with sentinel-filled outputs ---------------------------------------------------------------------------------------------------
def _d(n=1):
    return np.full(n, SENTINEL)


def _i(n=1, dtype=np.int64):
    return np.full(n, ISENTINEL, dtype=dtype)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def unwritten(outs):
    return all(np.all(o == (SENTINEL if o.dtype == np.float64 else ISENTINEL)) for o in outs)


RAW_SHAPE = (640, 302, 8)                    # N, M, K no smaller than any problem's here: a call that wrongly succeeds stays inside its outputs


def raw_staged_calls(partls, ctx, N, M, K):
    """every staged entry through the C ABI itself, each with outputs filled with a sentinel: [(name, status, outputs)]"""
    from test_gpu_diagnostics import _raw_call
    lib = partls.lowlevel.lib()
    h = ctx._h
    B, k = 4, 3
    calls = []
    o = [_d(), _i(), _d(1 << (K + 1)), _i()]
    calls.append(("opt_sweep", lib.partls_opt_sweep(h, 0, -1, _dp(o[0]), _ip(o[1]), _dp(o[2]), _ip(o[3])), o))
    o = [_d(M), _d(K), _d(), _d(), _i()]
    calls.append(("opt_finish", lib.partls_opt_finish(h, 0, _dp(o[0]), _dp(o[1]), _dp(o[2]), _dp(o[3]), _ip(o[4])), o))
    o = [_i(B), _d(B), _d(B * (M + 1)), _d(B * M), _d(B * K), _d(B), _i(), _i()]
    calls.append(("opt_models", lib.partls_opt_models(h, 0, B, _ip(o[0]), _dp(o[1]), _dp(o[2]), M + 1, _dp(o[3]), M, _dp(o[4]), K,
                                                      _dp(o[5]), _ip(o[6]), _ip(o[7])), o))
    o = [_i(k), _d(k), _d(k * (M + 1)), _d(k * M), _d(k * K), _d(k), _i(), _i(), _i()]
    calls.append(("opt_top", lib.partls_opt_top(h, 0, -1, k, _ip(o[0]), _dp(o[1]), _dp(o[2]), M + 1, _dp(o[3]), M, _dp(o[4]), K,
                                                _dp(o[5]), _ip(o[6]), _ip(o[7]), _ip(o[8])), o))
    st, o = _raw_call(partls, ctx, np.full(M, 0.5), np.ones(K), 0.25, N, M, K)
    calls.append(("diagnostics", st, o))
    a0, b0 = np.full(M + 1, 0.5), np.ones(K + 1)
    o = [_d(M), _d(K), _d(), _d(), _i()]
    calls.append(("alt_prepared", lib.partls_alt_prepared(h, 1e-6, 5, _dp(a0), _dp(b0), _dp(o[0]), _dp(o[1]), _dp(o[2]), _dp(o[3]),
                                                          _ip(o[4])), o))
    o = [_d(M), _d(K), _d(), _d(), _i()]
    calls.append(("bnb_prepared", lib.partls_bnb_prepared(h, _dp(o[0]), _dp(o[1]), _dp(o[2]), _dp(o[3]), _ip(o[4])), o))
    return calls


def raw_predict_many(partls, ctx, X, P, alpha, beta, t, B):
    """partls_predict_many with the model count given separately (B = 0 is refused) -> (status, yhat filled with a sentinel)"""
    X = np.asfortranarray(X, dtype=np.float64)
    P = np.asfortranarray(P, dtype=np.int64)
    N, M = X.shape
    a, b, tv = (np.ascontiguousarray(v, dtype=np.float64) for v in (alpha, beta, t))
    yh = _d(N * max(B, 1))
    st = partls.lowlevel.lib().partls_predict_many(ctx._h, X.ctypes.data, N, M, N, 0, P.ctypes.data, P.shape[1], M, B, _dp(a), _dp(b),
                                                   _dp(tv), yh.ctypes.data, N, 0, None, None, None)
    return st, yh


# ---- the intruders of part 2 --------------------------------------------------------------------------------------------------------------
class Query:
    """a prediction set of another shape and another partition than any base problem's, and five models over it"""
    N, M, K, B = 257, 13, 3, 5

    def __init__(self, partls):
        rng = np.random.default_rng(20260021)
        self.X = np.asfortranarray(rng.standard_normal((self.N, self.M)))
        self.X32 = np.asfortranarray(self.X, dtype=np.float32)
        self.P = np.zeros((self.M, self.K), dtype=np.int64)
        self.P[np.arange(self.M), (np.arange(self.M) * 2) % self.K] = 1
        self.alpha = rng.uniform(0.1, 1.0, (self.B, self.M))
        self.beta = rng.uniform(-1.0, 1.0, (self.B, self.K))
        self.t = rng.uniform(-1.0, 1.0, self.B)
        self.csr = to_csr(partls, sparsify(self.X, 20260022))
        self.obj = rng.uniform(1.0, 2.0, 8)
        self.obj[[2, 5]] = np.nan, self.obj[0]                 # a capped pattern and an exact tie
        self.dev = OnDevice(self.X)
        self.dyhat = self.dev.torch.zeros(self.N, dtype=self.dev.torch.float64, device="cuda")

    def predict_device(self, ctx):
        torch = self.dev.torch
        self.dyhat.fill_(SENTINEL)
        torch.cuda.synchronize()
        ctx.predict_device(self.dev.ptr("X"), self.N, self.M, self.dev.ld, self.P, self.alpha[1], self.beta[1], self.t[1],
                           self.dyhat.data_ptr())
        torch.cuda.synchronize()
        return self.dyhat.cpu().numpy()


class Base:
    """a base problem of part 2 and what the intruders need of its uninterrupted fresh run"""

    def __init__(self, name, kind, env, M, K):
        self.name, self.kind, self.env, self.M, self.K = name, kind, env, M, K
        rng = np.random.default_rng(20260023 + M)
        self.a0, self.b0 = rng.uniform(0.1, 1.0, (3, M + 1)), rng.uniform(-1.0, 1.0, (3, K + 1))
        self.winner, self.model = None, None                 # set from the fresh run


def intruders(q):
    """name -> (kind, call(ctx, base)); "pure": the headers promise that the prepared problem or the sweep's state stays untouched;
    "solve": a single solve on the prepared problem"""
    full = lambda b: (1 << (b.K + 1)) - 1

    def bnb_nodes(b):
        f = full(b)
        return [0, 0, 1, 2], [f, f & ~1, f & ~1, f & ~3]

    def snapshots(ctx, b):
        f = full(b)
        ctx.bnb_snap_begin()
        lb0, br0, dst0 = ctx.bnb_bound_snap([0], [f], [-1])
        k = max(int(br0[0]), 0)
        lb1, br1, dst1 = ctx.bnb_bound_snap([0, 1 << k], [f & ~(1 << k)] * 2, [int(dst0[0])] * 2)
        ctx.bnb_snap_release([int(s) for s in list(dst0) + list(dst1) if s >= 0])
        return lb0, br0, dst0, lb1, br1, dst1

    return {
        "predict": ("pure", lambda ctx, b: (ctx.predict(q.X, q.P, q.alpha[0], q.beta[0], q.t[0]),
                                            ctx.predict(q.X32, q.P, q.alpha[2], q.beta[2], q.t[2]))),
        "predict_device": ("pure", lambda ctx, b: q.predict_device(ctx)),
        "predict_csr": ("pure", lambda ctx, b: ctx.predict_csr(q.csr, q.P, q.alpha[3], q.beta[3], q.t[3])),
        "predict_many": ("pure", lambda ctx, b: ctx.predict_many(q.X, q.P, q.alpha, q.beta, q.t, ranks=[0, 2, 4], want_mean=True)),
        "contributions": ("pure", lambda ctx, b: ctx.contributions(q.X, q.P, q.alpha[:3], q.beta[:3], ranks=[1], want_mean=True,
                                                                   want_sums=True)),
        "diagnostics": ("pure", lambda ctx, b: ctx.diagnostics(*b.model)),
        "opt_models partial": ("pure", lambda ctx, b: ctx.opt_models(3, 11, raw=True)),
        "opt_models full": ("pure", lambda ctx, b: ctx.opt_models()),
        "opt_top partial": ("pure", lambda ctx, b: ctx.opt_top(5, 3, 11)),
        "opt_top full": ("pure", lambda ctx, b: ctx.opt_top(5, raw=True)),
        "opt_top_select": ("pure", lambda ctx, b: ctx.opt_top_select(q.obj, 2, 3)),
        "opt_candidates": ("pure", lambda ctx, b: ctx.opt_candidates()),
        "gram": ("pure", lambda ctx, b: ctx.gram()),
        "bit_order": ("pure", lambda ctx, b: ctx.bit_order()),
        "opt_pattern": ("solve", lambda ctx, b: ctx.opt_pattern(b.winner ^ 1)),
        "alt_prepared": ("solve", lambda ctx, b: ctx.alt_prepared(b.a0[0], b.b0[0], eps=1e-6, T=20)),
        "alt_multistart": ("solve", lambda ctx, b: ctx.alt_multistart(b.a0, b.b0, eps=1e-6, T=20)),
        "bnb_prepared": ("solve", lambda ctx, b: ctx.bnb_prepared()),
        "bnb_bound": ("solve", lambda ctx, b: ctx.bnb_bound(*bnb_nodes(b))),
        "bnb_leaf": ("solve", lambda ctx, b: ctx.bnb_leaf(b.winner, 0)),
        "bnb_search": ("solve", lambda ctx, b: ctx.bnb_search(0)),
        "bnb snapshots": ("solve", snapshots),
    }
