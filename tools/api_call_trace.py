"""What the Python binding hands to the library, as text: a fake library object stands in for libpartls_hip.so, every call is written
down as one canonical line, and a fixed list of cases drives fit / predict / cross_validate / Context / Frontier / MultiContext through it.
Needs no GPU and no built library.

    python tools/api_call_trace.py                       # the trace of partitionedls.jl_amd/api.py, to stdout
    python tools/api_call_trace.py --api OTHER/api.py    # the same cases through another copy of api.py (e.g. the parent commit's)
    python tools/api_call_trace.py -o tests/golden/api_call_trace.txt

A line is `symbol(arg, ...) -> status`: scalars by value, handles by the order of their creation (c1, m1, m1.r0, f1), input arrays as
`name[count]=<first 8 hex digits of the sha1 of their bytes>` with the count taken from the call's own scalar arguments (from the handle's
last prepare where the call carries none), device addresses by value, output pointers as `out`, null pointers as `NULL`.  The fake
writes nothing to the outputs except the scalars control flow reads (handles, partls_opt_num_patterns, the sweep's best_pattern,
n_unconverged = 0, partls_multi_size, the round size of partls_frontier_next, partls_opt_top's patterns and counts) and returns FakeLib.status[symbol] (default 0).
partls_destroy and its kin are not written down: most of them run from __del__, when the garbage collector pleases.
tests/test_api_call_trace.py compares the trace with tests/golden/api_call_trace.txt."""
import argparse
import contextlib
import ctypes as C
import functools
import hashlib
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import partls_amd  # noqa: E402

# one token per parameter.  h: handle; out: output pointer; NAME: scalar; NAME:code:count: input array (d double, x the element type of
# X, q int64, i int32, Q uint64, c int; X, y and w are addresses when the call's `dev` is 1); NAME:@: device address
_XY = "X:x:ldX*M N M ldX y:d:N"
_P = "P:q:ldP*K K ldP"
_OUT5 = "out out out out out"
_CV = "fold_ptr:q:F+1 F etas:d:E E flags out ld_alpha out ld_beta out out out out out"
_PREDICT = "h X:%s N M ldX " + _P + " alpha:d:M beta:d:K t %s"
_PREDICT_MANY = "h X:x:ldX*M N M ldX dev " + _P + " B alpha:d:M*B beta:d:K*B t:d:B yhat:@ ldY nr ranks:q:nr stats:@ mean:@"
_CONTRIB = "h X:x:ldX*M N M ldX dev " + _P + " B alpha:d:lda*B lda beta:d:ldb*B ldb contrib:@ ldC nr ranks:q:nr stats:@ mean:@ out"
SPEC = {
    "partls_version": "", "partls_last_error": "", "partls_device_count": "",
    "partls_create": "device out", "partls_destroy": "h",
    "partls_fit_opt": f"h {_XY} {_P} eta flags {_OUT5} out",
    "partls_multi_create": "devices:c:n n out", "partls_multi_destroy": "h", "partls_multi_size": "h", "partls_multi_uses_rccl": "h",
    "partls_multi_context": "h rank",
    "partls_fit_opt_multi": f"h {_XY} {_P} eta flags {_OUT5} out",
    "partls_fit_bnb_multi": f"h {_XY} {_P} eta {_OUT5}",
    "partls_multi_get_timing": "h rank which out",
    "partls_opt_prepare": f"h {_XY} dev {_P} eta flags",
    "partls_opt_prepare_weighted": f"h {_XY} w:d:N dev {_P} eta flags",
    "partls_opt_prepare_f32": f"h {_XY} w:d:N dev {_P} eta flags",
    "partls_opt_sweep": "h g_begin g_end out out out out",
    "partls_opt_finish": f"h pattern {_OUT5}",
    "partls_opt_candidates": "h cap out out out",
    "partls_opt_merge_candidates": "h n objs:d:n pats:q:n out out",
    "partls_opt_pattern": "h pattern out out",
    "partls_opt_models": "h g_begin g_end out out out ld_raw out ld_alpha out ld_beta out out out",
    "partls_opt_top": "h g_begin g_end k out out out ld_raw out ld_alpha out ld_beta out out out out",
    "partls_opt_top_select": "h obj:d:cnt cnt g0 k out out out out",
    "partls_cv_opt": f"h {_XY} dev {_P} {_CV}",
    "partls_cv_opt_weighted": f"h {_XY} w:d:N dev {_P} {_CV}",
    "partls_opt_weightings": f"h {_XY} dev {_P} w:d:ldW*B ldW B eta flags out ld_alpha out ld_beta out out out out out out",
    "partls_opt_num_patterns": "h", "partls_opt_bit_order": "h out out",
    "partls_fit_alt": f"h {_XY} {_P} eta eps T alpha0:d:M+1 beta0:d:K+1 {_OUT5}",
    "partls_fit_bnb": f"h {_XY} {_P} eta {_OUT5}",
    "partls_alt_prepared": f"h eps T alpha0:d:M+1 beta0:d:K+1 {_OUT5}",
    "partls_bnb_prepared": f"h {_OUT5}",
    "partls_alt_multistart": f"h eps T R alpha0s:d:R*lda lda beta0s:d:R*ldb ldb {_OUT5} out out ld_alpha out ld_beta out out out out",
    "partls_cv_alt": f"h {_XY} w:d:N dev {_P} fold_ptr:q:F+1 F etas:d:E E flags eps T R alpha0s:d:R*lda lda beta0s:d:R*ldb ldb "
                     "out ld_alpha out ld_beta out out out out out out out out out",
    "partls_bnb_bound": "h n pats:Q:n frees:Q:n out out",
    "partls_bnb_snap_begin": "h",
    "partls_bnb_bound_snap": "h n pats:Q:n frees:Q:n src:i:n out out out",
    "partls_bnb_snap_release": "h n slots:i:n",
    "partls_frontier_create": "n_groups rank world batch out", "partls_frontier_destroy": "h",
    "partls_frontier_next": "h out out out out out out",
    "partls_frontier_ingest": "h lb:d:total branch:i:total dst:i:total out cap out",
    "partls_frontier_result": "h out out out out",
    "partls_bnb_search": "h max_nodes out out out out",
    "partls_bnb_leaf": "h pat free out out out out",
    "partls_predict": _PREDICT % ("x:ldX*M", "out"), "partls_predict_f32": _PREDICT % ("x:ldX*M", "out"),
    "partls_predict_device": _PREDICT % ("@", "yhat:@"), "partls_predict_device_f32": _PREDICT % ("@", "yhat:@"),
    "partls_predict_many": _PREDICT_MANY, "partls_predict_many_f32": _PREDICT_MANY,
    "partls_contributions": _CONTRIB, "partls_contributions_f32": _CONTRIB,
    "partls_diagnostics": "h alpha:d:M beta:d:K t out out out out out out out out out", "partls_get_diagnostics_timing": "h out out out",
    "partls_synth_truth": "seed D K out out",
    "partls_synth_device": "h seed N D wstar:d:D X:@ y:@",
    "partls_get_timing": "h which out", "partls_get_upload": "h out out", "partls_get_gram": "h out", "partls_get_pivots": "h out",
    "partls_get_vetoes": "h out", "partls_get_blocks": "h out", "partls_get_kkt_violation": "h out out", "partls_get_near_ties": "h out",
    "partls_get_sweep_route": "h out out", "partls_get_rescue_stats": "h out out out",
}
_DTYPES = {"d": np.float64, "q": np.int64, "i": np.int32, "Q": np.uint64, "c": np.intc}
_UNRECORDED = ("partls_destroy", "partls_multi_destroy", "partls_frontier_destroy")
ROUND = 3                      # nodes the fake frontier deals per round (all to this rank)


def _addr(a):
    """the address a pointer argument carries, in whichever form ctypes takes one (0: null)"""
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, C.c_void_p):
        return a.value or 0
    if isinstance(a, C.Array):
        return C.addressof(a)
    if hasattr(a, "_obj"):                                   # C.byref(x)
        return C.addressof(a._obj)
    return C.cast(a, C.c_void_p).value or 0                  # a typed pointer (ndarray.ctypes.data_as)


def _scalar(a, argtype):
    v = a.value if isinstance(a, C._SimpleCData) else a
    return float(v) if argtype is C.c_double else int(v)


class FakeLib:
    def __init__(self, lowlevel):
        self.lines = []
        self.status = {}               # symbol -> status it returns (default 0)
        self.best_pattern = 1          # what partls_opt_sweep reports
        self.top_vetoes = 0            # what partls_opt_top reports in n_vetoes
        self.names = {}                # handle -> c1 / m1 / m1.r0 / f1
        self.state = {}                # handle -> the scalars later calls on it are sized by (M, K, npat; total of a frontier round)
        self.ranks = {}                # multi handle -> its rank handles
        symbols = lowlevel.SYMBOLS + lowlevel.SYMBOLS_F32 + lowlevel.SYMBOLS_F32_MORE + lowlevel.SYMBOLS_CONTRIB + lowlevel.SYMBOLS_DIAG
        assert {s[0] for s in symbols} == set(SPEC), "SPEC and the symbol tables disagree"
        for name, res, argtypes in symbols:
            assert len(SPEC[name].split()) == len(argtypes), name
            setattr(self, name, functools.partial(self._call, name, argtypes))

    def note(self, text):
        self.lines.append(text)

    @contextlib.contextmanager
    def scripted(self, **status):
        self.status.update(status)
        try:
            yield
        finally:
            for k in status:
                del self.status[k]

    def _handle(self, prefix, **state):
        h = 0x1000 + 0x10 * len(self.names)
        self.names[h] = prefix if "." in prefix else "%s%d" % (prefix, 1 + sum(n[0] == prefix and "." not in n for n in self.names.values()))
        self.state[h] = state
        return h

    def _array(self, tok, a, env, f32):
        name, code, *count = tok.split(":")
        addr = _addr(a)
        if not addr:
            return name + "=NULL"
        if code == "@" or (env.get("dev") and name in ("X", "y", "w")):
            return "%s=@%#x" % (name, addr)
        n = int(eval(count[0], {}, env))
        dtype = (np.float32 if f32 else np.float64) if code == "x" else _DTYPES[code]
        raw = C.string_at(addr, n * np.dtype(dtype).itemsize)
        return "%s[%d]=%s" % (name, n, hashlib.sha1(raw).hexdigest()[:8])

    def _call(self, name, argtypes, *args):
        toks = SPEC[name].split()
        assert len(args) == len(toks), (name, len(args))
        h = _addr(args[0]) if toks[:1] == ["h"] else 0
        env = dict(self.state.get(h, {}))
        for tok, a, ty in zip(toks, args, argtypes):
            if ":" not in tok and tok not in ("h", "out"):
                env[tok] = _scalar(a, ty)
        parts = []
        for tok, a in zip(toks, args):
            if tok == "h":
                parts.append(self.names.get(_addr(a), "NULL"))
            elif tok == "out":
                parts.append("out" if _addr(a) else "NULL")
            elif ":" in tok:
                parts.append(self._array(tok, a, env, name.endswith("_f32")))
            else:
                parts.append("%s=%r" % (tok, env[tok]))
        ret = self._effect(name, h, env, args)
        if name not in _UNRECORDED:
            self.lines.append("%s(%s) -> %s" % (name, ", ".join(parts), self.names.get(ret, ret) if name == "partls_multi_context" else ret))
        return ret

    def _effect(self, name, h, env, args):
        """the few things control flow reads, and the return value"""
        if name in ("partls_opt_prepare", "partls_opt_prepare_weighted", "partls_opt_prepare_f32", "partls_fit_opt", "partls_fit_alt",
                    "partls_fit_bnb", "partls_fit_opt_multi", "partls_fit_bnb_multi", "partls_cv_opt", "partls_cv_opt_weighted",
                    "partls_opt_weightings"):
            faithful = env.get("flags", 1) & 1               # partls_fit_alt / _bnb prepare with OPT_FAITHFUL_INTERCEPT
            for hh in [h] + self.ranks.get(h, []):
                self.state[hh] = dict(M=env["M"], K=env["K"], npat=1 << (env["K"] + faithful))
        if name == "partls_create":
            args[1]._obj.value = self._handle("c")
        elif name == "partls_frontier_create":
            args[4]._obj.value = self._handle("f", total=0)
        elif name == "partls_multi_create":
            m = self._handle("m")
            self.ranks[m] = [self._handle("%s.r%d" % (self.names[m], r)) for r in range(env["n"] or 2)]    # no list: two visible devices
            args[2]._obj.value = m
        elif name == "partls_multi_size":
            return len(self.ranks[h])
        elif name == "partls_multi_context":
            return self.ranks[h][env["rank"]] if 0 <= env["rank"] < len(self.ranks[h]) else None
        elif name == "partls_opt_num_patterns":
            return env.get("npat", 0)
        elif name == "partls_opt_sweep":
            args[4]._obj.value, args[6]._obj.value = self.best_pattern, 0
        elif name == "partls_opt_top":                       # patterns 0, 1, ... of the range, as many as it holds up to k
            g_end = env["g_end"] if env["g_end"] >= 0 else env.get("npat", 0)
            got = max(0, min(env["k"], g_end - env["g_begin"]))
            for i in range(got):
                args[4][i] = i
            args[13]._obj.value, args[14]._obj.value, args[15]._obj.value = got, 0, self.top_vetoes
        elif name == "partls_frontier_next":
            args[1]._obj.value = args[2]._obj.value = self.state[h]["total"] = ROUND
        elif name == "partls_last_error":
            return b"scripted status"
        elif name == "partls_version":
            return 103
        elif name in ("partls_device_count", "partls_multi_uses_rccl"):
            return 1 if name == "partls_device_count" else 0
        elif name in _UNRECORDED:
            return None
        return self.status.get(name, 0)


def load_api(path=None):
    """the api module of the package, or another copy of api.py loaded beside it (its relative imports find the same _lib)"""
    pkg = partls_amd.package()
    if path is None:
        return pkg.api
    spec = importlib.util.spec_from_file_location(pkg.__name__ + "._api_traced", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def fake_library(api):
    """FakeLib in place of the loaded library, and fresh default contexts, for the duration of the block.  Whatever context was made
    inside is closed on the way out, while its handle still means something to the library that made it."""
    L = partls_amd.package().lowlevel
    fake = FakeLib(L)
    saved = L._lib, api._default_ctx, api._default_multi
    before = set(api._live_contexts)
    L._lib, api._default_ctx, api._default_multi = fake, {}, {}
    try:
        yield fake
    finally:
        for c in [c for c in api._live_contexts if c not in before]:
            c.close()
        L._lib, api._default_ctx, api._default_multi = saved


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def problem():
    """N = 12, M = 3, K = 2: X in both dtypes and three layouts, y, P, weights"""
    rng = np.random.default_rng(0)
    big = rng.normal(size=(24, 6))
    X = {}
    for dt in (np.float64, np.float32):
        b = big.astype(dt)
        X[dt, "F"], X[dt, "C"], X[dt, "strided"] = np.asfortranarray(b[:12, :3]), np.ascontiguousarray(b[:12, :3]), b[::2, ::2]
    return X, rng.normal(size=12), np.array([[1, 0], [1, 0], [0, 1]]), np.arange(1.0, 13.0) / 4


FINISHERS = dict(partls_opt_finish=9, partls_fit_alt=9, partls_alt_prepared=9, partls_alt_multistart=9, partls_fit_bnb=9,
                 partls_bnb_prepared=9, partls_fit_opt_multi=9, partls_fit_bnb_multi=9)


def run_cases(api, fake):
    Xs, y, P, w = problem()
    X64, X32 = Xs[np.float64, "F"], Xs[np.float32, "F"]
    M, K = 3, 2
    algs = (api.Opt, api.Alt, api.BnB)

    def case(title, fn, *a, **kw):
        """one call: its title, the library calls it made, what it raised and the warnings it gave"""
        fake.note("# " + title)
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter("always")
            try:
                out = fn(*a, **kw)
            except Exception as e:
                fake.note("raised %s: %s" % (type(e).__name__, e))
                out = None
        for wn in ws:
            fake.note("warned %s" % wn.category.__name__)
        return out

    def fit(title, alg, X, **kw):
        if alg is api.Alt and not ({"alpha0", "rng"} & set(kw)):
            kw["rng"] = 3
        return case("fit %s %s" % (alg.__name__, title), api.fit, alg, X, y, P, **kw)

    for alg in algs:
        for (dt, layout), X in Xs.items():
            for wt in (None, w):
                fit("%s %s weights=%s" % (np.dtype(dt).name, layout, wt is not None), alg, X, η=0.5, weights=wt)
        for dt in (np.float64, np.float32):
            fit("%s devices=[0, 0]" % np.dtype(dt).name, alg, Xs[dt, "C"], devices=[0, 0], eta=0.25)
        for opt in ("faithful_intercept", "generic_kernel"):
            fit(opt, alg, X64, **{opt: True})
            fit(opt + " float32 weighted", alg, X32, weights=w, **{opt: True})
        for on_ill in ("warn", "raise"):
            with fake.scripted(**FINISHERS):
                fit("status 9 %s" % on_ill, alg, X64, on_ill_conditioned=on_ill)
                fit("status 9 %s float32" % on_ill, alg, X32, on_ill_conditioned=on_ill)
                fit("status 9 %s devices=[0, 0]" % on_ill, alg, X64, on_ill_conditioned=on_ill, devices=[0, 0])
    with fake.scripted(partls_opt_sweep=6):
        fit("status 6 from the sweep", api.Opt, X64)
    a1, b1 = np.linspace(0.1, 0.9, M + 1), np.linspace(-1.0, 1.0, K + 1)
    a2, b2 = np.random.default_rng(1).random((3, M + 1)), np.random.default_rng(2).random((3, K + 1)) - 0.5
    for X in (X64, X32):
        fit("restarts=3 rng=7", api.Alt, X, restarts=3, rng=7, ϵ=1e-4, T=7)
        fit("rng=Generator", api.Alt, X, rng=np.random.default_rng(7))
        fit("1-D starts", api.Alt, X, alpha0=a1, beta0=b1)
        fit("2-D starts", api.Alt, X, alpha0=a2, beta0=b2, weights=w)
        with fake.scripted(**FINISHERS):
            fit("status 9 warn restarts=2", api.Alt, X, restarts=2, rng=1)

    def walk(title, s):
        case(title + " [1], [-1]", lambda: (s[1], s[-1]))
        case(title + " blocks(3)", lambda: list(s.blocks(3)))
        case(title + " arrays()", s.arrays)

    for title, kw in (("float64", {}), ("float32 weighted", dict(weights=w)), ("devices=[0, 0]", dict(devices=[0, 0]))):
        X = X32 if "float32" in title else X64
        s = fit("returnAllSolutions " + title, api.Opt, X, returnAllSolutions=True, η=0.5, **kw)[2].solutions
        walk("solutions %s" % title, s)
        fit("another fit takes the shared context", api.Opt, Xs[np.float64, "C"], **({"devices": [0, 0]} if "devices" in kw else {}))
        walk("solutions %s afterwards" % title, s)

    for kw in (dict(nfolds=3), dict(nfolds=0), dict(nfolds=4, shuffle=True, rng=5), dict(nfolds=3, weights=w),
               dict(nfolds=3, shuffle=True, rng=np.random.default_rng(5), weights=w, η=[0.0, 0.5, 2.0], faithful_intercept=True),
               dict(nfolds=2, eta=[0.1, 1.0], generic_kernel=True)):
        for X in (Xs[np.float64, "strided"], Xs[np.float32, "C"]):
            case("cross_validate %s %s" % (X.dtype.name, sorted(kw)), api.cross_validate, api.Opt, X, y, P, **kw)

    model = api.PartLSFitResult(np.array([0.5, 0.25, 1.0]), np.array([2.0, -1.0]), 0.5, P)
    for (dt, layout), X in Xs.items():
        case("predict %s %s" % (np.dtype(dt).name, layout), api.predict, model, X)
    case("predict five arguments", api.predict, model.α, model.β, model.t, P, X32)
    dX, dy, dw, dyh = 0x7f0000001000, 0x7f0000002000, 0x7f0000003000, 0x7f0000004000
    for dt in (np.float64, np.float32):
        case("predict_device %s" % np.dtype(dt).name, api.predict_device, model, dX, 12, 16, dyh, dtype=dt)

    ctx = api.Context(0)
    for dt in (np.float64, np.float32):
        for wp in (None, dw):
            case("opt_prepare_device %s dw_ptr=%s" % (np.dtype(dt).name, wp is not None), ctx.opt_prepare_device, dX, dy, 12, M, 16, P, 0.5,
                 1, dw_ptr=wp, dtype=dt)
    case("Context.predict_device", ctx.predict_device, dX, 12, M, 16, P, model.α, model.β, 0.5, dyh, dtype=np.float32)
    for ptrs in ((dX, dy, 12, 16), (dX, dy, 12, 16, None), (dX, dy, 12, 16, dw)):
        case("cv_opt device_ptrs of length %d" % len(ptrs), ctx.cv_opt, None, None, P, [0, 4, 8, 12], [0.0, 1.0], 1, device_ptrs=ptrs)
    case("cv_opt host", ctx.cv_opt, Xs[np.float32, "C"], y, P, None, 0.5)
    case("cv_opt host weighted", ctx.cv_opt, Xs[np.float64, "C"], y, P, [0, 6, 12], [0.5], weights=w)
    case("cv_opt weights with device_ptrs", ctx.cv_opt, None, None, P, None, 0.5, device_ptrs=(dX, dy, 12, 16), weights=w)
    case("opt_prepare host weighted", ctx.opt_prepare, Xs[np.float64, "strided"], y, P, 0.5, 1, weights=w.astype(np.float32))
    case("opt_prepare weights of the wrong length", ctx.opt_prepare, X64, y, P, weights=w[:5])
    for title, fn, a in (("num_patterns", ctx.num_patterns, ()), ("bit_order", ctx.bit_order, ()), ("opt_sweep", ctx.opt_sweep, (2, 6, True)),
                         ("opt_finish", ctx.opt_finish, (5,)), ("opt_candidates", ctx.opt_candidates, ()),
                         ("opt_merge_candidates", ctx.opt_merge_candidates, ([3.0, 1.5], [4, 2])),
                         ("near_ties_evaluated", ctx.near_ties_evaluated, ()), ("opt_pattern", ctx.opt_pattern, (3,)),
                         ("opt_models", ctx.opt_models, (1, 7, True)), ("opt_models all", ctx.opt_models, ()),
                         ("alt_prepared", ctx.alt_prepared, (a1, b1, 1e-5, 9)), ("alt_multistart", ctx.alt_multistart, (a2, b2, 1e-5, 9)),
                         ("bnb_prepared", ctx.bnb_prepared, ()), ("bnb_bound empty", ctx.bnb_bound, ([], [])),
                         ("bnb_bound", ctx.bnb_bound, ([1, 2, 3], [4, 4, 0])), ("bnb_snap_begin", ctx.bnb_snap_begin, ()),
                         ("bnb_bound_snap empty", ctx.bnb_bound_snap, ([], [], [])),
                         ("bnb_bound_snap", ctx.bnb_bound_snap, ([1, 2], [4, 0], [-1, 3])),
                         ("bnb_snap_release empty", ctx.bnb_snap_release, ([],)), ("bnb_snap_release", ctx.bnb_snap_release, ([3, 1],)),
                         ("bnb_search", ctx.bnb_search, (100,)), ("bnb_leaf", ctx.bnb_leaf, (5, 2)), ("timing", ctx.timing, (2,)),
                         ("upload", ctx.upload, ()), ("pivots", ctx.pivots, ()), ("vetoes", ctx.vetoes, ()), ("blocks", ctx.blocks, ()),
                         ("sweep_route", ctx.sweep_route, ()), ("kkt_violation", ctx.kkt_violation, ()), ("min_pivot", ctx.min_pivot, ()),
                         ("gram", ctx.gram, ()), ("synth_device", ctx.synth_device, (9, 12, M, [1.0, 2.0, 3.0], dX, dy))):
        case("Context." + title, fn, *a)
    with fake.scripted(**FINISHERS, partls_bnb_leaf=9):
        for tol in (False, True):
            ctx.tolerate_ill = tol
            for title, fn, a in (("opt_finish", ctx.opt_finish, (0,)), ("alt_prepared", ctx.alt_prepared, (a1, b1)),
                                 ("alt_multistart", ctx.alt_multistart, (a2, b2)), ("bnb_prepared", ctx.bnb_prepared, ()),
                                 ("bnb_leaf", ctx.bnb_leaf, (1, 0))):
                case("Context.%s with status 9, tolerate_ill=%s" % (title, tol), fn, *a)
                fake.note("last_ill=%s" % ctx.last_ill)
    with fake.scripted(partls_alt_multistart=6):
        case("Context.alt_multistart no start finished", ctx.alt_multistart, a2, b2, raise_if_none=False)
    ctx.close()
    case("synth_truth", api.synth_truth, 7, 6, 2)

    fr = case("Frontier", api.Frontier, 5, 0, 1, 8)
    try:
        case("Frontier.next", fr.next)
        case("Frontier.ingest", fr.ingest, [0.5, 1.5, 2.5], [1, -1, 0], [0, 1, -1])
        case("Frontier.result", fr.result)
    finally:
        fr.close()                 # under the fake: nothing tracks a Frontier, and its handle means nothing to the real library

    for devices in ([0, 0], 2, None):
        mc = case("MultiContext(%r)" % (devices,), api.MultiContext, devices)
        fake.note("devices=%r size=%d uses_rccl=%s" % (mc.devices, mc.size, mc.uses_rccl))
        for want_all in (False, True):
            case("MultiContext.fit_opt want_all=%s" % want_all, mc.fit_opt, Xs[np.float32, "C"], y, P, 0.5, 1, want_all=want_all)
        case("MultiContext.fit_bnb", mc.fit_bnb, Xs[np.float64, "strided"], y, P, 0.5)
        view = case("MultiContext.context(0)", mc.context, 0)
        view._shape = (12, M, K)
        case("view.opt_finish", view.opt_finish, 3)
        case("MultiContext.context out of range", mc.context, 5)
        case("MultiContext.timing", mc.timing, 1, 2)
        with fake.scripted(**FINISHERS):
            case("MultiContext.fit_opt with status 9", mc.fit_opt, X64, y, P)
            mc.tolerate_ill = True
            case("MultiContext.fit_bnb with status 9, tolerated", mc.fit_bnb, X64, y, P)
            fake.note("last_ill=%s" % mc.last_ill)
        mc.close()


def generate(api_path=None):
    api = load_api(api_path)
    with fake_library(api) as fake:
        run_cases(api, fake)
    return fake.lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--api", help="another copy of api.py to trace instead of the package's")
    ap.add_argument("-o", "--output", help="write the trace here instead of stdout")
    a = ap.parse_args()
    text = "\n".join(generate(a.api)) + "\n"
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
