#!/usr/bin/env python3
"""What fit_robust saves over the loop a user had to write before it: one fit_robust call against the host loop of
fit(alg, X, y, P, weights=w_j) calls with numpy weights formed from predict(model, X) (tests/robust_reference.py: host_loop) that
reaches the same model, on HOST arrays — the uploads and downloads are what the feature removes.  Shapes: C2 and C3 of bench.py with
Opt, the C4 shape (N = 1 000 000, M = 512) with Alt; synthetic X and y with a tenth of the rows of y shifted by 50 noise standard
deviations; Huber loss, MAD scale, `iters` re-weighted fits in both arms (tol = 0, max_iter = iters).
Both arms run in one process, alternated; per arm the median of `reps` runs after one warm-up of each, every run recorded.  The two
models are compared bit for bit.  Then the loop once more through the Context methods with a clock around every phase: the weights
pass (wall, and its device split into residual pass / selection / weight kernel from partls_get_robust_timing), the re-prepare (wall,
and its Gram build from PARTLS_T_GRAM) and the staged fit.
Not a bench line: for DESIGN.md §4.18.

    python tools/robust_timing.py [OUT.json] [--reps R] [--iters J] [--shapes c2,c3,c4]
"""
import json, os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import partls_amd
import robust_reference as R
pls = partls_amd.package()
L = pls.lowlevel

opts = {"--reps": 5, "--iters": 3, "--shapes": "c2,c3,c4"}
skip = {i + 1 for i, a in enumerate(sys.argv) if a in opts}
args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
out_path = args[0] if args else "profiles/robust_timing.json"
for i, a in enumerate(sys.argv):
    if a in opts:
        opts[a] = type(opts[a])(sys.argv[i + 1])
reps, iters = opts["--reps"], opts["--iters"]
SHAPES = dict(c2=("opt", 20260002, 10_000, 128, 12), c3=("opt", 20260003, 100_000, 256, 20), c4=("alt", 20260004, 1_000_000, 512, 16))


def median(v):
    return float(np.median(v))


def host_data(seed, N, M, K):
    """bench.py's synthetic problem, a tenth of the rows of y shifted by 50 noise standard deviations, as F-ordered host arrays"""
    P, ws = pls.synth_truth(seed, M, K)
    ctx = pls.Context(0)
    dX = torch.empty(N * M, dtype=torch.float64, device="cuda")
    dy = torch.empty(N, dtype=torch.float64, device="cuda")
    ctx.synth_device(seed, N, M, ws, dX.data_ptr(), dy.data_ptr())
    torch.cuda.synchronize()
    X = np.asfortranarray(dX.view(M, N).t().cpu().numpy())
    y = dy.cpu().numpy()
    ctx.close()
    del dX, dy
    torch.cuda.empty_cache()
    y[np.random.default_rng(seed).random(N) < 0.1] += 5.0       # the noise of synth.hip has standard deviation 0.1
    return X, y, P


res = dict(reps=reps, iters=iters, loss="huber", scale="mad", shapes={})
warnings.simplefilter("ignore", pls.RobustConvergenceWarning)
warnings.simplefilter("ignore", pls.IllConditionedWarning)
for name in opts["--shapes"].split(","):
    kind, seed, N, M, K = SHAPES[name]
    X, y, P = host_data(seed, N, M, K)
    alg = pls.Opt if kind == "opt" else pls.Alt
    kw = {}
    if kind == "alt":
        a0, b0 = pls.api._draw_start(np.random.default_rng(123), M, K)
        kw = dict(alpha0=a0, beta0=b0, T=200, eps=1e-6)

    def arm_robust():
        t0 = time.perf_counter()
        out = pls.fit_robust(alg, X, y, P, loss="huber", max_iter=iters, tol=0.0, **kw)
        return 1e3 * (time.perf_counter() - t0), out[0], out[2]

    def arm_host():
        t0 = time.perf_counter()
        h = R.host_loop(pls, alg, X, y, P, loss="huber", max_iter=iters, tol=0.0, **kw)
        return 1e3 * (time.perf_counter() - t0), h["models"][-1], h

    arm_robust(); arm_host()                                     # warm-up of both
    t_rob, t_host = [], []
    for _ in range(reps):
        ms, model, rep = arm_robust(); t_rob.append(ms)
        ms, hmodel, h = arm_host(); t_host.append(ms)
    same = bool(model.α.tobytes() == hmodel.α.tobytes() and model.β.tobytes() == hmodel.β.tobytes() and model.t == hmodel.t
                and rep.robust.weights.tobytes() == h["weights"].tobytes())
    rec = dict(alg=alg.__name__, N=N, M=M, K=K, refits=rep.robust.iterations, fit_robust_ms=median(t_rob), host_loop_ms=median(t_host),
               fit_robust_ms_all=t_rob, host_loop_ms_all=t_host, same_model_and_weights=same, scales=rep.robust.scales,
               max_dw=rep.robust.max_dw, n_down=rep.robust.n_down, opt=float(rep.opt))
    rec["host_loop_over_fit_robust"] = rec["host_loop_ms"] / rec["fit_robust_ms"]

    # the phases, through the Context methods (what fit_robust runs), median over the runs of the per-run sums
    ctx = pls.default_context(0)
    flags = 0 if kind == "opt" else L.OPT_FAITHFUL_INTERCEPT

    def staged():
        if kind == "opt":
            return ctx.opt_finish(ctx.opt_sweep(0, -1)[1])[:3]
        return ctx.alt_prepared(a0, b0, 1e-6, 200)[:3]

    phases = {k: [] for k in ("prepare_ms", "upload_ms", "first_fit_ms", "weights_call_ms", "residual_ms", "select_ms", "weight_kernel_ms",
                              "reweight_call_ms", "gram_ms", "refit_ms")}
    for r in range(reps + 1):
        s = {k: 0.0 for k in phases}
        t0 = time.perf_counter(); ctx.opt_prepare(X, y, P, 0.0, flags); s["prepare_ms"] = 1e3 * (time.perf_counter() - t0)
        s["upload_ms"] = ctx.upload()[0]
        t0 = time.perf_counter(); m = staged(); s["first_fit_ms"] = 1e3 * (time.perf_counter() - t0)
        for _ in range(iters):
            t0 = time.perf_counter(); ctx.robust_weights(*m, loss="huber", want_weights=False); s["weights_call_ms"] += 1e3 * (time.perf_counter() - t0)
            a, b, c = ctx.robust_timing()
            s["residual_ms"] += a; s["select_ms"] += b; s["weight_kernel_ms"] += c
            t0 = time.perf_counter(); ctx.opt_reweight(); s["reweight_call_ms"] += 1e3 * (time.perf_counter() - t0)
            s["gram_ms"] += ctx.timing(L.T_GRAM)
            t0 = time.perf_counter(); m = staged(); s["refit_ms"] += 1e3 * (time.perf_counter() - t0)
        if r:
            for k in phases:
                phases[k].append(s[k])
    rec["phases_ms"] = {k: median(v) for k, v in phases.items()}
    rec["phases_note"] = "sums over the %d iterations of one run; *_call_ms are host wall clock, the others device events" % iters
    res["shapes"][name] = rec
    print(name, json.dumps(rec), flush=True)
    del X, y
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
