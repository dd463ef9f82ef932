#!/usr/bin/env python3
"""What fit_glm saves over the loop a user had to write before it: one fit_glm call against the host loop that takes
the working rows as numpy arrays (Context.glm_working on a context of its own) and calls fit(alg, X, z, P, weights=W) with a fresh
upload each time (tests/glm_reference.py: host_loop), on HOST arrays.  Shapes: those of tools/robust_timing.py — C2 and C3 of bench.py
with Opt, the C4 shape (N = 1 000 000, M = 512) with Alt; X is bench.py's synthetic matrix, the 0/1 response is drawn from the logistic
model of its standardised linear response; `iters` re-weighted fits in both arms (tol = 0, max_iter = iters).
Both arms run in one process, alternated; per arm the median of `reps` runs after one warm-up of each, every run recorded.  The two
models are compared bit for bit.  Then the loop once more through the Context methods with a clock around every phase: the working
call (wall, and its device split into residual pass / row kernel from partls_get_glm_timing; the row kernel's bytes per second
against the measured HBM copy rate of the MI355X, 6.29 TB/s), the rework (wall, and its Gram build from PARTLS_T_GRAM), the staged fit,
and the first prepare, whose Gram and tableau the first rework discards.
Not a bench line: for DESIGN.md §4.19.

    python tools/glm_timing.py [OUT.json] [--reps R] [--iters J] [--shapes c2,c3,c4]
"""
import json, os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import partls_amd
import glm_reference as G
pls = partls_amd.package()
L = pls.lowlevel

opts = {"--reps": 5, "--iters": 3, "--shapes": "c2,c3,c4"}
skip = {i + 1 for i, a in enumerate(sys.argv) if a in opts}
args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
out_path = args[0] if args else "profiles/glm_timing.json"
for i, a in enumerate(sys.argv):
    if a in opts:
        opts[a] = type(opts[a])(sys.argv[i + 1])
reps, iters = opts["--reps"], opts["--iters"]
SHAPES = dict(c2=("opt", 20260002, 10_000, 128, 12), c3=("opt", 20260003, 100_000, 256, 20), c4=("alt", 20260004, 1_000_000, 512, 16))
HBM_COPY_TBS = 6.29                                             # measured float4 copy rate (8.0 TB/s spec)
FAMILY = "binomial"


def median(v):
    return float(np.median(v))


def host_data(seed, N, M, K):
    """bench.py's synthetic X as an F-ordered host array, and a 0/1 response from the logistic model of its standardised response"""
    P, ws = pls.synth_truth(seed, M, K)
    ctx = pls.Context(0)
    dX = torch.empty(N * M, dtype=torch.float64, device="cuda")
    dy = torch.empty(N, dtype=torch.float64, device="cuda")
    ctx.synth_device(seed, N, M, ws, dX.data_ptr(), dy.data_ptr())
    torch.cuda.synchronize()
    X = np.asfortranarray(dX.view(M, N).t().cpu().numpy())
    lin = dy.cpu().numpy()
    ctx.close()
    del dX, dy
    torch.cuda.empty_cache()
    s = (lin - lin.mean()) / lin.std()
    y = (np.random.default_rng(seed).random(N) < 1.0 / (1.0 + np.exp(-s))).astype(np.float64)
    return X, y, P


res = dict(reps=reps, iters=iters, family=FAMILY, hbm_copy_tb_s=HBM_COPY_TBS, shapes={})
warnings.simplefilter("ignore", pls.GLMConvergenceWarning)
warnings.simplefilter("ignore", pls.IllConditionedWarning)
rows_ctx = pls.Context(0)                                       # the host loop's source of working rows
for name in opts["--shapes"].split(","):
    kind, seed, N, M, K = SHAPES[name]
    X, y, P = host_data(seed, N, M, K)
    alg = pls.Opt if kind == "opt" else pls.Alt
    kw = {}
    if kind == "alt":
        a0, b0 = pls.api._draw_start(np.random.default_rng(123), M, K)
        kw = dict(alpha0=a0, beta0=b0, T=200, eps=1e-6)

    def arm_glm():
        t0 = time.perf_counter()
        out = pls.fit_glm(alg, X, y, P, family=FAMILY, max_iter=iters, tol=0.0, **kw)
        return 1e3 * (time.perf_counter() - t0), out[0], out[2]

    def arm_host():
        t0 = time.perf_counter()
        h = G.host_loop(pls, rows_ctx, alg, X, y, P, family=FAMILY, max_iter=iters, tol=0.0, **kw)
        return 1e3 * (time.perf_counter() - t0), h["models"][-1], h

    arm_glm(); arm_host()                                        # warm-up of both
    t_glm, t_host = [], []
    for _ in range(reps):
        ms, model, rep = arm_glm(); t_glm.append(ms)
        ms, hmodel, h = arm_host(); t_host.append(ms)
    same = bool(model.α.tobytes() == hmodel.α.tobytes() and model.β.tobytes() == hmodel.β.tobytes() and model.t == hmodel.t
                and rep.glm.deviance == h["deviance"])
    rec = dict(alg=alg.__name__, N=N, M=M, K=K, refits=rep.glm.iterations, fit_glm_ms=median(t_glm), host_loop_ms=median(t_host),
               fit_glm_ms_all=t_glm, host_loop_ms_all=t_host, same_model_and_deviance=same, deviance=rep.glm.deviance,
               null_deviance=rep.glm.null_deviance, n_clamped=rep.glm.n_clamped, opt=float(rep.opt))
    rec["host_loop_over_fit_glm"] = rec["host_loop_ms"] / rec["fit_glm_ms"]

    # the phases, through the Context methods (what fit_glm runs), median over the runs of the per-run sums
    ctx = pls.default_context(0)
    flags = 0 if kind == "opt" else L.OPT_FAITHFUL_INTERCEPT

    def staged():
        if kind == "opt":
            return ctx.opt_finish(ctx.opt_sweep(0, -1)[1])[:3]
        return ctx.alt_prepared(a0, b0, 1e-6, 200)[:3]

    phases = {k: [] for k in ("prepare_ms", "upload_ms", "discarded_gram_ms", "discarded_tableau_ms", "start_call_ms", "start_rows_ms",
                              "working_call_ms", "residual_ms", "rows_kernel_ms", "rework_call_ms", "gram_ms", "refit_ms")}
    for r in range(reps + 1):
        s = {k: 0.0 for k in phases}
        t0 = time.perf_counter(); ctx.opt_prepare(X, y, P, 0.0, flags); s["prepare_ms"] = 1e3 * (time.perf_counter() - t0)
        s["upload_ms"] = ctx.upload()[0]
        s["discarded_gram_ms"], s["discarded_tableau_ms"] = ctx.timing(L.T_GRAM), ctx.timing(L.T_PREP)
        t0 = time.perf_counter(); ctx.glm_working(None, FAMILY, want_rows=False); s["start_call_ms"] = 1e3 * (time.perf_counter() - t0)
        s["start_rows_ms"] = ctx.glm_timing()[1]
        for _ in range(iters):
            t0 = time.perf_counter(); ctx.opt_rework(); s["rework_call_ms"] += 1e3 * (time.perf_counter() - t0)
            s["gram_ms"] += ctx.timing(L.T_GRAM)
            t0 = time.perf_counter(); m = staged(); s["refit_ms"] += 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter(); ctx.glm_working(m, FAMILY, want_rows=False); s["working_call_ms"] += 1e3 * (time.perf_counter() - t0)
            a, b = ctx.glm_timing()
            s["residual_ms"] += a; s["rows_kernel_ms"] += b
        if r:
            for k in phases:
                phases[k].append(s[k])
    rec["phases_ms"] = {k: median(v) for k, v in phases.items()}
    rec["phases_note"] = ("sums over the %d iterations of one run (prepare, upload, discarded_*, start_*: once); *_call_ms are host wall "
                          "clock, the others device events" % iters)
    per_call_us = 1e3 * rec["phases_ms"]["rows_kernel_ms"] / iters
    moved = 40.0 * N                                              # eta and y in, W, z and mu out: 8 bytes each per row
    rec["rows_kernel"] = dict(us_per_call=per_call_us, bytes_per_call=moved, tb_per_s=moved / (per_call_us * 1e-6) / 1e12 if per_call_us else 0.0,
                              share_of_hbm_copy_rate=(moved / (per_call_us * 1e-6) / 1e12 / HBM_COPY_TBS) if per_call_us else 0.0)
    res["shapes"][name] = rec
    print(name, json.dumps(rec), flush=True)
    del X, y
rows_ctx.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
