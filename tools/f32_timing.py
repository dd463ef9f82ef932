#!/usr/bin/env python3
"""Cost of float32 design matrices: the float32 path against the fp64 path on the widened data, the two alternated in
one process, median of `reps` warm runs each.  The synthetic X is a multiple of 2^-16 below 2^3 in magnitude, so its
float32 copy is exact and both paths see the same values: every result is also compared bit for bit.
  gram — the Gram at C4 (N = 1e6, D = 512) and C3 (N = 1e5, D = 256), device-resident: partls_get_timing(GRAM) of a prepare (HIP events
         around gram_kernel + gram_reduce_kernel); `fp64_spread` is the min-max range of the fp64 runs, the margin a difference is
         judged against;
  fit  — a device-resident C3 fit(Opt): prepare + sweep + finish (the finish runs residual_kernel / xtr_kernel: a rocprofv3
         --kernel-trace --stats pass of `--parts gram,fit` gives their times for both element types);
  host — the host-pointer fits of bench.py's host_inclusive leg (C3 fit(Opt), C4 fit(Alt)), on a reused array and on a freshly
         allocated one: wall time, and partls_get_upload's ms and bytes.
Not a bench line.

    python tools/f32_timing.py [OUT.json] [--reps R] [--parts gram,fit,host]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package(); L = pls.lowlevel

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps, parts = 7, ("gram", "fit", "host")
for i, a in enumerate(sys.argv):
    if a == "--reps":
        reps = int(sys.argv[i + 1]); args.remove(sys.argv[i + 1])
    if a == "--parts":
        parts = tuple(sys.argv[i + 1].split(",")); args.remove(sys.argv[i + 1])
out_path = args[0] if args else "profiles/f32_timing.json"
KINDS = (("f64", np.float64), ("f32", np.float32))


def device_data(ctx, seed, N, D, K):
    """(P, {"f64": X, "f32": X as float32}, y) on the device, column-major with leading dimension N"""
    P, ws = pls.synth_truth(seed, D, K)
    dX = torch.empty(N * D, dtype=torch.float64, device="cuda"); dy = torch.empty(N, dtype=torch.float64, device="cuda")
    ctx.synth_device(seed, N, D, ws, dX.data_ptr(), dy.data_ptr())
    torch.cuda.synchronize()
    dX32 = dX.float()
    assert bool((dX32.double() == dX).all()), "the float32 copy of the synthetic X is not exact"
    return P, {"f64": dX, "f32": dX32}, dy


def med(v):
    return float(np.median(v))


ctx = pls.Context(0)
res = dict(reps=reps, parts=list(parts))

if "gram" in parts:
    for name, seed, N, D, K in (("c4_gram", 20260004, 1_000_000, 512, 16), ("c3_gram", 20260003, 100_000, 256, 20)):
        P, dX, dy = device_data(ctx, seed, N, D, K)
        g = {k: [] for k, _ in KINDS}
        G = {}
        for it in range(reps + 1):
            for kind, dt in KINDS:
                ctx.opt_prepare_device(dX[kind].data_ptr(), dy.data_ptr(), N, D, N, P, 0.0, L.OPT_FAITHFUL_INTERCEPT, dtype=dt)
                if it > 0:
                    g[kind].append(ctx.timing(L.T_GRAM))
                else:
                    G[kind] = ctx.gram()
        res[name] = dict(N=N, D=D, gram_ms={k: med(v) for k, v in g.items()}, gram_ms_all=g,
                         fp64_spread_ms=max(g["f64"]) - min(g["f64"]), f32_minus_f64_ms=med(g["f32"]) - med(g["f64"]),
                         ratio=med(g["f32"]) / med(g["f64"]), bitwise=bool(np.array_equal(G["f32"], G["f64"])))
        del dX, dy
        torch.cuda.empty_cache()

if "fit" in parts:
    seed, N, D, K = 20260003, 100_000, 256, 20
    P, dX, dy = device_data(ctx, seed, N, D, K)
    ph = {k: [] for k, _ in KINDS}
    out = {}
    for it in range(reps + 1):
        for kind, dt in KINDS:
            t0 = time.perf_counter()
            ctx.opt_prepare_device(dX[kind].data_ptr(), dy.data_ptr(), N, D, N, P, 0.0, 0, dtype=dt)
            bo, bp, _, nu = ctx.opt_sweep(0, -1)
            r = ctx.opt_finish(bp)
            t1 = time.perf_counter()
            if it > 0:
                ph[kind].append(dict(wall_ms=1e3 * (t1 - t0), gram_ms=ctx.timing(L.T_GRAM), prep_ms=ctx.timing(L.T_PREP),
                                     sweep_ms=ctx.timing(L.T_SWEEP), finish_ms=ctx.timing(L.T_FINISH)))
            else:
                out[kind] = (bo, bp, nu) + tuple(np.asarray(x).tobytes() for x in r)
    summ = {k: {f: med([d[f] for d in v]) for f in v[0]} for k, v in ph.items()}
    res["c3_fit_device"] = dict(N=N, D=D, K=K, median=summ, ratio_wall=summ["f32"]["wall_ms"] / summ["f64"]["wall_ms"],
                                bitwise=out["f32"] == out["f64"])
    del dX, dy
    torch.cuda.empty_cache()

if "host" in parts:
    for name, alg, seed, N, D, K in (("c3_host_fit", "opt", 20260003, 100_000, 256, 20), ("c4_host_fit", "alt", 20260004, 1_000_000, 512, 16)):
        P, dX, dy = device_data(ctx, seed, N, D, K)
        hy = dy.cpu().numpy()
        hX = {k: np.asfortranarray(dX[k].view(D, N).t().cpu().numpy()) for k, _ in KINDS}
        del dX, dy
        torch.cuda.empty_cache()
        rng = np.random.default_rng(seed)
        a0, b0 = rng.random(D + 1), (rng.random(K + 1) - 0.5) * 10

        def host_fit(Xh):
            t0 = time.perf_counter()
            if alg == "alt":
                ctx.opt_prepare(Xh, hy, P, 0.0, L.OPT_FAITHFUL_INTERCEPT)
                up = ctx.upload()
                r = ctx.alt_prepared(a0, b0, eps=1e-6, T=200)
            else:
                ctx.opt_prepare(Xh, hy, P, 0.0, 0)
                up = ctx.upload()
                r = ctx.opt_finish(ctx.opt_sweep(0, -1)[1])
            return dict(wall_ms=1e3 * (time.perf_counter() - t0), upload_ms=up[0], upload_bytes=up[1],
                        gbs=up[1] / up[0] / 1e6), tuple(np.asarray(x).tobytes() for x in r)

        runs = {k: dict(reused=[], fresh=[]) for k, _ in KINDS}
        outs = {}
        nrep = max(2, min(reps, 3))
        for it in range(nrep + 1):
            for kind, _ in KINDS:
                m, o = host_fit(hX[kind])
                outs.setdefault(kind, o)
                assert outs[kind] == o
                if it > 0:
                    runs[kind]["reused"].append(m)
        for it in range(2):
            for kind, _ in KINDS:
                Xf = np.empty_like(hX[kind], order="F"); Xf[...] = hX[kind]   # a new allocation per fit: pages the runtime never pinned
                runs[kind]["fresh"].append(host_fit(Xf)[0]); del Xf
        summ = {k: {c: {f: med([d[f] for d in v]) for f in v[0]} for c, v in r.items()} for k, r in runs.items()}
        res[name] = dict(N=N, D=D, K=K, alg=alg, median=summ, all=runs, bitwise=outs["f32"] == outs["f64"],
                         wall_ratio_reused=summ["f32"]["reused"]["wall_ms"] / summ["f64"]["reused"]["wall_ms"],
                         wall_ratio_fresh=summ["f32"]["fresh"]["wall_ms"] / summ["f64"]["fresh"]["wall_ms"])
        del hX

ctx.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk not in ("gram_ms_all", "all")} if isinstance(v, dict) else v)
                  for k, v in res.items()}, indent=1))
