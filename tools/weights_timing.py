#!/usr/bin/env python3
"""Cost of sample weights: the weighted against the unweighted path on the same device-resident data, the two
alternated in one process, median of `reps` warm runs each:
  gram — the C4 Gram (N = 1e6, D = 512): partls_get_timing(GRAM) of a prepare (HIP events around gram_kernel + gram_reduce_kernel;
         the weighted prepare's one weight_prep_kernel pass is outside it and reported as prepare wall time);
  fit  — a C3 fit(Opt) (N = 1e5, D = 256, K = 20): prepare + sweep + finish, device events per phase and host wall time.
Unit weights are used for the timing, and the results of both paths are compared bit for bit (unit weights are the
unweighted path).  Not a bench line.

    python tools/weights_timing.py [OUT.json] [--reps R]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package(); L = pls.lowlevel

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else "profiles/weights_timing.json"
reps = 7
for i, a in enumerate(sys.argv):
    if a == "--reps":
        reps = int(sys.argv[i + 1])


def device_data(ctx, seed, N, D, K):
    P, ws = pls.synth_truth(seed, D, K)
    dX = torch.empty(N * D, dtype=torch.float64, device="cuda"); dy = torch.empty(N, dtype=torch.float64, device="cuda")
    ctx.synth_device(seed, N, D, ws, dX.data_ptr(), dy.data_ptr())
    torch.cuda.synchronize()
    return P, dX, dy


def med(v):
    return float(np.median(v))


ctx = pls.Context(0)
res = dict(reps=reps)

# ---- C4 Gram
N, D, K = 1_000_000, 512, 16
P, dX, dy = device_data(ctx, 20260004, N, D, K)
dw = torch.ones(N, dtype=torch.float64, device="cuda")
g = {"unweighted": [], "weighted": []}
wall = {"unweighted": [], "weighted": []}
G = {}
for it in range(reps + 1):
    for kind, ptr in (("unweighted", None), ("weighted", dw.data_ptr())):
        t0 = time.perf_counter()
        ctx.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, D, N, P, 0.0, L.OPT_FAITHFUL_INTERCEPT, dw_ptr=ptr)
        t1 = time.perf_counter()
        if it > 0:
            g[kind].append(ctx.timing(L.T_GRAM)); wall[kind].append(1e3 * (t1 - t0))
        else:
            G[kind] = ctx.gram()
res["c4_gram"] = dict(N=N, D=D, gram_ms={k: med(v) for k, v in g.items()}, gram_ms_all=g,
                      prepare_wall_ms={k: med(v) for k, v in wall.items()},
                      ratio=med(g["weighted"]) / med(g["unweighted"]), unit_weights_bitwise=bool(np.array_equal(G["weighted"], G["unweighted"])))
del dX, dy, dw
torch.cuda.empty_cache()

# ---- C3 fit(Opt)
N, D, K = 100_000, 256, 20
P, dX, dy = device_data(ctx, 20260003, N, D, K)
dw = torch.ones(N, dtype=torch.float64, device="cuda")
ph = {"unweighted": [], "weighted": []}
out = {}
for it in range(reps + 1):
    for kind, ptr in (("unweighted", None), ("weighted", dw.data_ptr())):
        t0 = time.perf_counter()
        ctx.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, D, N, P, 0.0, 0, dw_ptr=ptr)
        bo, bp, _, nu = ctx.opt_sweep(0, -1)
        r = ctx.opt_finish(bp)
        t1 = time.perf_counter()
        if it > 0:
            ph[kind].append(dict(wall_ms=1e3 * (t1 - t0), gram_ms=ctx.timing(L.T_GRAM), prep_ms=ctx.timing(L.T_PREP),
                                 sweep_ms=ctx.timing(L.T_SWEEP), finish_ms=ctx.timing(L.T_FINISH)))
        else:
            out[kind] = (bo, bp, nu) + tuple(np.asarray(x).tobytes() for x in r)
summ = {k: {f: med([d[f] for d in v]) for f in v[0]} for k, v in ph.items()}
res["c3_fit"] = dict(N=N, D=D, K=K, median=summ, ratio_wall=summ["weighted"]["wall_ms"] / summ["unweighted"]["wall_ms"],
                     unit_weights_bitwise=out["weighted"] == out["unweighted"])
ctx.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({k: (v if k == "reps" else {kk: vv for kk, vv in v.items() if kk != "gram_ms_all"}) for k, v in res.items()}, indent=1))
