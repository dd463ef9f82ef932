#!/usr/bin/env python3
"""Cost of every Opt pattern's model at C3, faithful (N = 100k, D = 256, K = 20: 2^21 patterns) — partls_opt_models against the
per-pattern path.  Not a bench line: for DESIGN.md §4, "Every pattern's model".

    python tools/models_timing.py [OUT.json]            # wall times: solutions.arrays(), the C entry alone, 64 opt_finish calls
    python tools/models_timing.py --kernels             # one plain faithful sweep + one export of the same range, nothing else:
                                                        # run under rocprofv3 --kernel-trace --stats for the kernel times
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package(); L = pls.lowlevel

seed, N, D, K = 20260003, 100_000, 256, 20                   # bench.py C3
P, ws = pls.synth_truth(seed, D, K)
dX = torch.empty(N * D, dtype=torch.float64, device="cuda"); dy = torch.empty(N, dtype=torch.float64, device="cuda")
ctx = pls.Context(0)
ctx.synth_device(seed, N, D, ws, dX.data_ptr(), dy.data_ptr()); torch.cuda.synchronize()
npat = 1 << (K + 1)

if "--kernels" in sys.argv:
    ctx.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, D, N, P, 0.0, L.OPT_FAITHFUL_INTERCEPT)
    ctx.opt_sweep(0, -1)                                     # the calibration runs here, before both timed kernels
    ctx.opt_sweep(0, -1)
    ctx.opt_models(0, -1)
    ctx.close()
    sys.exit(0)

out = dict(config="C3 faithful", N=N, D=D, K=K, patterns=npat, piece_bytes_cap=1 << 30)
Xh = dX.view(D, N).t().cpu().numpy()                         # host copy (column-major N x D on the device)
yh = dy.cpu().numpy()
del dX, dy; torch.cuda.empty_cache()

t0 = time.perf_counter()
model, _, rep = pls.fit(pls.Opt, Xh, yh, P, returnAllSolutions=True)
out["fit_returnAllSolutions_s"] = time.perf_counter() - t0
sols = rep.solutions
sols.arrays(chunk=1 << 16)                                   # warm: page-locked staging, first-touch of the result arrays
for chunk in (1 << 18, 1 << 21):
    t0 = time.perf_counter()
    opt, alpha, beta, t = sols.arrays(chunk=chunk)
    out[f"arrays_s_chunk_2^{chunk.bit_length() - 1}"] = time.perf_counter() - t0
ctx2 = sols._context()
t0 = time.perf_counter()
r = ctx2.opt_models(0, -1)
out["opt_models_full_range_s"] = time.perf_counter() - t0
out["n_unconverged"], out["n_vetoes"] = r["n_unconverged"], r["n_vetoes"]
del r
t0 = time.perf_counter()
r = ctx2.opt_models(0, 1 << 18)
out["opt_models_2^18_s"] = time.perf_counter() - t0
del r
rng = np.random.default_rng(1)
pats = rng.choice(npat, 64, replace=False)
t0 = time.perf_counter()
fin = [sols[int(b)] for b in pats]
dt = time.perf_counter() - t0
out["opt_finish_64_s"] = dt
out["opt_finish_extrapolated_all_s"] = dt / 64 * npat
err = max(float(np.abs(alpha[b] - m.α).max()) for b, (_, m) in zip(pats, fin))
out["max_abs_alpha_vs_opt_finish_64"] = err
print(json.dumps(out, indent=1))
if len(sys.argv) > 1 and not sys.argv[1].startswith("-"):
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
