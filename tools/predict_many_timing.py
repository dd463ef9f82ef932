#!/usr/bin/env python3
"""Cost of predicting from B models at the C3 test-set size (synthetic X, N = 100 000, M = 256, K = 16; B = 100 random models) three
ways, for a host X and a device-resident X, float64 and float32:
  many   — one partls_predict_many call for the full N x B matrix (one upload of a host X, one pass over X per 16 models);
  stats  — one partls_predict_many call for four order statistics and the mean of every row (what a percentile band needs): no N x B
           array on the host, nothing but N x 5 doubles across PCIe;
  loop   — the B partls_predict / partls_predict_device calls the two replace (each uploads a host X and reads it once).
All in one process, alternating the three; wall times in ms around calls that end in a stream synchronise: median, minimum and
maximum of `reps` rounds after one warm-up round.  The columns of `many` are compared bit for bit with the loop's at the timed size, and
`stats` with numpy on them.  Not a bench line: for DESIGN.md §4.12.

    python tools/predict_many_timing.py [OUT.json] [--reps R] [--N N] [--B B]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package()

opts = {"--reps": 5, "--N": 100_000, "--B": 100}
skip = {i + 1 for i, a in enumerate(sys.argv) if a in opts}
args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
out_path = args[0] if args else "profiles/predict_many_timing.json"
for i, a in enumerate(sys.argv):
    if a in opts:
        opts[a] = int(sys.argv[i + 1])
reps, N, B = opts["--reps"], opts["--N"], opts["--B"]
SEED, M, K = 20260103, 256, 16

P, ws = pls.synth_truth(SEED, M, K)
ctx = pls.Context(0)
dX64 = torch.empty(N * M, dtype=torch.float64, device="cuda")
dy = torch.empty(N, dtype=torch.float64, device="cuda")
ctx.synth_device(SEED, N, M, ws, dX64.data_ptr(), dy.data_ptr())
torch.cuda.synchronize()
dX32 = dX64.to(torch.float32)
rng = np.random.default_rng(SEED)
alpha, beta, t = rng.random((B, M)), rng.normal(size=(B, K)), rng.normal(size=B)
ranks = pls.api._percentile_ranks(B, [2.5, 97.5])[0]


def rounds(fns):
    """every function once to warm up, then `reps` rounds of all of them in turn: {name: (median, min, max)} in ms"""
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); ts[k].append(1e3 * (time.perf_counter() - t0))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v))) for k, v in ts.items()}


res = dict(N=N, M=M, K=K, B=B, reps=reps, ranks=ranks.tolist(), forms={})
for name, dX, dtype in (("float64", dX64, np.float64), ("float32", dX32, np.float32)):
    # ---- host pointers
    X = np.asfortranarray(dX.view(M, N).t().cpu().numpy())
    keep = {}

    def many():
        keep["many"] = ctx.predict_many(X, P, alpha, beta, t)["yhat"]

    def stats():
        keep["stats"] = ctx.predict_many(X, P, alpha, beta, t, ranks=ranks, want_yhat=False, want_mean=True)

    def loop():
        keep["loop"] = [ctx.predict(X, P, alpha[b], beta[b], t[b]) for b in range(B)]

    rec = rounds(dict(many=many, stats=stats, loop=loop))
    Y = keep["many"]
    rec["columns_equal_loop_bitwise"] = all(np.array_equal(Y[:, b], keep["loop"][b]) for b in range(B))
    rec["stats_equal_numpy"] = bool(np.array_equal(keep["stats"]["stats"], np.sort(Y, axis=1)[:, ranks]))
    rec["many_speedup_vs_loop"] = rec["loop"]["median_ms"] / rec["many"]["median_ms"]
    rec["stats_speedup_vs_loop"] = rec["loop"]["median_ms"] / rec["stats"]["median_ms"]
    res["forms"]["host_" + name] = rec
    print("host", name, json.dumps(rec), flush=True)
    del X
    # ---- device pointers: X, yhat (N x B), stats (N x nr) and mean stay in HBM
    dY = torch.zeros((B, N), dtype=torch.float64, device="cuda")
    dL = torch.zeros((B, N), dtype=torch.float64, device="cuda")
    dS = torch.zeros((len(ranks), N), dtype=torch.float64, device="cuda")
    dM = torch.zeros(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def many_d():
        ctx.predict_many_device(dX.data_ptr(), N, M, N, P, alpha, beta, t, dyhat_ptr=dY.data_ptr(), ldY=N, dtype=dtype)

    def stats_d():
        ctx.predict_many_device(dX.data_ptr(), N, M, N, P, alpha, beta, t, ranks=ranks, dstats_ptr=dS.data_ptr(), dmean_ptr=dM.data_ptr(),
                                dtype=dtype)

    def loop_d():
        for b in range(B):
            ctx.predict_device(dX.data_ptr(), N, M, N, P, alpha[b], beta[b], t[b], dL.data_ptr() + 8 * N * b, dtype=dtype)

    rec = rounds(dict(many=many_d, stats=stats_d, loop=loop_d))
    rec["columns_equal_loop_bitwise"] = bool(torch.equal(dY, dL))
    rec["equal_host_form_bitwise"] = bool(np.array_equal(dY.cpu().numpy().T, Y))
    rec["stats_equal_numpy"] = bool(np.array_equal(dS.cpu().numpy().T, np.sort(Y, axis=1)[:, ranks]))
    rec["many_speedup_vs_loop"] = rec["loop"]["median_ms"] / rec["many"]["median_ms"]
    rec["stats_speedup_vs_loop"] = rec["loop"]["median_ms"] / rec["stats"]["median_ms"]
    res["forms"]["device_" + name] = rec
    print("device", name, json.dumps(rec), flush=True)
    del dY, dL, dS, dM, Y
ctx.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
