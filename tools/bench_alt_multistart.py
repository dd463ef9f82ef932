#!/usr/bin/env python3
"""Timing of fit(Alt) from many starts: one partls_alt_multistart call for R starts against R sequential
partls_alt_prepared calls from the same starts, both on ONE context prepared once with device-generated data (synth_device), so
neither side pays an upload or a Gram build.  Median wall time of `reps` runs after a warm-up run of each.
  deferred — N = 100 000, D = 512, K = 16: n = 513, alpha-steps on the deferred-update kernel (the loop: cooperative kernel)
  many_groups — N = 100 000, D = 100, K = 50: beyond the enumeration of Opt
A `rocprofv3 --kernel-trace --stats -- python tools/bench_alt_multistart.py OUT.json --reps 1 --R 1024 --no-loop` run of its own gives
the per-kernel split of the batched call (--no-loop: the sequential calls, which share the sweep kernels, are left out).  Not a bench line.

    python tools/bench_alt_multistart.py [OUT.json] [--reps 5] [--R 64,1024,4096] [--shapes deferred,many_groups] [--no-loop]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package(); L = pls.lowlevel

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps, Rs, shapes = 5, (64, 1024, 4096), ("deferred", "many_groups")
for i, a in enumerate(sys.argv):
    if a == "--reps":
        reps = int(sys.argv[i + 1]); args.remove(sys.argv[i + 1])
    if a == "--R":
        Rs = tuple(int(v) for v in sys.argv[i + 1].split(",")); args.remove(sys.argv[i + 1])
    if a == "--shapes":
        shapes = tuple(sys.argv[i + 1].split(",")); args.remove(sys.argv[i + 1])
with_loop = "--no-loop" not in sys.argv
out_path = args[0] if args else "profiles/alt_multistart_timing.json"
SHAPES = {"deferred": (20260004, 100_000, 512, 16), "many_groups": (20260007, 100_000, 100, 50)}
EPS, T = 1e-6, 100


def med(v):
    return float(np.median(v))


res = dict(reps=reps, eps=EPS, T=T)
for name in shapes:
    seed, N, D, K = SHAPES[name]
    ctx = pls.Context(0)
    ctx.tolerate_ill = True
    P, ws = pls.synth_truth(seed, D, K)
    dX = torch.empty(N * D, dtype=torch.float64, device="cuda"); dy = torch.empty(N, dtype=torch.float64, device="cuda")
    ctx.synth_device(seed, N, D, ws, dX.data_ptr(), dy.data_ptr())
    torch.cuda.synchronize()
    ctx.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, D, N, P, 0.0, L.OPT_FAITHFUL_INTERCEPT)
    route = ctx.sweep_route()
    gen = np.random.default_rng(123)
    Rmax = max(Rs)
    a0 = np.empty((Rmax, D + 1)); b0 = np.empty((Rmax, K + 1))
    for r in range(Rmax):
        a0[r] = gen.random(D + 1); b0[r] = (gen.random(K + 1) - 0.5) * 10
    rows = {}
    for R in Rs:
        batched, loop = [], []
        out = None
        for it in range(reps + 1):
            t0 = time.perf_counter()
            out = ctx.alt_multistart(a0[:R], b0[:R], EPS, T)
            t1 = time.perf_counter()
            single_opt = np.empty(R); single_it = np.empty(R, dtype=np.int64)
            failed = 0
            for r in range(R if with_loop else 0):
                try:
                    _, _, _, single_opt[r], single_it[r] = ctx.alt_prepared(a0[r], b0[r], EPS, T)
                except pls.PartlsError:
                    single_opt[r], single_it[r], failed = np.nan, 0, failed + 1
            t2 = time.perf_counter()
            if it > 0:
                batched.append(1e3 * (t1 - t0)); loop.append(1e3 * (t2 - t1))
        st = out[6]
        ok = st["status"] == L.OK
        rows[str(R)] = dict(batched_ms=med(batched), batched_ms_all=batched, starts_ok=int(ok.sum()), best_start=int(out[5]),
                            best_opt=float(out[3]), distinct_optima=int(len(np.unique(np.round(st["opt"][ok], 6)))),
                            iters_min=int(st["iters"][ok].min()), iters_max=int(st["iters"][ok].max()), iters_total=int(st["iters"][ok].sum()))
        if with_loop:
            # the loop's opt is taken from the data where the single call takes it from the data; the per-start opt is the Gram-form loss
            gap = float(np.nanmax(np.abs(st["opt"][ok] - single_opt[ok]) / np.maximum(1.0, single_opt[ok]))) if ok.any() else float("nan")
            rows[str(R)].update(loop_ms=med(loop), speedup=med(loop) / med(batched), loop_ms_all=loop, loop_failed=failed,
                                same_iters_as_loop=int((st["iters"][ok] == single_it[ok]).sum()), max_rel_opt_gap_vs_loop=gap)
        print(name, R, {k: v for k, v in rows[str(R)].items() if not k.endswith("_all")}, flush=True)
    res[name] = dict(N=N, D=D, K=K, route=route[0], tiles=route[1], R=rows)
    ctx.close()
    del dX, dy
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
