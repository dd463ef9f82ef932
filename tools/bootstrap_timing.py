#!/usr/bin/env python3
"""Cost of B bootstrap replicates of fit(Opt) (partls_opt_weightings) three ways, on the same data and the same multinomial counts:
  batched  — one partls_opt_weightings call (one upload of X, y, W; one weighted Gram per column; batched prep and sweep; per-problem
             finish; one out-of-bag pass);
  serial   — the same call under PARTLS_RESAMPLE_SERIAL=1 (every problem prepared and swept on its own; same upload and Grams);
  fits     — B plain fit(Opt, weights=counts[:, b]) calls from host arrays (each uploads X and builds its own Gram).
Shapes: (a) N = 2e4, D = 48, K = 6, B = 200; (b) C2 (N = 1e4, D = 128, K = 12), B = 64; (c) N = 1e5, D = 256, K = 16, B = 8.
Reports wall times (median of `reps` calls after one warm-up; host arrays, one process) and the phase split of the calls
(partls_get_timing: GRAM, PREP, SWEEP summed over the batch, FINISH = host wall time of the per-problem finishes, OOB = the out-of-bag
kernels).  Not a bench line: for DESIGN.md §4.10.

    python tools/bootstrap_timing.py [OUT.json] [--shapes a,b,c] [--reps R]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package(); L = pls.lowlevel

SHAPES = {"a": (20260101, 20_000, 48, 6, 200), "b": (20260002, 10_000, 128, 12, 64), "c": (20260103, 100_000, 256, 16, 8)}
skip = {i + 1 for i, a in enumerate(sys.argv) if a in ("--shapes", "--reps")}
args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
out_path = args[0] if args else "profiles/bootstrap_timing.json"
which = "abc"
reps = 5
for i, a in enumerate(sys.argv):
    if a == "--shapes":
        which = sys.argv[i + 1].replace(",", "")
    if a == "--reps":
        reps = int(sys.argv[i + 1])


def data(seed, N, D, K):
    P, ws = pls.synth_truth(seed, D, K)
    dX = torch.empty(N * D, dtype=torch.float64, device="cuda"); dy = torch.empty(N, dtype=torch.float64, device="cuda")
    c = pls.Context(0)
    c.synth_device(seed, N, D, ws, dX.data_ptr(), dy.data_ptr()); torch.cuda.synchronize()
    X = np.asfortranarray(dX.view(D, N).t().cpu().numpy()); y = dy.cpu().numpy()
    c.close()
    return X, y, P


def phases(ctx):
    return {k: ctx.timing(w) for k, w in (("gram_ms", L.T_GRAM), ("prep_ms", L.T_PREP), ("sweep_ms", L.T_SWEEP), ("finish_ms", L.T_FINISH),
                                          ("oob_ms", L.T_OOB), ("calib_ms", L.T_CALIB))}


def timed(fn):
    fn()
    ts, ph = [], None
    for _ in range(reps):
        t0 = time.perf_counter(); r = fn(); ts.append(1e3 * (time.perf_counter() - t0))
        ph = r
    return float(np.median(ts)), ph


os.environ.pop("PARTLS_RESAMPLE_SERIAL", None)
ctx = pls.Context(0)
os.environ["PARTLS_RESAMPLE_SERIAL"] = "1"
ctx_s = pls.Context(0)
del os.environ["PARTLS_RESAMPLE_SERIAL"]
res = dict(reps=reps, shapes={})
for s in which:
    seed, N, D, K, B = SHAPES[s]
    X, y, P = data(seed, N, D, K)
    counts = np.random.default_rng(seed).multinomial(N, np.full(N, 1.0 / N), size=B).T
    W = np.asfortranarray(counts, dtype=np.float64)
    rec = dict(N=N, D=D, K=K, B=B)

    def run(c):
        r = c.opt_weightings(X, y, P, W, 0.0, 0)
        return dict(phases(c), status_nonzero=int(np.count_nonzero(r["status"])), best_index=r["best_index"].tolist(),
                    opt=r["opt"].tolist())

    rec["batched_ms"], rec["batched_phases"] = timed(lambda: run(ctx))
    rec["serial_ms"], rec["serial_phases"] = timed(lambda: run(ctx_s))
    bb, sb = rec["batched_phases"].pop("best_index"), rec["serial_phases"].pop("best_index")
    bo, so = np.array(rec["batched_phases"].pop("opt")), np.array(rec["serial_phases"].pop("opt"))
    rec["batched_serial_same_winners"] = bb == sb
    rec["batched_serial_opt_max_rel"] = float(np.max(np.abs(bo - so) / so))
    cols = [np.ascontiguousarray(W[:, b]) for b in range(B)]
    fit_opt = []

    def fits():
        fit_opt.clear()
        for w in cols:
            fit_opt.append(pls.fit(pls.Opt, X, y, P, weights=w)[2].opt)
        return None
    rec["fits_ms"], _ = timed(fits)
    rec["batched_fits_opt_max_rel"] = float(np.max(np.abs(bo - np.array(fit_opt)) / np.array(fit_opt)))
    rec["sweep_speedup_vs_serial"] = rec["serial_phases"]["sweep_ms"] / max(rec["batched_phases"]["sweep_ms"], 1e-9)
    rec["end_to_end_speedup_vs_serial"] = rec["serial_ms"] / rec["batched_ms"]
    rec["end_to_end_speedup_vs_fits"] = rec["fits_ms"] / rec["batched_ms"]
    res["shapes"][s] = rec
    print(s, json.dumps(rec), flush=True)
ctx.close(); ctx_s.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
