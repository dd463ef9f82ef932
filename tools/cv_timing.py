#!/usr/bin/env python3
"""Cost of a cross-validation table of fit(Opt) (partls_cv_opt) three ways, on the same data and the same folds x η grid:
  batched  — one partls_cv_opt call (one upload, one Gram pass per fold, batched prep and sweep, per-problem finish);
  serial   — the same call under PARTLS_CV_SERIAL=1 (every problem prepared and swept on its own, same upload and fold Grams);
  fits     — E (F + 1) plain fit() calls from host arrays (each uploads its training rows and builds its own Gram).
Shapes: (a) N = 2e4, D = 48, K = 6, F = 5, E = 16; (b) C2 (N = 1e4, D = 128, K = 12), F = 5, E = 8; (c) N = 1e5, D = 256, K = 16, F = 5, E = 4.
Reports wall times (median of `reps` calls after one warm-up) and the phase split of the calls (partls_get_timing: GRAM, PREP, SWEEP summed
over the batch, FINISH = host wall time of the per-problem finishes).  Not a bench line: for DESIGN.md §4.6 / §7.

    python tools/cv_timing.py [OUT.json] [--shapes a,b,c] [--reps R]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package(); L = pls.lowlevel

SHAPES = {"a": (20260101, 20_000, 48, 6, 5, 16), "b": (20260002, 10_000, 128, 12, 5, 8), "c": (20260103, 100_000, 256, 16, 5, 4)}
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else "profiles/cv_timing.json"
which = "abc"
reps = 3
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
                                          ("calib_ms", L.T_CALIB))}


def timed(fn):
    fn()
    ts, ph = [], None
    for _ in range(reps):
        t0 = time.perf_counter(); r = fn(); ts.append(1e3 * (time.perf_counter() - t0))
        ph = r
    return float(np.median(ts)), ph


os.environ.pop("PARTLS_CV_SERIAL", None)
ctx = pls.Context(0)
os.environ["PARTLS_CV_SERIAL"] = "1"
ctx_s = pls.Context(0)
del os.environ["PARTLS_CV_SERIAL"]
res = dict(reps=reps, shapes={})
for s in which:
    seed, N, D, K, F, E = SHAPES[s]
    X, y, P = data(seed, N, D, K)
    fp, _ = pls.cv_folds(N, F)
    etas = np.concatenate([[0.0], np.logspace(-4, 1, E - 1)])
    rec = dict(N=N, D=D, K=K, F=F, E=E, problems=(F + 1) * E)

    def run(c):
        r = c.cv_opt(X, y, P, fp, etas, 0)
        return dict(phases(c), status_nonzero=int(np.count_nonzero(r["status"])), best_index=r["best_index"].tolist())

    rec["batched_ms"], rec["batched_phases"] = timed(lambda: run(ctx))
    rec["serial_ms"], rec["serial_phases"] = timed(lambda: run(ctx_s))
    same = rec["batched_phases"].pop("best_index") == rec["serial_phases"].pop("best_index")
    rec["batched_serial_same_winners"] = same
    train = []
    for f in range(F + 1):
        m = np.ones(N, dtype=bool)
        if f < F:
            m[fp[f]:fp[f + 1]] = False
        train.append((np.asfortranarray(X[m]), np.ascontiguousarray(y[m])))

    def fits():
        for Xt, yt in train:
            for eta in etas:
                pls.fit(pls.Opt, Xt, yt, P, η=float(eta))
        return None
    rec["fits_ms"], _ = timed(fits)
    rec["sweep_speedup_vs_serial"] = rec["serial_phases"]["sweep_ms"] / max(rec["batched_phases"]["sweep_ms"], 1e-9)
    rec["end_to_end_speedup_vs_fits"] = rec["fits_ms"] / rec["batched_ms"]
    res["shapes"][s] = rec
    print(s, json.dumps(rec), flush=True)
ctx.close(); ctx_s.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
