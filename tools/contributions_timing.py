#!/usr/bin/env python3
"""Cost of the N x K group contributions at the C3 test-set size (synthetic X, N = 100 000, M = 256, K = 16) for B = 1 and B = 100
random models, a host X and a device-resident X, float64 and float32, two ways:
  one    — one partls_contributions call for the full N x K x B array (one upload of a host X, one pass over X per 16 models);
  masked — the only route without it: K calls with all but one beta zeroed and t = 0 — partls_predict(_device) for B = 1,
           partls_predict_many(_device) for B = 100 — each of which uploads a host X and reads all of it;
and, beside them, `sums`: one partls_contributions call for the 3 K B sums alone (what group_importance asks for).
For B = 1 on a device-resident X the single partls_predict_device call on the same X is timed too: both read X once.
All in one process, alternating the forms; wall times in ms around calls that end in a stream synchronise: median, minimum and
maximum of `reps` rounds after one warm-up round.  `one` is compared with `masked` at the timed size (to rounding: the masked
predictions sum each group in predict's four-chain order).  Not a bench line: for DESIGN.md §4.16.

    python tools/contributions_timing.py [OUT.json] [--reps R] [--N N] [--B B]
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
out_path = args[0] if args else "profiles/contributions_timing.json"
for i, a in enumerate(sys.argv):
    if a in opts:
        opts[a] = int(sys.argv[i + 1])
reps, N, BMANY = opts["--reps"], opts["--N"], opts["--B"]
SEED, M, K = 20260103, 256, 16

P, ws = pls.synth_truth(SEED, M, K)
ctx = pls.Context(0)
dX64 = torch.empty(N * M, dtype=torch.float64, device="cuda")
dy = torch.empty(N, dtype=torch.float64, device="cuda")
ctx.synth_device(SEED, N, M, ws, dX64.data_ptr(), dy.data_ptr())
torch.cuda.synchronize()
dX32 = dX64.to(torch.float32)
rng = np.random.default_rng(SEED)


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


def close(c, masked):
    """`one` against the masked predictions, entry by entry, to the rounding of two summation orders of M / K terms each"""
    scale = np.abs(c).max()
    return bool(np.allclose(c, masked, rtol=0, atol=1e-12 * scale))


res = dict(N=N, M=M, K=K, reps=reps, cells={})
for B in (1, BMANY):
    alpha, beta = rng.random((B, M)), rng.normal(size=(B, K))
    zero_t = np.zeros(B)
    masks = [np.where(np.arange(K) == k, beta, 0.0) for k in range(K)]          # K copies of beta with one column kept
    for name, dX, dtype in (("float64", dX64, np.float64), ("float32", dX32, np.float32)):
        # ---- host pointers
        X = np.asfortranarray(dX.view(M, N).t().cpu().numpy())
        keep = {}

        def one():
            keep["one"] = ctx.contributions(X, P, alpha, beta)["contrib"]

        def sums():
            keep["sums"] = ctx.contributions(X, P, alpha, beta, want_contrib=False, want_sums=True)["sums"]

        def masked():
            if B == 1:
                keep["masked"] = np.stack([ctx.predict(X, P, alpha[0], mk[0], 0.0) for mk in masks], axis=1)[:, :, None]
            else:
                keep["masked"] = np.stack([ctx.predict_many(X, P, alpha, mk, zero_t)["yhat"] for mk in masks], axis=1)

        rec = rounds(dict(one=one, sums=sums, masked=masked))
        rec["one_close_to_masked"] = close(keep["one"], keep["masked"])
        rec["sums_equal_in_both_calls"] = bool(np.array_equal(
            keep["sums"], ctx.contributions(X, P, alpha, beta, want_contrib=True, want_sums=True)["sums"]))
        rec["speedup_vs_masked"] = rec["masked"]["median_ms"] / rec["one"]["median_ms"]
        res["cells"]["B%d_host_%s" % (B, name)] = rec
        print("B", B, "host", name, json.dumps(rec), flush=True)
        host_one = keep["one"]
        del X, keep
        # ---- device pointers: X and the N x K x B outputs stay in HBM
        dC = torch.zeros((B * K, N), dtype=torch.float64, device="cuda")
        dL = torch.zeros((K, B, N), dtype=torch.float64, device="cuda")
        dP = torch.zeros(N, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def one_d():
            ctx.contributions_device(dX.data_ptr(), N, M, N, P, alpha, beta, dcontrib_ptr=dC.data_ptr(), ldC=N, dtype=dtype)

        def sums_d():
            ctx.contributions_device(dX.data_ptr(), N, M, N, P, alpha, beta, want_sums=True, dtype=dtype)

        def masked_d():
            for k, mk in enumerate(masks):
                if B == 1:
                    ctx.predict_device(dX.data_ptr(), N, M, N, P, alpha[0], mk[0], 0.0, dL.data_ptr() + 8 * N * B * k, dtype=dtype)
                else:
                    ctx.predict_many_device(dX.data_ptr(), N, M, N, P, alpha, mk, zero_t, dyhat_ptr=dL.data_ptr() + 8 * N * B * k, ldY=N, dtype=dtype)

        def predict_d():
            ctx.predict_device(dX.data_ptr(), N, M, N, P, alpha[0], beta[0], 0.0, dP.data_ptr(), dtype=dtype)

        fns = dict(one=one_d, sums=sums_d, masked=masked_d)
        if B == 1:
            fns["predict"] = predict_d
        rec = rounds(fns)
        got = dC.cpu().numpy().reshape(B, K, N).transpose(2, 1, 0)
        rec["equal_host_form_bitwise"] = bool(np.array_equal(got, host_one))
        rec["one_close_to_masked"] = close(got, dL.cpu().numpy().transpose(2, 0, 1))
        rec["speedup_vs_masked"] = rec["masked"]["median_ms"] / rec["one"]["median_ms"]
        if B == 1:
            rec["one_over_predict"] = rec["one"]["median_ms"] / rec["predict"]["median_ms"]
        res["cells"]["B%d_device_%s" % (B, name)] = rec
        print("B", B, "device", name, json.dumps(rec), flush=True)
        del dC, dL, dP, got, host_one
ctx.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
