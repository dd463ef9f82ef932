#!/usr/bin/env python3
"""Cost of the k best patterns at C3, faithful (N = 100k, D = 256, K = 20: 2^21 patterns) — partls_opt_top against the export sweep of
the same range alone and against solutions.arrays() + np.lexsort.  Not a bench line: for DESIGN.md §4.13.

    python tools/opt_top_timing.py [OUT.json]      # wall times: opt_top(k) for k = 10, 100, 4096; the export sweep alone; arrays() + lexsort
    python tools/opt_top_timing.py --kernels K     # one opt_top(K) of the full range and nothing else after the warm-up: run under
                                                   # rocprofv3 --kernel-trace --stats for the selection / sort / gather / cleanup kernels
    python tools/opt_top_timing.py --merge STATS.csv OUT.json TAG   # fold the kernel times of such a run into OUT.json as kernels_TAG
                                                   # (TAG = yardstick: the trace of tools/models_timing.py --kernels, partls_opt_models' export sweep)

The export sweep alone is taken from the kernel traces (its launches are the same for every k); the wall time of opt_top(1) is
reported beside it.
"""
import csv, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = (("select", ("topk_init_kernel", "topk_hist_kernel", "topk_scan_kernel", "topk_compact_kernel")), ("sort", ("topk_sort_kernel",)),
          ("gather", ("topk_gather_kernel",)), ("cleanup", ("models_cleanup_kernel",)), ("sweep", ("sweep_",)))


def merge(stats_csv, out_json, tag):
    """kernel-trace --stats CSV (Name, Calls, TotalDurationNs, ...) -> out["kernels_" + tag]: ms and calls per phase, and the ratios"""
    out = json.load(open(out_json)) if os.path.exists(out_json) else {}
    ms = {p: 0.0 for p, _ in PHASES}
    calls = {p: 0 for p, _ in PHASES}
    sweeps = []
    for row in csv.DictReader(open(stats_csv)):
        name = row.get("Name") or row.get("KernelName") or ""
        for phase, keys in PHASES:
            if any(k in name for k in keys):
                if phase == "sweep":
                    sweeps.append((float(row["TotalDurationNs"]) * 1e-6, int(row["Calls"]), name))
                else:
                    ms[phase] += float(row["TotalDurationNs"]) * 1e-6
                    calls[phase] += int(row["Calls"])
                break
    # the export sweep is the row of the export instantiation (<T, false, true, ...>: chain mode, models); the plain sweep of
    # models_timing.py and the bit-order calibration's node-mode launch are the others
    export = [s for s in sweeps if ", false, true," in s[2]]
    rec = dict(ms=ms, calls=calls)
    if export:
        ms["sweep"], calls["sweep"], rec["export_sweep_kernel"] = max(export)
        rec["select_over_sweep"] = ms["select"] / ms["sweep"]
        rec["select_sort_gather_cleanup_over_sweep"] = (ms["select"] + ms["sort"] + ms["gather"] + ms["cleanup"]) / ms["sweep"]
    out["kernels_" + tag] = rec
    y = out.get("kernels_yardstick", {}).get("ms", {}).get("sweep")
    if y:
        for k in (10, 100, 4096):
            if "opt_top_k%d_s" % k in out:
                out["opt_top_k%d_wall_over_yardstick_sweep" % k] = out["opt_top_k%d_s" % k] * 1e3 / y
    json.dump(out, open(out_json, "w"), indent=1)
    print(json.dumps(out, indent=1))


if "--merge" in sys.argv:
    i = sys.argv.index("--merge")
    merge(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3])
    sys.exit(0)

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
ctx.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, D, N, P, 0.0, L.OPT_FAITHFUL_INTERCEPT)

if "--kernels" in sys.argv:                                  # no plain sweep: the only chain-mode sweep launches of the trace are the export's
    k = int(sys.argv[sys.argv.index("--kernels") + 1])
    ctx.opt_top(k)
    ctx.close()
    sys.exit(0)
ctx.opt_sweep(0, -1)                                         # the calibration runs here, before anything timed

out = dict(config="C3 faithful", N=N, D=D, K=K, patterns=npat, piece_bytes_cap=1 << 30)
ctx.opt_top(4096)                                            # warm: buffers, page-locked staging
for k in (1, 10, 100, 4096):
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        r = ctx.opt_top(k)
        best = min(best, time.perf_counter() - t0)
    out["opt_top_k%d_s" % k] = best
    assert r["count"] == k and r["n_unconverged"] == 0
out["n_vetoes"] = r["n_vetoes"]
top = r
t0 = time.perf_counter()
full = ctx.opt_models(0, -1)
out["opt_models_full_range_s"] = time.perf_counter() - t0
t0 = time.perf_counter()
order = np.lexsort((full["pattern"], full["opt"] + 0.0))[:4096]
out["lexsort_s"] = time.perf_counter() - t0
out["export_and_lexsort_s"] = out["opt_models_full_range_s"] + out["lexsort_s"]
# five pieces against partls_opt_models' nine: other chains, so the same patterns unless near ties swap places
out["top4096_patterns_equal_lexsort"] = bool(np.array_equal(top["pattern"], full["pattern"][order]))
out["top4096_max_abs_opt_difference"] = float(np.abs(top["opt"] - full["opt"][order]).max())
for k in (10, 100, 4096):
    out["opt_top_k%d_over_k1" % k] = out["opt_top_k%d_s" % k] / out["opt_top_k1_s"]
ctx.close()
print(json.dumps(out, indent=1))
if len(sys.argv) > 1 and not sys.argv[1].startswith("-"):
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
