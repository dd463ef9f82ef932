#!/usr/bin/env python3
"""Cost of PARTLS_OPT_RESCUE_CAPPED on the design that is correlated throughout (n = 176, K = 5, every column from a
shared factor, 64 patterns of which 60 reach the default pivot cap).  Not a bench line: for DESIGN.md §4.14.

    python tools/rescue_timing.py [OUT.json]

One process, two contexts on the same data: without the flag (the sweep that gives up, its capped count and pivots) and with it (the
first pass, the second pass through the export pieces, the rescue kernel alone by HIP events, its pivots), each call repeated and the
median taken after a warm-up; then fit(Opt, rescue=True) end to end and the worst objective error against the CPU oracle.
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import partls_amd
import rescue_reference as R
from oracle import oracle as O

pls = partls_amd.package(); L = pls.lowlevel
REPS = 5
c = R.case("correlated")
X, y, P = c["X"], c["y"], c["P"]
O.build()
objs = O.fit_opt(X, y, P, return_all=True)["all_opt"]


def med(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        r = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), r


out = dict(design="correlated throughout (tests/rescue_reference.py: correlated_throughout)", n=c["n"], K=c["K"], patterns=64, reps=REPS,
           default_cap_rounds=20 * (c["n"] + 1), rescue_max_passes=3 * c["n"])
plain = pls.Context(0)
plain.opt_prepare(X, y, P, 0.0, L.OPT_FAITHFUL_INTERCEPT)
ms, r = med(lambda: plain.opt_sweep(0, -1, want_all=True))
out["plain_sweep_wall_ms"], out["plain_sweep_kernel_ms"] = ms, plain.timing(L.T_SWEEP)
out["plain_capped"], out["plain_pivots"] = int(r[3]), plain.pivots()
ms, m = med(lambda: plain.opt_models(raw=True))
out["plain_opt_models_wall_ms"], out["plain_opt_models_nan_rows"] = ms, int(np.isnan(m["opt"]).sum())
plain.close()

ctx = pls.Context(0)
ctx.opt_prepare(X, y, P, 0.0, L.OPT_FAITHFUL_INTERCEPT | L.OPT_RESCUE_CAPPED)
ms, r = med(lambda: ctx.opt_sweep(0, -1, want_all=True))
st = ctx.rescue_stats()
first = ctx.timing(L.T_SWEEP)                               # the first pass's kernel by HIP events + the second pass's wall time
out["rescue_sweep_wall_ms"] = ms
out["rescue_sweep_first_pass_kernel_plus_second_pass_wall_ms"] = first
out["second_pass_wall_ms"] = first - out["plain_sweep_kernel_ms"]
out["rescue_kernel_ms"] = ctx.timing(L.T_RESCUE)
out["rescued"], out["rescue_pivots"], out["rescue_failed"], out["unconverged_after_rescue"] = st.rescued, st.pivots, st.failed, int(r[3])
out["rescue_pivots_per_pattern"] = st.pivots / max(1, st.rescued)
out["total_pivots_with_rescue"] = ctx.pivots()
out["all_opt_max_rel_error_vs_oracle"] = float(np.max(np.abs(r[2] - objs) / np.maximum(1.0, objs)))
out["winner"], out["oracle_winner"] = int(r[1]), int(np.argmin(objs))
ms, m = med(lambda: ctx.opt_models(raw=True))
out["rescue_opt_models_wall_ms"], out["rescue_opt_models_nan_rows"] = ms, int(np.isnan(m["opt"]).sum())
out["rescue_opt_models_rescue_kernel_ms"] = ctx.timing(L.T_RESCUE)
ms, t = med(lambda: ctx.opt_top(8))
out["rescue_opt_top8_wall_ms"], out["rescue_opt_top8_count"] = ms, int(t["count"])
ctx.close()

ms, fit = med(lambda: pls.fit(pls.Opt, X, y, P, faithful_intercept=True, rescue=True))
out["fit_rescue_wall_ms"], out["fit_rescued"] = ms, int(fit[2].rescued)
out["fit_opt_rel_error_vs_oracle"] = float(abs(fit[2].opt - objs.min()) / max(1.0, objs.min()))
try:
    pls.fit(pls.Opt, X, y, P, faithful_intercept=True)
    out["fit_plain_status"] = 0
except pls.PartlsError as e:
    out["fit_plain_status"] = int(e.status)

print(json.dumps(out, indent=1))
if len(sys.argv) > 1 and not sys.argv[1].startswith("-"):
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
