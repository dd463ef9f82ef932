#!/usr/bin/env python3
"""Timing of the cross-validated multistart fit(Alt): the whole (F+1) x E x R table by
  batched — one partls_cv_alt call (all trajectories advance together),
  serial  — the same call under PARTLS_CV_SERIAL=1 (one problem after another: the single problem's prepare and multistart),
  loop    — (F+1) E public fit(Alt, X[train], y[train], P; η, alpha0=, beta0=) calls, what a user had to write before,
from host arrays, at the shapes
  many_groups — N = 20 000, D = 100, K = 50, F = 5, E = 8, R = 64      (K beyond the enumeration of Opt)
  wide        — N = 100 000, D = 256, K = 16, F = 5, E = 4, R = 256    (n = 257: the 512-thread register kernel)
Median wall time of 5 runs after a warm-up, with the minimum and maximum, and the call's phases (partls_get_timing: GRAM, PREP,
SWEEP = the iterations, FINISH) for the two cv_alt routes.  Every step is a child process of its own under a time limit; a step that
fails or runs out of time ends the tool (no retry) and is recorded as such.  Not a bench line.

    python tools/cv_alt_timing.py [OUT.json] [--shapes many_groups,wide] [--modes batched,serial,loop] [--reps 5] [--limit 600]
    rocprofv3 --kernel-trace --stats -- python tools/cv_alt_timing.py --step batched many_groups --reps 1     # the batched call alone
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"many_groups": dict(seed=31, N=20_000, D=100, K=50, F=5, R=64, etas=[0.0, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0]),
          "wide": dict(seed=37, N=100_000, D=256, K=16, F=5, R=256, etas=[0.0, 1.0, 10.0, 100.0])}
EPS, T = 1e-6, 100


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def step(mode, shape, reps):
    """one (mode, shape) measurement in this process; prints one JSON line"""
    if mode == "serial":
        os.environ["PARTLS_CV_SERIAL"] = "1"                 # read at partls_create
    sys.path.insert(0, ROOT)
    import numpy as np
    import partls_amd
    pls = partls_amd.package()
    L = pls.lowlevel
    s = SHAPES[shape]
    rng = np.random.default_rng(s["seed"])
    X = np.asfortranarray(rng.standard_normal((s["N"], s["D"])))
    P = np.zeros((s["D"], s["K"]), dtype=np.int64)
    P[np.arange(s["D"]), np.arange(s["D"]) % s["K"]] = 1
    y = X @ rng.standard_normal(s["D"]) + 0.2 * rng.standard_normal(s["N"])
    gen = np.random.default_rng(123)
    a0 = np.empty((s["R"], s["D"] + 1))
    b0 = np.empty((s["R"], s["K"] + 1))
    for r in range(s["R"]):
        a0[r] = gen.random(s["D"] + 1)
        b0[r] = (gen.random(s["K"] + 1) - 0.5) * 10
    fold_ptr, _ = pls.cv_folds(s["N"], s["F"])
    etas = np.asarray(s["etas"])
    ctx = pls.default_context(0)
    ctx.tolerate_ill = True
    ms, phases, opts = [], [], None
    for it in range(reps + 1):
        t0 = time.perf_counter()
        if mode == "loop":
            opts = np.empty((s["F"] + 1) * len(etas))
            for q in range(len(opts)):
                f, e = divmod(q, len(etas))
                tr = np.ones(s["N"], dtype=bool)
                if f < s["F"]:
                    tr[fold_ptr[f]:fold_ptr[f + 1]] = False
                _, _, rep = pls.fit(pls.Alt, X[tr], y[tr], P, η=float(etas[e]), ϵ=EPS, T=T, alpha0=a0, beta0=b0)
                opts[q] = rep.opt
        else:
            r = ctx.cv_alt(X, y, P, fold_ptr, etas, a0, b0, EPS, T)
            opts = r["opt"]
        dt = 1e3 * (time.perf_counter() - t0)
        if it > 0:
            ms.append(dt)
            if mode != "loop":
                phases.append({k: ctx.timing(getattr(L, "T_" + k)) for k in ("GRAM", "PREP", "SWEEP", "FINISH")})
    med = sorted(ms)[len(ms) // 2]
    out = dict(mode=mode, shape=shape, ms_median=med, ms_min=min(ms), ms_max=max(ms), ms_all=ms, opt_sum=float(np.nansum(opts)))
    if phases:
        out["phases_ms_median"] = {k: sorted(p[k] for p in phases)[len(phases) // 2] for k in phases[0]}
    print(json.dumps(out), flush=True)


def main():
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1].startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "cv_alt_timing.json")
    shapes = option("--shapes", "many_groups,wide").split(",")
    modes = option("--modes", "batched,serial,loop").split(",")
    reps, limit = int(option("--reps", "5")), int(option("--limit", "600"))
    res = dict(reps=reps, eps=EPS, T=T, shapes={k: {kk: vv for kk, vv in SHAPES[k].items()} for k in shapes}, steps=[])
    for shape in shapes:
        for mode in modes:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", mode, shape, "--reps", str(reps)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                res["steps"].append(dict(mode=mode, shape=shape, failed=True, returncode=p.returncode, stderr_tail=p.stderr[-2000:]))
                print("step %s / %s failed with exit status %d: stopping" % (mode, shape, p.returncode), flush=True)
                break
            res["steps"].append(json.loads(lines[-1]))
            print(lines[-1], flush=True)
        else:
            continue
        break
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    return 1 if any(s.get("failed") for s in res["steps"]) else 0


if __name__ == "__main__":
    if "--step" in sys.argv:
        i = sys.argv.index("--step")
        step(sys.argv[i + 1], sys.argv[i + 2], int(option("--reps", "5")))
    else:
        sys.exit(main())
