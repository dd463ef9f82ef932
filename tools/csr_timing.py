#!/usr/bin/env python3
"""Cost of sparse design matrices: the CSR path against the dense fp64 path of the same build on the densified matrix,
the two alternated in one process, median of `reps` warm runs each.  Random-sparse matrices: a Bernoulli(density) mask times N(1, 1)
values, generated on the device.
  gram — device-resident prepares at C4 size (N = 1e6, M = 512, K = 16) and C3 size (N = 1e5, M = 256, K = 20), densities 1 %, 6.25 %
         and 25 %: partls_get_timing(GRAM) — for CSR the validation, the transposition and the Gram together, for dense gram_kernel +
         gram_reduce_kernel — and the largest difference of the two Grams relative to sqrt(G_pp G_qq);
  fit  — a device-resident C3 fit(Opt) at 6.25 %: prepare + sweep + finish (the finish runs the residual and X'r kernels: a rocprofv3
         --kernel-trace --stats pass of `--parts gram,fit` gives every kernel's time, the transposition's share among them);
  host — host-pointer prepares (wall time, partls_get_upload's ms and bytes) of both forms.
Not a bench line.

    python tools/csr_timing.py [OUT.json] [--reps R] [--parts gram,fit,host] [--shapes c3,c4]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package(); L = pls.lowlevel

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps, parts, shapes = 7, ("gram", "fit", "host"), ("c3", "c4")
for i, a in enumerate(sys.argv):
    if a == "--reps":
        reps = int(sys.argv[i + 1]); args.remove(sys.argv[i + 1])
    if a == "--parts":
        parts = tuple(sys.argv[i + 1].split(",")); args.remove(sys.argv[i + 1])
    if a == "--shapes":
        shapes = tuple(sys.argv[i + 1].split(",")); args.remove(sys.argv[i + 1])
out_path = args[0] if args else "profiles/csr_timing.json"
SHAPES = dict(c4=(20260004, 1_000_000, 512, 16), c3=(20260003, 100_000, 256, 20))
DENSITIES = (0.01, 0.0625, 0.25)


def device_data(seed, N, M, K, density):
    """(P, dense X column-major with leading dimension N, (indptr, indices, values) of the same matrix, y) on the device"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    Xr = torch.randn(N, M, dtype=torch.float64, device="cuda", generator=g) + 1.0          # row-major
    Xr *= torch.rand(N, M, device="cuda", generator=g) < density
    wstar = torch.randn(M, dtype=torch.float64, device="cuda", generator=g)
    dy = Xr @ wstar + 2.0 + 0.3 * torch.randn(N, dtype=torch.float64, device="cuda", generator=g)
    sp = Xr.to_sparse_csr()
    csr = (sp.crow_indices().to(torch.int64).contiguous(), sp.col_indices().to(torch.int32).contiguous(), sp.values().contiguous())
    dX = Xr.t().contiguous()                                                               # M x N row-major = N x M column-major
    del Xr, sp
    P = np.zeros((M, K), dtype=np.int64, order="F")
    P[np.arange(M), np.arange(M) % K] = 1
    torch.cuda.synchronize()
    return P, dX, csr, dy


def med(v):
    return float(np.median(v))


def prepare(ctx, kind, N, M, P, dX, csr, dy, flags):
    if kind == "csr":
        ctx.opt_prepare_csr_device(csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), dy.data_ptr(), N, M, P, 0.0, flags)
    else:
        ctx.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, M, N, P, 0.0, flags)


ctx = pls.Context(0)
res = dict(reps=reps, parts=list(parts), shapes=list(shapes))

if "gram" in parts:
    for shape in shapes:
        seed, N, M, K = SHAPES[shape]
        for d in DENSITIES:
            P, dX, csr, dy = device_data(seed, N, M, K, d)
            g = dict(dense=[], csr=[])
            G = {}
            for it in range(reps + 1):
                for kind in ("dense", "csr"):
                    prepare(ctx, kind, N, M, P, dX, csr, dy, L.OPT_FAITHFUL_INTERCEPT)
                    if it > 0:
                        g[kind].append(ctx.timing(L.T_GRAM))
                    else:
                        G[kind] = ctx.gram()
            dg = np.sqrt(np.abs(np.outer(np.diag(G["dense"]), np.diag(G["dense"]))))
            res["%s_gram_d%g" % (shape, d)] = dict(
                N=N, M=M, density=d, nnz=int(csr[2].numel()), gram_ms={k: med(v) for k, v in g.items()}, gram_ms_all=g,
                dense_spread_ms=max(g["dense"]) - min(g["dense"]), csr_over_dense=med(g["csr"]) / med(g["dense"]),
                max_rel_diff=float(np.max(np.abs(G["csr"] - G["dense"]) / np.maximum(dg, 1e-300))))
            del dX, csr, dy
            torch.cuda.empty_cache()

if "fit" in parts:
    seed, N, M, K = SHAPES["c3"]
    P, dX, csr, dy = device_data(seed, N, M, K, 0.0625)
    ph = dict(dense=[], csr=[])
    out = {}
    for it in range(reps + 1):
        for kind in ("dense", "csr"):
            t0 = time.perf_counter()
            prepare(ctx, kind, N, M, P, dX, csr, dy, 0)
            bo, bp, _, nu = ctx.opt_sweep(0, -1)
            r = ctx.opt_finish(bp)
            t1 = time.perf_counter()
            if it > 0:
                ph[kind].append(dict(wall_ms=1e3 * (t1 - t0), gram_ms=ctx.timing(L.T_GRAM), prep_ms=ctx.timing(L.T_PREP),
                                     sweep_ms=ctx.timing(L.T_SWEEP), finish_ms=ctx.timing(L.T_FINISH)))
            else:
                out[kind] = (int(bp), float(r[3]))
    summ = {k: {f: med([x[f] for x in v]) for f in v[0]} for k, v in ph.items()}
    res["c3_fit_device_d0.0625"] = dict(N=N, M=M, K=K, median=summ, wall_csr_over_dense=summ["csr"]["wall_ms"] / summ["dense"]["wall_ms"],
                                        same_pattern=out["csr"][0] == out["dense"][0],
                                        opt_rel_diff=abs(out["csr"][1] - out["dense"][1]) / out["dense"][1])
    del dX, csr, dy
    torch.cuda.empty_cache()

if "host" in parts:
    for shape in shapes:
        seed, N, M, K = SHAPES[shape]
        for d in DENSITIES:
            P, dX, csr, dy = device_data(seed, N, M, K, d)
            hy = dy.cpu().numpy()
            hX = np.asfortranarray(dX.t().cpu().numpy())
            hcsr = pls.CSR(csr[0].cpu().numpy(), csr[1].cpu().numpy(), csr[2].cpu().numpy(), (N, M))
            del dX, csr, dy
            torch.cuda.empty_cache()
            runs = dict(dense=[], csr=[])
            nrep = max(2, min(reps, 3))
            for it in range(nrep + 1):
                for kind in ("dense", "csr"):
                    t0 = time.perf_counter()
                    ctx.opt_prepare(hX if kind == "dense" else hcsr, hy, P, 0.0, L.OPT_FAITHFUL_INTERCEPT)
                    wall = 1e3 * (time.perf_counter() - t0)
                    up = ctx.upload()
                    if it > 0:
                        runs[kind].append(dict(wall_ms=wall, upload_ms=up[0], upload_bytes=up[1], gram_ms=ctx.timing(L.T_GRAM)))
            summ = {k: {f: med([x[f] for x in v]) for f in v[0]} for k, v in runs.items()}
            res["%s_host_prepare_d%g" % (shape, d)] = dict(N=N, M=M, density=d, median=summ, all=runs,
                                                           wall_csr_over_dense=summ["csr"]["wall_ms"] / summ["dense"]["wall_ms"])
            del hX, hcsr

ctx.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk not in ("gram_ms_all", "all")} if isinstance(v, dict) else v)
                  for k, v in res.items()}, indent=1))
