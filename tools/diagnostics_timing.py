#!/usr/bin/env python3
"""Cost of partls_diagnostics on device-resident data at the C3 shape (N = 100 000, M = 256) and the C4 shape (N = 1 000 000, M = 512):
synthetic X and y, K = 4 groups, a model with every feature active (p = M + 1: the largest triangular product the shape admits; the
model is not a fit — the cost does not depend on its values), all five per-row outputs and both standard errors wanted.
Per shape, medians of `reps` warm runs (one warm-up before them), each recorded on its own:
  call_ms      the whole partls_diagnostics call, host wall clock around the call (it ends in a stream synchronise);
  kernel_ms    the leverage kernel alone (device events around its launch: partls_get_diagnostics_timing);
  factor_ms    gathering H from the Gram copy, its Cholesky factor, T = L^-1 and the packing of its tiles, on the host;
and beside them
  gram_ms      the dense Gram build of the same library on the same X (PARTLS_T_GRAM of partls_opt_prepare: the same flop count,
               N p^2, as the triangular product), and both rates in TFLOP/s;
  qr_ms        numpy's Householder QR of [X 1] and the row norms of Q on the host, on `qr_rows` rows (all of them when they are at most
               200 000, else the first 200 000, with qr_ms_at_N the linear extrapolation to N);
  jackknife    partls_opt_weightings with the 256 weightings that leave out one of the first 256 rows (device-resident W), one run:
               the route to leave-one-out residuals without this entry; jackknife_ms_at_N extrapolates its per-row cost to N rows.
Not a bench line: for DESIGN.md §4.17.

    python tools/diagnostics_timing.py [OUT.json] [--reps R] [--shapes c3,c4]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import partls_amd
pls = partls_amd.package()
L = pls.lowlevel

opts = {"--reps": 5, "--shapes": "c3,c4"}
skip = {i + 1 for i, a in enumerate(sys.argv) if a in opts}
args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
out_path = args[0] if args else "profiles/diagnostics_timing.json"
for i, a in enumerate(sys.argv):
    if a in opts:
        opts[a] = type(opts[a])(sys.argv[i + 1])
reps = opts["--reps"]
SHAPES = dict(c3=(100_000, 256), c4=(1_000_000, 512))
SEED, K, JK, QR_ROWS = 20260104, 4, 256, 200_000


def median(v):
    return float(np.median(v))


res = dict(K=K, reps=reps, shapes={})
for name in opts["--shapes"].split(","):
    N, M = SHAPES[name]
    P, ws = pls.synth_truth(SEED, M, K)
    ctx = pls.Context(0)
    dX = torch.empty(N * M, dtype=torch.float64, device="cuda")
    dy = torch.empty(N, dtype=torch.float64, device="cuda")
    ctx.synth_device(SEED, N, M, ws, dX.data_ptr(), dy.data_ptr())
    outs = [torch.zeros(N, dtype=torch.float64, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()
    rng = np.random.default_rng(SEED)
    alpha, beta, t = rng.random(M) + 0.5, rng.normal(size=K) + np.where(np.arange(K) % 2, -2.0, 2.0), 0.25
    gram = []
    for _ in range(reps + 1):
        ctx.opt_prepare_device(dX.data_ptr(), dy.data_ptr(), N, M, N, P, 0.0)
        gram.append(ctx.timing(L.T_GRAM))
    ptrs = dict(zip(("dleverage_ptr", "dloo_ptr", "dstudentized_ptr", "dcooks_ptr", "dresidual_ptr"), (o.data_ptr() for o in outs)))
    call, kern, fact = [], [], []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.diagnostics_device(alpha, beta, t, **ptrs)
        call.append(1e3 * (time.perf_counter() - t0))
        k, f, _ = ctx.diagnostics_timing()
        kern.append(k); fact.append(f)
    p = int(out["summary"][L.DIAG_P])
    flops = float(N) * p * p                                              # N p^2 / 2 multiply-adds
    rec = dict(N=N, M=M, p=p, call_ms=median(call[1:]), kernel_ms=median(kern[1:]), factor_ms=median(fact[1:]), gram_ms=median(gram[1:]),
               call_ms_all=call[1:], kernel_ms_all=kern[1:], factor_ms_all=fact[1:], gram_ms_all=gram[1:],
               dof=float(out["summary"][L.DIAG_DOF]))
    rec["kernel_tflops"] = flops / (rec["kernel_ms"] * 1e-3) / 1e12
    rec["gram_tflops"] = float(N) * (M + 2) ** 2 / (rec["gram_ms"] * 1e-3) / 1e12
    rec["kernel_rate_over_gram_rate"] = rec["kernel_tflops"] / rec["gram_tflops"]
    h_dev = outs[0].cpu().numpy()
    # the host QR
    nq = min(N, QR_ROWS)
    Xo = np.ones((nq, M + 1), order="F")
    Xo[:, :M] = dX.view(M, N)[:, :nq].t().cpu().numpy()
    t0 = time.perf_counter()
    Q = np.linalg.qr(Xo)[0]
    h_qr = np.einsum("ij,ij->i", Q, Q)
    rec["qr_rows"], rec["qr_ms"] = nq, 1e3 * (time.perf_counter() - t0)
    rec["qr_ms_at_N"] = rec["qr_ms"] * N / nq
    if nq == N:
        rec["max_abs_leverage_minus_qr"] = float(np.max(np.abs(h_dev - h_qr)))
    del Xo, Q
    # the jackknife of JK rows through the batched resampling entry
    dW = torch.ones((JK, N), dtype=torch.float64, device="cuda")        # column j of the N x JK matrix W: row j left out
    dW[torch.arange(JK), torch.arange(JK)] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    jk = ctx.opt_weightings(None, None, P, None, 0.0, device_ptrs=(dX.data_ptr(), dy.data_ptr(), N, N, dW.data_ptr(), N, JK), oob=False)
    rec["jackknife_rows"], rec["jackknife_ms"] = JK, 1e3 * (time.perf_counter() - t0)
    rec["jackknife_ms_at_N"] = rec["jackknife_ms"] * N / JK
    rec["jackknife_status_ok"] = int(np.count_nonzero(jk["status"] == 0))
    res["shapes"][name] = rec
    print(name, json.dumps(rec), flush=True)
    ctx.close()
    del dX, dy, dW, outs
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
