"""The rules of partls_robust_weights (include/partls_robust.h) restated in numpy, operation for operation, and the
IRLS loop of fit_robust written around fit(..., weights=): the yardsticks of tests/test_robust_binding.py and tests/test_gpu_robust.py.
Every numpy operation below is one IEEE fp64 operation per element, evaluated left to right as the header writes it."""
import warnings

import numpy as np

C_DEFAULT = {"huber": 1.345, "bisquare": 4.685}


def mad_scale(a):
    """median |residual| / 0.6745 with the median as 0.5 a_(lo) + 0.5 a_(hi), lo = (N - 1) // 2, hi = N // 2"""
    s = np.sort(np.asarray(a, dtype=np.float64))
    N = len(s)
    med = 0.5 * s[(N - 1) // 2] + 0.5 * s[N // 2]
    return med / 0.6745


def weights_rho(a, loss, c, s):
    """(w, rho) of the absolute residuals a at scale s > 0"""
    a = np.asarray(a, dtype=np.float64)
    c, s = float(c), float(s)
    k = c * s
    with np.errstate(all="ignore"):
        if loss == "huber":
            u = a / s
            inside = a <= k
            w = np.where(inside, 1.0, k / a)
            rho = np.where(inside, 0.5 * u * u, c * u - 0.5 * c * c)
        else:
            u = a / k
            v = 1.0 - u * u
            out = u >= 1.0
            top = c * c / 6.0
            w = np.where(out, 0.0, v * v)
            rho = np.where(out, top, top * (1.0 - v * v * v))
    return w, rho


def robust_info(a, loss="huber", c=None, scale=None, w_prev=None):
    """what partls_robust_weights returns for the absolute residuals a: dict(scale, weights, rho (per row), max_dw, n_down, n_zero);
    scale == 0: weights is None and the other fields are 0.  w_prev None: all ones"""
    a = np.asarray(a, dtype=np.float64)
    c = C_DEFAULT[loss] if c is None else c
    s = float(scale) if scale is not None and scale > 0 else float(mad_scale(a))
    if s == 0.0:
        return dict(scale=0.0, weights=None, rho=None, max_dw=0.0, n_down=0, n_zero=0)
    w, rho = weights_rho(a, loss, c, s)
    prev = np.ones(len(a)) if w_prev is None else w_prev
    return dict(scale=s, weights=w, rho=rho, max_dw=float(np.max(np.abs(w - prev))), n_down=int(np.sum(w < 1.0)),
                n_zero=int(np.sum(w == 0.0)))


def host_loop(partls, alg, X, y, P, *, loss="huber", c=None, scale=None, max_iter=50, tol=1e-6, **fit_kw):
    """The loop of fit_robust on the host: numpy weights and fit(alg, X, y, P, weights=w_j, ...).  Returns dict(models, reports,
    scales, max_dw, rho_sum (longdouble sums), iterations, converged, exact, weights)"""
    models, reports, scales, max_dws, rho_sums = [], [], [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", partls.IllConditionedWarning)
        m, _, rep = partls.fit(alg, X, y, P, **fit_kw)
        models.append(m); reports.append(rep)
        w = None
        iterations, converged, exact = 0, False, False
        for _ in range(max_iter):
            a = np.abs(partls.predict(models[-1], X) - np.asarray(y, dtype=np.float64))
            info = robust_info(a, loss, c, scale, w)
            scales.append(info["scale"]); max_dws.append(info["max_dw"])
            rho_sums.append(0.0 if info["rho"] is None else float(np.sum(info["rho"].astype(np.longdouble))))
            if info["scale"] == 0.0:
                converged = exact = True
                break
            w = info["weights"]
            if info["max_dw"] <= tol:
                converged = True
                break
            m, _, rep = partls.fit(alg, X, y, P, weights=w, **fit_kw)
            models.append(m); reports.append(rep)
            iterations += 1
    return dict(models=models, reports=reports, scales=scales, max_dw=max_dws, rho_sum=rho_sums, iterations=iterations,
                converged=converged, exact=exact, weights=np.ones(len(y)) if w is None else w)
