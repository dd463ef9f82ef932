"""The yardsticks of the generalised linear fits, none of them the code under test:
  * rows(): the operation lists of include/partls_glm.h restated in numpy, operation for operation, in float64 or — the reference of
    the GPU tests — in np.longdouble;
  * bounds(): the header's derived error bound of a row, from its constants (read from the header, not copied);
  * host_loop(): the loop of fit_glm written around Context.glm_working and fit(alg, X, z, P, weights=W);
  * irls(): an independent IRLS — numpy rows, and for the weighted least-squares step the oracle's Opt enumeration on homogeneous rows
    scaled by sqrt(W), the intercept column with them;
  * fixture(): the committed problems of tests/golden/glm_*.npz and how they were chosen (python tests/glm_reference.py writes them)."""
import os
import re
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "partls_glm.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FAMILIES = ("binomial", "poisson")
CLAMP = 30.0


def constants():
    """the PARTLS_GLM_* numbers of the header"""
    text = open(HEADER).read()
    return {k: float(v) for k, v in re.findall(r"#define PARTLS_GLM_(\w+) ([0-9.e+-]+)\s", text)}


def _xlogy(a):
    a = np.asarray(a)
    safe = np.where(a == 0, 1, a).astype(a.dtype)
    return np.where(a == 0, 0, a * np.log(safe)).astype(a.dtype)


def start_eta(y, family, dtype=np.float64):
    y = np.asarray(y, dtype=dtype)
    if family == "binomial":
        m0 = (y + dtype(0.5)) / dtype(2)
        return np.log(m0 / (dtype(1) - m0))
    return np.log(y + dtype(0.1))                            # the double nearest 0.1 in either precision: the device's constant


def rows(eta, y, family, dtype=np.float64):
    """dict(W, z, mu, d, ec, clamped, S): the header's formulas in `dtype`; S is the magnitude sum its bound of d refers to"""
    eta, y = np.asarray(eta, dtype=dtype), np.asarray(y, dtype=dtype)
    one, two = dtype(1), dtype(2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        ec = np.minimum(np.maximum(eta, dtype(-CLAMP)), dtype(CLAMP))
        if family == "binomial":
            ae = np.abs(ec)
            pos = ec >= 0
            e = np.exp(-ae)
            q = one / (one + e)
            p = e * q
            mu = np.where(pos, q, p)
            W = p * q
            z = ec + (y - mu) / W
            l = np.log1p(e)
            far = ae + l
            nlmu, nlnu = np.where(pos, l, far), np.where(pos, far, l)
            omy = one - y
            d = two * ((_xlogy(y) + _xlogy(omy)) + (y * nlmu + omy * nlnu))
            r = np.where((y > 0) & (y < 0.5), omy, 0)
            S = np.abs(_xlogy(y)) + np.abs(_xlogy(omy)) + r + y * nlmu + omy * nlnu
        else:
            mu = np.exp(ec)
            W = mu
            z = ec + (y - mu) / mu
            d = two * ((_xlogy(y) - y * ec) - (y - mu))
            S = np.abs(_xlogy(y)) + np.abs(y * ec) + np.abs(y) + mu
    return dict(W=W, z=z, mu=mu, d=d, ec=ec, clamped=eta != ec, S=S)


def bounds(ref, eta, y, start, family):
    """the header's bounds around the longdouble rows `ref` (of eta, y in longdouble): dict(mu, W, z, d), absolute, per row"""
    k = constants()
    u = np.longdouble(k["U"])
    y = np.asarray(y, dtype=np.longdouble)
    eta = np.asarray(eta, dtype=np.longdouble)
    mu, W, ec, S = ref["mu"], ref["W"], ref["ec"], ref["S"]
    lever = (np.abs(y) + mu) / W
    b = dict(mu=k["MU_ULPS"] * u * mu, W=k["W_ULPS"] * u * W, z=k["Z_ULPS"] * u * (np.abs(ec) + lever), d=k["D_ULPS"] * u * 2 * S)
    if start:
        de = (k["START_ETA_ULPS"] + 2 * np.abs(eta)) * u
        b = dict(mu=b["mu"] + de * mu, W=b["W"] + de * W, z=b["z"] + de * (1 + lever), d=b["d"] + 2 * de * (np.abs(y) + mu))
    return b


def check_rows(got, eta, y, family, start, where=""):
    """got: dict(W, z, mu[, d]) of float64 rows computed from (eta, y) — eta None for the start.  Asserts the header's bound against the
    longdouble restatement; returns (reference rows, bounds)."""
    yl = np.asarray(y, dtype=np.longdouble)
    el = start_eta(yl, family, np.longdouble) if start else np.asarray(eta, dtype=np.longdouble)
    ref = rows(el, yl, family, np.longdouble)
    b = bounds(ref, el, yl, start, family)
    worst = {}
    for name in ("mu", "W", "z", "d"):
        if name not in got or got[name] is None:
            continue
        err = np.abs(np.asarray(got[name], dtype=np.longdouble) - ref[name])
        ratio = np.where(err == 0, 0, err / np.where(b[name] == 0, np.finfo(np.longdouble).tiny, b[name]))
        worst[name] = float(np.max(ratio)) if ratio.size else 0.0
        i = int(np.argmax(ratio)) if ratio.size else 0
        assert worst[name] <= 1.0, (where, family, name, i, float(el[i]), float(yl[i]), float(np.asarray(got[name])[i]), float(ref[name][i]),
                                    float(err[i]), float(b[name][i]))
    print("[glm]%s %s start=%s N=%d: worst error / bound %r" % (where, family, start, len(yl), worst))
    return ref, b


def null_deviance(y, family):
    """the deviance of the intercept-only model: mu = mean(y) under both canonical links"""
    y = np.asarray(y, dtype=np.longdouble)
    m = np.mean(y)
    if family == "binomial":
        d = (_xlogy(y) + _xlogy(1 - y)) - (y * np.log(m) + (1 - y) * np.log1p(-m))
    else:
        d = (_xlogy(y) - y * np.log(m)) - (y - m)
    return float(2 * np.sum(d))


def converged(dev, prev, tol):
    return abs(dev - prev) <= tol * (abs(dev) + 0.1)


def host_loop(partls, ctx, alg, X, y, P, *, family, max_iter=25, tol=1e-8, **fit_kw):
    """The loop of fit_glm on the host: the rows of Context.glm_working (ctx prepared here on X, y) and a fresh
    fit(alg, X, z, P, weights=W, ...) per iteration.  Returns dict(models, reports, deviance, iterations, converged, last)."""
    models, reports, devs = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", partls.IllConditionedWarning)
        ctx.opt_prepare(X, y, P)
        info = ctx.glm_working(None, family)
        devs.append(info["deviance"])
        iterations, done = 0, False
        for _ in range(max_iter):
            m, _, rep = partls.fit(alg, X, info["working_response"], P, weights=info["weights"], **fit_kw)
            models.append(m); reports.append(rep)
            iterations += 1
            info = ctx.glm_working(m, family)
            devs.append(info["deviance"])
            if converged(devs[-1], devs[-2], tol):
                done = True
                break
    return dict(models=models, reports=reports, deviance=devs, iterations=iterations, converged=done, last=info)


# ---- an independent IRLS: numpy rows, the oracle's enumeration for every weighted least-squares step --------------------------------
def _oracle_wls(oracle, X, z, P, W):
    """min over sign patterns of || sqrt(W) (Xo w - z) ||, Xo = [X 1] — the loop body of the oracle's fit_opt on homogeneous rows scaled
    by sqrt(W), the intercept column with them.  Returns (alpha, beta, t, objectives of all 2^(K+1) patterns)."""
    M, K = P.shape
    Xo, Po = oracle.homogeneous(X, P)
    s = np.sqrt(W)
    objs, ra = oracle.opt_patterns(np.asfortranarray(Xo * s[:, None]), z * s, Po, np.arange(1 << (K + 1)), want_alpha=True)
    b = int(np.argmin(objs))
    a_r = ra[b][:M]
    sign = np.array([1.0 if (b >> k) & 1 else -1.0 for k in range(K)])
    sums = P.T @ a_r
    beta = sign * sums
    alpha = (P * (a_r[:, None] / np.where(sums == 0.0, 1.0, sums)[None, :])).sum(axis=1)
    t = (1.0 if (b >> K) & 1 else -1.0) * ra[b][M]
    return alpha, beta, float(t), objs


def irls(oracle, X, y, P, family, max_iter=25, tol=1e-8):
    """dict(alpha, beta, t, deviance (list), iterations, converged, gaps (per iteration: relative gap between the best and the second
    best DISTINCT pattern objective), margins (per iteration: |d dev| / (tol (|dev| + 0.1))))"""
    X = np.asarray(X, dtype=np.float64)
    r = rows(start_eta(y, family), y, family)
    devs, gaps, margins = [float(np.sum(r["d"]))], [], []
    done, model = False, None
    for _ in range(max_iter):
        alpha, beta, t, objs = _oracle_wls(oracle, X, r["z"], P, r["W"])
        so = np.sort(objs)
        gaps.append(float((so[1] - so[0]) / so[0]))
        model = (alpha, beta, t)
        r = rows(X @ (alpha * (P @ beta)) + t, y, family)
        devs.append(float(np.sum(r["d"])))
        margins.append(abs(devs[-1] - devs[-2]) / (tol * (abs(devs[-1]) + 0.1)))
        if converged(devs[-1], devs[-2], tol):
            done = True
            break
    return dict(alpha=model[0], beta=model[1], t=model[2], deviance=devs, iterations=len(gaps), converged=done, gaps=gaps, margins=margins)


# ---- the committed problems ----------------------------------------------------------------------------------------------------------
FIXTURES = {"binomial": ("glm_binomial.npz", 20261021), "poisson": ("glm_poisson.npz", 20261022)}
FIX_N, FIX_M, FIX_K = 400, 8, 3


def make_problem(family, seed):
    """a synthetic problem with a planted model: N = 400, M = 8, K = 3.  The response is the planted mean observed with 1 % noise — a
    proportion in (0, 1), a rate > 0 — not a 0/1 draw or a count: the final deviance has to lie below dev_0, the deviance of the
    STARTING means (y + 0.5) / 2 or y + 0.1, and those sit so close to the saturated model (0.2 per zero count, about 0.01 / y per
    larger one, 2 log(4/3) per 0/1 row) that only a response the model can nearly reproduce gets under it.  0/1 and count responses
    are the data of the host-loop tests (tests/test_gpu_glm.py, 3.)."""
    rng = np.random.default_rng(seed)
    N, M, K = FIX_N, FIX_M, FIX_K
    X = rng.normal(0.0, 1.0, (N, M))
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), np.arange(M) % K] = 1
    alpha = rng.uniform(0.3, 1.0, M)
    alpha /= P @ (P.T @ alpha)
    beta = np.array([1.2, -0.9, 0.7])
    eta = X @ (alpha * (P @ beta)) + (0.3 if family == "binomial" else 0.8)
    noise = 1.0 + 0.01 * rng.normal(size=N)
    y = np.clip(noise / (1.0 + np.exp(-eta)), 1e-3, 1.0 - 1e-3) if family == "binomial" else np.exp(eta) * noise
    return X, y, P


def fixture(family):
    """(X, y, P, recorded reference: dict(alpha, beta, t, deviance)) of tests/golden"""
    f = np.load(os.path.join(GOLDEN, FIXTURES[family][0]))
    return f["X"], f["y"], f["P"], dict(alpha=f["alpha"], beta=f["beta"], t=float(f["t"]), deviance=f["deviance"])


def fixture_ok(ref):
    """the two conditions a committed problem meets at every iteration of the reference's own loop, and a stopping decision that no
    rounding can turn (every |d dev| a factor 4 away from its threshold)"""
    return (ref["converged"] and ref["iterations"] <= 25 and min(ref["gaps"]) > 1e-6 and all(m < 0.25 or m > 4.0 for m in ref["margins"])
            and ref["deviance"][-1] < ref["deviance"][0])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    for fam, (name, seed) in FIXTURES.items():
        X, y, P = make_problem(fam, seed)
        ref = irls(O, X, y, P, fam)
        print(fam, "iterations", ref["iterations"], "min gap %.3g" % min(ref["gaps"]), "margins", ["%.3g" % m for m in ref["margins"]],
              "deviance", ref["deviance"][-1], "null", null_deviance(y, fam))
        assert fixture_ok(ref), fam
        np.savez(os.path.join(GOLDEN, name), X=X, y=y, P=P, alpha=ref["alpha"], beta=ref["beta"], t=ref["t"], deviance=np.array(ref["deviance"]))
