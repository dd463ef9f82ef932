"""Helpers of the model-export comparisons (partls_opt_models against the oracle), shared by test_gpu_models.py and
test_gpu_tile_counts.py.  TEST INFRASTRUCTURE ONLY (imported by tests; not a conftest.py, not collected)."""
import numpy as np


def _close(a, ref, tol=1e-9):
    a, ref = np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape
    err = np.abs(a - ref) / np.maximum(1.0, np.abs(ref))
    assert np.all(err <= tol), f"max relative error {err.max():.3e}"


def _scatter(r, npat):
    """export rows (visiting order) -> arrays indexed by the reference pattern; every pattern exactly once"""
    pat = r["pattern"]
    assert np.array_equal(np.sort(pat), np.arange(npat))
    out = {}
    for k in ("opt", "alpha", "beta", "t", "raw_alpha"):
        if k in r:
            v = np.empty_like(r[k])
            v[pat] = r[k]
            out[k] = v
    return out


def _cleanup(raw, P, b):
    """cleanupResult (Opt.jl:34-44) from nonneg_lsq's alpha of pattern b (numpy; the reference formula)"""
    M, K = P.shape
    a = raw[:M]
    s = np.array([1.0 if (b >> k) & 1 else -1.0 for k in range(K)])
    sums = P.T @ a
    beta = s * sums
    A = np.where(sums == 0.0, 1.0, sums)
    alpha = (P * (a[:, None] / A[None, :])).sum(axis=1)
    f = 1.0 if (b >> K) & 1 else -1.0
    return alpha, beta, f * raw[M]
