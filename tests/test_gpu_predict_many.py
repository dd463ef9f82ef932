"""GPU tests of partls_predict_many: every column equals the single prediction it replaces bit for bit (and a numpy
restatement of the four-chain order), for float64 and float32 X, host and device pointers; the per-row order statistics and the mean
are exact, ties included; the row chunks of a call join without a seam; bad calls are refused and leave the context usable; and a
bootstrap's band is np.percentile of its replicates' predictions."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _chunk(partls):
    return partls.lowlevel.PREDICT_MANY_CHUNK


def _partition(M):
    K = min(3, M)
    P = np.zeros((M, K), dtype=np.int64)
    P[np.arange(M), np.arange(M) % K] = 1
    return P


def _models(rng, B, M, K):
    return rng.normal(size=(B, M)), rng.normal(size=(B, K)), rng.normal(size=B)


@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_columns_equal_the_single_predictions_bitwise(partls, N):
    """N: one lane, a block less one row, a block and one row, four blocks; M: below, at and above the four chains and with every
    remainder; B: one model, a chunk less one, a chunk, a chunk and one, two chunks and three"""
    C = _chunk(partls)
    rng = np.random.default_rng(N)
    ctx = partls.default_context()
    for M in (1, 3, 4, 5, 17):
        P = _partition(M)
        X = np.asfortranarray(rng.normal(size=(N, M)))
        for B in (1, C - 1, C, C + 1, 2 * C + 3):
            a, b, t = _models(rng, B, M, P.shape[1])
            Y = partls.predict_many((a, b, t, P), X)
            assert Y.shape == (N, B) and Y.dtype == np.float64
            for j in range(B):
                assert np.array_equal(Y[:, j], ctx.predict(X, P, a[j], b[j], t[j])), (M, B, j)


def _exact_inputs(rng, N, M, K, B):
    """X, alpha, beta, t whose products are exact in float64 — X has 21 significant bits, alpha and beta 10 each, so w = alpha beta has
    20 and x w 41 — while the sums are not: the columns of X and the models differ in scale by up to 2^20.  On such data fma(x, w, a)
    is the rounded x * w + a of plain numpy, so the four-chain order can be restated without an fma."""
    X = rng.integers(-2 ** 20, 2 ** 20, size=(N, M)).astype(np.float64) * 2.0 ** rng.integers(-10, 11, size=(1, M))
    a = rng.integers(1, 1024, size=(B, M)).astype(np.float64) / 64.0
    b = rng.integers(-512, 512, size=(B, K)).astype(np.float64) * 2.0 ** rng.integers(-10, 1, size=(B, 1))
    t = rng.integers(-2 ** 20, 2 ** 20, size=B).astype(np.float64) / 1024.0
    return np.asfortranarray(X), a, b, t


def _four_chains(X, P, a, b, t):
    """the contract, restated: w_m = sum over k in order of P[m,k] alpha_m beta_k; chains c = 0..3 over the columns m = c mod 4 of the
    first 4 floor(M / 4), the remaining columns on chain 0; ((a0 + a1) + (a2 + a3)) + t"""
    N, M = X.shape
    w = np.zeros(M)
    for k in range(P.shape[1]):
        w = w + P[:, k] * a * b[k]
    acc = [np.zeros(N) for _ in range(4)]
    m4 = M - M % 4
    for m in range(m4):
        acc[m % 4] = X[:, m] * w[m] + acc[m % 4]
    for m in range(m4, M):
        acc[0] = X[:, m] * w[m] + acc[0]
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + t


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_columns_equal_the_four_chain_order_restated_in_numpy(partls, dtype):
    C = _chunk(partls)
    rng = np.random.default_rng(5)
    for N, M, B in ((257, 1, 1), (257, 3, C + 1), (1000, 4, C - 1), (255, 5, 2 * C + 3), (1000, 17, C), (257, 23, 3)):
        P = _partition(M)
        X, a, b, t = _exact_inputs(rng, N, M, P.shape[1], B)
        assert np.array_equal(X.astype(dtype).astype(np.float64), X)         # 21 bits: float32 holds them
        Y = partls.predict_many((a, b, t, P), X.astype(dtype))
        ref = np.stack([_four_chains(X, P, a[j], b[j], t[j]) for j in range(B)], axis=1)
        assert np.array_equal(Y, ref), (N, M, B)
        if M >= 8:
            naive = X @ (a * (b @ P.T)).T + t
            assert not np.array_equal(naive, ref)                             # the data do round: another order gives other bits


def test_float32_X_equals_its_widened_copy(partls):
    C = _chunk(partls)
    rng = np.random.default_rng(6)
    for N, M, B in ((257, 5, C + 1), (1000, 17, 2 * C + 3), (1, 1, 1)):
        P = _partition(M)
        X32 = rng.normal(size=(N, M)).astype(np.float32)
        a, b, t = _models(rng, B, M, P.shape[1])
        r32 = partls.default_context().predict_many(X32, P, a, b, t, ranks=[0, B - 1], want_mean=True)
        r64 = partls.default_context().predict_many(X32.astype(np.float64), P, a, b, t, ranks=[0, B - 1], want_mean=True)
        for k in ("yhat", "stats", "mean"):
            assert np.array_equal(r32[k], r64[k]), (N, M, B, k)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_pointers_with_padded_leading_dimensions(partls, dtype):
    import torch
    C = _chunk(partls)
    rng = np.random.default_rng(7)
    N, M, B, ldX, ldY = 257, 5, C + 1, 300, 290
    P = _partition(M)
    X = rng.normal(size=(N, M)).astype(dtype)
    a, b, t = _models(rng, B, M, P.shape[1])
    ranks = [0, 3, B - 1]
    want = partls.default_context().predict_many(X, P, a, b, t, ranks=ranks, want_mean=True)
    Xp = np.full((M, ldX), np.nan, dtype=dtype)                   # M x ldX row-major == N x M column-major with leading dimension ldX
    Xp[:, :N] = X.T
    dX = torch.from_numpy(Xp).cuda()
    dY = torch.full((B, ldY), -7.5, dtype=torch.float64, device="cuda")
    dS = torch.full((len(ranks), N), -7.5, dtype=torch.float64, device="cuda")
    dM = torch.full((N,), -7.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx = partls.default_context()
    ctx.predict_many_device(dX.data_ptr(), N, M, ldX, P, a, b, t, dyhat_ptr=dY.data_ptr(), ldY=ldY, ranks=ranks, dstats_ptr=dS.data_ptr(),
                            dmean_ptr=dM.data_ptr(), dtype=dtype)
    Y = dY.cpu().numpy()
    assert np.array_equal(Y[:, :N].T, want["yhat"])
    assert np.all(Y[:, N:] == -7.5)                               # the padding rows of yhat are not written
    assert np.array_equal(dS.cpu().numpy().T, want["stats"]) and np.array_equal(dM.cpu().numpy(), want["mean"])
    # statistics only: no yhat on the device either
    dS.fill_(-7.5)
    dM.fill_(-7.5)
    torch.cuda.synchronize()
    ctx.predict_many_device(dX.data_ptr(), N, M, ldX, P, a, b, t, ranks=ranks, dstats_ptr=dS.data_ptr(), dmean_ptr=dM.data_ptr(), dtype=dtype)
    assert np.array_equal(dS.cpu().numpy().T, want["stats"]) and np.array_equal(dM.cpu().numpy(), want["mean"])


def _index_ordered_mean(Y):
    return np.array([sum(row) / len(row) for row in Y.tolist()])


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 100, 1000])
def test_every_rank_and_the_mean_are_exact(partls, B):
    """B either side of a power of two (the sort pads to one), one and two models, more rows than one workgroup sorts at once (8 of
    them, 4 at B = 1000; N = 300 leaves the last workgroup of 8 half empty); ties: models 1 and B - 1 duplicate model 0, and the
    all-zero rows of X predict the intercepts, which take only three values"""
    _ranks_and_mean(partls, B, 300)


@pytest.mark.parametrize("B", [129, 256, 257, 512, 513, 1025, 2048, 2049])
def test_every_group_shape_of_the_row_sort(partls, B):
    """the sort pads a row to n = the power of two >= B and a workgroup sorts R = rows_per_group(n) rows at once: R = 8 at n = 256 and
    512 (B = 129, 256 | 257, 512), 4 at n = 1024 (513), 2 at n = 2048 (1025, 2048: nothing padded) and 1 at n = 4096 with 2047 pads of
    +inf (2049).  N = 37 leaves the last workgroup ragged for R = 8, 4 and 2.  Every rank, the duplicate models and the intercept-only
    rows as above; np.sort and the index-ordered mean, exact"""
    n = 1
    while n < B:
        n <<= 1
    assert (n, 8 if n <= 512 else 4096 // n) in ((256, 8), (512, 8), (1024, 4), (2048, 2), (4096, 1))
    _ranks_and_mean(partls, B, 37)


def _ranks_and_mean(partls, B, N):
    rng = np.random.default_rng(B)
    M = 4
    P = _partition(M)
    X = np.asfortranarray(rng.normal(size=(N, M)))
    X[::7] = 0.0
    a, b, t = _models(rng, B, M, P.shape[1])
    t = rng.integers(0, 3, size=B).astype(np.float64)
    a[B - 1], b[B - 1], t[B - 1] = a[0], b[0], t[0]
    if B > 2:
        a[1], b[1], t[1] = a[0], b[0], t[0]
    r = partls.default_context().predict_many(X, P, a, b, t, ranks=np.arange(B), want_mean=True)
    Y = r["yhat"]
    assert np.array_equal(Y[::7], np.broadcast_to(t, (len(Y[::7]), B)))
    assert np.array_equal(r["stats"], np.sort(Y, axis=1))
    assert np.array_equal(r["mean"], _index_ordered_mean(Y))
    # ranks in any order, repeated
    pick = [B - 1, 0, B // 2, 0]
    r2 = partls.default_context().predict_many(X, P, a, b, t, ranks=pick, want_yhat=False)
    assert r2["yhat"] is None and r2["mean"] is None and np.array_equal(r2["stats"], np.sort(Y, axis=1)[:, pick])


def test_row_chunks_join_without_a_seam(partls):
    """B at the cap and the smallest N whose N x B doubles exceed the byte budget: two row chunks, the second of one row; then B = 1000 and
    three chunks (twice 8388 rows and three), every output compared with the single-chunk calls on the chunks' rows"""
    L = partls.lowlevel
    B, M = L.PREDICT_MANY_MAX_B, 2
    rows = L.PREDICT_MANY_BYTES // (8 * B)
    N = rows + 1
    assert N * B * 8 > L.PREDICT_MANY_BYTES >= rows * B * 8
    rng = np.random.default_rng(11)
    P = _partition(M)
    X = np.asfortranarray(rng.normal(size=(N, M)))
    a, b, t = _models(rng, B, M, P.shape[1])
    ranks = [0, 1, B // 2 - 1, B // 2, B - 2, B - 1]
    ctx = partls.default_context()
    r = ctx.predict_many(X, P, a, b, t, ranks=ranks, want_mean=True)
    Y = r["yhat"]
    for j in (0, 1, 15, 16, B // 2, B - 17, B - 1):
        assert np.array_equal(Y[:, j], ctx.predict(X, P, a[j], b[j], t[j])), j
    srt = np.sort(Y, axis=1)
    edges = [0, rows - 1, rows, N - 1]                            # first and last row of either chunk
    for i in edges:
        assert np.array_equal(r["stats"][i], srt[i, ranks]), i
        assert r["mean"][i] == sum(Y[i].tolist()) / B, i
        w = a * (b @ P.T)                                          # one group per feature: w = alpha beta, no sum
        assert np.allclose(Y[i], X[i] @ w.T + t, rtol=0, atol=1e-12 * (1 + np.abs(X[i]) @ np.abs(w.T)))
    assert np.array_equal(r["stats"], srt[:, ranks])
    assert np.array_equal(r["mean"], _index_ordered_mean(Y))
    # the same statistics when no yhat is wanted (the intermediate never leaves the device)
    r2 = ctx.predict_many(X, P, a, b, t, ranks=ranks, want_yhat=False, want_mean=True)
    assert np.array_equal(r2["stats"], r["stats"]) and np.array_equal(r2["mean"], r["mean"])
    # host arrays, yhat, stats and mean all wanted, three row chunks with an odd tail of three rows: each output goes back to the host
    # chunk by chunk, and every chunk's rows are bit for bit those of the single-chunk call on that row range
    B, M = 1000, 7
    rows = L.PREDICT_MANY_BYTES // (8 * B)
    N = 2 * rows + 3
    P = _partition(M)
    X = np.asfortranarray(rng.normal(size=(N, M)))
    a, b, t = _models(rng, B, M, P.shape[1])
    ranks = [0, B // 2, B - 1]
    r = ctx.predict_many(X, P, a, b, t, ranks=ranks, want_mean=True)
    for r0 in range(0, N, rows):
        part = ctx.predict_many(np.asfortranarray(X[r0:r0 + rows]), P, a, b, t, ranks=ranks, want_mean=True)
        assert part["yhat"].shape[0] * max(B, len(ranks)) * 8 <= L.PREDICT_MANY_BYTES       # the reference call is one chunk
        for k in ("yhat", "stats", "mean"):
            assert np.array_equal(r[k][r0:r0 + rows], part[k]), (r0, k)


def test_bad_calls_are_refused_and_the_context_still_predicts(partls):
    L = partls.lowlevel
    rng = np.random.default_rng(12)
    N, M = 40, 5
    P = _partition(M)
    K = P.shape[1]
    X = np.asfortranarray(rng.normal(size=(N, M)))
    a, b, t = _models(rng, 6, M, K)
    ctx = partls.Context(0)
    want = ctx.predict(X, P, a[0], b[0], t[0])
    Pf = np.asfortranarray(P, dtype=np.int64)
    yh = np.zeros((N, L.PREDICT_MANY_MAX_B + 1), order="F")

    def call(a, b, t, yhat=yh, ranks=None, stats=None, mean=None):
        """the entry itself, past the binding's own checks"""
        a, b, t = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, b, t))
        r = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.int64)
        ctx._predict_many(X.ctypes.data, 0, False, N, M, N, Pf, a, b, t, None if yhat is None else yhat.ctypes.data, N, r,
                          None if stats is None else stats.ctypes.data, None if mean is None else mean.ctypes.data)

    def refused(status, *args, **kw):
        with pytest.raises(partls.PartlsError) as e:
            call(*args, **kw)
        assert e.value.status == status, e.value
        assert np.array_equal(ctx.predict(X, P, a[0], b[0], t[0]), want)

    big = L.PREDICT_MANY_MAX_B + 1
    refused(L.ERR_UNSUPPORTED, np.ones((big, M)), np.ones((big, K)), np.zeros(big))
    with pytest.raises(partls.PartlsError) as e:
        call(np.ones((big, M)), np.ones((big, K)), np.zeros(big))
    assert str(L.PREDICT_MANY_MAX_B) in str(e.value)                                   # the message names the cap
    st = np.zeros((N, 2), order="F")
    refused(L.ERR_BAD_ARG, a, b, t, ranks=[0, 6], stats=st)                             # a rank outside [0, B)
    refused(L.ERR_BAD_ARG, a, b, t, ranks=[-1, 2], stats=st)
    bn = b.copy()
    bn[3, 1] = np.nan
    refused(L.ERR_BAD_ARG, a, bn, t)                                                    # a NaN in beta
    ai, ti = a.copy(), t.copy()
    ai[5, 0], ti[2] = np.inf, -np.inf
    refused(L.ERR_BAD_ARG, ai, b, t)
    refused(L.ERR_BAD_ARG, a, b, ti)
    refused(L.ERR_BAD_ARG, a, b, t, yhat=None)                                          # no output wanted
    refused(L.ERR_BAD_ARG, a, b, t, ranks=[0, 1])                                       # ranks without stats
    refused(L.ERR_BAD_ARG, a[:0], b[:0], t[:0])                                         # B = 0
    assert np.all(yh == 0.0)                                                            # nothing was written
    call(a, b, t)
    assert np.array_equal(yh[:, 0], want)
    ctx.close()


def test_bootstrap_band_end_to_end(partls):
    """lo and hi equal np.percentile(yhat, [5, 95], axis=1) to the last bit: level 0.9 asks for exactly the 5th and 95th percentile
    (50 - 50 level), the device returns the exact order statistics either side of numpy's virtual index, and the host interpolates
    with numpy's own _lerp formula, its switch at gamma = 0.5 included — the same operations on the same numbers."""
    g = load_golden("synth_a")
    X, y, P = g["X"], g["y"], g["P"]
    res = partls.bootstrap(partls.Opt, X, y, P, B=40, rng=3)
    ok = np.flatnonzero(res.ok)
    assert len(ok) >= 2
    out = res.predict(X, level=0.9, return_all=True)
    Y = out["yhat"]
    assert Y.shape == (X.shape[0], len(ok))
    for j, q in enumerate(ok):
        assert np.array_equal(Y[:, j], partls.predict(res.models[q], X)), q
    lo, hi = np.percentile(Y, [5, 95], axis=1)
    assert np.array_equal(out["lo"], lo) and np.array_equal(out["hi"], hi)
    assert np.array_equal(out["mean"], _index_ordered_mean(Y))
    band = res.predict(X, level=0.9)
    assert set(band) == {"mean", "lo", "hi"}
    for k in band:
        assert np.array_equal(band[k], out[k]), k
    assert np.array_equal(partls.predict_many([res.models[q] for q in ok], X), Y)
