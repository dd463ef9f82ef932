"""GPU tests of partls_contributions: every entry equals a numpy restatement of its fma chain bit for bit on data
whose products are exact, and lies within the chain's error bound of a longdouble reference on real data; the row sums plus t are the
prediction; slab b of a many-model call is the single-model call, a float32 X equals its widened copy, device pointers with padded
leading dimensions leave the padding alone; the order statistics and the mean over the models are exact; the sums over the rows are
exact on integer data, within the summation bound on real data and the same bits whatever the byte budget, the other outputs wanted
or where X lives; bad calls are refused and leave the context usable; and a bootstrap's band is np.percentile of its replicates'
contributions."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _chunk(partls):
    return partls.lowlevel.CONTRIB_CHUNK


def _partitions(M):
    """[(name, P)]: one group; one group per feature; uneven groups; and, in one partition, an empty group (2), a feature in two groups
    (feature 0: groups 0 and 3) and a feature in no group (the last one)"""
    out = [("K=1", np.ones((M, 1), dtype=np.int64)), ("K=M", np.eye(M, dtype=np.int64))]
    if M >= 3:
        Pu = np.zeros((M, 2), dtype=np.int64)
        Pu[:M - 1, 0] = 1                                        # M - 1 features against one
        Pu[M - 1, 1] = 1
        out.append(("uneven", Pu))
    Pm = np.zeros((M, 4), dtype=np.int64)
    Pm[0, 0] = Pm[0, 3] = 1
    if M >= 3:
        Pm[1, 1] = 1
        Pm[2:M - 1, 0] = 1
    out.append(("mixed", Pm))
    return out


def _exact_inputs(rng, N, M, K, B):
    """X, alpha, beta whose products are exact in float64 — X has 21 significant bits, alpha and beta 10 each, so w = alpha beta has 20
    and x w 41 — while the sums are not: the columns of X and the models differ in scale by up to 2^20.  On such data fma(x, w, c) is
    the rounded x * w + c of plain numpy, so the chain can be restated without an fma.  (test_gpu_predict_many.py: _exact_inputs)"""
    X = rng.integers(-2 ** 20, 2 ** 20, size=(N, M)).astype(np.float64) * 2.0 ** rng.integers(-10, 11, size=(1, M))
    a = rng.integers(1, 1024, size=(B, M)).astype(np.float64) / 64.0
    b = rng.integers(-512, 512, size=(B, K)).astype(np.float64) * 2.0 ** rng.integers(-10, 1, size=(B, 1))
    return np.asfortranarray(X), a, b


def _chains(X, P, a, b, dtype=np.float64):
    """the contract, restated: c[i, k, b] = the chain over the features of group k in ascending m, from 0.0, of x w + c with
    w = (P[m,k] alpha_m) beta_k formed in float64; dtype=np.longdouble runs the chain (not the weights) in extended precision.
    Also returns the sum of |x w| per entry."""
    N, M = X.shape
    B, K = b.shape
    out, mag = np.zeros((N, K, B), dtype=dtype), np.zeros((N, K, B), dtype=dtype)
    for k in range(K):
        for m in np.flatnonzero(P[:, k]):
            w = (float(P[m, k]) * a[:, m]) * b[:, k]                                  # [B]
            term = X[:, m].astype(dtype)[:, None] * w.astype(dtype)[None, :]
            out[:, k, :] = term + out[:, k, :]
            mag[:, k, :] += np.abs(term)
    return out, mag


@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_entries_equal_the_chain_restated_in_numpy_bitwise(partls, N):
    """N: one lane, a block less one row, a block and one row, four blocks; B: one model, a chunk less one, a chunk, a chunk and one,
    two chunks and three; every partition of _partitions; float32 where it holds the data"""
    C = _chunk(partls)
    rng = np.random.default_rng(N)
    ctx = partls.default_context()
    rounds = 0
    for M in (1, 3, 5, 17):
        for name, P in _partitions(M):
            for B in (1, C - 1, C, C + 1, 2 * C + 3):
                X, a, b = _exact_inputs(rng, N, M, P.shape[1], B)
                ref, _ = _chains(X, P, a, b)
                got = ctx.contributions(X, P, a, b)["contrib"]
                assert got.shape == ref.shape and got.dtype == np.float64
                assert np.array_equal(got, ref), (M, name, B)
                assert not np.signbit(got[:, P.sum(0) == 0, :]).any()              # an empty group: +0.0
                if B == C + 1:
                    assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
                    assert np.array_equal(ctx.contributions(X.astype(np.float32), P, a, b)["contrib"], ref), (M, name)
                if M == 17 and name in ("K=1", "uneven") and N > 1:                   # the same chains in descending m
                    rounds += not np.array_equal(_chains(X[:, ::-1], P[::-1], a[:, ::-1], b)[0], ref)
    assert N == 1 or rounds > 0                                                       # the data do round: another order gives other bits


def test_real_data_within_the_chain_bound_of_longdouble(partls):
    """|c - exact| <= (n_k + 1) 2^-53 sum |x w|: n_k fma roundings (the standard bound of a chain of n_k terms, gamma_n ~ n u) and one
    more for the longdouble reference's own error; an empty group is exactly +0.0"""
    C = _chunk(partls)
    rng = np.random.default_rng(21)
    ctx = partls.default_context()
    for N, M, B in ((257, 5, C + 1), (1000, 17, 3), (255, 3, 2 * C + 3)):
        for name, P in _partitions(M):
            K = P.shape[1]
            X = np.asfortranarray(rng.normal(size=(N, M)) * 10.0 ** rng.integers(-3, 4, size=(1, M)))
            a, b = rng.normal(size=(B, M)), rng.normal(size=(B, K))
            got = ctx.contributions(X, P, a, b)["contrib"]
            ref, mag = _chains(X, P, a, b, np.longdouble)
            nk = P.sum(0).astype(np.float64)[None, :, None]
            err = np.abs(got.astype(np.longdouble) - ref)
            print("real data", N, M, B, name, "max err / bound", float(np.max(err / np.maximum((nk + 1) * U * mag, np.finfo(float).tiny))))
            assert np.all(err <= (nk + 1) * U * mag), (N, M, B, name)
            empty = P.sum(0) == 0
            assert np.all(got[:, empty, :] == 0.0) and not np.signbit(got[:, empty, :]).any()


def test_row_sums_plus_t_are_the_prediction(partls):
    rng = np.random.default_rng(22)
    ctx = partls.default_context()
    # every sum exact: small-integer X, dyadic alpha, beta, t — bit for bit, the feature in two groups included
    for N, M in ((257, 5), (1000, 17), (1, 1), (255, 3)):
        for name, P in _partitions(M):
            K = P.shape[1]
            X = np.asfortranarray(rng.integers(-64, 65, size=(N, M)).astype(np.float64))
            a = rng.integers(1, 33, size=M) / 16.0
            b = rng.integers(-32, 33, size=K) / 8.0
            t = float(rng.integers(-100, 101)) / 4.0
            c = partls.contributions(partls.PartLSFitResult(a, b, t, P), X)
            assert c.shape == (N, K)
            assert np.array_equal(c.sum(1) + t, ctx.predict(X, P, a, b, t)), (N, M, name)
    # real data, a partition: both sides sum the same M products and t, each in its own order, and a summation errs by at most (the
    # roundings a term passes through) u (sum |x w| + |t|).  Here a term passes through its group's ceil(M / K) fmas and the K adds of
    # sum(1) + t; in predict through its chain's ceil(M / 4) fmas (chain 0 also takes the M mod 4 last columns) and the 3 adds of
    # ((a0 + a1) + (a2 + a3)) + t: 5 + 5 of M + K + 2 = 10 at M = 5, K = 3, and 9 + 8 of 23 at M = 17, K = 4
    for N, M, K in ((257, 5, 3), (1000, 17, 4)):
        P = np.zeros((M, K), dtype=np.int64)
        P[np.arange(M), np.arange(M) % K] = 1
        X = np.asfortranarray(rng.normal(size=(N, M)))
        a, b, t = rng.normal(size=M), rng.normal(size=K), float(rng.normal())
        c = partls.contributions(partls.PartLSFitResult(a, b, t, P), X)
        w = a * (P @ b)
        bound = (M + K + 2) * U * (np.abs(X) @ np.abs(w) + abs(t))
        diff = np.abs((c.sum(1) + t) - ctx.predict(X, P, a, b, t))
        print("against predict", N, M, K, "max diff / bound", float(np.max(diff / bound)))
        assert np.all(diff <= bound)


def test_slabs_storage_forms_and_device_pointers(partls):
    import torch
    C = _chunk(partls)
    rng = np.random.default_rng(23)
    ctx = partls.default_context()
    N, M, B = 257, 5, 2 * C + 3
    P = _partitions(M)[-1][1]
    K = P.shape[1]
    X32 = rng.normal(size=(N, M)).astype(np.float32)
    X = np.asfortranarray(X32.astype(np.float64))
    a, b = rng.normal(size=(B, M)), rng.normal(size=(B, K))
    ranks = [0, 3, B - 1]
    want = ctx.contributions(X, P, a, b, ranks=ranks, want_mean=True, want_sums=True)
    many = partls.contributions_many((a, b, None, P), X)
    assert np.array_equal(many, want["contrib"])
    for j in (0, 1, C - 1, C, B - 1):                                                  # slab b = the single-model call
        assert np.array_equal(many[:, :, j], partls.contributions(partls.PartLSFitResult(a[j], b[j], 0.5, P), X)), j
        one = ctx.contributions(X, P, a[j:j + 1], b[j:j + 1], want_contrib=False, want_sums=True)["sums"]
        assert np.array_equal(one[:, :, 0], want["sums"][:, :, j]), j
    r32 = ctx.contributions(X32, P, a, b, ranks=ranks, want_mean=True, want_sums=True)  # float32 = its widened copy
    for k in ("contrib", "stats", "mean", "sums"):
        assert np.array_equal(r32[k], want[k]), k
    for dtype, ldX, ldC in ((np.float64, 300, 290), (np.float32, 300, 290), (np.float64, N, N)):
        Xp = np.full((M, ldX), np.nan, dtype=dtype)               # M x ldX row-major == N x M column-major with leading dimension ldX
        Xp[:, :N] = X32.T
        dX = torch.from_numpy(Xp).cuda()
        dC = torch.full((B * K, ldC), -7.5, dtype=torch.float64, device="cuda")
        dS = torch.full((len(ranks) * K, N), -7.5, dtype=torch.float64, device="cuda")
        dM = torch.full((K, N), -7.5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sums = ctx.contributions_device(dX.data_ptr(), N, M, ldX, P, a, b, dcontrib_ptr=dC.data_ptr(), ldC=ldC, ranks=ranks,
                                        dstats_ptr=dS.data_ptr(), dmean_ptr=dM.data_ptr(), want_sums=True, dtype=dtype)
        Cd = dC.cpu().numpy()
        assert np.array_equal(Cd[:, :N].reshape(B, K, N).transpose(2, 1, 0), want["contrib"])
        assert np.all(Cd[:, N:] == -7.5)                          # the padding rows are not written
        assert np.array_equal(dS.cpu().numpy().reshape(len(ranks), K, N).transpose(2, 1, 0), want["stats"])
        assert np.array_equal(dM.cpu().numpy().T, want["mean"]) and np.array_equal(sums, want["sums"])
        # statistics only: no contrib on the device either
        dS.fill_(-7.5)
        dM.fill_(-7.5)
        torch.cuda.synchronize()
        sums = ctx.contributions_device(dX.data_ptr(), N, M, ldX, P, a, b, ranks=ranks, dstats_ptr=dS.data_ptr(), dmean_ptr=dM.data_ptr(),
                                        want_sums=True, dtype=dtype)
        assert np.array_equal(dS.cpu().numpy().reshape(len(ranks), K, N).transpose(2, 1, 0), want["stats"])
        assert np.array_equal(dM.cpu().numpy().T, want["mean"]) and np.array_equal(sums, want["sums"])


def _index_ordered_mean(cube):
    return np.array([[sum(cell) / len(cell) for cell in row] for row in cube.tolist()])


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 100])
def test_every_rank_and_the_mean_are_exact(partls, B):
    """B either side of a power of two (the sort pads to one); ties: models 1 and B - 1 duplicate model 0, the all-zero rows of X
    contribute 0 under every model, and so does the empty group; N K = 1200 (row, group) pairs: more than one workgroup sorts"""
    _ranks_and_mean(partls, B, 300, _partitions(5)[-1][1])


@pytest.mark.parametrize("B", [257, 1025])
def test_group_shapes_of_the_row_sort_with_a_ragged_last_group(partls, B):
    """the (row, group) pairs of a call are the rows of the sort: R = 8 of them per workgroup at B = 257 (n = 512) and 2 at B = 1025
    (n = 2048).  One group per feature, K = 5, and N = 37: N K = 185 pairs, the last workgroup holds one"""
    N, P = 37, _partitions(5)[1][1]
    assert P.shape[1] == 5 and (N * P.shape[1]) % 8 == 1 and (N * P.shape[1]) % 2 == 1
    _ranks_and_mean(partls, B, N, P)


def _ranks_and_mean(partls, B, N, P):
    rng = np.random.default_rng(B)
    M, K = P.shape
    X = np.asfortranarray(rng.normal(size=(N, M)))
    X[::7] = 0.0
    a, b = rng.normal(size=(B, M)), rng.normal(size=(B, K))
    a[B - 1], b[B - 1] = a[0], b[0]
    if B > 2:
        a[1], b[1] = a[0], b[0]
    r = partls.default_context().contributions(X, P, a, b, ranks=np.arange(B), want_mean=True)
    cube = r["contrib"]
    assert np.all(cube[::7] == 0.0) and np.array_equal(cube[:, :, 0], cube[:, :, B - 1])
    assert np.array_equal(r["stats"], np.sort(cube, axis=2))
    assert np.array_equal(r["mean"], _index_ordered_mean(cube))
    pick = [B - 1, 0, B // 2, 0]                                                       # ranks in any order, repeated
    r2 = partls.default_context().contributions(X, P, a, b, ranks=pick, want_contrib=False)
    assert r2["contrib"] is None and r2["mean"] is None and np.array_equal(r2["stats"], np.sort(cube, axis=2)[:, :, pick])


def test_sums_are_exact_on_integers_and_within_the_summation_bound(partls):
    rng = np.random.default_rng(24)
    ctx = partls.default_context()
    C = _chunk(partls)
    for N, M, B in ((1, 3, 1), (255, 5, C + 1), (257, 17, 2), (1000, 5, 3)):
        P = _partitions(M)[-1][1]
        K = P.shape[1]
        # integers: c, |c| and c^2 and their sums over the rows are integers far below 2^53 — every order of summation is exact
        X = np.asfortranarray(rng.integers(-8, 9, size=(N, M)).astype(np.float64))
        a, b = rng.integers(1, 5, size=(B, M)).astype(np.float64), rng.integers(-4, 5, size=(B, K)).astype(np.float64)
        r = ctx.contributions(X, P, a, b, want_sums=True)
        ci = r["contrib"].astype(np.int64)
        assert np.array_equal(ci, r["contrib"])
        assert np.array_equal(r["sums"], np.stack([ci.sum(0), np.abs(ci).sum(0), (ci * ci).sum(0)]).astype(np.float64)), (N, M, B)
        # real data: any order of summing N terms is within (N - 1) u sum |term|; c^2 is rounded once before it is summed, and the
        # longdouble reference has an error of its own: (N + 1) u sum |term|
        X = np.asfortranarray(rng.normal(size=(N, M)))
        a, b = rng.normal(size=(B, M)), rng.normal(size=(B, K))
        r = ctx.contributions(X, P, a, b, want_sums=True)
        cl = r["contrib"].astype(np.longdouble)
        for s, term in enumerate((cl, np.abs(cl), cl * cl)):
            err = np.abs(r["sums"][s].astype(np.longdouble) - term.sum(0))
            bound = (N + 1) * U * np.abs(term).sum(0)
            print("sums", N, M, B, s, "max err / bound", float(np.max(err / np.maximum(bound, np.finfo(float).tiny))))
            assert np.all(err <= bound), (N, M, B, s)


def test_sums_do_not_depend_on_the_budget_the_outputs_or_where_X_lives(partls, monkeypatch):
    """N = 2049 under a budget of 768 rows: chunks of 768, 768 and 513 rows, the last block of one row"""
    import torch
    rng = np.random.default_rng(25)
    N, M, B = 2049, 5, 5
    P = _partitions(M)[-1][1]
    K = P.shape[1]
    X = np.asfortranarray(rng.normal(size=(N, M)))
    a, b = rng.normal(size=(B, M)), rng.normal(size=(B, K))
    ranks = [0, 2, B - 1]
    ctx = partls.default_context()
    want = ctx.contributions(X, P, a, b, ranks=ranks, want_mean=True, want_sums=True)
    assert np.array_equal(ctx.contributions(X, P, a, b, want_contrib=False, want_sums=True)["sums"], want["sums"])        # sums alone, again
    cl = want["contrib"].astype(np.longdouble)
    assert np.all(np.abs(want["sums"][0] - cl.sum(0)) <= (N + 1) * U * np.abs(cl).sum(0))
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    torch.cuda.synchronize()
    assert np.array_equal(ctx.contributions_device(dX.data_ptr(), N, M, N, P, a, b, want_sums=True), want["sums"])           # device X
    rows = 768
    monkeypatch.setenv("PARTLS_CONTRIB_BYTES", str(8 * K * B * rows))
    small = partls.Context(0)                                                          # the budget is read when a context is created
    try:
        assert -(-N // rows) >= 3
        got = small.contributions(X, P, a, b, ranks=ranks, want_mean=True, want_sums=True)
        for k in ("contrib", "stats", "mean", "sums"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(small.contributions(X, P, a, b, want_contrib=False, want_sums=True)["sums"], want["sums"])
        # device X under the small budget: the caller's contrib is the intermediate of every chunk
        dC = torch.full((B * K, N), -7.5, dtype=torch.float64, device="cuda")
        dS = torch.full((len(ranks) * K, N), -7.5, dtype=torch.float64, device="cuda")
        dM = torch.full((K, N), -7.5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sums = small.contributions_device(dX.data_ptr(), N, M, N, P, a, b, dcontrib_ptr=dC.data_ptr(), ldC=N, ranks=ranks,
                                          dstats_ptr=dS.data_ptr(), dmean_ptr=dM.data_ptr(), want_sums=True)
        assert np.array_equal(sums, want["sums"])
        assert np.array_equal(dC.cpu().numpy().reshape(B, K, N).transpose(2, 1, 0), want["contrib"])
        assert np.array_equal(dS.cpu().numpy().reshape(len(ranks), K, N).transpose(2, 1, 0), want["stats"])
        assert np.array_equal(dM.cpu().numpy().T, want["mean"])
    finally:
        small.close()


def test_bad_calls_are_refused_and_the_context_still_answers(partls):
    L = partls.lowlevel
    rng = np.random.default_rng(26)
    N, M = 40, 5
    P = _partitions(M)[-1][1]
    K = P.shape[1]
    X = np.asfortranarray(rng.normal(size=(N, M)))
    a, b = rng.normal(size=(6, M)), rng.normal(size=(6, K))
    ctx = partls.Context(0)
    want = ctx.contributions(X, P, a, b)["contrib"]
    Pf = np.asfortranarray(P, dtype=np.int64)
    out = np.zeros((N, K, L.PREDICT_MANY_MAX_B + 1), order="F")

    def call(a, b, contrib=out, ldC=N, ranks=None, stats=None, P=Pf):
        """the entry itself, past the binding's own checks"""
        a, b = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, b))
        r = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.int64)
        ctx._contributions(X.ctypes.data, 0, False, N, M, N, P, a, b, None if contrib is None else contrib.ctypes.data, ldC, r,
                           None if stats is None else stats.ctypes.data, None, None)

    def refused(status, *args, **kw):
        with pytest.raises(partls.PartlsError) as e:
            call(*args, **kw)
        assert e.value.status == status, e.value
        assert np.array_equal(ctx.contributions(X, P, a, b)["contrib"], want)

    an = a.copy()
    an[3, 1] = np.nan
    refused(L.ERR_BAD_ARG, an, b)                                                       # a NaN in alpha
    bi = b.copy()
    bi[5, 0] = np.inf
    refused(L.ERR_BAD_ARG, a, bi)
    st = np.zeros((N, K, 2), order="F")
    refused(L.ERR_BAD_ARG, a, b, ranks=[0, 6], stats=st)                                # a rank >= B
    big = L.PREDICT_MANY_MAX_B + 1
    refused(L.ERR_UNSUPPORTED, np.ones((big, M)), np.ones((big, K)))                    # B = 4097
    refused(L.ERR_BAD_ARG, a, b, contrib=None)                                          # no output wanted
    refused(L.ERR_BAD_ARG, a, b, ldC=N - 1)
    P2 = Pf.copy()
    P2[1, 1] = 2
    refused(L.ERR_BAD_PARTITION, a, b, P=P2)
    assert np.all(out == 0.0)                                                           # nothing was written
    call(a, b)
    assert np.array_equal(out[:, :, :6], want)
    ctx.close()


def test_bootstrap_band_and_group_importance_end_to_end(partls):
    """lo and hi equal np.percentile(all, [5, 95], axis=2) to the last bit (exact order statistics from the device, numpy's own
    interpolation on the host); group_importance's mean_abs comes from the device's sums: within (N + 1) u of numpy's mean of |c|"""
    g = load_golden("synth_a")
    X, y, P = g["X"], g["y"], g["P"]
    N = X.shape[0]
    res = partls.bootstrap(partls.Opt, X, y, P, B=20, rng=3)
    ok = np.flatnonzero(res.ok)
    assert len(ok) >= 2
    out = res.contributions(X, level=0.9, return_all=True)
    cube = out["all"]
    assert cube.shape == (N, P.shape[1], len(ok))
    for j, q in enumerate(ok):
        assert np.array_equal(cube[:, :, j], partls.contributions(res.models[q], X)), q
    lo, hi = np.percentile(cube, [5, 95], axis=2)
    assert np.array_equal(out["lo"], lo) and np.array_equal(out["hi"], hi)
    assert np.array_equal(out["mean"], _index_ordered_mean(cube))
    band = res.contributions(X, level=0.9)
    assert set(band) == {"mean", "lo", "hi"}
    for k in band:
        assert np.array_equal(band[k], out[k]), k
    rep = partls.group_importance(res, X)
    ref = np.abs(cube).mean(0).T
    assert rep.mean_abs.shape == ref.shape == (len(ok), P.shape[1])
    print("group_importance max rel err / bound", float(np.max(np.abs(rep.mean_abs - ref) / ((N + 1) * U * ref))))
    assert np.all(np.abs(rep.mean_abs - ref) <= (N + 1) * U * ref)
    assert np.allclose(rep.share.sum(1), 1.0, rtol=1e-14, atol=0)
    yhat = partls.predict(res.models[ok[0]], X)
    assert np.allclose(cube[:, :, 0].sum(1) + res.models[ok[0]].t, yhat, rtol=0, atol=1e-12 * (1 + np.abs(yhat).max()))


@pytest.mark.parametrize("N", [257, 1000])
def test_sums_past_1024_columns(partls, N):
    """contrib_sums_kernel walks the columns blockIdx.y, blockIdx.y + gridDim.y, ... with gridDim.y = min(K B, 1024) and reuses the LDS
    tree of its block sum from one column to the next.  K = 4 and B = 257 are 1028 columns: the workgroups of the columns 0 .. 3 make
    a second trip, to the columns 1024 .. 1027 of model 256.  Integer data: all three sums exact in any order, equality.  Real data:
    within (N + 1) u sum |term| (test_sums_are_exact_on_integers_and_within_the_summation_bound), and the same bits as the B
    single-model calls, in which every column is the first trip of its workgroup"""
    rng = np.random.default_rng(27 + N)
    ctx = partls.default_context()
    M, B = 5, 257
    P = _partitions(M)[-1][1]
    K = P.shape[1]
    assert K == 4 and K * B == 1028
    X = np.asfortranarray(rng.integers(-8, 9, size=(N, M)).astype(np.float64))
    a, b = rng.integers(1, 5, size=(B, M)).astype(np.float64), rng.integers(-4, 5, size=(B, K)).astype(np.float64)
    b[256] = [1.0, -2.0, 3.0, -4.0]                                                    # the model of the second trip: no zero sums
    r = ctx.contributions(X, P, a, b, want_sums=True)
    ci = r["contrib"].astype(np.int64)
    assert np.array_equal(ci, r["contrib"]) and np.array_equal(ci, _chains(X, P, a, b)[0])
    assert np.array_equal(r["sums"], np.stack([ci.sum(0), np.abs(ci).sum(0), (ci * ci).sum(0)]).astype(np.float64))
    assert np.all(r["sums"][1, P.sum(0) > 0, 256] > 0.0)
    X = np.asfortranarray(rng.normal(size=(N, M)))
    a, b = rng.normal(size=(B, M)), rng.normal(size=(B, K))
    r = ctx.contributions(X, P, a, b, want_sums=True)
    cl = r["contrib"].astype(np.longdouble)
    for s, term in enumerate((cl, np.abs(cl), cl * cl)):
        err = np.abs(r["sums"][s].astype(np.longdouble) - term.sum(0))
        bound = (N + 1) * U * np.abs(term).sum(0)
        print("sums past 1024 columns", N, s, "max err / bound", float(np.max(err / np.maximum(bound, np.finfo(float).tiny))))
        assert np.all(err <= bound), (N, s)
    assert np.array_equal(ctx.contributions(X, P, a, b, want_contrib=False, want_sums=True)["sums"], r["sums"])
    for j in range(B):
        one = ctx.contributions(X, P, a[j:j + 1], b[j:j + 1], want_contrib=False, want_sums=True)["sums"]
        assert np.array_equal(one[:, :, 0], r["sums"][:, :, j]), j


def test_a_workgroup_that_walks_several_groups(partls):
    """contrib_kernel deals the groups k = blockIdx.z, blockIdx.z + gridDim.z, ... to the workgroups of a (row block, model chunk), and
    gridDim.z = ceil(32 ncu / waves) clamped to [1, K] with waves = 4 x row blocks x model chunks (contrib.hip: contrib_group_split).
    6 ncu + 1 row blocks of one model (393 217 rows on 256 compute units, the last block of one row) give gridDim.z = 2 under K = 4:
    each workgroup computes two groups, one after the other.  The rule is restated here from the device's compute units, so the test
    cannot pass on another part without a partial split.  Entries: the chain restated in numpy, bit for bit; sums: exact integers"""
    import torch
    L = partls.lowlevel
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = 6 * ncu + 1
    N, M, B = 256 * blocks - 255, 5, 1
    P = _partitions(M)[-1][1]
    K = P.shape[1]
    assert (N + 255) // 256 == blocks and N % 256 == 1 and N * K * 8 <= L.PREDICT_MANY_BYTES         # one chunk of rows
    waves, target = blocks * 4 * -(-B // _chunk(partls)), ncu * 4 * 8
    z = min(max(-(-target // waves), 1), K)
    assert 1 < z < K, (ncu, z)
    rng = np.random.default_rng(28)
    ctx = partls.default_context()
    X, a, b = _exact_inputs(rng, N, M, K, B)
    ref, _ = _chains(X, P, a, b)
    got = ctx.contributions(X, P, a, b)["contrib"]
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert np.array_equal(ctx.contributions(X.astype(np.float32), P, a, b)["contrib"], ref)
    X = np.asfortranarray(rng.integers(-8, 9, size=(N, M)).astype(np.float64))
    a, b = rng.integers(1, 5, size=(B, M)).astype(np.float64), rng.integers(-4, 5, size=(B, K)).astype(np.float64)
    b[0, np.flatnonzero(b[0] == 0)] = 3.0                                              # every group with features contributes
    r = ctx.contributions(X, P, a, b, want_sums=True)
    ci = r["contrib"].astype(np.int64)
    assert np.array_equal(ci, r["contrib"]) and np.array_equal(ci, _chains(X, P, a, b)[0])
    assert np.array_equal(r["sums"], np.stack([ci.sum(0), np.abs(ci).sum(0), (ci * ci).sum(0)]).astype(np.float64))
    assert np.all(r["sums"][1, P.sum(0) > 0, 0] > 0.0)
