"""Every row-tile count of leverage_kernel<XT, RPW> (diag.hip), for float64 and float32 X.

A wave of the kernel owns the 16-row tiles R = wave, wave + 8, ... of T, RPW = ceil(nt / 8) of them at nt = ceil(p / 16) tiles.  The
shapes sit on both sides of every boundary of RPW: p = 128 j and 128 j + 1, j = 1 .. 7, is nt = 8 j (every wave holds j tiles: the
largest tile count of RPW = j) and nt = 8 j + 1 (wave 0 alone holds j + 1: the smallest of RPW = j + 1).  Data, reference and bounds
are those of test_gpu_diagnostics.py, unchanged: X ~ N(0, 1) (rounded to float32, so one data set serves both element types),
M = p + 20, K = 3, the Householder-QR reference, kappa <= 50 asserted and |h - h_ref| <= 8 p kappa^2 u.  N = 4 p + 1 at a multiple of
128 (the last workgroup of 32 rows holds one row) and 4 p + 13 otherwise (17 rows: a full 16-row tile and one row).
On these data kappa of the reference lies between 2.8 and 6.0 in all 28 cases, so delta <= 3e-11, while zeroing any single 16 x 16
tile of T (computed in numpy at p = 129, 513 and 897, both cases) moves some leverage by 1.4e-4 or more: a skipped, doubled or
misplaced tile cannot pass."""
import numpy as np
import pytest

from test_gpu_diagnostics import ROWS, DeviceProblem, check_problem, make_data

pytestmark = pytest.mark.gpu

K = 3
PS = [128 * j + r for j in range(1, 8) for r in (0, 1)]
CASES = ((0.0, True), (0.5, False))                      # (eta, weighted): weights with exact zeros; a ridge on unweighted rows
EVERYTHING = ROWS + ("se_w", "se_beta", "active", "summary")


def shape(p):
    return (4 * p + 1 if p % 128 == 0 else 4 * p + 13), p + 20


def tile_data(p, weighted, seed=None):
    N, M = shape(p)
    X, y, P, w, S = make_data(N, M, K, p, 5000 + p if seed is None else seed, 0.0, weighted)
    return np.asfortranarray(X.astype(np.float32).astype(np.float64)), y, P, w, S


def float32_calls(partls, X, y, P, w, eta, model):
    """the same problem from float32 X: device-resident (padded ldX, NaN padding), and from host arrays"""
    X32 = np.asfortranarray(X.astype(np.float32))
    assert np.array_equal(X32.astype(np.float64), X)
    dev = DeviceProblem(partls, X, y, P, w, eta, dtype=np.float32).diagnostics(model)
    ctx = partls.Context(0)
    ctx.opt_prepare(X32, y, P, eta, weights=w)
    host = ctx.diagnostics(model.α, model.β, model.t)
    ctx.close()
    return dev, host


def assert_same_bits(a, others, tag):
    for other in others:
        for k in EVERYTHING:
            assert np.array_equal(a[k], other[k], equal_nan=True), (tag, k)


@pytest.mark.parametrize("p", PS)
def test_every_row_tile_count_in_both_element_types(partls, p):
    """nt = ceil(p / 16) = 8, 9, 16, 17, ..., 56, 57: RPW = 1 .. 8, each at its largest or smallest tile count.  The float64 call against
    the QR reference within the project's bound (the standard errors too where the longdouble inverse is affordable, p <= 257), and both
    float32 calls equal to it bit for bit in every output"""
    nt = (p + 15) // 16
    for eta, weighted in CASES:
        X, y, P, w, S = tile_data(p, weighted)
        print("nt %d RPW %d" % (nt, (nt + 7) // 8))
        d, model = check_problem(partls, X, y, P, w, S, eta, want_se=p <= 257)
        assert_same_bits(d, float32_calls(partls, X, y, P, w, eta, model), (p, eta, weighted))


COPIES = (0, 15, 16, 31, 32, -1)            # both 16-row tiles of a workgroup at both ends, the next workgroup, the ragged last one


@pytest.mark.parametrize("p", [129, 897])
def test_one_row_one_sum(partls, p):
    """a row's leverage is a function of its values, its weight and T alone: copies of one row of (X, y, w) planted across the tiles of
    a workgroup, in the next workgroup and in the last, ragged one get the same bits of leverage and loo, in both element types"""
    for eta, weighted in CASES:
        X, y, P, w, S = tile_data(p, weighted)
        N = X.shape[0]
        src = 100
        if weighted:
            w[src] = 1.75                                # not one of the exact zeros
        rows = [r % N for r in COPIES]
        X[rows], y[rows] = X[src], y[src]
        if weighted:
            w[rows] = w[src]
        d, model = check_problem(partls, X, y, P, w, S, eta, want_se=False)       # (asserts kappa <= 50 on the planted data)
        for out in (d,) + float32_calls(partls, X, y, P, w, eta, model):
            for k in ("leverage", "loo"):
                v = out[k][rows + [src]]
                assert v[0] != 0.0 and np.all(v.view(np.int64) == v.view(np.int64)[0]), (p, eta, k, v)


def _resupport(X, S, seed):
    """y for the support S by make_data's rule (one sign per group, |truth| in [0.5, 1.5], intercept 0.7, noise 0.3)"""
    rng = np.random.default_rng(seed)
    truth = np.zeros(X.shape[1])
    truth[S] = np.where((S % K) % 2 == 0, 1.0, -1.0) * rng.uniform(0.5, 1.5, size=len(S))
    return X @ truth + 0.7 + 0.3 * rng.normal(size=X.shape[0])


@pytest.mark.parametrize("edge", ["first and last", "without feature 0"])
def test_supports_at_the_edges_of_the_feature_range(partls, edge):
    """p = 129: the index list of the active columns encodes the ones column as -1 and pads the last tile with -2, and both load
    column 0 and discard it.  A support with feature 0 and feature M - 1; and one without feature 0, where column 0 is loaded only to
    be discarded"""
    p = 129
    for eta, weighted in CASES:
        X, y, P, w, S = tile_data(p, weighted)
        M = X.shape[1]
        inside = set(int(m) for m in S)
        outside = [m for m in range(M) if m not in inside]
        if edge == "first and last":
            want = {0, M - 1}
            spare = [m for m in S if int(m) not in want]
            S2 = sorted(want | set(int(m) for m in spare[:p - 1 - len(want)]))
        else:
            S2 = sorted((inside - {0}) | ({next(m for m in outside if m != 0)} if 0 in inside else set()))
        S2 = np.array(S2, dtype=S.dtype)
        assert len(S2) == p - 1 and ((0 in S2 and M - 1 in S2) if edge == "first and last" else 0 not in S2)
        y = _resupport(X, S2, 7000 + p)
        d, model = check_problem(partls, X, y, P, w, S2, eta)
        assert bool(d["active"][0]) == (edge == "first and last")
        assert_same_bits(d, float32_calls(partls, X, y, P, w, eta, model), (edge, eta, weighted))
