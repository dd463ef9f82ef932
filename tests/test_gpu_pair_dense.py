"""The pair walk's DENSE pricing (csrc/sweep_blk.hip, PAIR: pair_solve and the rows behind it): a twin is priced from the
whole 16 x 16 block of the pair column as the tableau holds it — the solve's steps run over the column's 16 variables and skip those
outside the violator set C by a bit test, rows and columns outside C are carried along with whatever they hold, every row adds 16
terms of which those outside C have the coefficient 0.  What can go wrong in that form and not in a compacted one: an entry outside C
that reaches one inside, a step taken or skipped for the wrong column, a basis flag read at the wrong bit, a coefficient that is not
exactly 0, the guard tested on a column outside C.

Shapes: the 512-thread kernel at T = 11 (n = 161: the last tile column holds one variable, n = 176: full) and T = 16 (n = 241: one
variable in the last column, n = 256); faithful intercept (n = D + 1, all_opt exists), N = 3 D rows, K = 5 groups (64 patterns),
PARTLS_BIT_ORDER=identity with the decoupled group 0 on bit 0, PARTLS_PAIR=1, PARTLS_CHAIN_LEN = 16 and 7 — contexts, knobs and
tolerances as tests/test_gpu_pair.py (context, TOL_OBJ, TOL_WALKS) and tests/test_gpu_pair_static.py (run, ATOL_MODEL).

  gaps       group 0 of 12 features of which 6 carry no signal.  Without signal alone C has no gaps: a live variable of the flipped group
             whose reduced cost is above the tolerance violates under one of the two signs whatever its size, so C is the whole group
             in every twin (the emulation: |C| = 12 throughout and, the quiet half's coefficients changing sign with every flip, no
             priced twin at all).  So the quiet half also belongs to a second group each: where the two groups disagree such a
             variable's sign is 0, it is non-basic and stays out of C — C then has columns missing between its lowest and its highest
             and changes from twin to twin (|C| = 7 .. 10);
  full       16 live features: columns 0 and 15 of the block are in C;
  one        1 live feature: |C| = 1, fifteen columns of the block belong to other groups;
  nine       9 live features, the column filled up by seven variables of other groups;
  collinear  12 live features of which the second is the first plus EPS times a column of its own: where both enter, the second's pivot
             is ~EPS^2 = 6e-5 < 1e-4, the guard fires and the twin goes to the ordinary rounds, which accept the pivot.  With both
             in C in every twin no twin is priced (the emulation: every one guarded or left with violators), so the near-copy
             belongs to a second group as well and is out of C where the two disagree: 14 of 32 twins are priced, 16 guarded.

Every case, on both chain lengths: all_opt against the oracle at TOL_OBJ, the winner and the finish (alpha, beta, t, objective) against
the oracle's, unconverged == 0, pivots() strictly below the PARTLS_PAIR=0 walk's on the same chains and EQUAL to the count of the CPU emulation of the
walk, EMUL_PIVOTS (tools/pair_emul.py dense, which prices by the same dense form and checks it bit for bit against the compacted one).

The seeds were chosen on the CPU with `python tools/pair_emul.py dense` (which walks these very problems and fails unless each has the
twins it is there for): SEED below; the emulation reports at least one priced twin with a gap in its mask for `gaps` and at least one
guarded twin for `collinear` on either chain length."""
import numpy as np
import pytest

from test_gpu_pair import FAITHFUL, TOL_OBJ, TOL_WALKS
from test_gpu_pair_static import ATOL_MODEL, run

pytestmark = pytest.mark.gpu

K = 5
COUPLING = 0.01
EPS = 8e-3
CHAINS = ("16", "7")
LIVE = {"gaps": 12, "full": 16, "one": 1, "nine": 9, "collinear": 12}
CASES = (("gaps", 161), ("gaps", 256), ("full", 176), ("one", 241), ("nine", 256), ("collinear", 176))
SEED = {("gaps", 161): 2, ("gaps", 256): 2, ("full", 176): 0, ("one", 241): 0, ("nine", 256): 0, ("collinear", 176): 0}
# pivots of the emulated walk, (kind, n, chain length): python tools/pair_emul.py dense
EMUL_PIVOTS = {
    ("gaps", 161, 16): 2377, ("gaps", 161, 7): 2888, ("gaps", 256, 16): 3478, ("gaps", 256, 7): 4402,
    ("full", 176, 16): 2292, ("full", 176, 7): 2892, ("one", 241, 16): 3540, ("one", 241, 7): 4297,
    ("nine", 256, 16): 3645, ("nine", 256, 7): 4565, ("collinear", 176, 16): 2392, ("collinear", 176, 7): 2984,
}


def make(kind, n):
    """(X, y, P): K groups, group 0 = LIVE[kind] features decoupled from the others (tests/test_gpu_pair.py: most twins are then priced)"""
    D, live = n - 1, LIVE[kind]
    N = 3 * D
    rng = np.random.default_rng(20264000 + 1000 * n + 10 * live + SEED[kind, n])
    X = rng.standard_normal((N, D))
    others = np.arange(1, K)
    grp = others[rng.integers(0, K - 1, D)]
    grp[rng.choice(D, K - 1, replace=False)] = others                     # each of those groups has a feature
    gs = np.sort(rng.choice(np.flatnonzero(np.bincount(grp, minlength=K)[grp] > 1), live, replace=False))
    grp[gs] = 0
    assert all((grp == k).any() for k in range(K))
    w = rng.standard_normal(D) * (rng.random(D) < 0.6)
    w[gs] = rng.choice([-1.0, 1.0], live) * (0.5 + rng.random(live))
    noise = rng.standard_normal(N)
    if kind == "gaps":
        quiet = gs[rng.permutation(live)[:live // 2]]
        w[quiet] = 0.0                                                    # half of the group: no signal
    oth = np.flatnonzero(grp != 0)
    Q, _ = np.linalg.qr(np.column_stack([X[:, oth], np.ones(N)]))
    X[:, gs] += (COUPLING - 1.0) * (Q @ (Q.T @ X[:, gs]))
    if kind == "collinear":
        X[:, gs[1]] = X[:, gs[0]] + EPS * X[:, gs[1]]
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    if kind == "gaps":
        P[quiet, 1 + rng.integers(0, K - 1, len(quiet))] = 1              # ... and a second group each (see the module docstring)
    if kind == "collinear":
        P[gs[1], 1 + rng.integers(0, K - 1)] = 1                          # the near-copy too
    y = X @ w + 0.4 + 0.3 * noise
    return np.asfortranarray(X), y, np.asfortranarray(P)


@pytest.mark.parametrize("kind,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_dense_pricing(partls, oracle, monkeypatch, kind, n):
    X, y, P = make(kind, n)
    ref = oracle.fit_opt(X, y, P, return_all=True)
    objs = ref["all_opt"]
    for chain in CHAINS:
        off = run(partls, monkeypatch, X, y, P, FAITHFUL, pair=False, chain=chain, g=0)
        got = run(partls, monkeypatch, X, y, P, FAITHFUL, pair=True, chain=chain, g=0)
        err = np.abs(got["all"] - objs) / np.maximum(1.0, np.abs(objs))
        want = EMUL_PIVOTS[kind, n, int(chain)]
        print("[pair dense] %s n=%d chain %s: %d pivots (emulation %d; PARTLS_PAIR=0: %d); max error of all_opt %.3g; winner %d "
              "(oracle %d), objective %.17g (%.17g)" % (kind, n, chain, got["pivots"], want, off["pivots"], err.max(), got["pat"],
                                                        ref["best_index"], got["obj"], ref["opt"]))
        assert np.all(np.abs(got["all"] - objs) <= TOL_OBJ * np.maximum(1.0, np.abs(objs))), err.max()
        assert got["pat"] == ref["best_index"] == off["pat"]
        assert got["obj"] == got["all"][got["pat"]]
        assert abs(got["obj"] - off["obj"]) <= TOL_WALKS * max(1.0, off["obj"])
        fin = got["fin"]
        assert fin["index"] == ref["best_index"]
        assert abs(fin["opt"] - ref["opt"]) <= TOL_OBJ * max(1.0, ref["opt"])
        np.testing.assert_allclose(fin["alpha"], ref["alpha"], atol=ATOL_MODEL)
        np.testing.assert_allclose(fin["beta"], ref["beta"], atol=ATOL_MODEL)
        np.testing.assert_allclose(fin["t"], ref["t"], atol=ATOL_MODEL)
        assert got["pivots"] < off["pivots"], (got["pivots"], off["pivots"])          # twins were priced
        assert got["pivots"] == want, (got["pivots"], want)
