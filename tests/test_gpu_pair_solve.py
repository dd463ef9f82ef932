"""The pair walk's twin solve (csrc/sweep_blk.hip, pair_solve): the |C| x |C| solve of a twin's violators on one wave, its 16
steps written out, the pivot column of each step handed from the 16 lanes that hold it to all 64 through LDS, the pivot row and the
pivot column overwritten under EXEC and the guard accumulated without a branch.  What can go wrong in that form: a quarter or a
register index whose store or load takes the wrong lanes, a step that reads the exchange of the step before, a skipped step that
leaves the exchange stale for the next executed one, a basis flag or a guard taken at the wrong step, and the steps that still execute
behind a guarded pivot reaching anything that is read.

Shapes: the edges of the pair kernels, n = 161 (T = 11, the last tile column holds one variable) and n = 256 (T = 16); faithful
intercept (n = D + 1, all_opt exists), N = 3 D rows, K = 5 groups (64 patterns), PARTLS_BIT_ORDER=identity with the decoupled group 0
on bit 0, PARTLS_PAIR=1, PARTLS_CHAIN_LEN = 16 and 7 — problems, contexts, knobs and tolerances as tests/test_gpu_pair_dense.py.

  full       16 live features on bit 0, both n: |C| = 16 in every twin, so every quarter and every register index is a pivot column
             (emulation: 32 / 27 twins on chains of 16 / 7 at either n, 26 / 23 of them priced at n = 161 and 23 / 18 at n = 256);
  one, two, three   groups of 1, 2 and 3 live features (n = 161, 256, 161): masks 0x1, 0x3, 0x7 — steps 1 .. 15, 2 .. 15, 3 .. 15 are
             skipped; nearly every twin is priced;
  gaps       12 features of which the quiet half also belongs to a second group (tests/test_gpu_pair_dense.py's kind): the mask
             changes from twin to twin, with steps skipped at the start (bit 0 clear in 16 / 13 twins), in the middle (every twin)
             and at the end of the column (emulation: masks 0xb5e, 0xb7a, 0xb7b, 0xfca, 0xfeb, ...; |C| = 8 .. 11; 18 / 13 twins priced);
  mixed      9 live features: C holds basic AND non-basic variables, leaving and entering pivots in one solve with the basis flags
             mixed (emulation: every twin, 32 / 27 — as in every other kind here with |C| > 1; 27 / 23 priced);
  dup        12 features of which the sixth is an exact copy of the fifth: where both are in C the fifth enters, the copy's pivot
             is then ~1e-16 and the guard fires at a step that is NOT the first executed one — the steps behind it run on, on values
             nobody reads — and the twin goes to the ordinary rounds (emulation: 4 / 6 guarded twins, each at its 6th executed step of
             12; 23 / 18 twins priced).

Every case, on both chain lengths: every pattern's objective (all_opt) against the oracle (oracle.opt_patterns on the compressed
problem) at TOL_OBJ, unconverged == 0 and pivots() EQUAL to the count of the CPU emulation of the walk (tools/pair_emul.py's pair_sweep
with the dense pricing, on the problem after the host's relayout; for dup plus the columns it refuses, which the device counts as steps
of their blocks): EMUL_PIVOTS.  The counts, and what each kind is there for, were
computed on the CPU with that emulation; the seeds are the first for which every kind has its twins."""
import numpy as np
import pytest

from test_gpu_pair import FAITHFUL, TOL_OBJ
from test_gpu_pair_static import run

pytestmark = pytest.mark.gpu

K = 5
COUPLING = 0.01
CHAINS = ("16", "7")
LIVE = {"full": 16, "one": 1, "two": 2, "three": 3, "gaps": 12, "mixed": 9, "dup": 12}
CASES = (("full", 161), ("full", 256), ("one", 161), ("two", 256), ("three", 161), ("gaps", 161), ("mixed", 256), ("dup", 161))
SEED = {c: 4 if c[0] == "gaps" else 0 for c in CASES}
# pivots of the emulated walk, (kind, n, chain length)
EMUL_PIVOTS = {
    ("full", 161, 16): 2197, ("full", 161, 7): 2739, ("full", 256, 16): 3810, ("full", 256, 7): 4750,
    ("one", 161, 16): 2685, ("one", 161, 7): 3174, ("two", 256, 16): 3848, ("two", 256, 7): 4697,
    ("three", 161, 16): 2316, ("three", 161, 7): 2880, ("gaps", 161, 16): 2367, ("gaps", 161, 7): 2901,
    ("mixed", 256, 16): 3493, ("mixed", 256, 7): 4425, ("dup", 161, 16): 2565 + 8, ("dup", 161, 7): 3130 + 12,
}
# dup: the emulated walk's pivots + its `rejections`.  pivots() counts every step of a block the panel ran, also the step of a column it
# refused as dependent (d <= piv_eps: 1/d = 0, a no-op that leaves the variable blocked; panel_block, npiv += mx), where the emulation
# skips such a column and reports it apart.  Only dup has any: the copy's pivot of ~1e-16 in the ordinary rounds behind a guarded twin
# (8 on chains of 16, 12 on chains of 7); every other kind here walks with 0 rejections.


def make(kind, n):
    """(X, y, P): K groups, group 0 = LIVE[kind] features decoupled from the others (tests/test_gpu_pair.py: most twins are then priced)"""
    D, live = n - 1, LIVE[kind]
    N = 3 * D
    rng = np.random.default_rng(20265000 + 1000 * n + 10 * live + SEED[kind, n])
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
    if kind == "dup":
        X[:, gs[5]] = X[:, gs[4]]                                         # two features of group 0 that are copies of each other
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    if kind == "gaps":
        P[quiet, 1 + rng.integers(0, K - 1, len(quiet))] = 1              # ... and a second group each (tests/test_gpu_pair_dense.py)
    y = X @ w + 0.4 + 0.3 * noise
    return np.asfortranarray(X), y, np.asfortranarray(P)


@pytest.mark.parametrize("kind,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_pair_solve(partls, oracle, monkeypatch, kind, n):
    X, y, P = make(kind, n)
    Xo, Po = oracle.homogeneous(X, P)
    R, z = oracle.compress(Xo, y)
    objs = oracle.opt_patterns(R, z, Po, np.arange(1 << (K + 1)))
    for chain in CHAINS:
        got = run(partls, monkeypatch, X, y, P, FAITHFUL, pair=True, chain=chain, g=0)
        err = np.abs(got["all"] - objs) / np.maximum(1.0, np.abs(objs))
        want = EMUL_PIVOTS[kind, n, int(chain)]
        print("[pair solve] %s n=%d chain %s: %d pivots (emulation %d); max error of all_opt %.3g; winner %d (oracle %d)" % (
            kind, n, chain, got["pivots"], want, err.max(), got["pat"], int(np.argmin(objs))))
        assert np.all(np.abs(got["all"] - objs) <= TOL_OBJ * np.maximum(1.0, np.abs(objs))), err.max()
        assert got["pat"] == int(np.argmin(objs))
        assert got["pivots"] == want, (got["pivots"], want)
