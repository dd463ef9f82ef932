"""CPU checks of the per-node BnB reference (tests/bnb_reference.py) that test_gpu_bnb_nodes.py and test_dist.py rely on: the projected
solve against brute force over every orthant of the free variables and against BnB.jl's literal [Xp Xm] split, the fixed-at-zero rule
on overlapping partitions, and nu against the pairwise formula of BnB.jl:42-57."""
import numpy as np

from bnb_reference import NodeReference, node_codes, nu_groups, nu_pairwise


def _tiny(seed, N=40, D=6, K=3, overlap=False, offset=0.0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    grp = rng.permutation(np.arange(D) % K)
    P = np.zeros((D, K), dtype=np.int64)
    P[np.arange(D), grp] = 1
    if overlap:
        P[0, (grp[0] + 1) % K] = 1
        P[1, (grp[1] + 1) % K] = 1
    y = X @ rng.standard_normal(D) + offset + 0.3 * rng.standard_normal(N)
    return X, y, P


def _every_node(Kp):
    return [(pat, free) for free in range(1 << Kp) for pat in range(1 << Kp) if not pat & free]


def test_projected_solve_matches_brute_force_over_orthants():
    """every node of tiny problems with at most 8 free variables: lb == min over every sign orthant of the free variables of NNLS"""
    for seed, kw in ((1, {}), (2, dict(overlap=True)), (3, dict(offset=50.0)), (4, dict(D=5, K=2))):
        X, y, P = _tiny(seed, **kw)
        ref = NodeReference(X, y, P, 0.5 if seed == 3 else 0.0)
        n = 0
        for pat, free in _every_node(ref.Kp):
            if (node_codes(ref.Po, pat, free) == 2).sum() > 8:
                continue
            r = ref.node(pat, free)
            assert r["certified"], (seed, pat, free)
            bf = ref.brute_force(pat, free)
            assert abs(r["lb"] - bf) <= 1e-10 * bf, (seed, pat, free, r["lb"], bf)
            n += 1
        assert n > 20


def test_projected_solve_matches_the_literal_split():
    """BnB.jl:69-92 as written (NNLS on [Xp Xm] of the regularised data) gives the same bound and the same w"""
    for seed, eta in ((5, 0.0), (6, 0.3)):
        X, y, P = _tiny(seed, N=60, D=10, K=4, overlap=True, offset=5.0)
        ref = NodeReference(X, y, P, eta)
        for pat, free in _every_node(ref.Kp)[::3]:
            r = ref.node(pat, free)
            rn, w = ref.literal_split(pat, free)
            assert r["certified"]
            assert abs(r["lb"] - rn) <= 1e-10 * rn, (seed, pat, free, r["lb"], rn)
            np.testing.assert_allclose(r["w"], w, rtol=1e-7, atol=1e-9 * np.abs(w).max())


def test_overlap_fixes_a_variable_at_zero():
    """BnB.jl:74-79: Σ holding both i and -i zeroes both columns of i — feature 0 is in two groups; branched to opposite signs it is 0,
    to the same sign it is constrained, with one of them free it follows the branched one"""
    X, y, P = _tiny(7, overlap=True)
    g = np.flatnonzero(P[0])
    assert len(g) == 2
    a, b = 1 << int(g[0]), 1 << int(g[1])
    full = (1 << (P.shape[1] + 1)) - 1
    ref = NodeReference(X, y, P)
    cases = {(a, full & ~(a | b)): 0, (b, full & ~(a | b)): 0, (a | b, full & ~(a | b)): 1, (0, full & ~(a | b)): -1,
             (a, full & ~a): 1, (0, full & ~b): -1, (0, full): 2}
    for (pat, free), want in cases.items():
        assert node_codes(ref.Po, pat, free)[0] == want, (pat, free)
        r = ref.node(pat, free)
        rn, w = ref.literal_split(pat, free)
        assert abs(r["lb"] - rn) <= 1e-10 * rn
        if want == 0:
            assert r["w"][0] == 0.0 and w[0] == 0.0
    # the fixed variable really bites: the same node with feature 0 free has a lower bound
    Pf = P.copy()
    Pf[0, :] = 0
    loose = NodeReference(X, y, Pf).node(a, full & ~(a | b))["lb"]
    assert loose < ref.node(a, full & ~(a | b))["lb"] * (1 - 1e-6)


def test_nu_equals_the_pairwise_formula():
    rng = np.random.default_rng(8)
    X, y, P = _tiny(8, N=60, D=10, K=4, overlap=True)
    ref = NodeReference(X, y, P)
    for pat, free in _every_node(ref.Kp)[::7]:
        r = ref.node(pat, free)
        np.testing.assert_allclose(r["nu"], nu_pairwise(r["w"], ref.Po), rtol=1e-12, atol=0)
    for _ in range(20):
        w = rng.standard_normal(ref.Mp) * (rng.random(ref.Mp) < 0.7)
        np.testing.assert_allclose(nu_groups(w, ref.Po), nu_pairwise(w, ref.Po), rtol=1e-12, atol=0)


def test_branch_is_the_first_maximal_nu():
    X, y, P = _tiny(9, N=60, D=10, K=4)
    ref = NodeReference(X, y, P)
    seen = set()
    for pat, free in _every_node(ref.Kp):
        r = ref.node(pat, free)
        nu = r["nu"]
        if nu.max() == 0.0:
            assert r["branch"] == -1
        else:
            assert r["branch"] == int(np.flatnonzero(nu == nu.max())[0])
            assert r["gap"] == nu.max() - np.sort(nu)[-2]
        seen.add(r["branch"])
    assert -1 in seen and len(seen) > 2
