"""CPU checks of tests/wide_reference.py, the index arithmetic and oracle cache behind test_gpu_wide_patterns.py: the GPU tests
derive every expected pattern from these functions, so they are checked here against definitions of their own (bit lists, Gray's
one-bit-per-step property) at the values where a 32-bit slip would show."""
import random

import numpy as np
import pytest

from wide_reference import MAX_RANGE, OracleCache, gray, gray_inverse, guarded, internal_pattern, problem, reference_index

EDGES = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) - 1]


def _values():
    rnd = random.Random(40)
    return EDGES + [rnd.getrandbits(40) for _ in range(2000)]


def test_gray_and_its_inverse():
    for g in _values():
        q = gray(g)
        assert 0 <= q < 1 << 40
        assert gray_inverse(q) == g and gray(gray_inverse(g)) == g
        bits = [(g >> i) & 1 for i in range(41)]                                  # the definition, bit by bit: q_i = g_i xor g_(i+1)
        assert q == sum((bits[i] ^ bits[i + 1]) << i for i in range(40))
        if g + 1 < 1 << 40:
            d = gray(g) ^ gray(g + 1)                                             # one bit per step: the lowest set bit of g + 1
            assert d == (g + 1) & -(g + 1)


def test_bit_orders_are_inverse_to_each_other():
    rnd = random.Random(41)
    for kb in (32, 40, 41):
        orders = [list(range(kb)), list(reversed(range(kb)))] + [rnd.sample(range(kb), kb) for _ in range(20)]
        for gbit in orders:
            gb = np.array(gbit, dtype=np.int64)                                   # as Context.bit_order returns it
            for v in [e & ((1 << kb) - 1) for e in EDGES] + [rnd.getrandbits(kb) for _ in range(100)]:
                b = reference_index(v, gb)
                assert 0 <= b < 1 << kb and internal_pattern(b, gb) == v
                assert reference_index(internal_pattern(v, gb), gb) == v
                assert all((b >> k) & 1 == (v >> gbit[k]) & 1 for k in range(kb))
        assert reference_index(0x123456789A % (1 << kb), list(range(kb))) == 0x123456789A % (1 << kb)
    assert reference_index(1 << 39, [39] + list(range(39))) == 1 and internal_pattern(1, [39] + list(range(39))) == 1 << 39


def test_neighbours_at_bit_37():
    assert gray((1 << 37) - 1) == 0x1000000000 and gray(1 << 37) == 0x3000000000
    assert gray((1 << 37) - 1) ^ gray(1 << 37) == 1 << 37
    a, b = gray(3 * (1 << 37) - 1), gray(3 * (1 << 37))
    assert a ^ b == 1 << 37 and (a >> 37) & 1 == 1 and (b >> 37) & 1 == 0


class _FakeContext:
    def __init__(self, npat):
        self.npat, self.calls = npat, []

    def num_patterns(self):
        return self.npat

    def opt_sweep(self, g0, g1, **kw):
        self.calls.append(("opt_sweep", g0, g1, kw))
        return "swept"

    def opt_models(self, g0, g1, **kw):
        self.calls.append(("opt_models", g0, g1, kw))
        return "exported"


def test_the_gate_admits_short_ranges_inside_the_space_only():
    ctx = _FakeContext(1 << 40)
    assert guarded(ctx, "opt_sweep", (1 << 40) - 200, 1 << 40) == "swept"
    assert guarded(ctx, "opt_models", 1 << 32, (1 << 32) + MAX_RANGE, raw=True) == "exported"
    assert ctx.calls == [("opt_sweep", (1 << 40) - 200, 1 << 40, {}), ("opt_models", 1 << 32, (1 << 32) + MAX_RANGE, {"raw": True})]
    for bad in ((0, -1), (0, 0), (5, 4), (-1, 3), (0, MAX_RANGE + 1), ((1 << 40) - 1, (1 << 40) + 1)):
        with pytest.raises(AssertionError):
            guarded(ctx, "opt_sweep", *bad)
    with pytest.raises(AssertionError):
        guarded(ctx, "opt_sweep", 0, 16, want_all=True)
    with pytest.raises(AssertionError):
        guarded(ctx, "opt_finish", 0, 16)
    with pytest.raises(AssertionError):
        guarded(_FakeContext(0), "opt_sweep", 0, 16)                              # 41 sign bits: num_patterns() == 0
    assert len(ctx.calls) == 2


def test_generator_layout():
    X, y, P = problem(7, 44, 39)
    assert X.shape == (3 * 44 + 40, 44) and P.shape == (44, 39) and (P.sum(axis=1) == 1).all()
    assert (P.sum(axis=0) >= 1).all() and P[:, 8:].sum() == 31 and P[:, :8].sum() == 13          # the surplus sits in groups 0-7
    X2, y2, P2 = problem(7, 44, 39)
    assert np.array_equal(X, X2) and np.array_equal(y, y2) and np.array_equal(P, P2)
    _, _, Pe = problem(7, 44, 39, empty=37)
    assert Pe[:, 37].sum() == 0 and (np.delete(Pe, 37, axis=1).sum(axis=0) >= 1).all() and (Pe.sum(axis=1) == 1).all()


def test_oracle_takes_40_bit_patterns_and_ties_on_an_empty_group(oracle):
    """group 37 without a feature: the two patterns that differ in bit 37 only are one subproblem, bitwise; a pattern and its low
    32 bits are not (a truncation on the device cannot hide under the tests' 1e-9); QR-compressed and dense data agree"""
    c = OracleCache(oracle, *problem(11, 44, 39, empty=37))
    for lo, hi in (((1 << 37) - 1, 1 << 37), (3 * (1 << 37) - 1, 3 * (1 << 37))):
        o, ra = c.rows([gray(lo), gray(hi)])
        assert o[0] == o[1] and np.array_equal(ra[0], ra[1])
    full = OracleCache(oracle, *problem(12, 44, 39))
    pats = [gray(g) for g in range((1 << 32) - 20, (1 << 32) + 20)] + [gray((1 << 40) - 1), 0x80000000FF]
    o, ra = full.rows(pats)
    assert ra.shape == (len(pats), 45) and np.isfinite(o).all()
    o2, _ = full.rows(pats)                                                       # from the cache
    assert np.array_equal(o, o2)
    wide = [p for p in pats if p >> 32]
    ow, _ = full.rows(wide)
    ot, _ = full.rows([p & 0xFFFFFFFF for p in wide])
    assert np.min(np.abs(ow - ot) / ow) > 1e-6
    dense = np.array([full.data_objective(p) for p in pats[:6]])
    np.testing.assert_allclose(dense, o[:6], rtol=1e-12)
