"""GPU tests of fit(Opt)'s staged calls on 32- to 40-bit pattern spaces: Gray-index ranges at and above 2^31 / 2^32, the end of a
2^40 space, calibrated bit orders at 40 bits.  A sharded enumeration of K >= 32 groups starts every rank but the first above
Gray index 2^32; these tests run the device and host paths that carry a pattern, a Gray index or a bit position there: the register
kernels' 32-bit loop state (sweep_blk.hip), the 64-bit walks of sweep_lazy.hip / sweep_generic.hip, ref_index_less (common.h), the
cleanup kernel's Gray index -> internal pattern -> reference index (models.hip), the calibration's walk over bits 20-39 (misc.hip),
reference_pattern / install_sweep_result / partls_opt_finish / _pattern / _candidates / _merge_candidates (sweep_setup.hip, opt.hip), the wrappers (api.py).

SAFETY: a full sweep at 40 bits would keep a card busy for half a day and a running kernel cannot be stopped from Python.  Every
opt_sweep / opt_models call of this file goes through wide_reference.guarded (an explicit range of at most 4096 indices inside the
space; test_wide_reference.py checks the gate) — except test_41_sign_bits_stay_out_of_range, whose explicit 16-index calls must be
refused by the library.  Nothing here calls opt_sweep(0, -1), opt_models() without a range, want_all, fit(Opt), cross_validate or Solutions.

Problems (wide_reference.problem): D = 44 / 200 / 345 features for the 256-thread register kernel (T = 3), the 512-thread one (T = 13)
and the deferred-update / eager kernels; K = 39 faithful (40 bits), K = 31 faithful (the space ends exactly at 2^32), K = 40 with a
free intercept (40 bits, reference indices have 41).  Every case asserts its route (Context.sweep_route()) first.

Reference: the oracle's per-pattern NNLS on QR-compressed data (wide_reference.OracleCache), never a second run of the code under test;
the one exception is the suite's lazy-against-eager comparison (test_gpu_lazy.py).  Tolerances are the suite's own for these
quantities at these sizes: _close(1e-9) on exported objectives and models (test_gpu_models.py, test_gpu_tile_counts.py), rtol 1e-10
between the two global-memory kernels (test_gpu_lazy.py), 1e-9 on a finished objective and atol 1e-7 on a finished model
(test_gpu_lazy.py, test_gpu_opt.py: TOL_MODEL).  By the oracle, the two best objectives of every range used here lie > 6e-5 relative
apart (outside the tie test), so each winner is unambiguous; a wrong pattern index fails the exact comparison of the rows' patterns, and
a pattern solved under the signs of its low 32 bits misses the oracle's objective by 1e-4 and more in most rows of a range."""
import numpy as np
import pytest

from models_reference import _cleanup, _close
from wide_reference import cached, gray, gray_inverse, guarded, internal_pattern, reference_index

pytestmark = pytest.mark.gpu

FAITHFUL = 1
REG_256, REG_512, DEFERRED, EAGER = 1, 2, 3, 4              # partls_route (include/partls.h)
KNOBS = ("PARTLS_CHAIN_LEN", "PARTLS_BIT_ORDER", "PARTLS_EAGER_GENERIC", "PARTLS_REG_MAXT", "PARTLS_GRID", "PARTLS_NO_EXPORT",
         "PARTLS_NEAR_TIE_REL")

CASES = {
    "small": dict(seed=4401, D=44, K=39, flags=FAITHFUL, route=(REG_256, 3), rows="all"),
    "small32": dict(seed=4402, D=44, K=31, flags=FAITHFUL, route=(REG_256, 3), rows="all"),
    "mid": dict(seed=4423, D=200, K=39, flags=FAITHFUL, route=(REG_512, 13), rows="window"),
    "large": dict(seed=4404, D=345, K=39, flags=FAITHFUL, route=(DEFERRED, 0), rows="sample"),
    "free": dict(seed=4405, D=44, K=40, flags=0, route=(REG_256, 3)),
    "tie": dict(seed=4406, D=44, K=39, flags=FAITHFUL, route=(REG_256, 3), empty=37),
    "bits41": dict(seed=4407, D=44, K=40, flags=FAITHFUL, route=(REG_256, 3)),
}


def _ref(oracle, name):
    c = CASES[name]
    return cached(oracle, name, c["seed"], c["D"], c["K"], c.get("empty"))


def _ranges(kbits, width=200):
    """(name, g0, g1, focus row): starts that are no multiple of a chain length; the focus row is the first index past the boundary
    (the last index of the space; the 0x5A5A... index of the mixed bit picture)"""
    top = 1 << kbits
    lo = width // 2 + 1
    out = [("2^31", (1 << 31) - lo, (1 << 31) - lo + width, lo)]
    if kbits > 32:
        out.append(("2^32", (1 << 32) - lo, (1 << 32) - lo + width, lo))
    mixed = 0x5A5A5A5A5A & (top - 1)
    out += [("end", top - width, top, width - 1), ("mixed", mixed - 77, mixed - 77 + width, 77)]
    return out


def _context(partls, monkeypatch, name, order=None, chain=None, eager=False):
    """a prepared Context of a case with its knobs (read once, at partls_create); the route is asserted here"""
    c = CASES[name]
    env = {}
    if order:
        env["PARTLS_BIT_ORDER"] = order
    if chain:
        env["PARTLS_CHAIN_LEN"] = str(chain)
    if eager:
        env["PARTLS_EAGER_GENERIC"] = "1"
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = partls.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return ctx, c


def _prepare(ctx, c, ref, eager=False):
    ctx.opt_prepare(ref.X, ref.y, ref.P, 0.0, c["flags"])
    assert ctx.sweep_route() == ((EAGER, 0) if eager else c["route"])
    kbits = c["K"] + 1 if c["flags"] & FAITHFUL else c["K"]
    assert ctx.num_patterns() == 1 << kbits
    return kbits


def _order(ctx, kbits, order, wide_precondition=False):
    """the context's bit order; a forced calibration must have produced a true permutation — with wide_precondition one that moves a group
    k < 32 to a bit >= 32.  That is a precondition on the data, not a property of the library: if it fails, change the generator
    (wide_reference.problem makes groups 0-7 dear for this purpose), not the assertion."""
    gbit = [int(v) for v in ctx.bit_order()[0]]
    assert sorted(gbit) == list(range(kbits)), gbit
    if order == "identity":
        assert gbit == list(range(kbits))
    if order == "calibrate":
        assert gbit != list(range(kbits)), "the calibration kept the identity: the generator must make groups 0-7 dearer"
        if wide_precondition:
            assert any(gbit[k] >= 32 for k in range(32)), gbit
    return gbit


def _rows_to_compare(c, name, n, focus):
    if c["rows"] == "all":
        return list(range(n))
    if c["rows"] == "window":                                 # 128 rows around the focus
        a = min(max(0, focus - 64), n - 128)
        return list(range(a, a + 128))
    rng = np.random.default_rng(len(name) + focus)            # 48 rows: the boundary, the ends, and a fixed sample
    fixed = {0, n - 1, focus, max(0, focus - 1)}
    rest = [i for i in rng.permutation(n).tolist() if i not in fixed]
    return sorted(fixed | set(rest[:48 - len(fixed)]))


def _check_range(ctx, c, ref, gbit, name, g0, g1, focus, tag):
    """rows of opt_models against the oracle (identity of every row, values of the case's rows), the sweep's winner, its finish"""
    P = ref.P
    r = guarded(ctx, "opt_models", g0, g1, raw=True)
    want = [reference_index(gray(g), gbit) for g in range(g0, g1)]
    got = [int(v) for v in r["pattern"]]
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%s: row %d (Gray index %d) carries pattern %#x, expected %#x (%d rows differ)" % (
        tag, bad[0], g0 + bad[0], got[bad[0]], want[bad[0]], len(bad))
    assert r["n_unconverged"] == 0 and r["n_vetoes"] == 0, tag
    rows = _rows_to_compare(c, name, len(want), focus)
    objs, ra = ref.rows([want[i] for i in rows])
    err = np.abs(r["opt"][rows] - objs) / np.maximum(1.0, objs)
    print("[wide] %s: %d rows, max objective error %.3g at row %d" % (tag, len(rows), err.max(), rows[int(np.argmax(err))]))
    _close(r["opt"][rows], objs)
    _close(r["raw_alpha"][rows], ra)
    cl = [_cleanup(ra[j], P, want[i]) for j, i in enumerate(rows)]
    _close(r["alpha"][rows], np.stack([m[0] for m in cl]))
    _close(r["beta"][rows], np.stack([m[1] for m in cl]))
    _close(r["t"][rows], np.array([m[2] for m in cl]))
    # the sweep of the same range: its winner is the first reference index among the rows of least objective, bit for bit (both calls
    # walk one range on one chain plan: include/partls.h)
    bo, bp, _, unconv = guarded(ctx, "opt_sweep", g0, g1)
    assert unconv == 0, tag
    i = min(range(len(want)), key=lambda j: (float(r["opt"][j]), want[j]))
    assert (bo, bp) == (float(r["opt"][i]), want[i]), "%s: sweep's winner (%.17g, %#x), rows' minimum (%.17g, %#x) at row %d" % (
        tag, bo, bp, float(r["opt"][i]), want[i], i)
    _check_finish(ctx, ref, bp, tag)
    return r


def _check_finish(ctx, ref, b, tag, expect_index=None):
    """opt_finish(b): the pattern's own index, the oracle's data-space objective and the cleaned model of the oracle's raw alpha"""
    a, bt, t, opt, bi = ctx.opt_finish(b)
    want = b if expect_index is None else expect_index
    assert bi == want, "%s: opt_finish(%#x) returned best_index %#x, expected %#x" % (tag, b, bi, want)
    do = ref.data_objective(want)
    assert abs(opt - do) <= 1e-9 * max(1.0, do), "%s: finished objective %.17g, oracle %.17g" % (tag, opt, do)
    _, ra = ref.rows([want])
    ca, cb, ct = _cleanup(ra[0], ref.P, want)
    np.testing.assert_allclose(a, ca, atol=1e-7, err_msg=tag)
    np.testing.assert_allclose(bt, cb, atol=1e-7, err_msg=tag)
    np.testing.assert_allclose(t, ct, atol=1e-7, err_msg=tag)
    return a, bt, t, opt, bi


SWEEPS = ([("small", o, ch) for o in ("identity", "calibrate") for ch in (None, 64, 1)] + [("small", None, None)]
          + [("small32", "identity", ch) for ch in (None, 64, 1)] + [("small32", "calibrate", 64)]
          + [("mid", o, ch) for o in ("identity", "calibrate") for ch in (None, 64, 1)]
          + [("large", "identity", ch) for ch in (None, 64, 1)] + [("large", "calibrate", None)])


@pytest.mark.parametrize("name,order,chain", SWEEPS, ids=["%s-%s-chain%s" % (n, o or "default", ch or "plan") for n, o, ch in SWEEPS])
def test_rows_and_winner_of_every_range(partls, oracle, monkeypatch, name, order, chain):
    """Every range (straddling 2^31 and 2^32, the last 200 indices of the space, a mixed bit picture) under the default chain plan, with
    PARTLS_CHAIN_LEN=64 (one chain crosses the boundary in mid-chain: the low word of g0 + gi carries) and 1 (every pattern its own
    workgroup result: the host does all the ranking), in the identity order, a forced calibration and, once, whatever the default
    picks at 40 bits.  large (identity): the deferred-update kernel's rows also against the eager kernel's, every row."""
    ref = _ref(oracle, name)
    ctx, c = _context(partls, monkeypatch, name, order, chain)
    try:
        kbits = _prepare(ctx, c, ref)
        gbit = _order(ctx, kbits, order, wide_precondition=name in ("small", "mid"))
        out = {}
        for rname, g0, g1, focus in _ranges(kbits):
            tag = "%s %s order=%s chain=%s [%d, %d)" % (name, rname, order, chain, g0, g1)
            out[rname] = _check_range(ctx, c, ref, gbit, name, g0, g1, focus, tag)
    finally:
        ctx.close()
    if name != "large" or order != "identity":
        return
    ctx, c = _context(partls, monkeypatch, name, order, chain, eager=True)
    try:
        kbits = _prepare(ctx, c, ref, eager=True)
        gbit = _order(ctx, kbits, order)
        for rname, g0, g1, focus in _ranges(kbits):
            tag = "%s %s eager chain=%s [%d, %d)" % (name, rname, chain, g0, g1)
            eg = _check_range(ctx, c, ref, gbit, name, g0, g1, focus, tag)
            assert np.array_equal(eg["pattern"], out[rname]["pattern"]), tag
            np.testing.assert_allclose(out[rname]["opt"], eg["opt"], rtol=1e-10, err_msg=tag)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,order", [("small", "identity"), ("small", "calibrate"), ("mid", "calibrate")])
def test_scattered_single_indices(partls, oracle, monkeypatch, name, order):
    """16 reference patterns with bit 39 or 38 set -> their Gray indices -> one-row exports: the pattern comes back, the objective is
    the oracle's, and the per-pattern path (opt_pattern) returns the row's raw alpha and objective"""
    ref = _ref(oracle, name)
    rng = np.random.default_rng(39)
    pats = [int(rng.integers(0, 1 << 38)) | (int(rng.integers(1, 4)) << 38) for _ in range(16)]
    assert all(b >> 38 for b in pats) and any((b >> 39) & 1 for b in pats) and any(not (b >> 39) & 1 for b in pats)
    objs, ra = ref.rows(pats)
    ctx, c = _context(partls, monkeypatch, name, order)
    try:
        kbits = _prepare(ctx, c, ref)
        gbit = _order(ctx, kbits, order, wide_precondition=True)
        for j, b in enumerate(pats):
            g = gray_inverse(internal_pattern(b, gbit))
            tag = "%s order=%s pattern %#x at Gray index %d" % (name, order, b, g)
            r = guarded(ctx, "opt_models", g, g + 1, raw=True)
            assert int(r["pattern"][0]) == b, "%s: came back as %#x" % (tag, int(r["pattern"][0]))
            assert r["n_unconverged"] == 0 and r["n_vetoes"] == 0, tag
            _close(r["opt"], objs[j:j + 1])
            _close(r["raw_alpha"], ra[j:j + 1])
            pa, po = ctx.opt_pattern(b)
            _close(pa, r["raw_alpha"][0])
            _close(po, r["opt"][0])
    finally:
        ctx.close()
    assert sum(gray_inverse(internal_pattern(b, gbit)) >> 32 != 0 for b in pats) >= 8       # the indices do lie above 2^32


@pytest.mark.parametrize("order", ["identity", "calibrate"])
@pytest.mark.parametrize("world,rank", [(3, 1), (7, 3)])
def test_shards_meet_above_2_32(partls, oracle, monkeypatch, world, rank, order):
    """two neighbouring shards of a 2^40 space: their merged candidates name the winner one sweep across the boundary names, and the
    finish of that winner gives the same model"""
    ref = _ref(oracle, "small")
    ctx, c = _context(partls, monkeypatch, "small", order)
    try:
        kbits = _prepare(ctx, c, ref)
        _order(ctx, kbits, order, wide_precondition=True)
        b = partls.dist.shard_range(1 << 40, rank, world)[1]
        assert b == partls.dist.shard_range(1 << 40, rank + 1, world)[0] and b > 1 << 32 and b % 64 != 0
        bo, bp, _, unconv = guarded(ctx, "opt_sweep", b - 33, b + 31)
        assert unconv == 0
        single = _check_finish(ctx, ref, bp, "one sweep across the shard boundary %d" % b)
        cands = []
        for g0, g1 in ((b - 33, b), (b, b + 31)):            # the upper shard last: the context is then in the state of that rank
            _, _, _, unconv = guarded(ctx, "opt_sweep", g0, g1)
            assert unconv == 0
            cands.append(ctx.opt_candidates())
        assert all(len(o) >= 1 for o, _ in cands)
        wo, wp = ctx.opt_merge_candidates(np.concatenate([o for o, _ in cands]), np.concatenate([p for _, p in cands]))
        assert wp == bp and abs(wo - bo) <= 1e-10 * bo, (wo, wp, bo, bp)
        merged = _check_finish(ctx, ref, wp, "merged candidates at the shard boundary %d" % b)
    finally:
        ctx.close()
    assert np.array_equal(merged[4], single[4])
    for u, v in zip(merged[:4], single[:4]):
        np.testing.assert_allclose(u, v, atol=1e-9)


def _tie_pairs(p):
    """{clear bit visited first: x}: Gray indices x > 2^32 such that x - 1 and x differ in internal bit p only"""
    out = {}
    m = ((1 << 33) >> p) | 1
    while len(out) < 2 and (m << p) < 1 << 40:
        x = m << p
        assert x > 1 << 32 and gray(x - 1) ^ gray(x) == 1 << p
        out.setdefault((gray(x - 1) >> p) & 1 == 0, x)
        m += 2
    return out


@pytest.mark.parametrize("chain", [2, 1])
@pytest.mark.parametrize("order", ["identity", "calibrate"])
def test_exact_ties_on_a_high_bit(partls, oracle, monkeypatch, order, chain):
    """group 37 has no feature: the two patterns that differ in reference bit 37 are one subproblem (the oracle's objectives are
    bitwise equal) and the reference's argmin keeps the first index, the one with bit 37 clear (Opt.jl:96), whichever is visited first.
    PARTLS_CHAIN_LEN=2: both patterns in one workgroup, ref_index_less decides in the kernel; 1: two workgroups, the host decides."""
    ref = _ref(oracle, "tie")
    ctx, c = _context(partls, monkeypatch, "tie", order, chain)
    try:
        kbits = _prepare(ctx, c, ref)
        gbit = _order(ctx, kbits, order)
        pairs = _tie_pairs(gbit[37])
        assert set(pairs) == {True, False}, "group 37 sits on bit %d: no pair in either visiting order" % gbit[37]
        if order == "identity":
            assert pairs == {True: 1 << 37, False: 3 << 37}
        for first_clear, x in pairs.items():
            tag = "order=%s chain=%d [%d, %d), bit-37-clear pattern visited %s" % (order, chain, x - 1, x + 1, "first" if first_clear else "last")
            pats = [reference_index(gray(x - 1), gbit), reference_index(gray(x), gbit)]
            assert pats[0] ^ pats[1] == 1 << 37 and ((pats[0] >> 37) & 1 == 0) == first_clear
            o, _ = ref.rows(pats)
            assert o[0] == o[1]
            r = guarded(ctx, "opt_models", x - 1, x + 1, raw=True)
            assert [int(v) for v in r["pattern"]] == pats, tag
            _close(r["opt"], o)
            bo, bp, _, unconv = guarded(ctx, "opt_sweep", x - 1, x + 1)
            assert unconv == 0
            assert bp == min(pats) and (bp >> 37) & 1 == 0, "%s: the sweep kept %#x (device objectives %.17g, %.17g)" % (
                tag, bp, r["opt"][0], r["opt"][1])
            _close(bo, o[0])
            _check_finish(ctx, ref, bp, tag)
            _check_finish(ctx, ref, max(pats), tag, expect_index=min(pats))          # an unused group's bit never reaches best_index
    finally:
        ctx.close()


@pytest.mark.parametrize("order,chain", [("identity", None), ("calibrate", None), ("calibrate", 64)])
def test_free_intercept_at_40_groups(partls, oracle, monkeypatch, order, chain):
    """K = 40, flags = 0: 2^40 patterns of the groups' signs, the intercept free; reference indices carry the intercept's sign in bit 40.
    Sweep only (opt_models needs the faithful flag: test_gpu_models.py): the winner of 64-index ranges at the four offsets against the
    better of the oracle's two intercept signs per pattern, the finish's 41-bit best_index, and the bound of opt_finish's argument."""
    ref = _ref(oracle, "free")
    ctx, c = _context(partls, monkeypatch, "free", order, chain)
    try:
        kbits = _prepare(ctx, c, ref)
        assert kbits == 40
        gbit = _order(ctx, kbits, order, wide_precondition=True)
        for rname, g0, g1, _ in _ranges(kbits, width=64):
            tag = "free %s order=%s chain=%s [%d, %d)" % (rname, order, chain, g0, g1)
            pats = [reference_index(gray(g), gbit) for g in range(g0, g1)]
            neg, _ = ref.rows(pats)
            pos, _ = ref.rows([b | 1 << 40 for b in pats])
            both = sorted([(float(neg[i]), b) for i, b in enumerate(pats)] + [(float(pos[i]), b | 1 << 40) for i, b in enumerate(pats)])
            bo, bp, _, unconv = guarded(ctx, "opt_sweep", g0, g1)
            assert unconv == 0, tag
            assert abs(bo - both[0][0]) <= 1e-9 * max(1.0, both[0][0]), "%s: best objective %.17g, oracle %.17g" % (tag, bo, both[0][0])
            assert bp == both[0][1] & ((1 << 40) - 1), "%s: winner %#x, oracle %#x" % (tag, bp, both[0][1])
            _check_finish(ctx, ref, bp, tag, expect_index=both[0][1])
        with pytest.raises(partls.PartlsError) as ei:
            ctx.opt_finish(1 << 41)
        assert ei.value.status == partls.lowlevel.ERR_BAD_ARG
    finally:
        ctx.close()


def test_41_sign_bits_stay_out_of_range(partls, oracle, monkeypatch):
    """K = 40 with the faithful intercept is 41 sign bits: no pattern space, and explicit small ranges are refused before any launch
    (called directly: the gate's assertion needs a pattern space; fit(Opt)'s refusal is test_gpu_alt_bnb.py's)"""
    ref = _ref(oracle, "bits41")
    ctx, c = _context(partls, monkeypatch, "bits41")
    try:
        ctx.opt_prepare(ref.X, ref.y, ref.P, 0.0, FAITHFUL)
        assert ctx.num_patterns() == 0
        for call in (lambda: ctx.opt_sweep(0, 16), lambda: ctx.opt_models(0, 16), ctx.bit_order):
            with pytest.raises(partls.PartlsError) as ei:
                call()
            assert ei.value.status == partls.lowlevel.ERR_UNSUPPORTED and "K <= 39" in str(ei.value)
        assert ctx.pivots() == 0                                                 # nothing ran
    finally:
        ctx.close()
