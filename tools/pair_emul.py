"""numpy emulation of the PAIR WALK of sweep_blk.hip (development aid; never imported by the product or the tests).

The walk, the pricing of a twin and its guards follow the kernel statement by statement (sweep_body's pair_partner / pair_unit_end /
pair_target / pair_next and pair_solve), on tools/tableau_emul.py's dense tableau and its sequential pivot():

  * patterns g and g ^ 1 of a chain are a pair; the tableau visits the member whose bit 0 is the committed state's;
  * the twin is priced from the columns T[:, C] of its violators C: the |C| x |C| system of the pivot rows with the rhs entries q_C
    as a column, sequential pivots in ascending order (T_ik / |d|, T_kk = -1/d), a_k = +q'_k (entering) / -q'_k (leaving),
    q_i' = q_i - sum_k T_ik a_k, corner' = corner - sum_k q_k a_k;  every priced twin is ALSO pivoted sequentially on a copy of the
    tableau and the two results are compared (`formula error`: the check of the sign conventions);
  * hard twins (|C| > 16, an entering pivot at or below the guard, violators left) go to the ordinary rounds.

Reports, per problem: committed pivots against the plain walk's, easy / hard twins, |C|, tile columns of C, the smallest pivot, the
largest error against the oracle, and the twins that were priced although the ordinary path (the leave-one-out rule of the rounds)
rejects a column for them — that count must be 0.

  python tools/pair_emul.py tests            the problems of tests/test_gpu_pair.py and tests/test_gpu_pair_routes.py
  python tools/pair_emul.py fuzz [count]     problems drawn by tests/test_gpu_fuzz.py's _random_problem (default 200)
  python tools/pair_emul.py static [count]   the same fuzz problems after the host's relayout (pair_relayout, sweep_setup.hip): the live
                                             variables of the group on bit 0 in ONE tile column, the twin priced from that column alone
                                             (price_static: all its columns gathered, the violator mask taken from its rhs entries only).
                                             Fails if a twin has a violator outside the column, if the relayout moves another variable out
                                             of order, or on any priced-but-rejected twin.  The fuzz problems are small, so the tile width
                                             is 16 where two full columns exist and 8 or 4 below that; the tests' problems run at 16.
  python tools/pair_emul.py dense [count]    the kernel's DENSE pricing (price_dense: the whole 16 x 16 block of the column as it stands, the
                                             steps masked, every row 16 terms with a_k = 0 outside C) against price_static, bit for bit, on the
                                             same fuzz problems, the problems of tests/test_gpu_pair.py and those of
                                             tests/test_gpu_pair_dense.py (whose expected pivot counts come from here).  Exit status 0 or 1.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
sys.path.insert(0, os.path.join(os.getcwd(), "tools"))

from tableau_emul import pivot, prepare  # noqa: E402

PAIR_MAXC = 16
PIV_MIN = 1.00000000055e-4          # sweep_blk.hip: PAIR_PIV_MIN_HI (the high word of the pivot above that of 1e-4)
PIV_EPS = 1e-11


def pop(v):
    return bin(int(v)).count("1")


def signs(mask, n, pat):
    return np.array([2 * pop(int(mask[v]) & pat) - pop(mask[v]) for v in range(n)])


def violators(T, n, basic, f, tol, blocked=None):
    q = T[:n, n]
    fq = np.where(f > 0, q, np.where(f < 0, -q, 0.0))
    nb = (fq > tol) if blocked is None else ((fq > tol) & ~blocked)
    return np.where(basic, (f == 0) | (fq < -tol), nb)


def rounds(T, n, basic, f, tol, stats):
    """the ordinary exchange rounds (tableau_emul.sweep's body, leave-one-out rule); returns pivots applied"""
    blocked = np.zeros(n, dtype=bool)
    ninf_best, patience, nr, progress, npiv = n + 1, 3, 0, False, 0
    while True:
        if progress:
            blocked[:] = False
        progress = False
        viol = np.nonzero(violators(T, n, basic, f, tol, blocked))[0]
        if len(viol) == 0:
            return npiv
        if len(viol) < ninf_best:
            ninf_best, patience, allv = len(viol), 3, True
        elif patience > 0:
            patience -= 1
            allv = True
        else:
            allv = False
        nr += 1
        if nr > 20 * (n + 1):
            stats["capped"] += 1
            return npiv
        if not allv:
            viol = viol[-1:]
        for k in viol:
            d = T[k, k]
            if not basic[k]:
                col = np.delete(T[:n, k], k)
                cmax2 = float(np.max(col ** 2)) if len(col) else 0.0
                if d <= PIV_EPS * max(1.0, cmax2):
                    blocked[k] = True
                    stats["rejections"] += 1
                    continue
            pivot(T, k, d)
            basic[k] = not basic[k]
            progress = True
            npiv += 1


def price(T, n, basic, C):
    """pair_solve + the row phase: (guard fired, q', corner', smallest entering pivot)"""
    m = len(C)
    A = T[np.ix_(C, C)].copy()
    qc = T[C, n].copy()
    dmin = np.inf
    for s in range(m):
        d = A[s, s]
        if not basic[C[s]]:
            dmin = min(dmin, d)
            if not d >= PIV_MIN:
                return True, None, None, dmin
        inv = 1.0 / d
        ainv = abs(inv)
        col = A[:, s].copy()                      # the pivot COLUMN: u_j = col[j]
        qs = qc[s]
        for r in range(m):
            fz = -col[r] * inv
            if r == s:
                A[r, :] = col * ainv
                qc[r] = qs * ainv
            else:
                A[r, :] += fz * col
                qc[r] += fz * qs
        A[:, s] = col * ainv
        A[s, s] = -inv
    a = np.where(basic[C], -qc, qc)
    qt, ct = T[:n, n].copy(), T[n, n]
    for j in range(m):                            # the rows: one term per violator, ascending (the kernel's chain of FMAs)
        qt = qt + (-T[:n, C[j]]) * a[j]
        ct = ct + (-T[C[j], n]) * a[j]
    qt[C] = qc
    return False, qt, ct, dmin


def relayout(pr, width=16):
    """pair_relayout: the problem with the live variables of the group on bit 0 in tile column T - 2 (tiles of `width`), every other
    variable in its present relative order; None where the kernel would keep the parent's layout (the group does not fit, T < 2)"""
    n, mask, scale = pr["n"], pr["mask"], pr["scale"]
    T = (n + width - 1) // width
    on0 = np.array([bool(int(mask[i]) & 1) and scale[i] != 0.0 for i in range(n)])
    if T < 2 or on0.sum() > width:
        return None
    base = width * (T - 2)
    grp, oth = [i for i in range(n) if on0[i]], [i for i in range(n) if not on0[i]]
    idx = oth[:base] + grp + oth[base:]
    assert sorted(idx) == list(range(n)) and [i for i in idx if not on0[i]] == oth and idx[base:base + len(grp)] == grp
    full = idx + [n]
    out = dict(pr, T0=pr["T0"][np.ix_(full, full)].copy(), mask=mask[idx], perm=[pr["perm"][i] for i in idx], scale=scale[idx])
    out["pair_col"] = (base, width)
    return out


def price_static(T, n, basic, ft, tol, col):
    """the kernel's pricing from the fixed column: violator mask from the column's rhs entries alone, all `width` columns gathered, the
    solve and the rows restricted to the mask's variables.  (C, price(...)); C is None when a violator lies outside the column"""
    base, width = col
    viol = violators(T, n, basic, ft, tol)
    if viol[:base].any() or viol[base + width:].any():
        return None, None
    panel = T[:, base:base + width].copy()                  # the gather: every column of the tile column, rhs row included
    cm = [k for k in range(width) if viol[base + k]]
    C = np.array([base + k for k in cm], dtype=int)
    Tp = np.zeros_like(T)                                   # only what the panel holds may be read
    Tp[:, C] = panel[:, cm]
    Tp[C, n] = panel[n, cm]                                 # the rhs entries of C: the panel's rhs row, by symmetry
    Tp[:n, n] = np.where(np.isin(np.arange(n), C), Tp[:n, n], T[:n, n])
    Tp[n, n] = T[n, n]
    return C, price(Tp, n, basic, C)


def price_dense(T, n, basic, ft, tol, col):
    """the kernel's DENSE pricing from the fixed column: the whole width x width block of the column is loaded as it stands (rows and
    columns outside C carry the tableau's entries, never zeros), the steps run over k = 0 .. width - 1 and skip the columns outside C,
    every step updates every row and column of the block, a_k = 0 outside C and every row adds all `width` terms in ascending k.
    (C, (guard, q', corner', smallest entering pivot), mask of C) as price_static; C is None when a violator lies outside the column"""
    base, width = col
    viol = violators(T, n, basic, ft, tol)
    if viol[:base].any() or viol[base + width:].any():
        return None, None, 0
    panel = T[:, base:base + width].copy()                  # the gather: rows 0 .. n - 1 and the rhs row n
    cm = sum(1 << k for k in range(width) if viol[base + k])
    C = np.array([base + k for k in range(width) if (cm >> k) & 1], dtype=int)
    A = panel[base:base + width, :].copy()
    qc = panel[n, :].copy()
    bas = basic[base:base + width]
    dmin = np.inf
    for s in range(width):
        if not (cm >> s) & 1:
            continue
        d = A[s, s]
        if not bas[s]:
            dmin = min(dmin, d)
            if not d >= PIV_MIN:
                return C, (True, None, None, dmin), cm
        inv = 1.0 / d
        ainv = abs(inv)
        colv = A[:, s].copy()
        qs = qc[s]
        for r in range(width):
            fz = -colv[r] * inv
            if r == s:
                A[r, :] = colv * ainv
                qc[r] = qs * ainv
            else:
                A[r, :] += fz * colv
                qc[r] += fz * qs
        A[:, s] = colv * ainv
        A[s, s] = -inv
    a = np.array([(-qc[k] if bas[k] else qc[k]) if (cm >> k) & 1 else 0.0 for k in range(width)])
    qt, ct = T[:n, n].copy(), T[n, n]
    for k in range(width):
        qt = qt + (-panel[:n, k]) * a[k]
        ct = ct + (-panel[n, k]) * a[k]
    qt[C] = qc[C - base]
    return C, (False, qt, ct, dmin), cm


def same_price(x, y):
    """two pricings of one twin, bit for bit: guard, q', corner', smallest entering pivot"""
    if x[0] != y[0] or x[3] != y[3]:
        return False
    return x[0] or (np.array_equal(x[1], y[1]) and x[2] == y[2])


def pair_sweep(pr, chain_len, g_begin=0, g_end=None, pairing=True):
    n, T0, mask, kbits, tol = pr["n"], pr["T0"], pr["mask"], pr["kbits"], pr["tol"]
    pcol = pr.get("pair_col")
    g_end = (1 << kbits) if g_end is None else g_end
    out = np.full(1 << kbits, np.nan)
    st = dict(pivots=0, easy=0, empty=0, hard_wide=0, hard_guard=0, hard_left=0, capped=0, rejections=0, csize=[], ctiles=[],
              dmin=np.inf, formula_err=0.0, priced_but_rejected=0, outside=0, dense=0, dense_diff=0, gap_easy=0)
    dense = pr.get("dense", False)
    gray = lambda g: g ^ (g >> 1)
    for g0 in range(g_begin, g_end, chain_len):
        glen = min(chain_len, g_end - g0)
        T = T0.copy()
        basic = np.zeros(n, dtype=bool)

        def partner(i):
            j = i - 1 if (g0 + i) & 1 else i + 1
            return j if pairing and 0 <= j < glen else -1

        def unit_end(i):
            return max(i, partner(i)) + 1

        def target(u, i):
            if partner(u) < 0 or (g0 + u) & 1:
                return u
            return u + 1 if (gray(g0 + u) ^ gray(g0 + i)) & 1 else u

        gi, pending = 0, partner(0) >= 0
        while True:
            f = signs(mask, n, gray(g0 + gi))
            st["pivots"] += rounds(T, n, basic, f, tol, st)
            out[gray(g0 + gi)] = np.sqrt(max(T[n, n], 0.0))
            to_twin = False
            if pending:
                ft = signs(mask, n, gray(g0 + partner(gi)))
                C = np.nonzero(violators(T, n, basic, ft, tol))[0]
                to_twin = True
                static = None
                if pcol is not None:
                    Cs, static = price_static(T, n, basic, ft, tol, pcol)
                    if Cs is None:
                        st["outside"] += 1
                    else:
                        assert np.array_equal(Cs, C)
                        if dense and 0 < len(C) <= PAIR_MAXC:           # the dense form prices the walk; the compacted one is its check
                            Cd, dns, cmask = price_dense(T, n, basic, ft, tol, pcol)
                            st["dense"] += 1
                            st["dense_diff"] += not (np.array_equal(Cd, C) and same_price(static, dns))
                            static = dns
                if len(C) == 0:
                    st["empty"] += 1
                    out[gray(g0 + partner(gi))] = np.sqrt(max(T[n, n], 0.0))
                    to_twin = False
                elif len(C) > PAIR_MAXC:
                    st["hard_wide"] += 1
                else:
                    guard, qt, ct, dmin = price(T, n, basic, C) if static is None else static
                    st["dmin"] = min(st["dmin"], dmin)
                    if guard:
                        st["hard_guard"] += 1
                    else:
                        bt = basic.copy()
                        bt[C] = ~bt[C]
                        T2 = T.copy()
                        T2[:n, n] = qt
                        if violators(T2, n, bt, ft, tol).any():
                            st["hard_left"] += 1
                        else:
                            st["easy"] += 1
                            st["csize"].append(len(C))
                            if pcol is not None:                        # a column between the lowest and the highest of C is not in C
                                st["gap_easy"] += int(C[-1] - C[0] + 1 > len(C))
                            st["ctiles"].append(len(set(int(k) // 16 for k in C)))
                            out[gray(g0 + partner(gi))] = np.sqrt(max(ct, 0.0))
                            to_twin = False
                            # the sign conventions: sequential pivot() of the same block on a copy; and what the rounds would reject
                            T3 = T.copy()
                            rej = False
                            for k in C:
                                d = T3[k, k]
                                if not basic[k]:
                                    col = np.delete(T3[:n, k], k)
                                    rej = rej or d <= PIV_EPS * max(1.0, float(np.max(col ** 2)))
                                pivot(T3, k, d)
                            st["priced_but_rejected"] += int(rej)
                            scale = max(1.0, float(np.max(np.abs(T3[:n, n]))))
                            st["formula_err"] = max(st["formula_err"], float(np.max(np.abs(T3[:n, n] - qt))) / scale,
                                                    abs(T3[n, n] - ct) / max(1.0, abs(ct)))
            if to_twin:
                gi, pending = partner(gi), False
                continue
            u = unit_end(gi)
            if u >= glen:
                break
            gi = target(u, gi)
            pending = partner(gi) >= 0
    return out, st


def report(tag, pr, ref, chain_len, **kw):
    plain, sp = pair_sweep(pr, chain_len, pairing=False, **kw)
    got, st = pair_sweep(pr, chain_len, **kw)
    st["plain_pivots"] = sp["pivots"]
    seen = ~np.isnan(got)
    err = float(np.max(np.abs(got[seen] - ref[seen]) / np.maximum(1.0, ref[seen]))) if ref is not None else float("nan")
    hard = st["hard_wide"] + st["hard_guard"] + st["hard_left"]
    cs = st["csize"]
    print("%-28s pivots %6d (plain walk %6d)  twins: easy %4d empty %4d hard %4d (wide %d guard %d left %d)  |C| %s  tiles %s  min pivot %.3g  "
          "formula err %.2g  oracle err %.2g  priced-but-rejected %d  capped %d" % (
              tag, st["pivots"], sp["pivots"], st["easy"], st["empty"], hard, st["hard_wide"], st["hard_guard"], st["hard_left"],
              ("%d..%d" % (min(cs), max(cs))) if cs else "-", ("%d..%d" % (min(st["ctiles"]), max(st["ctiles"]))) if cs else "-",
              st["dmin"], st["formula_err"], err, st["priced_but_rejected"], st["capped"]))
    return st, err


def main():
    from oracle import oracle as O
    O.build()
    what = sys.argv[1] if len(sys.argv) > 1 else "tests"
    bad = 0
    if what == "tests":
        import test_gpu_pair as tp
        for kind, n, flags in tp.CASES:
            X, y, P = tp.problem(kind, n, flags)
            faithful = bool(flags & tp.FAITHFUL)
            ref = None
            if faithful:
                Xo, Po = O.homogeneous(X, P)
                R, z = O.compress(Xo, y)
                ref = O.opt_patterns(R, z, Po, np.arange(1 << (tp.K + 1)))
            pr = prepare(np.asarray(X), y, np.asarray(P), 0.0, faithful=faithful)
            for cl in (16, 7):
                st, err = report("%s n=%d flags=%d chain %d" % (kind, n, flags, cl), pr, ref, cl)
                bad += st["priced_but_rejected"] + (faithful and not err <= 1e-9) + (st["formula_err"] > 1e-9)
                # what each kind is there for (chains of 16 are the plan the tests run on; `plain walk` here is the emulation's own)
                hard = st["hard_wide"] + st["hard_guard"] + st["hard_left"]
                priced = st["easy"] + st["empty"]
                want = {"plain": st["easy"] >= 1 and hard >= 1,
                        "straddle": st["easy"] >= 1 and max(st["ctiles"], default=0) >= 2,
                        "wide": priced == 0 and hard == st["hard_wide"] >= 1,       # every twin is hard: none can be priced
                        "null": st["empty"] >= 1,
                        "dup": st["easy"] >= 1 and hard >= 1 and st["hard_guard"] >= 1,
                        "overlap": st["easy"] >= 1}[kind]
                if not want:
                    print("    ^ %s lacks the twins it is there for" % kind)
                    bad += 1
        # the problems of tests/test_gpu_pair_routes.py, each with its purpose as a failing condition
        import test_gpu_pair_routes as tr

        def objectives(X, y, P, pats):
            Xo, Po = O.homogeneous(X, P)
            R, z = O.compress(Xo, y)
            return O.opt_patterns(R, z, Po, pats)

        # A: every instantiation T = 11 .. 16 prices twins AND sends some to the rounds
        for n, flags in tr.TILE_CASES:
            X, y, P = tp.problem("plain", n, flags)
            faithful = bool(flags & tp.FAITHFUL)
            ref = objectives(X, y, P, np.arange(1 << (tp.K + 1))) if faithful else None
            pr = prepare(np.asarray(X), y, np.asarray(P), 0.0, faithful=faithful)
            st, err = report("A plain n=%d flags=%d chain 16" % (n, flags), pr, ref, 16)
            hard = st["hard_wide"] + st["hard_guard"] + st["hard_left"]
            bad += st["priced_but_rejected"] + (faithful and not err <= 1e-9) + (st["formula_err"] > 1e-9)
            if not (st["easy"] >= 1 and hard >= 1):
                print("    ^ n=%d lacks easy or hard twins" % n)
                bad += 1
        # B: the global winner has an odd Gray index g and is priced as the twin of g - 1 in the range [g - 1, g + 1)
        for kind, n, mirror, coupling in tr.TWIN_CASES:
            X, y, P = tr.twin_problem(kind, n, mirror, coupling)
            ref = objectives(X, y, P, np.arange(1 << (tp.K + 1)))
            w = int(np.argmin(ref))
            g = tr.gray_inverse(w)
            pr = prepare(np.asarray(X), y, np.asarray(P), 0.0, faithful=True)
            st, err = report("B %s n=%d%s coupling %g: winner %d = gray(%d)" % (kind, n, " mirrored" if mirror else "", coupling, w, g),
                             pr, ref, 16, g_begin=g - 1 + (~g & 1), g_end=g + 1 + (~g & 1))
            bad += st["priced_but_rejected"] + (not err <= 1e-9) + (st["formula_err"] > 1e-9)
            if not (g & 1 and st["easy"] == 1):
                print("    ^ the winner is no priced twin (Gray index %d, %d priced)" % (g, st["easy"]))
                bad += 1
        # C: the first 256 patterns of the long enumerations on which the automatic rule turns the walk on save pivots
        for tag, n, flags, K, live, null, _ in tr.ROUTE_CASES:
            if not 12 <= live <= 16 or n > 256 or K < 17:
                continue
            X, y, P = tr.route_problem(n, flags, K, live, null)
            faithful = bool(flags & tp.FAITHFUL)
            pr = prepare(np.asarray(X), y, np.asarray(P), 0.0, faithful=faithful)
            pats = np.arange(256) ^ (np.arange(256) >> 1)
            ref = None
            if faithful:
                ref = np.full(1 << (K + 1), np.nan)
                ref[pats] = objectives(X, y, P, pats)
            st, err = report("C %s K=%d n=%d flags=%d [0, 256)" % (tag, K, n, flags), pr, ref, 16, g_end=256)
            bad += st["priced_but_rejected"] + (faithful and not err <= 1e-9) + (st["formula_err"] > 1e-9)
            if not (st["easy"] >= 1 and st["pivots"] < st["plain_pivots"]):
                print("    ^ %s: the pair walk saves no pivots" % tag)
                bad += 1
    else:
        from test_gpu_fuzz import _random_problem
        cnt = int(sys.argv[2]) if len(sys.argv) > 2 else 200
        rng = np.random.default_rng(9000)
        laid = 0
        for i in range(cnt):
            X, y, P, eta = _random_problem(rng)
            ref = O.fit_opt(X, y, P, eta=eta, return_all=True)["all_opt"]
            pr = prepare(X, y, P, eta)
            tag = "fuzz %d %s K=%d" % (i, X.shape, P.shape[1])
            if what == "static":
                width = 16 if pr["n"] > 32 else (8 if pr["n"] > 16 else 4)
                pl = relayout(pr, width)
                if pl is None:
                    print("%-28s keeps its layout (group on bit 0 wider than a tile column of %d, or one column only)" % (tag, width))
                    continue
                laid += 1
                pr, tag = pl, tag + " w=%d" % width
            st, err = report(tag, pr, ref, 16)
            # (the oracle error is reported, not checked: the fuzz draws dependent columns, whose objectives the plain walk misses as well)
            bad += st["priced_but_rejected"] + st["outside"] + (what == "static" and st["formula_err"] > 1e-9)
        if what == "static":
            print("relaid out: %d of %d problems" % (laid, cnt))
            # the tests' problems at the kernel's own tile width
            import test_gpu_pair as tp
            for kind, n, flags in tp.CASES:
                X, y, P = tp.problem(kind, n, flags)
                faithful = bool(flags & tp.FAITHFUL)
                pl = relayout(prepare(np.asarray(X), y, np.asarray(P), 0.0, faithful=faithful))
                assert (pl is None) == (kind == "wide"), kind
                if pl is None:
                    continue
                st, err = report("%s n=%d flags=%d w=16" % (kind, n, flags), pl, None, 16)
                bad += st["priced_but_rejected"] + st["outside"] + (st["formula_err"] > 1e-9)
    print("priced-but-rejected / failed checks in total: %d" % bad)
    return 1 if bad else 0


def dense_against_static(tag, pl, chain_len):
    """one problem (laid out) walked twice, priced by price_static and by price_dense: every twin's two pricings, all objectives,
    verdicts and pivot counts bit for bit; returns (failures, stats and objectives of the dense walk)"""
    out_s, st_s = pair_sweep(pl, chain_len)
    out_d, st_d = pair_sweep(dict(pl, dense=True), chain_len)
    keys = ("pivots", "easy", "empty", "hard_wide", "hard_guard", "hard_left", "capped", "rejections", "outside")
    bad = st_d["dense_diff"] + (not np.array_equal(out_s, out_d, equal_nan=True)) + any(st_s[k] != st_d[k] for k in keys)
    bad += st_d["priced_but_rejected"] + st_d["outside"] + (st_d["formula_err"] > 1e-9)
    print("%-34s chain %2d: pivots %6d  twins: dense-priced %4d easy %4d (with a gap in C %4d) empty %4d guard %3d left %3d  |C| %s  "
          "differences from the compacted pricing %d%s" % (
              tag, chain_len, st_d["pivots"], st_d["dense"], st_d["easy"], st_d["gap_easy"], st_d["empty"], st_d["hard_guard"], st_d["hard_left"],
              ("%d..%d" % (min(st_d["csize"]), max(st_d["csize"]))) if st_d["csize"] else "-", st_d["dense_diff"], "   FAILED" if bad else ""))
    return int(bad), st_d, out_d


def main_dense():
    """python tools/pair_emul.py dense [count]: the fuzz problems of `static`, the 24 problems of tests/test_gpu_pair.py and the problems
    of tests/test_gpu_pair_dense.py, each walked with the compacted and with the dense pricing (dense_against_static).  For the last
    group also what each is there for, the oracle's objectives, and the pivot counts the GPU test expects (EMUL_PIVOTS there)."""
    from oracle import oracle as O
    O.build()
    from test_gpu_fuzz import _random_problem
    import test_gpu_pair as tp
    import test_gpu_pair_dense as td
    cnt = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rng = np.random.default_rng(9000)
    bad = laid = 0
    for i in range(cnt):
        X, y, P, eta = _random_problem(rng)
        pr = prepare(X, y, P, eta)
        width = 16 if pr["n"] > 32 else (8 if pr["n"] > 16 else 4)
        pl = relayout(pr, width)
        if pl is None:
            continue
        laid += 1
        bad += dense_against_static("fuzz %d %s K=%d w=%d" % (i, X.shape, P.shape[1], width), pl, 16)[0]
    print("relaid out: %d of %d fuzz problems" % (laid, cnt))
    for kind, n, flags in tp.CASES:
        X, y, P = tp.problem(kind, n, flags)
        pl = relayout(prepare(np.asarray(X), y, np.asarray(P), 0.0, faithful=bool(flags & tp.FAITHFUL)))
        assert (pl is None) == (kind == "wide"), kind
        if pl is not None:
            bad += dense_against_static("%s n=%d flags=%d" % (kind, n, flags), pl, 16)[0]
    for kind, n in td.CASES:
        X, y, P = td.make(kind, n)
        ref = O.fit_opt(X, y, P, return_all=True)["all_opt"]
        pl = relayout(prepare(np.asarray(X), y, np.asarray(P), 0.0, faithful=True))
        assert pl is not None and pl["pair_col"][1] == 16
        for cl in (16, 7):
            b, st, got = dense_against_static("dense test: %s n=%d seed %d" % (kind, n, td.SEED[kind, n]), pl, cl)
            err = float(np.max(np.abs(got - ref) / np.maximum(1.0, ref)))
            plain = pair_sweep(pl, cl, pairing=False)[1]["pivots"]
            want = {"gaps": st["gap_easy"] >= 1, "full": max(st["csize"], default=0) == 16, "one": st["easy"] >= 1 and max(st["csize"], default=0) == 1,
                    "nine": st["easy"] >= 1, "collinear": st["hard_guard"] >= 1 and st["easy"] >= 1}[kind]
            exp = td.EMUL_PIVOTS.get((kind, n, cl))
            print("    oracle err %.2g, plain walk %d pivots, tests/test_gpu_pair_dense.py expects %s" % (err, plain, exp))
            if not (want and err <= 1e-9 and st["pivots"] < plain and exp == st["pivots"]):
                print("    ^ lacks the twins it is there for, misses the oracle, saves no pivots or the test's count is another")
                b += 1
            bad += b
    print("failed checks in total: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main_dense() if len(sys.argv) > 1 and sys.argv[1] == "dense" else main())
