"""CPU checks of the k-best-patterns entries (partls_opt_top, partls_opt_top_select) against the fake library of
tools/api_call_trace.py: the header, the ctypes table, the trace tool's table and the Julia patch agree; fit(..., top=k) refuses bad
arguments before any call, makes the calls it documents in their order, and rebuilds the listed models through partls_opt_finish when
the sweep reports vetoes; dist.merge_top and TopPatterns on hand-made lists."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import api_call_trace as T  # noqa: E402
import check_julia_binding as CJ  # noqa: E402

X = np.array([[1., 2, 3], [3, 3, 4], [8, 1, 3], [5, 3, 1], [2, 7, 1], [4, 4, 9]])
Y = np.array([1., 1, 2, 3, 2, 5])
P = np.array([[1, 0], [1, 0], [0, 1]])


def _symbols(lines):
    return [ln.split("(")[0] for ln in lines if not ln.startswith(("#", "raised", "warned"))]


def test_header_tables_and_julia_patch_agree(partls):
    protos = CJ.parse_header()
    table = {name: args for name, _, args in partls.lowlevel.SYMBOLS}
    want = {"partls_opt_top": ["partls_ctx*", "int64_t", "int64_t", "int64_t", "int64_t*", "double*", "double*", "int64_t", "double*",
                               "int64_t", "double*", "int64_t", "double*", "int64_t*", "int64_t*", "int64_t*"],
            "partls_opt_top_select": ["partls_ctx*", "double*", "int64_t", "int64_t", "int64_t", "int64_t*", "int64_t*", "double*",
                                      "int64_t*"]}
    for name, params in want.items():
        assert protos[name] == ("partls_status", params), name
        assert len(table[name]) == len(T.SPEC[name].split()) == len(params), name
    text = open(os.path.join(ROOT, "include", "partls.h")).read()
    assert int(re.search(r"#define PARTLS_OPT_TOP_MAX_K (\d+)", text).group(1)) == partls.lowlevel.OPT_TOP_MAX_K == 4096
    assert partls.lowlevel.lib().partls_version() >= 106
    assert "TopPatterns" in partls.__all__ and partls.TopPatterns is partls.api.TopPatterns
    assert "partls_opt_top" in {c[0] for c in CJ.parse_ccalls()} and "partls_opt_top" in {s for s, _ in CJ.check()}


def test_argument_errors_come_before_any_call(partls):
    api = partls.api
    with T.fake_library(api) as fake:
        for bad in (0, -1, partls.lowlevel.OPT_TOP_MAX_K + 1, 2.0, "3", True):
            with pytest.raises(ValueError):
                api.fit(api.Opt, X, Y, P, top=bad)
        for alg in (api.Alt, api.BnB):
            with pytest.raises(ValueError):
                api.fit(alg, X, Y, P, top=3)
        with pytest.raises(NotImplementedError):
            api.fit(api.Opt, X, Y, P, top=3, devices=[0, 0])
        assert fake.lines == []


def test_call_sequence_of_fit_with_top(partls):
    api = partls.api
    with T.fake_library(api) as fake:
        model, _, rep = api.fit(api.Opt, X, Y, P, top=3)
        calls = [ln for ln in fake.lines if ln.startswith("partls_opt")]
        assert _symbols(calls) == ["partls_opt_prepare", "partls_opt_sweep", "partls_opt_finish", "partls_opt_top"]
        assert calls[0].split(") -> ")[0].endswith("flags=1")                 # the faithful enumeration, forced by top=
        assert "g_begin=0, g_end=-1, k=3," in calls[3] and "ld_raw=4" in calls[3] and "ld_alpha=3" in calls[3] and "ld_beta=2" in calls[3]
        top = rep.top
        assert isinstance(top, api.TopPatterns) and len(top) == 3 and top.n_vetoes == 0
        assert top.pattern.tolist() == [0, 1, 2] and top.alpha.shape == (3, 3) and top.beta.shape == (3, 2) and len(top.models) == 3
        assert "opt" in rep and "best_index" in rep
        # with the float32 X, weights and returnAllSolutions: the staged prepares, then the same tail
        for kw, first in ((dict(weights=np.arange(1.0, 7.0)), "partls_opt_prepare_weighted"), (dict(returnAllSolutions=True), "partls_opt_prepare")):
            del fake.lines[:]
            _, _, rep = api.fit(api.Opt, X, Y, P, top=2, **kw)
            seq = [s for s in _symbols(fake.lines) if s.startswith("partls_opt") and s != "partls_opt_num_patterns"]   # (want_all sizes all_opt by it)
            assert seq == [first, "partls_opt_sweep", "partls_opt_finish", "partls_opt_top"]
            assert len(rep.top) == 2 and ("solutions" in rep) == ("returnAllSolutions" in kw)
        del fake.lines[:]
        api.fit(api.Opt, X.astype(np.float32), Y, P, top=2)
        assert _symbols([ln for ln in fake.lines if ln.startswith("partls_opt")])[0] == "partls_opt_prepare_f32"
        # k beyond the patterns of the problem: the list is as long as the library says
        _, _, rep = api.fit(api.Opt, X, Y, P, top=100)
        assert len(rep.top) == 8
        # no top=: no call, no field
        del fake.lines[:]
        _, _, rep = api.fit(api.Opt, X, Y, P)
        assert "partls_opt_top" not in _symbols(fake.lines) and "top" not in rep


def test_vetoes_rebuild_the_models_through_opt_finish(partls):
    api = partls.api
    with T.fake_library(api) as fake:
        fake.top_vetoes = 5
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter("always")
            _, _, rep = api.fit(api.Opt, X, Y, P, top=3)
        assert [w.category for w in ws] == [api.IllConditionedWarning]
        calls = [ln for ln in fake.lines if ln.startswith("partls_opt")]
        assert _symbols(calls) == ["partls_opt_prepare", "partls_opt_sweep", "partls_opt_finish", "partls_opt_top"] + ["partls_opt_finish"] * 3
        assert [c.split("pattern=")[1].split(",")[0] for c in calls[4:]] == ["0", "1", "2"]        # the ranking is kept
        assert rep.top.n_vetoes == 5 and rep.top.pattern.tolist() == [0, 1, 2]
        # a scripted pivot cap: ERR_NOT_CONVERGED, as fit reports it
        inner = fake.partls_opt_top

        def capped(*args):
            st = inner(*args)
            args[14]._obj.value = 2
            return st
        fake.partls_opt_top = capped
        with pytest.raises(api.PartlsError) as ei:
            api.fit(api.Opt, X, Y, P, top=3)
        assert ei.value.status == partls.lowlevel.ERR_NOT_CONVERGED


def test_context_bindings_trim_to_count(partls):
    api = partls.api
    with T.fake_library(api) as fake:
        ctx = api.Context(0)
        ctx.opt_prepare(X, Y, P, 0.0, 1)
        r = ctx.opt_top(5, 2, 6, raw=True)
        assert r["count"] == 4 and all(len(r[k]) == 4 for k in ("pattern", "opt", "alpha", "beta", "t", "raw_alpha"))
        assert r["raw_alpha"].shape == (4, 4)
        assert "raw_alpha" not in ctx.opt_top(5)
        idx, pat, val = ctx.opt_top_select(np.array([3.0, 1.0, 2.0]), 1, 2)
        assert len(idx) == len(pat) == len(val) == 0                          # the fake selects nothing
        assert fake.lines[-1].startswith("partls_opt_top_select(c1, obj[3]=") and "cnt=3, g0=1, k=2" in fake.lines[-1]


def _shard(pattern, opt, M=2, K=2, raw=False, **counts):
    pattern = np.asarray(pattern, dtype=np.int64)
    n = len(pattern)
    r = dict(pattern=pattern, opt=np.asarray(opt, dtype=np.float64), alpha=np.repeat(pattern[:, None], M, 1) * 1.0,
             beta=np.repeat(pattern[:, None], K, 1) * -1.0, t=pattern * 10.0, count=n, n_unconverged=0, n_vetoes=0)
    if raw:
        r["raw_alpha"] = np.repeat(pattern[:, None], M + 1, 1) * 0.5
    r.update(counts)
    return r


def test_merge_top_orders_ties_across_shards(partls):
    merge = partls.dist.merge_top
    a = _shard([7, 2, 9], [1.0, 2.0, 2.0], raw=True, n_vetoes=1)
    b = _shard([3, 1, 12], [-0.0, 2.0, np.inf], raw=True, n_unconverged=2)
    c = _shard([5], [0.0], raw=True)
    m = merge([a, b, c], 6)
    # -0.0 and +0.0 tie: pattern 3 before 5; the three 2.0s by pattern across the shards
    assert m["pattern"].tolist() == [3, 5, 7, 1, 2, 9] and m["count"] == 6
    assert m["opt"].tolist() == [0.0, 0.0, 1.0, 2.0, 2.0, 2.0]
    assert np.array_equal(m["t"], m["pattern"] * 10.0) and np.array_equal(m["alpha"][:, 0], m["pattern"] * 1.0)
    assert np.array_equal(m["raw_alpha"][:, 2], m["pattern"] * 0.5)
    assert m["n_vetoes"] == 1 and m["n_unconverged"] == 2
    assert merge([a, b, c], 100)["pattern"].tolist() == [3, 5, 7, 1, 2, 9, 12]          # +inf is an ordinary value, last
    assert merge([a, b, c], 1)["pattern"].tolist() == [3]
    assert "raw_alpha" not in merge([a, _shard([4], [0.5])], 2)
    assert merge([_shard([], []), c], 3)["pattern"].tolist() == [5]
    for lists, k in (([a], 0), ([], 2)):
        with pytest.raises(ValueError):
            merge(lists, k)


def test_top_patterns_views(partls):
    TP, Fit = partls.TopPatterns, partls.PartLSFitResult
    K = 2                                                                      # patterns have 3 bits: bit 2 is the intercept's
    pattern = np.array([5, 1, 6, 2, 3], dtype=np.int64)                         # group patterns 1, 1, 2, 2, 3
    opt = np.array([1.0, 1.5, 1.5, 4.0, 7.0])
    beta = np.array([[1.0, -2.0], [1.0, -1.0], [-3.0, 0.0], [-1.0, 2.0], [0.5, 2.0]])
    alpha = np.arange(15.0).reshape(5, 3)
    t = np.arange(5.0)
    top = TP(pattern, opt, alpha, beta, t, [Fit(alpha[i], beta[i], t[i], P) for i in range(5)], 0)
    assert len(top) == 5
    assert np.array_equal(top.gap, opt[1:] - opt[0])
    want = np.stack([(beta < 0).mean(0), (beta == 0).mean(0), (beta > 0).mean(0)], axis=1)
    assert top.sign_agreement.shape == (K, 3) and np.array_equal(top.sign_agreement, want)
    assert np.allclose(top.sign_agreement.sum(1), 1.0)
    g = top.group_patterns()
    assert g.pattern.tolist() == [1, 2, 3] and g.opt.tolist() == [1.0, 1.5, 7.0]  # the better of each pair, the order kept
    assert np.array_equal(g.alpha, alpha[[0, 2, 4]]) and np.array_equal(g.beta, beta[[0, 2, 4]]) and g.t.tolist() == [0.0, 2.0, 4.0]
    assert [m.t for m in g.models] == [0.0, 2.0, 4.0]
    empty = TP(pattern[:0], opt[:0], alpha[:0], beta[:0], t[:0], [], 0)
    assert len(empty.gap) == 0 and np.isnan(empty.sign_agreement).all() and len(empty.group_patterns()) == 0
