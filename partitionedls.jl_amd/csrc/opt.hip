// opt.hip — the C ABI of fit(Opt): prepare, sweep, finish, single patterns, bit order, the candidate exchange (export: opt_export.hip).
#include "ctx.h"
#include "sweep_rules.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace partls {

// fit(Opt) enumerates 2^K' patterns: beyond K' = 40 that is out of range (and of the tables of the visiting order)
bool opt_range_ok(const partls_ctx *c, const char *who)
{
    if (c->kbits <= 40) return true;
    set_error("%s: %d sign bits: the enumeration of 2^(K+1) patterns is out of range (K <= 39); fit(Alt) and fit(BnB) take up to 61 groups", who, c->kbits);
    return false;
}

// cleanupResult (Opt.jl:34-44) from w = f∘α: raw α_m = w_m / f_m, raw β_k = s_k
static void cleanup_opt(const partls_ctx *c, const std::vector<double> &w, uint64_t pattern, double *alpha, double *beta, double *t)
{
    const int64_t M = c->M, K = c->K;
    std::vector<double> a((size_t)M, 0.0);
    for (int64_t m = 0; m < M; ++m) {
        const int f = sign_of_var(c->mask_aug[(size_t)m], pattern);
        a[(size_t)m] = (f != 0) ? w[(size_t)m] / (double)f : 0.0;
        if (a[(size_t)m] < 0.0) a[(size_t)m] = 0.0;      // round-off guard: nonneg_lsq never returns negatives
    }
    std::vector<double> A((size_t)K, 0.0);
    for (int64_t k = 0; k < K; ++k) {
        double s = 0.0;
        for (int64_t m = 0; m < M; ++m) s += (double)c->P[(size_t)m + (size_t)k * M] * a[(size_t)m];
        const double sk = ((pattern >> k) & 1ULL) ? 1.0 : -1.0;
        beta[k] = sk * s;
        A[(size_t)k] = (s == 0.0) ? 1.0 : s;
    }
    for (int64_t m = 0; m < M; ++m) {
        double s = 0.0;
        for (int64_t k = 0; k < K; ++k) s += (double)c->P[(size_t)m + (size_t)k * M] * a[(size_t)m] / A[(size_t)k];
        alpha[m] = s;
    }
    *t = w[(size_t)M];                                   // t = β[end]*α[end] = f_I α_I = w_I (Opt.jl:92)
}

// One reference pattern solved from the fresh tableau (sols: n scaled values, the final tableau kept for the refinement), by
// Lawson-Hanson when that solve hit the pivot cap and the context rescues (no final tableau then); *unconv: it is still unsolved.
static partls_status solve_pattern(partls_ctx *c, uint64_t pattern, std::vector<double> &sols, unsigned long long *unconv)
{
    std::vector<int8_t> codes;
    std::vector<double> obj2;
    opt_codes(c, pattern, codes);
    partls_status st = solve_nodes(c, codes, 1, sols, obj2, unconv, false, /*want_tab=*/true);
    if (st == PARTLS_OK && *unconv && rescue_on(c)) {
        st = rescue_pattern(c, pattern, sols, nullptr, unconv);
        c->tab_valid = false;
    }
    return st;
}

}  // namespace partls

using namespace partls;

extern "C" {

partls_status partls_opt_prepare(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                 int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta, uint32_t flags)
try {
    return ctx_prepare(c, X, N, M, ldX, y, x_on_device, P, K, ldP, eta, (flags & PARTLS_OPT_FAITHFUL_INTERCEPT) != 0, flags);
}
PARTLS_ABI_GUARD

partls_status partls_opt_prepare_weighted(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                          const double *w, int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta,
                                          uint32_t flags)
try {
    return ctx_prepare(c, X, N, M, ldX, y, x_on_device, P, K, ldP, eta, (flags & PARTLS_OPT_FAITHFUL_INTERCEPT) != 0, flags, w);
}
PARTLS_ABI_GUARD

partls_status partls_opt_prepare_f32(partls_ctx *c, const float *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w,
                                     int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta, uint32_t flags)
try {
    return ctx_prepare(c, X, N, M, ldX, y, x_on_device, P, K, ldP, eta, (flags & PARTLS_OPT_FAITHFUL_INTERCEPT) != 0, flags, w, /*x_f32=*/true);
}
PARTLS_ABI_GUARD

partls_status partls_opt_prepare_csr(partls_ctx *c, const int64_t *indptr, const int32_t *indices, const double *values, int64_t N, int64_t M,
                                     const double *y, const double *w, int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta,
                                     uint32_t flags)
try {
    return ctx_prepare_csr(c, indptr, indices, values, N, M, y, w, x_on_device, P, K, ldP, eta, (flags & PARTLS_OPT_FAITHFUL_INTERCEPT) != 0, flags);
}
PARTLS_ABI_GUARD

int64_t partls_opt_num_patterns(const partls_ctx *c) { return (c && c->prepared && c->kbits <= 40) ? ((int64_t)1 << c->kbits) : 0; }

partls_status partls_opt_sweep(partls_ctx *c, int64_t g_begin, int64_t g_end, double *best_obj, int64_t *best_pattern,
                               double *all_opt, int64_t *n_unconverged)
try {
    if (!c || !c->prepared) { set_error("partls_opt_sweep: context not prepared"); return PARTLS_ERR_STATE; }
    if (!opt_range_ok(c, "partls_opt_sweep")) return PARTLS_ERR_UNSUPPORTED;
    const int64_t npat = (int64_t)1 << c->kbits;
    if (g_end < 0) g_end = npat;
    if (g_begin < 0 || g_begin > g_end || g_end > npat) { set_error("bad Gray-index range [%lld,%lld)", (long long)g_begin, (long long)g_end); return PARTLS_ERR_BAD_ARG; }
    if (all_opt && !c->faithful) { set_error("all_opt needs PARTLS_OPT_FAITHFUL_INTERCEPT"); return PARTLS_ERR_BAD_ARG; }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    if (g_begin == g_end) {
        if (best_obj) *best_obj = INFINITY;
        if (best_pattern) *best_pattern = -1;
        if (n_unconverged) *n_unconverged = 0;
        return PARTLS_OK;
    }
    PARTLS_CHECK(prepare_sweep_order(c));
    const int n = c->n;
    const int64_t total = g_end - g_begin;
    int64_t chain_len = 0;
    int grid = 0;
    if (!sweep_plan(c, total, &chain_len, &grid, "partls_opt_sweep")) return PARTLS_ERR_UNSUPPORTED;

    // one output block on the device, one copy back (sweep_block, with the runner-up columns)
    const size_t sweep_words = sweep_block_words(grid, true);
    PARTLS_HIP_CHECK(c->bestObj.ensure(sizeof(double) * sweep_block_words(std::max(grid, 4096), true)));
    PARTLS_HIP_CHECK(hipMemsetAsync(c->bestObj.p, 0, 4 * sizeof(unsigned long long), c->stream));
    if (all_opt) {
        PARTLS_HIP_CHECK(c->allOpt.ensure((size_t)npat * sizeof(double)));
        if (total < npat) PARTLS_HIP_CHECK(hipMemsetAsync(c->allOpt.p, 0xFF, (size_t)npat * sizeof(double), c->stream));   // NaN outside the shard
    }
    PARTLS_CHECK(ensure_sweep_scratch(c, grid));

    SweepParams p = sweep_params(c, /*internal_order=*/true);
    p.g_begin = g_begin; p.g_end = g_end; p.chain_len = chain_len;
    p.pair = sweep_pairs(c, total) ? 1 : 0;
    p.all_opt = all_opt ? c->allOpt.as<double>() : nullptr;
    bind_sweep_block(p, c->bestObj.as<double>(), grid, true);
    if (!c->use_reg && c->knobs.lz_fault) p.coop_fault = 77;   // test hook of the deferred-update kernel's panel (SweepParams::coop_fault)
    // the register kernels leave the solution of every workgroup's best pattern behind: partls_opt_finish starts from the winner's
    // instead of solving that pattern again from the empty basis (C2: 89 us of a 0.58 ms fit)
    c->export_wg = -1;
    // (the 256-thread register kernel for small tableaus and the deferred-update kernel beyond n = 320; not the 512-thread kernel)
    if (((c->use_reg && (sweep_reg_small(c->T) || sweep_reg_exports(c->T))) || (!c->use_reg && !c->knobs.eager_generic)) && !c->knobs.no_export) {
        PARTLS_HIP_CHECK(c->bestSol.ensure((size_t)grid * n * sizeof(double)));
        p.best_sol = c->bestSol.as<double>();
        p.node_ld = n;
    }

    t_begin(c, PARTLS_T_SWEEP);
    PARTLS_HIP_CHECK(launch_any_sweep(c, p, grid));
    t_end(c, PARTLS_T_SWEEP);

    unsigned long long cnt[3] = {0, 0, 0};
    PARTLS_HIP_CHECK(c->sweepOut.resize(sweep_words));
    const double *sweep_out = c->sweepOut.data();
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->sweepOut.data(), c->bestObj.p, sweep_words * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    // only the entries of this shard are set, the others are NaN; the caller merges shards (entries are indexed by pattern)
    if (all_opt) PARTLS_CHECK(deliver_all_opt(c, all_opt));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    t_collect(c);
    std::memcpy(cnt, sweep_out, sizeof(cnt));
    if (c->knobs.print_stamps) {                         // diagnostic build (-DPARTLS_STAMPS): phase shares of workgroup 0
        double st[32] = {0};
        if (hipMemcpy(st, c->scratch.p, sizeof(st), hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "[partls stamps] scan: pre %.0f barrier %.0f post %.0f | gather: work %.0f barrier %.0f | panel: work %.0f barrier %.0f | "
                            "update %.0f | scatter %.0f | chain-load %.0f/%.0f | pivots %llu || gather split: block setup %.0f chain %.0f rhs/myj %.0f"
                            " || workgroup 0: %.0f blocks, %.0f scans, %.0f pivots || pair walk: twin scan %.0f, solve + rows + scan %.0f"
                            " = solve prologue %.0f steps %.0f (both on the solving wave only: PARTLS_STAMP_TID=192) barrier behind the solve %.0f"
                            " rows %.0f verdict %.0f\n",
                    st[9], st[10], st[0], st[12] + st[13] + st[8], st[1], st[11], st[2], st[3], st[4], st[5], st[6], cnt[1], st[12], st[13], st[8],
                    st[24], st[25], st[26], st[15], st[16] + st[17] + st[18] + st[19] + st[20], st[16], st[17], st[18], st[19], st[20]);
    }
    double bobj = INFINITY;
    int64_t bpat = -1;
    install_sweep_result(c, sweep_out, grid, p.best_sol != nullptr, &bobj, &bpat);
    if (rescue_on(c)) {
        rescue_begin_call(c);
        // patterns capped: the second pass is authoritative
        if (cnt[0]) PARTLS_CHECK(sweep_second_pass(c, g_begin, g_end, all_opt, &bobj, &bpat, &cnt[0]));
    }
    if (best_obj) *best_obj = bobj;
    if (best_pattern) *best_pattern = bpat;
    if (n_unconverged) *n_unconverged = (int64_t)cnt[0];
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_opt_finish(partls_ctx *c, int64_t pattern, double *alpha, double *beta, double *t, double *opt,
                                int64_t *best_index)
try {
    if (!c || !c->prepared) { set_error("partls_opt_finish: context not prepared"); return PARTLS_ERR_STATE; }
    if (!alpha || !beta || !t || !opt) { set_error("partls_opt_finish: NULL output"); return PARTLS_ERR_BAD_ARG; }
    if (pattern < 0 || pattern >= ((int64_t)1 << (c->K + 1))) { set_error("pattern out of range"); return PARTLS_ERR_BAD_ARG; }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    const uint64_t kmask = ((uint64_t)1 << c->kbits) - 1;
    // A group without any feature leaves the subproblem unchanged: the reference then sees bitwise equal objectives for the two
    // patterns and argmin keeps the first, i.e. the one with that group's bit clear (Opt.jl:96)
    // — and so does a group whose every feature is a null column (scale 0: never in a basis; the reference's X .* f' has +-0 columns)
    uint64_t used = 1ULL << c->K;
    for (int i = 0; i < c->n; ++i) if (c->hScale[(size_t)i] != 0.0) used |= c->mask_tab[(size_t)i];

    // candidates: the given pattern and, when it is the winner of this context's last sweep, the near ties that sweep recorded —
    // distinct subproblems only (patterns that differ in the bits of unused groups are the same subproblem)
    std::vector<uint64_t> cands{(uint64_t)pattern & kmask & used};
    if (pattern == c->near_for)
        for (int64_t q : c->near_pat) {
            const uint64_t v = (uint64_t)q & kmask & used;
            if (std::find(cands.begin(), cands.end(), v) == cands.end()) cands.push_back(v);
        }
    const int export_wg = (pattern == c->near_for) ? c->export_wg : -1;   // the sweep's winner: its solution was left behind by the kernel
    c->export_wg = -1;
    c->near_for = -1;
    c->near_pat.clear();
    c->last_near_evaluated = (int64_t)cands.size();

    t_begin(c, PARTLS_T_FINISH);
    const auto f0 = std::chrono::steady_clock::now();
    std::vector<double> sols, w, wbest, g, gbest;
    std::vector<int8_t> codes;
    unsigned long long unconv = 0, unconv_best = 0;
    double obest = INFINITY, loo_best = 0.0;
    uint64_t pbest = cands[0];
    for (size_t ci = 0; ci < cands.size(); ++ci) {
        partls_status st = PARTLS_OK;
        bool taken = false;
        if (ci == 0 && export_wg >= 0) {
            // the winner's solution as the sweep left it (scaled, 0 for nonbasic variables — the format of a node solve); accepted when
            // it carries the winning pattern's signs (on an exact objective tie the kernel keeps the FIRST pattern's solution, which
            // may belong to the other pattern of the tie), refined and KKT-checked below like any other
            PARTLS_HIP_CHECK(c->exportSol.resize((size_t)c->n));
            PARTLS_HIP_CHECK(hipMemcpyAsync(c->exportSol.data(), c->bestSol.as<double>() + (size_t)export_wg * c->n, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
            sols.assign(c->exportSol.data(), c->exportSol.data() + c->n);
            opt_codes(c, cands[ci], codes);
            taken = true;
            double smax = 0.0;
            for (int i = 0; i < c->n; ++i) smax = std::max(smax, std::fabs(sols[(size_t)i]));
            for (int i = 0; i < c->n && taken; ++i) {
                const double v = sols[(size_t)i];
                if (!std::isfinite(v)) taken = false;
                else if (v != 0.0 && (codes[(size_t)i] == 0 || (codes[(size_t)i] == 1 && v < -1e-9 * smax) || (codes[(size_t)i] == -1 && v > 1e-9 * smax))) taken = false;
            }
            if (taken) { c->tab_valid = false; unconv = 0; }
            if (c->knobs.finish_trace) fprintf(stderr, "[finish] the sweep's solution of its winner (workgroup %d): %s\n", export_wg, taken ? "taken" : "refused (signs), solving again");
        }
        if (!taken) PARTLS_CHECK(solve_pattern(c, cands[ci], sols, &unconv));
        unscale_solution(c, sols.data(), w);
        RefineOut ro;
        st = refine_solution(c, w, !c->faithful, 2, &ro); // QR-level accuracy of the winner on ill-conditioned data
        if (st != PARTLS_OK) return st;
        double o = 0.0;
        // Opt.jl:90 from the data, and Xo'(yo - Xo w) for the KKT check below: left by the refinement's last pass when it converged
        if (ro.have) { o = ro.obj; g.swap(ro.g); }
        else { st = data_objective(c, w, &o, &g); if (st != PARTLS_OK) return st; }
        if (c->knobs.finish_trace && cands.size() > 1) fprintf(stderr, "[finish] near tie: pattern %llu data objective %.17g\n", (unsigned long long)cands[ci], o);
        // argmin over the data objectives, first reference index on exact ties (Opt.jl:96)
        if (ci == 0 || o < obest || (o == obest && cands[ci] < pbest)) { obest = o; pbest = cands[ci]; wbest = w; gbest = g; unconv_best = unconv; loo_best = c->last_min_loo; }
    }
    const auto f1 = std::chrono::steady_clock::now();
    uint64_t full = pbest;
    if (!c->faithful) { if (wbest[(size_t)c->M] > 0.0) full |= (1ULL << c->K); }     // first-index tie-break when t == 0
    full &= used;
    // data-space KKT conditions of the winner, every variable — including those the leave-one-out rule kept out of the basis
    std::vector<int8_t> vcode((size_t)c->M + 1, 0);
    for (int64_t m = 0; m <= c->M; ++m) {
        if (m == c->M && !c->faithful) { vcode[(size_t)m] = 2; continue; }          // free intercept
        const int f = sign_of_var(c->mask_aug[(size_t)m], full);
        vcode[(size_t)m] = (int8_t)((f > 0) - (f < 0));
    }
    int worst = -1;
    c->last_kkt = kkt_violation_data(c, wbest, gbest, vcode, &worst);
    *opt = obest;
    if (c->knobs.finish_trace) {
        const auto f2 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[finish] %zu candidate(s): solve + refine + data objective / gradient %.3f ms, KKT check %.3f ms; data-space KKT violation %.3e (variable %d)\n",
                cands.size(), ms(f0, f1), ms(f1, f2), c->last_kkt, worst);
    }
    t_end(c, PARTLS_T_FINISH);
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    t_collect(c);
    cleanup_opt(c, wbest, full, alpha, beta, t);
    if (best_index) *best_index = (int64_t)full;
    if (unconv_best) { set_error("winner re-solve hit the pivot cap"); return PARTLS_ERR_NOT_CONVERGED; }
    c->last_min_loo = loo_best;
    if (kkt_says_ill_conditioned(c)) {
        set_error("the winner's KKT conditions do not hold in data space (violation %.2e of ||x|| ||y|| at variable %d, tolerance %.1e; %llu columns "
                  "refused as dependent in the sweep): X is too ill-conditioned for the fp64 Gram form (cond(X) >~ 1e6); the outputs hold the best "
                  "Gram-form model", c->last_kkt, worst, c->knobs.kkt_tol, c->sweep_vetoes);
        return PARTLS_ERR_ILL_CONDITIONED;
    }
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_opt_pattern(partls_ctx *c, int64_t pattern, double *raw_alpha, double *optval)
try {
    if (!c || !c->prepared) { set_error("partls_opt_pattern: context not prepared"); return PARTLS_ERR_STATE; }
    if (!c->faithful) { set_error("partls_opt_pattern needs a context prepared with PARTLS_OPT_FAITHFUL_INTERCEPT"); return PARTLS_ERR_STATE; }
    if (pattern < 0 || pattern >= ((int64_t)1 << c->kbits)) { set_error("pattern out of range"); return PARTLS_ERR_BAD_ARG; }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    std::vector<double> sols, w;
    unsigned long long unconv = 0;
    partls_status st = solve_pattern(c, (uint64_t)pattern, sols, &unconv);
    if (st != PARTLS_OK) return st;
    unscale_solution(c, sols.data(), w);
    st = refine_solution(c, w, false);
    if (st != PARTLS_OK) return st;
    if (optval) { st = data_objective(c, w, optval); if (st != PARTLS_OK) return st; }
    if (raw_alpha)
        for (int64_t m = 0; m <= c->M; ++m) {
            const int f = sign_of_var(c->mask_aug[(size_t)m], (uint64_t)pattern);
            const double a = (f != 0) ? w[(size_t)m] / (double)f : 0.0;
            raw_alpha[m] = a > 0.0 ? a : 0.0;
        }
    if (unconv) { set_error("pattern solve hit the pivot cap"); return PARTLS_ERR_NOT_CONVERGED; }
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_fit_opt(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                             const int64_t *P, int64_t K, int64_t ldP, double eta, uint32_t flags,
                             double *alpha, double *beta, double *t, double *opt, int64_t *best_index, double *all_opt)
try {
    if (all_opt) flags |= PARTLS_OPT_FAITHFUL_INTERCEPT;
    partls_status st = partls_opt_prepare(c, X, N, M, ldX, y, 0, P, K, ldP, eta, flags);
    if (st != PARTLS_OK) return st;
    double bobj; int64_t bpat, unconv;
    st = partls_opt_sweep(c, 0, -1, &bobj, &bpat, all_opt, &unconv);
    if (st != PARTLS_OK) return st;
    if (bpat < 0) { set_error("sweep produced no candidate"); return PARTLS_ERR_NOT_CONVERGED; }
    st = partls_opt_finish(c, bpat, alpha, beta, t, opt, best_index);
    if (st != PARTLS_OK) return st;
    if (unconv) { set_error("%lld subproblems hit the pivot cap", (long long)unconv); return PARTLS_ERR_NOT_CONVERGED; }
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_opt_bit_order(partls_ctx *c, int64_t *gbit, double *flip_cost)
try {
    if (!c || !c->prepared) { set_error("partls_opt_bit_order: context not prepared"); return PARTLS_ERR_STATE; }
    if (!gbit) { set_error("partls_opt_bit_order: gbit is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (!opt_range_ok(c, "partls_opt_bit_order")) return PARTLS_ERR_UNSUPPORTED;
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    PARTLS_CHECK(prepare_sweep_order(c));
    for (int k = 0; k < c->kbits; ++k) {
        gbit[k] = c->order.gbit[k];
        if (flip_cost) flip_cost[k] = c->flip_cost.empty() ? -1.0 : c->flip_cost[(size_t)k];
    }
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

// ---- near ties across shards -------------------------------------------------------------------------------------------------------
// A sharded enumeration (partls_fit_opt_multi's rank threads, dist.py's processes) must re-rank the SAME candidate set a single context
// would (Opt.jl:90,96: every objective from the data, first index on ties): each shard hands out its winner and its near ties with
// their tracked objectives, the lists of all shards are concatenated in rank order, and every rank installs the merged set.
partls_status partls_opt_candidates(const partls_ctx *c, int64_t capacity, double *obj, int64_t *pattern, int64_t *count)
try {
    if (!c || !c->prepared || !count || capacity < 0 || (capacity > 0 && (!obj || !pattern))) { set_error("partls_opt_candidates: bad argument"); return PARTLS_ERR_BAD_ARG; }
    const int64_t n = std::min<int64_t>(capacity, (int64_t)c->cand.size());
    for (int64_t i = 0; i < n; ++i) { obj[i] = c->cand[(size_t)i].first; pattern[i] = c->cand[(size_t)i].second; }
    *count = n;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_opt_merge_candidates(partls_ctx *c, int64_t count, const double *obj, const int64_t *pattern, double *win_obj, int64_t *win_pattern)
try {
    if (!c || !c->prepared || count < 0 || (count > 0 && (!obj || !pattern))) { set_error("partls_opt_merge_candidates: bad argument"); return PARTLS_ERR_BAD_ARG; }
    std::vector<std::pair<double, int64_t>> all;
    for (int64_t i = 0; i < count; ++i) if (pattern[i] >= 0 && obj[i] == obj[i]) all.emplace_back(obj[i], pattern[i]);
    const int64_t local_winner = c->cand.empty() ? -1 : c->cand[0].second;
    std::pair<double, int64_t> win{INFINITY, -1};
    if (!all.empty()) win = *std::min_element(all.begin(), all.end());   // lexicographic (objective, reference index): argmin's first-index rule
    install_candidates(c, win, std::move(all));
    if (local_winner != win.second || win.second < 0) c->export_wg = -1;   // the solution this rank's sweep left behind belongs to another pattern
    if (win_obj) *win_obj = win.first;
    if (win_pattern) *win_pattern = win.second;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

}  // extern "C"
