// opt.hip — the C ABI of fit(Opt): prepare, sweep, finish, single patterns, model export and the candidate exchange of sharded sweeps.
#include "ctx.h"
#include "near_tie.h"
#include "sweep_rules.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>

namespace partls {

// fit(Opt) enumerates 2^K' patterns: beyond K' = 40 that is out of range (and of the tables of the visiting order)
static bool opt_range_ok(const partls_ctx *c, const char *who)
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

static partls_status sweep_second_pass(partls_ctx *c, int64_t g_begin, int64_t g_end, double *all_opt, double *bobj_io, int64_t *bpat_io,
                                       unsigned long long *unconv_io);

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
    if (!c->order_ready) {
        partls_status st = prepare_sweep_order(c);
        if (st != PARTLS_OK) return st;
    }
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
    const partls_status ss = ensure_sweep_scratch(c, grid);
    if (ss != PARTLS_OK) return ss;

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
    if (all_opt) {
        // only the entries of this shard are set, the others are NaN; the caller merges shards (entries are indexed by pattern)
        const void *src = c->allOpt.p;
        if (!c->order_identity) {                        // the kernel indexed it by the internal pattern
            PARTLS_HIP_CHECK(c->allOptRef.ensure((size_t)npat * sizeof(double)));
            PARTLS_HIP_CHECK(launch_pattern_gather(c->allOpt.as<double>(), npat, c->kbits, c->order, c->allOptRef.as<double>(), c->stream));
            src = c->allOptRef.p;
        }
        PARTLS_HIP_CHECK(hipMemcpyAsync(all_opt, src, (size_t)npat * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
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
        if (cnt[0]) {                                    // patterns capped: the second pass is authoritative
            const partls_status rs = sweep_second_pass(c, g_begin, g_end, all_opt, &bobj, &bpat, &cnt[0]);
            if (rs != PARTLS_OK) return rs;
        }
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
    std::vector<double> sols, obj2, w, wbest, g, gbest;
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
        if (!taken) {
            opt_codes(c, cands[ci], codes);
            st = solve_nodes(c, codes, 1, sols, obj2, &unconv, false, /*want_tab=*/true);
            if (st != PARTLS_OK) return st;
            if (unconv && rescue_on(c)) {                    // the single solve capped: Lawson-Hanson instead; no final tableau then
                st = rescue_pattern(c, cands[ci], sols, nullptr, &unconv);
                if (st != PARTLS_OK) return st;
                c->tab_valid = false;
            }
        }
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
    std::vector<double> sols, obj2, w;
    unsigned long long unconv = 0;
    std::vector<int8_t> codes;
    opt_codes(c, (uint64_t)pattern, codes);
    partls_status st = solve_nodes(c, codes, 1, sols, obj2, &unconv, false, /*want_tab=*/true);
    if (st != PARTLS_OK) return st;
    if (unconv && rescue_on(c)) {                            // the single solve capped: Lawson-Hanson instead; no final tableau then
        st = rescue_pattern(c, (uint64_t)pattern, sols, nullptr, &unconv);
        if (st != PARTLS_OK) return st;
        c->tab_valid = false;
    }
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

// Models of a Gray-index range straight from the sweep (include/partls.h).  The range is cut into pieces whose device buffers (scaled
// rows, objectives, cleaned outputs) stay below PARTLS_OPT_MODELS_PIECE_BYTES; each piece is one sweep with the export instantiation of the
// kernel, on the chain plan partls_opt_sweep would choose for it, then one launch of the cleanup kernel (models.hip), then one copy back
// through page-locked staging.  Nothing of the last partls_opt_sweep's state is touched: the counters and per-workgroup results of the
// export go to a block of their own (mdlCtr), the winner's row of bestSol stays.
static void par_rows(int64_t rows, size_t row_bytes, const std::function<void(int64_t, int64_t)> &fn)
{
    // the host copy out of the staging buffer: one core moves ~10 GB/s, a piece at C3 is ~1 GB
    const int nt = (size_t)rows * row_bytes < ((size_t)32 << 20) ? 1 : 8;
    if (nt == 1) { fn(0, rows); return; }
    std::vector<std::thread> th;
    const int64_t per = (rows + nt - 1) / nt;
    try {
        for (int i = 1; i < nt; ++i) {
            const int64_t r0 = std::min<int64_t>(rows, i * per), r1 = std::min<int64_t>(rows, r0 + per);
            th.emplace_back(fn, r0, r1);
        }
    } catch (...) {                                          // out of threads: the caller's thread takes the rest
        const int64_t done_from = (int64_t)(th.size() + 1) * per;
        fn(std::min<int64_t>(rows, done_from), rows);
    }
    fn(0, std::min<int64_t>(rows, per));
    for (std::thread &t : th) t.join();
}

static void copy_rows(double *dst, int64_t ld_dst, const double *src, int64_t width, int64_t rows)
{
    if (!dst || width <= 0) return;
    par_rows(rows, (size_t)width * sizeof(double), [&](int64_t r0, int64_t r1) {
        if (ld_dst == width) std::memcpy(dst + (size_t)r0 * width, src + (size_t)r0 * width, (size_t)(r1 - r0) * width * sizeof(double));
        else for (int64_t r = r0; r < r1; ++r) std::memcpy(dst + (size_t)r * ld_dst, src + (size_t)r * width, (size_t)width * sizeof(double));
    });
}

// What partls_opt_models and partls_opt_top share.  export_begin: the preconditions and range rules (who: the entry's name in the messages),
// g_end = -1 resolved, the counters zeroed, the device selected and the visiting order fixed; *empty: an empty range, nothing to do.
static partls_status export_begin(partls_ctx *c, const char *who, int64_t g_begin, int64_t *g_end_io, const int64_t *pattern,
                                  const double *raw_alpha, int64_t ld_raw, const double *alpha, int64_t ld_alpha, const double *beta,
                                  int64_t ld_beta, const double *t, int64_t *n_unconverged, int64_t *n_vetoes, bool *empty)
{
    if (!c || !c->prepared) { set_error("%s: context not prepared", who); return PARTLS_ERR_STATE; }
    if (!c->faithful) { set_error("%s needs a context prepared with PARTLS_OPT_FAITHFUL_INTERCEPT", who); return PARTLS_ERR_STATE; }
    if (!opt_range_ok(c, who)) return PARTLS_ERR_UNSUPPORTED;
    const int64_t npat = (int64_t)1 << c->kbits, M = c->M, K = c->K;
    int64_t g_end = *g_end_io;
    if (g_end < 0) g_end = npat;
    if (g_begin < 0 || g_begin > g_end || g_end > npat) { set_error("%s: bad Gray-index range [%lld,%lld)", who, (long long)g_begin, (long long)g_end); return PARTLS_ERR_BAD_ARG; }
    if (!pattern) { set_error("%s: pattern is NULL", who); return PARTLS_ERR_BAD_ARG; }
    if ((alpha || beta || t) && !(alpha && beta && t)) { set_error("%s: alpha, beta and t go together (all three or none)", who); return PARTLS_ERR_BAD_ARG; }
    if ((raw_alpha && ld_raw < M + 1) || (alpha && (ld_alpha < M || ld_beta < K))) { set_error("%s: leading dimension too small", who); return PARTLS_ERR_BAD_ARG; }
    if (n_unconverged) *n_unconverged = 0;
    if (n_vetoes) *n_vetoes = 0;
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    *g_end_io = g_end;
    *empty = g_begin == g_end;
    if (*empty) return PARTLS_OK;
    if (!c->order_ready) {
        partls_status st = prepare_sweep_order(c);
        if (st != PARTLS_OK) return st;
    }
    return PARTLS_OK;
}

// export_piece: one piece [p0, p0 + cnt) of the range — one sweep with the export instantiation of the kernel on sweep_plan's plan for cnt
// patterns; the scaled rows go to rows (ld n), the objectives to obj, the counters to the head of mdlCtr.  On the context's stream.
static partls_status export_piece(partls_ctx *c, int64_t p0, int64_t cnt, double *rows, double *obj, const char *who)
{
    int64_t chain_len = 0;
    int grid = 0;
    if (!sweep_plan(c, cnt, &chain_len, &grid, who)) return PARTLS_ERR_UNSUPPORTED;
    // the kernel's per-workgroup block (sweep_block without the runner-up columns): only its counters are read here
    PARTLS_HIP_CHECK(c->mdlCtr.ensure(sizeof(double) * sweep_block_words(grid, false)));
    PARTLS_HIP_CHECK(hipMemsetAsync(c->mdlCtr.p, 0, 4 * sizeof(unsigned long long), c->stream));
    const partls_status ss = ensure_sweep_scratch(c, grid);
    if (ss != PARTLS_OK) return ss;
    SweepParams p = sweep_params(c, /*internal_order=*/true);
    p.g_begin = p0; p.g_end = p0 + cnt; p.chain_len = chain_len;
    bind_sweep_block(p, c->mdlCtr.as<double>(), grid, false);
    p.node_sol = rows; p.node_obj2 = obj; p.node_ld = c->n;
    PARTLS_HIP_CHECK(launch_any_sweep(c, p, grid, /*models=*/true));
    return PARTLS_OK;
}

// patterns per piece of partls_opt_models for a range of `total` (equal pieces: no short tail piece of cold chain starts)
static int64_t models_piece(const partls_ctx *c, int64_t total)
{
    const size_t out_w = 3 + (size_t)c->M + (size_t)c->K;           // cleaned output per pattern: pattern, optval, t, alpha, beta
    const size_t per_pat = (size_t)c->n + 1 + out_w;                  // + the scaled row (raw alpha in place) and its objective
    const int64_t cap = std::max<int64_t>(1, (int64_t)(PARTLS_OPT_MODELS_PIECE_BYTES / (per_pat * sizeof(double))));
    const int64_t npieces = (total + cap - 1) / cap;
    return (total + npieces - 1) / npieces;
}

// PARTLS_OPT_RESCUE_CAPPED: the second pass of a partls_opt_sweep that reported capped patterns (the plain kernels do not say which).
// The range is walked again through the export pieces of partls_opt_models, whose NaN rows the rescue kernel solves (rescue.hip); per
// piece the four best (objective, pattern) pairs are selected on the device (topk.hip) and the host merges them.  The pass is
// authoritative: its winner and near ties are installed the way partls_opt_merge_candidates installs a merged set (no exported
// winner row: partls_opt_finish solves the winner again), all_opt holds its objectives, *unconv_io what the rescue could not solve.
static partls_status sweep_second_pass(partls_ctx *c, int64_t g_begin, int64_t g_end, double *all_opt, double *bobj_io, int64_t *bpat_io,
                                       unsigned long long *unconv_io)
{
    const auto w0 = std::chrono::steady_clock::now();
    const int n = c->n;
    const int64_t npat = (int64_t)1 << c->kbits, total = g_end - g_begin, piece = models_piece(c, total);
    const int64_t K4 = 4, kmax = std::min<int64_t>(K4, piece);
    PARTLS_HIP_CHECK(c->mdlRows.ensure((size_t)piece * (n + 1) * sizeof(double)));
    PARTLS_HIP_CHECK(c->topWork.ensure(topk_work_bytes(kmax)));
    PARTLS_HIP_CHECK(c->topRows.ensure((size_t)kmax * (n + 2) * sizeof(double)));
    PARTLS_HIP_CHECK(c->mdlStage.resize(8 + 2 * (size_t)kmax));
    if (!c->use_reg) c->coop_state_valid = false;                    // the global-memory kernels overwrite the shared tableau scratch
    std::vector<std::pair<double, int64_t>> all;
    unsigned long long unconv = 0, pivots = 0, vetoes = 0;
    for (int64_t p0 = g_begin; p0 < g_end; p0 += piece) {
        const int64_t cnt = std::min<int64_t>(piece, g_end - p0), kk = std::min<int64_t>(K4, cnt);
        double *rows = c->mdlRows.as<double>(), *obj = rows + (size_t)cnt * n;
        double *crow = c->topRows.as<double>(), *cobj = crow + (size_t)kk * n;
        int64_t *glist = reinterpret_cast<int64_t *>(cobj + kk);
        partls_status st = export_piece(c, p0, cnt, rows, obj, "partls_opt_sweep");
        if (st == PARTLS_OK) st = rescue_piece(c, p0, cnt, rows, obj);
        if (st == PARTLS_OK && all_opt) st = rescue_all_opt(c, obj, p0, cnt, c->allOpt.as<double>());
        if (st != PARTLS_OK) return st;
        PARTLS_HIP_CHECK(launch_topk_select(obj, cnt, p0, K4, c->kbits, c->order, c->order_identity, c->topWork.p, c->stream));
        PARTLS_HIP_CHECK(launch_topk_gather(rows, obj, n, p0, cnt, kk, c->topWork.p, crow, cobj, glist, c->stream));
        const TopkWork w = topk_work(c->topWork.p, kk);
        double *hs = c->mdlStage.data();
        PARTLS_HIP_CHECK(hipMemcpyAsync(hs, c->mdlCtr.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(hs + 4, c->topWork.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(hs + 8, cobj, (size_t)kk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(hs + 8 + kk, w.out_pat, (size_t)kk * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        unsigned long long cn[8];
        std::memcpy(cn, hs, sizeof(cn));
        unsigned long long left = cn[0], vet = cn[2];
        rescue_collect(c, &left, &vet);
        unconv += left; pivots += cn[1]; vetoes += vet;
        const int64_t got = (int64_t)cn[7];
        if (got < 0 || got > kk) { set_error("partls_opt_sweep: the selection reported %lld rows of at most %lld", (long long)got, (long long)kk); return PARTLS_ERR_HIP; }
        for (int64_t i = 0; i < got; ++i) {
            int64_t pat = 0;
            std::memcpy(&pat, hs + 8 + kk + i, sizeof(pat));
            all.emplace_back(hs[8 + i], pat);
        }
    }
    if (all_opt) {                                           // as the first pass returned it, with this pass's entries
        const void *src = c->allOpt.p;
        if (!c->order_identity) {
            PARTLS_HIP_CHECK(c->allOptRef.ensure((size_t)npat * sizeof(double)));
            PARTLS_HIP_CHECK(launch_pattern_gather(c->allOpt.as<double>(), npat, c->kbits, c->order, c->allOptRef.as<double>(), c->stream));
            src = c->allOptRef.p;
        }
        PARTLS_HIP_CHECK(hipMemcpyAsync(all_opt, src, (size_t)npat * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    c->last_pivots += pivots + c->rescue_pivots;
    c->last_vetoes += vetoes;
    c->sweep_vetoes += vetoes;
    c->export_wg = -1;
    c->near_pat.clear();
    c->cand.clear();
    c->near_for = -1;
    double bobj = INFINITY;
    int64_t bpat = -1;
    if (!all.empty()) {
        const std::pair<double, int64_t> win = *std::min_element(all.begin(), all.end());   // argmin's first-index rule
        bobj = win.first; bpat = win.second;
        const double yy = h_reg(c, (int)c->M + 1, (int)c->M + 1);
        const double lim2 = bobj * bobj + c->knobs.near_tie_rel * (yy > 0.0 ? yy : 0.0);
        install_near_ties(win, std::move(all), lim2, 3, c->cand, c->near_pat, c->near_for);
    }
    *bobj_io = bobj; *bpat_io = bpat; *unconv_io = unconv;
    c->ms[PARTLS_T_SWEEP] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    return PARTLS_OK;
}

partls_status partls_opt_models(partls_ctx *c, int64_t g_begin, int64_t g_end, int64_t *pattern, double *optval, double *raw_alpha,
                                int64_t ld_raw, double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t,
                                int64_t *n_unconverged, int64_t *n_vetoes)
try {
    bool empty = false;
    const partls_status bs = export_begin(c, "partls_opt_models", g_begin, &g_end, pattern, raw_alpha, ld_raw, alpha, ld_alpha, beta, ld_beta, t,
                                          n_unconverged, n_vetoes, &empty);
    if (bs != PARTLS_OK || empty) return bs;
    const int64_t M = c->M, K = c->K;
    const int n = c->n;
    const int64_t total = g_end - g_begin;
    const size_t out_w = 3 + (size_t)M + (size_t)K;                 // cleaned output per pattern: pattern, optval, t, alpha, beta
    const int64_t piece = models_piece(c, total);
    PARTLS_HIP_CHECK(c->mdlRows.ensure((size_t)piece * (n + 1) * sizeof(double)));
    PARTLS_HIP_CHECK(c->mdlOut.ensure((size_t)piece * out_w * sizeof(double)));
    const size_t stage_words = 4 + (size_t)piece * (out_w + (raw_alpha ? (size_t)n : 0));
    PARTLS_HIP_CHECK(c->mdlStage.resize(stage_words));
    if (!c->use_reg) c->coop_state_valid = false;                    // the global-memory kernels overwrite the shared tableau scratch
    const bool rescue = rescue_on(c);                                // capped rows are solved before the cleanup (rescue.hip)
    if (rescue) rescue_begin_call(c);
    unsigned long long unconv = 0, vetoes = 0;
    for (int64_t p0 = g_begin; p0 < g_end; p0 += piece) {
        const int64_t cnt = std::min<int64_t>(piece, g_end - p0);
        double *rows = c->mdlRows.as<double>(), *obj = rows + (size_t)cnt * n, *out = c->mdlOut.as<double>();
        partls_status es = export_piece(c, p0, cnt, rows, obj, "partls_opt_models");
        if (es == PARTLS_OK && rescue) es = rescue_piece(c, p0, cnt, rows, obj);
        if (es != PARTLS_OK) return es;
        PARTLS_HIP_CHECK(launch_models_cleanup(rows, obj, p0, cnt, (int)M, (int)K, c->kbits, c->order, c->order_identity, c->permP,
                                               c->scale.as<double>(), c->maskAugD.as<uint64_t>(), raw_alpha != nullptr, out, c->stream));
        double *st = c->mdlStage.data();
        PARTLS_HIP_CHECK(hipMemcpyAsync(st, c->mdlCtr.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(st + 4, out, (size_t)cnt * out_w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (raw_alpha) PARTLS_HIP_CHECK(hipMemcpyAsync(st + 4 + (size_t)cnt * out_w, rows, (size_t)cnt * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        unsigned long long cn[3];
        std::memcpy(cn, st, sizeof(cn));
        if (rescue) rescue_collect(c, &cn[0], &cn[2]);
        unconv += cn[0];
        vetoes += cn[2];
        const double *o = st + 4;
        const size_t r = (size_t)(p0 - g_begin);
        std::memcpy(pattern + r, o, (size_t)cnt * sizeof(int64_t));
        if (optval) std::memcpy(optval + r, o + cnt, (size_t)cnt * sizeof(double));
        if (t) std::memcpy(t + r, o + 2 * cnt, (size_t)cnt * sizeof(double));
        if (alpha) {
            copy_rows(alpha + r * ld_alpha, ld_alpha, o + 3 * cnt, M, cnt);
            copy_rows(beta + r * ld_beta, ld_beta, o + 3 * cnt + (size_t)cnt * M, K, cnt);
        }
        if (raw_alpha) copy_rows(raw_alpha + r * ld_raw, ld_raw, o + (size_t)cnt * out_w, M + 1, cnt);
    }
    if (n_unconverged) *n_unconverged = (int64_t)unconv;
    if (n_vetoes) *n_vetoes = (int64_t)vetoes;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

// The k best patterns of a Gray-index range (include/partls.h).  Per piece, all on the context's stream: the export
// sweep (export_piece), the selection, sort and gather of its k best rows (topk.hip), the cleanup of those rows (models.hip with the
// list of their Gray indices), one copy back.  The host keeps the k best of the pieces' lists by the same order.
static bool top_before(double oa, int64_t pa, double ob, int64_t pb) { return oa < ob || (oa == ob && pa < pb); }

partls_status partls_opt_top(partls_ctx *c, int64_t g_begin, int64_t g_end, int64_t k, int64_t *pattern, double *optval, double *raw_alpha,
                             int64_t ld_raw, double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, int64_t *count,
                             int64_t *n_unconverged, int64_t *n_vetoes)
try {
    bool empty = false;
    const partls_status bs = export_begin(c, "partls_opt_top", g_begin, &g_end, pattern, raw_alpha, ld_raw, alpha, ld_alpha, beta, ld_beta, t,
                                          n_unconverged, n_vetoes, &empty);
    if (bs != PARTLS_OK) return bs;
    if (!optval || !count) { set_error("partls_opt_top: optval or count is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (k < 1 || k > PARTLS_OPT_TOP_MAX_K) { set_error("partls_opt_top: k = %lld outside 1 .. %d", (long long)k, PARTLS_OPT_TOP_MAX_K); return PARTLS_ERR_BAD_ARG; }
    *count = 0;
    if (empty) return PARTLS_OK;
    const int64_t M = c->M, K = c->K;
    const int n = c->n;
    const int64_t total = g_end - g_begin;
    const size_t out_w = 3 + (size_t)M + (size_t)K;                 // cleaned output per selected pattern, as partls_opt_models lays it out
    int64_t cap = std::max<int64_t>(1, (int64_t)(PARTLS_OPT_MODELS_PIECE_BYTES / (((size_t)n + 1) * sizeof(double))));
    if (c->knobs.top_piece > 0) cap = (int64_t)c->knobs.top_piece;
    cap = std::min<int64_t>(cap, (int64_t)1 << 30);                   // the selection counts in 32 bits
    const int64_t npieces = (total + cap - 1) / cap;
    const int64_t piece = (total + npieces - 1) / npieces;
    const int64_t kmax = std::min<int64_t>(k, piece);                 // rows a piece can contribute
    PARTLS_HIP_CHECK(c->mdlRows.ensure((size_t)piece * (n + 1) * sizeof(double)));
    PARTLS_HIP_CHECK(c->mdlOut.ensure((size_t)kmax * out_w * sizeof(double)));
    PARTLS_HIP_CHECK(c->topWork.ensure(topk_work_bytes(kmax)));
    PARTLS_HIP_CHECK(c->topRows.ensure((size_t)kmax * (n + 2) * sizeof(double)));
    const size_t stage_words = 8 + (size_t)kmax * (out_w + (raw_alpha ? (size_t)n : 0));
    PARTLS_HIP_CHECK(c->mdlStage.resize(stage_words));
    if (!c->use_reg) c->coop_state_valid = false;                    // the global-memory kernels overwrite the shared tableau scratch
    const bool rescue = rescue_on(c);                                // capped rows are solved before the selection (rescue.hip)
    if (rescue) rescue_begin_call(c);
    unsigned long long unconv = 0, vetoes = 0;
    // the best rows so far, in order: [optval | pattern | t | alpha (M) | beta (K) | raw (n)] per row
    const size_t roww = 3 + (alpha ? (size_t)(M + K) : 0) + (raw_alpha ? (size_t)n : 0);
    std::vector<double> best, next;
    int64_t nbest = 0;
    for (int64_t p0 = g_begin; p0 < g_end; p0 += piece) {
        const int64_t cnt = std::min<int64_t>(piece, g_end - p0), kk = std::min<int64_t>(k, cnt);
        double *rows = c->mdlRows.as<double>(), *obj = rows + (size_t)cnt * n, *out = c->mdlOut.as<double>();
        double *crow = c->topRows.as<double>(), *cobj = crow + (size_t)kk * n;
        int64_t *glist = reinterpret_cast<int64_t *>(cobj + kk);
        partls_status es = export_piece(c, p0, cnt, rows, obj, "partls_opt_top");
        if (es == PARTLS_OK && rescue) es = rescue_piece(c, p0, cnt, rows, obj);
        if (es != PARTLS_OK) return es;
        PARTLS_HIP_CHECK(launch_topk_select(obj, cnt, p0, k, c->kbits, c->order, c->order_identity, c->topWork.p, c->stream));
        PARTLS_HIP_CHECK(launch_topk_gather(rows, obj, n, p0, cnt, kk, c->topWork.p, crow, cobj, glist, c->stream));
        PARTLS_HIP_CHECK(launch_models_cleanup(crow, cobj, p0, kk, (int)M, (int)K, c->kbits, c->order, c->order_identity, c->permP,
                                               c->scale.as<double>(), c->maskAugD.as<uint64_t>(), raw_alpha != nullptr, out, c->stream, glist));
        double *st = c->mdlStage.data();
        PARTLS_HIP_CHECK(hipMemcpyAsync(st, c->mdlCtr.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(st + 4, c->topWork.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(st + 8, out, (size_t)kk * out_w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (raw_alpha) PARTLS_HIP_CHECK(hipMemcpyAsync(st + 8 + (size_t)kk * out_w, crow, (size_t)kk * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        unsigned long long cn[8];
        std::memcpy(cn, st, sizeof(cn));
        if (rescue) rescue_collect(c, &cn[0], &cn[2]);
        unconv += cn[0];
        vetoes += cn[2];
        const int64_t got = (int64_t)cn[7];                          // TopState::count: min(k, converged patterns of the piece)
        if (got < 0 || got > kk) { set_error("partls_opt_top: the selection reported %lld rows of at most %lld", (long long)got, (long long)kk); return PARTLS_ERR_HIP; }
        // merge: both lists are in order; keep the first k
        const double *o = st + 8;
        const int64_t *opat = reinterpret_cast<const int64_t *>(o);
        const double *oopt = o + kk, *ot = o + 2 * kk, *oal = o + 3 * kk, *obe = oal + (size_t)kk * M, *oraw = o + (size_t)kk * out_w;
        const int64_t keep = std::min<int64_t>(k, nbest + got);
        next.resize((size_t)keep * roww);
        int64_t ia = 0, ib = 0;
        for (int64_t r = 0; r < keep; ++r) {
            double *d = next.data() + (size_t)r * roww;
            const double *a = best.data() + (size_t)ia * roww;
            int64_t apat = 0;
            if (ia < nbest) std::memcpy(&apat, a + 1, sizeof(apat));
            const bool take_a = ia < nbest && (ib >= got || top_before(a[0], apat, oopt[ib], opat[ib]));
            if (take_a) { std::memcpy(d, a, roww * sizeof(double)); ++ia; continue; }
            d[0] = oopt[ib];
            std::memcpy(d + 1, &opat[ib], sizeof(int64_t));
            d[2] = ot[ib];
            double *e = d + 3;
            if (alpha) {
                std::memcpy(e, oal + (size_t)ib * M, (size_t)M * sizeof(double));
                std::memcpy(e + M, obe + (size_t)ib * K, (size_t)K * sizeof(double));
                e += M + K;
            }
            if (raw_alpha) std::memcpy(e, oraw + (size_t)ib * n, (size_t)n * sizeof(double));
            ++ib;
        }
        best.swap(next);
        nbest = keep;
    }
    for (int64_t r = 0; r < nbest; ++r) {
        const double *d = best.data() + (size_t)r * roww, *e = d + 3;
        optval[r] = d[0];
        std::memcpy(&pattern[r], d + 1, sizeof(int64_t));
        if (alpha) {
            t[r] = d[2];
            std::memcpy(alpha + (size_t)r * ld_alpha, e, (size_t)M * sizeof(double));
            std::memcpy(beta + (size_t)r * ld_beta, e + M, (size_t)K * sizeof(double));
            e += M + K;
        }
        if (raw_alpha) std::memcpy(raw_alpha + (size_t)r * ld_raw, e, (size_t)n * sizeof(double));
    }
    *count = nbest;
    if (n_unconverged) *n_unconverged = (int64_t)unconv;
    if (n_vetoes) *n_vetoes = (int64_t)vetoes;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_opt_top_select(partls_ctx *c, const double *obj, int64_t cnt, int64_t g0, int64_t k, int64_t *index, int64_t *pattern,
                                    double *optval, int64_t *count)
try {
    if (!c || !c->prepared) { set_error("partls_opt_top_select: context not prepared"); return PARTLS_ERR_STATE; }
    if (!opt_range_ok(c, "partls_opt_top_select")) return PARTLS_ERR_UNSUPPORTED;
    if (!obj || !index || !pattern || !optval || !count) { set_error("partls_opt_top_select: NULL argument"); return PARTLS_ERR_BAD_ARG; }
    if (k < 1 || k > PARTLS_OPT_TOP_MAX_K) { set_error("partls_opt_top_select: k = %lld outside 1 .. %d", (long long)k, PARTLS_OPT_TOP_MAX_K); return PARTLS_ERR_BAD_ARG; }
    const int64_t npat = (int64_t)1 << c->kbits;
    if (cnt < 0 || cnt >= ((int64_t)1 << 31) || g0 < 0 || g0 > npat || cnt > npat - g0) { set_error("partls_opt_top_select: bad range g0 = %lld, cnt = %lld", (long long)g0, (long long)cnt); return PARTLS_ERR_BAD_ARG; }
    *count = 0;
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    if (cnt == 0) return PARTLS_OK;
    if (!c->order_ready) {
        partls_status st = prepare_sweep_order(c);
        if (st != PARTLS_OK) return st;
    }
    const int64_t kk = std::min<int64_t>(k, cnt);
    PARTLS_HIP_CHECK(c->mdlRows.ensure((size_t)cnt * sizeof(double)));
    PARTLS_HIP_CHECK(c->topWork.ensure(topk_work_bytes(kk)));
    PARTLS_HIP_CHECK(c->mdlStage.resize(4 + 2 * (size_t)kk));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->mdlRows.p, obj, (size_t)cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PARTLS_HIP_CHECK(launch_topk_select(c->mdlRows.as<double>(), cnt, g0, k, c->kbits, c->order, c->order_identity, c->topWork.p, c->stream));
    const TopkWork w = topk_work(c->topWork.p, kk);
    double *st = c->mdlStage.data();
    PARTLS_HIP_CHECK(hipMemcpyAsync(st, c->topWork.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(st + 4, w.out_idx, 2 * (size_t)kk * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));   // out_idx | out_pat
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    unsigned long long hd[4];
    std::memcpy(hd, st, sizeof(hd));
    const int64_t got = (int64_t)hd[3];
    if (got < 0 || got > kk) { set_error("partls_opt_top_select: the selection reported %lld rows of at most %lld", (long long)got, (long long)kk); return PARTLS_ERR_HIP; }
    std::memcpy(index, st + 4, (size_t)got * sizeof(int64_t));
    std::memcpy(pattern, st + 4 + kk, (size_t)got * sizeof(int64_t));
    for (int64_t i = 0; i < got; ++i) {
        if (index[i] < 0 || index[i] >= cnt) { set_error("partls_opt_top_select: selected position out of range"); return PARTLS_ERR_HIP; }
        optval[i] = obj[index[i]];
    }
    *count = got;
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
    if (!c->order_ready) {
        partls_status st = prepare_sweep_order(c);
        if (st != PARTLS_OK) return st;
    }
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
    c->near_pat.clear();
    c->cand.clear();
    if (all.empty()) { c->near_for = -1; c->export_wg = -1; if (win_obj) *win_obj = INFINITY; if (win_pattern) *win_pattern = -1; return PARTLS_OK; }
    const std::pair<double, int64_t> win = *std::min_element(all.begin(), all.end());   // lexicographic (objective, reference index): argmin's first-index rule
    const double bobj = win.first;
    const int64_t bpat = win.second;
    const double yy = h_reg(c, (int)c->M + 1, (int)c->M + 1);
    const double lim2 = bobj * bobj + c->knobs.near_tie_rel * (yy > 0.0 ? yy : 0.0);
    install_near_ties(win, std::move(all), lim2, 3, c->cand, c->near_pat, c->near_for);
    if (local_winner != bpat) c->export_wg = -1;             // the solution this rank's sweep left behind belongs to another pattern
    if (win_obj) *win_obj = bobj;
    if (win_pattern) *win_pattern = bpat;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

}  // extern "C"
