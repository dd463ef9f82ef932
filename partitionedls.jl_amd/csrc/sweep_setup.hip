// sweep_setup.hip — everything between a prepared context and a sweep launch: the shared launch parameters, the scratch rule, the
// per-workgroup result block, the choice of the kernel, the bit-order calibration, the chain plan and the node-mode solves.  Host only.
#include "ctx.h"
#include "near_tie.h"
#include "sweep_rules.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace partls {

SweepParams sweep_params(const partls_ctx *c, bool internal_order)
{
    SweepParams p{};
    const bool permuted = internal_order && !c->order_identity;
    p.n = c->n; p.kbits = c->kbits;
    p.mask = permuted ? c->maskInt.as<uint64_t>() : c->maskTabP;
    p.scratch = c->scratch.as<double>();
    p.tol = c->tol; p.piv_eps = SWEEP_PIV_EPS; p.max_rounds = c->knobs.max_rounds >= 1 ? c->knobs.max_rounds : sweep_max_rounds(c->n);
    for (int k = 0; k < 40; ++k) p.rbit.gbit[k] = (uint8_t)k;
    if (permuted) for (int k = 0; k < c->kbits; ++k) p.rbit.gbit[c->order.gbit[k]] = (uint8_t)k;   // exact ties: first REFERENCE index
    return p;
}

partls_status ensure_sweep_scratch(partls_ctx *c, int grid)
{
    const size_t ld = (size_t)c->n + 1;
    PARTLS_HIP_CHECK(c->scratch.ensure((c->use_reg ? 64 : (size_t)grid * ld * ld) * sizeof(double)));
    return PARTLS_OK;
}

partls_status node_sweep_params(partls_ctx *c, size_t nodes, int64_t chain_len, int grid, SweepParams *p)
{
    const size_t wgs = (size_t)std::max(grid, 4096);
    PARTLS_HIP_CHECK(c->bestObj.ensure(sizeof(double) * wgs));
    PARTLS_HIP_CHECK(c->bestPat.ensure(sizeof(int64_t) * wgs));
    *p = sweep_params(c, false);
    p->g_begin = 0; p->g_end = (int64_t)nodes; p->chain_len = chain_len;
    p->best_obj = c->bestObj.as<double>(); p->best_pat = c->bestPat.as<int64_t>();
    return PARTLS_OK;
}

void bind_sweep_block(SweepParams &p, double *base, int grid, bool runner_up)
{
    const SweepBlock b = sweep_block(base, grid, runner_up);
    bind_counters(p, b.counters);
    p.best_obj = b.best_obj; p.best_pat = b.best_pat;
    p.second_obj = b.second_obj; p.second_pat = b.second_pat;
}

// (bnb_bound_batch, solvers.hip, needs tableau snapshots, which the eager global-memory kernel does not keep: it is only reached when
// snapshots_supported(c), i.e. use_reg || !eager_generic, so it never gets the third kernel here)
hipError_t launch_any_sweep(partls_ctx *c, SweepParams &p, int grid, bool models)
{
    if (c->use_reg) {
        p.T0 = c->T0reg.as<double>();
        return launch_sweep_blk(p, c->T, grid, c->stream, models);
    }
    p.T0 = c->Tfull.as<double>();
    return c->knobs.eager_generic ? launch_sweep_generic(p, grid, c->stream, models) : launch_sweep_lazy(p, grid, c->stream, models);
}

void opt_codes(const partls_ctx *c, uint64_t pattern, std::vector<int8_t> &codes)
{
    // multiplier of Opt.jl:28-29: f_m = sum_k P[m,k] s_k; only its sign matters for the constraint f_m w_m >= 0 (0: column is zero)
    codes.resize((size_t)c->n);
    for (int i = 0; i < c->n; ++i) {
        const int f = sign_of_var(c->mask_tab[(size_t)i], pattern);
        codes[(size_t)i] = (int8_t)((f > 0) - (f < 0));
    }
}

partls_status solve_nodes(partls_ctx *c, const std::vector<int8_t> &codes, size_t cnt, std::vector<double> &sols,
                          std::vector<double> &obj2, unsigned long long *unconv, bool resume, bool want_tab)
{
    c->tab_valid = false;
    const int n = c->n, ld = n + 1;
    sols.assign(cnt * (size_t)n, 0.0);
    obj2.assign(cnt, 0.0);
    if (unconv) *unconv = 0;
    if (cnt == 0) return PARTLS_OK;
    if (codes.size() != cnt * (size_t)n) { set_error("solve_nodes: code array has the wrong size"); return PARTLS_ERR_BAD_ARG; }
    const int grid = (int)std::min<size_t>(cnt, c->use_reg ? 2048 : 512);
    PARTLS_HIP_CHECK(c->nodeCode.ensure(cnt * (size_t)n));
    // one output block on the device, one copy back: [counters (4 x 8 B) | objective^2 (cnt) | solutions (cnt x n)]
    const size_t out_words = 4 + cnt + cnt * (size_t)n;
    PARTLS_HIP_CHECK(c->nodeSol.ensure(out_words * sizeof(double)));
    // one large problem: many workgroups on a single global-memory tableau (sweep_coop.hip) — unless a previous attempt of this very
    // call found the device too crowded for its grid barrier (`coop_fallback`, set below)
    const bool coop = !c->use_reg && cnt == 1 && !c->knobs.no_coop && !c->coop_fallback;
    c->coop_fallback = false;
    if (coop) {
        const size_t need = ((size_t)2 * ld * ld + (size_t)n / 8 + 2) * sizeof(double);  // two tableau images + basis flags + current image
        if (c->scratch.bytes < need) c->coop_state_valid = false;
        PARTLS_HIP_CHECK(c->scratch.ensure(need));
    } else {
        c->coop_state_valid = false;
        const partls_status ss = ensure_sweep_scratch(c, grid);
        if (ss != PARTLS_OK) return ss;
    }
    PARTLS_HIP_CHECK(hipMemsetAsync(c->nodeSol.p, 0, 4 * sizeof(unsigned long long), c->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->nodeCode.p, codes.data(), cnt * (size_t)n, hipMemcpyHostToDevice, c->stream));
    SweepParams p;
    const partls_status ps = node_sweep_params(c, cnt, 1, grid, &p);
    if (ps != PARTLS_OK) return ps;
    bind_counters(p, c->nodeSol.as<unsigned long long>());
    p.node_code = c->nodeCode.as<int8_t>();
    p.node_obj2 = c->nodeSol.as<double>() + 4; p.node_sol = c->nodeSol.as<double>() + 4 + cnt; p.node_ld = n;
    // the caller will refine this one solution: have the register kernel leave its final tableau (refine_solution's solver)
    // (the cooperative kernel's tableau already lives in global memory: the current image and its basis flags are copied below)
    const bool dump_reg = want_tab && cnt == 1 && c->use_reg, dump_coop = want_tab && coop;
    const bool dump = dump_reg || dump_coop;
    const size_t tabd = dump_reg ? sweep_reg_t0_doubles(c->T) : (dump_coop ? (size_t)ld * ld : 0);
    if (dump) {
        if (dump_reg) {
            PARTLS_HIP_CHECK(c->nodeTab.ensure(tabd * sizeof(double)));
            PARTLS_HIP_CHECK(c->nodeBasic.ensure((size_t)16 * c->T));
        }
        if (c->hTabDoubles < tabd) {                                   // pinned: the 0.3 MB copy then costs ~20 us instead of ~150
            c->hTabDoubles = 0;
            PARTLS_HIP_CHECK(c->hTab.alloc(tabd));
            PARTLS_HIP_CHECK(c->hBasic.alloc(1024 + 16 /* >= 16 x MAXT of sweep_blk.hip, >= n + 1 <= 1024 flags of the cooperative kernel */));
            c->hTabDoubles = tabd;
        }
        if (dump_reg) { p.node_tab = c->nodeTab.as<double>(); p.node_basic = c->nodeBasic.as<int8_t>(); }
    }
    if (coop) {
        // one large problem: many workgroups cooperate on a single global-memory tableau (sweep_coop.hip)
        p.T0 = c->Tfull.as<double>();
        p.resume = (resume && c->coop_state_valid) ? 1 : 0;
        PARTLS_HIP_CHECK(c->gridCtr.ensure(64));
        p.grid_ctr = c->gridCtr.as<unsigned>();
        p.coop_fault = c->knobs.coop_fault;
        c->coop_state_valid = false;                                   // until this launch is known to have completed
        // 6 rows per workgroup (measured at n = 513: 0.87 / 0.81 / 0.79 / 0.85 ms per alpha-step with 16 / 8 / 6 / 4): its 16 waves take
        // half a row each in the fused update (gj_apply); more workgroups than that only lengthen the grid barrier
        const int rows_wg = c->knobs.coop_rows > 0 ? c->knobs.coop_rows : 6;
        int nwg = (ld + rows_wg - 1) / rows_wg;
        if (nwg > 128) nwg = 128;
        PARTLS_HIP_CHECK(launch_sweep_coop(p, nwg, c->stream));
    } else {
        PARTLS_HIP_CHECK(launch_any_sweep(c, p, grid));
    }
    unsigned long long counters[4] = {0, 0, 0, 0};                 // unconverged, pivots, vetoes, (cooperative kernel) blocks
    // page-locked up to 64 MB (a fit's single solves and node batches: KBs to a few MB); a caller that bounds a million nodes in one cold
    // batch gets a pageable buffer instead of gigabytes of pinned host memory
    std::vector<double> outw_big;
    double *outw_buf;
    if (out_words <= ((size_t)64 << 20) / sizeof(double)) { PARTLS_HIP_CHECK(c->nodeOut.resize(out_words)); outw_buf = c->nodeOut.data(); }
    else { outw_big.resize(out_words); outw_buf = outw_big.data(); }
    const double *outw = outw_buf;
    PARTLS_HIP_CHECK(hipMemcpyAsync(outw_buf, c->nodeSol.p, out_words * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (dump_reg) {
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->hTab, c->nodeTab.p, tabd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->hBasic, c->nodeBasic.p, (size_t)16 * c->T, hipMemcpyDeviceToHost, c->stream));
    }
    if (dump_coop) {                                               // flags [n] + index of the current tableau image, then that image
        const char *flagbuf = static_cast<const char *>(c->scratch.p) + (size_t)2 * ld * ld * sizeof(double);
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->hBasic, flagbuf, (size_t)n + 1, hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        const size_t img = (size_t)(c->hBasic[n] & 1) * ld * ld;
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->hTab, c->scratch.as<double>() + img, tabd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::memcpy(counters, outw, sizeof(counters));
    if (coop && (counters[0] >> 40)) {
        // grid-barrier timeout: some workgroups of the cooperative grid were not resident (the device is shared with another
        // context or process).  Nothing of that attempt is used; the same node is solved again by ONE workgroup, which needs no
        // co-residency (slower, never hangs).
        c->coop_fallback = true;
        return solve_nodes(c, codes, cnt, sols, obj2, unconv, false, want_tab);
    }
    if (coop) c->coop_state_valid = counters[0] == 0;
    std::copy(outw + 4, outw + 4 + cnt, obj2.begin());
    std::copy(outw + 4 + cnt, outw + out_words, sols.begin());
    if (unconv) *unconv = counters[0];
    c->last_pivots = counters[1]; c->last_vetoes = counters[2]; c->last_blocks = counters[3];
    c->tab_valid = dump && counters[0] == 0;
    c->tab_full = dump_coop;                                       // layout of hTab: full (n+1)^2 matrix, or the register kernel's tiles
    return PARTLS_OK;
}

// T0reg == nullptr: the context's own problem on whichever kernel it runs; else another problem of the same shape on the register kernel
static partls_status nodes_on_stream(partls_ctx *c, const double *T0reg, double tol, size_t cnt, const int8_t *code, double *obj2,
                                     double *sol, unsigned long long *counters, int max_rounds)
{
    c->tab_valid = false;
    c->coop_state_valid = false;
    if (cnt == 0) return PARTLS_OK;
    const int n = c->n;
    const int grid = (int)std::min<size_t>(cnt, c->use_reg ? 2048 : 512);
    SweepParams p;
    partls_status st = ensure_sweep_scratch(c, grid);
    if (st == PARTLS_OK) st = node_sweep_params(c, cnt, 1, grid, &p);
    if (st != PARTLS_OK) return st;
    p.max_rounds = max_rounds;
    bind_counters(p, counters);
    p.node_code = code; p.node_obj2 = obj2; p.node_sol = sol; p.node_ld = n;
    if (T0reg) {
        p.T0 = T0reg; p.tol = tol;
        PARTLS_HIP_CHECK(launch_sweep_blk(p, c->T, grid, c->stream));
    } else {
        PARTLS_HIP_CHECK(launch_any_sweep(c, p, grid));
    }
    return PARTLS_OK;
}

partls_status solve_nodes_device(partls_ctx *c, size_t cnt, const int8_t *code, double *obj2, double *sol,
                                 unsigned long long *counters, int max_rounds)
{
    return nodes_on_stream(c, nullptr, 0.0, cnt, code, obj2, sol, counters, max_rounds);
}

partls_status solve_nodes_device_at(partls_ctx *c, const double *T0reg, double tol, size_t cnt, const int8_t *code, double *obj2,
                                    double *sol, unsigned long long *counters, int max_rounds)
{
    if (!c->use_reg || !T0reg) { set_error("solve_nodes_device_at: needs a register-kernel context and a tableau"); return PARTLS_ERR_STATE; }
    return nodes_on_stream(c, T0reg, tol, cnt, code, obj2, sol, counters, max_rounds);
}

}  // namespace partls

using namespace partls;

// Which group sits on which bit of the Gray index.  Bit b flips in 2^-(b+1) of all transitions and a flip exchanges roughly the
// variables of its group that carry signal, so the cheap groups belong on the fast bits: on C3 the reference's order (group k on
// bit k) costs 16.9 M pivots / 74.9 ms, the measured-cost order 13.2 M / 51.0 ms for the same 2^20 subproblems.  The cost of a flip
// is MEASURED on the prepared problem: `ncu` chains of nodes on the kernel the sweep will use, chain c solving a pseudo-random pattern from
// scratch and then flipping the groups of its half of the bits one after the other (each node warm-started from its predecessor,
// exactly as in the sweep); pivots per flip are averaged per group.  Wall time = one chain = (8 + K'/2) patterns' worth, paid once
// per prepare and only when the sweep is long enough to repay it.  Deterministic (fixed walks, no atomics in the solves), so every
// rank of a sharded sweep derives the same order from the same data; dist.py cross-checks that before trusting the shards.
partls_status partls::calibrate_bit_order(partls_ctx *c)
{
    const int kb = c->kbits, n = c->n;
    c->order_ready = true;
    c->order_identity = true;
    c->flip_cost.clear();
    for (int k = 0; k < 40; ++k) c->order.gbit[k] = (uint8_t)k;
    if (kb < 2 || c->knobs.bit_order == 1) return PARTLS_OK;
    const int ncu = c->ncu;
    const int nseg = kb >= 8 ? 2 : 1;
    const int seg_len = (kb + nseg - 1) / nseg, L = seg_len + 1;
    // one calibration chain costs about (8 + seg_len) patterns (8: the solve from scratch); the sweep gives every CU 2^kb / ncu of them.
    // What it buys depends on the data (nothing when the groups cost the same, a third of the sweep on C3): run it when it costs <= 3 %
    if (c->knobs.bit_order != 2 && ((int64_t)1 << kb) < (int64_t)ncu * 32 * (8 + seg_len)) return PARTLS_OK;
    const int chains = std::max(ncu - ncu % nseg, 2 * nseg);
    const size_t steps = (size_t)chains * L;

    PARTLS_HIP_CHECK(c->nodeCode.ensure(steps * (size_t)n));
    PARTLS_HIP_CHECK(c->nodePiv.ensure((3 * steps + 8) * sizeof(unsigned)));
    PARTLS_HIP_CHECK(c->nodeSol.ensure((4 + (size_t)chains + (size_t)chains * n) * sizeof(double)));
    SweepParams p;
    partls_status st = ensure_sweep_scratch(c, chains);
    if (st == PARTLS_OK) st = node_sweep_params(c, steps, L, chains, &p);
    if (st != PARTLS_OK) return st;
    PARTLS_HIP_CHECK(hipMemsetAsync(c->nodePiv.p, 0, 8 * sizeof(unsigned), c->stream));          // [unconverged (8 B) | ... | pivots per step]
    t_begin(c, PARTLS_T_CALIB);
    PARTLS_HIP_CHECK(launch_walk_codes(c->maskTabP, n, kb, chains, L, seg_len, nseg, c->nodeCode.as<int8_t>(), c->stream));
    p.n_unconverged = c->nodePiv.as<unsigned long long>();
    p.node_code = c->nodeCode.as<int8_t>();
    p.node_obj2 = c->nodeSol.as<double>() + 4; p.node_sol = c->nodeSol.as<double>() + 4 + chains; p.node_ld = n;
    p.node_piv = c->nodePiv.as<unsigned>() + 8;                    // 3 counters per step
    PARTLS_HIP_CHECK(launch_any_sweep(c, p, chains));
    t_end(c, PARTLS_T_CALIB);
    std::vector<unsigned> piv(3 * steps + 8);
    PARTLS_HIP_CHECK(hipMemcpyAsync(piv.data(), c->nodePiv.p, (3 * steps + 8) * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    t_collect(c);
    c->coop_state_valid = false;
    c->tab_valid = false;
    unsigned long long unconv = 0;
    std::memcpy(&unconv, piv.data(), sizeof(unconv));
    if (unconv) return PARTLS_OK;                            // a walk hit the pivot cap: the sample says nothing, keep the plain order

    // Cost of a flip in pivot equivalents.  On the register kernel a pattern's cycles split (stamp build) into ~730 + 4.4 NS
    // per pivot (panel step + update; NS = tile slots), ~4 400 per block pivot (gather, scatter, the update's start, barrier waits) and
    // ~2 100 per KKT scan beyond the first, which every pattern pays: a group whose variables straddle tile columns so that a flip takes
    // three blocks instead of two costs as much more as four extra pivots would.  All three counts are exact (no timing), so the
    // order stays a deterministic function of the data.
    const double ns = c->use_reg ? 0.5 * c->T * (c->T + 1) : 0.0;
    const double per_pivot = 730.0 + 4.4 * ns;
    const double w_block = c->use_reg ? c->knobs.cal_wb * 4400.0 / per_pivot : 0.0, w_scan = c->use_reg ? c->knobs.cal_ws * 2100.0 / per_pivot : 0.0;
    std::vector<double> cost((size_t)kb, 0.0);
    std::vector<int> cnt((size_t)kb, 0);
    for (int ch = 0; ch < chains; ++ch)
        for (int i = 1; i < L; ++i) {
            const int k = walk_flipped_bit(ch, i, kb, seg_len, nseg);
            const unsigned *now = &piv[8 + 3 * ((size_t)ch * L + i)], *was = now - 3;
            const double scans = (double)(now[2] - was[2]);
            cost[(size_t)k] += (double)(now[0] - was[0]) + w_block * (double)(now[1] - was[1]) + w_scan * (scans > 1.0 ? scans - 1.0 : 0.0);
            ++cnt[(size_t)k];
        }
    for (int k = 0; k < kb; ++k) cost[(size_t)k] = cnt[(size_t)k] ? cost[(size_t)k] / cnt[(size_t)k] : 0.0;
    std::vector<int> by_cost((size_t)kb);
    std::iota(by_cost.begin(), by_cost.end(), 0);
    std::stable_sort(by_cost.begin(), by_cost.end(), [&](int a, int b) { return cost[(size_t)a] < cost[(size_t)b]; });
    c->flip_cost = cost;
    // pivots per pattern the additive model predicts: sum_b 2^-(b+1) cost(group on bit b).  Sorting noisy estimates of equal costs always
    // "predicts" a gain of about their standard error (~1 %): below 2 % the reference's order stays (measured on such problems: +-1 %)
    double pred_ref = 0.0, pred_sorted = 0.0, wgt = 0.5;
    for (int b = 0; b < kb; ++b, wgt *= 0.5) { pred_ref += wgt * cost[(size_t)b]; pred_sorted += wgt * cost[(size_t)by_cost[(size_t)b]]; }
    if (c->knobs.bit_order != 2 && !(pred_sorted < 0.98 * pred_ref)) return PARTLS_OK;
    bool ident = true;
    for (int b = 0; b < kb; ++b) { c->order.gbit[by_cost[(size_t)b]] = (uint8_t)b; ident = ident && by_cost[(size_t)b] == b; }
    if (ident) return PARTLS_OK;
    std::vector<uint64_t> mi((size_t)n);
    for (int i = 0; i < n; ++i) {
        uint64_t m = c->mask_tab[(size_t)i], q = 0;
        for (; m; m &= m - 1) q |= 1ULL << c->order.gbit[__builtin_ctzll(m)];
        mi[(size_t)i] = q;
    }
    PARTLS_HIP_CHECK(c->maskInt.ensure((size_t)n * sizeof(uint64_t)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->maskInt.p, mi.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));     // `mi` is pageable and goes out of scope
    c->order_identity = false;
    return PARTLS_OK;
}

// internal pattern (group k on bit gbit[k]) -> the reference's pattern index (group k on bit k)
int64_t partls::reference_pattern(const partls_ctx *c, int64_t q)
{
    if (q < 0 || c->order_identity) return q;
    uint64_t r = 0;
    for (int k = 0; k < c->kbits; ++k) r |= (((uint64_t)q >> c->order.gbit[k]) & 1ULL) << k;
    return (int64_t)r;
}

// The pair walk (sweep_blk.hip, PAIR) runs on the 512-thread register kernel up to T = 16.  PARTLS_PAIR forces it off or on; left alone it
// is on where all of this holds:
//   * the bit-order calibration's length rule (calibrate_bit_order: K' >= 18 on 256 CUs) — the enumerations whose cheapest group sits on
//     bit 0 and that are long enough for the walk to matter; short ones keep the plain walk and their pivot counts;
//   * the range itself gives every CU 32 patterns or more: a short range of a long enumeration (partls_opt_models' companion sweeps,
//     whose winner is promised bit for bit among the export's rows: include/partls.h) keeps the plain walk;
//   * the group on bit 0 has 12..16 live variables.  A heuristic fitted to the two long enumerations the benchmark has, one each: with 12
//     (C3, K = 20) the walk gains 4.1 % (sweep 47.61 -> 45.65 ms), with 10 (C5, K = 24) it LOSES 3.3 % (669.2 -> 691.6 ms with the walk
//     forced) — pricing a twin (a scan, a gather pass through the block body, the solve on one wave, the rows, a scan: ~16k cycles in
//     the stamp build) costs about what 10 pivots in two block pivots cost (profiles/pair_ab_c3.txt).  Nothing between 10 and 12 was
//     measured; the rule stays on the side that was seen to win.  (With the static pricing column the forced walk wins on C5 as well,
//     586.9 against 679.4 ms — profiles/pair_static_ab_c3.txt §4; the bound is still 12 because tests/test_gpu_pair_routes.py pins it.)
//   * the kernel prices a twin from ONE tile column, so even the forced walk needs that group's live variables to fit one: with more
//     than 16 the walk is off whatever PARTLS_PAIR says (every twin went to the rounds there anyway).
// pair_rule is the rule; sweep_pairs also asks that the group has been laid into the pair column (pair_relayout).
// is tableau variable i a live variable of the group on Gray bit 0?
static bool on_bit0(const partls_ctx *c, int i)
{
    if (c->hScale[(size_t)i] == 0.0) return false;
    for (int k = 0; k < c->kbits; ++k)
        if (c->order.gbit[k] == 0 && ((c->mask_tab[(size_t)i] >> k) & 1ULL)) return true;
    return false;
}

static bool pair_rule(const partls_ctx *c, int64_t total)
{
    if (!c->use_reg || sweep_reg_small(c->T) || c->T > 16 || c->knobs.pair == 0) return false;
    int live = 0;
    for (int i = 0; i < c->n; ++i) live += on_bit0(c, i);
    if (live > 16) return false;
    if (c->knobs.pair == 1) return true;
    const int kb = c->kbits, seg_len = (kb + (kb >= 8 ? 2 : 1) - 1) / (kb >= 8 ? 2 : 1);
    if (kb < 2 || ((int64_t)1 << kb) < (int64_t)c->ncu * 32 * (8 + seg_len) || total < (int64_t)c->ncu * 32) return false;
    return live >= 12;
}

bool partls::sweep_pairs(const partls_ctx *c, int64_t total) { return c->pair_laid && pair_rule(c, total); }

// The pair column is tile column T - 2, not the last one: the last column holds n - 16 (T - 1) variables, as few as one, while T - 2 is
// full at every n of its tile count.  The new order: the other variables in their present order up to the pair column, then the group's
// live variables, then the other variables that fill the column, then the rest — the relative order of everything outside the group is
// kept (tools/layout_probe.py: the order of the other groups moves the sweep by +- 3 %).  scale and the tableau are functions of
// (perm[i], perm[j]) alone, so the kernels that rebuild them give a permutation of the former entries bit for bit and the host copy of the
// scale is permuted here instead of read back: no sync.  The calibrated order, the flip costs and dist.order_key's key were derived
// from the data before this and do not change.
partls_status partls::pair_relayout(partls_ctx *c)
{
    if (c->pair_laid || !pair_rule(c, (int64_t)1 << c->kbits)) return PARTLS_OK;
    const int n = c->n, base = 16 * (c->T - 2);
    std::vector<int> grp, oth, idx;
    for (int i = 0; i < n; ++i) (on_bit0(c, i) ? grp : oth).push_back(i);
    idx.assign(oth.begin(), oth.begin() + base);            // n >= 16 (T - 1) + 1 and at most 16 in the group: the others reach the column
    idx.insert(idx.end(), grp.begin(), grp.end());
    idx.insert(idx.end(), oth.begin() + base, oth.end());
    c->pair_laid = true;
    bool same = true;
    for (int i = 0; i < n; ++i) same = same && idx[(size_t)i] == i;
    if (same) return PARTLS_OK;
    std::vector<int> perm((size_t)n);
    std::vector<double> sc((size_t)n);
    for (int i = 0; i < n; ++i) { perm[(size_t)i] = c->perm[(size_t)idx[(size_t)i]]; sc[(size_t)i] = c->hScale[(size_t)idx[(size_t)i]]; }
    c->perm = perm;
    std::memcpy(c->hScale.data(), sc.data(), (size_t)n * sizeof(double));
    const partls_status st = ctx_layout_tableau(c, /*timed=*/false);
    if (st != PARTLS_OK) return st;
    if (!c->order_identity) {                               // the group masks in the internal bit order, as calibrate_bit_order builds them
        c->mask_int_host.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            uint64_t m = c->mask_tab[(size_t)i], q = 0;
            for (; m; m &= m - 1) q |= 1ULL << c->order.gbit[__builtin_ctzll(m)];
            c->mask_int_host[(size_t)i] = q;
        }
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->maskInt.p, c->mask_int_host.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    }
    c->coop_state_valid = false;
    c->tab_valid = false;
    return PARTLS_OK;
}

partls_status partls::prepare_sweep_order(partls_ctx *c)
{
    if (c->order_ready) return PARTLS_OK;
    const partls_status st = calibrate_bit_order(c);
    return st != PARTLS_OK ? st : pair_relayout(c);
}

// Chain length and grid of a sweep over `total` Gray indices (partls_opt_sweep; partls_opt_models per piece: the same plan for the same
// range, so its rows carry the objectives all_opt gets).  false (error set): the range needs more than 2^31 chains.
bool partls::sweep_plan(partls_ctx *c, int64_t total, int64_t *chain_len_out, int *grid_out, const char *who)
{
    // Chain length.  A chain start costs ~8 patterns' pivots, so chains should be long (~1024 patterns), but the register kernel runs ONE
    // chain per CU at a time and the chains of a range take almost equally long: the sweep lasts ceil(chains / CUs) chain times, and a
    // chain count that is not a multiple of the CU count pays for the whole last round (measured on C3, 256 CUs: 1024 chains of 1024
    // patterns 74.9 ms, 768 of 1366 75.1, but 820 of 1280 90.6 and 1366 of 768 81.5).  So: a whole number k >= 2 of chains per CU.
    int64_t chain_len;
    if (c->knobs.chain_len > 0) chain_len = c->knobs.chain_len;
    else if (c->use_reg) {
        const int ncu = c->ncu;
        // ~1024 patterns per chain; 2048 once that still leaves every CU 8 or more chains to balance with (C5, 2^24 patterns: 690.6 ->
        // 686.7 ms; 4096: 686.6, 8192: 689.8)
        const int64_t per_chain = total >= (int64_t)ncu * 2048 * 8 ? 2048 : 1024;
        const int conc = sweep_reg_concurrency(c->T);           // chains a CU runs at once: 1, or the 256-thread kernel's occupancy
        if (conc > 1) {
            // small tableaus: `slots` chains run at the same time, so a short enumeration is cut into exactly that many chains — down to
            // 4 patterns each: a chain start costs about 8 patterns' pivots, but an idle slot costs a whole chain (BASELINE config 2, 4096
            // patterns on 256 x 3 slots: 683 chains of 6 instead of 256 of 16)
            const int64_t slots = (int64_t)ncu * conc;
            const int64_t k = std::max<int64_t>(1, (total + slots * per_chain - 1) / (slots * per_chain));
            chain_len = std::max<int64_t>(4, (total + k * slots - 1) / (k * slots));
        } else {
        int64_t k = (total + (int64_t)ncu * per_chain - 1) / ((int64_t)ncu * per_chain);
        if (k < 2) k = 2;
        chain_len = (total + k * ncu - 1) / (k * ncu);
        if (chain_len < 16) chain_len = 16;                     // tiny ranges: fewer chains than CUs rather than chains of a few patterns
        }
    } else {
        // global-memory kernels (n > 320): a chain start costs ~n/2 pivots (the first pattern is solved from the empty basis) against ~25 per
        // warm-started pattern, so chains are as long as still leaves every CU one (measured at D = 340, 2^16 / 2^18 patterns: 64 -> 3.79 /
        // 4.17 M solves/s, 128 -> 3.90 / 4.37, 256 -> 4.01 / 4.46)
        const int ncu = c->ncu;
        chain_len = 256;
        while (chain_len > 16 && (total + chain_len - 1) / chain_len < ncu) chain_len >>= 1;
    }
    if (chain_len < 1) chain_len = 1;
    // pair walk: chains of even length (an odd one leaves a pattern without its partner at every chain end: solved the ordinary way).
    // A range with an odd g_begin keeps such end patterns; PARTLS_CHAIN_LEN is taken as given.
    if (c->knobs.chain_len <= 0 && sweep_pairs(c, total)) chain_len += chain_len & 1;
    const int64_t nchains = (total + chain_len - 1) / chain_len;
    if (nchains >= (1LL << 31) || chain_len >= (1LL << 31)) { set_error("%s: more than 2^31 chains in one call; split the Gray-index range", who); return false; }
    int grid = (int)std::min<int64_t>(nchains, c->knobs.grid > 0 ? c->knobs.grid : (c->use_reg ? 4096 : 1024));
    if (grid < 1) grid = 1;
    *chain_len_out = chain_len;
    *grid_out = grid;
    return true;
}

// The host half of a sweep: counters, winner and near ties from the per-workgroup block the kernel left (sweep_out: the host copy of a
// sweep_block with runner-up columns).  Installs what partls_opt_finish reads: export_wg (has_sol: the kernel wrote bestSol), near_for,
// near_pat, cand.  partls_opt_sweep and the batched sweep of partls_cv_opt (cv.hip, one block per problem) share it.
void partls::install_sweep_result(partls_ctx *c, const double *sweep_out, int grid, bool has_sol, double *bobj_out, int64_t *bpat_out)
{
    const SweepBlock b = sweep_block(const_cast<double *>(sweep_out), grid, true);     // read only
    c->last_pivots = b.counters[1];
    c->last_vetoes = b.counters[2];
    c->sweep_vetoes = b.counters[2];
    c->export_wg = -1;
    std::vector<int64_t> bp((size_t)grid);
    double bobj = INFINITY;
    int64_t bpat = -1;
    int best_wg = -1;
    for (int i = 0; i < grid; ++i) {                     // argmin with first-index tie-break (Opt.jl:96)
        bp[(size_t)i] = reference_pattern(c, b.best_pat[i]);
        if (bp[(size_t)i] < 0) continue;
        if (bpat < 0 || b.best_obj[i] < bobj || (b.best_obj[i] == bobj && bp[(size_t)i] < bpat)) { bobj = b.best_obj[i]; bpat = bp[(size_t)i]; best_wg = i; }
    }
    if (has_sol) c->export_wg = best_wg;                 // row of bestSol that holds the winner's solution (valid while near_for == winner)
    // Near ties: each workgroup reports its minimum and its runner-up; partls_opt_finish re-ranks those install_candidates keeps.
    std::vector<std::pair<double, int64_t>> others;
    if (bpat >= 0) for (int i = 0; i < grid; ++i) {
        if (bp[(size_t)i] >= 0) others.emplace_back(b.best_obj[i], bp[(size_t)i]);
        if (b.second_pat[i] >= 0) others.emplace_back(b.second_obj[i], reference_pattern(c, b.second_pat[i]));
    }
    install_candidates(c, {bobj, bpat}, std::move(others));
    *bobj_out = bobj;
    *bpat_out = bpat;
}

// The ONE install of a winner (pattern -1: none) and its near ties: of `others` those within near_tie_rel y'y of the winner's
// objective^2 are kept, at most 3, best first (near_tie.h).  Replaces cand, near_pat and near_for; export_wg is the caller's.
void partls::install_candidates(partls_ctx *c, std::pair<double, int64_t> winner, std::vector<std::pair<double, int64_t>> others)
{
    c->near_pat.clear();
    c->cand.clear();
    c->near_for = -1;
    if (winner.second < 0) return;
    const double yy = h_reg(c, (int)c->M + 1, (int)c->M + 1);
    const double lim2 = winner.first * winner.first + c->knobs.near_tie_rel * (yy > 0.0 ? yy : 0.0);
    install_near_ties(winner, std::move(others), lim2, 3, c->cand, c->near_pat, c->near_for);
}

// all_opt of a sweep (c->allOpt, indexed by the internal pattern) to the host under the reference index: queued on c->stream, no wait
partls_status partls::deliver_all_opt(partls_ctx *c, double *all_opt)
{
    const int64_t npat = (int64_t)1 << c->kbits;
    const void *src = c->allOpt.p;
    if (!c->order_identity) {
        PARTLS_HIP_CHECK(c->allOptRef.ensure((size_t)npat * sizeof(double)));
        PARTLS_HIP_CHECK(launch_pattern_gather(c->allOpt.as<double>(), npat, c->kbits, c->order, c->allOptRef.as<double>(), c->stream));
        src = c->allOptRef.p;
    }
    PARTLS_HIP_CHECK(hipMemcpyAsync(all_opt, src, (size_t)npat * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return PARTLS_OK;
}
