// sweep_rules.h — the per-pattern decisions of the four tableau kernels (sweep_blk.hip, sweep_lazy.hip, sweep_generic.hip,
// sweep_coop.hip), defined here.  DESIGN.md §4 promises that the kernels take the same decisions and agree up to rounding; what a
// kernel keeps to itself is only where its tableau lives and how a block of pivots is applied to it.  Here:
//   sign_of_var   the multiplier f_m of Opt.jl:28-29 from a group mask and a pattern;
//   kkt_violates  which variables violate KKT for a pattern (or a node's codes), given the rhs column;
//   ExchangeRule  which of the violators a round exchanges: all of them, or, once the count has stopped falling for three rounds, the
//                 largest only (Kim & Park's finite-termination backup), and when a pattern gives up (the pivot cap);
//   rank_pattern  the running (objective, pattern) minimum with its runner-up and the reference-index rule for exact ties;
//   rcp_newton, readlane_f64   the two arithmetic helpers every panel shares.
// Only sweep_generic.hip, the tests' reference, is built from all of these definitions.  The three production kernels take sign_of_var,
// rcp_newton, readlane_f64 (and coop: gj_panel.h's violator_list) from here but keep HAND-WRITTEN COPIES of the decision rules, because
// through the helpers their device code moves (profiles/sweep_rules_resource_usage.txt), each marked "(sweep_rules.h), written out":
//   sweep_blk.hip   sweep_body: the KKT scan — where the merged scan is compiled (MERGED) written out TWICE in the same scan, once under the pattern's signs and once
//                   under its successor's with no column rejected (the merged scan: `bad` and `nxt`) —, the round's exchange, with the
//                   first round of a pattern that starts from its predecessor's confirming scan set up next to it (ninf_best = count2,
//                   rounds = 1), and the ranking at the end of a pattern (finish_pattern, on objective^2 in LDS, its own form);
//   sweep_lazy.hip  sweep_lazy_kernel: the KKT scan, the exchange and the ranking;
//   sweep_coop.hip  sweep_coop_kernel: the KKT scan and the exchange (a single solve ranks nothing).
// A change to kkt_violates, ExchangeRule or rank_pattern is made here AND in those places (ten with the merged scan's two; the pair walk of
// sweep_blk.hip adds kkt_violates twice more, under the twin's signs: the scan for its violators and the scan of its priced rhs column, and
// the ranking once more: record_twin, the bookkeeping of a priced twin).
// tests/test_gpu_exchange_rule.py runs every copy of ExchangeRule against tests/exchange_reference.py, decision for decision.
#pragma once
#include "common.h"

namespace partls {

// f = sum_k P[v,k] * s_k with s_k = +1 if bit k of pat else -1  ==  2*popc(m & pat) - popc(m)
__host__ __device__ __forceinline__ int sign_of_var(uint64_t m, uint64_t pat)
{
    return 2 * __builtin_popcountll(m & pat) - __builtin_popcountll(m);
}

// Does a variable violate KKT?  q: its entry of the rhs column (w_i when basic, (c - G w)_i when not).  code: the sign the pattern asks of
// it — chain mode passes f = sign_of_var (only its sign counts; |f| = 2: a feature of two groups), node mode the node's code -1, 0, +1 or
// 2 = free (stationarity only).  NODE = false (chain mode) compiles no `free` test.  blocked: rejected as dependent on the current basis.
template <bool NODE>
__device__ __forceinline__ bool kkt_violates(int code, double q, bool basic, bool blocked, double tol)
{
    const bool isfree = NODE && code == 2;
    const int f = isfree ? 0 : code;
    const double fq = q * (double)(f > 1 ? 1 : (f < -1 ? -1 : f));     // sign(f) * q
    if (isfree) return !basic && !blocked && (fabs(q) > tol);
    if (basic) return (f == 0) || (fq < -tol);
    return (fq > tol) && !blocked;
}

// Block principal pivoting with Kim & Park's backup rule, one instance per pattern.  The order of the tests is part of the rule: a
// converged scan never counts as a round, and the patience is spent before the cap is looked at.
struct ExchangeRule {
    enum Step { CONVERGED, ALL, LARGEST, CAPPED };     // exchange ALL violators / the LARGEST (index) only / CAPPED: max_rounds reached
    int ninf_best, patience, rounds;
    __device__ __forceinline__ explicit ExchangeRule(int n) : ninf_best(n + 1), patience(3), rounds(0) {}
    __device__ __forceinline__ Step next(int count, int max_rounds)
    {
        if (count == 0) return CONVERGED;
        bool all;
        if (count < ninf_best) { ninf_best = count; patience = 3; all = true; }
        else if (patience > 0) { --patience; all = true; }
        else all = false;
        if (++rounds > max_rounds) return CAPPED;
        return all ? ALL : LARGEST;
    }
};

// lexicographic (objective, pattern) minimum with its runner-up (near-tie re-rank on the host); exact ties go to the pattern that comes
// first in the reference's visiting order (argmin's first-index rule) — for the runner-up as for the minimum, so that the two are the two
// smallest (objective, reference index) pairs whatever the order of the visits (the pair walk visits in another order than the plain
// walk, and partls_opt_candidates lists the same patterns after both).  (Works on copies and stores all four once: conditional stores
// through the references end up as one store to a selected address, which keeps the caller's variables in scratch memory.)
__device__ __forceinline__ void rank_pattern(double obj, uint64_t pat, double &best_obj, long long &best_pat, double &second_obj,
                                             long long &second_pat, const unsigned char *rbit)
{
    double bo = best_obj, so = second_obj;
    long long bp = best_pat, sp = second_pat;
    if (obj < bo || (obj == bo && bp >= 0 && ref_index_less(pat, (unsigned long long)bp, rbit))) {
        so = bo; sp = bp;
        bo = obj; bp = (long long)pat;
    } else if (obj < so || (obj == so && sp >= 0 && ref_index_less(pat, (unsigned long long)sp, rbit))) { so = obj; sp = (long long)pat; }
    best_obj = bo; best_pat = bp; second_obj = so; second_pat = sp;
}

__device__ __forceinline__ double rcp_newton(double d)       // v_rcp_f64 + two Newton steps: ~1 ulp
{
    double y = __builtin_amdgcn_rcp(d);
    y = fma(fma(-d, y, 1.0), y, y);
    y = fma(fma(-d, y, 1.0), y, y);
    return y;
}

__device__ __forceinline__ double readlane_f64(double v, int lane)      // lane: wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

}  // namespace partls
