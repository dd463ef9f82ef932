// near_tie.h — the near-tie rule of the Opt sweep, once.  Standard library only (no HIP): the stand-alone test program includes it as is.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace partls {

// Winner = lexicographic minimum of (objective, reference pattern index): argmin's first-index rule (Opt.jl:96); the caller found it.
// The tracked objective^2 carries the Gram form's absolute error (a few eps * y'y, growing about as the square root of the chain length:
// DESIGN.md §3), so two patterns closer than that can come out in the wrong order relative to the reference, which computes every
// objective from the data (Opt.jl:90).  Of `others` (objective, reference pattern; any order, duplicates and the winner itself allowed)
// those with another pattern than the winner's whose objective^2 is <= lim2 are kept, at most `cap` of them, best first.
// Installs what partls_opt_finish re-ranks with the objective from the data: near_for = the winner's pattern, near_pat = the kept
// patterns, cand = winner first, then the kept pairs (what the ranks of a sharded enumeration exchange).
inline void install_near_ties(std::pair<double, int64_t> winner, std::vector<std::pair<double, int64_t>> others, double lim2, size_t cap,
                              std::vector<std::pair<double, int64_t>> &cand, std::vector<int64_t> &near_pat, int64_t &near_for)
{
    others.erase(std::remove_if(others.begin(), others.end(), [&](const std::pair<double, int64_t> &o) {
                     return o.second == winner.second || !(o.first * o.first <= lim2);
                 }), others.end());
    std::sort(others.begin(), others.end());                  // lexicographic (objective, reference index)
    others.erase(std::unique(others.begin(), others.end()), others.end());
    if (others.size() > cap) others.resize(cap);
    near_for = winner.second;
    near_pat.clear();
    cand.assign(1, winner);
    for (const std::pair<double, int64_t> &o : others) { near_pat.push_back(o.second); cand.push_back(o); }
}

}  // namespace partls
