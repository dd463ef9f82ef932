// near_tie_check.cpp — stand-alone driver of install_near_ties (csrc/near_tie.h), built with the sanitizers by
// tests/test_near_tie.py.  One case per input line:
//   lim2 cap winner_obj winner_pat n  obj_1 pat_1 ... obj_n pat_n        (doubles in any strtod form, hex included)
// and per case one output line:  near_for | near_pat ... | cand_obj:cand_pat ...     (doubles as %a)
#include "near_tie.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string tok;
        auto num = [&]() { in >> tok; return std::strtod(tok.c_str(), nullptr); };
        auto idx = [&]() { in >> tok; return (int64_t)std::strtoll(tok.c_str(), nullptr, 10); };
        const double lim2 = num();
        const size_t cap = (size_t)idx();
        std::pair<double, int64_t> winner;
        winner.first = num();
        winner.second = idx();
        const int64_t n = idx();
        std::vector<std::pair<double, int64_t>> others;
        for (int64_t i = 0; i < n; ++i) { const double o = num(); others.emplace_back(o, idx()); }
        if (!in) { std::fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
        // stale contents: the function must replace them
        std::vector<std::pair<double, int64_t>> cand{{-1.0, 99}, {-2.0, 98}};
        std::vector<int64_t> near_pat{7, 8, 9, 10};
        int64_t near_for = -5;
        partls::install_near_ties(winner, others, lim2, cap, cand, near_pat, near_for);
        std::printf("%lld |", (long long)near_for);
        for (int64_t q : near_pat) std::printf(" %lld", (long long)q);
        std::printf(" |");
        for (const auto &c : cand) std::printf(" %a:%lld", c.first, (long long)c.second);
        std::printf("\n");
    }
    return 0;
}
