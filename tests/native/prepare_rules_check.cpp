// prepare_rules_check.cpp — stand-alone driver of the prepare path's host rules (csrc/prepare_rules.h), built by
// tests/test_prepare_rules.py with a plain host compiler, once as it is and once with the sanitizers.  One case per input line
// (doubles in any strtod form, hex included), one output line per case:
//   tol  tol_rel yy                      ->  problem_tol as %a
//   live d ref                           ->  column_is_live as 0 / 1
//   diag M ldg  g_0 ... g_(ldg*ldg-1)    ->  gram_diag_finite as 0 / 1   (G row by row, (M + 2) <= ldg)
//   fold nb  p_0 ... p_(4*nb-1)          ->  nonfinite negative sum(%a) zero_rows
#include "prepare_rules.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string rule, tok;
        in >> rule;
        auto num = [&]() { in >> tok; return std::strtod(tok.c_str(), nullptr); };
        auto idx = [&]() { in >> tok; return (int64_t)std::strtoll(tok.c_str(), nullptr, 10); };
        auto nums = [&](int64_t n) { std::vector<double> v((size_t)n); for (double &x : v) x = num(); return v; };   // exactly n: ASan sees an overrun
        if (rule == "tol") {
            const double tol_rel = num(), yy = num();
            if (in) std::printf("%a\n", partls::problem_tol(tol_rel, yy));
        } else if (rule == "live") {
            const double d = num(), ref = num();
            if (in) std::printf("%d\n", partls::column_is_live(d, ref) ? 1 : 0);
        } else if (rule == "diag") {
            const int64_t M = idx(), ldg = idx();
            const std::vector<double> G = nums(ldg * ldg);
            if (in) std::printf("%d\n", partls::gram_diag_finite(G.data(), ldg, M) ? 1 : 0);
        } else if (rule == "fold") {
            const int nb = (int)idx();
            const std::vector<double> part = nums(4 * (int64_t)nb);
            const partls::WeightFold f = partls::fold_weight_partials(part.data(), nb);
            if (in) std::printf("%d %d %a %lld\n", f.nonfinite ? 1 : 0, f.negative ? 1 : 0, f.sum, (long long)f.zero_rows);
        } else {
            in.setstate(std::ios::failbit);
        }
        if (!in) { std::fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
