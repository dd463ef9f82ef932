// prepare_rules.h — the rules of the prepare path that more than one of ctx_prepare (prepare.hip), partls_cv_opt (cv.hip),
// partls_opt_weightings (resample.hip) and the preparation kernels (misc.hip) applies, each written once: DESIGN.md §4 promises that the
// three entries agree bit for bit.  Nothing from HIP is included, so the header also builds with a plain host compiler
// (tests/native/prepare_rules_check.cpp); under hipcc the two rules the kernels share with the host are __host__ __device__.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PARTLS_RULE_HD __host__ __device__ inline
#else
#define PARTLS_RULE_HD inline
#endif

namespace partls {

// feasibility tolerance of a prepared problem (unit-diagonal scale): relative to ||y||, kept positive when y'y is 0, negative or tiny
PARTLS_RULE_HD double problem_tol(double tol_rel, double yy)
{
    const double t = tol_rel * sqrt(yy > 0.0 ? yy : 0.0);
    return t > 0.0 ? t : 1e-300;
}

// Does a tableau column carry information?  d: its diagonal after regularisation and intercept elimination; ref: its Gram diagonal
// before.  A (numerically) null column gets scale 0, which keeps it out of every basis.
PARTLS_RULE_HD bool column_is_live(double d, double ref)
{
    return d > 0.0 && d > 1e-14 * fabs(ref);
}

// NaN / Inf anywhere in column m of [X y] makes the diagonal Gram entry sum_i z_im^2 non-finite (so does a finite column whose squares
// overflow — equally outside the Gram form): M + 1 host compares instead of a separate pass over X, which cost 0.87 ms of the 4.1 GB
// read at C4 before the Gram kernel read the same bytes again.  G: host copy of the augmented Gram; the ones column (M) is not data.
inline bool gram_diag_finite(const double *G, int64_t ldg, int64_t M)
{
    for (int64_t i = 0; i < M + 2; ++i)
        if (i != M && !isfinite(G[i * ldg + i])) return false;
    return true;
}

// One column's per-block partials of the weight-prep kernel, part[4 x ..] = (any w < 0, any non-finite w, sum of the finite w, rows
// with w == 0) for block x, folded in index order.  The entries turn the result into their own statuses and messages.
struct WeightFold {
    bool nonfinite, negative;
    double sum;
    int64_t zero_rows;           // a count below 2^53: exact as a sum of doubles
};
inline WeightFold fold_weight_partials(const double *part, int nb)
{
    bool neg = false, bad = false;
    double sum = 0.0, zeros = 0.0;
    for (int x = 0; x < nb; ++x) {
        neg = neg || part[4 * x] != 0.0;
        bad = bad || part[4 * x + 1] != 0.0;
        sum += part[4 * x + 2];
        zeros += part[4 * x + 3];
    }
    return {bad, neg, sum, (int64_t)zeros};
}

}  // namespace partls
