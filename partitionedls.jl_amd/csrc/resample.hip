// resample.hip — partls_opt_weightings (include/partls.h): fit(Opt) under B row weightings of one (X, y, P) in one call — bootstrap
// replicates, jackknife, repeated splits.  X, y and W go up once; weight_prep_kernel — the single weighted fit's, one column per
// blockIdx.y — checks every column and writes sqrt(W); fold_weight_partials (prepare_rules.h) reads its partials as prepare_weights does;
// launch_gram_weightings — the weighted Gram kernel of a single fit with the weighting as a grid dimension (its summation order: an
// all-ones column is the unweighted Gram bit for bit) — fills one Gram per problem at the stride launch_prep_batch indexes with E = 1;
// the problems are then calibrated, prepared, swept and finished by the helpers partls_cv_opt uses (cv.hip: batch_calibrate,
// batch_sweep, finish_model) — the working context's rows are all N rows with column b of W and of sqrt(W) as its weights — and
// oob_sse_kernel evaluates every model on the rows its weighting left out.  DESIGN.md §4.10.
#include "ctx.h"
#include "prepare_rules.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

namespace partls {

static partls_status weightings_run(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device,
                                    const int64_t *P, int64_t K, int64_t ldP, const double *Wt, int64_t ldW, int64_t B, double eta,
                                    uint32_t flags, bool want_sse, CvOut &o, std::vector<int64_t> &oob_rows)
{
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    batch_reset(c, N, M, K, flags);

    // ---- the weightings: up once (a host W larger than 8 MB goes through the page-locked staging in column batches), then one pass
    // that checks every column before anything else is done with it
    const double *dW = Wt;
    int64_t ldd = ldW;
    if (!x_on_device) {
        PARTLS_HIP_CHECK(c->rsW.ensure((size_t)N * B * sizeof(double)));
        partls_status us = upload_matrix(c, c->rsW.p, Wt, N, B, ldW);
        if (us != PARTLS_OK) return us;
        dW = c->rsW.as<double>(); ldd = N;
    }
    const int nb = weight_prep_blocks(N);
    PARTLS_HIP_CHECK(c->rsS.ensure((size_t)N * B * sizeof(double)));
    PARTLS_HIP_CHECK(c->rsPart.ensure((size_t)4 * nb * std::min<int64_t>(B, 65535) * sizeof(double)));
    PARTLS_HIP_CHECK(c->rsHost.resize((size_t)4 * nb * B));
    double *dS = c->rsS.as<double>();
    for (int64_t b0 = 0; b0 < B; b0 += 65535) {
        const int bc = (int)std::min<int64_t>(65535, B - b0);
        PARTLS_HIP_CHECK(launch_weightings_prep(dW + b0 * ldd, N, ldd, bc, dS + b0 * N, c->rsPart.as<double>(), c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->rsHost.data() + (size_t)4 * nb * b0, c->rsPart.p, (size_t)4 * nb * bc * sizeof(double),
                                        hipMemcpyDeviceToHost, c->stream));
    }
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    oob_rows.assign((size_t)B, 0);
    int64_t neg_col = -1, zero_col = -1, inf_col = -1;
    for (int64_t b = 0; b < B; ++b) {
        const WeightFold f = fold_weight_partials(c->rsHost.data() + (size_t)4 * nb * b, nb);
        if (f.nonfinite) { set_error("partls_opt_weightings: weighting %lld contains NaN/Inf", (long long)b); return PARTLS_ERR_NONFINITE; }
        if (f.negative && neg_col < 0) neg_col = b;
        if (!(f.sum > 0.0) && zero_col < 0) zero_col = b;
        if (!std::isfinite(f.sum) && inf_col < 0) inf_col = b;
        oob_rows[(size_t)b] = f.zero_rows;
    }
    if (inf_col >= 0) { set_error("partls_opt_weightings: the sum of weighting %lld overflows", (long long)inf_col); return PARTLS_ERR_NONFINITE; }
    if (neg_col >= 0) { set_error("partls_opt_weightings: weighting %lld has a negative weight", (long long)neg_col); return PARTLS_ERR_BAD_ARG; }
    if (zero_col >= 0) { set_error("partls_opt_weightings: weighting %lld sums to 0", (long long)zero_col); return PARTLS_ERR_BAD_ARG; }

    // ---- one upload of X, y
    partls_status st = adopt_or_upload(c, X, N, M, ldX, y, x_on_device, sizeof(double));
    if (st != PARTLS_OK) return st;
    const double *Xd = static_cast<const double *>(c->dX);

    // ---- one weighted Gram per column, many columns per launch, at the stride of launch_prep_batch (E = 1: Gram q belongs to problem q)
    int ldg = 0, chunks = 0;
    const size_t slabd = gram_slab_doubles(N, M, c->knobs.gram_S, c->knobs.gram_cr, &chunks, &ldg);
    c->ldg = ldg;
    const int64_t gs = (int64_t)ldg * ldg;
    // a launch builds as many Grams as keep its partial-tile slabs within 256 MiB (the last-level cache: a slab is written once and read
    // once by the reduction right behind it)
    const int64_t gb_max = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(B, 65535), (int64_t)(((size_t)256 << 20) / (slabd * sizeof(double)))));
    PARTLS_HIP_CHECK(c->slab.ensure((size_t)gb_max * slabd * sizeof(double)));
    PARTLS_HIP_CHECK(c->cvG.ensure((size_t)B * gs * sizeof(double)));
    double *Gc = c->cvG.as<double>();
    t_begin(c, PARTLS_T_GRAM);
    for (int64_t b0 = 0; b0 < B; b0 += gb_max) {
        const int gb = (int)std::min<int64_t>(gb_max, B - b0);
        PARTLS_HIP_CHECK(launch_gram_weightings(Xd, N, M, c->ldX, c->dy, c->slab.as<double>(), (int64_t)slabd, chunks, ldg, c->knobs.gram_S,
                                                c->knobs.gram_cr, Gc + (size_t)b0 * gs, gs, dS + b0 * N, gb, c->stream));
    }
    t_end(c, PARTLS_T_GRAM);
    PARTLS_HIP_CHECK(c->cvHostG.resize((size_t)B * gs));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->cvHostG.data(), Gc, (size_t)B * gs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    t_collect(c);
    // NaN / Inf in [X y], on every weighting's Gram: a single weighted fit of that column fails the same way
    for (int64_t b = 0; b < B; ++b)
        if (!gram_diag_finite(c->cvHostG.data() + (size_t)b * gs, ldg, M)) {
            set_error("partls_opt_weightings: X or y contains NaN/Inf (or overflows in X'X)");
            return PARTLS_ERR_NONFINITE;
        }

    // ---- the working context: all N rows under the weights of column b; the visiting order is calibrated on weighting 0
    st = make_internal(c, &c->cv_work);
    if (st != PARTLS_OK) return st;
    partls_ctx *W = c->cv_work;
    auto point_column = [&](int64_t b) {
        W->peers.clear();
        W->dX = c->dX; W->dy = c->dy; W->ldX = c->ldX; W->N = N;
        W->dw = dW + b * ldd; W->ds = dS + b * N;
    };
    ProblemBatch pb;
    pb.B = B; pb.E = 1; pb.eta = &eta; pb.G = Gc; pb.hostG = c->cvHostG.data(); pb.gs = gs;
    pb.serial = c->knobs.resample_serial; pb.who = "partls_opt_weightings";
    pb.finish = [&](int64_t q, int64_t bpat, int64_t unconv) {
        point_column(q);
        return finish_model(c, q, bpat, unconv, o);
    };
    st = batch_calibrate(c, P, ldP, flags, ldg, chunks, pb, 0, [&](partls_ctx *) { point_column(0); });
    if (st != PARTLS_OK) return st;
    st = batch_sweep(c, pb);
    if (st != PARTLS_OK) return st;
    W->dw = nullptr; W->ds = nullptr;

    // ---- out of bag: every model on the rows its weighting left out, a chunk of problems per launch
    if (!want_sse) return PARTLS_OK;
    const int64_t oc_max = std::min<int64_t>(65535, std::max<int64_t>(1, (int64_t)(((size_t)32 << 20) / ((size_t)(M + 1 + nb) * sizeof(double)))));
    PARTLS_HIP_CHECK(c->rsWv.ensure((size_t)oc_max * (M + 1) * sizeof(double)));
    PARTLS_HIP_CHECK(c->rsPart.ensure((size_t)std::max<int64_t>(oc_max, 4 * std::min<int64_t>(B, 65535)) * nb * sizeof(double)));
    PARTLS_HIP_CHECK(c->rsHost.resize((size_t)oc_max * (M + 1 + nb)));
    double *hwv = c->rsHost.data(), *hpart = hwv + (size_t)oc_max * (M + 1);
    Events<2> ev;
    PARTLS_HIP_CHECK(ev.create());
    const hipEvent_t e0 = ev.e[0], e1 = ev.e[1];
    double ms_oob = 0.0;
    for (int64_t q0 = 0; q0 < B; q0 += oc_max) {
        const int oc = (int)std::min<int64_t>(oc_max, B - q0);
        for (int j = 0; j < oc; ++j) {
            double *w = hwv + (size_t)j * (M + 1);
            if (o.status[(size_t)(q0 + j)] == PARTLS_ERR_NOT_CONVERGED) std::fill(w, w + M + 1, 0.0);
            else model_weights(W, o, q0 + j, w);
        }
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->rsWv.p, hwv, (size_t)oc * (M + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PARTLS_HIP_CHECK(hipEventRecord(e0, c->stream));
        PARTLS_HIP_CHECK(launch_oob_sse(Xd, N, M, c->ldX, c->dy, dW + q0 * ldd, ldd, c->rsWv.as<double>(), oc, c->rsPart.as<double>(), c->stream));
        PARTLS_HIP_CHECK(hipEventRecord(e1, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(hpart, c->rsPart.p, (size_t)oc * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        float f = 0.f;
        if (hipEventElapsedTime(&f, e0, e1) == hipSuccess) ms_oob += f;
        for (int j = 0; j < oc; ++j) {
            const int64_t q = q0 + j;
            if (o.status[(size_t)q] == PARTLS_ERR_NOT_CONVERGED || oob_rows[(size_t)q] == 0) continue;      // stays NaN
            double s = 0.0;
            for (int x = 0; x < nb; ++x) s += hpart[(size_t)j * nb + x];
            o.sse[(size_t)q] = s;
        }
    }
    c->ms[PARTLS_T_OOB] = ms_oob;
    return PARTLS_OK;
}

}  // namespace partls

using namespace partls;

partls_status partls_opt_weightings(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device,
                                    const int64_t *P, int64_t K, int64_t ldP, const double *W, int64_t ldW, int64_t B, double eta,
                                    uint32_t flags, double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt,
                                    int64_t *best_index, double *oob_sse, int64_t *oob_rows, int32_t *status)
try {
    partls_status st = check_common(c, X, N, M, ldX, P, K, ldP);
    if (st != PARTLS_OK) return st;
    if (!y) { set_error("partls_opt_weightings: y is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (!W) { set_error("partls_opt_weightings: W is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (B < 1) { set_error("partls_opt_weightings: B = %lld weightings (need B >= 1)", (long long)B); return PARTLS_ERR_BAD_ARG; }
    if (ldW < N) { set_error("partls_opt_weightings: ldW = %lld is smaller than N = %lld", (long long)ldW, (long long)N); return PARTLS_ERR_BAD_ARG; }
    if (!(eta >= 0.0) || !std::isfinite(eta)) { set_error("partls_opt_weightings: eta = %g must be finite and >= 0", eta); return PARTLS_ERR_BAD_ARG; }
    if (!alpha || !beta || !t || !opt || !best_index || !status) { set_error("partls_opt_weightings: NULL output"); return PARTLS_ERR_BAD_ARG; }
    if (ld_alpha < M || ld_beta < K) { set_error("partls_opt_weightings: leading dimension of alpha / beta too small"); return PARTLS_ERR_BAD_ARG; }
    if (B > ((int64_t)1 << 40) / N) { set_error("partls_opt_weightings: too many weightings for N = %lld rows", (long long)N); return PARTLS_ERR_BAD_ARG; }
    if (c->multi_rank) {
        set_error("partls_opt_weightings: a context of a partls_multi is not supported (multi-GPU fits are unweighted)");
        return PARTLS_ERR_UNSUPPORTED;
    }
    if (flags & PARTLS_OPT_RESCUE_CAPPED) { set_error("partls_opt_weightings: PARTLS_OPT_RESCUE_CAPPED is not supported by the batched sweeps"); return PARTLS_ERR_UNSUPPORTED; }
    if ((flags & PARTLS_OPT_FAITHFUL_INTERCEPT ? K + 1 : K) > 40) {
        set_error("partls_opt_weightings: K = %lld: the enumeration of fit(Opt) is out of range (K <= 39)", (long long)K);
        return PARTLS_ERR_UNSUPPORTED;
    }
    CvOut o;
    o.assign(B, M, K);
    std::vector<int64_t> rows;
    st = weightings_run(c, X, N, M, ldX, y, x_on_device, P, K, ldP, W, ldW, B, eta, flags, oob_sse != nullptr, o, rows);
    if (st != PARTLS_OK) return st;
    o.deliver(B, M, K, alpha, ld_alpha, beta, ld_beta, t, opt, best_index, oob_sse, status);
    if (oob_rows) std::memcpy(oob_rows, rows.data(), (size_t)B * sizeof(int64_t));
    set_error("");
    return PARTLS_OK;
}
PARTLS_ABI_GUARD
