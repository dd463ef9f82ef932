// cv_alt.hip — partls_cv_alt (include/partls.h): K-fold cross-validation of the multistart fit(Alt) over an η grid, and the full-data
// path, in one call.  The upload, the fold Grams and the combined training Grams are partls_cv_opt's (cv_grams,
// cv.hip), and so are the steps of a batch (ctx.h: batch_work_prepare, batch_prepare_one, batch_pieces_begin, batch_piece_prepare,
// batch_install): the (F+1) x E problems are prepared a piece at a time and the R trajectories of every problem of a piece advance
// together (alt_multistart_core with AltProblems, alt_multi.hip): one block of records per iteration for the whole piece, one
// node-mode launch per problem that still has active starts.  Every problem's winner then goes through the ending of a single
// fit(Alt) (alt_finish) on the working context, whose data passes cover exactly its training rows, and one more pass over fold f
// gives the held-out SSE.  n > 288, PARTLS_OPT_GENERIC_KERNEL and PARTLS_CV_SERIAL=1 take one problem after another through
// batch_prepare_one and the multistart of a single problem instead; both routes end in the same finish.
#include "ctx.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace partls;

namespace {

struct CvAltArgs {
    const int64_t *fold_ptr; int64_t F, E, R;
    const double *eta;
    double eps; int64_t T;
    const double *alpha0; int64_t ld_alpha0; const double *beta0; int64_t ld_beta0;
};

struct CvAltOut {
    CvOut o;                                       // o.best: the winners' start indices
    std::vector<int64_t> iters;
    std::vector<double> opt_all;                   // R x B, filled when the caller asked for any per-trajectory table
    std::vector<int64_t> iters_all;
    std::vector<int32_t> status_all;
};

// Problem q is prepared on W (tableau, host Gram and scale copies, eta): its winner through alt_finish on the training rows of its
// fold, then the held-out SSE from the data.  Status 0 / 9 per problem, 6 when no start finished; anything else fails the call.
partls_status finish_problem(partls_ctx *c, partls_ctx *W, const CvAltArgs &a, int64_t q, const AltWinner &win, CvAltOut &out)
{
    const int64_t M = c->M, K = c->K, f = q / a.E;
    CvOut &o = out.o;
    double *al = o.alpha.data() + (size_t)q * M, *be = o.beta.data() + (size_t)q * K;
    o.sse[(size_t)q] = NAN;
    if (win.start < 0) {
        std::fill(al, al + M, NAN);
        std::fill(be, be + K, NAN);
        o.t[(size_t)q] = NAN; o.opt[(size_t)q] = NAN; o.best[(size_t)q] = -1; out.iters[(size_t)q] = 0;
        o.status[(size_t)q] = PARTLS_ERR_NOT_CONVERGED;
        return PARTLS_OK;
    }
    std::vector<double> gersh((size_t)W->n, 0.0);
    PARTLS_HIP_CHECK(W->altGersh.ensure((size_t)W->n * sizeof(double)));
    PARTLS_HIP_CHECK(launch_gersh(W->Tfull.as<double>(), W->n, W->altGersh.as<double>(), W->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(gersh.data(), W->altGersh.p, (size_t)W->n * sizeof(double), hipMemcpyDeviceToHost, W->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(W->stream));
    cv_point_rows(c, W, a.fold_ptr, a.F, f);
    const partls_status st = alt_finish(W, win.a, win.b, win.wv, win.vcode, win.hdiag, gersh, win.opt, win.iters, 0, al, be, &o.t[(size_t)q],
                                        &o.opt[(size_t)q], &out.iters[(size_t)q]);
    W->peers.clear();
    if (st != PARTLS_OK && st != PARTLS_ERR_ILL_CONDITIONED) return st;
    o.status[(size_t)q] = (int32_t)st;
    o.best[(size_t)q] = win.start;
    return f < a.F ? cv_heldout_sse(c, f, q, o) : PARTLS_OK;
}

partls_status cv_alt_run(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w, int x_on_device,
                         const int64_t *P, int64_t K, int64_t ldP, uint32_t flags, const CvAltArgs &a, bool want_tables, CvAltOut &out)
{
    const int64_t F = a.F, E = a.E, R = a.R, B = (F + 1) * E;
    int ldg = 0, chunks = 0;
    partls_status st = cv_grams(c, X, N, M, ldX, y, w, x_on_device, K, a.fold_ptr, F, flags, "partls_cv_alt", &ldg, &chunks);
    if (st != PARTLS_OK) return st;
    partls_ctx *W = c->cv_work;
    ProblemBatch pb;
    pb.B = B; pb.E = E; pb.eta = a.eta; pb.gs = (int64_t)ldg * ldg;
    pb.G = c->cvG.as<double>() + (size_t)(F > 0 ? F : 1) * pb.gs; pb.hostG = c->cvHostG.data();
    pb.serial = c->knobs.cv_serial; pb.who = "partls_cv_alt";

    // ---- the working context: prepared for the full-data problem at eta[0]; nothing is enumerated, so nothing is calibrated
    st = batch_work_prepare(c, P, ldP, flags, ldg, chunks, pb, F, [&](partls_ctx *Wc) { cv_point_rows(c, Wc, a.fold_ptr, F, F); });
    if (st != PARTLS_OK) return st;

    if (want_tables) {
        out.opt_all.assign((size_t)(B * R), NAN); out.iters_all.assign((size_t)(B * R), 0); out.status_all.assign((size_t)(B * R), 0);
    }
    auto tables_at = [&](int64_t q) {
        AltTables tb{};
        if (want_tables) { tb.opt_all = out.opt_all.data() + q * R; tb.iters_all = out.iters_all.data() + q * R; tb.status_all = out.status_all.data() + q * R; }
        return tb;
    };
    // c->ms[PREP / SWEEP = the iterations / FINISH] (0 since batch_reset) sum wall times over the problems or pieces
    const int n = W->n;

    // ---- one problem after another: the single problem's prepare, the single problem's multistart
    if (!W->use_reg || pb.serial) {
        AltWinner win;
        for (int64_t q = 0; q < B; ++q) {
            auto t0 = std::chrono::steady_clock::now();
            st = batch_prepare_one(c, pb, q);
            if (st != PARTLS_OK) return st;
            PARTLS_HIP_CHECK(hipStreamSynchronize(W->stream));
            c->ms[PARTLS_T_PREP] += ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            st = alt_multistart_core(W, nullptr, a.eps, a.T, R, a.alpha0, a.ld_alpha0, a.beta0, a.ld_beta0, tables_at(q), &win);
            if (st != PARTLS_OK) return st;
            c->ms[PARTLS_T_SWEEP] += ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            st = finish_problem(c, W, a, q, win, out);
            if (st != PARTLS_OK) return st;
            c->ms[PARTLS_T_FINISH] += ms_since(t0);
        }
        return PARTLS_OK;
    }

    // ---- batched: a piece of problems at a time, each with one double more than the common regions, its y'y
    int64_t bc_max = 0;
    st = batch_pieces_begin(c, pb, 1, &bc_max);
    if (st != PARTLS_OK) return st;
    std::vector<AltWinner> win;
    for (int64_t q0 = 0; q0 < B; q0 += bc_max) {
        const int bc = (int)std::min<int64_t>(bc_max, B - q0);
        auto t0 = std::chrono::steady_clock::now();
        BatchPiece pc;
        st = batch_piece_prepare(c, pb, q0, bc, (size_t)bc, &pc);
        if (st != PARTLS_OK) return st;
        // host: [scale | tol] (the piece's head) | y'y
        const size_t head_w = (size_t)bc * (n + 1);
        PARTLS_HIP_CHECK(c->cvHost.resize(head_w + (size_t)bc));
        double *h = c->cvHost.data(), *hyy = h + head_w;
        // y'y of a problem's regularised Gram (the eta rows leave y alone): the entry h_reg reads for a single problem
        for (int j = 0; j < bc; ++j) hyy[j] = pb.hostG[(size_t)((q0 + j) / E) * pb.gs + (size_t)(M + 1) * ldg + (size_t)(M + 1)];
        PARTLS_HIP_CHECK(hipMemcpyAsync(pc.tail, hyy, (size_t)bc * sizeof(double), hipMemcpyHostToDevice, c->stream));
        // the B tolerances (and the scales, for the finish) come back once per piece, not per iteration
        PARTLS_HIP_CHECK(hipMemcpyAsync(h, pc.scale, head_w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        c->ms[PARTLS_T_PREP] += ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        AltProblems pp;
        pp.B = bc; pp.E = E; pp.q0 = q0; pp.G = pb.G; pp.gs = pb.gs; pp.eta = c->cvEta.as<double>();
        pp.scale = pc.scale; pp.T0reg = pc.T0reg; pp.t0d = pc.t0d; pp.tol = h + (size_t)bc * n; pp.yy = pc.tail;
        win.assign((size_t)bc, AltWinner());
        st = alt_multistart_core(W, &pp, a.eps, a.T, R, a.alpha0, a.ld_alpha0, a.beta0, a.ld_beta0, tables_at(q0), win.data());
        if (st != PARTLS_OK) return st;
        c->ms[PARTLS_T_SWEEP] += ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        for (int j = 0; j < bc; ++j) {
            st = batch_install(c, pb, pc, j, h);
            if (st == PARTLS_OK) st = finish_problem(c, W, a, q0 + j, win[(size_t)j], out);
            if (st != PARTLS_OK) return st;
        }
        c->ms[PARTLS_T_FINISH] += ms_since(t0);
    }
    return PARTLS_OK;
}

}  // namespace

extern "C" {

partls_status partls_cv_alt(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w,
                            int x_on_device, const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F,
                            const double *eta, int64_t E, uint32_t flags, double eps, int64_t T, int64_t R,
                            const double *alpha0, int64_t ld_alpha0, const double *beta0, int64_t ld_beta0,
                            double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt, int64_t *iters,
                            int64_t *best_start, double *heldout_sse, int32_t *status,
                            double *opt_all, int64_t *iters_all, int32_t *status_all)
try {
    partls_status st = cv_check_inputs("partls_cv_alt", c, X, N, M, ldX, y, P, K, ldP, fold_ptr, F, eta, E);
    if (st != PARTLS_OK) return st;
    if (!alpha0 || !beta0 || !alpha || !beta || !t || !opt || !iters || !best_start || !heldout_sse || !status) {
        set_error("partls_cv_alt: NULL start or output");
        return PARTLS_ERR_BAD_ARG;
    }
    if (!(eps > 0.0) || T < 1 || R < 1) { set_error("partls_cv_alt: need eps > 0, T >= 1 and R >= 1"); return PARTLS_ERR_BAD_ARG; }
    if (ld_alpha0 < M + 1 || ld_beta0 < K + 1 || ld_alpha < M || ld_beta < K) {
        set_error("partls_cv_alt: leading dimension smaller than the row count");
        return PARTLS_ERR_BAD_ARG;
    }
    const int64_t B = (F + 1) * E;
    if (R > ((int64_t)1 << 40) / B) { set_error("partls_cv_alt: too many trajectories"); return PARTLS_ERR_BAD_ARG; }
    if (c->multi_rank) { set_error("partls_cv_alt: not on a context of a partls_multi"); return PARTLS_ERR_UNSUPPORTED; }
    flags |= PARTLS_OPT_FAITHFUL_INTERCEPT;
    const CvAltArgs a{fold_ptr, F, E, R, eta, eps, T, alpha0, ld_alpha0, beta0, ld_beta0};
    CvAltOut out;
    out.o.assign(B, M, K);
    out.iters.assign((size_t)B, 0);
    st = cv_alt_run(c, X, N, M, ldX, y, w, x_on_device, P, K, ldP, flags, a, opt_all || iters_all || status_all, out);
    if (st != PARTLS_OK) return st;
    out.o.deliver(B, M, K, alpha, ld_alpha, beta, ld_beta, t, opt, best_start, heldout_sse, status);
    std::memcpy(iters, out.iters.data(), (size_t)B * sizeof(int64_t));
    if (opt_all) std::memcpy(opt_all, out.opt_all.data(), (size_t)(B * R) * sizeof(double));
    if (iters_all) std::memcpy(iters_all, out.iters_all.data(), (size_t)(B * R) * sizeof(int64_t));
    if (status_all) std::memcpy(status_all, out.status_all.data(), (size_t)(B * R) * sizeof(int32_t));
    set_error("");
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

}  // extern "C"
