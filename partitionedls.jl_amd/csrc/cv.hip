// cv.hip — partls_cv_opt (include/partls.h): K-fold cross-validation of fit(Opt) over an η grid, and the full-data regularisation
// path, in one call.  X goes up once; every fold's Gram products are built once (one launch_gram per row slice) and combined into the
// training Gram of every fold (the sum of the other folds') and of all rows; the (F+1) x E problems are prepared in one batched launch
// and swept in one launch of the BATCH instantiation of the register kernels (blockIdx.y = problem).  Each problem is then finished as
// partls_opt_finish finishes a single fit (near-tie re-rank from the data, refinement, KKT check, cleanupResult), on an internal working
// context whose data passes cover exactly its training rows (row-block views of the folds as its peers).  DESIGN.md §4.6.
// The parts that do not know about folds — the reset, the working context's prepare and calibration, the piece rule, the prepare of a
// piece and the install of one of its problems, the batched / serial sweep of B problems over Grams at a fixed stride with the finish
// as a callback, the finish of one model — are the batch_* helpers of ctx.h, which partls_opt_weightings (resample.hip) and, up to the
// sweep, partls_cv_alt (cv_alt.hip) share.  The steps a single prepare has too are the single prepare's (prepare.hip, prepare_rules.h):
// forget_problem, adopt_or_upload, prepare_weights, gram_diag_finite, ctx_prepare_tableau and the preparation kernels.
#include "ctx.h"
#include "prepare_rules.h"
#include <cmath>
#include <cstring>
#include <algorithm>

namespace partls {

// out[f] = sum over the folds g != f of Gf[g], g ascending (f < F); out[F] = sum over every fold.  nf = max(F, 1) fold Grams at stride gs.
// A fixed order and no atomics: bitwise reproducible.
__global__ __launch_bounds__(256) void fold_gram_combine_kernel(const double *__restrict__ Gf, int nf, int F, int64_t gs, int64_t cnt,
                                                                double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const int f = blockIdx.y;
    double s = 0.0;
    for (int g = 0; g < nf; ++g)
        if (f == F || g != f) s += Gf[(int64_t)g * gs + i];
    out[(int64_t)f * gs + i] = s;
}

static hipError_t launch_fold_gram_combine(const double *Gf, int nf, int F, int64_t gs, double *out, hipStream_t s)
{
    const int64_t cnt = gs;
    hipLaunchKernelGGL(fold_gram_combine_kernel, dim3((unsigned)((cnt + 255) / 256), F + 1), dim3(256), 0, s, Gf, nf, F, gs, cnt, out);
    return hipGetLastError();
}

partls_status make_internal(partls_ctx *c, partls_ctx **slot)
{
    if (*slot) return PARTLS_OK;
    partls_status st = partls_create(c->device, slot);
    if (st != PARTLS_OK) return st;
    (*slot)->knobs = c->knobs;
    return PARTLS_OK;
}

// the working context sees the training rows of problem fold f (f == F: all rows): its own rows are the first training fold, the
// other training folds are its peers (data_pass, refine.hip, sums context then peers in order)
void cv_point_rows(partls_ctx *c, partls_ctx *W, const int64_t *fold_ptr, int64_t F, int64_t f)
{
    W->peers.clear();
    W->ldX = c->ldX;
    if (f == F) { W->dX = c->dX; W->dy = c->dy; W->dw = c->dw; W->ds = c->ds; W->N = c->N; return; }
    bool first = true;
    for (int64_t g = 0; g < F; ++g) {
        if (g == f) continue;
        if (first) {
            W->dX = static_cast<const double *>(c->dX) + fold_ptr[g]; W->dy = c->dy + fold_ptr[g]; W->N = fold_ptr[g + 1] - fold_ptr[g];
            W->dw = c->dw ? c->dw + fold_ptr[g] : nullptr; W->ds = c->ds ? c->ds + fold_ptr[g] : nullptr;
            first = false;
        } else {
            W->peers.push_back(c->cv_view[(size_t)g]);
        }
    }
}

void CvOut::assign(int64_t B, int64_t M, int64_t K)
{
    alpha.assign((size_t)B * M, 0.0); beta.assign((size_t)B * K, 0.0);
    t.assign((size_t)B, 0.0); opt.assign((size_t)B, 0.0); sse.assign((size_t)B, NAN);
    best.assign((size_t)B, -1); status.assign((size_t)B, 0);
}

void CvOut::deliver(int64_t B, int64_t M, int64_t K, double *alpha_out, int64_t ld_alpha, double *beta_out, int64_t ld_beta, double *t_out,
                    double *opt_out, int64_t *best_out, double *sse_out, int32_t *status_out) const
{
    for (int64_t q = 0; q < B; ++q) {
        std::memcpy(alpha_out + q * ld_alpha, alpha.data() + (size_t)q * M, (size_t)M * sizeof(double));
        std::memcpy(beta_out + q * ld_beta, beta.data() + (size_t)q * K, (size_t)K * sizeof(double));
    }
    std::memcpy(t_out, t.data(), (size_t)B * sizeof(double));
    std::memcpy(opt_out, opt.data(), (size_t)B * sizeof(double));
    std::memcpy(best_out, best.data(), (size_t)B * sizeof(int64_t));
    if (sse_out) std::memcpy(sse_out, sse.data(), (size_t)B * sizeof(double));
    std::memcpy(status_out, status.data(), (size_t)B * sizeof(int32_t));
}

partls_status finish_model(partls_ctx *c, int64_t q, int64_t bpat, int64_t unconv, CvOut &o)
{
    const int64_t M = c->M, K = c->K;
    double *a = o.alpha.data() + (size_t)q * M, *b = o.beta.data() + (size_t)q * K;
    partls_status st = PARTLS_ERR_NOT_CONVERGED;
    if (bpat >= 0) {
        st = partls_opt_finish(c->cv_work, bpat, a, b, &o.t[(size_t)q], &o.opt[(size_t)q], &o.best[(size_t)q]);
        if (st == PARTLS_OK && unconv) st = PARTLS_ERR_NOT_CONVERGED;
    }
    if (st != PARTLS_OK && st != PARTLS_ERR_ILL_CONDITIONED && st != PARTLS_ERR_NOT_CONVERGED) return st;
    o.status[(size_t)q] = (int32_t)st;
    o.sse[(size_t)q] = NAN;
    if (st == PARTLS_ERR_NOT_CONVERGED) {
        std::fill(a, a + M, NAN);
        std::fill(b, b + K, NAN);
        o.t[(size_t)q] = NAN; o.opt[(size_t)q] = NAN; o.best[(size_t)q] = -1;
    }
    return PARTLS_OK;
}

void model_weights(const partls_ctx *work, const CvOut &o, int64_t q, double *w)
{
    const int64_t M = work->M, K = work->K;
    const double *a = o.alpha.data() + (size_t)q * M, *b = o.beta.data() + (size_t)q * K;
    for (int64_t m = 0; m < M; ++m) {
        double s = 0.0;
        for (int64_t k = 0; k < K; ++k) if (work->P[(size_t)m + (size_t)k * M]) s += b[k];
        w[m] = a[m] * s;
    }
    w[M] = o.t[(size_t)q];
}

partls_status cv_heldout_sse(partls_ctx *c, int64_t f, int64_t q, CvOut &o)
{
    // predict (PartitionedLS.jl:132): yhat = X (P .* alpha) beta .+ t on fold f's rows
    std::vector<double> w((size_t)c->M + 1, 0.0);
    model_weights(c->cv_work, o, q, w.data());
    double s2 = 0.0;
    const partls_status st = data_pass(c->cv_view[(size_t)f], w, true, false, &s2, nullptr, {});
    if (st == PARTLS_OK) o.sse[(size_t)q] = s2;
    return st;
}

// Finish problem q on W (prepared state already installed): the tested single-fit finish, then the held-out SSE on fold f's rows.
static partls_status finish_one(partls_ctx *c, partls_ctx *W, const int64_t *fold_ptr, int64_t F, int64_t f, int64_t q, int64_t bpat,
                                int64_t unconv, CvOut &o)
{
    if (bpat >= 0) cv_point_rows(c, W, fold_ptr, F, f);
    const partls_status st = finish_model(c, q, bpat, unconv, o);
    W->peers.clear();
    if (st != PARTLS_OK || o.status[(size_t)q] == PARTLS_ERR_NOT_CONVERGED || f == F) return st;
    return cv_heldout_sse(c, f, q, o);
}

void batch_reset(partls_ctx *c, int64_t N, int64_t M, int64_t K, uint32_t flags)
{
    // this context keeps the upload and the Gram products; it holds no prepared problem afterwards
    forget_problem(c);
    for (int w = 0; w < PARTLS_T_COUNT; ++w) c->ms[w] = 0.0;
    c->N = N; c->M = M; c->K = K; c->flags = flags; c->faithful = (flags & PARTLS_OPT_FAITHFUL_INTERCEPT) != 0;
}

partls_status batch_prepare_one(partls_ctx *c, const ProblemBatch &pb, int64_t q)
{
    partls_ctx *W = c->cv_work;
    PARTLS_HIP_CHECK(hipMemcpyAsync(W->G.p, pb.G + (size_t)(q / pb.E) * pb.gs, (size_t)pb.gs * sizeof(double), hipMemcpyDeviceToDevice, W->stream));
    W->eta = pb.eta[q % pb.E];
    return ctx_prepare_tableau(W);
}

partls_status batch_work_prepare(partls_ctx *c, const int64_t *P, int64_t ldP, uint32_t flags, int ldg, int chunks, const ProblemBatch &pb,
                                 int64_t cal_gram, const std::function<void(partls_ctx *)> &point_rows)
{
    partls_ctx *W = c->cv_work;
    const int64_t M = c->M, K = c->K;
    forget_problem(W);
    W->knobs = c->knobs;
    W->gram_hook = nullptr;
    partls_status st = load_partition(W, P, M, K, ldP);
    if (st != PARTLS_OK) return st;
    W->M = M; W->K = K; W->flags = flags; W->faithful = c->faithful;
    W->ldg = ldg; W->chunks = chunks;
    PARTLS_HIP_CHECK(W->G.ensure((size_t)pb.gs * sizeof(double)));
    point_rows(W);
    st = batch_prepare_one(c, pb, cal_gram * pb.E);          // Gram cal_gram at eta[0]
    W->peers.clear();
    return st;
}

partls_status batch_calibrate(partls_ctx *c, const int64_t *P, int64_t ldP, uint32_t flags, int ldg, int chunks, const ProblemBatch &pb,
                              int64_t cal_gram, const std::function<void(partls_ctx *)> &point_rows)
{
    partls_ctx *W = c->cv_work;
    partls_status st = batch_work_prepare(c, P, ldP, flags, ldg, chunks, pb, cal_gram, point_rows);
    if (st != PARTLS_OK) return st;
    if ((int64_t)W->kbits > 40) { set_error("%s: %d sign bits: the enumeration is out of range (K <= 39)", pb.who, W->kbits); return PARTLS_ERR_UNSUPPORTED; }
    st = calibrate_bit_order(W);
    if (st != PARTLS_OK) return st;
    c->ms[PARTLS_T_CALIB] = W->ms[PARTLS_T_CALIB];
    return PARTLS_OK;
}

partls_status batch_pieces_begin(partls_ctx *c, const ProblemBatch &pb, size_t extra, int64_t *per_piece)
{
    // Per problem a piece stacks its full tableau ((n+1)^2), its tile-cyclic tableau, its scale (n), its tolerance (1) and the caller's
    // `extra` doubles; what else a caller keeps in the tail is not counted.  PARTLS_BATCH_PIECE (tests) replaces the byte bound.
    const partls_ctx *W = c->cv_work;
    const size_t n = (size_t)W->n, per = ((n + 1) * (n + 1) + sweep_reg_t0_doubles(W->T) + n + 1 + extra) * sizeof(double);
    *per_piece = std::max<int64_t>(1, std::min<int64_t>(65535, (int64_t)(PARTLS_OPT_MODELS_PIECE_BYTES / per)));
    if (c->knobs.batch_piece > 0) *per_piece = std::min(65535, c->knobs.batch_piece);
    PARTLS_HIP_CHECK(c->cvEta.ensure((size_t)pb.E * sizeof(double)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->cvEta.p, pb.eta, (size_t)pb.E * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return PARTLS_OK;
}

partls_status batch_piece_prepare(partls_ctx *c, const ProblemBatch &pb, int64_t q0, int bc, size_t tail_words, BatchPiece *pc)
{
    const partls_ctx *W = c->cv_work;
    const int n = W->n;
    pc->q0 = q0; pc->bc = bc;
    pc->tfd = (size_t)(n + 1) * (n + 1); pc->t0d = sweep_reg_t0_doubles(W->T);
    PARTLS_HIP_CHECK(c->cvBatch.ensure(((size_t)bc * (n + 1 + pc->tfd + pc->t0d) + tail_words) * sizeof(double)));
    // the one statement of the order: [scale (bc x n) | tol (bc) | Tfull (bc x tfd) | T0reg (bc x t0d) | tail (tail_words)]
    pc->scale = c->cvBatch.as<double>(); pc->tol = pc->scale + (size_t)bc * n; pc->Tfull = pc->tol + bc;
    pc->T0reg = pc->Tfull + (size_t)bc * pc->tfd; pc->tail = pc->T0reg + (size_t)bc * pc->t0d;
    PARTLS_HIP_CHECK(launch_prep_batch(pb.G, pb.gs, (int)pb.E, q0, c->cvEta.as<double>(), W->ldg, (int)c->M, W->maskAugD.as<uint64_t>(),
                                       W->faithful ? 0 : 1, W->permP, c->knobs.tol_rel, pc->scale, pc->Tfull, pc->tol, n, bc, c->stream));
    PARTLS_HIP_CHECK(launch_layout_reg_batch(pc->Tfull, n, W->T, bc, pc->T0reg, c->stream));
    return PARTLS_OK;
}

partls_status batch_install(partls_ctx *c, const ProblemBatch &pb, const BatchPiece &pc, int j, const double *head)
{
    partls_ctx *W = c->cv_work;
    const int64_t q = pc.q0 + j, f = q / pb.E;
    const size_t n = (size_t)W->n, gs = (size_t)pb.gs;
    W->eta = pb.eta[q % pb.E];
    std::memcpy(W->hG.data(), pb.hostG + (size_t)f * gs, gs * sizeof(double));
    std::memcpy(W->hScale.data(), head + (size_t)j * n, n * sizeof(double));
    W->tol = head[(size_t)pc.bc * n + (size_t)j];
    PARTLS_HIP_CHECK(hipMemcpyAsync(W->G.p, pb.G + (size_t)f * gs, gs * sizeof(double), hipMemcpyDeviceToDevice, W->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(W->scale.p, pc.scale + (size_t)j * n, n * sizeof(double), hipMemcpyDeviceToDevice, W->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(W->Tfull.p, pc.Tfull + (size_t)j * pc.tfd, pc.tfd * sizeof(double), hipMemcpyDeviceToDevice, W->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(W->T0reg.p, pc.T0reg + (size_t)j * pc.t0d, pc.t0d * sizeof(double), hipMemcpyDeviceToDevice, W->stream));
    W->coop_state_valid = false;
    W->tab_valid = false;
    W->prepared = true;
    return PARTLS_OK;
}

partls_status batch_sweep(partls_ctx *c, const ProblemBatch &pb)
{
    partls_ctx *W = c->cv_work;
    const int64_t B = pb.B;
    const int n = W->n;
    const int64_t npat = (int64_t)1 << W->kbits;
    partls_status st = PARTLS_OK;

    // c->ms[PREP / SWEEP / FINISH] (0 since batch_reset) sum over the problems or pieces
    // ---- every problem on its own through the existing launchers: n > 288, PARTLS_OPT_GENERIC_KERNEL, the entry's serial knob
    if (!W->use_reg || pb.serial) {
        for (int64_t q = 0; q < B; ++q) {
            st = batch_prepare_one(c, pb, q);
            if (st != PARTLS_OK) return st;
            c->ms[PARTLS_T_PREP] += W->ms[PARTLS_T_PREP];
            double bobj = 0.0;
            int64_t bpat = -1, unconv = 0;
            st = partls_opt_sweep(W, 0, -1, &bobj, &bpat, nullptr, &unconv);
            if (st != PARTLS_OK) return st;
            c->ms[PARTLS_T_SWEEP] += W->ms[PARTLS_T_SWEEP];
            const auto f0 = std::chrono::steady_clock::now();
            st = pb.finish(q, bpat, unconv);
            if (st != PARTLS_OK) return st;
            c->ms[PARTLS_T_FINISH] += ms_since(f0);
        }
        return PARTLS_OK;
    }

    // ---- batched: a piece of problems at a time
    const int T = W->T;
    int64_t bc_max = 0;
    st = batch_pieces_begin(c, pb, 0, &bc_max);
    if (st != PARTLS_OK) return st;
    const bool want_sol = (sweep_reg_small(T) || sweep_reg_exports(T)) && !c->knobs.no_export;
    PARTLS_HIP_CHECK(c->scratch.ensure(64 * sizeof(double)));      // the register kernels' share (ensure_sweep_scratch goes by W, the prepared context)
    Events<4> evs;
    PARTLS_HIP_CHECK(evs.create());
    hipEvent_t *ev = evs.e;
    for (int64_t q0 = 0; q0 < B; q0 += bc_max) {
        const int bc = (int)std::min<int64_t>(bc_max, B - q0);
        int64_t chain_len = 0;
        int grid_all = 0;
        if (!sweep_plan(W, npat * bc, &chain_len, &grid_all, pb.who)) return PARTLS_ERR_UNSUPPORTED;
        const int64_t nch = (npat + chain_len - 1) / chain_len;
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(nch, (grid_all + bc - 1) / bc));
        // the piece's tail: [sweep blocks (bc x out_w) | best_sol (bc x gx x n), when exported]
        const size_t out_w = sweep_block_words(gx, true), sol_w = want_sol ? (size_t)gx * n : 0, head_w = (size_t)bc * (n + 1);
        BatchPiece pc;
        PARTLS_HIP_CHECK(hipEventRecord(ev[0], c->stream));
        st = batch_piece_prepare(c, pb, q0, bc, (size_t)bc * (out_w + sol_w), &pc);
        if (st != PARTLS_OK) return st;
        double *d_out = pc.tail, *d_sol = pc.tail + (size_t)bc * out_w;
        PARTLS_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)bc * out_w * sizeof(double), c->stream));
        PARTLS_HIP_CHECK(hipEventRecord(ev[1], c->stream));
        SweepParams p = sweep_params(W, /*internal_order=*/true);
        p.T0 = pc.T0reg;
        p.scratch = c->scratch.as<double>();
        p.g_begin = 0; p.g_end = npat; p.chain_len = chain_len;
        p.tol = 0.0;                                             // every problem has its own: batch_tol
        bind_sweep_block(p, d_out, gx, true);                    // problem 0's block; problem q's lies q * batch_out words further
        if (want_sol) { p.best_sol = d_sol; p.node_ld = n; }
        p.batch_t0 = (int64_t)pc.t0d; p.batch_out = (int64_t)out_w; p.batch_tol = pc.tol;
        PARTLS_HIP_CHECK(launch_sweep_blk_batch(p, T, gx, bc, c->stream));
        PARTLS_HIP_CHECK(hipEventRecord(ev[2], c->stream));
        // host copies: [scale | tol] (the piece's head), then the sweep blocks
        PARTLS_HIP_CHECK(c->cvHost.resize(head_w + (size_t)bc * out_w));
        double *h = c->cvHost.data(), *hout = h + head_w;
        PARTLS_HIP_CHECK(hipMemcpyAsync(h, pc.scale, head_w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(hout, d_out, (size_t)bc * out_w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        float f01 = 0.f, f12 = 0.f;
        if (hipEventElapsedTime(&f01, ev[0], ev[1]) == hipSuccess) c->ms[PARTLS_T_PREP] += f01;
        if (hipEventElapsedTime(&f12, ev[1], ev[2]) == hipSuccess) c->ms[PARTLS_T_SWEEP] += f12;
        const auto f0 = std::chrono::steady_clock::now();
        for (int j = 0; j < bc; ++j) {
            // what ctx_prepare_tableau would have left (batch_install), then what partls_opt_sweep would have left: the winner's exported
            // solution, the winner and the near ties
            st = batch_install(c, pb, pc, j, h);
            if (st != PARTLS_OK) return st;
            if (want_sol) {
                PARTLS_HIP_CHECK(W->bestSol.ensure(sol_w * sizeof(double)));
                PARTLS_HIP_CHECK(hipMemcpyAsync(W->bestSol.p, d_sol + (size_t)j * sol_w, sol_w * sizeof(double), hipMemcpyDeviceToDevice, W->stream));
            }
            double bobj = 0.0;
            int64_t bpat = -1;
            const double *blk = hout + (size_t)j * out_w;
            install_sweep_result(W, blk, gx, want_sol, &bobj, &bpat);
            unsigned long long unconv = 0;
            std::memcpy(&unconv, blk, sizeof(unconv));
            st = pb.finish(q0 + j, bpat, (int64_t)unconv);
            if (st != PARTLS_OK) return st;
        }
        c->ms[PARTLS_T_FINISH] += ms_since(f0);
    }
    return PARTLS_OK;
}

partls_status cv_grams(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w, int x_on_device,
                       int64_t K, const int64_t *fold_ptr, int64_t F, uint32_t flags, const char *who, int *ldg_out, int *chunks_out)
{
    const int nf = F > 0 ? (int)F : 1;
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    batch_reset(c, N, M, K, flags);
    // ---- sample weights (partls_cv_opt_weighted): checked and square-rooted before anything else; every fold Gram and every data pass
    // (finish, held-out SSE) then reads its rows' slice of them
    if (w) {
        partls_status ws = prepare_weights(c, w, N, x_on_device);
        if (ws != PARTLS_OK) return ws;
    }

    // ---- one upload
    partls_status st = adopt_or_upload(c, X, N, M, ldX, y, x_on_device, sizeof(double));
    if (st != PARTLS_OK) return st;
    const double *Xd = static_cast<const double *>(c->dX);

    // ---- internal contexts: the working context and one row view per fold
    st = make_internal(c, &c->cv_work);
    if (st != PARTLS_OK) return st;
    if (c->cv_view.size() < (size_t)F) c->cv_view.resize((size_t)F, nullptr);
    for (int64_t g = 0; g < F; ++g) {
        st = make_internal(c, &c->cv_view[(size_t)g]);
        if (st != PARTLS_OK) return st;
        partls_ctx *v = c->cv_view[(size_t)g];
        v->dX = Xd + fold_ptr[g]; v->dy = c->dy + fold_ptr[g]; v->ldX = c->ldX;
        v->dw = c->dw ? c->dw + fold_ptr[g] : nullptr; v->ds = c->ds ? c->ds + fold_ptr[g] : nullptr;
        v->N = fold_ptr[g + 1] - fold_ptr[g]; v->M = M; v->K = K;
        v->peers.clear();
    }

    // ---- one Gram launch per fold (row slice X + fold_ptr[g], y + fold_ptr[g], ldX unchanged), then the combine
    int ldg = 0, chunks = 0;
    size_t slabd = 0;
    for (int g = 0; g < nf; ++g) {
        const int64_t n_g = F > 0 ? fold_ptr[g + 1] - fold_ptr[g] : N;
        slabd = std::max(slabd, gram_slab_doubles(n_g, M, c->knobs.gram_S, c->knobs.gram_cr, &chunks, &ldg));
    }
    c->ldg = ldg;
    const int64_t gs = (int64_t)ldg * ldg;
    PARTLS_HIP_CHECK(c->slab.ensure(slabd * sizeof(double)));
    PARTLS_HIP_CHECK(c->cvG.ensure((size_t)(nf + F + 1) * gs * sizeof(double)));
    double *Gf = c->cvG.as<double>(), *Gc = Gf + (size_t)nf * gs;
    t_begin(c, PARTLS_T_GRAM);
    for (int g = 0; g < nf; ++g) {
        const int64_t r0 = F > 0 ? fold_ptr[g] : 0, n_g = F > 0 ? fold_ptr[g + 1] - fold_ptr[g] : N;
        int ch = 0, ld2 = 0;
        (void)gram_slab_doubles(n_g, M, c->knobs.gram_S, c->knobs.gram_cr, &ch, &ld2);
        PARTLS_HIP_CHECK(launch_gram(Xd + r0, n_g, M, c->ldX, c->dy + r0, c->slab.as<double>(), ch, ldg, c->knobs.gram_S, c->knobs.gram_cr,
                                     Gf + (size_t)g * gs, c->stream, c->ds ? c->ds + r0 : nullptr));
    }
    PARTLS_HIP_CHECK(launch_fold_gram_combine(Gf, nf, (int)F, gs, Gc, c->stream));
    t_end(c, PARTLS_T_GRAM);
    PARTLS_HIP_CHECK(c->cvHostG.resize((size_t)(F + 1) * gs));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->cvHostG.data(), Gc, (size_t)(F + 1) * gs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    t_collect(c);
    // NaN / Inf in [X y]: the all-rows Gram decides (its diagonal is the sum of the folds' non-negative diagonals)
    if (!gram_diag_finite(c->cvHostG.data() + (size_t)F * gs, ldg, M)) {
        set_error("%s: X or y contains NaN/Inf (or overflows in X'X)", who);
        return PARTLS_ERR_NONFINITE;
    }
    // weighted: every training set needs weight (its ones-column entry is sum_i s_i^2 over its rows)
    if (c->ds)
        for (int64_t f = 0; f < F; ++f)
            if (!(c->cvHostG[(size_t)f * gs + (size_t)M * ldg + M] > 0.0)) {
                set_error("%s: the training rows of fold %lld have zero total weight", who, (long long)f);
                return PARTLS_ERR_BAD_ARG;
            }
    *ldg_out = ldg; *chunks_out = chunks;
    return PARTLS_OK;
}

static partls_status cv_run(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w,
                            int x_on_device, const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F, const double *eta,
                            int64_t E, uint32_t flags, CvOut &o)
{
    int ldg = 0, chunks = 0;
    partls_status st = cv_grams(c, X, N, M, ldX, y, w, x_on_device, K, fold_ptr, F, flags, "partls_cv_opt", &ldg, &chunks);
    if (st != PARTLS_OK) return st;
    partls_ctx *W = c->cv_work;
    const int64_t gs = (int64_t)ldg * ldg;
    const double *Gc = c->cvG.as<double>() + (size_t)(F > 0 ? F : 1) * gs;

    // ---- the working context: prepared first for the full-data problem at eta[0], on which the visiting order is calibrated
    ProblemBatch pb;
    pb.B = (F + 1) * E; pb.E = E; pb.eta = eta; pb.G = Gc; pb.hostG = c->cvHostG.data(); pb.gs = gs;
    pb.serial = c->knobs.cv_serial; pb.who = "partls_cv_opt";
    pb.finish = [&](int64_t q, int64_t bpat, int64_t unconv) { return finish_one(c, W, fold_ptr, F, q / E, q, bpat, unconv, o); };
    st = batch_calibrate(c, P, ldP, flags, ldg, chunks, pb, F, [&](partls_ctx *Wc) { cv_point_rows(c, Wc, fold_ptr, F, F); });
    if (st != PARTLS_OK) return st;
    return batch_sweep(c, pb);
}

// the input checks partls_cv_opt and partls_cv_alt share (everything but their outputs and their own options)
partls_status cv_check_inputs(const char *who, partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                              const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F, const double *eta, int64_t E)
{
    partls_status st = check_common(c, X, N, M, ldX, P, K, ldP);
    if (st != PARTLS_OK) return st;
    if (!y) { set_error("%s: y is NULL", who); return PARTLS_ERR_BAD_ARG; }
    if (F < 0 || F == 1) { set_error("%s: F = %lld folds (need F = 0 for the path only, or F >= 2)", who, (long long)F); return PARTLS_ERR_BAD_ARG; }
    if (F > 0) {
        if (!fold_ptr) { set_error("%s: fold_ptr is NULL", who); return PARTLS_ERR_BAD_ARG; }
        if (F > N) { set_error("%s: F = %lld folds for N = %lld rows", who, (long long)F, (long long)N); return PARTLS_ERR_BAD_ARG; }
        if (fold_ptr[0] != 0 || fold_ptr[F] != N) { set_error("%s: fold_ptr must start at 0 and end at N", who); return PARTLS_ERR_BAD_ARG; }
        for (int64_t g = 0; g < F; ++g)
            if (!(fold_ptr[g] < fold_ptr[g + 1])) { set_error("%s: fold_ptr must be strictly increasing (fold %lld)", who, (long long)g); return PARTLS_ERR_BAD_ARG; }
    }
    if (E < 1 || !eta) { set_error("%s: need E >= 1 eta values", who); return PARTLS_ERR_BAD_ARG; }
    for (int64_t e = 0; e < E; ++e)
        if (!(eta[e] >= 0.0) || !std::isfinite(eta[e])) { set_error("%s: eta[%lld] = %g must be finite and >= 0", who, (long long)e, eta[e]); return PARTLS_ERR_BAD_ARG; }
    if ((F + 1) > ((int64_t)1 << 40) / E) { set_error("%s: too many problems", who); return PARTLS_ERR_BAD_ARG; }
    return PARTLS_OK;
}

}  // namespace partls

using namespace partls;

static partls_status cv_opt(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w,
                            int x_on_device, const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F,
                            const double *eta, int64_t E, uint32_t flags,
                            double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt,
                            int64_t *best_index, double *heldout_sse, int32_t *status)
{
    partls_status st = cv_check_inputs("partls_cv_opt", c, X, N, M, ldX, y, P, K, ldP, fold_ptr, F, eta, E);
    if (st != PARTLS_OK) return st;
    if (!alpha || !beta || !t || !opt || !best_index || !heldout_sse || !status) { set_error("partls_cv_opt: NULL output"); return PARTLS_ERR_BAD_ARG; }
    if (ld_alpha < M || ld_beta < K) { set_error("partls_cv_opt: leading dimension of alpha / beta too small"); return PARTLS_ERR_BAD_ARG; }
    if (flags & PARTLS_OPT_RESCUE_CAPPED) { set_error("partls_cv_opt: PARTLS_OPT_RESCUE_CAPPED is not supported by the batched sweeps"); return PARTLS_ERR_UNSUPPORTED; }
    if ((flags & PARTLS_OPT_FAITHFUL_INTERCEPT ? K + 1 : K) > 40) {
        set_error("partls_cv_opt: K = %lld: the enumeration of fit(Opt) is out of range (K <= 39)", (long long)K);
        return PARTLS_ERR_UNSUPPORTED;
    }
    const int64_t B = (F + 1) * E;
    CvOut o;
    o.assign(B, M, K);
    st = cv_run(c, X, N, M, ldX, y, w, x_on_device, P, K, ldP, fold_ptr, F, eta, E, flags, o);
    if (st != PARTLS_OK) return st;
    o.deliver(B, M, K, alpha, ld_alpha, beta, ld_beta, t, opt, best_index, heldout_sse, status);
    set_error("");
    return PARTLS_OK;
}

partls_status partls_cv_opt(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device,
                            const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F,
                            const double *eta, int64_t E, uint32_t flags,
                            double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt,
                            int64_t *best_index, double *heldout_sse, int32_t *status)
try {
    return cv_opt(c, X, N, M, ldX, y, nullptr, x_on_device, P, K, ldP, fold_ptr, F, eta, E, flags, alpha, ld_alpha, beta, ld_beta, t, opt,
                  best_index, heldout_sse, status);
}
PARTLS_ABI_GUARD

partls_status partls_cv_opt_weighted(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w,
                                     int x_on_device, const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F,
                                     const double *eta, int64_t E, uint32_t flags,
                                     double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt,
                                     int64_t *best_index, double *heldout_sse, int32_t *status)
try {
    return cv_opt(c, X, N, M, ldX, y, w, x_on_device, P, K, ldP, fold_ptr, F, eta, E, flags, alpha, ld_alpha, beta, ld_beta, t, opt,
                  best_index, heldout_sse, status);
}
PARTLS_ABI_GUARD
