// refine.hip — the data-space half of a fit: passes over X (objective, gradient), the KKT check of a winner and its iterative
// refinement (final tableau of the node solve, or a host Cholesky of the Gram copy).
#include "ctx.h"
#include "prepare_rules.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <functional>

namespace partls {

void unscale_solution(const partls_ctx *c, const double *sol, std::vector<double> &w)
{
    const int M = (int)c->M;
    w.assign((size_t)M + 1, 0.0);
    for (int i = 0; i < c->n; ++i) w[(size_t)c->perm[(size_t)i]] = sol[i] * c->hScale[(size_t)i];
    if (!c->faithful) {
        // intercept eliminated up front: t = (c_I - sum_f G_If w_f) / G_II   (row I of the normal equations)
        double s = h_reg(c, M, M + 1);
        for (int f = 0; f < M; ++f) s -= h_reg(c, M, f) * w[(size_t)f];
        w[(size_t)M] = s / h_reg(c, M, M);
    }
}

// One pass over the DATA of the prepared problem — all of it: this context's rows and, when the rows of X are sharded over several
// devices (partls_fit_opt_multi), those its peers hold:  *obj2 = sum_i (Xo w - y)_i^2  (without the eta rows) and, optionally,
// g = Xo'(y - Xo w) over [features, intercept].  With sample weights (q->dw) the rows are weighted: sum_i w_i r_i^2 and Xo' W r.  The kernels of every device are queued first (one host thread drives them all), the
// caller's `overlap` work runs on the host meanwhile, then the partial sums are added in a fixed order (context, then peers; slices in
// order): run-to-run reproducible.
partls_status data_pass(partls_ctx *c, const std::vector<double> &w, bool want_obj, bool want_grad, double *obj2, std::vector<double> *g,
                        const std::function<void()> &overlap)
{
    const int64_t M = c->M;
    const int nb = 1024;
    std::vector<partls_ctx *> cs{c};
    cs.insert(cs.end(), c->peers.begin(), c->peers.end());
    for (partls_ctx *q : cs) {
        PARTLS_HIP_CHECK(hipSetDevice(q->device));
        const int64_t N = q->N;
        const int xr = xtr_slices(N);
        PARTLS_HIP_CHECK(q->wdev.ensure((size_t)(M + 1) * sizeof(double)));
        PARTLS_HIP_CHECK(hipMemcpyAsync(q->wdev.p, w.data(), (size_t)(M + 1) * sizeof(double), hipMemcpyHostToDevice, q->stream));
        double *yhat = nullptr;
        if (want_obj) { PARTLS_HIP_CHECK(q->partial.ensure(nb * sizeof(double))); PARTLS_HIP_CHECK(q->hPart.resize((size_t)nb)); }
        if (want_grad) {
            PARTLS_HIP_CHECK(q->yhatD.ensure((size_t)N * sizeof(double)));
            PARTLS_HIP_CHECK(q->gD.ensure((size_t)xr * (M + 1) * sizeof(double)));
            yhat = q->yhatD.as<double>();
            PARTLS_HIP_CHECK(q->hGpart.resize((size_t)xr * (M + 1)));
        }
        // the two kernels by the storage of X (a sparse X: csr.hip, the same outputs and fold rules)
        const bool sparse = q->storage == XStorage::csr;
        if (sparse)
            PARTLS_HIP_CHECK(launch_csr_residual(q->csr, want_obj ? q->dy : nullptr, q->wdev.as<double>(), w[(size_t)M],
                                                 want_obj ? q->partial.as<double>() : nullptr, nb, yhat, q->stream, q->dw));
        else
            PARTLS_HIP_CHECK(launch_residual(q->dX, N, M, q->ldX, want_obj ? q->dy : nullptr, q->wdev.as<double>(), w[(size_t)M],
                                             want_obj ? q->partial.as<double>() : nullptr, nb, yhat, q->stream, q->dw, q->x_f32));
        if (want_grad) {
            if (sparse) PARTLS_HIP_CHECK(launch_csr_xtr(q->csc, N, M, q->dy, yhat, q->gD.as<double>(), q->stream, q->dw));
            else PARTLS_HIP_CHECK(launch_xtr(q->dX, N, M, q->ldX, q->dy, yhat, q->gD.as<double>(), q->stream, q->dw, q->x_f32));
            PARTLS_HIP_CHECK(hipMemcpyAsync(q->hGpart.data(), q->gD.p, q->hGpart.size() * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        }
        if (want_obj) PARTLS_HIP_CHECK(hipMemcpyAsync(q->hPart.data(), q->partial.p, nb * sizeof(double), hipMemcpyDeviceToHost, q->stream));
    }
    if (overlap) overlap();
    double s = 0.0;
    if (want_grad) g->assign((size_t)M + 1, 0.0);
    for (partls_ctx *q : cs) {
        PARTLS_HIP_CHECK(hipSetDevice(q->device));
        PARTLS_HIP_CHECK(hipStreamSynchronize(q->stream));
        if (want_obj) for (int b = 0; b < nb; ++b) s += q->hPart[(size_t)b];
        if (want_grad) {
            const int xr = xtr_slices(q->N);
            for (int64_t m = 0; m <= M; ++m) {
                double sg = 0.0;
                for (int r = 0; r < xr; ++r) sg += q->hGpart[(size_t)r * (M + 1) + m];
                (*g)[(size_t)m] += sg;
            }
        }
    }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    if (want_obj) *obj2 = s;
    return PARTLS_OK;
}

// the eta rows of regularizeProblem (PartitionedLS.jl:108-123): sqrt(eta) * sum_{m in group k} w_m  ->  their share of obj^2 and of g
static void eta_terms(const partls_ctx *c, const std::vector<double> &w, double *obj2, std::vector<double> *grad)
{
    if (c->eta == 0.0) return;
    const int64_t M = c->M;
    for (int64_t k = 0; k <= c->K; ++k) {
        double gs = 0.0;
        for (int64_t m = 0; m <= M; ++m) if (c->mask_aug[(size_t)m] & (1ULL << k)) gs += w[(size_t)m];
        if (obj2) *obj2 += c->eta * gs * gs;
        if (grad) for (int64_t m = 0; m <= M; ++m) if (c->mask_aug[(size_t)m] & (1ULL << k)) (*grad)[(size_t)m] -= c->eta * gs;
    }
}

partls_status data_objective(partls_ctx *c, const std::vector<double> &w, double *opt, std::vector<double> *grad)
{
    double s = 0.0;
    partls_status st = data_pass(c, w, true, grad != nullptr, &s, grad, {});
    if (st != PARTLS_OK) return st;
    eta_terms(c, w, &s, grad);
    *opt = std::sqrt(s);
    return PARTLS_OK;
}

// When is a data-space KKT violation evidence that the Gram form has lost the problem?  Measured on problems of cond(Xo) 7e2 .. 8e7
// (tools/illcond_check.py, three seeds, Opt and BnB): every fit that equals the oracle's has a violation <= 3e-15 (the rounding of the
// data passes: eps * sqrt(N) * ||r|| / ||y||), every fit that differs from it has one >= 1.2e-11 — the residual gradient along a nearly
// dependent column the tableau could not resolve (d ~ 1e-13: worth g^2 / d in the objective, i.e. the whole difference to the reference's
// model).  The threshold sits between the two bands.  Neither the pivots of the final basis nor the refusals of the sweep separate the
// cases (a basis that avoids the nearly dependent columns is perfectly conditioned), so the violation alone decides.  The cost of the
// tight threshold: a well-conditioned optimum with a variable at its bound whose gradient lies within (1e-12, 1e-11] * ||x|| ||y|| of zero
// — inside the sweep's own tolerance — is reported although it is fine; on continuous data that has probability ~1e-8 per variable.
bool kkt_says_ill_conditioned(const partls_ctx *c)
{
    return c->last_kkt > c->knobs.kkt_tol;
}

double kkt_violation_data(const partls_ctx *c, const std::vector<double> &w, const std::vector<double> &g, const std::vector<int8_t> &code,
                          int *worst)
{
    const int M = (int)c->M;
    const double yy = h_reg(c, M + 1, M + 1);
    const double ynorm = std::sqrt(yy > 0.0 ? yy : 0.0);
    double worstv = 0.0, wmax = 0.0;
    for (int m = 0; m <= M; ++m) wmax = std::max(wmax, std::fabs(w[(size_t)m]));
    if (worst) *worst = -1;
    for (int m = 0; m <= M; ++m) {
        const double d = h_reg(c, m, m);
        if (!column_is_live(d, c->hG[(size_t)m * c->ldg + m])) continue;                       // null column: never in any basis
        const double gs = g[(size_t)m] / (std::sqrt(d) * (ynorm > 0.0 ? ynorm : 1.0));
        const int f = code[(size_t)m];
        double v = 0.0;
        if (f == 2 || w[(size_t)m] != 0.0) v = std::fabs(gs);
        else if (f != 0) v = std::max(0.0, (double)f * gs);
        if (f == 1 || f == -1) v = std::max(v, wmax > 0.0 ? std::max(0.0, -(double)f * w[(size_t)m] / wmax) : 0.0);
        if (v > worstv) { worstv = v; if (worst) *worst = m; }
    }
    return worstv;
}

// Row-oriented Cholesky of a dense SPD matrix, in place (lower triangle, row-major, leading dimension p): L[i][j] = (B[i][j] - <L[i][:j],
// L[j][:j]>) / L[j][j].  The inner products run on 2 x 4 AVX2 lanes where the host has them (every host an MI355X ships in; checked at
// run time) — 358 k multiply-adds at p = 129 in ~25 us instead of ~100: short enough to hide behind the first data pass of the refinement.
// The sums are taken in a fixed order per build target (reproducible run to run; the correction they serve is ~1e-15 of the solution).
#if defined(__x86_64__)
#include <immintrin.h>
// 4 rows x 2 columns at a time: L[i][j] for i = i0..i0+3 and j = j0, j0+1 share the six row loads of a k-step (0.75 loads per FMA instead of
// 2: the plain dot-product form streams the whole factor from L2 once per row — 45 MB at p = 256, which is what bounded it at ~5 GFLOP/s).
__attribute__((target("avx2,fma"))) static inline double hsum4(__m256d v)
{
    double t[4];
    _mm256_storeu_pd(t, v);
    return (t[0] + t[1]) + (t[2] + t[3]);
}
__attribute__((target("avx2,fma"))) static bool chol_rows_avx2(double *L, int p)
{
    int i0 = 0;
    for (; i0 + 3 < p; i0 += 4) {
        double *R0 = L + (size_t)i0 * p, *R1 = R0 + p, *R2 = R1 + p, *R3 = R2 + p;
        // columns strictly before the diagonal block, two at a time
        int j = 0;
        for (; j + 1 < i0; j += 2) {
            const double *C0 = L + (size_t)j * p, *C1 = C0 + p;
            __m256d a00 = _mm256_setzero_pd(), a01 = a00, a10 = a00, a11 = a00, a20 = a00, a21 = a00, a30 = a00, a31 = a00;
            int k = 0;
            for (; k + 3 < j; k += 4) {
                const __m256d c0 = _mm256_loadu_pd(C0 + k), c1 = _mm256_loadu_pd(C1 + k);
                const __m256d r0 = _mm256_loadu_pd(R0 + k), r1 = _mm256_loadu_pd(R1 + k), r2 = _mm256_loadu_pd(R2 + k), r3 = _mm256_loadu_pd(R3 + k);
                a00 = _mm256_fmadd_pd(r0, c0, a00); a01 = _mm256_fmadd_pd(r0, c1, a01);
                a10 = _mm256_fmadd_pd(r1, c0, a10); a11 = _mm256_fmadd_pd(r1, c1, a11);
                a20 = _mm256_fmadd_pd(r2, c0, a20); a21 = _mm256_fmadd_pd(r2, c1, a21);
                a30 = _mm256_fmadd_pd(r3, c0, a30); a31 = _mm256_fmadd_pd(r3, c1, a31);
            }
            double d[4][2] = {{hsum4(a00), hsum4(a01)}, {hsum4(a10), hsum4(a11)}, {hsum4(a20), hsum4(a21)}, {hsum4(a30), hsum4(a31)}};
            double *R[4] = {R0, R1, R2, R3};
            for (int a = 0; a < 4; ++a) {
                for (int kk = k; kk < j; ++kk) { d[a][0] += R[a][kk] * C0[kk]; d[a][1] += R[a][kk] * C1[kk]; }
                const double l0 = (R[a][j] - d[a][0]) / C0[j];
                R[a][j] = l0;
                R[a][j + 1] = (R[a][j + 1] - (d[a][1] + l0 * C1[j])) / C1[j + 1];       // column j + 1 also needs the entry of column j just made
            }
        }
        // the odd column before the block, then the 4 x 4 diagonal block: plain
        for (int a = 0; a < 4; ++a) {
            double *Ri = L + (size_t)(i0 + a) * p;
            for (int jj = j; jj <= i0 + a; ++jj) {
                const double *Cj = L + (size_t)jj * p;
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
                int k = 0;
                for (; k + 3 < jj; k += 4) { s0 += Ri[k] * Cj[k]; s1 += Ri[k + 1] * Cj[k + 1]; s2 += Ri[k + 2] * Cj[k + 2]; s3 += Ri[k + 3] * Cj[k + 3]; }
                for (; k < jj; ++k) s0 += Ri[k] * Cj[k];
                const double sv = Ri[jj] - ((s0 + s1) + (s2 + s3));
                if (jj == i0 + a) { if (!(sv > 0.0)) return false; Ri[jj] = std::sqrt(sv); }
                else Ri[jj] = sv / Cj[jj];
            }
        }
    }
    for (int i = i0; i < p; ++i) {                           // the last p mod 4 rows
        double *Li = L + (size_t)i * p;
        for (int j = 0; j <= i; ++j) {
            const double *Lj = L + (size_t)j * p;
            double s0 = 0.0, s1 = 0.0;
            int k = 0;
            for (; k + 1 < j; k += 2) { s0 += Li[k] * Lj[k]; s1 += Li[k + 1] * Lj[k + 1]; }
            for (; k < j; ++k) s0 += Li[k] * Lj[k];
            const double sv = Li[j] - (s0 + s1);
            if (i == j) { if (!(sv > 0.0)) return false; Li[i] = std::sqrt(sv); }
            else Li[j] = sv / Lj[j];
        }
    }
    return true;
}
#endif
static bool chol_rows_plain(double *L, int p)
{
    for (int i = 0; i < p; ++i) {
        double *Li = L + (size_t)i * p;
        for (int j = 0; j <= i; ++j) {
            const double *Lj = L + (size_t)j * p;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int k = 0;
            for (; k + 3 < j; k += 4) { s0 += Li[k] * Lj[k]; s1 += Li[k + 1] * Lj[k + 1]; s2 += Li[k + 2] * Lj[k + 2]; s3 += Li[k + 3] * Lj[k + 3]; }
            for (; k < j; ++k) s0 += Li[k] * Lj[k];
            const double s = Li[j] - ((s0 + s1) + (s2 + s3));
            if (i == j) { if (!(s > 0.0)) return false; Li[i] = std::sqrt(s); }
            else Li[j] = s / Lj[j];
        }
    }
    return true;
}
bool chol_rows(double *L, int p)
{
#if defined(__x86_64__)
    static const bool fast = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    if (fast) return chol_rows_avx2(L, p);
#endif
    return chol_rows_plain(L, p);
}

partls_status refine_solution(partls_ctx *c, std::vector<double> &w, bool free_intercept, int steps, RefineOut *out)
{
    const int64_t M = c->M;
    if (out) out->have = false;
    std::vector<int> sup;
    for (int m = 0; m <= (int)M; ++m)
        if (w[(size_t)m] != 0.0 || (m == (int)M && free_intercept)) sup.push_back(m);
    const int p = (int)sup.size();
    if (p == 0) return PARTLS_OK;
    // Solver of the correction equations.  With the final tableau of the node solve at hand (register kernel), its basic x basic
    // block is -(D B_BB D)^-1 (D = unit-diagonal scaling, B = regularised Gram, with the free intercept already eliminated by its
    // Schur complement): delta_B = -D T_BB D rhs is one p x p matrix-vector product per step instead of a p^3/6 factorisation.
    // Valid when the basis IS the support (a basic variable that came out exactly 0 would not be in `sup`): otherwise Cholesky.
    std::vector<int> tabsup;                             // tableau indices of the support, when the tableau path applies
    // conditioning of the basis the node solve ended on, while its tableau is at hand: the diagonal of the basic block is -1 / (leave-one-out
    // pivot of that variable), so the smallest leave-one-out pivot is a lower bound of 1 / cond(G~_BB)  (0 = unknown: no tableau)
    c->last_min_loo = 0.0;
    if (c->tab_valid) {
        double tmax = 0.0;
        for (int i = 0; i < c->n; ++i) {
            if (!c->hBasic[i]) continue;
            const int ti = i >> 4, a = i & 15;
            const double d = c->tab_full ? c->hTab[(size_t)i * (c->n + 1) + i] : c->hTab[((size_t)(ti * (ti + 1) / 2 + ti)) * 256 + a + 16 * a];
            tmax = std::max(tmax, std::fabs(d));
        }
        c->last_min_loo = tmax > 0.0 ? 1.0 / tmax : 1.0;
    }
    bool use_tab = c->tab_valid && free_intercept == !c->faithful && !c->knobs.no_tab_refine;
    c->tab_valid = false;                                // one use: the next node solve overwrites the buffers
    if (use_tab) {
        std::vector<int> inv_perm((size_t)M + 1, -1);
        for (int i = 0; i < c->n; ++i) inv_perm[(size_t)c->perm[(size_t)i]] = i;
        int nb = 0;
        for (int i = 0; i < c->n; ++i) nb += c->hBasic[i] ? 1 : 0;
        for (int m : sup) {
            if (m == (int)M && !c->faithful) continue;   // free intercept: eliminated from the tableau, recovered below
            const int i = inv_perm[(size_t)m];
            if (i < 0 || !c->hBasic[i]) { use_tab = false; break; }
            tabsup.push_back(i);
        }
        if ((int)tabsup.size() != nb) use_tab = false;
    }
    const bool tab_full = c->tab_full;
    const int tld = c->n + 1;
    std::vector<double> g((size_t)M + 1), d((size_t)p);
    // `out`: the pass that finds the correction negligible has already computed the squared residual and Xo'(yo - Xo w) one tiny step
    // before the final w; both are carried over exactly (obj^2 -= 2 g'delta, g -= B delta with the host Gram copy) instead of being
    // recomputed by two more passes over X
    std::vector<double> delta;
    if (out) delta.assign((size_t)M + 1, 0.0);
    double obj2_pre = 0.0;
    auto finish_out = [&]() {                                 // w = w_pre + delta, delta tiny: first-order update of (obj^2, g)
        double o2 = obj2_pre;
        for (int64_t m = 0; m <= M; ++m) o2 -= 2.0 * g[(size_t)m] * delta[(size_t)m];
        out->g = g;
        for (int64_t j = 0; j <= M; ++j) {
            const double dj = delta[(size_t)j];
            if (dj == 0.0) continue;
            const double *row = c->hG.data() + (size_t)j * c->ldg;          // row j of the symmetric Gram copy: contiguous
            double *og = out->g.data();
            for (int64_t m = 0; m <= M; ++m) og[m] -= row[m] * dj;
            if (c->eta != 0.0) {
                const uint64_t mj = c->mask_aug[(size_t)j];
                for (int64_t m = 0; m <= M; ++m) og[m] -= c->eta * (double)__builtin_popcountll(c->mask_aug[(size_t)m] & mj) * dj;
            }
        }
        out->obj = std::sqrt(o2 > 0.0 ? o2 : 0.0);
        out->have = true;
    };
    std::vector<double> Lc;                                  // Cholesky factor: allocated only when that path runs
    // row-oriented Cholesky of the regularised Gram on the support (host copy); the inner products carry four independent
    // partial sums so the compiler can vectorise them (the support is all of [features, intercept] in the typical case:
    // p^3 / 6 multiply-adds).  It runs while the device computes the first residual and gradient.
    auto factorise = [&]() -> bool {
        Lc.assign((size_t)p * p, 0.0);
        for (int i = 0; i < p; ++i) {                        // the regularised Gram block of the support, lower triangle
            const double *row = c->hG.data() + (size_t)sup[(size_t)i] * c->ldg;
            double *Li = &Lc[(size_t)i * p];
            for (int j = 0; j <= i; ++j) Li[j] = row[sup[(size_t)j]];
            if (c->eta != 0.0) {
                const uint64_t mi = c->mask_aug[(size_t)sup[(size_t)i]];
                for (int j = 0; j <= i; ++j) Li[j] += c->eta * (double)__builtin_popcountll(mi & c->mask_aug[(size_t)sup[(size_t)j]]);
            }
        }
        return chol_rows(Lc.data(), p);
    };
    const auto r0 = std::chrono::steady_clock::now();
    for (int it = 0; it < steps; ++it) {
        bool spd = true;
        // residual (and squared residual) and gradient on the device(s); the Cholesky factorisation, when it is needed, overlaps with them
        // (round 4 tried to skip the factorisation when the data-space gradient on the support is rounding noise already — C2: 2.6e-16 of
        // ||x|| ||y|| — and took it back: a tiny gradient says nothing about the error along a weak direction of the Gram block (error =
        // gradient / lambda_min: at cond(Xo) = 8e4 a gradient of 1e-16 goes with an error of 1e-7, exactly the case the refinement exists
        // for; found by test_ill_conditioned_model_parity under a forced bit-order calibration).  The factorisation is made cheap instead.)
        partls_status dst = data_pass(c, w, out != nullptr, true, &obj2_pre, &g, [&]() { if (it == 0 && !use_tab) spd = factorise(); });
        if (dst != PARTLS_OK) return dst;
        if (out) {
            eta_terms(c, w, &obj2_pre, nullptr);
            std::fill(delta.begin(), delta.end(), 0.0);
        }
        eta_terms(c, w, nullptr, &g);                        // gradient of the η rows: -eta * sum_k 1_k (1_k' w)
        if (!spd) return PARTLS_OK;                          // not numerically SPD: give up quietly, w unchanged
        if (use_tab) {
            const int nb = (int)tabsup.size();
            const bool elim = !c->faithful;                  // free intercept: rhs and solution go through its Schur complement
            const double gII = elim ? h_reg(c, (int)M, (int)M) : 1.0, gI = g[(size_t)M];
            std::vector<double> rhs((size_t)nb), ds((size_t)nb);
            for (int a = 0; a < nb; ++a) {
                const int i = tabsup[(size_t)a], m = c->perm[(size_t)i];
                double r = g[(size_t)m];
                if (elim) r -= h_reg(c, m, (int)M) * gI / gII;
                rhs[(size_t)a] = r * c->hScale[(size_t)i];
            }
            // y = T x over ALL tableau indices with x = 0 outside the basis (only the basic entries of y are used): contiguous inner
            // loops over the stored layout instead of p^2 indexed look-ups (100 us at p = 256)
            const int nt_ = tab_full ? 0 : c->T, nx = tab_full ? c->n : 16 * c->T;
            std::vector<double> xt((size_t)nx, 0.0), yt((size_t)nx, 0.0);
            for (int a = 0; a < nb; ++a) xt[(size_t)tabsup[(size_t)a]] = rhs[(size_t)a];
            if (tab_full) {
                for (int a = 0; a < nb; ++a) {
                    const double *row = c->hTab + (size_t)tabsup[(size_t)a] * tld;
                    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
                    int j = 0;
                    for (; j + 3 < nx; j += 4) { s0 += row[j] * xt[(size_t)j]; s1 += row[j + 1] * xt[(size_t)j + 1]; s2 += row[j + 2] * xt[(size_t)j + 2]; s3 += row[j + 3] * xt[(size_t)j + 3]; }
                    for (; j < nx; ++j) s0 += row[j] * xt[(size_t)j];
                    yt[(size_t)tabsup[(size_t)a]] = (s0 + s1) + (s2 + s3);
                }
            } else {
                for (int tj = 0; tj < nt_; ++tj)
                    for (int ti = 0; ti <= tj; ++ti) {                     // stored tiles: element (16 ti + a, 16 tj + b) at [a + 16 b]
                        const double *tile = c->hTab + ((size_t)(tj * (tj + 1) / 2 + ti)) * 256;
                        double *yi = &yt[(size_t)16 * ti], *yj = &yt[(size_t)16 * tj];
                        const double *xi = &xt[(size_t)16 * ti], *xj = &xt[(size_t)16 * tj];
                        for (int b = 0; b < 16; ++b) {
                            const double xb = xj[b];
                            double sj = 0.0;
                            for (int a = 0; a < 16; ++a) { const double v = tile[a + 16 * b]; yi[a] += v * xb; sj += v * xi[a]; }
                            if (ti != tj) yj[b] += sj;                     // the mirrored tile (a diagonal tile is stored whole)
                        }
                    }
            }
            for (int a = 0; a < nb; ++a) {
                ds[(size_t)a] = -yt[(size_t)tabsup[(size_t)a]];
            }
            double dn = 0.0, wn = 0.0, dI = gI;
            for (int a = 0; a < nb; ++a) {
                const int i = tabsup[(size_t)a], m = c->perm[(size_t)i];
                const double dl = ds[(size_t)a] * c->hScale[(size_t)i];
                if (elim) dI -= h_reg(c, (int)M, m) * dl;
                w[(size_t)m] += dl; dn += dl * dl; wn += w[(size_t)m] * w[(size_t)m];
                if (out) delta[(size_t)m] = dl;
            }
            if (elim) { dI /= gII; w[(size_t)M] += dI; dn += dI * dI; wn += w[(size_t)M] * w[(size_t)M]; if (out) delta[(size_t)M] = dI; }
            if (c->knobs.finish_trace) fprintf(stderr, "[refine] step %d: |delta|/|w| = %.3e\n", it, std::sqrt(dn / (wn > 0 ? wn : 1)));
            if (dn <= 1e-18 * wn) { if (out) finish_out(); break; }
            continue;
        }
        for (int i = 0; i < p; ++i) {                        // L z = g_P
            double s = g[(size_t)sup[(size_t)i]];
            for (int k = 0; k < i; ++k) s -= Lc[(size_t)i * p + k] * d[(size_t)k];
            d[(size_t)i] = s / Lc[(size_t)i * p + i];
        }
        for (int i = p - 1; i >= 0; --i) {                   // L' delta = z
            double s = d[(size_t)i];
            for (int k = i + 1; k < p; ++k) s -= Lc[(size_t)k * p + i] * d[(size_t)k];
            d[(size_t)i] = s / Lc[(size_t)i * p + i];
        }
        double dn = 0.0, wn = 0.0;
        for (int i = 0; i < p; ++i) { w[(size_t)sup[(size_t)i]] += d[(size_t)i]; dn += d[(size_t)i] * d[(size_t)i]; wn += w[(size_t)sup[(size_t)i]] * w[(size_t)sup[(size_t)i]]; if (out) delta[(size_t)sup[(size_t)i]] = d[(size_t)i]; }
        if (c->knobs.finish_trace) {
            double gmax = 0.0;
            const double yy = h_reg(c, (int)M + 1, (int)M + 1);
            for (int i = 0; i < p; ++i) { const int m = sup[(size_t)i]; const double dd = h_reg(c, m, m); if (dd > 0.0 && yy > 0.0) gmax = std::max(gmax, std::fabs(g[(size_t)m]) / std::sqrt(dd * yy)); }
            fprintf(stderr, "[refine] step %d (Cholesky): |delta|/|w| = %.3e, max |g_S| / (|x||y|) before it = %.3e\n", it, std::sqrt(dn / (wn > 0 ? wn : 1)), gmax);
        }
        // the iteration contracts by cond^2 eps per step: once a correction is below 1e-9 relative, the next one is below
        // round-off for every problem the Gram path can solve at all
        if (dn <= 1e-18 * wn) { if (out) finish_out(); break; }
    }
    if (c->knobs.finish_trace)
        fprintf(stderr, "[refine] support %d: %.3f ms (factorisation overlapped with the first residual / gradient pass)\n", p,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r0).count());
    return PARTLS_OK;
}

}  // namespace partls
