/*
 * partls_glm.h — the primitives of a generalised linear fit (logistic, Poisson) by iteratively reweighted least squares on a prepared
 * problem: the working rows of a family at a model, formed on the device; a re-prepare that swaps sample weights AND response of the
 * prepared problem without touching X; the inverse link.  Included by partls.h (include that, not this file): the
 * types, conventions and status codes are partls.h's, and these prototypes sit inside its extern "C" block.  A header of its own for
 * the reason partls_robust.h gives: the entries are bound in SYMBOLS_GLM; tests/test_glm_binding.py checks header, library and table.
 *
 * partls_glm_working.  The problem is the one the context is prepared for (N rows; a double, float or CSR X).  The response y is the one
 * the problem was PREPARED with — not a z that a later partls_opt_rework installed: the context remembers it across reworks, every other
 * prepare forgets it.  The model is (alpha[M], beta[K], t), HOST arrays; eta_i is what partls_predict returns for it on the problem's X,
 * bit for bit.  alpha == NULL && beta == NULL is the start: no pass over X; eta_i is formed from y_i as R's glm.fit forms it,
 *     binomial: m0 = (y + 0.5) / 2, eta = log(m0 / (1 - m0));      Poisson: m0 = y + 0.1, eta = log(m0).
 * Then per row, with xlogy(a) = a == 0 ? 0 : a log(a) and ec = min(max(eta, -30), 30), every line one IEEE fp64 operation or one call of
 * exp / log / log1p, in this order, without contraction:
 *   PARTLS_GLM_BINOMIAL (logit link, 0 <= y <= 1):
 *     e = exp(-|ec|), q = 1 / (1 + e), p = e q;   mu = ec >= 0 ? q : p  (nu = ec >= 0 ? p : q is 1 - mu without cancellation)
 *     W = p q;   z = ec + (y - mu) / W
 *     l = log1p(e);   nlmu = ec >= 0 ? l : |ec| + l;   nlnu = ec >= 0 ? |ec| + l : l          (-log mu, -log nu)
 *     d = 2 ((xlogy(y) + xlogy(1 - y)) + (y nlmu + (1 - y) nlnu))
 *   PARTLS_GLM_POISSON (log link, y >= 0):
 *     mu = exp(ec);   W = mu;   z = ec + (y - mu) / mu;   d = 2 ((xlogy(y) - y ec) - (y - mu))
 * The clamp keeps W >= e^-30 / (1 + e^-30)^2 > 9.3e-14 > 0, so a working weight always passes the checks of sample weights and a
 * separable logistic problem ends instead of overflowing.
 *   outputs (each pointer optional): *deviance = sum_i d_i — consecutive blocks of 1024 rows, each summed by a fixed tree, the block
 *   sums added in ascending order from 0.0 on the host, no floating-point atomics: two calls return the same bits;  *max_abs_eta =
 *   max_i |eta_i| BEFORE the clamp (exact);  *n_clamped = #{eta_i != ec_i};  w_out, z_out, mu_out: the N working weights, working
 *   responses and means — HOST arrays after a prepare from host pointers, DEVICE addresses after a prepare from device pointers (the
 *   convention of partls_robust_weights).  W and z are also kept in buffers of the context for partls_opt_rework.
 *   The prepared problem is untouched: a sweep after the call returns what it returned before.
 *   The first call of a family after a prepare checks y on the device before anything is written: a NaN / Inf, a binomial y outside
 *   [0, 1] or a Poisson y < 0 -> PARTLS_ERR_BAD_ARG, the message names the first offending row.
 *   Other errors, also found before anything is written: PARTLS_ERR_BAD_ARG without a prepared problem, for exactly one of alpha / beta
 *   NULL, a NaN / Inf in alpha, beta or t, an unknown family; PARTLS_ERR_UNSUPPORTED on a context of a partls_multi.
 *
 * Error bound of a row (tests/test_gpu_glm.py uses these constants; tests/test_glm_binding.py holds a numpy restatement to them).
 * u = PARTLS_GLM_U = 2^-53: an arithmetic operation errs by at most u relative (half an ulp); exp, log and log1p err by at most 1 ulp
 * <= 2u relative (the documented maximum of the HIP math API in fp64).  First-order terms are counted and one unit is added for the
 * higher orders.  With eta given exactly (a model):
 *   binomial.  e: 2u.  1 + e: u; the error of e enters q = 1 / (1 + e) with the factor e / (1 + e) <= 1/2: q: u + u + u = 3u.
 *     p = e q: 2 + 3 + 1 = 6u.  mu, nu: <= 6u.  W = p q: 6 + 3 + 1 = 10u.
 *     z: the numerator y - mu errs by 6u mu + u |y - mu| <= 7u (|y| + mu) absolutely — the subtraction cancels, so the bound is in its
 *     operands; the quotient adds (10 + 1)u of itself: <= 18u (|y| + mu) / W; the last addition adds u |z| <= u (|ec| + (|y| + mu) / W):
 *     19u (|ec| + (|y| + mu) / W).
 *     d: l = log1p(e): 2u + the 2u of e times e / ((1 + e) log1p(e)) <= 1: 4u.  |ec| + l: 5u.  y nlmu: 6u; 1 - y: u (exact for y == 0 and
 *     for y >= 1/2), (1 - y) nlnu: 7u; their sum: 8u.  xlogy(y): 3u.  xlogy(a) at a = fl(1 - y): 3u, and the error of a moves it by
 *     |log a + 1| u a <= u (|xlogy(a)| + a); the sum of the two: 5u.  The outer addition: 9u — of S = |xlogy(y)| + |xlogy(1 - y)| +
 *     r + y nlmu + (1 - y) nlnu with r = 1 - y where that subtraction can round (0 < y < 1/2), else 0.  For y in {0, 1} S is d / 2: the
 *     bound is relative.
 *   Poisson.  mu = W = exp(ec): 2u.  z: numerator 2u mu + u |y - mu| <= 3u (|y| + mu), quotient + (2 + 1)u, addition + u: 8u (|ec| + (|y| + mu) / W).
 *     d: xlogy(y): 3u, y ec: u, their difference: 4u; y - mu: 3u of its operands; the outer subtraction: 5u of
 *     S = |xlogy(y)| + |y ec| + |y| + mu.
 *   One set of constants covers both families:
 *     |mu^ - mu| <= MU u mu;   |W^ - W| <= W_ u W;   |z^ - z| <= Z u (|ec| + (|y| + mu) / W);   |d^ - d| <= D u 2 S.
 *   The start forms eta itself: binomial, three roundings in front of the log and the log's own 2u |eta|; Poisson, one:
 *     |eta^ - eta| <= de = (START_ETA + 2 |eta|) u (absolutely: eta may be 0).  By the derivatives d mu / d eta = mu nu (W for Poisson),
 *     |d W / d eta| <= W, |d z / d eta| <= 1 + (|y| + mu) / W, d d / d eta = 2 (mu - y), the start's bounds are the ones above plus
 *     de mu, de W, de (1 + (|y| + mu) / W) and 2 de (|y| + mu).
 *
 * partls_opt_rework.  Replaces the sample weights of the prepared problem by w[N] and its response by z[N] (host arrays, or device
 * addresses when on_device) and rebuilds the Gram products and the tableau.  w == NULL && z == NULL: the rows of the last
 * partls_glm_working call on this context, copied into buffers the problem owns (PARTLS_ERR_STATE when there was no such call since
 * the last prepare).  z == NULL, w given: partls_opt_reweight — the two entries are one function.  z given without w:
 * PARTLS_ERR_BAD_ARG.  X, P, eta and the flags stay; nothing is uploaded except host w / z.  The context is then, bit for bit, in the
 * state partls_opt_prepare_weighted (or its _f32 / _csr form) would leave it in with response z and weights w — partls_get_gram, every
 * sweep, every finish, Alt and BnB — except that it still remembers the response it was first prepared with, and the records of
 * partls_glm_working and partls_robust_weights.  Device w / z must stay valid while the context holds the problem.  A refused call
 * names its reason in partls_last_error and leaves the context unprepared, as a refused prepare does.  PARTLS_ERR_STATE without a
 * prepared problem; PARTLS_ERR_UNSUPPORTED on a context of a partls_multi.
 *
 * partls_glm_mean.  mu[i] = the inverse link of the family at eta[i], i < N, by the device function of the row kernel, clamp included
 * (the same bits as mu_out for the same eta).  eta and mu: host arrays, or device addresses when on_device.  Needs no prepared problem.
 */
#ifndef PARTLS_GLM_H
#define PARTLS_GLM_H
#ifndef PARTLS_H
#error "include partls.h, which includes this header"
#endif

#define PARTLS_GLM_BINOMIAL 0
#define PARTLS_GLM_POISSON 1
#define PARTLS_GLM_CLAMP 30.0
/* the row bound above, in units of PARTLS_GLM_U = 2^-53 (first-order count + 1) */
#define PARTLS_GLM_U 1.1102230246251565e-16
#define PARTLS_GLM_MU_ULPS 7
#define PARTLS_GLM_W_ULPS 11
#define PARTLS_GLM_Z_ULPS 20
#define PARTLS_GLM_D_ULPS 10
#define PARTLS_GLM_START_ETA_ULPS 4
partls_status partls_glm_working(partls_ctx *ctx, const double *alpha, const double *beta, double t, int family, double *deviance,
                                 double *max_abs_eta, int64_t *n_clamped, double *w_out, double *z_out, double *mu_out);
partls_status partls_opt_rework(partls_ctx *ctx, const double *w, const double *z, int on_device);
partls_status partls_glm_mean(partls_ctx *ctx, int family, const double *eta, int64_t N, int on_device, double *mu);
/* where the last partls_glm_working call on the context spent its device time, in ms (tools/glm_timing.py): the residual pass (0 for
 * the start), the row kernel.  Zeros before the first call. */
partls_status partls_get_glm_timing(const partls_ctx *ctx, double *residual_ms, double *rows_ms);

#endif
