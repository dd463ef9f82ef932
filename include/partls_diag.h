/*
 * partls_diag.h — regression diagnostics of one model on the context's prepared problem: leverage, leave-one-out residuals,
 * studentized residuals, Cook's distances, degrees of freedom and standard errors.  Included by partls.h (include
 * that, not this file): the types, conventions and status codes are partls.h's, and these prototypes sit inside its extern "C" block.
 *
 * Why a header of its own: tests/test_abi.py reads partls.h as the list of the symbols of the main ctypes table (SYMBOLS, _lib.py).
 * That test stays as it is, so the entries below are declared here and bound in SYMBOLS_DIAG; tests/test_diagnostics_binding.py
 * applies the header / library / table / ccall checks to them.
 *
 * The contract.  The problem is the one the context is prepared for: X (N x M), y, optional row weights w_i (else 1), the partition P
 * and eta.  The model is (alpha[M], beta[K], t), HOST arrays.  u = 2^-53 below.
 *   v_m = alpha_m * sum_k P[m,k] beta_k (m < M), v_M = t;  Xo = [X 1];  A = {m < M : v_m != 0} u {M}, ascending, p = |A|
 *   H = Xo_A' W Xo_A + eta Q_A = L L'   with Q = sum_{k = 0..K} p_k p_k' the penalty of regularizeProblem (the intercept's group
 *       included), B = Xo_A' W Xo_A taken from the Gram products of the prepare (X is not read again for it)
 *   leverage_i    = w_i ||L^-1 x_iA||^2                   (a sum of squares: never negative; 0 for a row of weight 0)
 *   residual_i    = y_i - yhat_i, yhat what partls_predict returns for the model, bit for bit
 *   loo_i         = residual_i / (1 - leverage_i)         (plain IEEE: no special case at leverage 1) — by Sherman-Morrison the
 *                   residual of row i under the model refitted without row i on the same sign pattern and support
 *   studentized_i = sqrt(w_i) residual_i / sqrt(sigma2 (1 - leverage_i))
 *   cooks_i       = studentized_i^2 leverage_i / (dof (1 - leverage_i))
 *   summary[PARTLS_DIAG_...]: NPLUS = rows with w_i > 0;  P = p;  DOF = sum_i leverage_i;  RSS = sum_i w_i residual_i^2;
 *       PRESS = sum_i w_i loo_i^2;  SIGMA2 = RSS / (NPLUS - DOF), NaN when NPLUS - DOF <= 0;  TSS = sum_i w_i (y_i - ybar_w)^2 from the
 *       corner of the Gram products;  R2 = 1 - RSS / TSS;  R2_LOO = 1 - PRESS / TSS;  STATIONARITY = ||Xo_A' W e - eta Q_A v_A||_inf /
 *       (||y||_W max_{m in A} sqrt(B_mm)) from the Gram products: whether the model IS the penalised least-squares solution on its
 *       support — the leave-one-out identity, sigma2 and the standard errors mean what they say only then.
 *   Cov = sigma2 S B S with S = H^-1 (sigma2 S at eta = 0);  se_w[m] = sqrt(Cov_mm) for m in A and 0 elsewhere (se_w[M]: the
 *       intercept's);  se_beta[k] = sqrt(p_k' Cov p_k) over A;  active[m] = 1 for m in A, else 0.
 * Everything is conditional on the model's sign pattern and support: nothing is adjusted for their selection.  The weights are
 * precision weights (w_i = 1 / variance_i up to a factor), not frequencies.
 *
 * Order of the sums.  A row's leverage is summed in an order that is a function of p alone — not of N, the launch or the row's
 * position.  DOF, RSS and PRESS follow the rule of partls_contributions' sums: consecutive blocks of 256 rows, each summed by a fixed
 * tree, the block sums added in ascending order from 0.0.  No floating-point atomics: two calls return the same bits.
 *
 * Outputs, each optional (NULL), at least one of them wanted.  Per row, N doubles each: leverage, loo, studentized, cooks, residual —
 * HOST arrays after a prepare from host pointers, DEVICE addresses after a prepare from device pointers.  Always host: se_w[M + 1],
 * se_beta[K], active[M + 1] (int32), summary[PARTLS_DIAG_NSUM].
 * The prepared problem is untouched: a sweep after the call returns what it returned before.  Storage: a double or a float X.
 * Errors, all found before anything is written: PARTLS_ERR_STATE without a prepared problem; PARTLS_ERR_UNSUPPORTED for a problem
 * prepared from CSR or a context of a partls_multi; PARTLS_ERR_BAD_ARG for a NULL alpha / beta, no output wanted, a NaN / Inf in alpha,
 * beta or t; PARTLS_ERR_ILL_CONDITIONED when the factorisation of H meets a pivot below the sweep's dependence threshold (1e-11 of
 * its diagonal entry: two active columns that are numerically dependent).
 */
#ifndef PARTLS_DIAG_H
#define PARTLS_DIAG_H
#ifndef PARTLS_H
#error "include partls.h, which includes this header"
#endif

#define PARTLS_DIAG_NPLUS 0
#define PARTLS_DIAG_P 1
#define PARTLS_DIAG_DOF 2
#define PARTLS_DIAG_RSS 3
#define PARTLS_DIAG_PRESS 4
#define PARTLS_DIAG_SIGMA2 5
#define PARTLS_DIAG_TSS 6
#define PARTLS_DIAG_R2 7
#define PARTLS_DIAG_R2_LOO 8
#define PARTLS_DIAG_STATIONARITY 9
#define PARTLS_DIAG_NSUM 10
partls_status partls_diagnostics(partls_ctx *ctx, const double *alpha, const double *beta, double t, double *leverage, double *loo,
                                 double *studentized, double *cooks, double *residual, double *se_w, double *se_beta, int32_t *active,
                                 double *summary);
/* where the last partls_diagnostics call on the context spent its time, in ms (tools/diagnostics_timing.py): the leverage kernel (device
 * events), the factorisation of H and T = L^-1 on the host, the whole call (host wall clock).  Zeros before the first call. */
partls_status partls_get_diagnostics_timing(const partls_ctx *ctx, double *kernel_ms, double *factor_ms, double *call_ms);

#endif
