/*
 * partls_robust.h — the two primitives of a robust (M-estimator) fit by iteratively reweighted least squares on a prepared problem:
 * the row weights of a Huber or bisquare loss at a model, formed on the device, and a re-prepare that swaps the sample weights of the
 * prepared problem without touching X.  Included by partls.h (include that, not this file): the types, conventions
 * and status codes are partls.h's, and these prototypes sit inside its extern "C" block.
 *
 * Why a header of its own: tests/test_abi.py reads partls.h as the list of the symbols of the main ctypes table (SYMBOLS, _lib.py).
 * That test stays as it is, so the entries below are declared here and bound in SYMBOLS_ROBUST; tests/test_robust_binding.py applies
 * the header / library / table checks to them.
 *
 * partls_robust_weights.  The problem is the one the context is prepared for (N rows; a double, float or CSR X); the model is
 * (alpha[M], beta[K], t), HOST arrays.  yhat_i is what partls_predict returns for the model on the problem's X, bit for bit;
 * a_i = |yhat_i - y_i|.  The eta rows and the problem's own sample weights take no part.
 *   scale:  scale_in > 0: s = scale_in.  scale_in <= 0 ("mad"): lo = (N - 1) / 2, hi = N / 2 (integer division), a_(k) the k-th
 *           smallest of a (0-based, an exact selection: ties, zeros, denormals and huge values are ordinary values),
 *           med = 0.5 a_(lo) + 0.5 a_(hi), s = med / 0.6745.  s == 0 (at least half of the rows are fitted exactly): the call returns
 *           PARTLS_OK with *scale = 0, zeros in the other scalar outputs, and writes no weights (the record of the previous weights stays).
 *   loss, with k = c s (c > 0; the usual 95 %-efficiency values are 1.345 and 4.685):
 *     PARTLS_ROBUST_HUBER:     w_i = a_i <= k ? 1 : k / a_i;           u = a_i / s;  rho_i = a_i <= k ? (0.5 u) u : c u - (0.5 c) c
 *     PARTLS_ROBUST_BISQUARE:  u = a_i / k;  v = 1 - u u;  w_i = u >= 1 ? 0 : v v;   rho_i = u >= 1 ? (c c) / 6 : ((c c) / 6) (1 - (v v) v)
 *   Every operation is one IEEE fp64 operation (no contraction, correctly rounded division): w is a bit-exact function of (a, c, s).
 *   outputs (each pointer optional): *scale = s;  *rho_sum = sum_i rho_i — consecutive blocks of 1024 rows, each summed by a fixed
 *   tree, the block sums added in ascending order from 0.0 on the host, no floating-point atomics: two calls return the same bits;
 *   *max_dw = max_i |w_i - wprev_i| (exact), wprev the weights of the previous call on this context since its last prepare (all ones
 *   when there was none; partls_opt_reweight keeps the record, every other prepare clears it);  *n_down = #{w_i < 1};
 *   *n_zero = #{w_i == 0};  w_out (optional): the N weights — a HOST array after a prepare from host pointers, a DEVICE address after
 *   a prepare from device pointers (the convention of partls_diagnostics).  The weights are also kept in a buffer of the context.
 *   The prepared problem is untouched: a sweep after the call returns what it returned before.
 *   Errors, all found before anything is written: PARTLS_ERR_BAD_ARG without a prepared problem, for a NULL alpha / beta, a NaN / Inf
 *   in alpha, beta or t, a c that is not finite or <= 0, an unknown loss, a NaN / Inf scale_in; PARTLS_ERR_UNSUPPORTED on a context of a
 *   partls_multi.
 *
 * partls_opt_reweight.  Replaces the sample weights of the prepared problem by w[N] (a host array, or a device address when
 * w_on_device; w == NULL: the weights of the last partls_robust_weights call on this context, PARTLS_ERR_STATE when there was none)
 * and rebuilds the Gram products and the tableau.  X, y, P, eta and the flags stay; nothing is uploaded except a host w, and
 * partls_get_upload reads 0 afterwards.  The context is then in the state partls_opt_prepare_weighted (or its _f32 / _csr form) would
 * leave it in with the same inputs and these weights — the same checks of w with the same statuses, the same Gram launch, the same
 * tableau: partls_get_gram, every sweep, every finish, Alt and BnB are bit-equal to that fresh prepare.  A device w must stay valid
 * while the context holds the problem.  A refused call names its reason in partls_last_error and leaves the context unprepared, as a
 * refused prepare does.  PARTLS_ERR_STATE without a prepared problem; PARTLS_ERR_UNSUPPORTED on a context of a partls_multi.
 */
#ifndef PARTLS_ROBUST_H
#define PARTLS_ROBUST_H
#ifndef PARTLS_H
#error "include partls.h, which includes this header"
#endif

#define PARTLS_ROBUST_HUBER 0
#define PARTLS_ROBUST_BISQUARE 1
partls_status partls_robust_weights(partls_ctx *ctx, const double *alpha, const double *beta, double t, int loss, double c,
                                    double scale_in, double *scale, double *rho_sum, double *max_dw, int64_t *n_down, int64_t *n_zero,
                                    double *w_out);
partls_status partls_opt_reweight(partls_ctx *ctx, const double *w, int w_on_device);
/* where the last partls_robust_weights call on the context spent its device time, in ms (tools/robust_timing.py): the residual pass,
 * the selection of the median (0 with a fixed scale), the weight kernel.  Zeros before the first call. */
partls_status partls_get_robust_timing(const partls_ctx *ctx, double *residual_ms, double *select_ms, double *weights_ms);

#endif
