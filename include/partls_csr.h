/*
 * partls_csr.h — the sparse (CSR) entry points of the C ABI of libpartls_hip.so.  Included by partls.h (include that, not this file):
 * the types, conventions and status codes are partls.h's, and these prototypes sit inside its extern "C" block.
 *
 * Why a header of its own: the ABI-consistency tests of the dense entry points parse partls.h with a type map without `int32_t *`
 * column indices.  They stay as they are, so these prototypes and their ctypes table (SYMBOLS_CSR in _lib.py) live beside partls.h, and
 * tests/test_csr_binding.py applies the same header / library / table / ccall checks to them (the rule of partls_f32.h).
 */
#ifndef PARTLS_CSR_H
#define PARTLS_CSR_H
#ifndef PARTLS_H
#error "include partls.h, which includes this header"
#endif

/* ---- sparse design matrices: the prepare of partls_opt_prepare_weighted for an X stored in CSR, never densified ------
 * Format: CSR, 0-based.  indptr[N + 1] (int64), indptr[0] = 0, indptr[N] = nnz; row i is indices / values over
 * [indptr[i], indptr[i + 1]); column indices (int32) strictly increase within a row (no duplicates) and lie in [0, M).  Stored zeros
 * count as zeros; empty rows and empty columns are allowed (a null column behaves as in the dense path).  M <= 1022 and N < 2^31;
 * every offset into indices / values is 64-bit.
 * x_on_device != 0: indptr, indices, values, y and w are DEVICE arrays that stay owned by the caller and must stay valid while the
 * context holds the problem (the rule of partls_opt_prepare_weighted).  x_on_device == 0: host arrays; the upload is
 * 8 (N + 1) + 12 nnz bytes plus y, and partls_get_upload reports the bytes of the matrix.
 * w: NULL (unweighted) or N sample weights under the rules and errors of partls_opt_prepare_weighted.
 * Validation runs on the device before anything of the problem is built; on failure the context is left unprepared:
 *   indptr[0] != 0, a decreasing indptr, an index outside [0, M), indices not strictly increasing in a row -> PARTLS_ERR_BAD_ARG (the
 *   message names the first offending row);  NaN / Inf in values -> PARTLS_ERR_NONFINITE;  a context of a partls_multi ->
 *   PARTLS_ERR_UNSUPPORTED.
 * The context then owns a column-ordered (CSC) image of the matrix (another 12 nnz + 8 (M + 1) bytes of HBM) and the augmented Gram
 * products of the dense prepare, built from the nonzeros alone (sum_i r_i^2 multiply-adds, r_i = nonzeros of row i) in an order fixed by
 * the data: bitwise reproducible, no floating-point atomics.
 * Every staged call on the prepared problem then works as after a dense prepare, weighted or not, on every sweep route:
 * partls_opt_sweep, _finish, _pattern, _candidates, _merge_candidates, _models, _top, _bit_order (PARTLS_OPT_RESCUE_CAPPED included),
 * partls_alt_prepared, partls_alt_multistart, partls_bnb_prepared, partls_bnb_bound(_snap), partls_bnb_leaf, partls_bnb_search,
 * partls_get_gram.  The next prepare of any kind decides the storage again.
 * Out of scope (dense only): partls_cv_opt*, partls_opt_weightings, partls_cv_alt, partls_predict_many, partls_fit_*_multi. */
partls_status partls_opt_prepare_csr(partls_ctx *ctx, const int64_t *indptr, const int32_t *indices, const double *values,
                                     int64_t N, int64_t M, const double *y, const double *w, int x_on_device, const int64_t *P,
                                     int64_t K, int64_t ldP, double eta, uint32_t flags);

/* partls_predict for a CSR X (format and x_on_device as above; yhat follows x_on_device): yhat_i = sum over the nonzeros of row i, in
 * ascending column order, of x_im w_m, plus t; an empty row gives exactly t.  The structure is validated as in the prepare (same
 * errors).  The context's prepared problem, if any, is untouched. */
partls_status partls_predict_csr(partls_ctx *ctx, const int64_t *indptr, const int32_t *indices, const double *values, int64_t N,
                                 int64_t M, int x_on_device, const int64_t *P, int64_t K, int64_t ldP, const double *alpha,
                                 const double *beta, double t, double *yhat);

#endif
