/*
 * partls_contrib.h — group contributions: the N x K breakdown of the predictions of one or many models.  Included by
 * partls.h (include that, not this file): the types, conventions and status codes are partls.h's, and these prototypes sit inside its
 * extern "C" block.
 *
 * Why a header of its own: tests/test_abi.py reads partls.h as the list of the symbols of the main ctypes table (SYMBOLS, _lib.py), and
 * the float32 and CSR headers are pinned to their entry points by tests of their own.  Those tests stay as they are, so the two
 * entries below are declared here and bound in SYMBOLS_CONTRIB; tests/test_contributions_binding.py applies the header / library /
 * table / ccall checks to them.
 *
 * The contract.  For model b = (alpha[:, b], beta[:, b]) over the partition P (entries in {0,1}) and row i of X,
 *     w_mkb  = (double)P[m,k] * alpha[m,b] * beta[k,b]        evaluated as partls_predict evaluates the terms of its weights
 *     c_ikb  = the fma chain over the features m of group k (P[m,k] = 1) in ascending m, from 0.0:  c = fma((double)x_im, w_mkb, c)
 * one chain per (row, group, model).  The intercept belongs to no group: it is not an argument.  An empty group gives exactly +0.0, a
 * feature in no group contributes nowhere, a feature in two groups contributes to both.  For a partition sum_k c_ikb + t_b is the
 * prediction of partls_predict up to the order of summation: the weights are the same products.
 *
 * Models: alpha is M x B (leading dimension ld_alpha >= M), beta K x B (leading dimension ld_beta >= K) — the layouts
 * partls_opt_weightings writes — HOST arrays, as are P and ranks.
 * Outputs, each optional, at least one of them wanted:
 *   contrib (N x K x B column-major: element (i, k, b) at i + ldC (k + K b), ldC >= N; NULL: not wanted, ldC ignored): slab b is the
 *           result of a call with model b alone, bit for bit; rows N .. ldC of a column are not written;
 *   stats   (N x K x nr, leading dimension N: element (i, k, q) at i + N (k + K q); NULL if and only if nr == 0): the value at position
 *           ranks[q] (0-based, 0 <= ranks[q] < B) of the ascending sort of c[i, k, 0 .. B) — exact, ties included;
 *   mean    (N x K, leading dimension N; NULL: not wanted): (((c_ik0 + c_ik1) + c_ik2) + ...) / B, summed in index order;
 *   sums    (3 x K x B: element (s, k, b) at s + 3 (k + K b); ALWAYS host memory; NULL: not wanted): over the rows i, s = 0: sum of c,
 *           s = 1: sum of |c|, s = 2: sum of c^2.  The order of summation is a function of N alone: the rows are cut into consecutive
 *           blocks of 256, each block is summed by a fixed tree, and the block sums are added in ascending order from 0.0 — the same
 *           bits whatever the byte budget, the other outputs wanted, or where X lives.
 * x_on_device = 0: X is a host array, uploaded once and released afterwards, and contrib, stats and mean are host arrays.  When only
 * sums (or stats / mean) is wanted no N x K x B array exists on the host or crosses PCIe.  x_on_device = 1: X, contrib, stats and mean
 * are DEVICE addresses that stay owned by the caller.  Either way the rows are processed in chunks (multiples of 256 rows, at least
 * 256) whose rows x K x max(B, nr) intermediate in HBM stays within PARTLS_PREDICT_MANY_BYTES (PARTLS_CONTRIB_BYTES, read at
 * partls_create: another budget; tests); X is read once per PARTLS_CONTRIB_CHUNK models.
 * Errors, all found before any device work: PARTLS_ERR_BAD_ARG for B < 1, no output wanted, stats and nr that disagree, a rank outside
 * [0, B), ldC < N, ld_alpha < M, ld_beta < K, a NaN / Inf in alpha or beta; PARTLS_ERR_UNSUPPORTED for B or nr above
 * PARTLS_PREDICT_MANY_MAX_B; PARTLS_ERR_BAD_PARTITION for an entry of P outside {0,1}; otherwise those of partls_predict.  The
 * context's prepared problem, if any, is untouched, and a refused call leaves the context as it was.
 */
#ifndef PARTLS_CONTRIB_H
#define PARTLS_CONTRIB_H
#ifndef PARTLS_H
#error "include partls.h, which includes this header"
#endif

#define PARTLS_CONTRIB_CHUNK 16                      /* models per pass over X                          */
partls_status partls_contributions(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, int x_on_device,
                                   const int64_t *P, int64_t K, int64_t ldP, int64_t B, const double *alpha, int64_t ld_alpha,
                                   const double *beta, int64_t ld_beta, double *contrib, int64_t ldC, int64_t nr,
                                   const int64_t *ranks, double *stats, double *mean, double *sums);
/* the same for an X stored as float (N x M floats, ldX in elements): every output is double and equals partls_contributions on the
 * widened matrix bit for bit */
partls_status partls_contributions_f32(partls_ctx *ctx, const float *X, int64_t N, int64_t M, int64_t ldX, int x_on_device,
                                       const int64_t *P, int64_t K, int64_t ldP, int64_t B, const double *alpha, int64_t ld_alpha,
                                       const double *beta, int64_t ld_beta, double *contrib, int64_t ldC, int64_t nr,
                                       const int64_t *ranks, double *stats, double *mean, double *sums);

#endif
