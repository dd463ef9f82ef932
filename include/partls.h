/*
 * partls.h — C ABI of the MI355X-native Partitioned-LS hot path (libpartls_hip.so, gfx950).
 *
 * The reference (/root/reference, pure Julia) has no FFI layer; its boundary is Julia multiple dispatch on
 *   fit(::Type{Opt}, X, y, P; η, nnlsalg, returnAllSolutions)        src/PartitionedLSOpt.jl:73-74
 *   fit(::Type{Alt}, X, y, P; η, ϵ, T, nnlsalg, rng)                 src/PartitionedLSAlt.jl:50-51
 *   fit(::Type{BnB}, X, y, P; η, nnlsalg)                            src/PartitionedLSBnB.jl:30
 *   predict(α, β, t, P, X) / predict(model, X)                       src/PartitionedLS.jl:132,152
 * A Julia shim keeps those signatures and `ccall`s the entry points below (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain C symbols, plain pointers and sizes; no C++ exception crosses this boundary;
 *   - matrices are COLUMN-MAJOR (Julia native) with an explicit leading dimension;
 *   - P is int64 (Julia Int on x64) with entries in {0,1}, M x K;
 *   - every output buffer is caller-allocated; the library never retains or frees caller memory;
 *   - every call returns a partls_status; partls_last_error() gives the thread-local message;
 *   - calls are synchronous (they return after the device work has completed);
 *   - a context is not thread-safe; distinct contexts may be used from distinct threads.
 *   - there is NO CPU fallback: without a HIP device every compute entry returns PARTLS_ERR_NO_DEVICE.
 */
#ifndef PARTLS_H
#define PARTLS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PARTLS_OK = 0,
    PARTLS_ERR_BAD_ARG = 1,        /* null pointer, negative size, ld < rows ...                         */
    PARTLS_ERR_BAD_PARTITION = 2,  /* P has an entry outside {0,1} (PartitionedLS.jl:292 validity clause) */
    PARTLS_ERR_NONFINITE = 3,      /* NaN/Inf in X or y, or a column whose sum of squares overflows fp64    */
    PARTLS_ERR_NO_DEVICE = 4,      /* no HIP device / device index out of range                           */
    PARTLS_ERR_HIP = 5,            /* a HIP runtime call failed (message has the hipError string)         */
    PARTLS_ERR_NOT_CONVERGED = 6,  /* an active-set solve hit its pivot cap (fit(Opt): and PARTLS_OPT_RESCUE_CAPPED was not set, or
                                      the rescue ran out of main passes too; partls_get_rescue_stats)   */
    PARTLS_ERR_UNSUPPORTED = 7,    /* shape outside what the kernels are built for: M > 1022 features, ldX >= 2^30, K > 61 groups,
                                      K > 39 for the 2^K enumeration of fit(Opt)                                              */
    PARTLS_ERR_STATE = 8,          /* staged calls issued out of order                                    */
    PARTLS_ERR_ILL_CONDITIONED = 9 /* the model's KKT conditions fail when checked against the DATA: X is too ill-conditioned for the
                                      fp64 Gram form (cond(X)^2 * eps >~ 1).  Outputs are filled with the best Gram-form model;
                                      a QR-based solver (the reference's, Opt.jl:89) is the right tool for this input          */
} partls_status;

/* flags for the Opt entry points */
#define PARTLS_OPT_FAITHFUL_INTERCEPT 1u /* enumerate all 2^(K+1) sign vectors incl. the intercept's, as Opt.jl:81,85 does.
                                            Without it the intercept is left free and 2^K subproblems are solved: the
                                            optimum (model and objective) is identical, min over the ± pair.             */
#define PARTLS_OPT_GENERIC_KERNEL     2u /* force the global-memory tableau kernel (testing / cross-check)               */
#define PARTLS_OPT_RESCUE_CAPPED      4u /* a pattern that hits the pivot cap of 20 (n + 1) exchange rounds (designs that are
                                            correlated throughout) is solved again on the device by
                                            Lawson-Hanson from the empty basis, at most 3 n main passes
                                            (PARTLS_RESCUE_MAX_PASSES, read at partls_create: another bound; tests), instead of
                                            being reported: partls_opt_sweep, partls_fit_opt, partls_opt_models, partls_opt_top,
                                            partls_opt_finish and partls_opt_pattern (see each).  A rescued pattern meets the
                                            sweeps' own KKT test under the context's tolerance; one that runs out of main
                                            passes stays NaN / PARTLS_ERR_NOT_CONVERGED.  A sweep or single solve without a
                                            capped pattern runs nothing extra (the export entries add two launches per piece
                                            that find an empty list), and without the flag nothing changes.  partls_cv_opt(_weighted),
                                            partls_opt_weightings and partls_fit_opt_multi answer the flag with
                                            PARTLS_ERR_UNSUPPORTED; the Alt and BnB calls on a context prepared with it
                                            ignore it (their solves are not rescued).                                      */

typedef struct partls_ctx partls_ctx;

int          partls_version(void);                 /* 10000*major + 100*minor + patch */
const char  *partls_last_error(void);              /* thread-local, never NULL        */
int          partls_device_count(void);            /* 0 when no HIP device is visible */

partls_status partls_create(int device, partls_ctx **out);
void          partls_destroy(partls_ctx *ctx);

/* ---- fit(Opt, X, y, P; η, returnAllSolutions)  — replaces Opt.jl:73-104 ----------------------------------------------
 * X: N x M (N <= ldX < 2^30), y: N, P: M x K (ldP >= M).  Outputs follow cleanupResult (Opt.jl:34-44):
 *   alpha[M] (sums to 1 per group), beta[K], *t, *opt = ||Xo w - yo||_2 of the winner (un-squared, incl. the η rows),
 *   *best_index = the reference's 0-based pattern index b (bit k = sign of group k+1, bit K = intercept sign; in
 *   free-intercept mode bit K is set from the sign of the fitted intercept).
 *   all_opt: optional (may be NULL); needs PARTLS_OPT_FAITHFUL_INTERCEPT; 2^(K+1) doubles, all_opt[b] = optval of pattern b
 *   (Opt.jl:90) computed from the Gram form.  Models of every pattern: partls_opt_models(); of one pattern, refined in data space:
 *   partls_opt_finish() / partls_opt_pattern(). */
partls_status partls_fit_opt(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                             const int64_t *P, int64_t K, int64_t ldP, double eta, uint32_t flags,
                             double *alpha, double *beta, double *t, double *opt, int64_t *best_index, double *all_opt);

/* ---- fit(Opt) on several GPUs of one node, inside the library  — the loop Opt.jl:85-94 has no loop-carried state ---------
 * One process, one host thread and one context per device.  Device r uploads rows [r N / R, (r+1) N / R) of X and y (1 / R of the PCIe
 * traffic each) and builds the Gram products of its block; their sum — ncclAllReduce(ncclSum) on (M+2)^2 doubles over xGMI — is the
 * problem every device then prepares.  Device r sweeps the Gray-index range [r * 2^K' / R, (r+1) * 2^K' / R) of the pattern space
 * and leaves its winner and near ties in host memory; the first device merges them into the global lexicographic minimum
 * (objective, reference pattern index) — argmin's first-index rule, Opt.jl:96 — and the near ties a single context would re-rank.
 * Ranks that disagree on the key of the visiting order fail with PARTLS_ERR_STATE instead of combining shards that do not partition
 * the pattern space.  The winner is re-solved on the first device; the passes over the data it needs (refinement, objective, KKT
 * check) run on every device's row block and are summed in rank order.
 *   devices[ndev]: HIP device indices (devices == NULL: devices 0 .. ndev-1; ndev == 0: every visible device).
 *   A list that names one device more than once (rehearsal of the R-rank control flow on a one-GPU box) cannot form an RCCL
 *   communicator: its Gram sum runs through the host instead; everything else is the same code.
 *   librccl.so.1 is loaded when the first communicator is needed (PARTLS_RCCL_LIB overrides the name), never for partls_fit_opt.
 * partls_fit_opt_multi: arguments and outputs exactly as partls_fit_opt (all_opt: the shards' entries merged, with
 * PARTLS_ERR_ILL_CONDITIONED too).
 * partls_multi_context: the context of rank r (rank 0 holds the winner's problem after a fit: partls_opt_finish /
 * partls_opt_pattern on it rebuild the models of returnAllSolutions, Opt.jl:99-101).  A partls_multi is not thread-safe. */
typedef struct partls_multi partls_multi;
partls_status partls_multi_create(const int *devices, int ndev, partls_multi **out);
void          partls_multi_destroy(partls_multi *mc);
int           partls_multi_size(const partls_multi *mc);                 /* number of ranks (0 for NULL)                  */
int           partls_multi_uses_rccl(const partls_multi *mc);            /* 1: Gram products of row-sharded fits summed over
                                                                            RCCL, 0: through the host (see above)          */
partls_ctx   *partls_multi_context(partls_multi *mc, int rank);          /* NULL when out of range                         */
partls_status partls_fit_opt_multi(partls_multi *mc, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                   const int64_t *P, int64_t K, int64_t ldP, double eta, uint32_t flags,
                                   double *alpha, double *beta, double *t, double *opt, int64_t *best_index, double *all_opt);
/* ---- fit(BnB) on several GPUs of one node, inside the library  — BnB.jl:94-132: subtrees are independent given the incumbent --------
 * Same handle, same row-sharded upload and Gram sum as partls_fit_opt_multi.  Every rank thread runs the same best-first frontier
 * (partls_frontier_*): per round the batch * R most promising nodes are dealt — a node goes to the rank that holds its parent's tableau
 * snapshot (warm start), the surplus and the cold nodes to the least loaded ranks —, every rank bounds its share on its own GPU, and ONE
 * exchange of (bound, branch, snapshot slot) per round through host memory carries the incumbent, so that all ranks prune, branch
 * and count snapshot references identically.  The incumbent's model is built on the first device (partls_bnb_leaf, data passes over
 * every rank's row block).  Outputs as partls_fit_bnb; *nopen = nodes bounded by
 * all ranks (not a parity quantity: the search order differs from the reference's depth-first recursion). */
partls_status partls_fit_bnb_multi(partls_multi *mc, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                   const int64_t *P, int64_t K, int64_t ldP, double eta,
                                   double *alpha, double *beta, double *t, double *opt, int64_t *nopen);
/* Robustness of the rank threads (both fits): every phase ends in a rendezvous at which the ranks agree to go on or to leave together; a
 * rank that cannot keep the protocol, or does not reach a rendezvous within PARTLS_MULTI_TIMEOUT_S seconds (default 3600), fails the
 * fit with PARTLS_ERR_STATE instead of hanging it; a failed enqueue of the Gram sum aborts the communicators (ncclCommAbort) and the
 * handle sums through host memory from then on (partls_multi_uses_rccl turns 0). */
/* per-rank HIP-event time (ms) of stage `which` in the last partls_fit_opt_multi */
partls_status partls_multi_get_timing(const partls_multi *mc, int rank, int which, double *ms);

/* ---- staged form of the same path (multi-GPU sharding, device-resident inputs, benchmarking) ------------------------
 * prepare:  builds G = Xo'Xo, c = Xo'y, yy (fp64 MFMA), applies η, scales, lays the tableau out for the sweep.
 *           x_on_device != 0: X and y are DEVICE pointers (hipMalloc / torch) and stay owned by the caller.
 * sweep:    enumerates Gray indices [g_begin, g_end) of the 2^K' pattern space (K' = K+1 faithful, K free intercept);
 *           g_end = -1 means "to the end".  Returns the shard's lexicographic minimum (objective, pattern index) —
 *           the pair a rank feeds into the all-reduce(min).  all_opt as above (indexed by pattern, not by Gray index;
 *           entries of patterns outside [g_begin, g_end) are set to NaN).
 *           Gray indices are positions in the context's own visiting order: which group sits on which Gray bit is chosen
 *           per prepared problem (partls_opt_bit_order; measured on the first sweep of long enumerations, deterministic in
 *           the data, so ranks that prepared the same problem agree).  Any disjoint ranges covering [0, 2^K') visit every
 *           pattern exactly once; every pattern index that crosses this boundary is the reference's (group k = bit k).
 * finish:   solves the given pattern once more on its own, computes opt from the data, normalises (cleanupResult).
 * With PARTLS_OPT_RESCUE_CAPPED: a sweep that reports capped patterns walks its range a second time through the export pieces of
 * partls_opt_models, whose capped rows the rescue kernel solves; that pass is authoritative: winner, near ties and candidates
 * (partls_opt_candidates), all_opt and *n_unconverged (what the rescue could not solve) are its results.  finish (and
 * partls_opt_pattern): a single solve that hits the cap is solved by the rescue kernel instead of failing.
 * A refused prepare (this one, _weighted, _f32, _csr).  The argument checks come first and leave the context as it was, so a problem
 * prepared before still sweeps and finishes to the same bits: a NULL X, y or P, N, M or K < 1, ldX < N, ldP < M, a size beyond the
 * build's limits, eta < 0 or NaN.  Every failure found later leaves the context unprepared (the next staged call returns
 * PARTLS_ERR_STATE until a prepare succeeds): the weights, the structure or values of a CSR matrix, an entry of P outside {0,1},
 * NaN / Inf in X or y (found in the Gram products), a HIP error.  tests/test_gpu_context_reuse.py holds both to it. */
partls_status partls_opt_prepare(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                 int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta, uint32_t flags);
/* ---- sample weights: the same prepare for the weighted problem (MLJ's supports_weights, scikit-learn's sample_weight) ---------------
 *   minimise  sum_i w_i (x_i' (P .* α) β + t - y_i)^2  +  the η rows of regularizeProblem (PartitionedLS.jl:108-123, NOT weighted)
 * over the same feasible set and sign patterns.  w[N]: every w_i finite and >= 0, sum w_i > 0; a row with w_i = 0 acts as an absent row
 * (its X and y must still be finite).  w follows x_on_device: a host array, or a DEVICE array that stays owned by the caller and must
 * stay valid while the context holds this problem.  w == NULL is exactly partls_opt_prepare.
 * Errors (found before anything else is written; the context is left unprepared): NaN / Inf in w -> PARTLS_ERR_NONFINITE; a negative
 * weight or sum w_i = 0 -> PARTLS_ERR_BAD_ARG; a context of a partls_multi -> PARTLS_ERR_UNSUPPORTED (multi-GPU fits are unweighted).
 * Every staged call on the problem is then weighted — partls_opt_sweep, _finish, _pattern, _candidates, _merge_candidates, _models,
 * _bit_order, partls_alt_prepared, partls_bnb_prepared, partls_bnb_bound(_snap), partls_bnb_leaf, partls_bnb_search — with "sum over
 * rows" read as "weighted sum over rows" in every output: opt, all_opt, best_index, the near-tie window (1e-13 of y'Wy on obj^2),
 * the data-space KKT check and PARTLS_ERR_ILL_CONDITIONED.  partls_predict is unchanged (weights do not enter a prediction).
 * A weighted fit(Opt) is this + partls_opt_sweep + partls_opt_finish; a weighted fit(Alt) is
 * partls_opt_prepare_weighted(..., PARTLS_OPT_FAITHFUL_INTERCEPT) + partls_alt_prepared, a weighted fit(BnB) the same prepare +
 * partls_bnb_prepared.  The next plain prepare (or fit) on the context is unweighted again.  DESIGN.md §4.7. */
partls_status partls_opt_prepare_weighted(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                          const double *w, int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta,
                                          uint32_t flags);
/* float32 design matrices: partls_opt_prepare_f32 is this prepare for an X stored as float, with or without weights (partls_f32.h,
 * included at the end of this header). */
partls_status partls_opt_sweep(partls_ctx *ctx, int64_t g_begin, int64_t g_end,
                               double *best_obj, int64_t *best_pattern, double *all_opt, int64_t *n_unconverged);
partls_status partls_opt_finish(partls_ctx *ctx, int64_t pattern,
                                double *alpha, double *beta, double *t, double *opt, int64_t *best_index);
/* Near ties across shards.  The sweep ranks patterns on the Gram-form objective, whose absolute error in obj^2 is a few u * y'y (u = 2^-53;
 * measured on real-valued data against a QR reference: <= 3.3 u y'y uncentred, <= 248 u y'y on centred data with 8192-pattern chains,
 * growing about as the square root of the chain length).  partls_opt_finish re-ranks the winner and the (at most 3) patterns
 * within 1e-13 y'y (= 901 u y'y) of it on obj^2 by the objective computed from the DATA, first reference index on exact
 * ties (Opt.jl:90,96).  A host that shards the enumeration (one context per GPU) must give every rank the candidate set a single
 * context would have had:
 *   candidates: the shard's winner and its near ties with their tracked objectives, best first (count <= 4 <= capacity);
 *   merge:      the concatenation of ALL ranks' candidate lists (any order; the same list on every rank) -> the global lexicographic
 *               minimum (objective, reference index) in *win_obj / *win_pattern, installed together with its near ties for the next
 *               partls_opt_finish(ctx, *win_pattern, ...) on this context.  Every rank then returns the same model.
 * partls_fit_opt_multi does this between its rank threads; partitionedls.jl_amd/dist.py with one all-gather of 64 bytes per rank. */
partls_status partls_opt_candidates(const partls_ctx *ctx, int64_t capacity, double *obj, int64_t *pattern, int64_t *count);
partls_status partls_opt_merge_candidates(partls_ctx *ctx, int64_t count, const double *obj, const int64_t *pattern,
                                          double *win_obj, int64_t *win_pattern);
/* raw NNLS solution of one pattern b (reference indexing, K+1 bits): raw_alpha[M+1] >= 0 as nonneg_lsq returns it at
 * Opt.jl:89, and its optval (Opt.jl:90).  Needs a prepared context.  Every pattern at once: partls_opt_models. */
partls_status partls_opt_pattern(partls_ctx *ctx, int64_t pattern, double *raw_alpha, double *optval);
/* Models of a Gray-index range straight from the sweep (Opt.jl:87-101 without one solve per pattern).
 * The range [g_begin, g_end) is the one partls_opt_sweep takes: the context's own visiting order, g_end = -1 = to the end.
 * Row i (0 <= i < g_end - g_begin) describes Gray index g_begin + i; every array is column-major with one pattern per column
 * (leading dimensions >= M+1, M, K: Julia passes an M x B matrix as it is):
 *   pattern[i]                          reference index b of that pattern (required)
 *   optval[i]                           Opt.jl:90 in the Gram form, = all_opt[b] of a plain sweep (optional)
 *   raw_alpha[i * ld_raw + m], m <= M   nonneg_lsq's alpha (Opt.jl:89), as partls_opt_pattern returns it (optional)
 *   alpha[i * ld_alpha + m], beta[i * ld_beta + k], t[i]
 *                                       cleanupResult(Opt, ...) (Opt.jl:34-44), as partls_opt_finish returns it (optional; all three or none)
 *   *n_unconverged, *n_vetoes           patterns of the range that hit the pivot cap / entering pivots refused by the
 *                                       leave-one-out rule (optional)
 * Accuracy: these are the Gram-form solutions that rank all_opt, not refined in data space as partls_opt_finish's are ("Every pattern's model").
 * With *n_vetoes > 0 the data has (nearly) dependent columns and the Gram form carries no guarantee: use partls_opt_finish per pattern.
 * A pattern that hit the pivot cap gets NaN in its optval and model rows. The caller re-solves it with partls_opt_finish.
 * With PARTLS_OPT_RESCUE_CAPPED the capped rows of every piece are solved on the device by the rescue kernel before the cleanup: they
 * are ordinary rows then, *n_unconverged counts only what the rescue could not solve (those rows stay NaN) and *n_vetoes includes the
 * rescue's refusals.
 * The range is processed in pieces whose device buffers stay below PARTLS_OPT_MODELS_PIECE_BYTES; a range whose buffers fit is one piece
 * on the chain plan of partls_opt_sweep for the same range.  To spread one export over several devices, give each device's context a
 * disjoint Gray range of the same prepared problem (equal visiting order: compare partls_opt_bit_order).
 * Needs a context prepared with PARTLS_OPT_FAITHFUL_INTERCEPT (else PARTLS_ERR_STATE). Leaves the state of the last
 * partls_opt_sweep untouched: winner, near ties, exported winner row, candidates, pivot and veto counters. */
#define PARTLS_OPT_MODELS_PIECE_BYTES (1ULL << 30)   /* 1 GiB */
partls_status partls_opt_models(partls_ctx *ctx, int64_t g_begin, int64_t g_end, int64_t *pattern, double *optval,
                                double *raw_alpha, int64_t ld_raw, double *alpha, int64_t ld_alpha,
                                double *beta, int64_t ld_beta, double *t, int64_t *n_unconverged, int64_t *n_vetoes);
/* The k best patterns of a Gray-index range and their models, selected on the device: what partls_opt_models
 * returns for the range, reduced to its k best rows before anything is copied back.  Preconditions, range rules and error statuses
 * are those of partls_opt_models; additionally 1 <= k <= PARTLS_OPT_TOP_MAX_K (else PARTLS_ERR_BAD_ARG).
 * Row i of every output (laid out as partls_opt_models' outputs; pattern and optval required, raw_alpha optional, alpha / beta / t all
 * three or none) is the i-th best pattern of [g_begin, g_end) in the total order
 *     a before b  iff  optval_a < optval_b, or optval_a == optval_b as doubles (-0.0 equals +0.0; +inf is an ordinary value) and
 *                      pattern_a < pattern_b   (pattern: the reference index b).
 * A pattern that hit the pivot cap (NaN objective) is never selected, only counted in *n_unconverged.  With PARTLS_OPT_RESCUE_CAPPED
 * the capped patterns of a piece are rescued before the selection (see partls_opt_models), so they are selectable.
 * *count = min(k, converged patterns of the range); rows at and beyond *count are not written.  Two calls with the same arguments
 * return the same bits.  The models are the Gram-form models of partls_opt_models, bit for bit the rows it returns for the same
 * patterns when both run the same piece; accuracy and the meaning of *n_vetoes are partls_opt_models'.
 * The range is cut into equal pieces, ceil(total / npieces), whose scaled rows and objectives ((n + 1) doubles per pattern, n = M + 1)
 * stay below PARTLS_OPT_MODELS_PIECE_BYTES (PARTLS_TOP_PIECE, a test knob read at partls_create: patterns per piece instead, here, in
 * partls_opt_models and in the second pass of a rescuing sweep); each piece is one
 * export sweep on the chain plan of partls_opt_sweep for its length, a selection, sort and gather of its k best rows on the device, the
 * cleanup of those rows and one copy back; the host merges the pieces' lists by the same order.
 * Leaves the state of the last partls_opt_sweep untouched, as partls_opt_models does. */
#define PARTLS_OPT_TOP_MAX_K 4096
partls_status partls_opt_top(partls_ctx *ctx, int64_t g_begin, int64_t g_end, int64_t k, int64_t *pattern, double *optval,
                             double *raw_alpha, int64_t ld_raw, double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta,
                             double *t, int64_t *count, int64_t *n_unconverged, int64_t *n_vetoes);
/* The selection stage of partls_opt_top alone (tests, diagnosis): obj is a HOST array of cnt objectives of Gray indices
 * g0 .. g0 + cnt - 1 of the prepared problem (g0 + cnt <= number of patterns, cnt < 2^31); it is uploaded and goes through the kernels
 * partls_opt_top runs per piece, without a sweep.  index[i] (position in obj), pattern[i] (reference index) and optval[i] describe the
 * i-th best entry in the order above; *count = min(k, non-NaN entries).  Needs a prepared context (any intercept mode). */
partls_status partls_opt_top_select(partls_ctx *ctx, const double *obj, int64_t cnt, int64_t g0, int64_t k, int64_t *index,
                                    int64_t *pattern, double *optval, int64_t *count);
/* visiting order of the sweep: gbit[k] = Gray-index bit that carries group k (K' entries; identity unless calibrated);
 * flip_cost (optional, K' doubles): measured cost of a flip of group k in pivot equivalents (pivots + weighted block pivots and
 * extra KKT scans; exact counts, no timing), -1 when the calibration did not run (sweeps too short
 * to repay it, PARTLS_BIT_ORDER=identity); gbit stays the identity when the measured costs promise less than 2 % fewer pivots.  Runs the calibration if no sweep has done so yet.  Ranks of a sharded
 * sweep must hold the same gbit (partitionedls.jl_amd/dist.py checks it inside its first all-reduce). */
partls_status partls_opt_bit_order(partls_ctx *ctx, int64_t *gbit, double *flip_cost);
/* number of subproblems one full sweep solves (2^K or 2^(K+1)) for the prepared problem */
int64_t       partls_opt_num_patterns(const partls_ctx *ctx);

/* ---- cross-validation of fit(Opt) over folds x an η grid, and the full-data regularisation path, in one call ------------------------
 * The reference's MLJ model PartLS exposes η (PartitionedLS.jl:290-297); it can only be chosen on held-out rows.  Inputs as
 * partls_opt_prepare (x_on_device: X, y are DEVICE pointers), plus
 *   fold_ptr[F+1]: fold boundaries, 0 = fold_ptr[0] < ... < fold_ptr[F] = N; fold f = rows [fold_ptr[f], fold_ptr[f+1]).  F = 0
 *                  (fold_ptr may be NULL): no CV, the path only.  F = 1 is an error.
 *   eta[E]:        E >= 1 values, each finite and >= 0;   flags: those of partls_fit_opt (no all_opt).
 * Problems: B = (F+1) E, indexed q = f E + e.  Problem (f < F, e) is fit(Opt, X[train_f], y[train_f], P; η = eta[e]) with train_f = every
 * row outside fold f in its original order (the η rows are not rescaled by the training size: regularizeProblem, PartitionedLS.jl:108-123).
 * Problem (F, e) is the fit on all rows (the regularisation path).  Outputs, column q of each (caller-allocated, column-major):
 *   alpha[q * ld_alpha + m] (ld_alpha >= M), beta[q * ld_beta + k] (ld_beta >= K), t[q], opt[q], best_index[q]: as partls_fit_opt;
 *   heldout_sse[q]: sum over the rows i of fold f of (predict(model, x_i) - y_i)^2 (PartitionedLS.jl:132), from the data; NaN for f = F;
 *   status[q]: 0, PARTLS_ERR_ILL_CONDITIONED (the model as fit() returns it, see there) or PARTLS_ERR_NOT_CONVERGED (NaN outputs,
 *              best_index -1).
 * Any other failure (bad arguments, NaN/Inf data, HIP errors) fails the whole call and writes no output.
 * Accuracy: every problem's model is the refined, KKT-checked model partls_opt_finish returns for a single fit; the Gram products of a
 * training set are the sum of its folds' (fixed order), so an objective can differ from a single fit's by the Gram form's own rounding
 * and a winner within the near-tie window (1e-13 y'y on obj^2) may be the other pattern of the tie.  Bitwise reproducible.
 * The visiting order of the sweep is calibrated once, on the full-data problem at eta[0], and shared by every problem.  Register-kernel
 * problems (n <= 288) are swept together in launches of up to 65535 problems; larger ones, PARTLS_OPT_GENERIC_KERNEL and the
 * PARTLS_CV_SERIAL=1 knob (read at partls_create) sweep one problem after another.
 * Context state afterwards: it keeps the upload of X (host inputs) but holds no prepared problem (a staged call must prepare again);
 * partls_get_timing gives the phases of the whole call (GRAM: fold Grams + combine, PREP, SWEEP: sums over the batch, FINISH: host wall time of
 * the per-problem finishes, held-out passes included). */
partls_status partls_cv_opt(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device,
                            const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F,
                            const double *eta, int64_t E, uint32_t flags,
                            double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt,
                            int64_t *best_index, double *heldout_sse, int32_t *status);
/* The same with sample weights w[N] (rules and errors of partls_opt_prepare_weighted; w follows x_on_device; w == NULL is exactly
 * partls_cv_opt): problem (f, e) is the weighted fit on the training rows of fold f with their weights, and
 * heldout_sse[q] = sum over the rows i of fold f of w_i (predict(model, x_i) - y_i)^2.  A fold whose training rows weigh 0 in total
 * fails the call with PARTLS_ERR_BAD_ARG. */
partls_status partls_cv_opt_weighted(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                     const double *w, int x_on_device, const int64_t *P, int64_t K, int64_t ldP,
                                     const int64_t *fold_ptr, int64_t F, const double *eta, int64_t E, uint32_t flags,
                                     double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt,
                                     int64_t *best_index, double *heldout_sse, int32_t *status);

/* ---- fit(Opt) under B row weightings of one (X, y, P) in one call: bootstrap replicates (integer counts), jackknife and repeated
 * train / validation splits (0/1 weights), any other reweighting --------------------------------------------------------------------
 * Inputs as partls_opt_prepare (x_on_device: X, y AND W are device pointers), plus
 *   W: N x B doubles, column-major, leading dimension ldW >= N; column b is weighting b (rules of partls_opt_prepare_weighted: finite,
 *      >= 0, sum > 0; a row of weight 0 acts as an absent row of problem b);   eta: finite, >= 0;   flags: those of partls_fit_opt.
 * Problem b is exactly partls_opt_prepare_weighted(w = W[:, b], eta, flags), partls_opt_sweep(0, -1), partls_opt_finish(winner): the
 * meanings, the near-tie window and the data-space KKT check are a single weighted fit's.  Outputs, column b of each (caller-allocated):
 *   alpha[b * ld_alpha + m], beta[b * ld_beta + k], t[b], opt[b], best_index[b], status[b]: as partls_cv_opt (status 0 / 9 / 6; NaN
 *              outputs and best_index -1 on 6);
 *   oob_rows[b] (optional, NULL to skip): the number of rows with W[i, b] == 0 — the out-of-bag rows of a bootstrap replicate;
 *   oob_sse[b]  (optional, NULL to skip): sum over those rows of (predict(model_b, x_i) - y_i)^2, unweighted, from the data; NaN when
 *              oob_rows[b] is 0 or the problem failed (status 6).
 * Every column of W is checked before any output is written: NaN / Inf anywhere -> PARTLS_ERR_NONFINITE; a negative entry, a column of
 * sum 0, B < 1, ldW < N or a NULL W / required output -> PARTLS_ERR_BAD_ARG; a context of a partls_multi -> PARTLS_ERR_UNSUPPORTED;
 * other argument errors as partls_cv_opt.  Any failure of the whole call writes no output.
 * One upload of X, y, W; one weighted Gram per column (the single fit's kernel and summation order: an all-ones column gives the
 * unweighted fit bit for bit); prepare, layout and sweep batched as in partls_cv_opt (register kernels, n <= 288, chunks of up to 65535
 * problems) or one problem after another (larger n, PARTLS_OPT_GENERIC_KERNEL, PARTLS_RESAMPLE_SERIAL=1 read at partls_create); the
 * visiting order is calibrated once on weighting 0; each problem is finished like a single fit with its column's weights.  The same call
 * twice is bitwise equal.  The chain plan of a sweep goes by the size of the batch, so a problem swept in another batch (or alone) may
 * start its finish from another chain's solution of the same winner: equal within a single fit's tolerances, not always bit for bit.
 * oob_sse is a function of the model and the column alone (fixed blocks, fixed order, no atomics).  The device holds W, sqrt(W) (16 N B bytes) and one Gram per column for the call.
 * Context state afterwards as after partls_cv_opt: no prepared problem; partls_get_sweep_route reports this call's route;
 * partls_get_timing its phases (GRAM: the B Gram builds, PREP, SWEEP, FINISH: host wall time of the per-problem finishes, OOB: the
 * out-of-bag pass). */
partls_status partls_opt_weightings(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                    int x_on_device, const int64_t *P, int64_t K, int64_t ldP,
                                    const double *W, int64_t ldW, int64_t B, double eta, uint32_t flags,
                                    double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt,
                                    int64_t *best_index, double *oob_sse, int64_t *oob_rows, int32_t *status);

/* ---- fit(Alt, X, y, P; η, ϵ, T)  — replaces Alt.jl:50-124 ------------------------------------------------------------
 * alpha0[M+1], beta0[K+1]: the random initial point the Julia shim draws exactly as Alt.jl:58-66 does.
 * Outputs as Alt.jl:119: alpha[M], beta[K], *t = β[end]*α[end], *opt, *iters = completed iterations. */
partls_status partls_fit_alt(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                             const int64_t *P, int64_t K, int64_t ldP, double eta, double eps, int64_t T,
                             const double *alpha0, const double *beta0,
                             double *alpha, double *beta, double *t, double *opt, int64_t *iters);

/* The same on a context already prepared with partls_opt_prepare(..., flags | PARTLS_OPT_FAITHFUL_INTERCEPT) — e.g. with
 * device-resident inputs; partls_fit_alt / partls_fit_bnb are "prepare from host pointers" + these. */
partls_status partls_alt_prepared(partls_ctx *ctx, double eps, int64_t T, const double *alpha0, const double *beta0,
                                  double *alpha, double *beta, double *t, double *opt, int64_t *iters);
partls_status partls_bnb_prepared(partls_ctx *ctx, double *alpha, double *beta, double *t, double *opt, int64_t *nopen);

/* ---- fit(Alt) from R starting points in one batched call ----------------------------------------------
 * On a context prepared like partls_alt_prepared's (any prepare: plain, weighted, float32, device-resident; else PARTLS_ERR_STATE).
 * alpha0: (M+1) x R, column r = start r (leading dimension ld_alpha0 >= M+1); beta0: (K+1) x R (ld_beta0 >= K+1).  Start r runs
 * exactly the iteration of partls_alt_prepared(ctx, eps, T, alpha0[:, r], beta0[:, r]) — up to the rounding of the alpha-step solver,
 * which solves every alpha-step from the fresh tableau here — and stops on its own; all active starts advance together on the
 * device.  A start's result does not depend on R, on its position or on the chunking (PARTLS_ALT_MS_CHUNK), bit for bit.
 * Per start (each array optional, NULL to skip): alpha_all (M x R, ld_alpha_all >= M), beta_all (K x R, ld_beta_all >= K), t_all[R]
 * (Alt.jl:119), opt_all[R] = the Gram-form loss of its last iteration, iters_all[R] = completed iterations, status_all[R]:
 *   PARTLS_OK;  PARTLS_ERR_NONFINITE: NaN / Inf in its alpha0 / beta0 (checked on the host; the start takes no part);
 *   PARTLS_ERR_NOT_CONVERGED: an alpha-step hit the pivot cap or its beta-step system is singular.  Rows of a failed start are NaN.
 * The winner — the PARTLS_OK start with the smallest final loss, lowest index on an exact tie, *best_start — goes through the ending
 * of partls_alt_prepared: alpha[M], beta[K], *t, *opt (from the data where that function takes it from the data), *iters, the
 * data-space KKT check (partls_get_kkt_violation) and PARTLS_ERR_ILL_CONDITIONED with the outputs filled.  Without a PARTLS_OK start:
 * PARTLS_ERR_NOT_CONVERGED, the per-start arrays filled, the winner's outputs NaN and *best_start = -1.
 * PARTLS_ERR_BAD_ARG: eps <= 0, T < 1, R < 1, a NULL start or winner output, a leading dimension below its row count. */
partls_status partls_alt_multistart(partls_ctx *ctx, double eps, int64_t T, int64_t R,
                                    const double *alpha0, int64_t ld_alpha0, const double *beta0, int64_t ld_beta0,
                                    double *alpha, double *beta, double *t, double *opt, int64_t *iters, int64_t *best_start,
                                    double *alpha_all, int64_t ld_alpha_all, double *beta_all, int64_t ld_beta_all,
                                    double *t_all, double *opt_all, int64_t *iters_all, int32_t *status_all);

/* ---- cross-validation of the multistart fit(Alt) over folds x an η grid, and the full-data path, in one call -------
 * Beyond K = 39 groups fit(Opt) cannot enumerate and fit(Alt) from many starts is the tool; this entry chooses its η.  Data arguments,
 * folds, grid and problem indexing (B = (F+1) E, q = f E + e, f = F: all rows) are partls_cv_opt_weighted's (w may be NULL); every
 * problem is prepared with PARTLS_OPT_FAITHFUL_INTERCEPT whatever flags says (PARTLS_OPT_GENERIC_KERNEL is honoured).  eps, T, R,
 * alpha0 ((M+1) x R, ld_alpha0 >= M+1), beta0 ((K+1) x R, ld_beta0 >= K+1) are partls_alt_multistart's; the SAME R starts are used for
 * every problem.  Outputs, column q of each (caller-allocated, column-major):
 *   alpha (ld_alpha >= M), beta (ld_beta >= K), t[q], opt[q], iters[q], best_start[q]: the problem's winner — its smallest final
 *              Gram-form loss among the PARTLS_OK starts, lowest index on an exact tie — after the ending of partls_alt_prepared on
 *              exactly the problem's training rows;
 *   heldout_sse[q]: as partls_cv_opt_weighted (NaN for f = F);
 *   status[q]: 0, PARTLS_ERR_ILL_CONDITIONED (outputs filled) or PARTLS_ERR_NOT_CONVERGED when no start of the problem finished
 *              (NaN outputs, iters 0, best_start -1);
 *   opt_all, iters_all, status_all (each optional, NULL to skip): R x B per-trajectory tables, entry q R + r = start r of problem q, with
 *              the meanings of partls_alt_multistart (NaN / 0 rows for a failed start).
 * Any other failure fails the whole call and writes no output; bad arguments (also eps <= 0, T < 1, R < 1, short leading dimensions)
 * write nothing.  A trajectory's result does not depend on R, on the other η values, on its position in the batch or on the chunking
 * (PARTLS_ALT_MS_CHUNK), bit for bit.  Register-kernel problems (n <= 288) advance all B R trajectories together; larger ones,
 * PARTLS_OPT_GENERIC_KERNEL and PARTLS_CV_SERIAL=1 take one problem after another — the same per-trajectory results and the same
 * winners' models, bit for bit.  Context state afterwards as after partls_cv_opt; partls_get_timing: GRAM, then host wall times of
 * PREP, SWEEP (the iterations) and FINISH. */
partls_status partls_cv_alt(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w,
                            int x_on_device, const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F,
                            const double *eta, int64_t E, uint32_t flags, double eps, int64_t T, int64_t R,
                            const double *alpha0, int64_t ld_alpha0, const double *beta0, int64_t ld_beta0,
                            double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, double *opt, int64_t *iters,
                            int64_t *best_start, double *heldout_sse, int32_t *status,
                            double *opt_all, int64_t *iters_all, int32_t *status_all);

/* ---- fit(BnB, X, y, P; η)  — replaces BnB.jl:30-132 -------------------------------------------------------------------
 * Outputs as BnB.jl:36-40; *nopen = nodes bounded (search order differs from the reference's DFS, so it is not a
 * parity quantity). */
partls_status partls_fit_bnb(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                             const int64_t *P, int64_t K, int64_t ldP, double eta,
                             double *alpha, double *beta, double *t, double *opt, int64_t *nopen);

/* The two primitives of the BnB search on a prepared (PARTLS_OPT_FAITHFUL_INTERCEPT) context — what a host that shards the
 * frontier across GPUs calls (partitionedls.jl_amd/dist.py: one process per GPU, batches dealt round-robin, one all-gather of
 * (bound, branch) per batch carries the incumbent).  A node is (pat, free): group k < K+1 is branched iff bit k of free is
 * clear, then α_pk >= 0 if bit k of pat is set, <= 0 otherwise (BnB.jl:120-121; group K is the intercept's).
 *   bound: lb[i] = lower bound of node i (BnB.jl:69-92); branch[i] = argmax_k ν_k (BnB.jl:107,117) or -1 when the relaxed
 *          solution is already feasible (BnB.jl:109-115: lb[i] is then an upper bound too).
 *   leaf:  model of one feasible node, normalised as BnB.jl:36-39, *opt from the data. */
partls_status partls_bnb_bound(partls_ctx *ctx, int64_t count, const uint64_t *pat, const uint64_t *free_groups,
                               double *lb, int32_t *branch);
partls_status partls_bnb_leaf(partls_ctx *ctx, uint64_t pat, uint64_t free_groups,
                              double *alpha, double *beta, double *t, double *opt);
/* Node bounds with tableau SNAPSHOTS, for a host that runs the search itself and shards it over GPUs (dist.py deals every node to the
 * rank that holds its parent's snapshot): node i starts from the final tableau stored in src_slot[i] (-1: the fresh tableau) and leaves
 * its own in dst_slot[i] (out; -1: pool full, no free group left, or the PARTLS_EAGER_GENERIC test kernel; both production kernels take
 * snapshots, at any n <= 1023).  The host keeps the reference counts and returns slots
 * with partls_bnb_snap_release; partls_bnb_snap_begin (after every prepare, before the first bound) empties the pool. */
partls_status partls_bnb_snap_begin(partls_ctx *ctx);
partls_status partls_bnb_bound_snap(partls_ctx *ctx, int64_t count, const uint64_t *pat, const uint64_t *free_groups,
                                    const int32_t *src_slot, int32_t *dst_slot, double *lb, int32_t *branch);
partls_status partls_bnb_snap_release(partls_ctx *ctx, int64_t count, const int32_t *slots);
/* The FRONTIER of the search as an object, for a host that shards the search over processes (one per GPU): every rank creates one with
 * its (rank, world) and drives rounds —
 *   next:    pops the batch * world most promising nodes (pruned against the incumbent, BnB.jl:102) and deals them: a node goes to the
 *            rank that holds its parent's snapshot, up to that rank's quota; the rest, cold, to the least loaded ranks.  *total = nodes
 *            of the round (0: the search is over), per_rank[world] = every rank's share, this rank's share in pat / free_groups /
 *            src_slot (capacity >= batch) ready for partls_bnb_bound_snap;
 *   (the ranks exchange lb / branch / dst_slot of their shares: one all-gather)
 *   ingest:  the results of ALL ranks in rank-major order (rank 0's nodes in the order `next` gave them, then rank 1's, ...): prunes,
 *            records feasible nodes, branches (BnB.jl:107-124), counts snapshot references; `dead` receives this rank's slots that lost
 *            their last reference (at most dead_capacity per call; call again with an empty round for the rest) for
 *            partls_bnb_snap_release.
 * All ranks make identical decisions (the frontier depends on shared data only).  partls_bnb_search is this loop with world = 1. */
typedef struct partls_frontier partls_frontier;
partls_status partls_frontier_create(int n_groups, int rank, int world, int64_t batch, partls_frontier **out);
void          partls_frontier_destroy(partls_frontier *f);
partls_status partls_frontier_next(partls_frontier *f, int64_t *total, int64_t *mine, uint64_t *pat, uint64_t *free_groups,
                                   int32_t *src_slot, int32_t *per_rank);
partls_status partls_frontier_ingest(partls_frontier *f, const double *lb, const int32_t *branch, const int32_t *dst_slot,
                                     int32_t *dead, int64_t dead_capacity, int64_t *ndead);
partls_status partls_frontier_result(const partls_frontier *f, double *mu, uint64_t *pat, uint64_t *free_groups, int64_t *nodes);
/* The search itself (what partls_fit_bnb / partls_bnb_prepared run before partls_bnb_leaf): best-first frontier, device batches,
 * every node warm-started from its parent's final tableau, which stays in HBM while the node has children in the frontier
 * (BnB.jl:120-124: a child is the parent's constraint set plus one group).  Returns the incumbent node (pat, free_groups), its
 * value *mu and the number of nodes bounded.  max_nodes > 0 stops the search there (measurement; *mu = +inf when no feasible
 * node was met yet); max_nodes <= 0 runs to optimality. */
partls_status partls_bnb_search(partls_ctx *ctx, int64_t max_nodes, double *mu, uint64_t *pat, uint64_t *free_groups, int64_t *nodes);

/* ---- predict(α, β, t, P, X)  — replaces PartitionedLS.jl:132-134: yhat = X*(P.*α)*β .+ t ------------------------------ */
partls_status partls_predict(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX,
                             const int64_t *P, int64_t K, int64_t ldP, const double *alpha, const double *beta, double t,
                             double *yhat);
/* The same with X (N x M, ldX) and yhat (N) resident in HBM: DEVICE pointers that stay owned by the caller (the large-N
 * form of PartitionedLS.jl:132-134 — no PCIe copy of X; P, alpha, beta stay host pointers, they are M*K numbers). */
partls_status partls_predict_device(partls_ctx *ctx, const double *dX, int64_t N, int64_t M, int64_t ldX,
                                    const int64_t *P, int64_t K, int64_t ldP, const double *alpha, const double *beta,
                                    double t, double *dyhat);

/* partls_predict_f32 / partls_predict_device_f32: the two predicts for an X stored as float (partls_f32.h). */

/* ---- predict from B models in one pass over X; per-row order statistics and mean of the B predictions ------------
 * Model b is (alpha[:, b], beta[:, b], t[b]) over the one partition P: alpha is M x B (leading dimension M), beta K x B (leading
 * dimension K), t has B entries — the layouts partls_opt_weightings writes (with ld_alpha = M, ld_beta = K), all HOST arrays, as are P
 * and ranks.  Column b of the N x B predictions is what partls_predict returns for model b, bit for bit (the same weights w_b, the same
 * four chains over m mod 4, ((a0 + a1) + (a2 + a3)) + t_b); X is read once per PARTLS_PREDICT_MANY_CHUNK models, not once per model.
 * Outputs, each optional, at least one of them wanted:
 *   yhat  (N x B column-major, leading dimension ldY >= N; NULL: not wanted, ldY ignored): rows N .. ldY of a column are not written;
 *   stats (N x nr column-major, leading dimension N; NULL if and only if nr == 0): stats[i, q] = the value at position ranks[q]
 *         (0-based, 0 <= ranks[q] < B, nr <= PARTLS_PREDICT_MANY_MAX_B) of the ascending sort of row i's B predictions — exact, ties
 *         included, for finite predictions;
 *   mean  (N; NULL: not wanted): (((y_i0 + y_i1) + y_i2) + ... + y_i,B-1) / B, summed in that order.
 * x_on_device = 0: X is a host array, uploaded once and released afterwards; the outputs are host arrays.  When only stats / mean are
 * wanted no N x B array exists on the host or crosses PCIe.  x_on_device = 1 (as in partls_cv_opt): X and every non-NULL output are
 * DEVICE addresses that stay owned by the caller.  Either way the rows are processed in chunks whose N x B intermediate in HBM stays
 * within PARTLS_PREDICT_MANY_BYTES.
 * Errors, all found before any device work: PARTLS_ERR_BAD_ARG for B < 1, no output wanted, stats and nr that disagree, a rank outside
 * [0, B), ldY < N, a NaN / Inf in alpha, beta or t (a failed replicate's NaN row never reaches the selection); PARTLS_ERR_UNSUPPORTED
 * for B or nr above PARTLS_PREDICT_MANY_MAX_B (predict a larger set of models in slices of columns); otherwise those of partls_predict.
 * The context's prepared problem, if any, is untouched. */
#define PARTLS_PREDICT_MANY_CHUNK 16                 /* models per pass over X                          */
#define PARTLS_PREDICT_MANY_MAX_B 4096               /* most models (and most ranks) of one call        */
#define PARTLS_PREDICT_MANY_BYTES (64ULL << 20)      /* 64 MiB: the N x B intermediate of a row chunk   */
partls_status partls_predict_many(partls_ctx *ctx, const double *X, int64_t N, int64_t M, int64_t ldX, int x_on_device,
                                  const int64_t *P, int64_t K, int64_t ldP, int64_t B, const double *alpha, const double *beta,
                                  const double *t, double *yhat, int64_t ldY, int64_t nr, const int64_t *ranks, double *stats,
                                  double *mean);
/* partls_predict_many_f32: the same for an X stored as float (partls_f32_more.h). */

/* ---- synthetic inputs of BASELINE.md §4, generated in HBM (bit-identical to oracle_synth on the host) -----------------
 * dX: device N x D (ld = N), dy: device N; wstar: HOST D doubles (alpha*_j beta*_g(j), from partls_synth_truth). */
partls_status partls_synth_truth(uint64_t seed, int64_t D, int64_t K, int64_t *P, double *wstar);
partls_status partls_synth_device(partls_ctx *ctx, uint64_t seed, int64_t N, int64_t D, const double *wstar,
                                  double *dX, double *dy);

/* ---- measurement: HIP-event timings (ms) of the kernels of the LAST staged/fit call on this context -------------------- */
typedef enum {
    PARTLS_T_GRAM = 0,      /* gram_build + slab reduction            */
    PARTLS_T_PREP = 1,      /* η / scaling / tableau layout           */
    PARTLS_T_SWEEP = 2,     /* the sign-pattern sweep kernel          */
    PARTLS_T_FINISH = 3,    /* winner re-solve + residual from data   */
    PARTLS_T_CALIB = 4,     /* bit-order calibration of the sweep (0 when it did not run) */
    PARTLS_T_OOB = 5,       /* out-of-bag pass of partls_opt_weightings (0 after every other call) */
    PARTLS_T_RESCUE = 6,    /* PARTLS_OPT_RESCUE_CAPPED: the last launch of the rescue kernel (the last piece's; 0 when none ran) */
    PARTLS_T_COUNT = 7
} partls_timer;
partls_status partls_get_timing(const partls_ctx *ctx, partls_timer which, double *ms);
/* host -> device upload of X inside the last prepare / fit on this context: wall time (ms) and bytes (0 / 0 when the inputs were device
 * pointers).  A host X larger than 8 MB is staged through page-locked buffers by four copier threads (42-55 GB/s on a 57 GB/s link
 * whatever the array's history; a plain copy from pageable memory pays for the pinning first: 8-25 GB/s on a fresh array).  The bytes
 * are those moved: 8 N M for a double X, 4 N M after partls_opt_prepare_f32. */
partls_status partls_get_upload(const partls_ctx *ctx, double *ms, double *bytes);
/* principal pivots executed by the last partls_opt_sweep (fp64 flop accounting: each pivot updates the whole symmetric tableau) */
partls_status partls_get_pivots(const partls_ctx *ctx, int64_t *pivots);
/* entering pivots the last partls_opt_sweep refused under the leave-one-out dependence rule (0 on well-conditioned data; a
 * large count says the data are rank deficient on the unit-diagonal scale — see DESIGN.md §4, numerical notes) */
partls_status partls_get_vetoes(const partls_ctx *ctx, int64_t *vetoes);
/* PARTLS_OPT_RESCUE_CAPPED: what the rescue kernel did in the last partls_opt_sweep, partls_opt_models or partls_opt_top of the context
 * and in the partls_opt_finish / partls_opt_pattern calls since (a partls_fit_opt: its sweep and its finish; zeros when nothing capped,
 * after a prepare, or without the flag): patterns it solved, the pivots it spent on all of them, patterns that ran out of main
 * passes (each optional) */
partls_status partls_get_rescue_stats(const partls_ctx *ctx, int64_t *rescued, int64_t *pivots, int64_t *failed);
/* pivot blocks the cooperative kernel (one node on a global-memory tableau, n > 288) exchanged in the last single-node solve; 0 when
 * that solve ran on another kernel — including the one-workgroup retry after a grid-barrier timeout on a crowded device */
partls_status partls_get_blocks(const partls_ctx *ctx, int64_t *blocks);
/* data-space KKT violation of the model the last partls_opt_finish / partls_bnb_leaf (hence fit(Opt), fit(BnB)) returned: the largest
 * of |x_m'r| (passive or free variable), f_m x_m'r (variable at its bound) and -f_m w_m / max|w| over every variable, r = yo - Xo w
 * computed from the data, in units of ||x_m|| ||y||.  <= 3e-15 on data the Gram form resolves; above 1e-12 (PARTLS_KKT_TOL) the call
 * returns PARTLS_ERR_ILL_CONDITIONED (see there).  min_pivot (optional): the smallest leave-one-out pivot of that model's basis on the
 * unit-diagonal scale, a lower bound of 1 / cond(G_BB) (0 when unknown). */
partls_status partls_get_kkt_violation(const partls_ctx *ctx, double *violation, double *min_pivot);
/* debugging / tests: the sweep kernel the prepared problem runs on (partls_opt_sweep, partls_opt_models, the node solves of
 * partls_bnb_bound* / fit(Alt) / partls_opt_finish) and its tile count T = ceil(n / 16) on the register kernels (0 on the global-memory
 * kernels).  After a partls_cv_opt or partls_opt_weightings (which leave no prepared problem on ctx): the route of that call's
 * problems, which are swept in one batched launch on the register kernels unless PARTLS_CV_SERIAL / PARTLS_RESAMPLE_SERIAL is set.  Read-only: the prepare decides it from n, the flags and the
 * knobs read at partls_create.  PARTLS_ERR_STATE when neither holds. */
typedef enum {
    PARTLS_ROUTE_REG_256 = 1,   /* register-resident tableau, 256-thread workgroups (T <= 10)                            */
    PARTLS_ROUTE_REG_512 = 2,   /* register-resident tableau, 512-thread workgroups (T = 11 .. 18; 19, 20: PARTLS_REG_MAXT) */
    PARTLS_ROUTE_DEFERRED = 3,  /* global-memory tableau, deferred updates (n > 288, PARTLS_OPT_GENERIC_KERNEL)          */
    PARTLS_ROUTE_EAGER = 4      /* global-memory tableau, every block applied at once (PARTLS_EAGER_GENERIC)             */
} partls_route;
partls_status partls_get_sweep_route(const partls_ctx *ctx, int *kernel, int *tiles);
/* distinct subproblems the last partls_opt_finish solved and compared on the data objective (1: the sweep recorded no near tie) */
partls_status partls_get_near_ties(const partls_ctx *ctx, int64_t *evaluated);
/* debugging / tests: copy the Gram products of the prepared problem to the host: G ((M+2) x (M+2), column-major,
 * variables ordered [features, intercept, y]), i.e. G, c = G[:, M+1], yy = G[M+1, M+1], after η has been applied. */
partls_status partls_get_gram(const partls_ctx *ctx, double *G_aug);

/* ---- float32 design matrices: one prepare and two predicts that take X as float (uploaded, kept and read as float; results equal the
 * fp64 path on the widened matrix bit for bit).  Part of this ABI; kept in a header of their own.  partls_f32_more.h: the float32
 * entry points added since (partls_predict_many_f32). */
#include "partls_f32.h"
#include "partls_f32_more.h"
/* ---- sparse design matrices: the prepare and the predict for an X stored in CSR (never densified). */
#include "partls_csr.h"
/* ---- group contributions: the N x K breakdown of the predictions of one or many models, per-row order statistics and mean over the
 * models, per-group sums over the rows. */
#include "partls_contrib.h"
/* ---- regression diagnostics of one model on the prepared problem: leverage, leave-one-out residuals, studentized residuals, Cook's
 * distances, degrees of freedom, standard errors. */
#include "partls_diag.h"
/* ---- robust fits: the Huber / bisquare row weights of a model on the prepared problem, formed on the device, and the re-prepare that
 * swaps the sample weights of a prepared problem without touching X. */
#include "partls_robust.h"
/* ---- generalised linear fits: the working rows of a logistic / Poisson family at a model on the prepared problem, formed on the device,
 * the re-prepare that swaps sample weights and response without touching X, and the inverse link. */
#include "partls_glm.h"

#ifdef __cplusplus
}
#endif
#endif
