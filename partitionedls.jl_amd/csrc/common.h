// common.h — internal declarations shared by the HIP translation units of libpartls_hip.so (gfx950 only).  (The rules that the prepare
// path's kernels share with its host code are in prepare_rules.h, which needs no HIP.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>
#include <vector>
#include <string>
#include "../../include/partls.h"

namespace partls {

// ---------------------------------------------------------------------------------------------------------------------
// error plumbing: no exception crosses the C ABI; every entry point returns a status and records a message.
// ---------------------------------------------------------------------------------------------------------------------
void set_error(const char *fmt, ...);
#define PARTLS_HIP_CHECK(expr)                                                                      \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            ::partls::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return PARTLS_ERR_HIP;                                                                  \
        }                                                                                           \
    } while (0)
// the ending of every C-ABI entry (a function-try-block): `try { ... } PARTLS_ABI_GUARD`
#define PARTLS_ABI_GUARD                                                                                                          \
    catch (const std::bad_alloc &) { ::partls::set_error("out of host memory"); return PARTLS_ERR_BAD_ARG; }                      \
    catch (...) { ::partls::set_error("internal error: an exception reached the C ABI"); return PARTLS_ERR_BAD_ARG; }

// The block sum of the 256-thread kernels (misc.hip, contrib.hip): a fixed-order tree over red[256] (LDS).  Every thread calls it; all get the sum.
__device__ __forceinline__ double block_sum_256(double *red, double v)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}

// NV values at once: one pass of the same tree over NV rows of LDS, slot j by fmax when bit j of MAXMASK is set, else by + (operands
// and order are block_sum_256's: a sum keeps its bits).  All threads get all results; a barrier goes in front of a second call.
template <int NV, unsigned MAXMASK = 0>
__device__ __forceinline__ void block_tree_256(double (*red)[256], double (&v)[NV])
{
#pragma unroll
    for (int j = 0; j < NV; ++j) red[j][threadIdx.x] = v[j];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                if ((MAXMASK >> j) & 1u) red[j][threadIdx.x] = fmax(red[j][threadIdx.x], red[j][threadIdx.x + h]);
                else red[j][threadIdx.x] += red[j][threadIdx.x + h];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = red[j][0];
}

// ---------------------------------------------------------------------------------------------------------------------
// sweep parameters (shared by the register-resident and the global-memory tableau kernels)
// ---------------------------------------------------------------------------------------------------------------------
struct BitOrder { uint8_t gbit[40]; };                  // group k of the reference sits on bit gbit[k] of the internal pattern

struct SweepParams {
    int n;                       // tableau variables (features [+ intercept when it is sign-constrained])
    int kbits;                   // bits of the pattern space (K' = number of groups that carry a sign)
    const uint64_t *mask;        // [n] group-membership bit mask of every variable (bit k = member of group k)
    const double *T0;            // initial tableau, kernel-specific layout
    double *scratch;             // generic kernel: per-workgroup tableau scratch
    int64_t g_begin, g_end;      // Gray-index range [g_begin, g_end)
    int64_t chain_len;           // patterns per chain (fresh tableau at the start of every chain)
    double tol;                  // feasibility tolerance on the rhs column (scaled units)
    double piv_eps;              // an entering pivot below this is treated as a dependent column and skipped
    int max_rounds;              // cap on exchange rounds per pattern
    int pair;                    // host only (launch_sweep_blk picks the instantiation; no kernel reads it): != 0: the pair walk — of two patterns that
                                 // differ in internal bit 0 the tableau visits one, the other is priced from its violators' columns (chain mode
                                 // of the 512-thread register kernel up to T = 16, sweep_blk.hip).  It sits in the padding behind max_rounds: no
                                 // field moves and the kernel argument keeps its size — appended at the end it grew the argument by 8 bytes and
                                 // the BATCH kernels' scratch from 320 to 328 bytes
    double *all_opt;             // optional [2^kbits] objective per pattern index
    double *best_obj;            // [gridDim.x] per-workgroup minimum objective
    int64_t *best_pat;           // [gridDim.x] its pattern index (internal bit order; ties broken on the REFERENCE index, see rbit)
    double *best_sol;            // optional [gridDim.x][node_ld] (register kernels, chain mode): scaled solution of the workgroup's best pattern
                                 // (0 for nonbasic variables), written whenever the workgroup finds a new minimum
    double *second_obj;          // optional [gridDim.x]: the workgroup's runner-up (second smallest objective, a different pattern) and
    int64_t *second_pat;         // its pattern, -1 if none: candidates of the host's near-tie re-rank by the data objective (api.hip)
    BitOrder rbit;               // chain mode: rbit.gbit[b] = the reference's bit (group) that internal pattern bit b carries.  Only
                                 // exact objective ties read it: argmin keeps the first REFERENCE index (Opt.jl:96)
    unsigned long long *n_unconverged;   // patterns that hit max_rounds
    unsigned long long *n_pivots;        // total pivots on the (n+1)^2 tableau (diagnostics / flop accounting)
    unsigned long long *n_vetoes;        // entering pivots refused by the leave-one-out rule (diagnostics)
    // Node mode (Alt alpha-steps, BnB node bounds): when node_code != nullptr chain c is ONE subproblem whose constraint on
    // tableau variable v is node_code[c * node_ld + v]:  +1 (w_v >= 0), -1 (w_v <= 0), 0 (w_v = 0: zero multiplier, or both
    // sign constraints of an overlapping partition), 2 (free: BnB's not yet branched groups, BnB.jl:70-79).  Per VARIABLE, not
    // per group: Alt's multipliers sum_k P[m,k] beta_k (Alt.jl:80-81) and BnB's accumulated constraints (BnB.jl:120-121) are
    // not functions of a group sign pattern once a feature sits in two groups.  Outputs per node:
    // node_sol[c * node_ld + v] = scaled solution (0 for nonbasic), node_obj2[c] = objective^2.
    // chain_len is 1 everywhere except in the bit-order calibration (api.hip: calibrate_bit_order; register and one-workgroup
    // global-memory kernel): there chain c
    // solves the nodes c * chain_len + 0, 1, ... one after the other, each warm-started from its predecessor's tableau, node_sol /
    // node_obj2 describe the LAST node of the chain, and node_piv[3 * (c * chain_len + i) + 0 / 1 / 2] = pivots / block pivots / KKT
    // scans of the workgroup up to and including node i (the global-memory kernel reports pivots only).
    const int8_t *node_code;
    double *node_sol;
    double *node_obj2;
    int node_ld;
    // optional (register kernel, node mode): the final tableau of node c in the tile-cyclic layout of T0 (sweep_reg_t0_doubles per
    // node) and its basis flags [16 T per node] — the basic x basic block is -(B_BB)^-1 on the unit-diagonal scale, which the
    // winner's iterative refinement uses as its solver (api.hip: refine_solution)
    double *node_tab;
    int8_t *node_basic;
    unsigned *node_piv;          // optional (see above)
    // optional (register kernel, node mode, chain_len == 1): tableau SNAPSHOTS — warm starts of BnB node bounds (BnB.jl:120-124: a child
    // is its parent's problem plus one group's sign constraint, so it starts from the parent's final tableau and exchanges only that
    // group's wrong-signed variables).  node_src[c]: snapshot node c starts from (nullptr: the fresh tableau T0); node_dst[c]: where its
    // final state is stored (nullptr: nowhere).  A snapshot = sweep_reg_t0_doubles(T) doubles in the layout of T0 (tiles, rhs column,
    // corner) followed by 16 T basis flags (bytes).
    const double *const *node_src;
    double *const *node_dst;
    // cooperative single-node kernel only: continue from the tableau / basis left in `scratch` by the previous launch
    // (warm start of consecutive Alt alpha-steps) instead of reloading T0
    int resume;
    unsigned *grid_ctr;          // multi-workgroup kernel: arrival counter [0] and abort word [1] of its grid barrier (zeroed by the launcher)
    int coop_fault;              // test hook (PARTLS_COOP_FAULT): the grid barrier expects this many arrivals too many, i.e. it can
                                 // only time out — exercises the abort word and the host's one-workgroup fallback.  77 in a launch of the deferred-update
                                 // kernel (PARTLS_LZ_FAULT): workgroup 0's first two-phase panel never publishes its progress word
    // Batched chain-mode sweep (partls_cv_opt, cv.hip): the BATCH instantiation of the register kernels runs one problem per blockIdx.y.
    // Problem q starts from T0 + q * batch_t0 with tolerance batch_tol[q]; best_obj, best_pat, second_obj, second_pat and the three
    // counters are offset by q * batch_out 8-byte words, best_sol by q * gridDim.x rows of node_ld.  mask, rbit and the chain plan are
    // the batch's.  Not read by any other instantiation.
    int64_t batch_t0, batch_out;
    const double *batch_tol;
};

// launchers (each returns hipError_t of the launch)
// Exact objective ties (rare path): does internal pattern a come before internal pattern b in the reference's index order?  The
// reference index of a pattern is sum_b bit_b << rbit[b]; of two patterns the one with a 0 in the differing bit of highest reference
// weight is the smaller.
__device__ __forceinline__ bool ref_index_less(unsigned long long a, unsigned long long b, const unsigned char *rbit)
{
    unsigned long long d = a ^ b;
    int top = -1, at = 0;
    while (d) {
        const int i = __builtin_ctzll(d);
        d &= d - 1;
        const int r = rbit[i];
        if (r > top) { top = r; at = i; }
    }
    return top >= 0 && !((a >> at) & 1ULL);
}

// models = true (chain mode only, partls_opt_models): the export instantiation of the kernel — every pattern's scaled solution goes to
// row g - g_begin of node_sol (leading dimension node_ld) and its objective (sqrt of the corner, all_opt's value) to node_obj2[g - g_begin];
// NaN in both for a pattern that hit the pivot cap.  best_sol is not written.
hipError_t launch_sweep_generic(const SweepParams &p, int grid, hipStream_t s, bool models = false);   // tableau in global memory, every block applied at once
hipError_t launch_sweep_lazy(const SweepParams &p, int grid, hipStream_t s, bool models = false);      // ... updates deferred (sweep_lazy.hip): the n > 320 path
hipError_t launch_sweep_blk(const SweepParams &p, int T, int grid, hipStream_t s, bool models = false);
// the BATCH instantiation (chain mode, no export): grid x batch workgroups, problem q = blockIdx.y (see SweepParams::batch_t0)
hipError_t launch_sweep_blk_batch(const SweepParams &p, int T, int grid, int batch, hipStream_t s);
// layout_reg of `batch` stacked problems: Tfull + q * (n+1)^2 -> T0reg + q * sweep_reg_t0_doubles(T)
hipError_t launch_layout_reg_batch(const double *Tfull, int n, int T, int batch, double *T0reg, hipStream_t s);
hipError_t launch_sweep_coop(const SweepParams &p, int nwg, hipStream_t s);   // one node, many workgroups (n > 320)
bool       sweep_reg_supported(int n);
int        sweep_reg_tiles(int n);
bool       sweep_reg_exports(int T);                     // the 512-thread kernel of this build leaves its winner's solution behind as well
bool       sweep_reg_small(int T);                       // T tile columns run on the 256-thread kernel (which also exports best_sol)
size_t     sweep_reg_t0_doubles(int T);                  // size of the tile-cyclic initial tableau
int        sweep_reg_concurrency(int T);                 // chains a CU runs at the same time (1: the 512-thread kernel, > 1: small tableaus)
hipError_t launch_layout_reg(const double *Tfull, int n, int T, double *T0reg, hipStream_t s);

// gram build: G_aug = Z'Z with Z = [X 1 y]  (n_aug = M + 2), full symmetric, ld = ldg (multiple of 64)
// (gram_S / gram_cr: tuning overrides read once at partls_create, 0 = automatic)
// sw (optional, device, N): s = sqrt(w) of the sample weights -> G_aug = Z~'Z~ with Z~ = diag(s) [X 1 y]
size_t     gram_slab_doubles(int64_t N, int64_t M, int gram_S, int gram_cr, int *chunks_out, int *ldg_out);
// x_f32 (here and in launch_residual / launch_xtr): X holds float elements (ldX counts elements); each is widened to double as it is
// loaded, so the results are those of the widened matrix bit for bit
hipError_t launch_gram(const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, double *slab, int chunks,
                       int ldg, int gram_S, int gram_cr, double *G, hipStream_t s, const double *sw = nullptr, bool x_f32 = false);
// `batch` weighted Grams of one X in one launch pair (partls_opt_weightings): weighting b stages sw + b N, uses the slab
// slab + b slab_stride (slab_stride >= gram_slab_doubles) and writes G + b gstride; each is launch_gram(..., sw + b N)'s result bit for
// bit (the same workgroup body, decomposition and reduction order).  Double X only; batch <= 65535.
hipError_t launch_gram_weightings(const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, double *slab, int64_t slab_stride,
                                  int chunks, int ldg, int gram_S, int gram_cr, double *G, int64_t gstride, const double *sw, int batch,
                                  hipStream_t s);
// sample weights (misc.hip, one kernel): column b of W (N x batch, ld ldW) -> column b of S = sqrt(W) (ld N) and, per block x of
// weight_prep_blocks(N) = nb, part[4 (b nb + x) ..] = (any w < 0, any non-finite w, sum of w, rows with w == 0); batch <= 65535.  The
// host folds a column's blocks in index order (fold_weight_partials, prepare_rules.h).  launch_weight_prep: one column, ldW = N.
int        weight_prep_blocks(int64_t N);
hipError_t launch_weightings_prep(const double *W, int64_t N, int64_t ldW, int batch, double *S, double *part, hipStream_t st);
inline hipError_t launch_weight_prep(const double *w, int64_t N, double *s, double *part, hipStream_t st) { return launch_weightings_prep(w, N, N, 1, s, part, st); }
// out-of-bag SSE of `batch` models: part[b nb + x] = sum over block x's rows with W[i, b] == 0 of (X[i,:] wv_b[0..M) + wv_b[M] - y_i)^2,
// wv: batch x (M + 1), nb = weight_prep_blocks(N); the host adds a problem's blocks in index order; batch <= 65535
hipError_t launch_oob_sse(const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *W, int64_t ldW,
                          const double *wv, int batch, double *part, hipStream_t st);

// tableau prep: B = regularised (and, free-intercept mode, intercept-eliminated) Gram; Tfull = unit-diagonal scaled
// perm[i] = augmented-Gram index of tableau variable i (variables are grouped by partition so a flip touches few tiles)
hipError_t launch_prep(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, int free_intercept,
                       const int *perm, double *scale, double *Tfull, int n, hipStream_t s);
// the same entries (prep_scale_entry, prep_tableau_entry) for `batch` problems at once: slot q = blockIdx.y holds problem q0 + q, which reads the Gram
// G + ((q0 + q) / E) * gstride with eta[(q0 + q) % E] (device array); writes scale + q * n, Tfull + q * (n+1)^2 and
// tol[q] = problem_tol(tol_rel, y'y of the problem's Gram) (prepare_rules.h)
hipError_t launch_prep_batch(const double *G, int64_t gstride, int E, int64_t q0, const double *eta, int ldg, int M, const uint64_t *mask_aug,
                             int free_intercept, const int *perm, double tol_rel, double *scale, double *Tfull, double *tol, int n,
                             int batch, hipStream_t s);

// bit-order calibration (misc.hip): node codes of the calibration walks, and all_opt from internal to reference pattern order
int        walk_flipped_bit(int chain, int step, int kbits, int seg_len, int nseg);
hipError_t launch_walk_codes(const uint64_t *mask, int n, int kbits, int chains, int L, int seg_len, int nseg, int8_t *codes, hipStream_t s);
hipError_t launch_pattern_gather(const double *in, int64_t npat, int kbits, const BitOrder &order, double *out, hipStream_t s);

// partls_opt_models (models.hip): the sweep's scaled solutions of Gray indices [g0, g0 + cnt) -> reference pattern, raw alpha (in place
// over the solution rows, ld n = M + 1), cleanupResult's alpha / beta / t; out = [pattern (cnt int64) | optval (cnt) | t (cnt) |
// alpha (cnt x M) | beta (cnt x K)].  A row whose objective is NaN (pivot cap) gets NaN everywhere.
// glist (optional, device, cnt): row i is Gray index glist[i] instead of g0 + i (partls_opt_top's compact rows)
hipError_t launch_models_cleanup(double *sol, const double *obj, int64_t g0, int64_t cnt, int M, int K, int kbits, const BitOrder &order,
                                 bool order_identity, const int *perm, const double *scale, const uint64_t *mask_aug, bool want_raw,
                                 double *out, hipStream_t s, const int64_t *glist = nullptr);

// partls_opt_top / partls_opt_top_select (topk.hip): the k smallest of obj[0 .. cnt) (device; Gray indices g0 + i) by (objective with
// -0 = +0, reference index), NaN never selected, in that order.  work: topk_work_bytes(kk) device bytes, kk = min(k, cnt); after
// launch_topk_select its first four 8-byte words are [threshold hi | threshold lo | 0 | count] and out_idx / out_pat hold the selected
// positions and their reference indices.  launch_topk_gather: rows out_idx[i] of `rows` (cnt x n) -> crow (kk x n), their objectives ->
// cobj and Gray indices -> glist; rows at and beyond the count get a NaN objective.
constexpr int64_t TOPK_MAX_K = PARTLS_OPT_TOP_MAX_K;
constexpr size_t  TOPK_STATE_BYTES = 2048;
struct TopkWork { uint64_t *sel_hi, *sel_lo; int64_t *sel_idx, *out_idx, *out_pat; };
inline TopkWork topk_work(void *work, int64_t kk)
{
    uint64_t *b = reinterpret_cast<uint64_t *>(static_cast<char *>(work) + TOPK_STATE_BYTES);
    const size_t k = (size_t)kk;
    return {b, b + k, reinterpret_cast<int64_t *>(b + 2 * k), reinterpret_cast<int64_t *>(b + 3 * k), reinterpret_cast<int64_t *>(b + 4 * k)};
}
size_t     topk_work_bytes(int64_t kk);
hipError_t launch_topk_select(const double *obj, int64_t cnt, int64_t g0, int64_t k, int kbits, const BitOrder &order, bool order_identity,
                              void *work, hipStream_t s);
hipError_t launch_topk_gather(const double *rows, const double *obj, int n, int64_t g0, int64_t cnt, int64_t kk, const void *work, double *crow,
                              double *cobj, int64_t *glist, hipStream_t s);

// BnB node batches (misc.hip): per-variable constraint codes of the nodes (pat, free) and (bound, branch) from their solutions
hipError_t launch_bnb_codes(const uint64_t *mask_tab, int n, const uint64_t *pat, const uint64_t *free_, int cnt, int8_t *codes, hipStream_t s);
hipError_t launch_bnb_nu(const double *sol, const double *obj2, int n, const double *scale, const uint64_t *mask_tab, int Kp,
                         const uint64_t *free_, int cnt, double *lb, int *branch, hipStream_t s);

hipError_t launch_gersh(const double *Tfull, int n, double *out, hipStream_t s);   // Gershgorin radii of the scaled Gram block (n doubles)
// residual from the data: out[0] = sum_i (sum_m X[i,m] w[m] + t - y[i])^2   (y may be nullptr -> plain prediction into yhat)
// beta-step system of fit(Alt): Hg[k * (Kp + 1) + k2] = H[k][k2] (k2 < Kp), g[k] (k2 = Kp); GA is (M + 1) x Kp scratch
hipError_t launch_alt_beta_system(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, const double *a, int Kp,
                                  double *GA, double *Hg, hipStream_t s);
// ... of `cnt` starts at once: start j reads a + slot[j] (M + 1), writes GA + j (M + 1) Kp and Hg + j Kp (Kp + 1)   (misc.hip)
hipError_t launch_alt_beta_system_batch(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, const double *a, int Kp,
                                        const int *slot, int cnt, double *GA, double *Hg, hipStream_t s);
// ... of starts of different problems of a batch (partls_cv_alt): start j belongs to problem q = q0 + prob[j] (device array) and reads the
// Gram G + (q / E) gstride with eta[q % E] (device array), the indexing of launch_prep_batch; summed exactly as above
hipError_t launch_alt_beta_system_problems(const double *G, int64_t gstride, int E, int64_t q0, const double *eta, const int *prob, int ldg,
                                           int M, const uint64_t *mask_aug, const double *a, int Kp, const int *slot, int cnt, double *GA,
                                           double *Hg, hipStream_t s);
// wt (optional, device, N): sample weights -> sum_i wt[i] (...)^2
hipError_t launch_residual(const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w, double t,
                           double *partial, int nblocks, double *yhat, hipStream_t s, const double *wt = nullptr, bool x_f32 = false);
// g[0..M] = Xo' (y - yhat): the gradient pass of the data-space refinement (wt: Xo' W (y - yhat))
// gpart: xtr_slices(N) x (M + 1) partial sums; g[m] = sum over the slices in order
int        xtr_slices(int64_t N);
hipError_t launch_xtr(const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *yhat, double *gpart,
                      hipStream_t s, const double *wt = nullptr, bool x_f32 = false);

// ---- a design matrix stored in CSR (csr.hip): device views of the matrix and of its column-ordered (CSC) copy
struct CsrView { const int64_t *indptr = nullptr; const int32_t *indices = nullptr; const double *values = nullptr; int64_t N = 0, M = 0; };
struct CscView { const int64_t *colptr = nullptr; const int32_t *rows = nullptr; const double *values = nullptr; };
constexpr int CSR_MAX_WAVES = 4096;                          // the rows are dealt to at most this many waves, in contiguous ranges
constexpr unsigned long long CSR_NO_ROW = ~0ULL;
int64_t    csr_rows_per_wave(int64_t N);
int        csr_row_waves(int64_t N);
// Validation: err[0..2] (device) = the first row with a bad indptr entry / an index outside [0, M) or not above its predecessor / a
// NaN or Inf value, CSR_NO_ROW where there is none.  nnz = indptr[N] as read by the host (indptr[0] == 0 is the host's check too);
// nothing outside [0, nnz) is read.  wcnt (optional, csr_row_waves(N) x M): the per-wave column counts launch_csr_transpose starts from.
hipError_t launch_csr_check(const CsrView &A, int64_t nnz, unsigned long long *err, unsigned *wcnt, hipStream_t s);
// The CSC copy of a VALID matrix from those counts: launch_csr_colptr (wcnt -> per-wave offsets in place, cnt: M column totals,
// colptr[M + 1]; safe on an invalid matrix too, so it can run before the host has seen err) and launch_csr_place (rows ascending within
// every column, by construction: no sort, no atomics).
hipError_t launch_csr_colptr(const CsrView &A, unsigned *wcnt, unsigned long long *cnt, int64_t *colptr, hipStream_t s);
hipError_t launch_csr_place(const CsrView &A, const unsigned *wcnt, const int64_t *colptr, int32_t *crow, double *cval, hipStream_t s);
// The image launch_gram leaves in G (ldg x ldg, [features, ones, y], full symmetric), from the nonzeros alone; wt (optional): the
// sample weights w (not their roots), entry = sum_i w_i x_ip x_iq.  longest: nonzeros of the longest column; seg / S: nonzeros per wave
// of a column and the most ranges a column has; part: csr_gram_part_doubles(M, S) doubles; corner: 3 doubles.
void       csr_gram_plan(int64_t M, int64_t longest, int64_t *seg_out, int *S_out);
size_t     csr_gram_part_doubles(int64_t M, int S);
hipError_t launch_csr_gram(const CsrView &A, const CscView &T, const double *y, const double *wt, int64_t seg, int S, double *part,
                           double *corner, int ldg, double *G, hipStream_t s);
// launch_residual / launch_xtr for a CSR matrix (X'r reads the CSC copy): the same outputs and fold rules
hipError_t launch_csr_residual(const CsrView &A, const double *y, const double *w, double t, double *partial, int nblocks, double *yhat,
                               hipStream_t s, const double *wt = nullptr);
hipError_t launch_csr_xtr(const CscView &T, int64_t N, int64_t M, const double *y, const double *yhat, double *gpart, hipStream_t s,
                          const double *wt = nullptr);

hipError_t launch_synth(uint64_t seed, int64_t N, int64_t D, const double *wstar_dev, double *X, double *y, hipStream_t s);

// host-side mirror of the device generator (synth.hip); also used by partls_synth_truth
uint64_t rnd64(uint64_t seed, uint64_t stream, uint64_t idx);

}  // namespace partls
