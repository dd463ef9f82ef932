// ctx.h — the context behind the opaque partls_ctx handle, the owning buffer types it is made of, and the host helpers the host
// translation units share: api.hip (create / destroy / predict / getters), prepare.hip, sweep_setup.hip, opt.hip, opt_export.hip, refine.hip,
// solvers.hip, multi.hip and the host halves of cv.hip, alt_multi.hip, predict_many.hip, contrib.hip, diag.hip and robust.hip.
#pragma once
#include "common.h"
#include <chrono>
#include <functional>
#include <vector>

namespace partls {

// Every device / page-locked allocation of a context lives in one of the owning types below: non-copyable, released by the
// destructor, so `delete c` frees whatever partls_ctx declares and no list has to be kept in step with it.  runtime_gone() (api.hip)
// is true while partls_destroy drops a context whose HIP runtime no longer answers: release() then only forgets the handle.
bool runtime_gone();
enum class XStorage { dense64, dense32, csr };      // how the prepared problem's X is stored (partls_ctx::storage)
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

struct DevBuf : NoCopy {
    void *p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t b)
    {
        if (b <= bytes && p) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; bytes = 0; if (e != hipSuccess) return e; }
        hipError_t e = hipMalloc(&p, b ? b : 8);
        if (e == hipSuccess) bytes = b;
        return e;
    }
    void release() { if (p && !runtime_gone()) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// device chunks allocated one by one and freed together (the snapshot pool of the BnB search, solvers.hip)
struct DevChunks : NoCopy {
    std::vector<void *> v;
    ~DevChunks() { release(); }
    void release() { if (!runtime_gone()) for (void *q : v) (void)hipFree(q); v.clear(); }
    size_t size() const { return v.size(); }
    void push_back(void *q) { v.push_back(q); }
    void *operator[](size_t i) const { return v[i]; }
};

// page-locked host array of doubles (device -> host copies at full PCIe rate instead of through a staging buffer)
struct PinnedDoubles : NoCopy {
    double *p = nullptr;
    size_t cap = 0, n = 0, cap_prev = 0;
    ~PinnedDoubles() { release(); }
    hipError_t resize(size_t count)
    {
        if (count > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr; cap = 0;
            // (page-locking costs ~0.4 ms a call: grow geometrically, at least a page — the node batches of a BnB search double from round to round)
            size_t want = count > 512 ? count : 512;
            if (want < 2 * cap_prev) want = 2 * cap_prev;
            hipError_t e = hipHostMalloc((void **)&p, want * sizeof(double), hipHostMallocDefault);
            if (e != hipSuccess) return e;
            cap = cap_prev = want;
        }
        n = count;
        return hipSuccess;
    }
    void release() { if (p && !runtime_gone()) (void)hipHostFree(p); p = nullptr; cap = n = 0; }
    double *data() const { return p; }
    size_t size() const { return n; }
    double &operator[](size_t i) const { return p[i]; }
};

// page-locked host array of exactly `count` elements; reads like the plain pointer it owns
template <class T> struct PinnedArray : NoCopy {
    T *p = nullptr;
    ~PinnedArray() { release(); }
    hipError_t alloc(size_t count)
    {
        release();
        const hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void release() { if (p && !runtime_gone()) (void)hipHostFree(p); p = nullptr; }
    operator T *() const { return p; }
};

// staged upload of a host X (prepare.hip: upload_matrix): 4 copier threads x 2 page-locked buffers, one stream each
struct UploadStaging : NoCopy {
    char *pin[8] = {};
    hipStream_t stream[4] = {};
    hipEvent_t event[8] = {};
    ~UploadStaging()
    {
        if (runtime_gone()) return;
        for (int i = 0; i < 8; ++i) { if (pin[i]) (void)hipHostFree(pin[i]); if (event[i]) (void)hipEventDestroy(event[i]); }
        for (int t = 0; t < 4; ++t) if (stream[t]) (void)hipStreamDestroy(stream[t]);
    }
};

// the N events of one call (timing its phases): created together, and whatever was created is destroyed on every way out
template <int N> struct Events : NoCopy {
    hipEvent_t e[N] = {};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipError_t create() { for (hipEvent_t &x : e) { const hipError_t r = hipEventCreate(&x); if (r != hipSuccess) { x = nullptr; return r; } } return hipSuccess; }
};

}  // namespace partls

// Tuning / diagnostic knobs, read from the environment ONCE at partls_create (never on the per-call path).
struct partls_knobs {
    double tol_rel = 1e-11;      // PARTLS_TOL_REL: KKT tolerance relative to ||y||
    long long chain_len = 0;     // PARTLS_CHAIN_LEN: patterns per Gray chain (0 = automatic)
    long long grid = 0;          // PARTLS_GRID: workgroups of the sweep (0 = automatic)
    int gram_S = 0, gram_cr = 0; // PARTLS_GRAM_S / PARTLS_GRAM_CR: Gram work decomposition overrides
    int coop_rows = 0;           // PARTLS_COOP_ROWS: tableau rows per workgroup of the cooperative kernel (0 = automatic)
    bool no_coop = false;        // PARTLS_NO_COOP: single large solves on the one-workgroup kernel
    int reg_maxt = 18;           // PARTLS_REG_MAXT (1..20): tile columns up to which the register kernel runs (n <= 16 x this).  Its T = 19 / 20
                                 // instantiations spill 120-600 VGPRs and lose to the deferred-update kernel since round 4 (65 536 patterns: D = 304
                                 // 5.5 against 6.3 M solves/s, D = 320 2.3 against 6.1 M; BnB nodes 1.03 / 1.01 against 1.12 / 1.01 M per second)
    bool no_staged_upload = false; // PARTLS_NO_STAGED_UPLOAD: host X goes up with one pageable hipMemcpy2DAsync, as through round 3 (A/B tests)
    bool no_export = false;      // PARTLS_NO_EXPORT: the winner is always solved again from the empty basis (A/B tests)
    bool eager_generic = false;  // PARTLS_EAGER_GENERIC: n > 320 on sweep_generic.hip (every block applied to the whole tableau) instead of sweep_lazy.hip (A/B tests)
    int bnb_batch = 1024;        // PARTLS_BNB_BATCH: nodes bounded per device batch of the BnB search
    int bnb_pool_mb = 65536;     // PARTLS_BNB_POOL_MB: cap of the tableau-snapshot pool of the BnB search (warm-started node bounds); chunks are allocated on
                                 // demand, never beyond half of the free HBM.  16 GB (round 3) ran out in the 173 717-node search of bench.py's bnb_hard: the
                                 // late rounds then bounded a sixth of their nodes from the fresh tableau (47 pivots per node instead of 5.7) and took 3x longer
    int bnb_wg_per_cu = 8;       // PARTLS_BNB_WG_PER_CU: workgroups per resident slot in a node batch's grid (1: persistent; 8: one node per workgroup as in round 3)
    bool bnb_cold = false;       // PARTLS_BNB_COLD: every BnB node from the fresh tableau (A/B tests)
    bool lz_fault = false;       // PARTLS_LZ_FAULT (tests): the deferred-update kernel's first panel of workgroup 0 loses its progress word — the followers' bounded
                                 // wait must end it and the sweep must report PARTLS_ERR_NOT_CONVERGED instead of a result
    int coop_fault = 0;          // PARTLS_COOP_FAULT (tests): make the cooperative kernel's grid barrier time out (see SweepParams)
    bool no_tab_refine = false;  // PARTLS_NO_TAB_REFINE: refinement by host Cholesky even when the node solve left its tableau (A/B tests)
    bool finish_trace = false;   // PARTLS_FINISH_TRACE
    bool alt_trace = false;      // PARTLS_ALT_TRACE
    bool alt_always_check = false; // PARTLS_ALT_ALWAYS_CHECK: fit(Alt) verifies its last iteration against the data even when Gershgorin certifies the Gram form (tests)
    bool print_stamps = false;   // PARTLS_PRINT_STAMPS (diagnostic build only)
    int alt_ms_max_rounds = 0;   // PARTLS_ALT_MS_MAX_ROUNDS: pivot cap of the alpha-steps of partls_alt_multistart only (0: 20 (n + 1), as everywhere); tests
    int max_rounds = 0;          // PARTLS_MAX_ROUNDS: pivot cap of every launch that takes the default one (sweep_params; values below 1: 20 (n + 1)); tests
    int rescue_max_passes = 0;   // PARTLS_RESCUE_MAX_PASSES: main passes of the rescue kernel (rescue.hip; values below 1: 3 n); tests
    long long alt_ms_chunk = 0;  // PARTLS_ALT_MS_CHUNK: starts per chunk of partls_alt_multistart (0: what fits 256 MB of per-start scratch)
    double kkt_tol = 1e-12;      // PARTLS_KKT_TOL: data-space KKT violation of the winner (units of ||x_m|| ||y||) above which fit(Opt) / fit(BnB) report
                                 // PARTLS_ERR_ILL_CONDITIONED instead of PARTLS_OK (see kkt_says_ill_conditioned, refine.hip)
    double near_tie_rel = 1e-13; // PARTLS_NEAR_TIE_REL (tests): width of the near-tie window of the sweep, in units of y'y on the objective^2
    double cal_wb = 1.0, cal_ws = 1.0;  // PARTLS_CAL_WB / PARTLS_CAL_WS: multipliers of the block / scan weights of the bit-order cost model (experiments)
    bool cv_serial = false;      // PARTLS_CV_SERIAL: partls_cv_opt sweeps its problems one after another through partls_opt_sweep (A/B tests, timing)
    bool resample_serial = false; // PARTLS_RESAMPLE_SERIAL: the same for partls_opt_weightings (resample.hip)
    int pair = -1;               // PARTLS_PAIR: 0 / 1 force the pair walk of the 512-thread register kernel off / on; -1 automatic (sweep_pairs, sweep_setup.hip)
    long long top_piece = 0;     // PARTLS_TOP_PIECE: patterns per piece of partls_opt_models, partls_opt_top and a sweep's second pass (0: what PARTLS_OPT_MODELS_PIECE_BYTES admits); tests
    int bit_order = 0;           // PARTLS_BIT_ORDER: 0 automatic (calibrate when the sweep is long enough to repay it), "identity" = 1
                                 // (group k on Gray bit k), "calibrate" = 2 (always measure; small problems in the tests)
    long long contrib_bytes = 0; // PARTLS_CONTRIB_BYTES: byte budget of a row chunk's intermediate in partls_contributions (0: PARTLS_PREDICT_MANY_BYTES);
                                 // tests, which reach a chunk boundary with N ~ 2000 through it
    int batch_piece = 0;         // PARTLS_BATCH_PIECE: problems per piece of the batched routes of partls_cv_opt, partls_opt_weightings and partls_cv_alt
                                 // (0: batch_pieces_begin's byte rule; at most 65535); tests
};

struct partls_ctx {
    int device = 0;
    int ncu = 256;                                 // compute units of the device (256 when the attribute cannot be read); set by partls_create
    partls_knobs knobs;
    hipStream_t stream = nullptr;
    hipEvent_t ev0[PARTLS_T_COUNT] = {}, ev1[PARTLS_T_COUNT] = {};
    bool timed[PARTLS_T_COUNT] = {};
    double ms[PARTLS_T_COUNT] = {};

    // Reset by forget_problem (prepare.hip), the one reset of ctx_prepare, batch_reset and batch_work_prepare — whatever below is derived
    // from a prepared problem or its last sweep or solve: prepared, peers; near_for, near_pat, cand, export_wg; sweep_vetoes, rescue_*,
    // coop_state_valid, coop_fallback; tab_valid; order_ready, order_identity, flip_cost, pair_laid; dw, ds, x_f32, storage; last_upload_*; ms[CALIB], ms[OOB]; rb_have; gl_y0, gl_have, gl_checked.
    // (Not last_kkt / last_min_loo: partls_get_kkt_violation reports them, for the last model returned, without a prepared problem.)
    // problem
    bool prepared = false;
    int64_t N = 0, M = 0, K = 0, ldX = 0;
    double eta = 0.0;
    uint32_t flags = 0;
    bool faithful = false;                         // intercept is a sign-constrained tableau variable (2^(K+1) patterns)
    const void *dX = nullptr;                      // device views (owned copies below, or the caller's): X, elements of type ...
    bool x_f32 = false;                            // ... float (partls_opt_prepare_f32) or double; set by every prepare
    // ... or X is sparse (partls_opt_prepare_csr): dX is nullptr and the data passes read csr (the caller's device arrays, or
    // the uploads ownPtr / ownIdx / ownVal) and csc, the column-ordered copy the prepare builds into cscPtr / cscRow / cscVal.  csrWork: the
    // transposition's per-wave column counts, column totals and error words; csrPart: the Gram's partial columns and corner.  storage says
    // which of the three kinds the prepared problem is; every prepare sets it, forget_problem resets it.
    partls::XStorage storage = partls::XStorage::dense64;
    partls::CsrView csr;
    partls::CscView csc;
    partls::DevBuf ownPtr, ownIdx, ownVal, cscPtr, cscRow, cscVal, csrWork, csrPart;
    partls::DevBuf predPtr, predIdx;               // partls_predict_csr: indptr / indices of a host prediction set (values: predX), released after the call
    const double *dy = nullptr;
    partls::DevBuf ownX, ownY;
    // sample weights of the prepared problem (partls_opt_prepare_weighted / partls_cv_opt_weighted; nullptr: unweighted): dw = w (the
    // caller's device array, or ownW, the upload of a host one), ds = sqrt(w) (ownS, written by weight_prep_kernel; wPart / hPart: its
    // four partials per block).  Every Gram build and every data pass (data_pass) of the problem reads them; a plain prepare clears
    // them.  DESIGN.md §4.7.
    const double *dw = nullptr, *ds = nullptr;
    partls::DevBuf ownW, ownS, wPart;
    bool multi_rank = false;                       // this context belongs to a partls_multi (weighted prepares are refused)
    std::vector<int64_t> P;                        // M x K compact
    std::vector<uint64_t> mask_aug;                // M + 2: features, intercept (bit K), y (0)
    std::vector<uint64_t> pack;                    // staging of the one upload of masks and permutation
    const uint64_t *maskTabP = nullptr;            // views into maskAugD: group masks in tableau order, permutation
    const int *permP = nullptr;
    // gram
    int ldg = 0, chunks = 0;
    partls::DevBuf slab, G, maskAugD /* + maskTabP, permP: one upload */, scale, Tfull, T0reg, scratch, bestObj, bestSol /* [workgroups][n]: solution of every workgroup's best pattern (register kernels) */, bestPat, counters, allOpt,
        wdev, partial, yhatD, gD, nodeCode, nodeSol, nodeObj, predX, predY, gridCtr, nodeTab, nodeBasic, altA, altGA, altHg,
        nodePiv, maskInt, allOptRef, bnbIn, bnbOut, altGersh, amsState, amsWork;   // ams*: partls_alt_multistart (alt_multi.hip)
    // BnB: tableau snapshots of open nodes (solvers.hip: SnapshotPool), kept across fits; host staging of a node batch
    partls::DevChunks bnbChunks;
    size_t bnbSlotBytes = 0, bnbMaxSlots = 0;
    int bnbChunkSlots = 512;
    std::vector<int> bnbFree, bnbRefs;             // free slots; reference counts of the in-library search (the ABI's host keeps its own)
    // rows of X sharded over several devices (partls_fit_opt_multi): the contexts that hold the OTHER row blocks of the problem this
    // context is prepared for; every pass over the data (data_pass, refine.hip) then covers them too.  Cleared by every prepare.
    std::vector<partls_ctx *> peers;
    partls::PinnedDoubles hPart, hGpart;           // host staging of a data pass (page-locked like every device -> host destination of a fit: a pageable
                                                   // one costs 17-30 us of runtime staging per copy and blocks the caller — a third of a C2-sized fit's host time)
    partls::PinnedDoubles sweepOut, nodeOut, exportSol;   // ... of a sweep's per-workgroup results, of a node batch, of the sweep's solution of its winner
    // partls_opt_models: one piece's scaled rows + objectives, its cleaned outputs, the export's own counters, and their page-locked staging
    partls::DevBuf mdlRows, mdlOut, mdlCtr;
    partls::PinnedDoubles mdlStage;
    // partls_opt_top (topk.hip) shares them (mdlRows: a piece's rows + objectives; mdlOut: the cleaned outputs of its k
    // rows) and adds: topWork, the selection's state and survivor lists; topRows, the k selected rows, objectives and Gray indices
    partls::DevBuf topWork, topRows;
    // PARTLS_OPT_RESCUE_CAPPED (rescue.hip): rescueScratch, one tableau per workgroup of the rescue kernel; rescueList,
    // [count | rescued | pivots | failed | vetoes | ...] and the list of a piece's capped rows (or one pattern, its row and objective);
    // rescueStage, the host copy of that head (and of the single pattern's row).  rescue_*: the sums of the last call that can rescue
    // (partls_get_rescue_stats), zeroed when such a call begins
    partls::DevBuf rescueScratch, rescueList;
    partls::PinnedDoubles rescueStage;
    unsigned long long rescue_rescued = 0, rescue_pivots = 0, rescue_failed = 0;
    // called between the Gram build and the tableau preparation (partls_fit_opt_multi: the Gram products of the row blocks are summed)
    std::function<partls_status(partls_ctx *)> gram_hook;
    partls::PinnedDoubles amsHostIn, amsHostOut;   // ... of an iteration of partls_alt_multistart: the active list up, the records back
    partls::PinnedDoubles bnbHostIn, bnbHostOut;   // page-locked staging of a node batch (8-byte words): the two copies of a round cost ~10 us each instead of ~25 pageable
    // staged upload of a host X (upload_matrix); wall time and bytes of the last one (0 when the inputs were device-resident)
    partls::UploadStaging up;
    double last_upload_ms = 0.0, last_upload_bytes = 0.0;
    partls::PinnedDoubles hG;                      // host copy of the augmented Gram (pinned: 0.8 MB per prepare at C3)
    partls::PinnedDoubles hScale;
    // tableau: variable i of the tableau is augmented-Gram index perm[i] (features grouped by partition)
    int n = 0, kbits = 0, T = 0;
    std::vector<int> perm;
    std::vector<uint64_t> mask_tab;
    bool use_reg = false;
    // pair walk: the live variables of the group on Gray bit 0 have been moved into one tile column (pair_relayout, sweep_setup.hip; perm and
    // everything laid out by it rebuilt), once per prepare behind the calibration (prepare_sweep_order).  Cleared by ctx_prepare_tableau;
    // sweep_pairs holds only on such a context, so the problems partls_cv_opt prepares one after another on cv_work under one calibration
    // keep the prepare's layout and the plain walk.
    bool pair_laid = false;
    std::vector<uint64_t> mask_int_host;           // staging of maskInt's upload after a relayout (lives as long as the copy may)
    // Opt sweep: which group sits on which bit of the Gray index (calibrate_bit_order, once per prepare, on the first sweep).
    // The boundary speaks the reference's pattern index (group k = bit k, Opt.jl:4-12) everywhere; only the sweep kernel and the
    // Gray-index ranges of partls_opt_sweep live in the internal order.
    partls::BitOrder order{};
    bool order_ready = false, order_identity = true;
    std::vector<double> flip_cost;                 // measured pivots per flip of group k (empty when not calibrated)
    double tol = 0.0;
    unsigned long long last_pivots = 0, last_vetoes = 0, last_blocks = 0;
    // near ties of the last sweep (reference pattern indices whose tracked objective^2 lies within the Gram form's own error of the
    // winner's): partls_opt_finish re-ranks them by the objective computed from the data before it fixes the winner
    std::vector<int64_t> near_pat;
    int64_t near_for = -1;
    // the same with the tracked objectives, winner first: what the ranks of a sharded enumeration exchange (partls_opt_candidates /
    // partls_opt_merge_candidates) so that every rank re-ranks the set a single context would
    std::vector<std::pair<double, int64_t>> cand;
    int64_t last_near_evaluated = 0;               // distinct subproblems the last partls_opt_finish solved (1: no near tie)
    int export_wg = -1;                            // row of bestSol with the solution of the last sweep's winner (-1: none)
    double last_kkt = 0.0;                         // data-space KKT violation of the last finished winner
    double last_min_loo = 0.0;                     // smallest leave-one-out pivot of the basis of the last refined node solve (0: unknown)
    unsigned long long sweep_vetoes = 0;           // leave-one-out refusals of the last sweep (node solves overwrite last_vetoes)
    bool coop_state_valid = false;                 // scratch holds the tableau/basis of the previous cooperative solve
    bool coop_fallback = false;                    // the cooperative attempt of the current solve timed out at its grid barrier
    // final tableau of the last single-node solve on the register kernel (pinned host copies; see solve_nodes `want_tab`)
    partls::PinnedArray<double> hTab;
    partls::PinnedArray<int8_t> hBasic;
    size_t hTabDoubles = 0;
    bool tab_valid = false, tab_full = false;
    // partls_cv_opt (cv.hip): internal same-device contexts, created on first use and destroyed with this one.  cv_work holds one problem
    // at a time for the finish (its G, tableau, winner); cv_view[g] is a view of the rows of fold g (dX, dy, N, ldX into this context's
    // upload) — the peers of cv_work's data passes and the target of the held-out residual.  cvG: fold Grams, then the combined Grams;
    // cvBatch: stacked per-problem state of a piece (BatchPiece: scale, tolerances, Tfull, T0reg, the caller's tail); cvHost: host copies.
    partls_ctx *cv_work = nullptr;
    std::vector<partls_ctx *> cv_view;
    partls::DevBuf cvG, cvBatch, cvEta;
    partls::PinnedDoubles cvHost, cvHostG;
    // partls_opt_weightings (resample.hip) shares cv_work and the cv* buffers above (cvG: one Gram per weighting) and
    // adds: rsW, the upload of a host W (N x B, ld N); rsS = sqrt(W) (ld N); rsPart / rsHost, the per-block partials of
    // weight_prep_kernel and of oob_sse_kernel and their host copies; rsWv, the models of a chunk of problems as weight vectors
    partls::DevBuf rsW, rsS, rsPart, rsWv;
    partls::PinnedDoubles rsHost;
    // partls_predict_many and partls_contributions (many_model_pass, predict_many.hip): mmW, the models of a call
    // as the entry blocks them by chunk (predict_many: weight vectors and intercepts; contributions: weights of the group lists, then the
    // lists themselves, gptr[K + 1] and feature indices, int32); mmRanks, the ranks wanted; mmY, the rows x K x B intermediate of a row
    // chunk (K = 1: predictions); mmStats / mmMean, the device images of a host caller's stats and mean for one row chunk; mmSums
    // (contributions), the 3 K B running sums carried across the row chunks, followed by the per-block partial sums of one chunk
    partls::DevBuf mmW, mmRanks, mmY, mmStats, mmMean, mmSums;
    // partls_diagnostics (diag.hip): dgT, the packed tiles of T = L^-1, the index list of the active columns and the
    // prediction weights of the model; dgRow, yhat and the squared norms ||T x_iA||^2 of the rows, followed by the device images of a host
    // caller's per-row outputs; dgSums, the four running sums, followed by the per-block partial sums.  dg_ms: kernel /
    // factorisation / whole call of the last call (partls_get_diagnostics_timing)
    partls::DevBuf dgT, dgRow, dgSums;
    double dg_ms[3] = {0.0, 0.0, 0.0};
    // partls_robust_weights / partls_opt_reweight (robust.hip): rbA, the absolute residuals of the model; rbW, the
    // weights of the last call (read as the previous weights by the next one, which updates them in place); rbState, the selection's
    // state followed by the prediction weights of the model; rbPart / rbHost, the per-block partials of the weight kernel and their host
    // copy.  rb_have: rbW holds the weights of a call since the last prepare (forget_problem clears it; partls_opt_reweight keeps it).
    // csr_seg / csr_S: the Gram plan of a problem prepared from CSR (csr_gram_plan), kept for partls_opt_reweight.  rb_ms: residual
    // pass / selection / weight kernel of the last partls_robust_weights call (partls_get_robust_timing)
    partls::DevBuf rbA, rbW, rbState, rbPart;
    partls::PinnedDoubles rbHost;
    bool rb_have = false;
    int64_t csr_seg = 0;
    int csr_S = 1;
    double rb_ms[3] = {0.0, 0.0, 0.0};
    // partls_glm_working / partls_opt_rework (glm.hip): glEta, the linear predictor of the model; glW, glZ, glMu, the
    // working weights, working response and mean of the last call; glPart / glHost, the row kernel's per-block partials (and the
    // validation's error word) and their host copy; glMean, the staging of partls_glm_mean.  gl_y0: the response the problem was
    // PREPARED with, once a rework has put another one into dy (nullptr: dy is still that response); ownZ: a reworked response the
    // problem owns.  gl_have: glW / glZ hold the rows of a call since the last prepare; gl_checked: bit f set when that response passed
    // the domain check of family f.  forget_problem clears the three, partls_opt_rework keeps them.  gl_ms: residual pass / row kernel
    // of the last partls_glm_working call (partls_get_glm_timing)
    partls::DevBuf glEta, glW, glZ, glMu, glPart, glMean, ownZ;
    partls::PinnedDoubles glHost;
    const double *gl_y0 = nullptr;
    bool gl_have = false;
    unsigned gl_checked = 0;
    double gl_ms[2] = {0.0, 0.0};
};

// propagate a partls_status that is not PARTLS_OK (the host code's counterpart of PARTLS_HIP_CHECK)
#define PARTLS_CHECK(...) do { const partls_status _st = (__VA_ARGS__); if (_st != PARTLS_OK) return _st; } while (0)

namespace partls {

void t_begin(partls_ctx *c, int w);
void t_end(partls_ctx *c, int w);
void t_collect(partls_ctx *c);
// host wall time since t0, in ms (the phases that events cannot time: finishes on the host, the iterations of partls_cv_alt)
inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// Upload (or adopt) X, y; build the Gram products; lay the tableau out.  faithful = intercept is a regular variable.
// w (optional): sample weights, a device pointer when x_on_device (see prepare_weights)
// x_f32: X holds float elements (host or device; ldX in elements) and is kept, uploaded and read as such
partls_status ctx_prepare(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device,
                          const int64_t *P, int64_t K, int64_t ldP, double eta, bool faithful, uint32_t flags, const double *w = nullptr,
                          bool x_f32 = false);
// The same for an X stored in CSR (prepare.hip): everything of ctx_prepare except adopt / upload, the validation and
// the Gram launch.  Host arrays when !x_on_device (the upload is timed and counted: 8 (N + 1) + 12 nnz bytes)
partls_status ctx_prepare_csr(partls_ctx *c, const int64_t *indptr, const int32_t *indices, const double *values, int64_t N, int64_t M,
                              const double *y, const double *w, int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta,
                              bool faithful, uint32_t flags);
// What it shares with partls_predict_csr (api.hip); who: the entry's name in the messages.
// csr_adopt: indptr[0] == 0 and indptr[N] >= 0 checked and read (*nnz), N < 2^31; then device arrays are adopted, host arrays go up into
// up_ptr / up_idx / up_val on c->stream (*bytes = 8 (N + 1) + 12 nnz, *ms: the wall time of the copies) -> *A.
partls_status csr_adopt(partls_ctx *c, const char *who, const int64_t *indptr, const int32_t *indices, const double *values, int64_t N,
                        int64_t M, int x_on_device, DevBuf &up_ptr, DevBuf &up_idx, DevBuf &up_val, CsrView *A, int64_t *nnz,
                        double *bytes, double *ms);
// csr_check: launch_csr_check into err (3 device words) and wcnt (optional), `queue` (optional: more work for the stream, results
// the caller wants after the same wait), one wait, and the status and message of the first failed check: a bad indptr or index ->
// PARTLS_ERR_BAD_ARG naming the first offending row, else NaN / Inf -> PARTLS_ERR_NONFINITE.
partls_status csr_check(partls_ctx *c, const char *who, const CsrView &A, int64_t nnz, unsigned long long *err, unsigned *wcnt,
                        const std::function<partls_status()> &queue);
// c forgets its prepared problem and what its last sweep or solve left behind (the list: partls_ctx); buffers and the upload of X stay
void forget_problem(partls_ctx *c);
// X (elements of esz bytes: 8 or 4) and y: device arrays are adopted, host arrays go up into ownX (ld N) / ownY and the upload is timed
partls_status adopt_or_upload(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device, size_t esz);
// Sample weights w[N] (host, or device when on_device) -> c->dw, c->ds after one weight_prep_kernel pass, or the status of the first
// failed check: NaN / Inf -> PARTLS_ERR_NONFINITE; a negative weight or a sum that is not > 0 -> PARTLS_ERR_BAD_ARG.
partls_status prepare_weights(partls_ctx *c, const double *w, int64_t N, int on_device);
// partls_opt_rework / partls_opt_reweight: the prepared problem of c takes the sample weights w
// (prepare_weights' rules; never NULL) and, unless z is NULL, the response z (host: uploaded into ownZ; device: adopted), and its Gram
// products and tableau are built again — forget_problem, prepare_weights, the storage kind's Gram launch and the ending of every
// prepare, from the X, partition, eta and flags the context holds.  The records of the robust weights and of the GLM rows (with the
// response the problem was first prepared with) survive.  A refusal leaves the context unprepared.
partls_status ctx_rework(partls_ctx *c, const double *w, const double *z, int on_device);
// The second half of ctx_prepare: from the Gram products in c->G (c->M, K, eta, flags, faithful and the partition already set) to the
// tableau, the host copies and the tolerance.  partls_cv_opt calls it on a context whose G it filled itself.
partls_status ctx_prepare_tableau(partls_ctx *c);
// The part of it that follows from c->perm: mask_tab, the packed upload, scale, Tfull, T0reg.  Queues on c->stream, no sync; timed: under
// the PARTLS_T_PREP events
partls_status ctx_layout_tableau(partls_ctx *c, bool timed);
partls_status load_partition(partls_ctx *c, const int64_t *P, int64_t M, int64_t K, int64_t ldP);
// host X (N x M, ldX, elements of `esz` bytes) -> packed device image (ld N) on c->stream, staged through page-locked buffers when large
partls_status upload_matrix(partls_ctx *c, void *dst, const void *X, int64_t N, int64_t M, int64_t ldX, size_t esz = sizeof(double));
// ---- the set-up of a sweep launch (sweep_setup.hip): every launch of a sweep kernel goes through these
constexpr double SWEEP_PIV_EPS = 1e-11;                      // SweepParams::piv_eps of every launch
inline int sweep_max_rounds(int n) { return 20 * (n + 1); }  // SweepParams::max_rounds unless PARTLS_MAX_ROUNDS or the caller overrides it
// The fields every launch shares: n, kbits, mask, scratch (ensure it first: ensure_sweep_scratch), tol, piv_eps, max_rounds, rbit.
// internal_order (chain mode): patterns run in the calibrated bit order — mask = maskInt and rbit = the inverse of c->order unless that
// order is the identity; otherwise mask = maskTabP and rbit = identity.  The caller sets what is its own: the range, the chain
// length, the outputs, the node pointers, the snapshot arrays, the batch fields, the fault hooks, a max_rounds override.
SweepParams sweep_params(const partls_ctx *c, bool internal_order);
// the one scratch-sizing rule: the register kernels take 64 doubles, the global-memory kernels a tableau per workgroup
partls_status ensure_sweep_scratch(partls_ctx *c, int grid);
// Node mode (SweepParams::node_code): sweep_params plus the range [0, nodes) in chains of chain_len, and bestObj / bestPat (sized for the
// grid) for the per-workgroup minima, which the kernels rank in node mode too and nobody reads.  Ensure the scratch first.
partls_status node_sweep_params(partls_ctx *c, size_t nodes, int64_t chain_len, int grid, SweepParams *p);
// the counter words of a launch: [unconverged | pivots | vetoes | (cooperative kernel) blocks], 8 bytes each, zeroed by the caller
inline void bind_counters(SweepParams &p, unsigned long long *w) { p.n_unconverged = w; p.n_pivots = w + 1; p.n_vetoes = w + 2; }
// The per-workgroup result block of a chain-mode sweep, 8-byte words: [counters (4) | best objective (grid) | best pattern (grid)] and,
// with runner_up, [runner-up objective (grid) | runner-up pattern (grid)]; patterns in the internal bit order.
struct SweepBlock { unsigned long long *counters; double *best_obj; int64_t *best_pat; double *second_obj; int64_t *second_pat; };
inline size_t sweep_block_words(int grid, bool runner_up) { return 4 + (runner_up ? 4 : 2) * (size_t)grid; }
inline SweepBlock sweep_block(double *base, int grid, bool runner_up)
{
    double *b = base + 4;
    const size_t g = (size_t)grid;
    return {reinterpret_cast<unsigned long long *>(base), b, reinterpret_cast<int64_t *>(b + g), runner_up ? b + 2 * g : nullptr,
            runner_up ? reinterpret_cast<int64_t *>(b + 3 * g) : nullptr};
}
void bind_sweep_block(SweepParams &p, double *base, int grid, bool runner_up);   // counters, best_*, second_* of p -> the block at base
// The only place that picks a sweep kernel: the register kernel (T0reg), else the deferred-update or, with PARTLS_EAGER_GENERIC, the
// eager global-memory kernel (Tfull).  models: the export instantiation (partls_opt_models; see launch_sweep_blk in common.h)
hipError_t launch_any_sweep(partls_ctx *c, SweepParams &p, int grid, bool models = false);
// the Opt sweep's pieces that partls_cv_opt shares
partls_status calibrate_bit_order(partls_ctx *c);
// fit(Opt) enumerates 2^K' patterns: false (error set, who: the entry's name) beyond K' = 40 (opt.hip)
bool opt_range_ok(const partls_ctx *c, const char *who);
// What every entry that sweeps in chain mode does once per prepare: calibrate_bit_order, then pair_relayout; nothing when the order
// is ready (c->order_ready)
partls_status prepare_sweep_order(partls_ctx *c);
// Pair walk: where the rule of sweep_pairs holds for the whole enumeration, the live variables of the group on Gray bit 0 move into tile
// column T - 2 (sweep_blk.hip prices twins from that column's fixed tile slots); every other variable keeps its relative order.  c->perm
// stays the one map from tableau index to feature.  No host sync.  Nothing changes where the rule does not hold.
partls_status pair_relayout(partls_ctx *c);
bool sweep_plan(partls_ctx *c, int64_t total, int64_t *chain_len_out, int *grid_out, const char *who);
bool sweep_pairs(const partls_ctx *c, int64_t total);   // does partls_opt_sweep walk a range of `total` Gray indices in pairs on this context?
int64_t reference_pattern(const partls_ctx *c, int64_t q);
// sweep_out: the host copy of a result block with runner-up columns (sweep_block)
void install_sweep_result(partls_ctx *c, const double *sweep_out, int grid, bool has_sol, double *bobj_out, int64_t *bpat_out);
// winner (objective, reference pattern; pattern -1: none) and the list it is the best of -> cand, near_pat, near_for (near_tie.h)
void install_candidates(partls_ctx *c, std::pair<double, int64_t> winner, std::vector<std::pair<double, int64_t>> others);
// c->allOpt -> the caller's all_opt under the reference index (through allOptRef unless the order is the identity); queues, no wait
partls_status deliver_all_opt(partls_ctx *c, double *all_opt);

// ---- many problems over one (X, y, P) in one call (cv.hip): what partls_cv_opt, partls_opt_weightings (resample.hip) and partls_cv_alt
// (cv_alt.hip) share.  The caller's context c keeps the upload and the Gram products (c->cvG) and holds no prepared problem
// afterwards; c->cv_work, an internal context on the same device, holds one problem at a time for its finish.  The steps, each
// defined once: batch_work_prepare (cv_work takes the batch's shape); then either batch_prepare_one per problem (the serial route)
// or, after batch_pieces_begin (the piece rule), per piece batch_piece_prepare (all of them prepared on the device) and
// batch_install per problem (its prepared state onto cv_work).  The Opt entries go through batch_calibrate and batch_sweep, which add
// the calibration, the sweeps and the finish callback; partls_cv_alt runs its iterations between the steps itself.
// what the caller gets per problem (host staging; nothing reaches the caller's arrays before the whole call has succeeded); sse: the
// held-out SSE of a cross-validation problem, the out-of-bag SSE of a weighting
struct CvOut {
    std::vector<double> alpha, beta, t, opt, sse;
    std::vector<int64_t> best;
    std::vector<int32_t> status;
    void assign(int64_t B, int64_t M, int64_t K);
    // column q of every array -> the caller's (sse to sse_out unless that is NULL)
    void deliver(int64_t B, int64_t M, int64_t K, double *alpha_out, int64_t ld_alpha, double *beta_out, int64_t ld_beta, double *t_out,
                 double *opt_out, int64_t *best_out, double *sse_out, int32_t *status_out) const;
};
// B problems: problem q reads the Gram G + (q / E) * gs (device; hostG: the host copies at the same stride) with eta[q % E] (host).
// finish(q, bpat, unconv): cv_work holds problem q prepared and swept (winner bpat, -1 when none; unconv patterns hit the pivot cap);
// batch_sweep alone calls it.
struct ProblemBatch {
    int64_t B = 0, E = 1;
    const double *eta = nullptr;
    const double *G = nullptr, *hostG = nullptr;
    int64_t gs = 0;
    bool serial = false;                           // the entry's serial knob: every problem through ctx_prepare_tableau + partls_opt_sweep
    const char *who = "";
    std::function<partls_status(int64_t q, int64_t bpat, int64_t unconv)> finish;
};
partls_status make_internal(partls_ctx *c, partls_ctx **slot);
// ---- what partls_cv_opt and partls_cv_alt (cv_alt.hip) share of a cross-validation call
// the checks of the inputs (not of the outputs or of an entry's own options); who: the entry's name in the messages
partls_status cv_check_inputs(const char *who, partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                              const int64_t *P, int64_t K, int64_t ldP, const int64_t *fold_ptr, int64_t F, const double *eta, int64_t E);
// batch_reset, the weights, the one upload, cv_work and one row view per fold, one Gram per fold and the combined training Grams:
// c->cvG = [max(F, 1) fold Grams | F + 1 training Grams] at stride ldg^2 (the last is all rows'), c->cvHostG = host copy of the latter
partls_status cv_grams(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w, int x_on_device,
                       int64_t K, const int64_t *fold_ptr, int64_t F, uint32_t flags, const char *who, int *ldg_out, int *chunks_out);
// W's data passes cover the training rows of fold f (f == F: all rows): its own rows are the first training fold, the others its peers
void cv_point_rows(partls_ctx *c, partls_ctx *W, const int64_t *fold_ptr, int64_t F, int64_t f);
// o.sse[q] = the SSE of the model in column q of o (with cv_work's partition) on the rows of fold f, from the data
partls_status cv_heldout_sse(partls_ctx *c, int64_t f, int64_t q, CvOut &o);
// c forgets its prepared problem (forget_problem), zeroes every timer and takes the shape of the batch's
void batch_reset(partls_ctx *c, int64_t N, int64_t M, int64_t K, uint32_t flags);
// cv_work takes the batch's shape, partition and Gram layout and is prepared for Gram `cal_gram` at eta[0] with its rows set by
// point_rows(cv_work); no enumeration is set up (partls_cv_alt has none, and so no limit on K)
partls_status batch_work_prepare(partls_ctx *c, const int64_t *P, int64_t ldP, uint32_t flags, int ldg, int chunks, const ProblemBatch &pb,
                                 int64_t cal_gram, const std::function<void(partls_ctx *)> &point_rows);
// ... and the visiting order of the whole batch is calibrated there (the rule of a single fit decides whether that pays)
partls_status batch_calibrate(partls_ctx *c, const int64_t *P, int64_t ldP, uint32_t flags, int ldg, int chunks, const ProblemBatch &pb,
                              int64_t cal_gram, const std::function<void(partls_ctx *)> &point_rows);
// the serial route's prepare of problem q on cv_work: its training Gram, its eta, ctx_prepare_tableau
partls_status batch_prepare_one(partls_ctx *c, const ProblemBatch &pb, int64_t q);
// The batched route begins: *per_piece = the problems of a piece — at most 65535 (gridDim.y), and no more than keep a piece's stacked
// state below PARTLS_OPT_MODELS_PIECE_BYTES; extra: doubles per problem the caller stacks besides the common regions (partls_cv_alt: 1,
// its y'y) — and the eta grid goes to c->cvEta, where the batched kernels read it.
partls_status batch_pieces_begin(partls_ctx *c, const ProblemBatch &pb, size_t extra, int64_t *per_piece);
// Problems [q0, q0 + bc) prepared together: regions of c->cvBatch (their order: batch_piece_prepare), problem q0 + j at row j of each.
struct BatchPiece {
    int64_t q0 = 0;
    int bc = 0;
    size_t tfd = 0, t0d = 0;                       // doubles of one problem's Tfull / T0reg
    double *scale = nullptr, *tol = nullptr, *Tfull = nullptr, *T0reg = nullptr;   // bc x n, bc, bc x tfd, bc x t0d
    double *tail = nullptr;                        // tail_words doubles of the caller's, uninitialised
};
// Ensures and carves c->cvBatch and queues launch_prep_batch and launch_layout_reg_batch on c->stream.  Queues only: the
// caller copies back what it needs ([scale | tol] are contiguous: the piece's head, bc (n + 1) doubles) and waits once per piece.
partls_status batch_piece_prepare(partls_ctx *c, const ProblemBatch &pb, int64_t q0, int bc, size_t tail_words, BatchPiece *pc);
// Problem q0 + j's prepared state onto cv_work — what ctx_prepare_tableau would have left (the batched kernels compute the same
// entries): eta, the host Gram, scale and tolerance from `head` (the host copy of the piece's head), G, scale, Tfull, T0reg, the flags.
partls_status batch_install(partls_ctx *c, const ProblemBatch &pb, const BatchPiece &pc, int j, const double *head);
// prepare and sweep every problem — batched on the register kernels, a piece at a time, or one after another (n > 288,
// PARTLS_OPT_GENERIC_KERNEL, pb.serial) — and call pb.finish on each; fills c->ms
partls_status batch_sweep(partls_ctx *c, const ProblemBatch &pb);
// the tested single-fit finish of problem q on cv_work (its rows already set): partls_opt_finish into column q of o, o.status[q] =
// 0 / PARTLS_ERR_ILL_CONDITIONED / PARTLS_ERR_NOT_CONVERGED (then NaN outputs, best -1); any other status fails the call
partls_status finish_model(partls_ctx *c, int64_t q, int64_t bpat, int64_t unconv, CvOut &o);
// w_m = alpha_m sum_k P[m,k] beta_k over the features and w_M = t: the model of column q of o as predict applies it (PartitionedLS.jl:132)
void model_weights(const partls_ctx *work, const CvOut &o, int64_t q, double *w);

// Solve a batch of `cnt` independent subproblems ("nodes") from the fresh tableau.  codes[i * n + v] is the constraint on
// tableau variable v in node i: +1 (w >= 0), -1 (w <= 0), 0 (w = 0), 2 (free) — see SweepParams::node_code.  sols: cnt x n
// scaled solutions in tableau order (0 for nonbasic); obj2: objective^2 from the tableau corner.
partls_status solve_nodes(partls_ctx *c, const std::vector<int8_t> &codes, size_t cnt, std::vector<double> &sols,
                          std::vector<double> &obj2, unsigned long long *unconv, bool resume = false, bool want_tab = false);
// The same for codes that are already on the device, with everything left there (partls_alt_multistart): enqueues the node-mode
// sweep of `cnt` nodes on c->stream and returns.  code: cnt x n; obj2: cnt; sol: cnt x n; counters: 4 words (unconverged, pivots,
// vetoes, -), zeroed by the caller.  Grid and scratch as solve_nodes; never the cooperative kernel; always from the fresh tableau.
partls_status solve_nodes_device(partls_ctx *c, size_t cnt, const int8_t *code, double *obj2, double *sol,
                                 unsigned long long *counters, int max_rounds);
// ... for ANOTHER problem of the context's shape, partition and kernel (partls_cv_alt): its tile-cyclic tableau T0reg (device) and its
// tolerance instead of the context's.  Register-kernel contexts only.
partls_status solve_nodes_device_at(partls_ctx *c, const double *T0reg, double tol, size_t cnt, const int8_t *code, double *obj2,
                                    double *sol, unsigned long long *counters, int max_rounds);

// ---- the multistart of fit(Alt) (alt_multi.hip), for one problem or for a batch of them
// B problems of the context's shape at the strides of launch_prep_batch / launch_layout_reg_batch: problem p of the piece is problem
// q0 + p of the whole batch and reads the Gram G + ((q0 + p) / E) gs with eta[(q0 + p) % E]
struct AltProblems {
    int64_t B = 1, E = 1, q0 = 0;
    const double *G = nullptr;                     // device
    int64_t gs = 0;
    const double *eta = nullptr;                   // device, E values
    const double *scale = nullptr;                 // device, B x n
    const double *T0reg = nullptr;                 // device, B x t0d
    size_t t0d = 0;
    const double *tol = nullptr;                   // HOST, B
    const double *yy = nullptr;                    // device, B: y'y of each problem's regularised Gram
};
// per-slot tables, slot = problem R + start (each optional); meanings: partls_alt_multistart
struct AltTables {
    double *alpha_all; int64_t ld_alpha_all; double *beta_all; int64_t ld_beta_all;
    double *t_all, *opt_all; int64_t *iters_all; int32_t *status_all;
};
// a problem's best start (-1: none finished) and what alt_finish needs of it
struct AltWinner {
    int64_t start = -1, iters = 0;
    double opt = 0.0;
    std::vector<double> a, b, wv, hdiag;
    std::vector<int8_t> vcode;
};
// pp == nullptr: the context's prepared problem (any kernel); else pp's B problems together (register-kernel context prepared for one
// of them).  Start r of every problem begins at row r of alpha0 / beta0.  win: B winners.  No ending: the caller runs alt_finish.
partls_status alt_multistart_core(partls_ctx *c, const AltProblems *pp, double eps, int64_t T, int64_t R,
                                  const double *alpha0, int64_t ld_alpha0, const double *beta0, int64_t ld_beta0,
                                  const AltTables &tb, AltWinner *win);
// the ending of fit(Alt) (solvers.hip)
partls_status alt_finish(partls_ctx *c, const std::vector<double> &a, const std::vector<double> &b, const std::vector<double> &wv,
                         const std::vector<int8_t> &vcode_last, const std::vector<double> &hdiag, const std::vector<double> &gersh,
                         double optval, int64_t iters_done, unsigned long long unconv_total,
                         double *alpha, double *beta, double *t, double *opt, int64_t *iters);
// ---- PARTLS_OPT_RESCUE_CAPPED (rescue.hip): capped patterns solved again by Lawson-Hanson, one workgroup each, on c->stream
inline bool rescue_on(const partls_ctx *c) { return (c->flags & PARTLS_OPT_RESCUE_CAPPED) != 0; }
// The piece [p0, p0 + cnt) of an export sweep (rows: cnt x n, obj: cnt, both on the device): the rows whose objective is NaN are listed
// and solved, their rows and objectives written in place; a subproblem that runs out of main passes keeps its NaN.  Enqueues the copy
// of the counters to rescueStage; after the stream has been synchronised, rescue_collect adds them to c->rescue_* and turns the
// piece's *unconv (the export's count of capped patterns) into what is still unsolved; the rescue's vetoes are added to *vetoes.
// rescue_begin_call: the counters and the timer of "the last call" start at 0.
void rescue_begin_call(partls_ctx *c);
partls_status rescue_piece(partls_ctx *c, int64_t p0, int64_t cnt, double *rows, double *obj);
// obj[i], the objective of Gray index p0 + i -> all_opt[internal pattern of that index] (the second pass of a sweep)
partls_status rescue_all_opt(partls_ctx *c, const double *obj, int64_t p0, int64_t cnt, double *all_opt);
void rescue_collect(partls_ctx *c, unsigned long long *unconv, unsigned long long *vetoes);
// The second pass of a partls_opt_sweep that reported capped patterns (opt_export.hip): the range again through the export pieces of
// partls_opt_models with the rescue; installs its winner and near ties, fills all_opt (optional), *unconv_io = what stayed unsolved.
// The caller has run rescue_begin_call.
partls_status sweep_second_pass(partls_ctx *c, int64_t g_begin, int64_t g_end, double *all_opt, double *bobj_io, int64_t *bpat_io,
                                unsigned long long *unconv_io);
// one reference pattern, in the format of solve_nodes (sol: n scaled values, 0 for non-basic; obj2; *unconv = 1 when it failed)
partls_status rescue_pattern(partls_ctx *c, uint64_t pattern, std::vector<double> &sol, double *obj2, unsigned long long *unconv);
// node codes of one Opt sign pattern (Opt.jl:28-29): sign of the multiplier sum_k P[m,k] s_k of every tableau variable
void opt_codes(const partls_ctx *c, uint64_t pattern, std::vector<int8_t> &codes);

// scaled tableau solution -> w over [features, intercept] (length M+1); a free intercept is recovered from the Gram copy
void unscale_solution(const partls_ctx *c, const double *sol, std::vector<double> &w);
// ||Xo w - yo||_2 from the data (+ the eta rows): Opt.jl:90
partls_status data_pass(partls_ctx *c, const std::vector<double> &w, bool want_obj, bool want_grad, double *obj2, std::vector<double> *g,
                        const std::function<void()> &overlap);
// grad (optional): Xo'(yo - Xo w) over [features, intercept], from the data (one more pass over X)
partls_status data_objective(partls_ctx *c, const std::vector<double> &w, double *opt, std::vector<double> *grad = nullptr);
bool kkt_says_ill_conditioned(const partls_ctx *c);
double kkt_violation_data(const partls_ctx *c, const std::vector<double> &w, const std::vector<double> &g, const std::vector<int8_t> &code,
                          int *worst);
// Iterative refinement of a solution w (over [features, intercept]) on its own support, in data space: residual and
// X'r on the device; the small SPD solve uses the inverse the pivoting left in the final tableau of the node solve (want_tab;
// register kernel) or, without one, a Cholesky factorisation of the host Gram copy.  Brings a Gram-based solution (error ~ cond^2 eps) to the
// accuracy of a QR-based one (the reference's NNLS) as long as cond^2 eps < 1.  `free_intercept`: the intercept is part
// of the support even when w[M] == 0.
// `out` (optional): objective ||Xo w - yo|| and gradient Xo'(yo - Xo w) at the returned w, when the refinement converged (have)
struct RefineOut { bool have = false; double obj = 0.0; std::vector<double> g; };
partls_status refine_solution(partls_ctx *c, std::vector<double> &w, bool free_intercept, int steps = 2, RefineOut *out = nullptr);
// regularised augmented Gram entry on the host copy
double h_reg(const partls_ctx *c, int a, int b);
// Row-oriented Cholesky of a dense SPD matrix, in place (refine.hip): lower triangle, row-major, leading dimension p; false when a pivot
// is not positive.  The finish's refinement and partls_diagnostics factor the regularised Gram block of a support with it.
bool chol_rows(double *L, int p);
partls_status check_common(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, const void *P, int64_t K, int64_t ldP);
// The weights a prediction applies (api.hip), w[m] = sum over k = 0 .. K-1, in that order, of P[m,k] alpha[m] beta[k]: the ONE definition
// behind partls_predict* and partls_predict_many*, whose columns equal the single predictions bit for bit.  Checks P on the way:
// PARTLS_ERR_BAD_PARTITION for an entry outside {0,1}.
partls_status predict_weights(const int64_t *P, int64_t M, int64_t K, int64_t ldP, const double *alpha, const double *beta, double *w);
// The per-row statistics of predict_many.hip for any column-major rows x B matrix Y on the device (partls_contributions hands them its
// (row, group) pairs as rows), queued on `stream`.  launch_row_select: S[i + q ldS] = the value at position ranks[q] (device array, nr
// of them) of the ascending sort of Y[i, 0 .. B); B <= PARTLS_PREDICT_MANY_MAX_B.  launch_row_mean: mean[i] = the index-ordered sum / B.
hipError_t launch_row_select(const double *Y, int64_t rows, int64_t ldY, int64_t B, const int64_t *ranks, int64_t nr, double *S, int64_t ldS,
                             hipStream_t stream);
hipError_t launch_row_mean(const double *Y, int64_t rows, int64_t ldY, int64_t B, double *mean, hipStream_t stream);
// run[q] += part[blk stride + q] for blk ascending, q < stride: the ONE device fold of per-block partial sums (the callers zero run)
hipError_t launch_fold_partials(const double *part, int64_t blocks, int64_t stride, double *run, hipStream_t stream);
// Shared by the post-fit entries (api.hip).  check_prepared_single: c is not NULL, not a context of a partls_multi and prepared (else
// `unprepared`, which differs between the two robust entries; partls_diagnostics asks in another order and keeps its own lines).  check_models: alpha, beta and (unless NULL) t of B models are finite, else
// PARTLS_ERR_BAD_ARG naming the first that is not ("model b" when the entry takes many).  stage_dense_x: a host X goes up into
// c->predX (packed, ld N); *dX / *ld say where the pass reads X.
partls_status check_prepared_single(const partls_ctx *c, const char *who, partls_status unprepared);
partls_status check_models(const char *who, const double *alpha, int64_t ld_alpha, const double *beta, int64_t ld_beta, const double *t,
                           int64_t M, int64_t K, int64_t B, bool many);
partls_status stage_dense_x(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, int x_on_device, bool x_f32, const void **dX,
                            int64_t *ld);
// One pass of B models over X in row chunks (predict_many.hip), shared by partls_predict_many (K = 1) and partls_contributions (a row
// of X is K rows of the intermediate).  The entry blocks its models into c->mmW and says how a chunk is produced; many_model_check
// holds the rules of nr / stats / ranks and the caps; many_model_pass stages X, walks the chunks (a device caller's `out` is the
// intermediate itself), selects, averages, copies back and releases.
struct ManyModelPass {
    const char *who, *ld_name, *slices;            // the entry, its name for ld_out, its advice at the cap
    int64_t K = 1, B = 0, rmax = 0, ld_out = 0, nr = 0;   // rmax: rows per chunk, by the entry's own rule
    bool x_f32 = false;
    const int64_t *ranks = nullptr;
    double *out = nullptr, *stats = nullptr, *mean = nullptr;   // optional: N x (K B), ld_out (yhat / contrib); N x (K nr) and N x K, ld N
    // rows [r0, r0 + rows) of X (dX, ld: the staged or the caller's matrix, not yet offset) into Y (ld ldy): the entry's kernel
    std::function<hipError_t(const void *dX, int64_t ld, int64_t r0, int64_t rows, double *Y, int64_t ldy)> produce;
    // optional, after a chunk's statistics are queued (partls_contributions: its sums); last: no chunk follows
    std::function<partls_status(const double *Y, int64_t rows, int64_t ldy, bool last)> chunk_done;
};
partls_status many_model_check(const ManyModelPass &mp, int64_t N);
partls_status many_model_pass(partls_ctx *c, const ManyModelPass &mp, const void *X, int64_t N, int64_t M, int64_t ldX, int x_on_device);

}  // namespace partls
