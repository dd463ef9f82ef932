// opt_export.hip — the models of a Gray-index range straight from the sweep kernels: one piece rule and one walk over the pieces for
// partls_opt_models, partls_opt_top and the second pass of a rescuing partls_opt_sweep (DESIGN.md §4 "Every pattern's model", §4.13, §4.14).
#include "ctx.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

namespace partls {

static void par_rows(int64_t rows, size_t row_bytes, const std::function<void(int64_t, int64_t)> &fn)
{
    // the host copy out of the staging buffer: one core moves ~10 GB/s, a piece at C3 is ~1 GB
    const int nt = (size_t)rows * row_bytes < ((size_t)32 << 20) ? 1 : 8;
    if (nt == 1) { fn(0, rows); return; }
    std::vector<std::thread> th;
    const int64_t per = (rows + nt - 1) / nt;
    try {
        for (int i = 1; i < nt; ++i) {
            const int64_t r0 = std::min<int64_t>(rows, i * per), r1 = std::min<int64_t>(rows, r0 + per);
            th.emplace_back(fn, r0, r1);
        }
    } catch (...) {                                          // out of threads: the caller's thread takes the rest
        const int64_t done_from = (int64_t)(th.size() + 1) * per;
        fn(std::min<int64_t>(rows, done_from), rows);
    }
    fn(0, std::min<int64_t>(rows, per));
    for (std::thread &t : th) t.join();
}

static void copy_rows(double *dst, int64_t ld_dst, const double *src, int64_t width, int64_t rows)
{
    if (!dst || width <= 0) return;
    par_rows(rows, (size_t)width * sizeof(double), [&](int64_t r0, int64_t r1) {
        if (ld_dst == width) std::memcpy(dst + (size_t)r0 * width, src + (size_t)r0 * width, (size_t)(r1 - r0) * width * sizeof(double));
        else for (int64_t r = r0; r < r1; ++r) std::memcpy(dst + (size_t)r * ld_dst, src + (size_t)r * width, (size_t)width * sizeof(double));
    });
}

// What partls_opt_models and partls_opt_top share.  export_begin: the preconditions and range rules (who: the entry's name in the messages),
// g_end = -1 resolved, the counters zeroed, the device selected and the visiting order fixed; *empty: an empty range, nothing to do.
// The faithful intercept it requires makes n = M + 1 (ctx_prepare_tableau): a scaled row of the sweep is a raw_alpha row of the caller.
static partls_status export_begin(partls_ctx *c, const char *who, int64_t g_begin, int64_t *g_end_io, const int64_t *pattern,
                                  const double *raw_alpha, int64_t ld_raw, const double *alpha, int64_t ld_alpha, const double *beta,
                                  int64_t ld_beta, const double *t, int64_t *n_unconverged, int64_t *n_vetoes, bool *empty)
{
    if (!c || !c->prepared) { set_error("%s: context not prepared", who); return PARTLS_ERR_STATE; }
    if (!c->faithful) { set_error("%s needs a context prepared with PARTLS_OPT_FAITHFUL_INTERCEPT", who); return PARTLS_ERR_STATE; }
    if (!opt_range_ok(c, who)) return PARTLS_ERR_UNSUPPORTED;
    const int64_t npat = (int64_t)1 << c->kbits, M = c->M, K = c->K;
    int64_t g_end = *g_end_io;
    if (g_end < 0) g_end = npat;
    if (g_begin < 0 || g_begin > g_end || g_end > npat) { set_error("%s: bad Gray-index range [%lld,%lld)", who, (long long)g_begin, (long long)g_end); return PARTLS_ERR_BAD_ARG; }
    if (!pattern) { set_error("%s: pattern is NULL", who); return PARTLS_ERR_BAD_ARG; }
    if ((alpha || beta || t) && !(alpha && beta && t)) { set_error("%s: alpha, beta and t go together (all three or none)", who); return PARTLS_ERR_BAD_ARG; }
    if ((raw_alpha && ld_raw < M + 1) || (alpha && (ld_alpha < M || ld_beta < K))) { set_error("%s: leading dimension too small", who); return PARTLS_ERR_BAD_ARG; }
    if (n_unconverged) *n_unconverged = 0;
    if (n_vetoes) *n_vetoes = 0;
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    *g_end_io = g_end;
    *empty = g_begin == g_end;
    return *empty ? PARTLS_OK : prepare_sweep_order(c);
}

// export_piece: one piece [p0, p0 + cnt) of the range — one sweep with the export instantiation of the kernel on sweep_plan's plan for cnt
// patterns; the scaled rows go to rows (ld n), the objectives to obj, the counters to the head of mdlCtr.  On the context's stream.
static partls_status export_piece(partls_ctx *c, int64_t p0, int64_t cnt, double *rows, double *obj, const char *who)
{
    int64_t chain_len = 0;
    int grid = 0;
    if (!sweep_plan(c, cnt, &chain_len, &grid, who)) return PARTLS_ERR_UNSUPPORTED;
    // the kernel's per-workgroup block (sweep_block without the runner-up columns): only its counters are read here
    PARTLS_HIP_CHECK(c->mdlCtr.ensure(sizeof(double) * sweep_block_words(grid, false)));
    PARTLS_HIP_CHECK(hipMemsetAsync(c->mdlCtr.p, 0, 4 * sizeof(unsigned long long), c->stream));
    PARTLS_CHECK(ensure_sweep_scratch(c, grid));
    SweepParams p = sweep_params(c, /*internal_order=*/true);
    p.g_begin = p0; p.g_end = p0 + cnt; p.chain_len = chain_len;
    bind_sweep_block(p, c->mdlCtr.as<double>(), grid, false);
    p.node_sol = rows; p.node_obj2 = obj; p.node_ld = c->n;
    PARTLS_HIP_CHECK(launch_any_sweep(c, p, grid, /*models=*/true));
    return PARTLS_OK;
}

// The piece rule: as many patterns as stay below PARTLS_OPT_MODELS_PIECE_BYTES, or PARTLS_TOP_PIECE when that test knob is set; at
// most 2^30 (the selection counts in 32 bits); equal pieces (no short tail piece of cold chain starts).
static int64_t export_piece_size(const partls_ctx *c, int64_t total, size_t bytes_per_pattern)
{
    int64_t cap = std::max<int64_t>(1, (int64_t)(PARTLS_OPT_MODELS_PIECE_BYTES / bytes_per_pattern));
    if (c->knobs.top_piece > 0) cap = (int64_t)c->knobs.top_piece;
    cap = std::min<int64_t>(cap, (int64_t)1 << 30);
    const int64_t npieces = (total + cap - 1) / cap;
    return (total + npieces - 1) / npieces;
}

static size_t models_out_words(const partls_ctx *c) { return 3 + (size_t)c->M + (size_t)c->K; }   // cleaned output per pattern: pattern, optval, t, alpha, beta
// partls_opt_models and the second pass, whose all_opt must be that entry's objectives bit for bit: row, objective, cleaned output
static int64_t models_piece_size(const partls_ctx *c, int64_t total)
{
    return export_piece_size(c, total, ((size_t)c->n + 1 + models_out_words(c)) * sizeof(double));
}

// the kk = min(k, cnt) best rows of a piece in topRows, their objectives and Gray indices; out_pat: their reference patterns (topWork)
struct PieceTop { int64_t kk; double *crow, *cobj; int64_t *glist, *out_pat; };
// a piece as its caller sees it: the export's device rows and objectives, and the words of mdlStage behind the 4-word counter head; top: filled by an enqueue step that selects
struct Piece { int64_t p0, cnt; double *rows, *obj, *stage; PieceTop top; };
struct PieceTotals { unsigned long long unconv = 0, pivots = 0, vetoes = 0; };
using PieceStep = std::function<partls_status(Piece &)>;

// The walk, on the context's stream.  Per piece: the export sweep, the rescue of its capped rows (the caller has run rescue_begin_call),
// the counter head to mdlStage, `enqueue` (the caller's kernels, its copies to pc.stage), ONE synchronisation, the counters (after
// rescue_collect) summed into *tot, `take` (the caller consumes pc.stage).  The caller has sized mdlRows and mdlStage (4 words + its own).
static partls_status walk_pieces(partls_ctx *c, const char *who, int64_t g_begin, int64_t g_end, int64_t piece, bool rescue,
                                 const PieceStep &enqueue, const std::function<partls_status(const Piece &)> &take, PieceTotals *tot)
{
    if (!c->use_reg) c->coop_state_valid = false;                    // the global-memory kernels overwrite the shared tableau scratch
    for (int64_t p0 = g_begin; p0 < g_end; p0 += piece) {
        const int64_t cnt = std::min<int64_t>(piece, g_end - p0);
        double *head = c->mdlStage.data();
        Piece pc{p0, cnt, c->mdlRows.as<double>(), c->mdlRows.as<double>() + (size_t)cnt * c->n, head + 4, {}};
        PARTLS_CHECK(export_piece(c, p0, cnt, pc.rows, pc.obj, who));
        if (rescue) PARTLS_CHECK(rescue_piece(c, p0, cnt, pc.rows, pc.obj));
        PARTLS_HIP_CHECK(hipMemcpyAsync(head, c->mdlCtr.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_CHECK(enqueue(pc));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        unsigned long long cn[3];
        std::memcpy(cn, head, sizeof(cn));
        if (rescue) rescue_collect(c, &cn[0], &cn[2]);
        tot->unconv += cn[0]; tot->pivots += cn[1]; tot->vetoes += cn[2];
        PARTLS_CHECK(take(pc));
    }
    return PARTLS_OK;
}

// select, sort and gather the k best rows of the piece; the selection's 4-word head ([threshold hi | lo | 0 | count]) goes to pc.stage, where they are to pc.top
static partls_status enqueue_piece_top(partls_ctx *c, Piece &pc, int64_t k)
{
    const int64_t kk = std::min<int64_t>(k, pc.cnt);
    double *crow = c->topRows.as<double>(), *cobj = crow + (size_t)kk * c->n;
    pc.top = {kk, crow, cobj, reinterpret_cast<int64_t *>(cobj + kk), topk_work(c->topWork.p, kk).out_pat};
    PARTLS_HIP_CHECK(launch_topk_select(pc.obj, pc.cnt, pc.p0, k, c->kbits, c->order, c->order_identity, c->topWork.p, c->stream));
    PARTLS_HIP_CHECK(launch_topk_gather(pc.rows, pc.obj, c->n, pc.p0, pc.cnt, kk, c->topWork.p, crow, cobj, pc.top.glist, c->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(pc.stage, c->topWork.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return PARTLS_OK;
}

// the count the selection reported in the host copy of its head (TopState::count: min(k, non-NaN entries)), checked against kk
static partls_status top_count(const char *who, const double *head, int64_t kk, int64_t *got)
{
    unsigned long long hd[4];
    std::memcpy(hd, head, sizeof(hd));
    *got = (int64_t)hd[3];
    if (*got < 0 || *got > kk) { set_error("%s: the selection reported %lld rows of at most %lld", who, (long long)*got, (long long)kk); return PARTLS_ERR_HIP; }
    return PARTLS_OK;
}

// `count` scaled rows (in place: raw alpha) -> the cleaned outputs in mdlOut (launch_models_cleanup's layout) -> stage, followed by the
// raw rows when wanted.  glist: the rows' Gray indices (selected rows), or nullptr: p0, p0 + 1, ...
static partls_status enqueue_cleanup(partls_ctx *c, double *rows, const double *obj, int64_t p0, int64_t count, bool want_raw,
                                     const int64_t *glist, double *stage)
{
    const size_t out_w = models_out_words(c);
    double *out = c->mdlOut.as<double>();
    PARTLS_HIP_CHECK(launch_models_cleanup(rows, obj, p0, count, (int)c->M, (int)c->K, c->kbits, c->order, c->order_identity, c->permP,
                                           c->scale.as<double>(), c->maskAugD.as<uint64_t>(), want_raw, out, c->stream, glist));
    PARTLS_HIP_CHECK(hipMemcpyAsync(stage, out, (size_t)count * out_w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (want_raw) PARTLS_HIP_CHECK(hipMemcpyAsync(stage + (size_t)count * out_w, rows, (size_t)count * c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return PARTLS_OK;
}

// PARTLS_OPT_RESCUE_CAPPED: the second pass of a partls_opt_sweep that reported capped patterns (the plain kernels do not say which).
// The range is walked again through the export pieces of partls_opt_models, whose NaN rows the rescue kernel solves (rescue.hip); per
// piece the four best (objective, pattern) pairs are selected on the device (topk.hip) and the host merges them.  The pass is
// authoritative: winner and near ties are installed as a merged set's are (no exported winner row: partls_opt_finish solves the winner
// again), all_opt holds its objectives, *unconv_io what the rescue could not solve.
partls_status sweep_second_pass(partls_ctx *c, int64_t g_begin, int64_t g_end, double *all_opt, double *bobj_io, int64_t *bpat_io,
                                unsigned long long *unconv_io)
{
    const auto w0 = std::chrono::steady_clock::now();
    const int n = c->n;
    const int64_t piece = models_piece_size(c, g_end - g_begin);
    const int64_t K4 = 4, kmax = std::min<int64_t>(K4, piece);
    PARTLS_HIP_CHECK(c->mdlRows.ensure((size_t)piece * (n + 1) * sizeof(double)));
    PARTLS_HIP_CHECK(c->topWork.ensure(topk_work_bytes(kmax)));
    PARTLS_HIP_CHECK(c->topRows.ensure((size_t)kmax * (n + 2) * sizeof(double)));
    PARTLS_HIP_CHECK(c->mdlStage.resize(8 + 2 * (size_t)kmax));
    std::vector<std::pair<double, int64_t>> all;
    PieceTotals tot;
    // behind the counter head: [selection head (4) | objectives (kk) | patterns (kk)]
    PARTLS_CHECK(walk_pieces(c, "partls_opt_sweep", g_begin, g_end, piece, /*rescue=*/true,
        [&](Piece &pc) -> partls_status {
            if (all_opt) PARTLS_CHECK(rescue_all_opt(c, pc.obj, pc.p0, pc.cnt, c->allOpt.as<double>()));
            PARTLS_CHECK(enqueue_piece_top(c, pc, K4));
            PARTLS_HIP_CHECK(hipMemcpyAsync(pc.stage + 4, pc.top.cobj, (size_t)pc.top.kk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            PARTLS_HIP_CHECK(hipMemcpyAsync(pc.stage + 4 + pc.top.kk, pc.top.out_pat, (size_t)pc.top.kk * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
            return PARTLS_OK;
        },
        [&](const Piece &pc) -> partls_status {
            int64_t got = 0;
            PARTLS_CHECK(top_count("partls_opt_sweep", pc.stage, pc.top.kk, &got));
            for (int64_t i = 0; i < got; ++i) {
                int64_t pat = 0;
                std::memcpy(&pat, pc.stage + 4 + pc.top.kk + i, sizeof(pat));
                all.emplace_back(pc.stage[4 + i], pat);
            }
            return PARTLS_OK;
        }, &tot));
    if (all_opt) {                                           // as the first pass returned it, with this pass's entries
        PARTLS_CHECK(deliver_all_opt(c, all_opt));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    c->last_pivots += tot.pivots + c->rescue_pivots;
    c->last_vetoes += tot.vetoes; c->sweep_vetoes += tot.vetoes;
    c->export_wg = -1;
    std::pair<double, int64_t> win{INFINITY, -1};
    if (!all.empty()) win = *std::min_element(all.begin(), all.end());   // argmin's first-index rule
    install_candidates(c, win, std::move(all));
    *bobj_io = win.first; *bpat_io = win.second; *unconv_io = tot.unconv;
    c->ms[PARTLS_T_SWEEP] += ms_since(w0);
    return PARTLS_OK;
}

}  // namespace partls

using namespace partls;

extern "C" {

// Models of a Gray-index range straight from the sweep (include/partls.h).  Per piece (models_piece_size, walk_pieces): the export sweep,
// one launch of the cleanup kernel (models.hip), one copy back through page-locked staging.  Nothing of the last partls_opt_sweep's state
// is touched: the counters and per-workgroup results of the export go to a block of their own (mdlCtr), the winner's row of bestSol stays.
partls_status partls_opt_models(partls_ctx *c, int64_t g_begin, int64_t g_end, int64_t *pattern, double *optval, double *raw_alpha,
                                int64_t ld_raw, double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t,
                                int64_t *n_unconverged, int64_t *n_vetoes)
try {
    bool empty = false;
    const partls_status bs = export_begin(c, "partls_opt_models", g_begin, &g_end, pattern, raw_alpha, ld_raw, alpha, ld_alpha, beta, ld_beta, t,
                                          n_unconverged, n_vetoes, &empty);
    if (bs != PARTLS_OK || empty) return bs;
    const int64_t M = c->M, K = c->K;
    const int n = c->n;
    const size_t out_w = models_out_words(c);
    const int64_t piece = models_piece_size(c, g_end - g_begin);
    PARTLS_HIP_CHECK(c->mdlRows.ensure((size_t)piece * (n + 1) * sizeof(double)));
    PARTLS_HIP_CHECK(c->mdlOut.ensure((size_t)piece * out_w * sizeof(double)));
    PARTLS_HIP_CHECK(c->mdlStage.resize(4 + (size_t)piece * (out_w + (raw_alpha ? (size_t)n : 0))));
    const bool rescue = rescue_on(c);                                // capped rows are solved before the cleanup (rescue.hip)
    if (rescue) rescue_begin_call(c);
    PieceTotals tot;
    PARTLS_CHECK(walk_pieces(c, "partls_opt_models", g_begin, g_end, piece, rescue,
        [&](const Piece &pc) -> partls_status { return enqueue_cleanup(c, pc.rows, pc.obj, pc.p0, pc.cnt, raw_alpha != nullptr, nullptr, pc.stage); },
        [&](const Piece &pc) -> partls_status {
            const double *o = pc.stage;
            const int64_t cnt = pc.cnt;
            const size_t r = (size_t)(pc.p0 - g_begin);
            std::memcpy(pattern + r, o, (size_t)cnt * sizeof(int64_t));
            if (optval) std::memcpy(optval + r, o + cnt, (size_t)cnt * sizeof(double));
            if (t) std::memcpy(t + r, o + 2 * cnt, (size_t)cnt * sizeof(double));
            if (alpha) {
                copy_rows(alpha + r * ld_alpha, ld_alpha, o + 3 * cnt, M, cnt);
                copy_rows(beta + r * ld_beta, ld_beta, o + 3 * cnt + (size_t)cnt * M, K, cnt);
            }
            if (raw_alpha) copy_rows(raw_alpha + r * ld_raw, ld_raw, o + (size_t)cnt * out_w, n, cnt);
            return PARTLS_OK;
        }, &tot));
    if (n_unconverged) *n_unconverged = (int64_t)tot.unconv;
    if (n_vetoes) *n_vetoes = (int64_t)tot.vetoes;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

// The k best patterns of a Gray-index range (include/partls.h).  Per piece (walk_pieces): the export sweep, the
// selection, sort and gather of its k best rows (topk.hip), the cleanup of those rows (models.hip with the list of their Gray
// indices), one copy back.  The host keeps the k best of the pieces' lists by the same order.
static bool top_before(double oa, int64_t pa, double ob, int64_t pb) { return oa < ob || (oa == ob && pa < pb); }

partls_status partls_opt_top(partls_ctx *c, int64_t g_begin, int64_t g_end, int64_t k, int64_t *pattern, double *optval, double *raw_alpha,
                             int64_t ld_raw, double *alpha, int64_t ld_alpha, double *beta, int64_t ld_beta, double *t, int64_t *count,
                             int64_t *n_unconverged, int64_t *n_vetoes)
try {
    bool empty = false;
    const partls_status bs = export_begin(c, "partls_opt_top", g_begin, &g_end, pattern, raw_alpha, ld_raw, alpha, ld_alpha, beta, ld_beta, t,
                                          n_unconverged, n_vetoes, &empty);
    if (bs != PARTLS_OK) return bs;
    if (!optval || !count) { set_error("partls_opt_top: optval or count is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (k < 1 || k > PARTLS_OPT_TOP_MAX_K) { set_error("partls_opt_top: k = %lld outside 1 .. %d", (long long)k, PARTLS_OPT_TOP_MAX_K); return PARTLS_ERR_BAD_ARG; }
    *count = 0;
    if (empty) return PARTLS_OK;
    const int64_t M = c->M, K = c->K;
    const int n = c->n;
    const size_t out_w = models_out_words(c);                         // per selected pattern, as partls_opt_models lays it out
    // the cleaned outputs exist for k rows only: a piece is bounded by its scaled rows and objectives
    const int64_t piece = export_piece_size(c, g_end - g_begin, ((size_t)n + 1) * sizeof(double));
    const int64_t kmax = std::min<int64_t>(k, piece);                 // rows a piece can contribute
    PARTLS_HIP_CHECK(c->mdlRows.ensure((size_t)piece * (n + 1) * sizeof(double)));
    PARTLS_HIP_CHECK(c->mdlOut.ensure((size_t)kmax * out_w * sizeof(double)));
    PARTLS_HIP_CHECK(c->topWork.ensure(topk_work_bytes(kmax)));
    PARTLS_HIP_CHECK(c->topRows.ensure((size_t)kmax * (n + 2) * sizeof(double)));
    PARTLS_HIP_CHECK(c->mdlStage.resize(8 + (size_t)kmax * (out_w + (raw_alpha ? (size_t)n : 0))));
    const bool rescue = rescue_on(c);                                // capped rows are solved before the selection (rescue.hip)
    if (rescue) rescue_begin_call(c);
    // the best rows so far, in order: [optval | pattern | t | alpha (M) | beta (K) | raw (n)] per row
    const size_t roww = 3 + (alpha ? (size_t)(M + K) : 0) + (raw_alpha ? (size_t)n : 0);
    std::vector<double> best, next;
    int64_t nbest = 0;
    PieceTotals tot;
    // behind the counter head: [selection head (4) | cleaned outputs of kk rows | their raw rows]
    PARTLS_CHECK(walk_pieces(c, "partls_opt_top", g_begin, g_end, piece, rescue,
        [&](Piece &pc) -> partls_status {
            PARTLS_CHECK(enqueue_piece_top(c, pc, k));
            return enqueue_cleanup(c, pc.top.crow, pc.top.cobj, pc.p0, pc.top.kk, raw_alpha != nullptr, pc.top.glist, pc.stage + 4);
        },
        [&](const Piece &pc) -> partls_status {
            const int64_t kk = pc.top.kk;
            int64_t got = 0;
            PARTLS_CHECK(top_count("partls_opt_top", pc.stage, kk, &got));
            // merge: both lists are in order; keep the first k
            const double *o = pc.stage + 4;
            const int64_t *opat = reinterpret_cast<const int64_t *>(o);
            const double *oopt = o + kk, *ot = o + 2 * kk, *oal = o + 3 * kk, *obe = oal + (size_t)kk * M, *oraw = o + (size_t)kk * out_w;
            const int64_t keep = std::min<int64_t>(k, nbest + got);
            next.resize((size_t)keep * roww);
            int64_t ia = 0, ib = 0;
            for (int64_t r = 0; r < keep; ++r) {
                double *d = next.data() + (size_t)r * roww;
                const double *a = best.data() + (size_t)ia * roww;
                int64_t apat = 0;
                if (ia < nbest) std::memcpy(&apat, a + 1, sizeof(apat));
                const bool take_a = ia < nbest && (ib >= got || top_before(a[0], apat, oopt[ib], opat[ib]));
                if (take_a) { std::memcpy(d, a, roww * sizeof(double)); ++ia; continue; }
                d[0] = oopt[ib];
                std::memcpy(d + 1, &opat[ib], sizeof(int64_t));
                d[2] = ot[ib];
                double *e = d + 3;
                if (alpha) {
                    std::memcpy(e, oal + (size_t)ib * M, (size_t)M * sizeof(double));
                    std::memcpy(e + M, obe + (size_t)ib * K, (size_t)K * sizeof(double));
                    e += M + K;
                }
                if (raw_alpha) std::memcpy(e, oraw + (size_t)ib * n, (size_t)n * sizeof(double));
                ++ib;
            }
            best.swap(next);
            nbest = keep;
            return PARTLS_OK;
        }, &tot));
    for (int64_t r = 0; r < nbest; ++r) {
        const double *d = best.data() + (size_t)r * roww, *e = d + 3;
        optval[r] = d[0];
        std::memcpy(&pattern[r], d + 1, sizeof(int64_t));
        if (alpha) {
            t[r] = d[2];
            std::memcpy(alpha + (size_t)r * ld_alpha, e, (size_t)M * sizeof(double));
            std::memcpy(beta + (size_t)r * ld_beta, e + M, (size_t)K * sizeof(double));
            e += M + K;
        }
        if (raw_alpha) std::memcpy(raw_alpha + (size_t)r * ld_raw, e, (size_t)n * sizeof(double));
    }
    *count = nbest;
    if (n_unconverged) *n_unconverged = (int64_t)tot.unconv;
    if (n_vetoes) *n_vetoes = (int64_t)tot.vetoes;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_opt_top_select(partls_ctx *c, const double *obj, int64_t cnt, int64_t g0, int64_t k, int64_t *index, int64_t *pattern,
                                    double *optval, int64_t *count)
try {
    if (!c || !c->prepared) { set_error("partls_opt_top_select: context not prepared"); return PARTLS_ERR_STATE; }
    if (!opt_range_ok(c, "partls_opt_top_select")) return PARTLS_ERR_UNSUPPORTED;
    if (!obj || !index || !pattern || !optval || !count) { set_error("partls_opt_top_select: NULL argument"); return PARTLS_ERR_BAD_ARG; }
    if (k < 1 || k > PARTLS_OPT_TOP_MAX_K) { set_error("partls_opt_top_select: k = %lld outside 1 .. %d", (long long)k, PARTLS_OPT_TOP_MAX_K); return PARTLS_ERR_BAD_ARG; }
    const int64_t npat = (int64_t)1 << c->kbits;
    if (cnt < 0 || cnt >= ((int64_t)1 << 31) || g0 < 0 || g0 > npat || cnt > npat - g0) { set_error("partls_opt_top_select: bad range g0 = %lld, cnt = %lld", (long long)g0, (long long)cnt); return PARTLS_ERR_BAD_ARG; }
    *count = 0;
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    if (cnt == 0) return PARTLS_OK;
    PARTLS_CHECK(prepare_sweep_order(c));
    const int64_t kk = std::min<int64_t>(k, cnt);
    PARTLS_HIP_CHECK(c->mdlRows.ensure((size_t)cnt * sizeof(double)));
    PARTLS_HIP_CHECK(c->topWork.ensure(topk_work_bytes(kk)));
    PARTLS_HIP_CHECK(c->mdlStage.resize(4 + 2 * (size_t)kk));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->mdlRows.p, obj, (size_t)cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PARTLS_HIP_CHECK(launch_topk_select(c->mdlRows.as<double>(), cnt, g0, k, c->kbits, c->order, c->order_identity, c->topWork.p, c->stream));
    double *hs = c->mdlStage.data();                                  // [selection head (4) | out_idx (kk) | out_pat (kk)]
    PARTLS_HIP_CHECK(hipMemcpyAsync(hs, c->topWork.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(hs + 4, topk_work(c->topWork.p, kk).out_idx, 2 * (size_t)kk * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    int64_t got = 0;
    PARTLS_CHECK(top_count("partls_opt_top_select", hs, kk, &got));
    std::memcpy(index, hs + 4, (size_t)got * sizeof(int64_t));
    std::memcpy(pattern, hs + 4 + kk, (size_t)got * sizeof(int64_t));
    for (int64_t i = 0; i < got; ++i) {
        if (index[i] < 0 || index[i] >= cnt) { set_error("partls_opt_top_select: selected position out of range"); return PARTLS_ERR_HIP; }
        optval[i] = obj[index[i]];
    }
    *count = got;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

}  // extern "C"
