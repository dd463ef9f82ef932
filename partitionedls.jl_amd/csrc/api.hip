// api.hip — the C ABI of include/partls.h that is not a solver: error text, timers, create / destroy, predict, the synthetic data and
// the getters.  (prepare.hip: upload, Gram, tableau; sweep_setup.hip: everything up to a sweep launch; opt.hip: fit(Opt); refine.hip:
// data passes and refinement; solvers.hip: fit(Alt), fit(BnB).)  No CPU fallback: every compute entry needs a HIP device and fails
// with PARTLS_ERR_NO_DEVICE / PARTLS_ERR_HIP otherwise.
#include "ctx.h"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

namespace partls {

static thread_local char g_err[512] = "";
static thread_local bool g_runtime_gone = false;            // set by partls_destroy around `delete c` (ctx.h: runtime_gone)
bool runtime_gone() { return g_runtime_gone; }
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

void t_begin(partls_ctx *c, int w) { (void)hipEventRecord(c->ev0[w], c->stream); }
void t_end(partls_ctx *c, int w) { (void)hipEventRecord(c->ev1[w], c->stream); c->timed[w] = true; }
void t_collect(partls_ctx *c)
{
    for (int w = 0; w < PARTLS_T_COUNT; ++w)
        if (c->timed[w]) {
            float f = 0.f;
            if (hipEventElapsedTime(&f, c->ev0[w], c->ev1[w]) == hipSuccess) c->ms[w] = (double)f;
            c->timed[w] = false;
        }
}

partls_status check_common(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, const void *P, int64_t K, int64_t ldP)
{
    if (!c) { set_error("context is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (!X || !P) { set_error("X or P is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (N < 1 || M < 1 || K < 1) { set_error("need N, M, K >= 1 (got %lld, %lld, %lld)", (long long)N, (long long)M, (long long)K); return PARTLS_ERR_BAD_ARG; }
    if (ldX < N || ldP < M) { set_error("leading dimension smaller than the row count"); return PARTLS_ERR_BAD_ARG; }
    if (ldX >= ((int64_t)1 << 30)) { set_error("ldX = %lld: this build supports leading dimensions below 2^30 rows", (long long)ldX); return PARTLS_ERR_UNSUPPORTED; }
    // group masks are 64-bit words with the intercept's group on bit K; the ENUMERATION of Opt is limited further (see opt_range_ok)
    if (K > 61) { set_error("K = %lld groups: this build supports K <= 61 (Alt, BnB, predict) and K <= 39 for the enumeration of fit(Opt)", (long long)K); return PARTLS_ERR_UNSUPPORTED; }
    if (M + 1 > 1023) { set_error("M = %lld features: this build supports M <= 1022", (long long)M); return PARTLS_ERR_UNSUPPORTED; }
    return PARTLS_OK;
}

double h_reg(const partls_ctx *c, int a, int b)
{
    double v = c->hG[(size_t)a * c->ldg + b];
    if (c->eta != 0.0 && a <= c->M && b <= c->M) v += c->eta * (double)__builtin_popcountll(c->mask_aug[a] & c->mask_aug[b]);
    return v;
}

partls_status predict_weights(const int64_t *P, int64_t M, int64_t K, int64_t ldP, const double *alpha, const double *beta, double *w)
{
    for (int64_t m = 0; m < M; ++m) {
        double s = 0.0;
        for (int64_t k = 0; k < K; ++k) {
            const int64_t v = P[m + k * ldP];
            if (v != 0 && v != 1) { set_error("P has an entry outside {0,1}"); return PARTLS_ERR_BAD_PARTITION; }
            s += (double)v * alpha[m] * beta[k];
        }
        w[m] = s;
    }
    return PARTLS_OK;
}

partls_status check_prepared_single(const partls_ctx *c, const char *who, partls_status unprepared)
{
    if (!c) { set_error("context is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (c->multi_rank || !c->peers.empty()) { set_error("%s: a context of a partls_multi is not supported", who); return PARTLS_ERR_UNSUPPORTED; }
    if (!c->prepared) { set_error("%s: context not prepared", who); return unprepared; }
    return PARTLS_OK;
}

partls_status check_models(const char *who, const double *alpha, int64_t ld_alpha, const double *beta, int64_t ld_beta, const double *t,
                           int64_t M, int64_t K, int64_t B, bool many)
{
    for (int64_t b = 0; b < B; ++b) {
        bool fin = !t || std::isfinite(t[b]);
        for (int64_t m = 0; m < M && fin; ++m) fin = std::isfinite(alpha[m + b * ld_alpha]);
        for (int64_t k = 0; k < K && fin; ++k) fin = std::isfinite(beta[k + b * ld_beta]);
        if (fin) continue;
        if (many) set_error("%s: model %lld has a NaN / Inf in %s", who, (long long)b, t ? "alpha, beta or t" : "alpha or beta");
        else set_error("%s: the model has a NaN / Inf in %s", who, t ? "alpha, beta or t" : "alpha or beta");
        return PARTLS_ERR_BAD_ARG;
    }
    return PARTLS_OK;
}

partls_status stage_dense_x(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, int x_on_device, bool x_f32, const void **dX,
                            int64_t *ld)
{
    *dX = X; *ld = ldX;
    if (x_on_device) return PARTLS_OK;
    const size_t esz = x_f32 ? sizeof(float) : sizeof(double);
    PARTLS_HIP_CHECK(c->predX.ensure((size_t)N * M * esz));
    const partls_status us = upload_matrix(c, c->predX.p, X, N, M, ldX, esz);
    if (us != PARTLS_OK) return us;
    *dX = c->predX.p; *ld = N;
    return PARTLS_OK;
}

}  // namespace partls

using namespace partls;

extern "C" {

int partls_version(void) { return 110; }
const char *partls_last_error(void) { return g_err; }

int partls_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

partls_status partls_create(int device, partls_ctx **out)
try {
    if (!out) { set_error("partls_create: out is NULL"); return PARTLS_ERR_BAD_ARG; }
    *out = nullptr;
    int n = partls_device_count();
    if (n <= 0 || device < 0 || device >= n) {
        set_error("partls_create: no usable HIP device (count=%d, requested=%d); this library has no CPU fallback", n, device);
        return PARTLS_ERR_NO_DEVICE;
    }
    PARTLS_HIP_CHECK(hipSetDevice(device));
    partls_ctx *c = new (std::nothrow) partls_ctx();
    if (!c) { set_error("out of host memory"); return PARTLS_ERR_BAD_ARG; }
    c->device = device;
    if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->ncu < 1) c->ncu = 256;
    // environment knobs: read here, once (the compute entries never call getenv)
    if (const char *e = getenv("PARTLS_TOL_REL")) c->knobs.tol_rel = atof(e);
    if (const char *e = getenv("PARTLS_CHAIN_LEN")) c->knobs.chain_len = atoll(e);
    if (const char *e = getenv("PARTLS_GRID")) c->knobs.grid = atoll(e);
    if (const char *e = getenv("PARTLS_GRAM_S")) c->knobs.gram_S = atoi(e);
    if (const char *e = getenv("PARTLS_GRAM_CR")) c->knobs.gram_cr = atoi(e);
    if (const char *e = getenv("PARTLS_COOP_ROWS")) c->knobs.coop_rows = atoi(e);
    if (const char *e = getenv("PARTLS_PAIR")) c->knobs.pair = atoi(e) != 0 ? 1 : 0;
    if (const char *e = getenv("PARTLS_BIT_ORDER")) c->knobs.bit_order = !strcmp(e, "identity") ? 1 : (!strcmp(e, "calibrate") ? 2 : 0);
    if (const char *e = getenv("PARTLS_ALT_MS_MAX_ROUNDS")) c->knobs.alt_ms_max_rounds = atoi(e);
    if (const char *e = getenv("PARTLS_MAX_ROUNDS")) { const int v = atoi(e); if (v >= 1) c->knobs.max_rounds = v; }
    if (const char *e = getenv("PARTLS_RESCUE_MAX_PASSES")) { const int v = atoi(e); if (v >= 1) c->knobs.rescue_max_passes = v; }
    if (const char *e = getenv("PARTLS_ALT_MS_CHUNK")) c->knobs.alt_ms_chunk = atoll(e);
    if (const char *e = getenv("PARTLS_TOP_PIECE")) c->knobs.top_piece = atoll(e);
    if (const char *e = getenv("PARTLS_BATCH_PIECE")) c->knobs.batch_piece = atoi(e);
    if (const char *e = getenv("PARTLS_CONTRIB_BYTES")) c->knobs.contrib_bytes = atoll(e);
    if (const char *e = getenv("PARTLS_KKT_TOL")) c->knobs.kkt_tol = atof(e);
    if (const char *e = getenv("PARTLS_NEAR_TIE_REL")) c->knobs.near_tie_rel = atof(e);
    if (const char *e = getenv("PARTLS_CAL_WB")) c->knobs.cal_wb = atof(e);
    if (const char *e = getenv("PARTLS_CAL_WS")) c->knobs.cal_ws = atof(e);
    c->knobs.no_coop = getenv("PARTLS_NO_COOP") != nullptr;
    c->knobs.no_export = getenv("PARTLS_NO_EXPORT") != nullptr;
    c->knobs.no_staged_upload = getenv("PARTLS_NO_STAGED_UPLOAD") != nullptr;
    if (const char *e = getenv("PARTLS_REG_MAXT")) { const int v = atoi(e); if (v >= 1 && v <= 20) c->knobs.reg_maxt = v; }
    c->knobs.eager_generic = getenv("PARTLS_EAGER_GENERIC") != nullptr;
    c->knobs.bnb_cold = getenv("PARTLS_BNB_COLD") != nullptr;
    if (const char *e = getenv("PARTLS_BNB_BATCH")) c->knobs.bnb_batch = atoi(e);
    if (const char *e = getenv("PARTLS_BNB_POOL_MB")) c->knobs.bnb_pool_mb = atoi(e);
    if (const char *e = getenv("PARTLS_BNB_WG_PER_CU")) c->knobs.bnb_wg_per_cu = atoi(e);
    if (const char *e = getenv("PARTLS_COOP_FAULT")) c->knobs.coop_fault = atoi(e);
    c->knobs.lz_fault = getenv("PARTLS_LZ_FAULT") != nullptr;
    c->knobs.no_tab_refine = getenv("PARTLS_NO_TAB_REFINE") != nullptr;
    c->knobs.finish_trace = getenv("PARTLS_FINISH_TRACE") != nullptr;
    c->knobs.alt_trace = getenv("PARTLS_ALT_TRACE") != nullptr;
    c->knobs.alt_always_check = getenv("PARTLS_ALT_ALWAYS_CHECK") != nullptr;
    c->knobs.print_stamps = getenv("PARTLS_PRINT_STAMPS") != nullptr;
    c->knobs.cv_serial = getenv("PARTLS_CV_SERIAL") != nullptr && strcmp(getenv("PARTLS_CV_SERIAL"), "0") != 0;
    c->knobs.resample_serial = getenv("PARTLS_RESAMPLE_SERIAL") != nullptr && strcmp(getenv("PARTLS_RESAMPLE_SERIAL"), "0") != 0;
    // a failure below must not leak the context (or the objects already created)
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int w = 0; w < PARTLS_T_COUNT && e == hipSuccess; ++w) {
        e = hipEventCreate(&c->ev0[w]);
        if (e == hipSuccess) e = hipEventCreate(&c->ev1[w]);
    }
    if (e != hipSuccess) {
        set_error("partls_create: stream / event creation failed: %s", hipGetErrorString(e));
        partls_destroy(c);
        return PARTLS_ERR_HIP;
    }
    *out = c;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

void partls_destroy(partls_ctx *c)
{
    if (!c) return;
    partls_destroy(c->cv_work);                           // partls_cv_opt's / partls_opt_weightings' internal contexts (NULL when neither ran)
    for (partls_ctx *v : c->cv_view) partls_destroy(v);
    c->cv_work = nullptr;
    c->cv_view.clear();
    // At process exit the HIP runtime (or a profiler layered on it) may already be torn down when a late destructor gets
    // here: touch the device only while the runtime still answers, otherwise just drop the host object.
    int ndev = 0;
    const bool alive = hipGetDeviceCount(&ndev) == hipSuccess && ndev > c->device && hipSetDevice(c->device) == hipSuccess;
    if (alive && c->stream) (void)hipStreamSynchronize(c->stream);
    // every buffer frees itself (the owning types of ctx.h); the events and the stream go after them
    const hipStream_t stream = c->stream;
    hipEvent_t ev[2 * PARTLS_T_COUNT];
    for (int w = 0; w < PARTLS_T_COUNT; ++w) { ev[2 * w] = c->ev0[w]; ev[2 * w + 1] = c->ev1[w]; }
    g_runtime_gone = !alive;
    delete c;
    g_runtime_gone = false;
    if (alive) {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
}

// predict: w_m = sum_k P[m,k] alpha_m beta_k on the host (predict_weights: M*K flops), yhat = X w + t on the device (one pass over X)
// pass(wdev, dyh): the one step that knows how X is stored — a host X goes up into the context's pred* buffers, then the prediction
// pass is queued on c->stream: dyh = X wdev + t (dense_predict_pass below; csr_predict_pass for a sparse X)
using PredictPass = std::function<partls_status(const double *wdev, double *dyh)>;
static partls_status predict_common(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, int x_on_device,
                                    const int64_t *P, int64_t K, int64_t ldP, const double *alpha, const double *beta,
                                    double *yhat, const PredictPass &pass)
{
    partls_status st = check_common(c, X, N, M, ldX, P, K, ldP);
    if (st != PARTLS_OK) return st;
    if (!alpha || !beta || !yhat) { set_error("partls_predict: NULL argument"); return PARTLS_ERR_BAD_ARG; }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    std::vector<double> w((size_t)M, 0.0);
    st = predict_weights(P, M, K, ldP, alpha, beta, w.data());
    if (st != PARTLS_OK) return st;
    PARTLS_HIP_CHECK(c->wdev.ensure((size_t)(M + 1) * sizeof(double)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->wdev.p, w.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, c->stream));
    auto run = [&]() -> partls_status {
        double *dyh = yhat;
        if (!x_on_device) {
            PARTLS_HIP_CHECK(c->predY.ensure((size_t)N * sizeof(double)));
            dyh = c->predY.as<double>();
        }
        const partls_status ps = pass(c->wdev.as<double>(), dyh);
        if (ps != PARTLS_OK) return ps;
        if (!x_on_device)
            PARTLS_HIP_CHECK(hipMemcpyAsync(yhat, c->predY.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return PARTLS_OK;
    };
    st = run();
    if (!x_on_device) { c->predX.release(); c->predY.release(); c->predPtr.release(); c->predIdx.release(); }    // a prediction set is not retained
    return st;
}

static partls_status predict_dense(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, int x_on_device,
                                   const int64_t *P, int64_t K, int64_t ldP, const double *alpha, const double *beta, double t,
                                   double *yhat, bool x_f32 = false)
{
    return predict_common(c, X, N, M, ldX, x_on_device, P, K, ldP, alpha, beta, yhat, [&](const double *wdev, double *dyh) -> partls_status {
        const void *dX = nullptr; int64_t ld = 0;
        const partls_status us = stage_dense_x(c, X, N, M, ldX, x_on_device, x_f32, &dX, &ld);
        if (us != PARTLS_OK) return us;
        PARTLS_HIP_CHECK(launch_residual(dX, N, M, ld, nullptr, wdev, t, nullptr, 1024, dyh, c->stream, nullptr, x_f32));
        return PARTLS_OK;
    });
}

partls_status partls_predict_csr(partls_ctx *c, const int64_t *indptr, const int32_t *indices, const double *values, int64_t N, int64_t M,
                                 int x_on_device, const int64_t *P, int64_t K, int64_t ldP, const double *alpha, const double *beta,
                                 double t, double *yhat)
try {
    const char *who = "partls_predict_csr";
    return predict_common(c, indptr, N, M, N, x_on_device, P, K, ldP, alpha, beta, yhat, [&](const double *wdev, double *dyh) -> partls_status {
        CsrView A;
        int64_t nnz = 0;
        double bytes = 0.0, ms = 0.0;
        partls_status st = csr_adopt(c, who, indptr, indices, values, N, M, x_on_device, c->predPtr, c->predIdx, c->predX, &A, &nnz, &bytes, &ms);
        if (st != PARTLS_OK) return st;
        DevBuf err;                                          // the validation's three words (a prepared problem's buffers stay untouched)
        PARTLS_HIP_CHECK(err.ensure(3 * sizeof(unsigned long long)));
        st = csr_check(c, who, A, nnz, err.as<unsigned long long>(), nullptr, {});
        if (st != PARTLS_OK) return st;
        PARTLS_HIP_CHECK(launch_csr_residual(A, nullptr, wdev, t, nullptr, 1024, dyh, c->stream));
        return PARTLS_OK;
    });
}
PARTLS_ABI_GUARD

partls_status partls_predict(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, const int64_t *P, int64_t K,
                             int64_t ldP, const double *alpha, const double *beta, double t, double *yhat)
try {
    return predict_dense(c, X, N, M, ldX, 0, P, K, ldP, alpha, beta, t, yhat);
}
PARTLS_ABI_GUARD

partls_status partls_predict_device(partls_ctx *c, const double *dX, int64_t N, int64_t M, int64_t ldX, const int64_t *P,
                                    int64_t K, int64_t ldP, const double *alpha, const double *beta, double t, double *dyhat)
try {
    return predict_dense(c, dX, N, M, ldX, 1, P, K, ldP, alpha, beta, t, dyhat);
}
PARTLS_ABI_GUARD

partls_status partls_predict_f32(partls_ctx *c, const float *X, int64_t N, int64_t M, int64_t ldX, const int64_t *P, int64_t K,
                                 int64_t ldP, const double *alpha, const double *beta, double t, double *yhat)
try {
    return predict_dense(c, X, N, M, ldX, 0, P, K, ldP, alpha, beta, t, yhat, /*x_f32=*/true);
}
PARTLS_ABI_GUARD

partls_status partls_predict_device_f32(partls_ctx *c, const float *dX, int64_t N, int64_t M, int64_t ldX, const int64_t *P,
                                        int64_t K, int64_t ldP, const double *alpha, const double *beta, double t, double *dyhat)
try {
    return predict_dense(c, dX, N, M, ldX, 1, P, K, ldP, alpha, beta, t, dyhat, /*x_f32=*/true);
}
PARTLS_ABI_GUARD

partls_status partls_synth_truth(uint64_t seed, int64_t D, int64_t K, int64_t *P, double *wstar)
try {
    if (D < 1 || K < 1 || K > D) { set_error("partls_synth_truth: bad D/K"); return PARTLS_ERR_BAD_ARG; }
    std::vector<int64_t> grp((size_t)D);
    int64_t j = 0;
    for (int64_t k = 0; k < K; ++k) {
        const int64_t sz = D / K + ((k < D % K) ? 1 : 0);
        for (int64_t q = 0; q < sz; ++q) grp[(size_t)j++] = k;
    }
    if (P) {
        memset(P, 0, (size_t)D * K * sizeof(int64_t));
        for (int64_t m = 0; m < D; ++m) P[m + grp[(size_t)m] * D] = 1;
    }
    auto uni = [&](uint64_t stream, uint64_t idx) { return (double)(rnd64(seed, stream, idx) >> 11) * 0x1.0p-53; };
    if (wstar)
        for (int64_t k = 0; k < K; ++k) {
            double sum = 0.0;
            for (int64_t m = 0; m < D; ++m) if (grp[(size_t)m] == k) sum += uni(2, (uint64_t)m);
            const double bk = (uni(3, (uint64_t)k) - 0.5) * 10.0;
            for (int64_t m = 0; m < D; ++m) if (grp[(size_t)m] == k) wstar[m] = (uni(2, (uint64_t)m) / sum) * bk;
        }
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_synth_device(partls_ctx *c, uint64_t seed, int64_t N, int64_t D, const double *wstar, double *dX, double *dy)
try {
    if (!c || !wstar || !dX || !dy || N < 1 || D < 1) { set_error("partls_synth_device: bad argument"); return PARTLS_ERR_BAD_ARG; }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    PARTLS_HIP_CHECK(c->wdev.ensure((size_t)D * sizeof(double)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->wdev.p, wstar, (size_t)D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PARTLS_HIP_CHECK(launch_synth(seed, N, D, c->wdev.as<double>(), dX, dy, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_timing(const partls_ctx *c, partls_timer which, double *ms)
try {
    if (!c || !ms || (int)which < 0 || (int)which >= PARTLS_T_COUNT) { set_error("partls_get_timing: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *ms = c->ms[(int)which];
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_upload(const partls_ctx *c, double *ms, double *bytes)
try {
    if (!c || !ms || !bytes) { set_error("partls_get_upload: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *ms = c->last_upload_ms; *bytes = c->last_upload_bytes;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_pivots(const partls_ctx *c, int64_t *pivots)
try {
    if (!c || !pivots) { set_error("partls_get_pivots: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *pivots = (int64_t)c->last_pivots;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_kkt_violation(const partls_ctx *c, double *violation, double *min_pivot)
try {
    if (!c || !violation) { set_error("partls_get_kkt_violation: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *violation = c->last_kkt;
    if (min_pivot) *min_pivot = c->last_min_loo;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_rescue_stats(const partls_ctx *c, int64_t *rescued, int64_t *pivots, int64_t *failed)
try {
    if (!c) { set_error("partls_get_rescue_stats: bad argument"); return PARTLS_ERR_BAD_ARG; }
    if (rescued) *rescued = (int64_t)c->rescue_rescued;
    if (pivots) *pivots = (int64_t)c->rescue_pivots;
    if (failed) *failed = (int64_t)c->rescue_failed;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_vetoes(const partls_ctx *c, int64_t *vetoes)
try {
    if (!c || !vetoes) { set_error("partls_get_vetoes: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *vetoes = (int64_t)c->last_vetoes;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_blocks(const partls_ctx *c, int64_t *blocks)
try {
    if (!c || !blocks) { set_error("partls_get_blocks: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *blocks = (int64_t)c->last_blocks;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_sweep_route(const partls_ctx *c, int *kernel, int *tiles)
try {
    if (!c || !kernel || !tiles) { set_error("partls_get_sweep_route: bad argument"); return PARTLS_ERR_BAD_ARG; }
    // partls_cv_opt and partls_opt_weightings prepare their problems on the working context (cv.hip), which carries this context's knobs
    const partls_ctx *p = c->prepared ? c : (c->cv_work && c->cv_work->prepared ? c->cv_work : nullptr);
    if (!p) { set_error("partls_get_sweep_route: context not prepared"); return PARTLS_ERR_STATE; }
    *kernel = p->use_reg ? (sweep_reg_small(p->T) ? PARTLS_ROUTE_REG_256 : PARTLS_ROUTE_REG_512)
                         : (p->knobs.eager_generic ? PARTLS_ROUTE_EAGER : PARTLS_ROUTE_DEFERRED);
    *tiles = p->use_reg ? p->T : 0;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_near_ties(const partls_ctx *c, int64_t *evaluated)
try {
    if (!c || !evaluated) { set_error("partls_get_near_ties: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *evaluated = c->last_near_evaluated;
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

partls_status partls_get_gram(const partls_ctx *c, double *G_aug)
try {
    if (!c || !c->prepared || !G_aug) { set_error("partls_get_gram: context not prepared"); return PARTLS_ERR_STATE; }
    const int na = (int)c->M + 2;
    for (int j = 0; j < na; ++j)
        for (int i = 0; i < na; ++i) G_aug[(size_t)i + (size_t)j * na] = h_reg(c, i, j);
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

}  // extern "C"
