// prepare.hip — from the caller's arrays to a prepared context: upload of X, y and the sample weights, the Gram products, the tableau.
// The steps the batched entries (cv.hip, resample.hip) share with ctx_prepare are defined here once: forget_problem (the reset),
// adopt_or_upload (X and y), prepare_weights, ctx_prepare_tableau; the rules they apply are those of prepare_rules.h.  DESIGN.md §4.
#include "ctx.h"
#include "prepare_rules.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <numeric>
#include <thread>

namespace partls {

partls_status load_partition(partls_ctx *c, const int64_t *P, int64_t M, int64_t K, int64_t ldP)
{
    c->P.assign((size_t)M * K, 0);
    c->mask_aug.assign((size_t)M + 2, 0);
    for (int64_t k = 0; k < K; ++k)
        for (int64_t m = 0; m < M; ++m) {
            const int64_t v = P[m + k * ldP];
            if (v != 0 && v != 1) { set_error("P[%lld,%lld] = %lld is not 0/1", (long long)m, (long long)k, (long long)v); return PARTLS_ERR_BAD_PARTITION; }
            c->P[(size_t)m + (size_t)k * M] = v;
            if (v) c->mask_aug[(size_t)m] |= (1ULL << k);
        }
    c->mask_aug[(size_t)M] = 1ULL << K;            // the intercept's own group (homogeneousCoords, PartitionedLS.jl:78)
    c->mask_aug[(size_t)M + 1] = 0;                // y
    return PARTLS_OK;
}

// Host -> device copy of a column-major matrix (N x M, leading dimension ldX) into a packed device image (leading dimension N).
// Measured on the MI355X box (tools/ubench/h2d_paths.hip, profiles/r04_h2d_paths.txt): the link gives 57 GB/s from page-locked memory;
// hipMemcpy2DAsync from PAGEABLE memory reaches that only when the runtime has pinned the very same pages before — a caller's fresh
// array goes at 8 GB/s (205 MB, C3) to 25 GB/s (4.1 GB, C4), the pinning itself costs as much as the transfer.  Staged through
// page-locked buffers by a few copier threads the same array goes at 42-55 GB/s whatever its history: UP_T threads, each with its own
// stream and two staging buffers, own a contiguous range of columns; a thread packs a batch of columns into one buffer (memcpy) while
// the DMA of its previous batch runs from the other.  Small matrices (< 8 MB) take the plain copy.
namespace {
constexpr int UP_T = 4;
constexpr size_t UP_BUF = (size_t)8 << 20;
}
partls_status upload_matrix(partls_ctx *c, void *dst_, const void *X_, int64_t N, int64_t M, int64_t ldX, size_t esz)
{
    char *dst = static_cast<char *>(dst_);                 // everything below goes by bytes: esz = 8 (double) or 4 (float)
    const char *X = static_cast<const char *>(X_);
    const size_t bytes = (size_t)N * M * esz;
    if (bytes < ((size_t)8 << 20) || c->knobs.no_staged_upload) {
        PARTLS_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)N * esz, X, (size_t)ldX * esz, (size_t)N * esz, (size_t)M,
                                          hipMemcpyHostToDevice, c->stream));
        return PARTLS_OK;
    }
    if (!c->up.pin[0]) {
        for (int i = 0; i < 2 * UP_T; ++i) PARTLS_HIP_CHECK(hipHostMalloc((void **)&c->up.pin[i], UP_BUF, hipHostMallocDefault));
        for (int t = 0; t < UP_T; ++t) PARTLS_HIP_CHECK(hipStreamCreateWithFlags(&c->up.stream[t], hipStreamNonBlocking));
        for (int i = 0; i < 2 * UP_T; ++i) PARTLS_HIP_CHECK(hipEventCreateWithFlags(&c->up.event[i], hipEventDisableTiming));
    }
    // rows per piece of a column (a column longer than a staging buffer goes in pieces), columns per batch otherwise
    const size_t col_bytes = (size_t)N * esz, ld_bytes = (size_t)ldX * esz;
    hipError_t err[UP_T];
    for (int t = 0; t < UP_T; ++t) err[t] = hipSuccess;
    const int device = c->device;
    auto worker = [&](int t) {
        hipError_t e = hipSetDevice(device);
        const int64_t c0 = M * t / UP_T, c1 = M * (t + 1) / UP_T;
        char *pin[2] = {c->up.pin[2 * t], c->up.pin[2 * t + 1]};
        bool used[2] = {false, false};
        int b = 0;
        auto flush = [&](char *d, size_t n) {           // DMA of the buffer just filled; the other buffer is filled meanwhile
            if (e == hipSuccess) e = hipMemcpyAsync(d, pin[b], n, hipMemcpyHostToDevice, c->up.stream[t]);
            if (e == hipSuccess) e = hipEventRecord(c->up.event[2 * t + b], c->up.stream[t]);
            used[b] = true;
            b ^= 1;
            if (used[b] && e == hipSuccess) e = hipEventSynchronize(c->up.event[2 * t + b]);      // the buffer about to be refilled is free again
        };
        if (col_bytes <= UP_BUF) {
            const int64_t per = (int64_t)(UP_BUF / col_bytes);
            for (int64_t j0 = c0; j0 < c1 && e == hipSuccess; j0 += per) {
                const int64_t j1 = j0 + per < c1 ? j0 + per : c1;
                for (int64_t j = j0; j < j1; ++j) std::memcpy(pin[b] + (size_t)(j - j0) * col_bytes, X + (size_t)j * ld_bytes, col_bytes);
                flush(dst + (size_t)j0 * col_bytes, (size_t)(j1 - j0) * col_bytes);
            }
        } else {
            const int64_t rows = (int64_t)(UP_BUF / esz);
            for (int64_t j = c0; j < c1 && e == hipSuccess; ++j)
                for (int64_t r0 = 0; r0 < N && e == hipSuccess; r0 += rows) {
                    const int64_t r1 = r0 + rows < N ? r0 + rows : N;
                    std::memcpy(pin[b], X + (size_t)j * ld_bytes + (size_t)r0 * esz, (size_t)(r1 - r0) * esz);
                    flush(dst + (size_t)j * col_bytes + (size_t)r0 * esz, (size_t)(r1 - r0) * esz);
                }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->up.stream[t]);
        err[t] = e;
    };
    {
        std::vector<std::thread> th;
        th.reserve(UP_T);
        bool spawned = true;
        try { for (int t = 1; t < UP_T; ++t) th.emplace_back(worker, t); }
        catch (...) { spawned = false; }
        worker(0);
        for (std::thread &w : th) w.join();
        if (!spawned) for (int t = (int)th.size() + 1; t < UP_T; ++t) worker(t);      // out of threads: the caller's thread takes the rest
    }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    for (int t = 0; t < UP_T; ++t) if (err[t] != hipSuccess) { set_error("staged upload of X failed: %s", hipGetErrorString(err[t])); return PARTLS_ERR_HIP; }
    return PARTLS_OK;                                    // every copier has synchronised its stream: the image is complete for c->stream
}

partls_status prepare_weights(partls_ctx *c, const double *w, int64_t N, int on_device)
{
    c->dw = nullptr; c->ds = nullptr;
    const double *dw = w;
    if (!on_device) {
        PARTLS_HIP_CHECK(c->ownW.ensure((size_t)N * sizeof(double)));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->ownW.p, w, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
        dw = c->ownW.as<double>();
    }
    const int nb = weight_prep_blocks(N);
    PARTLS_HIP_CHECK(c->ownS.ensure((size_t)N * sizeof(double)));
    PARTLS_HIP_CHECK(c->wPart.ensure((size_t)4 * nb * sizeof(double)));
    PARTLS_HIP_CHECK(c->hPart.resize((size_t)4 * nb));
    PARTLS_HIP_CHECK(launch_weight_prep(dw, N, c->ownS.as<double>(), c->wPart.as<double>(), c->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->hPart.data(), c->wPart.p, (size_t)4 * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    const WeightFold f = fold_weight_partials(c->hPart.data(), nb);
    if (f.nonfinite) { set_error("the sample weights contain NaN/Inf"); return PARTLS_ERR_NONFINITE; }
    if (f.negative) { set_error("a sample weight is negative"); return PARTLS_ERR_BAD_ARG; }
    if (!(f.sum > 0.0)) { set_error("the sample weights sum to 0"); return PARTLS_ERR_BAD_ARG; }
    if (!std::isfinite(f.sum)) { set_error("the sum of the sample weights overflows"); return PARTLS_ERR_NONFINITE; }
    c->dw = dw; c->ds = c->ownS.as<double>();
    return PARTLS_OK;
}

void forget_problem(partls_ctx *c)
{
    c->prepared = false;
    c->peers.clear();                              // a row-sharded fit sets them again after every rank has prepared its block
    c->near_for = -1; c->near_pat.clear(); c->cand.clear(); c->export_wg = -1;
    c->sweep_vetoes = 0;
    c->rescue_rescued = c->rescue_pivots = c->rescue_failed = 0;
    c->coop_state_valid = false; c->coop_fallback = false;
    c->tab_valid = false;
    c->order_ready = false; c->order_identity = true; c->flip_cost.clear();
    c->pair_laid = false;
    c->dw = nullptr; c->ds = nullptr;
    c->x_f32 = false; c->storage = XStorage::dense64;
    c->last_upload_ms = 0.0; c->last_upload_bytes = 0.0;
    c->ms[PARTLS_T_CALIB] = 0.0; c->ms[PARTLS_T_OOB] = 0.0;
    c->rb_have = false;
    c->gl_y0 = nullptr; c->gl_have = false; c->gl_checked = 0;
}

partls_status adopt_or_upload(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device, size_t esz)
{
    if (x_on_device) {
        c->dX = X; c->dy = y; c->ldX = ldX;
        return PARTLS_OK;
    }
    PARTLS_HIP_CHECK(c->ownX.ensure((size_t)N * M * esz));
    PARTLS_HIP_CHECK(c->ownY.ensure((size_t)N * sizeof(double)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->ownY.p, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const auto u0 = std::chrono::steady_clock::now();
    const partls_status st = upload_matrix(c, c->ownX.p, X, N, M, ldX, esz);
    if (st != PARTLS_OK) return st;
    c->last_upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
    c->last_upload_bytes = (double)N * (double)M * (double)esz;
    c->dX = c->ownX.p; c->dy = c->ownY.as<double>(); c->ldX = N;
    return PARTLS_OK;
}

// The two ends of a single problem's prepare, whatever the storage of X (ctx_prepare, ctx_prepare_csr).  prepare_begin: the checks,
// the reset, the weights, the partition and the shape — everything before X is touched (X: any non-NULL pointer of the matrix; no_multi:
// the refusal of a context of a partls_multi, NULL where such a context is fine).  prepare_end: from the Gram products in c->G on.
static partls_status prepare_begin(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device,
                                   const int64_t *P, int64_t K, int64_t ldP, double eta, bool faithful, uint32_t flags, const double *w,
                                   const char *no_multi)
{
    partls_status st = check_common(c, X, N, M, ldX, P, K, ldP);
    if (st != PARTLS_OK) return st;
    if (!y) { set_error("y is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (!(eta >= 0.0)) { set_error("eta must be >= 0"); return PARTLS_ERR_BAD_ARG; }
    forget_problem(c);
    if (no_multi && c->multi_rank) { set_error("%s", no_multi); return PARTLS_ERR_UNSUPPORTED; }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    if (w) {
        if (c->multi_rank) { set_error("sample weights: a context of a partls_multi is not supported (multi-GPU fits are unweighted)"); return PARTLS_ERR_UNSUPPORTED; }
        st = prepare_weights(c, w, N, x_on_device);
        if (st != PARTLS_OK) return st;
    }
    st = load_partition(c, P, M, K, ldP);
    if (st != PARTLS_OK) return st;
    c->N = N; c->M = M; c->K = K; c->eta = eta; c->flags = flags; c->faithful = faithful;
    return PARTLS_OK;
}

static partls_status prepare_end(partls_ctx *c)
{
    // rows of X sharded over several devices: the Gram products of the blocks are summed here (partls_fit_opt_multi, multi.hip)
    if (c->gram_hook) { const partls_status st = c->gram_hook(c); if (st != PARTLS_OK) return st; }
    return ctx_prepare_tableau(c);
}

// The Gram launch of the problem c holds, queued on c->stream (no sync) — one definition per storage kind, shared by the prepare and by
// ctx_rework, so that a re-prepare builds exactly what a fresh prepare builds.  Dense (fp64 MFMA): X, y, ds = sqrt(w) -> c->G, timed
// as PARTLS_T_GRAM (the launch alone, not the allocations in front of it).
static partls_status queue_dense_gram(partls_ctx *c)
{
    const size_t slabd = gram_slab_doubles(c->N, c->M, c->knobs.gram_S, c->knobs.gram_cr, &c->chunks, &c->ldg);
    PARTLS_HIP_CHECK(c->slab.ensure(slabd * sizeof(double)));
    PARTLS_HIP_CHECK(c->G.ensure((size_t)c->ldg * c->ldg * sizeof(double)));
    t_begin(c, PARTLS_T_GRAM);
    PARTLS_HIP_CHECK(launch_gram(c->dX, c->N, c->M, c->ldX, c->dy, c->slab.as<double>(), c->chunks, c->ldg, c->knobs.gram_S, c->knobs.gram_cr,
                                 c->G.as<double>(), c->stream, c->ds, c->x_f32));
    t_end(c, PARTLS_T_GRAM);
    return PARTLS_OK;
}
// CSR: the matrix, its CSC copy, y, dw = w and the plan (csr_seg, csr_S) the prepare made from the column lengths -> c->G (c->ldg set).
// Not timed here: the prepare's PARTLS_T_GRAM spans the validation and the transposition in front of it as well.
static partls_status queue_csr_gram(partls_ctx *c)
{
    const size_t partd = csr_gram_part_doubles(c->M, c->csr_S);
    PARTLS_HIP_CHECK(c->csrPart.ensure((partd + 3) * sizeof(double)));
    PARTLS_HIP_CHECK(launch_csr_gram(c->csr, c->csc, c->dy, c->dw, c->csr_seg, c->csr_S, c->csrPart.as<double>(),
                                     c->csrPart.as<double>() + partd, c->ldg, c->G.as<double>(), c->stream));
    return PARTLS_OK;
}

partls_status ctx_prepare(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, int x_on_device,
                          const int64_t *P, int64_t K, int64_t ldP, double eta, bool faithful, uint32_t flags, const double *w, bool x_f32)
{
    partls_status st = prepare_begin(c, X, N, M, ldX, y, x_on_device, P, K, ldP, eta, faithful, flags, w,
                                     x_f32 ? "float X: a context of a partls_multi is not supported (row-sharded multi-GPU fits are fp64)" : nullptr);
    if (st != PARTLS_OK) return st;
    st = adopt_or_upload(c, X, N, M, ldX, y, x_on_device, x_f32 ? sizeof(float) : sizeof(double));
    if (st != PARTLS_OK) return st;
    c->x_f32 = x_f32; c->storage = x_f32 ? XStorage::dense32 : XStorage::dense64;

    st = queue_dense_gram(c);
    if (st != PARTLS_OK) return st;
    return prepare_end(c);
}

// ---- X stored in CSR
// a host array -> dst on c->stream: as four columns through upload_matrix (its copier threads and page-locked staging), the tail behind
static partls_status upload_array(partls_ctx *c, void *dst, const void *src, size_t bytes)
{
    const size_t col = (bytes / 4) & ~(size_t)7;
    if (col) { const partls_status st = upload_matrix(c, dst, src, (int64_t)col, 4, (int64_t)col, 1); if (st != PARTLS_OK) return st; }
    if (bytes > 4 * col)
        PARTLS_HIP_CHECK(hipMemcpyAsync(static_cast<char *>(dst) + 4 * col, static_cast<const char *>(src) + 4 * col, bytes - 4 * col,
                                        hipMemcpyHostToDevice, c->stream));
    return PARTLS_OK;
}

partls_status csr_adopt(partls_ctx *c, const char *who, const int64_t *indptr, const int32_t *indices, const double *values, int64_t N,
                        int64_t M, int x_on_device, DevBuf &up_ptr, DevBuf &up_idx, DevBuf &up_val, CsrView *A, int64_t *nnz,
                        double *bytes, double *ms)
{
    if (N >= ((int64_t)1 << 31)) { set_error("%s: N = %lld rows: this build supports N < 2^31 for a sparse X", who, (long long)N); return PARTLS_ERR_UNSUPPORTED; }
    int64_t ends[2] = {0, 0};
    if (x_on_device) {
        PARTLS_HIP_CHECK(hipMemcpyAsync(&ends[0], indptr, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(&ends[1], indptr + N, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    } else { ends[0] = indptr[0]; ends[1] = indptr[N]; }
    if (ends[0] != 0) { set_error("%s: indptr[0] = %lld, not 0 (row 0)", who, (long long)ends[0]); return PARTLS_ERR_BAD_ARG; }
    if (ends[1] < 0) { set_error("%s: indptr[N] = %lld is negative (row %lld)", who, (long long)ends[1], (long long)(N - 1)); return PARTLS_ERR_BAD_ARG; }
    *nnz = ends[1];
    if (*nnz > 0 && (!indices || !values)) { set_error("%s: indices or values is NULL", who); return PARTLS_ERR_BAD_ARG; }
    *bytes = 0.0; *ms = 0.0;
    A->N = N; A->M = M;
    if (x_on_device) { A->indptr = indptr; A->indices = indices; A->values = values; return PARTLS_OK; }
    const size_t bp = (size_t)(N + 1) * sizeof(int64_t), bi = (size_t)*nnz * sizeof(int32_t), bv = (size_t)*nnz * sizeof(double);
    PARTLS_HIP_CHECK(up_ptr.ensure(bp));
    PARTLS_HIP_CHECK(up_idx.ensure(bi));
    PARTLS_HIP_CHECK(up_val.ensure(bv));
    const auto u0 = std::chrono::steady_clock::now();
    partls_status st = upload_array(c, up_ptr.p, indptr, bp);
    if (st == PARTLS_OK && bi) st = upload_array(c, up_idx.p, indices, bi);
    if (st == PARTLS_OK && bv) st = upload_array(c, up_val.p, values, bv);
    if (st != PARTLS_OK) return st;
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    *ms = ms_since(u0);
    *bytes = (double)bp + (double)bi + (double)bv;
    A->indptr = up_ptr.as<int64_t>(); A->indices = up_idx.as<int32_t>(); A->values = up_val.as<double>();
    return PARTLS_OK;
}

partls_status csr_check(partls_ctx *c, const char *who, const CsrView &A, int64_t nnz, unsigned long long *err, unsigned *wcnt,
                        const std::function<partls_status()> &queue)
{
    unsigned long long h[3] = {CSR_NO_ROW, CSR_NO_ROW, CSR_NO_ROW};
    PARTLS_HIP_CHECK(launch_csr_check(A, nnz, err, wcnt, c->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(h, err, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    if (queue) { const partls_status st = queue(); if (st != PARTLS_OK) return st; }
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (h[0] != CSR_NO_ROW && h[0] <= h[1]) {
        set_error("%s: indptr decreases, is negative or exceeds indptr[N] at row %llu", who, h[0]);
        return PARTLS_ERR_BAD_ARG;
    }
    if (h[1] != CSR_NO_ROW) {
        set_error("%s: row %llu has a column index outside [0, %lld) or indices that do not strictly increase", who, h[1], (long long)A.M);
        return PARTLS_ERR_BAD_ARG;
    }
    if (h[2] != CSR_NO_ROW) { set_error("%s: values contains NaN/Inf (row %llu)", who, h[2]); return PARTLS_ERR_NONFINITE; }
    return PARTLS_OK;
}

partls_status ctx_prepare_csr(partls_ctx *c, const int64_t *indptr, const int32_t *indices, const double *values, int64_t N, int64_t M,
                              const double *y, const double *w, int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta,
                              bool faithful, uint32_t flags)
{
    const char *who = "partls_opt_prepare_csr";
    partls_status st = prepare_begin(c, indptr, N, M, N, y, x_on_device, P, K, ldP, eta, faithful, flags, w,
                                     "sparse X: a context of a partls_multi is not supported (row-sharded multi-GPU fits are dense)");
    if (st != PARTLS_OK) return st;
    int64_t nnz = 0;
    double up_bytes = 0.0, up_ms = 0.0;
    CsrView A;
    st = csr_adopt(c, who, indptr, indices, values, N, M, x_on_device, c->ownPtr, c->ownIdx, c->ownVal, &A, &nnz, &up_bytes, &up_ms);
    if (st != PARTLS_OK) return st;
    if (x_on_device) c->dy = y;
    else {
        PARTLS_HIP_CHECK(c->ownY.ensure((size_t)N * sizeof(double)));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->ownY.p, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
        c->dy = c->ownY.as<double>();
    }
    c->last_upload_ms = up_ms; c->last_upload_bytes = up_bytes;

    // csrWork: [error words (3) | column totals (M) | per-wave column counts (waves x M, 32-bit)]
    const int W = csr_row_waves(N);
    PARTLS_HIP_CHECK(c->csrWork.ensure((size_t)(3 + M) * 8 + (size_t)W * M * sizeof(unsigned)));
    unsigned long long *err = c->csrWork.as<unsigned long long>(), *cnt = err + 3;
    unsigned *wcnt = reinterpret_cast<unsigned *>(cnt + M);
    PARTLS_HIP_CHECK(c->cscPtr.ensure((size_t)(M + 1) * sizeof(int64_t)));
    PARTLS_HIP_CHECK(c->cscRow.ensure((size_t)nnz * sizeof(int32_t)));
    PARTLS_HIP_CHECK(c->cscVal.ensure((size_t)nnz * sizeof(double)));
    (void)gram_slab_doubles(N, M, c->knobs.gram_S, c->knobs.gram_cr, &c->chunks, &c->ldg);       // the dense image's leading dimension
    PARTLS_HIP_CHECK(c->G.ensure((size_t)c->ldg * c->ldg * sizeof(double)));
    std::vector<int64_t> colptr((size_t)M + 1, 0);
    t_begin(c, PARTLS_T_GRAM);                            // validation, transposition and Gram
    // the column pointers are safe to form from the counts of an invalid matrix too: they ride on the validation's one wait
    st = csr_check(c, who, A, nnz, err, wcnt, [&]() -> partls_status {
        PARTLS_HIP_CHECK(launch_csr_colptr(A, wcnt, cnt, c->cscPtr.as<int64_t>(), c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(colptr.data(), c->cscPtr.p, colptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        return PARTLS_OK;
    });
    if (st != PARTLS_OK) return st;
    c->csr = A;
    c->csc = CscView{c->cscPtr.as<int64_t>(), c->cscRow.as<int32_t>(), c->cscVal.as<double>()};
    c->dX = nullptr; c->ldX = N; c->x_f32 = false; c->storage = XStorage::csr;
    PARTLS_HIP_CHECK(launch_csr_place(A, wcnt, c->csc.colptr, c->cscRow.as<int32_t>(), c->cscVal.as<double>(), c->stream));
    int64_t longest = 0, seg = 0;
    int S = 1;
    for (int64_t m = 0; m < M; ++m) longest = std::max(longest, colptr[(size_t)m + 1] - colptr[(size_t)m]);
    csr_gram_plan(M, longest, &seg, &S);
    c->csr_seg = seg; c->csr_S = S;                       // kept: partls_opt_reweight builds the Gram again by the same plan
    st = queue_csr_gram(c);
    if (st != PARTLS_OK) return st;
    t_end(c, PARTLS_T_GRAM);
    return prepare_end(c);
}

// ---- partls_opt_rework / partls_opt_reweight: new sample weights and, unless z is NULL, a new response for the
// prepared problem, X untouched
partls_status ctx_rework(partls_ctx *c, const double *w, const double *z, int on_device)
{
    const XStorage storage = c->storage;
    const bool x_f32 = c->x_f32, had = c->rb_have, gl_had = c->gl_have;
    const unsigned gl_checked = c->gl_checked;
    const double *y0 = c->gl_y0 ? c->gl_y0 : c->dy;       // the response of the prepare, whatever reworks came since
    const int64_t N = c->N;
    forget_problem(c);
    c->storage = storage; c->x_f32 = x_f32;               // the kind of the X the context keeps holding
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    if (z) {
        if (!on_device) {
            PARTLS_HIP_CHECK(c->ownZ.ensure((size_t)N * sizeof(double)));
            PARTLS_HIP_CHECK(hipMemcpyAsync(c->ownZ.p, z, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
            z = c->ownZ.as<double>();
        }
        c->dy = z;
    }
    partls_status st = prepare_weights(c, w, N, on_device);
    if (st != PARTLS_OK) return st;
    if (storage == XStorage::csr) {
        t_begin(c, PARTLS_T_GRAM);
        st = queue_csr_gram(c);
        if (st == PARTLS_OK) t_end(c, PARTLS_T_GRAM);
    } else st = queue_dense_gram(c);
    if (st != PARTLS_OK) return st;
    st = prepare_end(c);
    if (st == PARTLS_OK) {                                // the records of the robust weights and of the GLM rows survive a re-prepare
        c->rb_have = had;
        c->gl_have = gl_had; c->gl_checked = gl_checked;
        c->gl_y0 = c->dy == y0 ? nullptr : y0;
    }
    return st;
}

// c->perm -> everything that is laid out by it: the group masks in tableau order, the one upload of masks and permutation, the scale, the
// tableau and the register kernels' image of it.  Queues on c->stream only (no sync); ctx_prepare_tableau and pair_relayout
// (sweep_setup.hip) call it.
partls_status ctx_layout_tableau(partls_ctx *c, bool timed)
{
    const int64_t M = c->M;
    const double eta = c->eta;
    const bool faithful = c->faithful;
    const uint32_t flags = c->flags;
    c->mask_tab.resize((size_t)c->n);
    for (int i = 0; i < c->n; ++i) c->mask_tab[(size_t)i] = c->mask_aug[(size_t)c->perm[(size_t)i]];

    // one upload: [group masks of the augmented variables (M + 2) | group masks in tableau order (n) | permutation (n ints)]
    {
        const size_t words = (size_t)M + 2 + (size_t)c->n + ((size_t)c->n + 1) / 2;
        c->pack.assign(words, 0);
        std::memcpy(c->pack.data(), c->mask_aug.data(), ((size_t)M + 2) * sizeof(uint64_t));
        std::memcpy(c->pack.data() + M + 2, c->mask_tab.data(), (size_t)c->n * sizeof(uint64_t));
        std::memcpy(c->pack.data() + M + 2 + c->n, c->perm.data(), (size_t)c->n * sizeof(int));
        PARTLS_HIP_CHECK(c->maskAugD.ensure(words * sizeof(uint64_t)));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->maskAugD.p, c->pack.data(), words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        c->maskTabP = c->maskAugD.as<uint64_t>() + M + 2;
        c->permP = reinterpret_cast<int *>(c->maskAugD.as<uint64_t>() + M + 2 + c->n);
    }
    PARTLS_HIP_CHECK(c->scale.ensure((size_t)c->n * sizeof(double)));
    PARTLS_HIP_CHECK(c->Tfull.ensure((size_t)(c->n + 1) * (c->n + 1) * sizeof(double)));
    if (timed) t_begin(c, PARTLS_T_PREP);
    PARTLS_HIP_CHECK(launch_prep(c->G.as<double>(), c->ldg, (int)M, eta, c->maskAugD.as<uint64_t>(), faithful ? 0 : 1,
                                 c->permP, c->scale.as<double>(), c->Tfull.as<double>(), c->n, c->stream));
    c->use_reg = sweep_reg_supported(c->n) && c->n <= 16 * c->knobs.reg_maxt && !(flags & PARTLS_OPT_GENERIC_KERNEL);
    if (c->use_reg) {
        c->T = sweep_reg_tiles(c->n);
        PARTLS_HIP_CHECK(c->T0reg.ensure(sweep_reg_t0_doubles(c->T) * sizeof(double)));
        PARTLS_HIP_CHECK(launch_layout_reg(c->Tfull.as<double>(), c->n, c->T, c->T0reg.as<double>(), c->stream));
    }
    if (timed) t_end(c, PARTLS_T_PREP);
    return PARTLS_OK;
}

partls_status ctx_prepare_tableau(partls_ctx *c)
{
    const int64_t M = c->M, K = c->K;
    const bool faithful = c->faithful;
    // tableau variables, grouped by partition (stable sort on the lowest group a variable belongs to) so that the
    // variables one Gray-code flip touches sit in as few 16-wide tile columns as possible
    c->n = faithful ? (int)M + 1 : (int)M;
    c->kbits = faithful ? (int)K + 1 : (int)K;
    c->perm.resize((size_t)c->n);
    std::iota(c->perm.begin(), c->perm.end(), 0);
    auto key = [&](int v) { const uint64_t m = c->mask_aug[(size_t)v]; return m ? __builtin_ctzll(m) : 64; };
    std::stable_sort(c->perm.begin(), c->perm.end(), [&](int a, int b) { return key(a) < key(b); });
    c->pair_laid = false;
    partls_status st = ctx_layout_tableau(c, /*timed=*/true);
    if (st != PARTLS_OK) return st;
    PARTLS_HIP_CHECK(c->hG.resize((size_t)c->ldg * c->ldg));
    PARTLS_HIP_CHECK(c->hScale.resize((size_t)c->n));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->hG.data(), c->G.p, c->hG.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->hScale.data(), c->scale.p, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    t_collect(c);
    if (!gram_diag_finite(c->hG.data(), c->ldg, M)) { set_error("X or y contains NaN/Inf (or overflows in X'X)"); return PARTLS_ERR_NONFINITE; }
    c->tol = problem_tol(c->knobs.tol_rel, c->hG[(size_t)(M + 1) * c->ldg + (M + 1)]);
    c->prepared = true;
    return PARTLS_OK;
}

}  // namespace partls
