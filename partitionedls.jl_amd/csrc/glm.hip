// glm.hip — the device side of a generalised linear fit by iteratively reweighted least squares (partls_glm_working, partls_opt_rework,
// partls_glm_mean).  One call turns a model (or no model: the start) into the working rows of a family on the
// prepared problem:
//   1. eta by the residual pass of the problem's storage kind (launch_residual / launch_csr_residual, the pass of partls_predict);
//   2. the row kernel: per row the clamp, the inverse link, W, z, mu and the deviance term, by the operation lists of partls_glm.h
//      (this file is compiled without contraction); per block of GL_ROWS rows the three partials (sum d, max |eta|, clamped rows)
//      by the fixed tree.
// The host adds the block partials in ascending order.  The first call of a family after a prepare checks the response's domain first
// (one kernel, the first offending row by an integer atomicMin).  Kernels first, then the host drivers and the entries.
#include "ctx.h"
#include <cmath>

namespace partls {

static constexpr int GL_THREADS = 256;
static constexpr int GL_ROWS = 1024;                       // rows of a workgroup of the row kernel: two 16-byte accesses per thread and array
static constexpr double GL_CLAMP = 30.0;
static constexpr unsigned long long GL_NO_ROW = ~0ULL;

__device__ __forceinline__ double glm_xlogy(double a) { return a == 0.0 ? 0.0 : a * log(a); }
__device__ __forceinline__ double glm_clamp(double eta) { return fmin(fmax(eta, -GL_CLAMP), GL_CLAMP); }

struct GlmRow { double W, z, mu, d; };
// the working row of (eta clamped, y): the one definition of the inverse link (partls_glm_mean reads .mu of it)
template <int FAMILY> __device__ __forceinline__ GlmRow glm_row(double ec, double y)
{
    GlmRow r;
    if constexpr (FAMILY == PARTLS_GLM_BINOMIAL) {
        const double ae = fabs(ec);
        const bool pos = ec >= 0.0;
        const double e = exp(-ae), q = 1.0 / (1.0 + e), p = e * q;
        r.mu = pos ? q : p;
        r.W = p * q;
        r.z = ec + (y - r.mu) / r.W;
        const double l = log1p(e), far = ae + l;
        const double nlmu = pos ? l : far, nlnu = pos ? far : l;
        const double omy = 1.0 - y;
        r.d = 2.0 * ((glm_xlogy(y) + glm_xlogy(omy)) + (y * nlmu + omy * nlnu));
    } else {
        r.mu = exp(ec);
        r.W = r.mu;
        r.z = ec + (y - r.mu) / r.mu;
        r.d = 2.0 * ((glm_xlogy(y) - y * ec) - (y - r.mu));
    }
    return r;
}

// the start: eta from y alone, as R's glm.fit forms it
template <int FAMILY> __device__ __forceinline__ double glm_start_eta(double y)
{
    if constexpr (FAMILY == PARTLS_GLM_BINOMIAL) {
        const double m0 = (y + 0.5) / 2.0;
        return log(m0 / (1.0 - m0));
    } else {
        return log(y + 0.1);
    }
}

// err[0] = the first row whose y is NaN / Inf or outside the family's domain (GL_NO_ROW: none); integer min: no order dependence
template <int FAMILY>
__global__ __launch_bounds__(GL_THREADS) void glm_check_kernel(const double *__restrict__ y, int64_t N, unsigned long long *err)
{
    for (int64_t i = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * GL_THREADS) {
        const double v = y[i];
        bool ok = v >= 0.0 && v <= (FAMILY == PARTLS_GLM_BINOMIAL ? 1.0 : 1.7976931348623157e308);      // false for a NaN
        if (!ok) atomicMin(err, (unsigned long long)i);
    }
}

struct GlmAcc { double dev, emax, nclamp; };
template <int FAMILY, bool START>
__device__ __forceinline__ GlmRow glm_one(double eta_in, double y, GlmAcc &acc)
{
    const double eta = START ? glm_start_eta<FAMILY>(y) : eta_in;
    const double ec = glm_clamp(eta);
    const GlmRow r = glm_row<FAMILY>(ec, y);
    acc.dev += r.d;
    acc.emax = fmax(acc.emax, fabs(eta));
    acc.nclamp += eta != ec ? 1.0 : 0.0;
    return r;
}

// block b: rows [GL_ROWS b, GL_ROWS (b + 1)); thread t takes the row pairs 2 t and 512 + 2 t of the block and adds its up to four
// deviance terms in ascending row order; part[3 b ..] = (sum d, max |eta| before the clamp, clamped rows).  eta, W, z, mu are the
// context's own allocations (16-byte accesses); y is read so when y_vec says the caller's array is 16-byte aligned too.
template <int FAMILY, bool START>
__global__ __launch_bounds__(GL_THREADS) void glm_row_kernel(const double *__restrict__ eta, const double *__restrict__ y, int64_t N, int y_vec,
                                                              double *__restrict__ W, double *__restrict__ z, double *__restrict__ mu,
                                                              double *__restrict__ part)
{
    __shared__ double red[3][GL_THREADS];
    GlmAcc acc = {0.0, 0.0, 0.0};
    const int64_t b0 = (int64_t)blockIdx.x * GL_ROWS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t i = b0 + j * (GL_ROWS / 2) + 2 * (int64_t)threadIdx.x;
        if (i + 1 < N) {
            double2 ev = make_double2(0.0, 0.0), yv;
            if (!START) ev = *reinterpret_cast<const double2 *>(eta + i);
            if (y_vec) yv = *reinterpret_cast<const double2 *>(y + i);
            else yv = make_double2(y[i], y[i + 1]);
            const GlmRow r0 = glm_one<FAMILY, START>(ev.x, yv.x, acc);
            const GlmRow r1 = glm_one<FAMILY, START>(ev.y, yv.y, acc);
            *reinterpret_cast<double2 *>(W + i) = make_double2(r0.W, r1.W);
            *reinterpret_cast<double2 *>(z + i) = make_double2(r0.z, r1.z);
            if (mu) *reinterpret_cast<double2 *>(mu + i) = make_double2(r0.mu, r1.mu);
        } else if (i < N) {                                       // the last row of an odd N
            const GlmRow r0 = glm_one<FAMILY, START>(START ? 0.0 : eta[i], y[i], acc);
            W[i] = r0.W; z[i] = r0.z;
            if (mu) mu[i] = r0.mu;
        }
    }
    double v[3] = {acc.dev, acc.emax, acc.nclamp};
    block_tree_256<3, 0x2u>(red, v);                              // sum, max, sum
    if (threadIdx.x == 0) {
        double *p = part + (int64_t)blockIdx.x * 3;
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
    }
}

// mu[i] = the inverse link of eta[i], clamp included: .mu of the row kernel's own device function (y takes no part in it)
template <int FAMILY>
__global__ __launch_bounds__(GL_THREADS) void glm_mean_kernel(const double *__restrict__ eta, int64_t N, double *__restrict__ mu)
{
    const int64_t i = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x;
    if (i < N) mu[i] = glm_row<FAMILY>(glm_clamp(eta[i]), 0.0).mu;
}

template <int FAMILY>
static void launch_glm_rows(bool start, unsigned blocks, hipStream_t s, const double *eta, const double *y, int64_t N, int y_vec, double *W,
                            double *z, double *mu, double *part)
{
    if (start) hipLaunchKernelGGL((glm_row_kernel<FAMILY, true>), dim3(blocks), dim3(GL_THREADS), 0, s, eta, y, N, y_vec, W, z, mu, part);
    else hipLaunchKernelGGL((glm_row_kernel<FAMILY, false>), dim3(blocks), dim3(GL_THREADS), 0, s, eta, y, N, y_vec, W, z, mu, part);
}

static bool glm_family_ok(int family) { return family == PARTLS_GLM_BINOMIAL || family == PARTLS_GLM_POISSON; }

static partls_status glm_working_common(partls_ctx *c, const double *alpha, const double *beta, double t, int family, double *deviance,
                                        double *max_abs_eta, int64_t *n_clamped, double *w_out, double *z_out, double *mu_out)
{
    const char *who = "partls_glm_working";
    partls_status st = check_prepared_single(c, who, PARTLS_ERR_BAD_ARG);
    if (st != PARTLS_OK) return st;
    if ((alpha == nullptr) != (beta == nullptr)) { set_error("%s: alpha and beta are both NULL (the start) or both given", who); return PARTLS_ERR_BAD_ARG; }
    if (!glm_family_ok(family)) { set_error("%s: unknown family %d", who, family); return PARTLS_ERR_BAD_ARG; }
    const bool start = alpha == nullptr;
    const int64_t N = c->N, M = c->M, K = c->K;
    std::vector<double> wp((size_t)M, 0.0);
    if (!start) {
        st = check_models(who, alpha, M, beta, K, &t, M, K, 1, /*many=*/false);
        if (st != PARTLS_OK) return st;
        st = predict_weights(c->P.data(), M, K, M, alpha, beta, wp.data());
        if (st != PARTLS_OK) return st;
    }

    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    const bool host_rows = c->storage == XStorage::csr ? c->csr.indptr == c->ownPtr.p : c->dX == c->ownX.p;   // the prepare uploaded host arrays
    const double *y = c->gl_y0 ? c->gl_y0 : c->dy;                // the response of the prepare, not a z a rework installed
    const int64_t blocks = (N + GL_ROWS - 1) / GL_ROWS;
    // glPart: [error word (16 bytes) | prediction weights (M, rounded up to even) | partials (3 per block)]
    const size_t wp_off = 2, part_off = wp_off + (((size_t)M + 1) & ~(size_t)1);
    PARTLS_HIP_CHECK(c->glPart.ensure((part_off + (size_t)3 * blocks) * sizeof(double)));
    PARTLS_HIP_CHECK(c->glHost.resize((size_t)3 * blocks + 1));
    double *base = c->glPart.as<double>(), *dWp = base + wp_off, *dPart = base + part_off;
    hipStream_t s = c->stream;

    if (!(c->gl_checked & (1u << family))) {                      // before anything is written
        unsigned long long *derr = c->glPart.as<unsigned long long>(), herr = GL_NO_ROW;
        PARTLS_HIP_CHECK(hipMemcpyAsync(derr, &herr, sizeof(herr), hipMemcpyHostToDevice, s));
        const int64_t cb = (N + GL_THREADS - 1) / GL_THREADS;
        const unsigned grid = (unsigned)(cb < 1024 ? cb : 1024);
        if (family == PARTLS_GLM_BINOMIAL) hipLaunchKernelGGL(glm_check_kernel<PARTLS_GLM_BINOMIAL>, dim3(grid), dim3(GL_THREADS), 0, s, y, N, derr);
        else hipLaunchKernelGGL(glm_check_kernel<PARTLS_GLM_POISSON>, dim3(grid), dim3(GL_THREADS), 0, s, y, N, derr);
        PARTLS_HIP_CHECK(hipGetLastError());
        PARTLS_HIP_CHECK(hipMemcpyAsync(&herr, derr, sizeof(herr), hipMemcpyDeviceToHost, s));
        PARTLS_HIP_CHECK(hipStreamSynchronize(s));
        if (herr != GL_NO_ROW) {
            set_error("%s: the response is NaN / Inf or outside the domain of the %s family (%s) at row %llu", who,
                      family == PARTLS_GLM_BINOMIAL ? "binomial" : "Poisson", family == PARTLS_GLM_BINOMIAL ? "0 <= y <= 1" : "y >= 0", herr);
            return PARTLS_ERR_BAD_ARG;
        }
        c->gl_checked |= 1u << family;
    }

    PARTLS_HIP_CHECK(c->glEta.ensure((size_t)N * sizeof(double)));
    PARTLS_HIP_CHECK(c->glW.ensure((size_t)N * sizeof(double)));
    PARTLS_HIP_CHECK(c->glZ.ensure((size_t)N * sizeof(double)));
    PARTLS_HIP_CHECK(c->glMu.ensure((size_t)N * sizeof(double)));
    Events<3> ev;
    PARTLS_HIP_CHECK(ev.create());
    double *dEta = c->glEta.as<double>(), *dW = c->glW.as<double>(), *dZ = c->glZ.as<double>(), *dMu = c->glMu.as<double>();
    if (!start) PARTLS_HIP_CHECK(hipMemcpyAsync(dWp, wp.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, s));
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[0], s));
    if (!start) {
        if (c->storage == XStorage::csr) PARTLS_HIP_CHECK(launch_csr_residual(c->csr, nullptr, dWp, t, nullptr, 1024, dEta, s));
        else PARTLS_HIP_CHECK(launch_residual(c->dX, N, M, c->ldX, nullptr, dWp, t, nullptr, 1024, dEta, s, nullptr, c->x_f32));
    }
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[1], s));
    const int y_vec = (reinterpret_cast<uintptr_t>(y) & 15u) == 0 ? 1 : 0;
    if (family == PARTLS_GLM_BINOMIAL) launch_glm_rows<PARTLS_GLM_BINOMIAL>(start, (unsigned)blocks, s, dEta, y, N, y_vec, dW, dZ, dMu, dPart);
    else launch_glm_rows<PARTLS_GLM_POISSON>(start, (unsigned)blocks, s, dEta, y, N, y_vec, dW, dZ, dMu, dPart);
    PARTLS_HIP_CHECK(hipGetLastError());
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[2], s));
    double *hp = c->glHost.data();
    PARTLS_HIP_CHECK(hipMemcpyAsync(hp, dPart, (size_t)3 * blocks * sizeof(double), hipMemcpyDeviceToHost, s));
    const hipMemcpyKind kind = host_rows ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (w_out) PARTLS_HIP_CHECK(hipMemcpyAsync(w_out, dW, (size_t)N * sizeof(double), kind, s));
    if (z_out) PARTLS_HIP_CHECK(hipMemcpyAsync(z_out, dZ, (size_t)N * sizeof(double), kind, s));
    if (mu_out) PARTLS_HIP_CHECK(hipMemcpyAsync(mu_out, dMu, (size_t)N * sizeof(double), kind, s));
    PARTLS_HIP_CHECK(hipStreamSynchronize(s));
    for (int ph = 0; ph < 2; ++ph) {
        float f = 0.f;
        c->gl_ms[ph] = hipEventElapsedTime(&f, ev.e[ph], ev.e[ph + 1]) == hipSuccess ? (double)f : 0.0;
    }
    double dev = 0.0, em = 0.0, nc = 0.0;
    for (int64_t b = 0; b < blocks; ++b) {
        const double *p = hp + 3 * b;
        dev += p[0];
        em = p[1] > em ? p[1] : em;
        nc += p[2];
    }
    c->gl_have = true;
    if (deviance) *deviance = dev;
    if (max_abs_eta) *max_abs_eta = em;
    if (n_clamped) *n_clamped = (int64_t)nc;
    return PARTLS_OK;
}

static partls_status rework_common(partls_ctx *c, const double *w, const double *z, int on_device)
{
    const char *who = "partls_opt_rework";
    const partls_status st = check_prepared_single(c, who, PARTLS_ERR_STATE);
    if (st != PARTLS_OK) return st;
    if (!w && !z) {
        if (!c->gl_have) { set_error("%s: w and z are NULL and no partls_glm_working call has left rows since the last prepare", who); return PARTLS_ERR_STATE; }
        // the prepared problem gets copies of its own: the next partls_glm_working call overwrites glW and glZ
        const size_t bytes = (size_t)c->N * sizeof(double);
        PARTLS_HIP_CHECK(hipSetDevice(c->device));
        PARTLS_HIP_CHECK(c->ownW.ensure(bytes));
        PARTLS_HIP_CHECK(c->ownZ.ensure(bytes));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->ownW.p, c->glW.p, bytes, hipMemcpyDeviceToDevice, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->ownZ.p, c->glZ.p, bytes, hipMemcpyDeviceToDevice, c->stream));
        return ctx_rework(c, c->ownW.as<double>(), c->ownZ.as<double>(), 1);
    }
    if (!w) { set_error("%s: z is given without w", who); return PARTLS_ERR_BAD_ARG; }
    return ctx_rework(c, w, z, on_device ? 1 : 0);               // z == NULL: partls_opt_reweight
}

static partls_status glm_mean_common(partls_ctx *c, int family, const double *eta, int64_t N, int on_device, double *mu)
{
    const char *who = "partls_glm_mean";
    if (!c || !eta || !mu || N < 1) { set_error("%s: bad argument", who); return PARTLS_ERR_BAD_ARG; }
    if (!glm_family_ok(family)) { set_error("%s: unknown family %d", who, family); return PARTLS_ERR_BAD_ARG; }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const double *din = eta;
    double *dout = mu;
    if (!on_device) {
        PARTLS_HIP_CHECK(c->glMean.ensure((size_t)2 * N * sizeof(double)));
        double *b = c->glMean.as<double>();
        PARTLS_HIP_CHECK(hipMemcpyAsync(b, eta, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s));
        din = b; dout = b + N;
    }
    const unsigned blocks = (unsigned)((N + GL_THREADS - 1) / GL_THREADS);
    if (family == PARTLS_GLM_BINOMIAL) hipLaunchKernelGGL(glm_mean_kernel<PARTLS_GLM_BINOMIAL>, dim3(blocks), dim3(GL_THREADS), 0, s, din, N, dout);
    else hipLaunchKernelGGL(glm_mean_kernel<PARTLS_GLM_POISSON>, dim3(blocks), dim3(GL_THREADS), 0, s, din, N, dout);
    PARTLS_HIP_CHECK(hipGetLastError());
    if (!on_device) PARTLS_HIP_CHECK(hipMemcpyAsync(mu, dout, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
    PARTLS_HIP_CHECK(hipStreamSynchronize(s));
    return PARTLS_OK;
}

}  // namespace partls

using namespace partls;

extern "C" {

partls_status partls_glm_working(partls_ctx *c, const double *alpha, const double *beta, double t, int family, double *deviance,
                                 double *max_abs_eta, int64_t *n_clamped, double *w_out, double *z_out, double *mu_out)
try {
    return glm_working_common(c, alpha, beta, t, family, deviance, max_abs_eta, n_clamped, w_out, z_out, mu_out);
}
PARTLS_ABI_GUARD

partls_status partls_opt_rework(partls_ctx *c, const double *w, const double *z, int on_device)
try {
    return rework_common(c, w, z, on_device);
}
PARTLS_ABI_GUARD

partls_status partls_glm_mean(partls_ctx *c, int family, const double *eta, int64_t N, int on_device, double *mu)
try {
    return glm_mean_common(c, family, eta, N, on_device, mu);
}
PARTLS_ABI_GUARD

partls_status partls_get_glm_timing(const partls_ctx *c, double *residual_ms, double *rows_ms)
try {
    if (!c || !residual_ms || !rows_ms) { set_error("partls_get_glm_timing: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *residual_ms = c->gl_ms[0]; *rows_ms = c->gl_ms[1];
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

}
