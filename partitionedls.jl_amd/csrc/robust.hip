// robust.hip — the device side of a robust fit by iteratively reweighted least squares (partls_robust_weights, partls_opt_reweight;
// DESIGN.md §4.18).  One call turns a model into the row weights of a Huber or bisquare loss on the prepared problem:
//   1. yhat by the residual pass of the problem's storage kind (launch_residual / launch_csr_residual, the pass of partls_predict), then
//      a_i = |yhat_i - y_i| in place;
//   2. unless the scale is given: the order statistics a_(lo), a_(hi) of the median by a radix select, 8 bits a pass, most significant
//      digit first, from the pieces of radix_select.h, which topk.hip shares.  The bit pattern of a non-negative double orders as an
//      unsigned integer, so the key is the value itself.  A pass is a histogram kernel and a one-workgroup scan that fixes the next
//      digit of each threshold and the rank still to find below it.  Both statistics ride the same eight passes (two histograms
//      while their prefixes agree, which is almost always all of them); after the last pass each threshold IS its statistic.
//      Integer counts do not depend on arrival order; nothing returns to the host between the passes;
//   3. the weight kernel: w from (a, c, s), rho, |w - w_prev|, the two counts; per block of RB_ROWS rows the four partials by a fixed
//      tree; w_prev is read from and w written to the same buffer, every row by its own thread.
// The host adds the block partials in ascending order.  Kernels first, then the host driver and the entries.
#include "ctx.h"
#include "radix_select.h"
#include <cmath>

namespace partls {

static constexpr int RB_THREADS = 256;
static constexpr int RB_ROWS = 1024;                       // rows of a workgroup of the weight kernel: two 16-byte accesses per thread
static constexpr size_t RB_STATE_BYTES = 4096;             // RobustState's slot in rbState; the prediction weights follow it

struct RobustState {
    uint64_t thr[2];             // keys of a_(lo), a_(hi): the digits fixed so far, zeros below them
    uint64_t k_rem[2];           // 1-based rank still to find among the entries that match the fixed digits
    double scale;                // written by the weight kernel's block 0: the s it used
    unsigned hist[2][256];
};
static_assert(sizeof(RobustState) <= RB_STATE_BYTES, "RobustState outgrew its slot");

// a_i = |yhat_i - y_i|, in place over yhat (64-bit row indices; fabs folds -0 to +0, so every key is a non-negative pattern)
__global__ __launch_bounds__(RB_THREADS) void robust_abs_kernel(double *__restrict__ a, const double *__restrict__ y, int64_t N)
{
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    if (i < N) a[i] = fabs(a[i] - y[i]);
}

__global__ void robust_init_kernel(RobustState *st, int64_t N)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < 512; i += blockDim.x) st->hist[i >> 8][i & 255] = 0;
    if (tid == 0) {
        st->thr[0] = 0; st->thr[1] = 0;
        st->k_rem[0] = (uint64_t)((N - 1) / 2) + 1; st->k_rem[1] = (uint64_t)(N / 2) + 1;
        st->scale = 0.0;
    }
}

// pass p: digit 7 - p of the keys that agree with a threshold above that digit; nsel: thresholds to find (1 when lo == hi)
__global__ __launch_bounds__(RB_THREADS) void robust_hist_kernel(const double *__restrict__ a, int64_t N, RobustState *st, int pass, int nsel)
{
    __shared__ unsigned h[2][256];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 512; i += RB_THREADS) h[i >> 8][i & 255] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    // the bits above the digit (0 in the first pass, where every key takes part): two shifts, as a shift by 64 is undefined
    const uint64_t top0 = (st->thr[0] >> shift) >> 8, top1 = (st->thr[1] >> shift) >> 8;
    for (int64_t base = (int64_t)blockIdx.x * RB_THREADS; base < N; base += (int64_t)gridDim.x * RB_THREADS) {   // block-uniform trip count
        const int64_t i = base + tid;
        uint64_t key = 0;
        const bool in = i < N;
        if (in) key = (uint64_t)__double_as_longlong(a[i]);
        const uint64_t top = (key >> shift) >> 8;
        const int d = (int)((key >> shift) & 255ULL);
        for (int j = 0; j < nsel; ++j) radix_wave_add(h[j], in && top == (j ? top1 : top0), d, lane);
    }
    __syncthreads();
    radix_flush(&h[0][0], &st->hist[0][0], 256 * nsel, tid, RB_THREADS);      // the histograms lie one behind the other on both sides
}

__global__ __launch_bounds__(RB_THREADS) void robust_scan_kernel(RobustState *st, int pass, int nsel)
{
    __shared__ unsigned h[2][256];
    const int tid = threadIdx.x;
    radix_take(&h[0][0], &st->hist[0][0], 512, tid, RB_THREADS);
    __syncthreads();
    if (tid >= nsel) return;
    uint64_t cum = 0;
    const uint64_t krem = st->k_rem[tid];
    const int d = radix_digit(h[tid], krem, &cum);
    st->thr[tid] |= (uint64_t)d << (56 - 8 * pass);
    st->k_rem[tid] = krem - cum;
}

// the scale every workgroup of the weight kernel forms for itself (the same three operations on the same two values)
__device__ __forceinline__ double robust_scale(const RobustState *st, double scale_in, int nsel)
{
    if (scale_in > 0.0) return scale_in;
    const double alo = __longlong_as_double((long long)st->thr[0]);
    const double ahi = nsel > 1 ? __longlong_as_double((long long)st->thr[1]) : alo;
    return (0.5 * alo + 0.5 * ahi) / 0.6745;
}

struct RobustRow { double w, rho; };
template <int LOSS> __device__ __forceinline__ RobustRow robust_row(double a, double c, double s, double k)
{
    RobustRow r;
    if constexpr (LOSS == PARTLS_ROBUST_HUBER) {
        const double u = a / s;
        const bool in = a <= k;
        r.w = in ? 1.0 : k / a;
        r.rho = in ? (0.5 * u) * u : c * u - (0.5 * c) * c;
    } else {
        const double u = a / k, v = 1.0 - u * u, top = (c * c) / 6.0;
        const bool out = u >= 1.0;
        r.w = out ? 0.0 : v * v;
        r.rho = out ? top : top * (1.0 - (v * v) * v);
    }
    return r;
}

// block b: rows [RB_ROWS b, RB_ROWS (b + 1)); thread t takes the row pairs 2 t and 512 + 2 t of the block (16-byte accesses: both buffers
// are the context's own allocations) and adds its up to four rho in ascending row order; part[4 b ..] = (sum rho, max |w - w_prev|,
// rows with w < 1, rows with w == 0).  have_prev == 0: w_prev is all ones and w is not read.  s == 0: nothing is written but the scale.
template <int LOSS>
__global__ __launch_bounds__(RB_THREADS) void robust_weight_kernel(const double *__restrict__ a, double *w, int64_t N, RobustState *st,
                                                                    double c, double scale_in, int nsel, int have_prev,
                                                                    double *__restrict__ part)
{
    __shared__ double red[4][RB_THREADS];
    const double s = robust_scale(st, scale_in, nsel);
    if (blockIdx.x == 0 && threadIdx.x == 0) st->scale = s;
    if (s == 0.0) return;                                         // grid-uniform
    const double k = c * s;
    double rho = 0.0, dmax = 0.0, down = 0.0, zero = 0.0;
    const int64_t b0 = (int64_t)blockIdx.x * RB_ROWS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t i = b0 + j * (RB_ROWS / 2) + 2 * (int64_t)threadIdx.x;
        if (i + 1 < N) {
            const double2 av = *reinterpret_cast<const double2 *>(a + i);
            double2 wp = make_double2(1.0, 1.0);
            if (have_prev) wp = *reinterpret_cast<const double2 *>(w + i);
            const RobustRow r0 = robust_row<LOSS>(av.x, c, s, k), r1 = robust_row<LOSS>(av.y, c, s, k);
            *reinterpret_cast<double2 *>(w + i) = make_double2(r0.w, r1.w);
            rho += r0.rho; rho += r1.rho;
            dmax = fmax(dmax, fmax(fabs(r0.w - wp.x), fabs(r1.w - wp.y)));
            down += (r0.w < 1.0 ? 1.0 : 0.0) + (r1.w < 1.0 ? 1.0 : 0.0);
            zero += (r0.w == 0.0 ? 1.0 : 0.0) + (r1.w == 0.0 ? 1.0 : 0.0);
        } else if (i < N) {                                       // the last row of an odd N
            const double wp = have_prev ? w[i] : 1.0;
            const RobustRow r0 = robust_row<LOSS>(a[i], c, s, k);
            w[i] = r0.w;
            rho += r0.rho;
            dmax = fmax(dmax, fabs(r0.w - wp));
            down += r0.w < 1.0 ? 1.0 : 0.0;
            zero += r0.w == 0.0 ? 1.0 : 0.0;
        }
    }
    double v[4] = {rho, dmax, down, zero};
    block_tree_256<4, 0x2u>(red, v);                              // sum, max, sum, sum
    if (threadIdx.x == 0) {
        double *p = part + (int64_t)blockIdx.x * 4;
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}

static partls_status robust_weights_common(partls_ctx *c, const double *alpha, const double *beta, double t, int loss, double cc,
                                           double scale_in, double *scale, double *rho_sum, double *max_dw, int64_t *n_down,
                                           int64_t *n_zero, double *w_out)
{
    const char *who = "partls_robust_weights";
    partls_status st = check_prepared_single(c, who, PARTLS_ERR_BAD_ARG);
    if (st != PARTLS_OK) return st;
    if (!alpha || !beta) { set_error("%s: alpha or beta is NULL", who); return PARTLS_ERR_BAD_ARG; }
    if (loss != PARTLS_ROBUST_HUBER && loss != PARTLS_ROBUST_BISQUARE) { set_error("%s: unknown loss %d", who, loss); return PARTLS_ERR_BAD_ARG; }
    if (!std::isfinite(cc) || !(cc > 0.0)) { set_error("%s: the tuning constant c must be finite and > 0", who); return PARTLS_ERR_BAD_ARG; }
    if (!std::isfinite(scale_in)) { set_error("%s: scale_in is NaN / Inf", who); return PARTLS_ERR_BAD_ARG; }
    const int64_t N = c->N, M = c->M, K = c->K;
    st = check_models(who, alpha, M, beta, K, &t, M, K, 1, /*many=*/false);
    if (st != PARTLS_OK) return st;
    std::vector<double> wp((size_t)M, 0.0);
    st = predict_weights(c->P.data(), M, K, M, alpha, beta, wp.data());
    if (st != PARTLS_OK) return st;

    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    const bool host_rows = c->storage == XStorage::csr ? c->csr.indptr == c->ownPtr.p : c->dX == c->ownX.p;   // the prepare uploaded host arrays
    const int64_t blocks = (N + RB_ROWS - 1) / RB_ROWS, rblocks = (N + RB_THREADS - 1) / RB_THREADS;
    const int hgrid = (int)(rblocks < 1024 ? rblocks : 1024);
    const int nsel = (N - 1) / 2 == N / 2 ? 1 : 2;
    const bool select = !(scale_in > 0.0);
    PARTLS_HIP_CHECK(c->rbA.ensure((size_t)N * sizeof(double)));
    PARTLS_HIP_CHECK(c->rbW.ensure((size_t)N * sizeof(double)));
    PARTLS_HIP_CHECK(c->rbState.ensure(RB_STATE_BYTES + (size_t)M * sizeof(double)));
    PARTLS_HIP_CHECK(c->rbPart.ensure((size_t)4 * blocks * sizeof(double)));
    PARTLS_HIP_CHECK(c->rbHost.resize((size_t)4 * blocks + 1));
    Events<4> ev;                                                 // between the phases of the call
    PARTLS_HIP_CHECK(ev.create());
    RobustState *dst = c->rbState.as<RobustState>();
    double *dWp = reinterpret_cast<double *>(c->rbState.as<char>() + RB_STATE_BYTES), *dA = c->rbA.as<double>(), *dW = c->rbW.as<double>();
    hipStream_t s = c->stream;
    PARTLS_HIP_CHECK(hipMemcpyAsync(dWp, wp.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(robust_init_kernel, dim3(1), dim3(RB_THREADS), 0, s, dst, N);
    PARTLS_HIP_CHECK(hipGetLastError());
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[0], s));
    if (c->storage == XStorage::csr) PARTLS_HIP_CHECK(launch_csr_residual(c->csr, nullptr, dWp, t, nullptr, 1024, dA, s));
    else PARTLS_HIP_CHECK(launch_residual(c->dX, N, M, c->ldX, nullptr, dWp, t, nullptr, 1024, dA, s, nullptr, c->x_f32));
    hipLaunchKernelGGL(robust_abs_kernel, dim3((unsigned)rblocks), dim3(RB_THREADS), 0, s, dA, c->dy, N);
    PARTLS_HIP_CHECK(hipGetLastError());
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[1], s));
    if (select)
        for (int pass = 0; pass < 8; ++pass) {
            hipLaunchKernelGGL(robust_hist_kernel, dim3(hgrid), dim3(RB_THREADS), 0, s, dA, N, dst, pass, nsel);
            hipLaunchKernelGGL(robust_scan_kernel, dim3(1), dim3(RB_THREADS), 0, s, dst, pass, nsel);
        }
    PARTLS_HIP_CHECK(hipGetLastError());
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[2], s));
    const int have_prev = c->rb_have ? 1 : 0;
    if (loss == PARTLS_ROBUST_HUBER)
        hipLaunchKernelGGL(robust_weight_kernel<PARTLS_ROBUST_HUBER>, dim3((unsigned)blocks), dim3(RB_THREADS), 0, s, dA, dW, N, dst, cc, scale_in,
                           nsel, have_prev, c->rbPart.as<double>());
    else
        hipLaunchKernelGGL(robust_weight_kernel<PARTLS_ROBUST_BISQUARE>, dim3((unsigned)blocks), dim3(RB_THREADS), 0, s, dA, dW, N, dst, cc,
                           scale_in, nsel, have_prev, c->rbPart.as<double>());
    PARTLS_HIP_CHECK(hipGetLastError());
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[3], s));
    double *hp = c->rbHost.data();
    PARTLS_HIP_CHECK(hipMemcpyAsync(hp, &dst->scale, sizeof(double), hipMemcpyDeviceToHost, s));
    PARTLS_HIP_CHECK(hipMemcpyAsync(hp + 1, c->rbPart.p, (size_t)4 * blocks * sizeof(double), hipMemcpyDeviceToHost, s));
    PARTLS_HIP_CHECK(hipStreamSynchronize(s));
    for (int ph = 0; ph < 3; ++ph) {
        float f = 0.f;
        c->rb_ms[ph] = hipEventElapsedTime(&f, ev.e[ph], ev.e[ph + 1]) == hipSuccess ? (double)f : 0.0;
    }
    const double sc = hp[0];
    double rs = 0.0, dm = 0.0, nd = 0.0, nz = 0.0;
    if (sc != 0.0) {                                              // (s == 0: the kernel wrote neither weights nor partials)
        for (int64_t b = 0; b < blocks; ++b) {
            const double *p = hp + 1 + 4 * b;
            rs += p[0];
            dm = p[1] > dm ? p[1] : dm;
            nd += p[2]; nz += p[3];
        }
        c->rb_have = true;
        if (w_out) {
            PARTLS_HIP_CHECK(hipMemcpyAsync(w_out, dW, (size_t)N * sizeof(double), host_rows ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
            PARTLS_HIP_CHECK(hipStreamSynchronize(s));
        }
    }
    if (scale) *scale = sc;
    if (rho_sum) *rho_sum = rs;
    if (max_dw) *max_dw = dm;
    if (n_down) *n_down = (int64_t)nd;
    if (n_zero) *n_zero = (int64_t)nz;
    return PARTLS_OK;
}

static partls_status reweight_common(partls_ctx *c, const double *w, int w_on_device)
{
    const char *who = "partls_opt_reweight";
    const partls_status st = check_prepared_single(c, who, PARTLS_ERR_STATE);
    if (st != PARTLS_OK) return st;
    if (!w) {
        if (!c->rb_have) { set_error("%s: w is NULL and no partls_robust_weights call has left weights since the last prepare", who); return PARTLS_ERR_STATE; }
        // the prepared problem gets a copy of its own: the next partls_robust_weights call updates rbW in place
        PARTLS_HIP_CHECK(hipSetDevice(c->device));
        PARTLS_HIP_CHECK(c->ownW.ensure((size_t)c->N * sizeof(double)));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->ownW.p, c->rbW.p, (size_t)c->N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return ctx_rework(c, c->ownW.as<double>(), nullptr, 1);
    }
    return ctx_rework(c, w, nullptr, w_on_device ? 1 : 0);
}

}  // namespace partls

using namespace partls;

extern "C" {

partls_status partls_robust_weights(partls_ctx *c, const double *alpha, const double *beta, double t, int loss, double cc, double scale_in,
                                    double *scale, double *rho_sum, double *max_dw, int64_t *n_down, int64_t *n_zero, double *w_out)
try {
    return robust_weights_common(c, alpha, beta, t, loss, cc, scale_in, scale, rho_sum, max_dw, n_down, n_zero, w_out);
}
PARTLS_ABI_GUARD

partls_status partls_opt_reweight(partls_ctx *c, const double *w, int w_on_device)
try {
    return reweight_common(c, w, w_on_device);
}
PARTLS_ABI_GUARD

partls_status partls_get_robust_timing(const partls_ctx *c, double *residual_ms, double *select_ms, double *weights_ms)
try {
    if (!c || !residual_ms || !select_ms || !weights_ms) { set_error("partls_get_robust_timing: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *residual_ms = c->rb_ms[0]; *select_ms = c->rb_ms[1]; *weights_ms = c->rb_ms[2];
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

}
