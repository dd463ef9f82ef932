// predict_many.hip — partls_predict_many(_f32): the predictions of B models in one pass over X per PARTLS_PREDICT_MANY_CHUNK models, and
// per-row order statistics and mean of the B predictions.  Kernels first, then the host driver and the two entries.
#include "ctx.h"
#include <cmath>
#include <vector>

namespace partls {

constexpr int PM_C = PARTLS_PREDICT_MANY_CHUNK;             // models a thread keeps in registers: 4 chains x PM_C accumulators
constexpr int PM_SORT_MAX = PARTLS_PREDICT_MANY_MAX_B;      // elements of one workgroup's sort (LDS: 8 bytes each)
constexpr int PM_SORT_ROWS = 8;                             // rows a workgroup sorts together when they fit (8 doubles = one 64-byte segment of a column)
static_assert((PM_SORT_MAX & (PM_SORT_MAX - 1)) == 0 && PM_SORT_MAX * sizeof(double) <= 65536, "a row of the cap is sorted in the LDS a launch gets without asking for more");

// ---------------------------------------------------------------------------------------------------------------------
// (a) Y[i, b] = row_predict(X, i, ., w_b, t_b) (misc.hip) for the PM_C models of chunk blockIdx.y: one thread per row, the four chains
// of every model of the chunk in registers, an element of X loaded (and widened) once per chunk.  Per (row, model) the arithmetic is
// row_predict's, operation for operation: a_c = fma(x[i, m], w[m], a_c) over m = c mod 4 in ascending m, the M mod 4 last columns on
// chain 0, ((a0 + a1) + (a2 + a3)) + t.  (Not the fp64 MFMA: its k-sum has another order.)
// Wt: the weights of chunk c at Wt + c M PM_C, [m][j] with j the model within the chunk (zero for a model past B); tv: the intercepts,
// padded alike.  Both are indexed by blockIdx and loop counters alone: wave-uniform, read through the scalar cache, and an fma takes
// the weight as its scalar operand.  A lane past N repeats row N - 1 and stores nothing.
// ---------------------------------------------------------------------------------------------------------------------
template <class XT>
__global__ __launch_bounds__(256) void predict_many_kernel(const XT *__restrict__ X, int64_t N, int64_t M, int64_t ldX,
                                                           const double *__restrict__ Wt, const double *__restrict__ tv, int64_t B,
                                                           double *__restrict__ Y, int64_t ldY)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const XT *x = X + (i < N ? i : N - 1);
    const double *w = Wt + (int64_t)blockIdx.y * M * PM_C;
    double a0[PM_C], a1[PM_C], a2[PM_C], a3[PM_C];
#pragma unroll
    for (int j = 0; j < PM_C; ++j) a0[j] = a1[j] = a2[j] = a3[j] = 0.0;
    int64_t m = 0;
    for (; m + 3 < M; m += 4) {
        const double x0 = (double)x[m * ldX], x1 = (double)x[(m + 1) * ldX], x2 = (double)x[(m + 2) * ldX], x3 = (double)x[(m + 3) * ldX];
        const double *wm = w + m * PM_C;
#pragma unroll
        for (int j = 0; j < PM_C; ++j) {
            a0[j] = fma(x0, wm[j], a0[j]);
            a1[j] = fma(x1, wm[PM_C + j], a1[j]);
            a2[j] = fma(x2, wm[2 * PM_C + j], a2[j]);
            a3[j] = fma(x3, wm[3 * PM_C + j], a3[j]);
        }
    }
    for (; m < M; ++m) {
        const double x0 = (double)x[m * ldX];
#pragma unroll
        for (int j = 0; j < PM_C; ++j) a0[j] = fma(x0, w[m * PM_C + j], a0[j]);
    }
    if (i >= N) return;
    const int64_t b0 = (int64_t)blockIdx.y * PM_C;
#pragma unroll
    for (int j = 0; j < PM_C; ++j)
        if (b0 + j < B) Y[i + (b0 + j) * ldY] = ((a0[j] + a1[j]) + (a2[j] + a3[j])) + tv[b0 + j];
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) stats[i, q] = the value at position ranks[q] of the ascending sort of Y[i, 0 .. B): a bitonic sort in LDS, exact for finite
// values, ties included (the network only ever exchanges values).  n = the power of two >= B; a workgroup sorts R = rows_per_group(n)
// consecutive rows at once, row r in s[r n .. (r + 1) n), padded with +inf (which sorts behind every prediction, so a rank below B
// never reads it).  The network over all R n elements with the last stage's direction forced up sorts every row ascending.  Loads
// walk the rows first: the R values of a column are one contiguous segment.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int rows_per_group(int n) { return n * PM_SORT_ROWS <= PM_SORT_MAX ? PM_SORT_ROWS : PM_SORT_MAX / n; }

__global__ __launch_bounds__(256) void row_select_kernel(const double *__restrict__ Y, int64_t rows, int64_t ldY, int B, int n,
                                                         const int64_t *__restrict__ ranks, int nr, double *__restrict__ S, int64_t ldS)
{
    extern __shared__ double s[];                        // R n doubles (dynamic: a small B leaves the LDS to more workgroups)
    const int R = rows_per_group(n), total = R * n;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int r = idx % R, b = idx / R;
        s[r * n + b] = (b < B && row0 + r < rows) ? Y[row0 + r + (int64_t)b * ldY] : INFINITY;
    }
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < total / 2; p += 256) {
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;     // a pair j apart within one row (j < n, rows n-aligned)
                const bool up = k == n || (lo & k) == 0;
                const double u = s[lo], v = s[hi];
                if ((u > v) == up) { s[lo] = v; s[hi] = u; }
            }
            __syncthreads();
        }
    for (int idx = threadIdx.x; idx < R * nr; idx += 256) {
        const int r = idx % R, q = idx / R;
        if (row0 + r < rows) S[row0 + r + (int64_t)q * ldS] = s[r * n + (int)ranks[q]];
    }
}

// mean[i] = (((Y[i,0] + Y[i,1]) + ...) + Y[i,B-1]) / B: one thread per row, the columns in index order
__global__ __launch_bounds__(256) void row_mean_kernel(const double *__restrict__ Y, int64_t rows, int64_t ldY, int64_t B, double *__restrict__ mean)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double s = 0.0;
    for (int64_t b = 0; b < B; ++b) s += Y[i + b * ldY];
    mean[i] = s / (double)B;
}

hipError_t launch_row_select(const double *Y, int64_t rows, int64_t ldY, int64_t B, const int64_t *ranks, int64_t nr, double *S, int64_t ldS,
                             hipStream_t stream)
{
    int n = 1;
    while (n < B) n <<= 1;
    const int R = rows_per_group(n);
    hipLaunchKernelGGL(row_select_kernel, dim3((unsigned)((rows + R - 1) / R)), dim3(256), (size_t)R * n * sizeof(double), stream, Y, rows, ldY, (int)B, n,
                       ranks, (int)nr, S, ldS);
    return hipGetLastError();
}

hipError_t launch_row_mean(const double *Y, int64_t rows, int64_t ldY, int64_t B, double *mean, hipStream_t stream)
{
    hipLaunchKernelGGL(row_mean_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, Y, rows, ldY, B, mean);
    return hipGetLastError();
}

// rows of a chunk: the N x B intermediate (and a host caller's device image of stats) within PARTLS_PREDICT_MANY_BYTES
static int64_t rows_per_chunk(int64_t N, int64_t B, int64_t nr)
{
    const int64_t cols = B > nr ? B : nr;
    const int64_t r = (int64_t)(PARTLS_PREDICT_MANY_BYTES / sizeof(double)) / cols;      // >= 2048: B, nr <= PARTLS_PREDICT_MANY_MAX_B
    return r < N ? r : N;
}

static partls_status predict_many_common(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, int x_on_device, const int64_t *P,
                                         int64_t K, int64_t ldP, int64_t B, const double *alpha, const double *beta, const double *t,
                                         double *yhat, int64_t ldY, int64_t nr, const int64_t *ranks, double *stats, double *mean, bool x_f32)
{
    const char *who = x_f32 ? "partls_predict_many_f32" : "partls_predict_many";
    partls_status st = check_common(c, X, N, M, ldX, P, K, ldP);
    if (st != PARTLS_OK) return st;
    if (B < 1) { set_error("%s: need B >= 1 (got %lld)", who, (long long)B); return PARTLS_ERR_BAD_ARG; }
    if (!alpha || !beta || !t) { set_error("%s: alpha, beta or t is NULL", who); return PARTLS_ERR_BAD_ARG; }
    if (!yhat && !stats && !mean) { set_error("%s: no output wanted (yhat, stats and mean are all NULL)", who); return PARTLS_ERR_BAD_ARG; }
    if (nr < 0 || (nr == 0) != (stats == nullptr) || (nr > 0 && !ranks)) {
        set_error("%s: stats must be NULL exactly when nr == 0, and ranks given when it is not (nr = %lld)", who, (long long)nr);
        return PARTLS_ERR_BAD_ARG;
    }
    if (yhat && ldY < N) { set_error("%s: ldY = %lld is smaller than N = %lld", who, (long long)ldY, (long long)N); return PARTLS_ERR_BAD_ARG; }
    if (B > PARTLS_PREDICT_MANY_MAX_B || nr > PARTLS_PREDICT_MANY_MAX_B) {
        set_error("%s: B = %lld models, nr = %lld ranks: this build supports at most %d of either in one call (predict in slices of columns)", who,
                  (long long)B, (long long)nr, PARTLS_PREDICT_MANY_MAX_B);
        return PARTLS_ERR_UNSUPPORTED;
    }
    for (int64_t q = 0; q < nr; ++q)
        if (ranks[q] < 0 || ranks[q] >= B) { set_error("%s: ranks[%lld] = %lld lies outside [0, B = %lld)", who, (long long)q, (long long)ranks[q], (long long)B); return PARTLS_ERR_BAD_ARG; }
    for (int64_t b = 0; b < B; ++b) {
        bool fin = std::isfinite(t[b]);
        for (int64_t m = 0; m < M && fin; ++m) fin = std::isfinite(alpha[m + b * M]);
        for (int64_t k = 0; k < K && fin; ++k) fin = std::isfinite(beta[k + b * K]);
        if (!fin) { set_error("%s: model %lld has a NaN / Inf in alpha, beta or t", who, (long long)b); return PARTLS_ERR_BAD_ARG; }
    }
    // the models as predict applies them, blocked by chunk: hw = [chunk][m][j] | intercepts, zero where a chunk runs past B
    const int64_t nch = (B + PM_C - 1) / PM_C, wcount = nch * M * PM_C;
    std::vector<double> hw((size_t)(wcount + nch * PM_C), 0.0), wb((size_t)M);
    for (int64_t b = 0; b < B; ++b) {
        st = predict_weights(P, M, K, ldP, alpha + b * M, beta + b * K, wb.data());
        if (st != PARTLS_OK) return st;
        double *dst = hw.data() + (b / PM_C) * M * PM_C + b % PM_C;
        for (int64_t m = 0; m < M; ++m) dst[m * PM_C] = wb[(size_t)m];
        hw[(size_t)(wcount + b)] = t[b];
    }

    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    PARTLS_HIP_CHECK(c->pmW.ensure(hw.size() * sizeof(double)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->pmW.p, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double *dW = c->pmW.as<double>(), *dT = dW + wcount;
    if (nr > 0) {
        PARTLS_HIP_CHECK(c->pmRanks.ensure((size_t)nr * sizeof(int64_t)));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->pmRanks.p, ranks, (size_t)nr * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    }
    const size_t esz = x_f32 ? sizeof(float) : sizeof(double);
    const char *dX = static_cast<const char *>(X);
    int64_t ld = ldX;
    if (!x_on_device) {
        PARTLS_HIP_CHECK(c->predX.ensure((size_t)N * M * esz));
        st = upload_matrix(c, c->predX.p, X, N, M, ldX, esz);
        if (st != PARTLS_OK) return st;
        dX = c->predX.as<char>(); ld = N;
    }
    const int64_t rmax = rows_per_chunk(N, B, nr);
    const bool direct = x_on_device && yhat;                 // the caller's device yhat is the intermediate
    if (!direct) PARTLS_HIP_CHECK(c->pmY.ensure((size_t)rmax * B * sizeof(double)));
    if (!x_on_device && nr > 0) PARTLS_HIP_CHECK(c->pmStats.ensure((size_t)rmax * nr * sizeof(double)));
    if (!x_on_device && mean) PARTLS_HIP_CHECK(c->pmMean.ensure((size_t)N * sizeof(double)));
    for (int64_t r0 = 0; r0 < N; r0 += rmax) {
        const int64_t rows = N - r0 < rmax ? N - r0 : rmax;
        double *Y = direct ? yhat + r0 : c->pmY.as<double>();
        const int64_t ldy = direct ? ldY : rows;
        const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)nch);
        if (x_f32) hipLaunchKernelGGL(predict_many_kernel<float>, grid, dim3(256), 0, c->stream, reinterpret_cast<const float *>(dX) + r0, rows, M, ld, dW, dT, B, Y, ldy);
        else hipLaunchKernelGGL(predict_many_kernel<double>, grid, dim3(256), 0, c->stream, reinterpret_cast<const double *>(dX) + r0, rows, M, ld, dW, dT, B, Y, ldy);
        PARTLS_HIP_CHECK(hipGetLastError());
        if (yhat && !direct)
            PARTLS_HIP_CHECK(hipMemcpy2DAsync(yhat + r0, (size_t)ldY * sizeof(double), Y, (size_t)rows * sizeof(double), (size_t)rows * sizeof(double),
                                              (size_t)B, hipMemcpyDeviceToHost, c->stream));
        if (nr > 0) {
            double *S = x_on_device ? stats + r0 : c->pmStats.as<double>();
            const int64_t lds = x_on_device ? N : rows;
            PARTLS_HIP_CHECK(launch_row_select(Y, rows, ldy, B, c->pmRanks.as<int64_t>(), nr, S, lds, c->stream));
            if (!x_on_device)
                PARTLS_HIP_CHECK(hipMemcpy2DAsync(stats + r0, (size_t)N * sizeof(double), S, (size_t)rows * sizeof(double), (size_t)rows * sizeof(double),
                                                  (size_t)nr, hipMemcpyDeviceToHost, c->stream));
        }
        if (mean) {
            double *mu = (x_on_device ? mean : c->pmMean.as<double>()) + r0;
            PARTLS_HIP_CHECK(launch_row_mean(Y, rows, ldy, B, mu, c->stream));
        }
    }
    if (!x_on_device && mean)
        PARTLS_HIP_CHECK(hipMemcpyAsync(mean, c->pmMean.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (!x_on_device) { c->predX.release(); c->pmY.release(); c->pmStats.release(); c->pmMean.release(); }    // a prediction set is not retained
    return PARTLS_OK;
}

}  // namespace partls

using namespace partls;

extern "C" {

partls_status partls_predict_many(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, int x_on_device, const int64_t *P,
                                  int64_t K, int64_t ldP, int64_t B, const double *alpha, const double *beta, const double *t, double *yhat,
                                  int64_t ldY, int64_t nr, const int64_t *ranks, double *stats, double *mean)
try {
    return predict_many_common(c, X, N, M, ldX, x_on_device, P, K, ldP, B, alpha, beta, t, yhat, ldY, nr, ranks, stats, mean, false);
}
PARTLS_ABI_GUARD

partls_status partls_predict_many_f32(partls_ctx *c, const float *X, int64_t N, int64_t M, int64_t ldX, int x_on_device, const int64_t *P,
                                      int64_t K, int64_t ldP, int64_t B, const double *alpha, const double *beta, const double *t,
                                      double *yhat, int64_t ldY, int64_t nr, const int64_t *ranks, double *stats, double *mean)
try {
    return predict_many_common(c, X, N, M, ldX, x_on_device, P, K, ldP, B, alpha, beta, t, yhat, ldY, nr, ranks, stats, mean, true);
}
PARTLS_ABI_GUARD

}
