// predict_many.hip — partls_predict_many(_f32): the predictions of B models in one pass over X per PARTLS_PREDICT_MANY_CHUNK models, and
// per-row order statistics and mean of the B predictions.  Kernels first, then the host driver of a many-model
// pass, which partls_contributions (contrib.hip) shares with the statistics kernels and the fold of partial sums, and the two entries.
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

// run[q] += part[blk stride + q], blk ascending: one thread per q, eight loads in flight, the adds in block order
__global__ __launch_bounds__(256) void fold_partials_kernel(const double *__restrict__ part, int64_t blocks, int64_t stride, double *__restrict__ run)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= stride) return;
    const double *p = part + q;
    double s = run[q];
    int64_t blk = 0;
    for (; blk + 8 <= blocks; blk += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(blk + k) * stride];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; blk < blocks; ++blk) s += p[blk * stride];
    run[q] = s;
}

hipError_t launch_fold_partials(const double *part, int64_t blocks, int64_t stride, double *run, hipStream_t stream)
{
    hipLaunchKernelGGL(fold_partials_kernel, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, stream, part, blocks, stride, run);
    return hipGetLastError();
}

// (c) the host driver of a many-model pass (ManyModelPass, ctx.h)
partls_status many_model_check(const ManyModelPass &mp, int64_t N)
{
    const char *who = mp.who; const int64_t B = mp.B, nr = mp.nr;
    if (nr < 0 || (nr == 0) != (mp.stats == nullptr) || (nr > 0 && !mp.ranks)) {
        set_error("%s: stats must be NULL exactly when nr == 0, and ranks given when it is not (nr = %lld)", who, (long long)nr);
        return PARTLS_ERR_BAD_ARG;
    }
    if (mp.out && mp.ld_out < N) { set_error("%s: %s = %lld is smaller than N = %lld", who, mp.ld_name, (long long)mp.ld_out, (long long)N); return PARTLS_ERR_BAD_ARG; }
    if (B > PARTLS_PREDICT_MANY_MAX_B || nr > PARTLS_PREDICT_MANY_MAX_B) {
        set_error("%s: B = %lld models, nr = %lld ranks: this build supports at most %d of either in one call (%s)", who, (long long)B,
                  (long long)nr, PARTLS_PREDICT_MANY_MAX_B, mp.slices);
        return PARTLS_ERR_UNSUPPORTED;
    }
    for (int64_t q = 0; q < nr; ++q)
        if (mp.ranks[q] < 0 || mp.ranks[q] >= B) { set_error("%s: ranks[%lld] = %lld lies outside [0, B = %lld)", who, (long long)q, (long long)mp.ranks[q], (long long)B); return PARTLS_ERR_BAD_ARG; }
    return PARTLS_OK;
}

partls_status many_model_pass(partls_ctx *c, const ManyModelPass &mp, const void *X, int64_t N, int64_t M, int64_t ldX, int x_on_device)
{
    const int64_t K = mp.K, B = mp.B, nr = mp.nr, rmax = mp.rmax;
    // a chunk's rows of ncol columns to the host; one column is contiguous on both sides and goes as the plain copy predict_many's mean always was
    auto to_host = [&](double *dst, int64_t ld_dst, const double *src, int64_t rows, int64_t ncol) {
        if (ncol == 1) return hipMemcpyAsync(dst, src, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        return hipMemcpy2DAsync(dst, (size_t)ld_dst * sizeof(double), src, (size_t)rows * sizeof(double), (size_t)rows * sizeof(double), (size_t)ncol,
                                hipMemcpyDeviceToHost, c->stream);
    };
    auto run = [&]() -> partls_status {
        if (nr > 0) {
            PARTLS_HIP_CHECK(c->mmRanks.ensure((size_t)nr * sizeof(int64_t)));
            PARTLS_HIP_CHECK(hipMemcpyAsync(c->mmRanks.p, mp.ranks, (size_t)nr * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        }
        const void *dX = nullptr; int64_t ld = 0;
        const partls_status us = stage_dense_x(c, X, N, M, ldX, x_on_device, mp.x_f32, &dX, &ld);
        if (us != PARTLS_OK) return us;
        const bool direct = x_on_device && mp.out;               // the caller's device output is the intermediate
        if (!direct) PARTLS_HIP_CHECK(c->mmY.ensure((size_t)rmax * K * B * sizeof(double)));
        if (!x_on_device && nr > 0) PARTLS_HIP_CHECK(c->mmStats.ensure((size_t)rmax * K * nr * sizeof(double)));
        if (!x_on_device && mp.mean) PARTLS_HIP_CHECK(c->mmMean.ensure((size_t)rmax * K * sizeof(double)));
        const int64_t *dRanks = c->mmRanks.as<int64_t>();
        for (int64_t r0 = 0; r0 < N; r0 += rmax) {
            const int64_t rows = N - r0 < rmax ? N - r0 : rmax;
            double *Y = direct ? mp.out + r0 : c->mmY.as<double>();
            const int64_t ldy = direct ? mp.ld_out : rows;
            PARTLS_HIP_CHECK(mp.produce(dX, ld, r0, rows, Y, ldy));
            if (mp.out && !direct) PARTLS_HIP_CHECK(to_host(mp.out + r0, mp.ld_out, Y, rows, K * B));
            // the (row, group) pairs of the chunk as the rows of a matrix with B columns, ld = ldy K: one matrix of rows K rows when the
            // groups follow each other without a gap on both sides (ldy == rows, and so for the output), else one of `rows` rows per group
            if (nr > 0) {
                double *S = x_on_device ? mp.stats + r0 : c->mmStats.as<double>();
                const int64_t lds = x_on_device ? N : rows;
                if (ldy == rows && lds == rows) PARTLS_HIP_CHECK(launch_row_select(Y, rows * K, ldy * K, B, dRanks, nr, S, lds * K, c->stream));
                else
                    for (int64_t k = 0; k < K; ++k)
                        PARTLS_HIP_CHECK(launch_row_select(Y + ldy * k, rows, ldy * K, B, dRanks, nr, S + lds * k, lds * K, c->stream));
                if (!x_on_device) PARTLS_HIP_CHECK(to_host(mp.stats + r0, N, S, rows, K * nr));
            }
            if (mp.mean) {
                double *mu = x_on_device ? mp.mean + r0 : c->mmMean.as<double>();
                const int64_t ldm = x_on_device ? N : rows;
                if (ldy == rows && ldm == rows) PARTLS_HIP_CHECK(launch_row_mean(Y, rows * K, ldy * K, B, mu, c->stream));
                else
                    for (int64_t k = 0; k < K; ++k) PARTLS_HIP_CHECK(launch_row_mean(Y + ldy * k, rows, ldy * K, B, mu + ldm * k, c->stream));
                if (!x_on_device) PARTLS_HIP_CHECK(to_host(mp.mean + r0, N, mu, rows, K));
            }
            if (mp.chunk_done) {
                const partls_status cs = mp.chunk_done(Y, rows, ldy, r0 + rows >= N);
                if (cs != PARTLS_OK) return cs;
            }
        }
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return PARTLS_OK;
    };
    const partls_status st = run();
    if (!x_on_device) { c->predX.release(); c->mmY.release(); c->mmStats.release(); c->mmMean.release(); }    // a prediction set is not retained
    return st;
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
    ManyModelPass mp;
    mp.who = who; mp.ld_name = "ldY"; mp.slices = "predict in slices of columns";
    mp.B = B; mp.x_f32 = x_f32; mp.out = yhat; mp.ld_out = ldY; mp.nr = nr; mp.ranks = ranks; mp.stats = stats; mp.mean = mean;
    if ((st = many_model_check(mp, N)) != PARTLS_OK) return st;
    if ((st = check_models(who, alpha, M, beta, K, t, M, K, B, /*many=*/true)) != PARTLS_OK) return st;
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
    PARTLS_HIP_CHECK(c->mmW.ensure(hw.size() * sizeof(double)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->mmW.p, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double *dW = c->mmW.as<double>(), *dT = dW + wcount;
    mp.rmax = rows_per_chunk(N, B, nr);
    mp.produce = [&](const void *dX, int64_t ld, int64_t r0, int64_t rows, double *Y, int64_t ldy) {
        const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)nch);
        if (x_f32) hipLaunchKernelGGL(predict_many_kernel<float>, grid, dim3(256), 0, c->stream, static_cast<const float *>(dX) + r0, rows, M, ld, dW, dT, B, Y, ldy);
        else hipLaunchKernelGGL(predict_many_kernel<double>, grid, dim3(256), 0, c->stream, static_cast<const double *>(dX) + r0, rows, M, ld, dW, dT, B, Y, ldy);
        return hipGetLastError();
    };
    return many_model_pass(c, mp, X, N, M, ldX, x_on_device);
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
