// contrib.hip — partls_contributions(_f32): the N x K group contributions of B models in one pass over X per PARTLS_CONTRIB_CHUNK
// models, their per-(row, group) order statistics and mean over the models (the kernels of predict_many.hip) and their per-(group,
// model) sums over the rows.  Kernels first, then the host driver and the two entries.
#include "ctx.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace partls {

constexpr int CT_C = PARTLS_CONTRIB_CHUNK;                  // models a thread keeps in registers: one chain each, of one group at a time

// ---------------------------------------------------------------------------------------------------------------------
// (a) C[i, k, b] = the fma chain over the features of group k in ascending m, from 0.0, for the CT_C models of chunk blockIdx.y: one
// thread per row, one group's accumulators live at a time, an element of X loaded (and widened, as row_predict widens it) once per
// chunk and group it belongs to — once per chunk for a partition.
// gptr[K + 1], gidx: the group lists (features of group k: gidx[gptr[k] .. gptr[k + 1]), ascending); Wt: the weights of chunk c at
// Wt + c L CT_C with L = gptr[K], [list entry][j] with j the model within the chunk (zero for a model past B).  All three are indexed
// by blockIdx and loop counters alone: wave-uniform, read through the scalar cache, and an fma takes the weight as its scalar
// operand.  Element (i, k, b) goes to C[i + ldC (k + K b)].  A lane past N repeats row N - 1 and stores nothing.  No LDS, no barrier,
// no atomics.  The groups k = blockIdx.z, blockIdx.z + gridDim.z, ... are this workgroup's: few rows and few models still fill the
// device (contrib_group_split), and an entry is the same chain whichever workgroup computes it.
// ---------------------------------------------------------------------------------------------------------------------
template <class XT>
__global__ __launch_bounds__(256) void contrib_kernel(const XT *__restrict__ X, int64_t N, int64_t ldX, int K, const int *__restrict__ gptr,
                                                      const int *__restrict__ gidx, const double *__restrict__ Wt, int64_t B,
                                                      double *__restrict__ C, int64_t ldC)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const XT *x = X + (i < N ? i : N - 1);
    const double *w = Wt + (int64_t)blockIdx.y * gptr[K] * CT_C;
    const int64_t b0 = (int64_t)blockIdx.y * CT_C;
    for (int k = blockIdx.z; k < K; k += gridDim.z) {
        double a[CT_C];
#pragma unroll
        for (int j = 0; j < CT_C; ++j) a[j] = 0.0;
        const int e1 = gptr[k + 1];
        int e = gptr[k];
        for (; e + 3 < e1; e += 4) {                         // four loads of X in flight; the chain takes them in ascending order
            const double x0 = (double)x[(int64_t)gidx[e] * ldX], x1 = (double)x[(int64_t)gidx[e + 1] * ldX];
            const double x2 = (double)x[(int64_t)gidx[e + 2] * ldX], x3 = (double)x[(int64_t)gidx[e + 3] * ldX];
            const double *we = w + (int64_t)e * CT_C;
#pragma unroll
            for (int j = 0; j < CT_C; ++j) a[j] = fma(x0, we[j], a[j]);
#pragma unroll
            for (int j = 0; j < CT_C; ++j) a[j] = fma(x1, we[CT_C + j], a[j]);
#pragma unroll
            for (int j = 0; j < CT_C; ++j) a[j] = fma(x2, we[2 * CT_C + j], a[j]);
#pragma unroll
            for (int j = 0; j < CT_C; ++j) a[j] = fma(x3, we[3 * CT_C + j], a[j]);
        }
        for (; e < e1; ++e) {
            const double xv = (double)x[(int64_t)gidx[e] * ldX];
            const double *we = w + (int64_t)e * CT_C;
#pragma unroll
            for (int j = 0; j < CT_C; ++j) a[j] = fma(xv, we[j], a[j]);
        }
        if (i < N) {
#pragma unroll
            for (int j = 0; j < CT_C; ++j)
                if (b0 + j < B) C[i + ldC * (k + (int64_t)K * (b0 + j))] = a[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) the sums over the rows, in an order that is a function of N alone.  The rows of a chunk (which begins at a multiple of 256 of the
// global row index) are cut into blocks of 256; workgroup (blockIdx.x, blockIdx.y) sums block blockIdx.x of the columns (k, b) =
// blockIdx.y, blockIdx.y + gridDim.y, ... by block_sum_256 (a fixed tree; a lane past the last row adds +0.0): part[(blk cols + col) 3
// + s] for s = 0: c, 1: |c|, 2: c^2.  Column col = k + K b of the chunk is C[. + ldC col].
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void contrib_sums_kernel(const double *__restrict__ C, int64_t rows, int64_t ldC, int64_t cols,
                                                           double *__restrict__ part)
{
    __shared__ double red[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t col = blockIdx.y; col < cols; col += gridDim.y) {
        const double v = i < rows ? C[i + ldC * col] : 0.0;
        const double s0 = block_sum_256(red, v);
        __syncthreads();                                     // every thread has read red[0] before the next sum overwrites it
        const double s1 = block_sum_256(red, fabs(v));
        __syncthreads();
        const double s2 = block_sum_256(red, v * v);
        __syncthreads();
        if (threadIdx.x == 0) {
            double *p = part + ((int64_t)blockIdx.x * cols + col) * 3;
            p[0] = s0; p[1] = s1; p[2] = s2;
        }
    }
}

// ... and the block sums of a chunk added to the running sums in ascending block order: one thread per (column, s).  run: 3 cols
// doubles, zeroed before the first chunk, so that every sum is ((0.0 + block 0) + block 1) + ... over the blocks of all chunks.
__global__ __launch_bounds__(256) void contrib_sums_fold_kernel(const double *__restrict__ part, int64_t blocks, int64_t cols, double *__restrict__ run)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= 3 * cols) return;
    double s = run[q];
    for (int64_t blk = 0; blk < blocks; ++blk) s += part[blk * 3 * cols + q];
    run[q] = s;
}

// rows of a chunk: the rows x K x max(B, nr) intermediate within `budget` bytes, a multiple of 256 rows and at least 256 (so that the
// blocks of the sums never straddle a seam); all of N when that fits
static int64_t contrib_rows_per_chunk(int64_t N, int64_t K, int64_t B, int64_t nr, int64_t budget)
{
    const int64_t cols = K * (B > nr ? B : nr);
    int64_t r = budget / (int64_t)sizeof(double) / cols / 256 * 256;
    if (r < 256) r = 256;
    return r < N ? r : N;
}

// gridDim.z of contrib_kernel: the groups are dealt to as many workgroups per (row block, model chunk) as bring the launch to about
// eight waves per SIMD, at most K (N = 1e5 rows and one model are 1564 waves for 1024 SIMDs, each walking all M features)
static unsigned contrib_group_split(const partls_ctx *c, int64_t blocks, int64_t nch, int64_t K)
{
    const int64_t waves = blocks * 4 * nch, target = (int64_t)c->ncu * 4 * 8;
    const int64_t z = (target + waves - 1) / waves;
    return (unsigned)(z < 1 ? 1 : (z > K ? K : z));
}

static partls_status contrib_common(partls_ctx *c, const void *X, int64_t N, int64_t M, int64_t ldX, int x_on_device, const int64_t *P,
                                    int64_t K, int64_t ldP, int64_t B, const double *alpha, int64_t ld_alpha, const double *beta,
                                    int64_t ld_beta, double *contrib, int64_t ldC, int64_t nr, const int64_t *ranks, double *stats,
                                    double *mean, double *sums, bool x_f32)
{
    const char *who = x_f32 ? "partls_contributions_f32" : "partls_contributions";
    partls_status st = check_common(c, X, N, M, ldX, P, K, ldP);
    if (st != PARTLS_OK) return st;
    if (B < 1) { set_error("%s: need B >= 1 (got %lld)", who, (long long)B); return PARTLS_ERR_BAD_ARG; }
    if (!alpha || !beta) { set_error("%s: alpha or beta is NULL", who); return PARTLS_ERR_BAD_ARG; }
    if (ld_alpha < M || ld_beta < K) {
        set_error("%s: ld_alpha = %lld, ld_beta = %lld are smaller than M = %lld, K = %lld", who, (long long)ld_alpha, (long long)ld_beta, (long long)M, (long long)K);
        return PARTLS_ERR_BAD_ARG;
    }
    if (!contrib && !stats && !mean && !sums) { set_error("%s: no output wanted (contrib, stats, mean and sums are all NULL)", who); return PARTLS_ERR_BAD_ARG; }
    if (nr < 0 || (nr == 0) != (stats == nullptr) || (nr > 0 && !ranks)) {
        set_error("%s: stats must be NULL exactly when nr == 0, and ranks given when it is not (nr = %lld)", who, (long long)nr);
        return PARTLS_ERR_BAD_ARG;
    }
    if (contrib && ldC < N) { set_error("%s: ldC = %lld is smaller than N = %lld", who, (long long)ldC, (long long)N); return PARTLS_ERR_BAD_ARG; }
    if (B > PARTLS_PREDICT_MANY_MAX_B || nr > PARTLS_PREDICT_MANY_MAX_B) {
        set_error("%s: B = %lld models, nr = %lld ranks: this build supports at most %d of either in one call (call in slices of models)", who,
                  (long long)B, (long long)nr, PARTLS_PREDICT_MANY_MAX_B);
        return PARTLS_ERR_UNSUPPORTED;
    }
    for (int64_t q = 0; q < nr; ++q)
        if (ranks[q] < 0 || ranks[q] >= B) { set_error("%s: ranks[%lld] = %lld lies outside [0, B = %lld)", who, (long long)q, (long long)ranks[q], (long long)B); return PARTLS_ERR_BAD_ARG; }
    for (int64_t b = 0; b < B; ++b) {
        bool fin = true;
        for (int64_t m = 0; m < M && fin; ++m) fin = std::isfinite(alpha[m + b * ld_alpha]);
        for (int64_t k = 0; k < K && fin; ++k) fin = std::isfinite(beta[k + b * ld_beta]);
        if (!fin) { set_error("%s: model %lld has a NaN / Inf in alpha or beta", who, (long long)b); return PARTLS_ERR_BAD_ARG; }
    }
    // the group lists of P, and the models as predict_weights forms its terms, blocked by chunk: hw = [chunk][list entry][j], zero where
    // a chunk runs past B
    std::vector<int> lists((size_t)K + 1, 0);
    for (int64_t k = 0; k < K; ++k) {
        for (int64_t m = 0; m < M; ++m) {
            const int64_t v = P[m + k * ldP];
            if (v != 0 && v != 1) { set_error("P has an entry outside {0,1}"); return PARTLS_ERR_BAD_PARTITION; }
            if (v) lists.push_back((int)m);
        }
        lists[(size_t)k + 1] = (int)(lists.size() - (size_t)(K + 1));
    }
    const int64_t L = lists[(size_t)K], nch = (B + CT_C - 1) / CT_C, cols = K * B;
    const size_t wcount = (size_t)(nch * L * CT_C), lbytes = lists.size() * sizeof(int);
    std::vector<double> hw(wcount + (lbytes + sizeof(double) - 1) / sizeof(double), 0.0);      // ... | the lists: one upload
    memcpy(hw.data() + wcount, lists.data(), lbytes);
    for (int64_t b = 0; b < B; ++b) {
        double *dst = hw.data() + (b / CT_C) * L * CT_C + b % CT_C;
        for (int64_t k = 0; k < K; ++k)
            for (int e = lists[(size_t)k]; e < lists[(size_t)k + 1]; ++e) {
                const int64_t m = lists[(size_t)(K + 1 + e)];
                dst[(int64_t)e * CT_C] = (double)P[m + k * ldP] * alpha[m + b * ld_alpha] * beta[k + b * ld_beta];
            }
    }

    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    PARTLS_HIP_CHECK(c->ctW.ensure(hw.size() * sizeof(double)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->ctW.p, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double *dW = c->ctW.as<double>();
    const int *dPtr = reinterpret_cast<const int *>(dW + wcount), *dIdx = dPtr + K + 1;
    if (nr > 0) {
        PARTLS_HIP_CHECK(c->pmRanks.ensure((size_t)nr * sizeof(int64_t)));
        PARTLS_HIP_CHECK(hipMemcpyAsync(c->pmRanks.p, ranks, (size_t)nr * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    }
    auto run = [&]() -> partls_status {
        const size_t esz = x_f32 ? sizeof(float) : sizeof(double);
        const char *dX = static_cast<const char *>(X);
        int64_t ld = ldX;
        if (!x_on_device) {
            PARTLS_HIP_CHECK(c->predX.ensure((size_t)N * M * esz));
            const partls_status us = upload_matrix(c, c->predX.p, X, N, M, ldX, esz);
            if (us != PARTLS_OK) return us;
            dX = c->predX.as<char>(); ld = N;
        }
        const int64_t budget = c->knobs.contrib_bytes > 0 ? (int64_t)c->knobs.contrib_bytes : (int64_t)PARTLS_PREDICT_MANY_BYTES;
        const int64_t rmax = contrib_rows_per_chunk(N, K, B, nr, budget), bmax = (rmax + 255) / 256;
        const bool direct = x_on_device && contrib;              // the caller's device contrib is the intermediate
        if (!direct) PARTLS_HIP_CHECK(c->ctC.ensure((size_t)rmax * cols * sizeof(double)));
        if (!x_on_device && nr > 0) PARTLS_HIP_CHECK(c->ctStats.ensure((size_t)rmax * K * nr * sizeof(double)));
        if (!x_on_device && mean) PARTLS_HIP_CHECK(c->ctMean.ensure((size_t)rmax * K * sizeof(double)));
        double *dRun = nullptr, *dPart = nullptr;
        if (sums) {
            PARTLS_HIP_CHECK(c->ctSums.ensure((size_t)(3 * cols * (1 + bmax)) * sizeof(double)));
            dRun = c->ctSums.as<double>(); dPart = dRun + 3 * cols;
            PARTLS_HIP_CHECK(hipMemsetAsync(dRun, 0, (size_t)(3 * cols) * sizeof(double), c->stream));     // all bits zero: +0.0
        }
        for (int64_t r0 = 0; r0 < N; r0 += rmax) {
            const int64_t rows = N - r0 < rmax ? N - r0 : rmax, blocks = (rows + 255) / 256;
            double *Cc = direct ? contrib + r0 : c->ctC.as<double>();
            const int64_t ldc = direct ? ldC : rows;
            const dim3 grid((unsigned)blocks, (unsigned)nch, contrib_group_split(c, blocks, nch, K));
            if (x_f32) hipLaunchKernelGGL(contrib_kernel<float>, grid, dim3(256), 0, c->stream, reinterpret_cast<const float *>(dX) + r0, rows, ld, (int)K, dPtr, dIdx, dW, B, Cc, ldc);
            else hipLaunchKernelGGL(contrib_kernel<double>, grid, dim3(256), 0, c->stream, reinterpret_cast<const double *>(dX) + r0, rows, ld, (int)K, dPtr, dIdx, dW, B, Cc, ldc);
            PARTLS_HIP_CHECK(hipGetLastError());
            if (contrib && !direct)
                PARTLS_HIP_CHECK(hipMemcpy2DAsync(contrib + r0, (size_t)ldC * sizeof(double), Cc, (size_t)rows * sizeof(double), (size_t)rows * sizeof(double),
                                                  (size_t)cols, hipMemcpyDeviceToHost, c->stream));
            // the (row, group) pairs of the chunk as the rows of a matrix with B columns, ld = ldc K: one matrix of rows K rows when the
            // groups follow each other without a gap on both sides (ldc == rows, and so for the output), else one of `rows` rows per group
            if (nr > 0) {
                double *S = x_on_device ? stats + r0 : c->ctStats.as<double>();
                const int64_t lds = x_on_device ? N : rows;
                if (ldc == rows && lds == rows) PARTLS_HIP_CHECK(launch_row_select(Cc, rows * K, ldc * K, B, c->pmRanks.as<int64_t>(), nr, S, lds * K, c->stream));
                else
                    for (int64_t k = 0; k < K; ++k)
                        PARTLS_HIP_CHECK(launch_row_select(Cc + ldc * k, rows, ldc * K, B, c->pmRanks.as<int64_t>(), nr, S + lds * k, lds * K, c->stream));
                if (!x_on_device)
                    PARTLS_HIP_CHECK(hipMemcpy2DAsync(stats + r0, (size_t)N * sizeof(double), S, (size_t)rows * sizeof(double), (size_t)rows * sizeof(double),
                                                      (size_t)(K * nr), hipMemcpyDeviceToHost, c->stream));
            }
            if (mean) {
                double *mu = x_on_device ? mean + r0 : c->ctMean.as<double>();
                const int64_t ldm = x_on_device ? N : rows;
                if (ldc == rows && ldm == rows) PARTLS_HIP_CHECK(launch_row_mean(Cc, rows * K, ldc * K, B, mu, c->stream));
                else
                    for (int64_t k = 0; k < K; ++k) PARTLS_HIP_CHECK(launch_row_mean(Cc + ldc * k, rows, ldc * K, B, mu + ldm * k, c->stream));
                if (!x_on_device)
                    PARTLS_HIP_CHECK(hipMemcpy2DAsync(mean + r0, (size_t)N * sizeof(double), mu, (size_t)rows * sizeof(double), (size_t)rows * sizeof(double),
                                                      (size_t)K, hipMemcpyDeviceToHost, c->stream));
            }
            if (sums) {
                const unsigned gy = (unsigned)(cols < 1024 ? cols : 1024);
                hipLaunchKernelGGL(contrib_sums_kernel, dim3((unsigned)blocks, gy), dim3(256), 0, c->stream, Cc, rows, ldc, cols, dPart);
                PARTLS_HIP_CHECK(hipGetLastError());
                hipLaunchKernelGGL(contrib_sums_fold_kernel, dim3((unsigned)((3 * cols + 255) / 256)), dim3(256), 0, c->stream, dPart, blocks, cols, dRun);
                PARTLS_HIP_CHECK(hipGetLastError());
            }
        }
        if (sums) PARTLS_HIP_CHECK(hipMemcpyAsync(sums, dRun, (size_t)(3 * cols) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return PARTLS_OK;
    };
    st = run();
    if (!x_on_device) { c->predX.release(); c->ctC.release(); c->ctStats.release(); c->ctMean.release(); }    // a prediction set is not retained
    return st;
}

}  // namespace partls

using namespace partls;

extern "C" {

partls_status partls_contributions(partls_ctx *c, const double *X, int64_t N, int64_t M, int64_t ldX, int x_on_device, const int64_t *P,
                                   int64_t K, int64_t ldP, int64_t B, const double *alpha, int64_t ld_alpha, const double *beta,
                                   int64_t ld_beta, double *contrib, int64_t ldC, int64_t nr, const int64_t *ranks, double *stats,
                                   double *mean, double *sums)
try {
    return contrib_common(c, X, N, M, ldX, x_on_device, P, K, ldP, B, alpha, ld_alpha, beta, ld_beta, contrib, ldC, nr, ranks, stats, mean, sums, false);
}
PARTLS_ABI_GUARD

partls_status partls_contributions_f32(partls_ctx *c, const float *X, int64_t N, int64_t M, int64_t ldX, int x_on_device, const int64_t *P,
                                       int64_t K, int64_t ldP, int64_t B, const double *alpha, int64_t ld_alpha, const double *beta,
                                       int64_t ld_beta, double *contrib, int64_t ldC, int64_t nr, const int64_t *ranks, double *stats,
                                       double *mean, double *sums)
try {
    return contrib_common(c, X, N, M, ldX, x_on_device, P, K, ldP, B, alpha, ld_alpha, beta, ld_beta, contrib, ldC, nr, ranks, stats, mean, sums, true);
}
PARTLS_ABI_GUARD

}
