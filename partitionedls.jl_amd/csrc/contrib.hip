// contrib.hip — partls_contributions(_f32): the N x K group contributions of B models in one pass over X per PARTLS_CONTRIB_CHUNK
// models, their per-(row, group) order statistics and mean over the models (the kernels of predict_many.hip) and their per-(group,
// model) sums over the rows.  Kernels first, then the entry's share of the host side (the row-chunk driver is
// many_model_pass, predict_many.hip) and the two entries.
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
// blockIdx.y, blockIdx.y + gridDim.y, ... by block_tree_256 (a fixed tree; a lane past the last row adds +0.0): part[(blk cols + col) 3
// + s] for s = 0: c, 1: |c|, 2: c^2.  Column col = k + K b of the chunk is C[. + ldC col].  launch_fold_partials then adds a chunk's
// block sums to the 3 cols running sums, zeroed before the first chunk: ((0.0 + block 0) + block 1) + ... over the blocks of all chunks.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void contrib_sums_kernel(const double *__restrict__ C, int64_t rows, int64_t ldC, int64_t cols,
                                                           double *__restrict__ part)
{
    __shared__ double red[3][256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t col = blockIdx.y; col < cols; col += gridDim.y) {
        const double v = i < rows ? C[i + ldC * col] : 0.0;
        double s[3] = {v, fabs(v), v * v};
        block_tree_256<3>(red, s);
        __syncthreads();                                     // every thread has read its results before the next column overwrites them
        if (threadIdx.x == 0) {
            double *p = part + ((int64_t)blockIdx.x * cols + col) * 3;
            p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
        }
    }
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
    ManyModelPass mp;
    mp.who = who; mp.ld_name = "ldC"; mp.slices = "call in slices of models";
    mp.K = K; mp.B = B; mp.x_f32 = x_f32; mp.out = contrib; mp.ld_out = ldC; mp.nr = nr; mp.ranks = ranks; mp.stats = stats; mp.mean = mean;
    if ((st = many_model_check(mp, N)) != PARTLS_OK) return st;
    if ((st = check_models(who, alpha, ld_alpha, beta, ld_beta, nullptr, M, K, B, /*many=*/true)) != PARTLS_OK) return st;
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
    PARTLS_HIP_CHECK(c->mmW.ensure(hw.size() * sizeof(double)));
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->mmW.p, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double *dW = c->mmW.as<double>();
    const int *dPtr = reinterpret_cast<const int *>(dW + wcount), *dIdx = dPtr + K + 1;
    const int64_t budget = c->knobs.contrib_bytes > 0 ? (int64_t)c->knobs.contrib_bytes : (int64_t)PARTLS_PREDICT_MANY_BYTES;
    mp.rmax = contrib_rows_per_chunk(N, K, B, nr, budget);
    mp.produce = [&](const void *dX, int64_t ld, int64_t r0, int64_t rows, double *Cc, int64_t ldc) {
        const int64_t blocks = (rows + 255) / 256;
        const dim3 grid((unsigned)blocks, (unsigned)nch, contrib_group_split(c, blocks, nch, K));
        if (x_f32) hipLaunchKernelGGL(contrib_kernel<float>, grid, dim3(256), 0, c->stream, static_cast<const float *>(dX) + r0, rows, ld, (int)K, dPtr, dIdx, dW, B, Cc, ldc);
        else hipLaunchKernelGGL(contrib_kernel<double>, grid, dim3(256), 0, c->stream, static_cast<const double *>(dX) + r0, rows, ld, (int)K, dPtr, dIdx, dW, B, Cc, ldc);
        return hipGetLastError();
    };
    if (sums) {
        const int64_t bmax = (mp.rmax + 255) / 256;
        PARTLS_HIP_CHECK(c->mmSums.ensure((size_t)(3 * cols * (1 + bmax)) * sizeof(double)));
        double *dRun = c->mmSums.as<double>(), *dPart = dRun + 3 * cols;
        PARTLS_HIP_CHECK(hipMemsetAsync(dRun, 0, (size_t)(3 * cols) * sizeof(double), c->stream));     // all bits zero: +0.0
        mp.chunk_done = [=](const double *Cc, int64_t rows, int64_t ldc, bool last) -> partls_status {
            const int64_t blocks = (rows + 255) / 256;
            const unsigned gy = (unsigned)(cols < 1024 ? cols : 1024);
            hipLaunchKernelGGL(contrib_sums_kernel, dim3((unsigned)blocks, gy), dim3(256), 0, c->stream, Cc, rows, ldc, cols, dPart);
            PARTLS_HIP_CHECK(hipGetLastError());
            PARTLS_HIP_CHECK(launch_fold_partials(dPart, blocks, 3 * cols, dRun, c->stream));
            if (last) PARTLS_HIP_CHECK(hipMemcpyAsync(sums, dRun, (size_t)(3 * cols) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            return PARTLS_OK;
        };
    }
    return many_model_pass(c, mp, X, N, M, ldX, x_on_device);
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
