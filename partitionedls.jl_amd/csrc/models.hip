// models.hip — every pattern's model straight from the sweep (partls_opt_models; Opt.jl:87-101 without one solve per pattern).
//
// The export instantiation of the sweep kernels leaves, for every Gray index g of a piece, the scaled solution of its subproblem in
// tableau order (basic ? q : 0) and its objective.  This kernel turns a piece of those rows into what the host path makes of ONE pattern,
// with the same arithmetic in the same order:
//   * reference index b: g ^ (g >> 1) through the visiting order (api.hip: reference_pattern);
//   * w over [features, intercept]: w[perm[v]] = sol[v] * scale[v] (api.hip: unscale_solution; null columns have scale 0);
//   * raw alpha of partls_opt_pattern: max(w_m / f_m, 0), f_m = sum_k P[m,k] s_k in {0, +-1, +-2, ...}, 0 where f_m = 0;
//   * cleanupResult (Opt.jl:34-44, api.hip: cleanup_opt): beta_k = s_k sum_{m in k} a_m, A_k = that sum or 1 where it is 0,
//     alpha_m = sum_{k ∋ m} a_m / A_k, t = w_I.
// One wave per pattern; the sums run sequentially in index order (member terms only: the host's zero terms add nothing), so the
// results are bitwise those of the host formulas applied to the same w.
#include "sweep_rules.h"

namespace partls {

static constexpr int MD_THREADS = 64;

__global__ __launch_bounds__(MD_THREADS) void models_cleanup_kernel(double *__restrict__ sol, const double *__restrict__ obj, int64_t g0,
                                                                    int64_t cnt, int M, int K, int kbits, BitOrder order, int order_identity,
                                                                    const int *__restrict__ perm, const double *__restrict__ scale,
                                                                    const uint64_t *__restrict__ mask_aug, int want_raw, double *__restrict__ out,
                                                                    const int64_t *__restrict__ glist)
{
    extern __shared__ double md_smem[];
    const int n = M + 1, lane = threadIdx.x;
    double *w = md_smem;                                          // [n] unscaled solution over [features, intercept]
    double *a = w + n;                                            // [M] raw alpha, clamped as cleanup_opt does
    double *A = a + M;                                            // [K] group sums (1 where the sum is 0)
    uint64_t *msk = reinterpret_cast<uint64_t *>(A + K);          // [n] group masks (reference bit order; intercept: bit K)
    for (int m = lane; m < n; m += MD_THREADS) msk[m] = mask_aug[m];
    int64_t *opat = reinterpret_cast<int64_t *>(out);
    double *oopt = out + cnt, *ot = out + 2 * cnt, *oal = out + 3 * cnt, *obe = oal + (size_t)cnt * M;
    __syncthreads();
    for (int64_t i = blockIdx.x; i < cnt; i += gridDim.x) {
        const uint64_t g = (uint64_t)(glist ? glist[i] : g0 + i), q = g ^ (g >> 1);   // glist: partls_opt_top's compact rows
        uint64_t b = q;
        if (!order_identity) {
            b = 0;
            for (int k = 0; k < kbits; ++k) b |= ((q >> order.gbit[k]) & 1ULL) << k;
        }
        const double o = obj[i];
        double *row = sol + (size_t)i * n;
        if (lane == 0) { opat[i] = (int64_t)b; oopt[i] = o; }
        if (o != o) {                                             // pivot cap: the sweep left NaN in the row (raw alpha stays NaN)
            const double nan = __builtin_nan("");
            for (int m = lane; m < M; m += MD_THREADS) oal[(size_t)i * M + m] = nan;
            for (int k = lane; k < K; k += MD_THREADS) obe[(size_t)i * K + k] = nan;
            if (lane == 0) ot[i] = nan;
            continue;                                             // wave-uniform
        }
        for (int v = lane; v < n; v += MD_THREADS) w[perm[v]] = row[v] * scale[v];
        __syncthreads();
        for (int m = lane; m < n; m += MD_THREADS) {
            const uint64_t mk = msk[m];
            const int f = sign_of_var(mk, b);
            const double r = (f != 0) ? w[m] / (double)f : 0.0;
            if (want_raw) row[m] = r > 0.0 ? r : 0.0;            // partls_opt_pattern's raw alpha, in place (row m of the output)
            if (m < M) a[m] = r < 0.0 ? 0.0 : r;
        }
        __syncthreads();
        for (int k = lane; k < K; k += MD_THREADS) {
            double s = 0.0;
            for (int m = 0; m < M; ++m)
                if ((msk[m] >> k) & 1ULL) s += a[m];
            obe[(size_t)i * K + k] = ((b >> k) & 1ULL) ? s : -s;
            A[k] = (s == 0.0) ? 1.0 : s;
        }
        __syncthreads();
        for (int m = lane; m < M; m += MD_THREADS) {
            const uint64_t mk = msk[m];
            double s = 0.0;
            for (int k = 0; k < K; ++k)
                if ((mk >> k) & 1ULL) s += a[m] / A[k];
            oal[(size_t)i * M + m] = s;
        }
        if (lane == 0) ot[i] = w[M];
        __syncthreads();                                          // w, a, A are the next pattern's
    }
}

hipError_t launch_models_cleanup(double *sol, const double *obj, int64_t g0, int64_t cnt, int M, int K, int kbits, const BitOrder &order,
                                 bool order_identity, const int *perm, const double *scale, const uint64_t *mask_aug, bool want_raw,
                                 double *out, hipStream_t s, const int64_t *glist)
{
    if (cnt <= 0) return hipSuccess;
    const size_t shmem = ((size_t)2 * (M + 1) + (size_t)M + (size_t)K) * sizeof(double);
    const int grid = (int)(cnt < 16384 ? cnt : 16384);
    hipLaunchKernelGGL(models_cleanup_kernel, dim3(grid), dim3(MD_THREADS), shmem, s, sol, obj, g0, cnt, M, K, kbits, order,
                       order_identity ? 1 : 0, perm, scale, mask_aug, want_raw ? 1 : 0, out, glist);
    return hipGetLastError();
}

}  // namespace partls
