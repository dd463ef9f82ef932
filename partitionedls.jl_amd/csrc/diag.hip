// diag.hip — partls_diagnostics: leverage, leave-one-out / studentized residuals, Cook's distances, degrees of freedom and standard
// errors of one model on the context's prepared problem.  Conditional on the model's support A the fit is a linear
// smoother, and everything follows from q_i = ||T x_iA||^2 with T = L^-1, H = Xo_A' W Xo_A + eta Q_A = L L': the host gathers H from the
// Gram copy, factors it and forms T (p <= 1023), the leverage kernel below contracts T with the rows of X on the fp64 MFMA, and three
// small kernels form the sums and the per-row outputs.  Kernels first, then the host driver and the entries.
#include "ctx.h"
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace partls {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int LV_WAVES = 8;                     // waves of a workgroup: wave w owns the row tiles R = w, w + 8, ... of T
constexpr int LV_ST = 2;                        // 16-row tiles of X per workgroup: every fragment of T feeds two MFMAs
constexpr int LV_ROWS = 16 * LV_ST;             // rows of X per workgroup
constexpr int LV_MAX_RPW = 8;                   // row tiles per wave at p = 1023 + padding (64 tiles)

// ---------------------------------------------------------------------------------------------------------------------
// (a) q[i] = ||T x_iA||^2 for the LV_ROWS rows of workgroup blockIdx.x.  T (lower triangular, p x p, zero-padded to 16 nt) arrives as
// packed 16 x 16 tiles, stored tiles R >= C only, tile (R, C) at R (R + 1) / 2 + C, each as four k-steps of 64 doubles in the lane order
// of the A operand of v_mfma_f64_16x16x4_f64 (A[row = lane & 15][k = lane >> 4]): a fragment of T is one coalesced 512-byte load,
// shared by every workgroup and resident in L2.  The B operand (B[k = lane >> 4][col = lane & 15]) is X itself: col = the row of X,
// k = the active column idx[16 C + 4 ks + (lane >> 4)], so 16 lanes read 16 consecutive rows of one column (idx: the feature, -1 for
// the ones column: 1.0, -2 for the padding behind p: 0.0, where the columns of T are zero too; both load column 0 and discard it).
// A lane past N repeats row N - 1 and stores nothing.
// Loop order: column tile C outermost, the wave's row tiles R >= C inside — the tiles above the diagonal are never visited, a B
// fragment is loaded once per wave and C, and accumulator (R, tile of X) sums its k-steps in ascending k.  There is no MFMA-free
// phase: the loads of a step are issued in front of the MFMAs that consume the previous ones, and no barrier stands in the loop.
// Epilogue (the order of a row's sum is a function of nt alone): each lane squares and adds its four rows of every owned tile in
// ascending R, the four lane groups of a column are folded by two butterflies, and the LV_WAVES partial sums are added in wave order.
// ---------------------------------------------------------------------------------------------------------------------
template <class XT, int RPW>
__global__ __launch_bounds__(64 * LV_WAVES) void leverage_kernel(const XT *__restrict__ X, int64_t N, int64_t ldX, const double *__restrict__ Tp,
                                                                 const int *__restrict__ idx, int nt, double *__restrict__ q)
{
    __shared__ double part[LV_WAVES][LV_ROWS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int fr = lane & 15, fk = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * LV_ROWS;
    const XT *xr[LV_ST];
#pragma unroll
    for (int s = 0; s < LV_ST; ++s) {
        const int64_t i = i0 + s * 16 + fr;
        xr[s] = X + (i < N ? i : N - 1);
    }
    double4_t acc[RPW][LV_ST];
#pragma unroll
    for (int j = 0; j < RPW; ++j)
#pragma unroll
        for (int s = 0; s < LV_ST; ++s) acc[j][s] = (double4_t){0.0, 0.0, 0.0, 0.0};
    int rmax = -1;                               // the last row tile this wave owns (wave-uniform)
#pragma unroll
    for (int j = 0; j < RPW; ++j)
        if (wave + LV_WAVES * j < nt) rmax = wave + LV_WAVES * j;
    for (int C = 0; C <= rmax; ++C) {
        double b[4][LV_ST];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int m = idx[C * 16 + ks * 4 + fk];
            const int64_t off = (int64_t)(m > 0 ? m : 0) * ldX;
#pragma unroll
            for (int s = 0; s < LV_ST; ++s) {
                const double v = (double)xr[s][off];
                b[ks][s] = m >= 0 ? v : (m == -1 ? 1.0 : 0.0);
            }
        }
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const int R = wave + LV_WAVES * j;
            if (R >= C && R < nt) {              // wave-uniform
                const double *tp = Tp + ((size_t)(R * (R + 1) / 2 + C) * 4) * 64 + lane;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const double a = tp[ks * 64];
#pragma unroll
                    for (int s = 0; s < LV_ST; ++s) acc[j][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ks][s], acc[j][s], 0, 0, 0);
                }
            }
        }
    }
    // C/D map: col = lane & 15 (the row of X), row = (lane >> 4) + 4 * reg (the row of T within its tile)
#pragma unroll
    for (int s = 0; s < LV_ST; ++s) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < RPW; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) sum += acc[j][s][reg] * acc[j][s][reg];
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        if (fk == 0) part[wave][s * 16 + fr] = sum;
    }
    __syncthreads();
    if (threadIdx.x < LV_ROWS) {
        double sum = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < LV_WAVES; ++w) sum += part[w][threadIdx.x];
        const int64_t i = i0 + threadIdx.x;
        if (i < N) q[i] = sum;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) the per-row terms, written once: the sums kernel and the output kernel evaluate the same expressions (the build does not contract
// a * b + c), so the sums are the sums of the values the caller receives.  w == nullptr: an unweighted problem, w_i = 1.
// ---------------------------------------------------------------------------------------------------------------------
struct RowTerms { double w, e, h, loo; };
__device__ __forceinline__ RowTerms row_terms(const double *__restrict__ y, const double *__restrict__ yhat, const double *__restrict__ w,
                                              const double *__restrict__ q, int64_t i)
{
    RowTerms r;
    r.w = w ? w[i] : 1.0;
    r.e = y[i] - yhat[i];
    r.h = r.w * q[i];
    r.loo = r.e / (1.0 - r.h);
    return r;
}

// the sums over the rows by the rule of contrib_sums_kernel: block blockIdx.x of 256 rows, a fixed tree (a lane past N adds +0.0):
// part[4 blk + s], s = 0: leverage, 1: w e^2, 2: w loo^2, 3: rows with w > 0
__global__ __launch_bounds__(256) void diag_sums_kernel(const double *__restrict__ y, const double *__restrict__ yhat, const double *__restrict__ w,
                                                        const double *__restrict__ q, int64_t N, double *__restrict__ part)
{
    __shared__ double red[4][256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < N) {
        const RowTerms r = row_terms(y, yhat, w, q, i);
        v[0] = r.h; v[1] = (r.w * r.e) * r.e; v[2] = (r.w * r.loo) * r.loo; v[3] = r.w > 0.0 ? 1.0 : 0.0;
    }
    block_tree_256<4>(red, v);
    if (threadIdx.x == 0) {
        double *p = part + (int64_t)blockIdx.x * 4;
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}

// ... launch_fold_partials adds them in ascending block order from 0.0 into run[0 .. 3]; sigma2 = rss / (n+ - dof), NaN when n+ - dof <= 0,
// is formed from these where it is used, on the device and on the host: the same two operations on the same doubles
__host__ __device__ inline double diag_sigma2(const double *run)
{
    const double df = run[3] - run[0];
    return df > 0.0 ? run[1] / df : __builtin_nan("");
}

// (c) the one elementwise kernel: every per-row output that is wanted (a NULL pointer: not wanted)
//   studentized = sqrt(w) e / sqrt(sigma2 (1 - h));  cooks = ((studentized studentized) h) / (dof (1 - h))
__global__ __launch_bounds__(256) void diag_rows_kernel(const double *__restrict__ y, const double *__restrict__ yhat, const double *__restrict__ w,
                                                        const double *__restrict__ q, int64_t N, const double *__restrict__ run,
                                                        double *__restrict__ lev, double *__restrict__ loo, double *__restrict__ stu,
                                                        double *__restrict__ cook, double *__restrict__ res)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const RowTerms r = row_terms(y, yhat, w, q, i);
    const double dof = run[0], sigma2 = diag_sigma2(run);
    const double om = 1.0 - r.h;
    const double st = (sqrt(r.w) * r.e) / sqrt(sigma2 * om);
    if (lev) lev[i] = r.h;
    if (loo) loo[i] = r.loo;
    if (stu) stu[i] = st;
    if (cook) cook[i] = ((st * st) * r.h) / (dof * om);
    if (res) res[i] = r.e;
}

template <class XT>
static hipError_t launch_leverage(const XT *X, int64_t N, int64_t ldX, const double *Tp, const int *idx, int nt, double *q, hipStream_t s)
{
    const dim3 grid((unsigned)((N + LV_ROWS - 1) / LV_ROWS)), block(64 * LV_WAVES);
    const int rpw = (nt + LV_WAVES - 1) / LV_WAVES;
    static_assert(LV_MAX_RPW == 8 && 16 * LV_WAVES * LV_MAX_RPW >= 1023, "one case per row-tile count up to p = 1023");
    switch (rpw) {
        case 1: hipLaunchKernelGGL((leverage_kernel<XT, 1>), grid, block, 0, s, X, N, ldX, Tp, idx, nt, q); break;
        case 2: hipLaunchKernelGGL((leverage_kernel<XT, 2>), grid, block, 0, s, X, N, ldX, Tp, idx, nt, q); break;
        case 3: hipLaunchKernelGGL((leverage_kernel<XT, 3>), grid, block, 0, s, X, N, ldX, Tp, idx, nt, q); break;
        case 4: hipLaunchKernelGGL((leverage_kernel<XT, 4>), grid, block, 0, s, X, N, ldX, Tp, idx, nt, q); break;
        case 5: hipLaunchKernelGGL((leverage_kernel<XT, 5>), grid, block, 0, s, X, N, ldX, Tp, idx, nt, q); break;
        case 6: hipLaunchKernelGGL((leverage_kernel<XT, 6>), grid, block, 0, s, X, N, ldX, Tp, idx, nt, q); break;
        case 7: hipLaunchKernelGGL((leverage_kernel<XT, 7>), grid, block, 0, s, X, N, ldX, Tp, idx, nt, q); break;
        case 8: hipLaunchKernelGGL((leverage_kernel<XT, 8>), grid, block, 0, s, X, N, ldX, Tp, idx, nt, q); break;
        default: return hipErrorInvalidValue;    // nt > 64: p > 1024, which check_common excludes
    }
    return hipGetLastError();
}

// T = L^-1 for the lower triangular L (both row-major, leading dimension p; T's upper triangle is left 0): row i is
// -(sum_{k < i} L[i][k] T[k][:]) / L[i][i] with 1 / L[i][i] on the diagonal, the sum taken in ascending k over contiguous rows
static void invert_lower(const double *L, int p, double *T)
{
    std::vector<double> s((size_t)p);
    for (int i = 0; i < p; ++i) {
        const double *Li = L + (size_t)i * p;
        std::fill(s.begin(), s.begin() + i, 0.0);
        for (int k = 0; k < i; ++k) {
            const double lik = Li[k];
            const double *Tk = T + (size_t)k * p;
            for (int j = 0; j <= k; ++j) s[(size_t)j] += lik * Tk[j];
        }
        double *Ti = T + (size_t)i * p;
        const double d = Li[i];
        for (int j = 0; j < i; ++j) Ti[j] = -s[(size_t)j] / d;
        Ti[i] = 1.0 / d;
    }
}

// diag(S Bm S) and g_k' S Bm S g_k / their eta = 0 forms, S = T'T (see partls_diag.h): uw[p], ub[K], both before the factor sigma2
static void se_units(const partls_ctx *c, const std::vector<int> &A, const double *T, bool want_w, bool want_b, std::vector<double> &uw,
                     std::vector<double> &ub)
{
    const int p = (int)A.size();
    const int64_t K = c->K;
    uw.assign((size_t)p, 0.0); ub.assign((size_t)K, 0.0);
    auto in_group = [&](int j, int64_t k) { return ((c->mask_aug[(size_t)A[(size_t)j]] >> k) & 1ULL) != 0; };
    if (c->eta == 0.0) {                                 // Cov = sigma2 S: column norms of T, and ||T g_k||^2
        if (want_w)
            for (int r = 0; r < p; ++r) {
                const double *Tr = T + (size_t)r * p;
                for (int j = 0; j <= r; ++j) uw[(size_t)j] += Tr[j] * Tr[j];
            }
        if (want_b)
            for (int64_t k = 0; k < K; ++k) {
                double s = 0.0;
                for (int r = 0; r < p; ++r) {
                    const double *Tr = T + (size_t)r * p;
                    double d = 0.0;
                    for (int j = 0; j <= r; ++j) if (in_group(j, k)) d += Tr[j];
                    s += d * d;
                }
                ub[(size_t)k] = s;
            }
        return;
    }
    std::vector<double> S((size_t)p * p, 0.0), Bm((size_t)p * p), tmp((size_t)p), z((size_t)p);
    for (int r = 0; r < p; ++r) {                        // S = T'T: rank-one updates by the rows of T, lower triangle, then mirrored
        const double *Tr = T + (size_t)r * p;
        for (int i = 0; i <= r; ++i) {
            const double tri = Tr[i];
            double *Si = &S[(size_t)i * p];
            for (int j = 0; j <= i; ++j) Si[j] += tri * Tr[j];
        }
    }
    for (int i = 0; i < p; ++i)
        for (int j = i + 1; j < p; ++j) S[(size_t)i * p + j] = S[(size_t)j * p + i];
    for (int i = 0; i < p; ++i) {
        const double *row = c->hG.data() + (size_t)A[(size_t)i] * c->ldg;
        for (int j = 0; j < p; ++j) Bm[(size_t)i * p + j] = row[A[(size_t)j]];
    }
    auto quad = [&](const double *zv) {                  // zv' Bm zv
        std::fill(tmp.begin(), tmp.end(), 0.0);
        for (int i = 0; i < p; ++i) {
            const double zi = zv[i];
            const double *Bi = &Bm[(size_t)i * p];
            for (int j = 0; j < p; ++j) tmp[(size_t)j] += zi * Bi[j];
        }
        double s = 0.0;
        for (int j = 0; j < p; ++j) s += tmp[(size_t)j] * zv[j];
        return s;
    };
    if (want_w)
        for (int m = 0; m < p; ++m) uw[(size_t)m] = quad(&S[(size_t)m * p]);
    if (want_b)
        for (int64_t k = 0; k < K; ++k) {
            std::fill(z.begin(), z.end(), 0.0);
            for (int j = 0; j < p; ++j)
                if (in_group(j, k)) {
                    const double *Sj = &S[(size_t)j * p];
                    for (int i = 0; i < p; ++i) z[(size_t)i] += Sj[i];
                }
            ub[(size_t)k] = quad(z.data());
        }
}

static partls_status diag_common(partls_ctx *c, const double *alpha, const double *beta, double t, double *leverage, double *loo,
                                 double *studentized, double *cooks, double *residual, double *se_w, double *se_beta, int32_t *active,
                                 double *summary)
{
    const char *who = "partls_diagnostics";
    const auto call0 = std::chrono::steady_clock::now();
    if (!c) { set_error("context is NULL"); return PARTLS_ERR_BAD_ARG; }
    if (!c->prepared) { set_error("%s: context not prepared", who); return PARTLS_ERR_STATE; }
    if (c->storage == XStorage::csr) { set_error("%s: a problem prepared from CSR is not supported", who); return PARTLS_ERR_UNSUPPORTED; }
    if (c->multi_rank || !c->peers.empty()) { set_error("%s: a context of a partls_multi is not supported", who); return PARTLS_ERR_UNSUPPORTED; }
    if (!alpha || !beta) { set_error("%s: alpha or beta is NULL", who); return PARTLS_ERR_BAD_ARG; }
    if (!leverage && !loo && !studentized && !cooks && !residual && !se_w && !se_beta && !active && !summary) {
        set_error("%s: no output wanted", who);
        return PARTLS_ERR_BAD_ARG;
    }
    const int64_t N = c->N, M = c->M, K = c->K;
    partls_status st = check_models(who, alpha, M, beta, K, &t, M, K, 1, /*many=*/false);
    if (st != PARTLS_OK) return st;

    // the weights the prediction applies (predict_weights: yhat is partls_predict's) and the model weights v that define the support
    std::vector<double> wp((size_t)M, 0.0), v((size_t)M + 1, 0.0);
    st = predict_weights(c->P.data(), M, K, M, alpha, beta, wp.data());
    if (st != PARTLS_OK) return st;
    std::vector<int> A;
    for (int64_t m = 0; m < M; ++m) {
        double s = 0.0;
        for (int64_t k = 0; k < K; ++k) if (c->P[(size_t)m + (size_t)k * M]) s += beta[k];
        v[(size_t)m] = alpha[m] * s;
        if (v[(size_t)m] != 0.0) A.push_back((int)m);
    }
    v[(size_t)M] = t;
    A.push_back((int)M);
    const int p = (int)A.size(), nt = (p + 15) / 16;

    // H on the support, its factor, T = L^-1 and the packed tiles
    const auto f0 = std::chrono::steady_clock::now();
    std::vector<double> Lc((size_t)p * p, 0.0), Tm((size_t)p * p, 0.0), hd((size_t)p);
    for (int i = 0; i < p; ++i) {
        for (int j = 0; j <= i; ++j) Lc[(size_t)i * p + j] = h_reg(c, A[(size_t)i], A[(size_t)j]);
        hd[(size_t)i] = Lc[(size_t)i * p + i];
    }
    bool spd = chol_rows(Lc.data(), p);
    for (int i = 0; i < p && spd; ++i) {                 // the sweep's dependence rule on the unit-diagonal scale (SweepParams::piv_eps)
        const double d = Lc[(size_t)i * p + i];
        spd = std::isfinite(d) && d * d > SWEEP_PIV_EPS * hd[(size_t)i];
    }
    if (!spd) {
        set_error("%s: the penalised normal matrix of the support (p = %d) is numerically singular: two active columns are dependent", who, p);
        return PARTLS_ERR_ILL_CONDITIONED;
    }
    invert_lower(Lc.data(), p, Tm.data());
    const size_t tdoubles = (size_t)nt * (nt + 1) / 2 * 256, ibytes = (size_t)nt * 16 * sizeof(int);
    std::vector<double> up(tdoubles + (size_t)M + (ibytes + sizeof(double) - 1) / sizeof(double), 0.0);   // [tiles | wp | idx]: one upload
    for (int R = 0; R < nt; ++R)
        for (int C = 0; C <= R; ++C) {
            double *tile = up.data() + ((size_t)R * (R + 1) / 2 + C) * 256;
            for (int ks = 0; ks < 4; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = R * 16 + (lane & 15), col = C * 16 + ks * 4 + (lane >> 4);
                    if (row < p && col <= row) tile[ks * 64 + lane] = Tm[(size_t)row * p + col];
                }
        }
    std::memcpy(up.data() + tdoubles, wp.data(), (size_t)M * sizeof(double));
    {
        std::vector<int> idx((size_t)nt * 16, -2);
        for (int k = 0; k < p; ++k) idx[(size_t)k] = A[(size_t)k] == (int)M ? -1 : A[(size_t)k];
        std::memcpy(up.data() + tdoubles + M, idx.data(), ibytes);
    }
    const double factor_ms = ms_since(f0);

    // device: yhat (the prediction pass of partls_predict), q, the sums, the per-row outputs
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    const bool host_rows = c->dX == c->ownX.p;           // the prepare uploaded host arrays: the per-row outputs are host arrays too
    double *rows_out[5] = {leverage, loo, studentized, cooks, residual};
    const int64_t blocks = (N + 255) / 256;
    PARTLS_HIP_CHECK(c->dgT.ensure(up.size() * sizeof(double)));
    PARTLS_HIP_CHECK(c->dgRow.ensure((size_t)N * (host_rows ? 7 : 2) * sizeof(double)));
    PARTLS_HIP_CHECK(c->dgSums.ensure((size_t)(4 + 4 * blocks) * sizeof(double)));
    Events<2> ev;                                        // around the leverage kernel
    PARTLS_HIP_CHECK(ev.create());
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->dgT.p, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double *dT = c->dgT.as<double>(), *dWp = dT + tdoubles;
    const int *dIdx = reinterpret_cast<const int *>(dWp + M);
    double *dYh = c->dgRow.as<double>(), *dQ = dYh + N, *dRun = c->dgSums.as<double>(), *dPart = dRun + 4;
    double *dev_out[5];
    for (int o = 0; o < 5; ++o) dev_out[o] = !rows_out[o] ? nullptr : (host_rows ? dQ + (int64_t)(o + 1) * N : rows_out[o]);
    PARTLS_HIP_CHECK(launch_residual(c->dX, N, M, c->ldX, nullptr, dWp, t, nullptr, 1024, dYh, c->stream, nullptr, c->x_f32));
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[0], c->stream));
    if (c->x_f32) PARTLS_HIP_CHECK(launch_leverage(static_cast<const float *>(c->dX), N, c->ldX, dT, dIdx, nt, dQ, c->stream));
    else PARTLS_HIP_CHECK(launch_leverage(static_cast<const double *>(c->dX), N, c->ldX, dT, dIdx, nt, dQ, c->stream));
    PARTLS_HIP_CHECK(hipEventRecord(ev.e[1], c->stream));
    PARTLS_HIP_CHECK(hipMemsetAsync(dRun, 0, 4 * sizeof(double), c->stream));                 // all bits zero: +0.0
    hipLaunchKernelGGL(diag_sums_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, c->dy, dYh, c->dw, dQ, N, dPart);
    PARTLS_HIP_CHECK(hipGetLastError());
    PARTLS_HIP_CHECK(launch_fold_partials(dPart, blocks, 4, dRun, c->stream));
    if (leverage || loo || studentized || cooks || residual) {
        hipLaunchKernelGGL(diag_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, c->dy, dYh, c->dw, dQ, N, dRun, dev_out[0],
                           dev_out[1], dev_out[2], dev_out[3], dev_out[4]);
        PARTLS_HIP_CHECK(hipGetLastError());
    }
    double run[4] = {0.0, 0.0, 0.0, 0.0};
    PARTLS_HIP_CHECK(hipMemcpyAsync(run, dRun, sizeof(run), hipMemcpyDeviceToHost, c->stream));

    // meanwhile, on the host: the standard errors before their factor sigma2, and the stationarity of the model on its support
    std::vector<double> uw, ub;
    if (se_w || se_beta) se_units(c, A, Tm.data(), se_w != nullptr, se_beta != nullptr, uw, ub);
    const double *G = c->hG.data();
    const int ldg = c->ldg;
    const double sw = G[(size_t)M * ldg + M], sy = G[(size_t)M * ldg + M + 1], yy = G[(size_t)(M + 1) * ldg + M + 1];
    double stationarity = 0.0;
    {
        long double gmax = 0.0L;
        double bmax = 0.0;
        for (int a = 0; a < p; ++a) {
            const int ma = A[(size_t)a];
            const double *row = G + (size_t)ma * ldg;
            long double g = (long double)row[M + 1];
            for (int b = 0; b < p; ++b) {
                const int mb = A[(size_t)b];
                g -= (long double)row[mb] * (long double)v[(size_t)mb];
                if (c->eta != 0.0)
                    g -= (long double)c->eta * (long double)__builtin_popcountll(c->mask_aug[(size_t)ma] & c->mask_aug[(size_t)mb]) * (long double)v[(size_t)mb];
            }
            if (fabsl(g) > gmax) gmax = fabsl(g);
            if (row[ma] > bmax) bmax = row[ma];
        }
        const double den = std::sqrt(yy > 0.0 ? yy : 0.0) * std::sqrt(bmax);
        stationarity = den > 0.0 ? (double)gmax / den : (gmax > 0.0L ? std::numeric_limits<double>::infinity() : 0.0);
    }

    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (host_rows)                                        // nothing has been written so far: every output follows the last possible refusal
        for (int o = 0; o < 5; ++o)
            if (rows_out[o]) PARTLS_HIP_CHECK(hipMemcpy(rows_out[o], dev_out[o], (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    float kms = 0.f;
    if (hipEventElapsedTime(&kms, ev.e[0], ev.e[1]) != hipSuccess) kms = 0.f;
    const double dof = run[0], rss = run[1], press = run[2], nplus = run[3], sigma2 = diag_sigma2(run);
    if (summary) {
        const double tss = yy - sy * sy / sw;
        summary[PARTLS_DIAG_NPLUS] = nplus; summary[PARTLS_DIAG_P] = (double)p; summary[PARTLS_DIAG_DOF] = dof;
        summary[PARTLS_DIAG_RSS] = rss; summary[PARTLS_DIAG_PRESS] = press; summary[PARTLS_DIAG_SIGMA2] = sigma2;
        summary[PARTLS_DIAG_TSS] = tss; summary[PARTLS_DIAG_R2] = 1.0 - rss / tss; summary[PARTLS_DIAG_R2_LOO] = 1.0 - press / tss;
        summary[PARTLS_DIAG_STATIONARITY] = stationarity;
    }
    if (se_w) {
        for (int64_t m = 0; m <= M; ++m) se_w[m] = 0.0;
        for (int j = 0; j < p; ++j) se_w[A[(size_t)j]] = std::sqrt(sigma2 * uw[(size_t)j]);
    }
    if (se_beta)
        for (int64_t k = 0; k < K; ++k) se_beta[k] = std::sqrt(sigma2 * ub[(size_t)k]);
    if (active) {
        for (int64_t m = 0; m <= M; ++m) active[m] = 0;
        for (int j = 0; j < p; ++j) active[A[(size_t)j]] = 1;
    }
    c->dg_ms[0] = (double)kms; c->dg_ms[1] = factor_ms; c->dg_ms[2] = ms_since(call0);
    return PARTLS_OK;
}

}  // namespace partls

using namespace partls;

extern "C" {

partls_status partls_diagnostics(partls_ctx *c, const double *alpha, const double *beta, double t, double *leverage, double *loo,
                                 double *studentized, double *cooks, double *residual, double *se_w, double *se_beta, int32_t *active,
                                 double *summary)
try {
    return diag_common(c, alpha, beta, t, leverage, loo, studentized, cooks, residual, se_w, se_beta, active, summary);
}
PARTLS_ABI_GUARD

partls_status partls_get_diagnostics_timing(const partls_ctx *c, double *kernel_ms, double *factor_ms, double *call_ms)
try {
    if (!c || !kernel_ms || !factor_ms || !call_ms) { set_error("partls_get_diagnostics_timing: bad argument"); return PARTLS_ERR_BAD_ARG; }
    *kernel_ms = c->dg_ms[0]; *factor_ms = c->dg_ms[1]; *call_ms = c->dg_ms[2];
    return PARTLS_OK;
}
PARTLS_ABI_GUARD

}
