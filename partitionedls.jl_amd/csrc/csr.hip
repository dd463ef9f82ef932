// csr.hip — the passes over a design matrix stored in CSR (partls_opt_prepare_csr, partls_predict_csr): validation,
// the column-ordered (CSC) copy, the augmented Gram products, the residual and X'r.  X is never densified: the Gram costs
// sum_i r_i^2 multiply-adds (r_i = nonzeros of row i), the data passes nnz.
//
// The contract of every other pass of the library holds: bitwise reproducible run to run, no floating-point atomics.  Every sum below
// has an order fixed by the data layout alone — which wave or workgroup runs first never enters:
//   * rows are dealt to waves in contiguous ranges (csr_rows_per_wave: a function of N); a wave walks its rows in order;
//   * the CSC copy is placed from per-wave, per-column counts scanned in wave order, so every column holds its rows ascending without
//     a sort and without placement atomics (the only atomics are integer ones: the validation's minima and the per-wave histograms);
//   * a column of the Gram is summed over the column's nonzeros in row order, a long column in fixed ranges of `seg` nonzeros whose
//     partial sums are added in range order;
//   * block reductions are trees over thread indices.
#include "common.h"

namespace partls {

namespace {
constexpr int CSR_WPB = 4;                              // waves per workgroup of the row-walking and the Gram kernels (256 threads)

__device__ __forceinline__ bool csr_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and Inf
}  // namespace

int64_t csr_rows_per_wave(int64_t N)
{
    int64_t r = (N + CSR_MAX_WAVES - 1) / CSR_MAX_WAVES;
    return r < 16 ? 16 : r;
}
int csr_row_waves(int64_t N) { const int64_t r = csr_rows_per_wave(N); return (int)((N + r - 1) / r); }

// ---------------------------------------------------------------------------------------------------------------------
// Validation (+ the per-wave column counts of the CSC copy, when wcnt != nullptr).  Wave g owns rows [g R, (g + 1) R); the lanes go
// across a row's nonzeros, so indices and values are read coalesced.  nnz is indptr[N] as the host read it; a row is touched only when
// 0 <= indptr[i] <= indptr[i + 1] <= nnz and it holds at most M entries (a strictly increasing row cannot hold more), so nothing outside
// [0, nnz) is ever read.  err[0] / err[1] / err[2]: the first row (minimum; integer atomics) with a bad indptr / a bad index / a
// non-finite value, CSR_NO_ROW when there is none.  The counts go through an LDS histogram per wave with integer LDS atomics (a row
// with duplicate indices is an error, but must not lose a count before it is reported) and are stored, not added: wcnt needs no zeroing.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * CSR_WPB) void csr_check_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                 const double *__restrict__ values, int64_t N, int M, int64_t nnz,
                                                                 int64_t R, unsigned long long *__restrict__ err,
                                                                 unsigned *__restrict__ wcnt)
{
    extern __shared__ unsigned csr_hist[];               // [CSR_WPB][M]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned *hist = csr_hist + (size_t)wave * M;
    const int64_t g = (int64_t)blockIdx.x * CSR_WPB + wave;
    if (wcnt) for (int m = lane; m < M; m += 64) hist[m] = 0u;
    const int64_t i0 = g * R, i1 = (i0 + R < N) ? i0 + R : N;
    unsigned long long bad_ptr = CSR_NO_ROW, bad_idx = CSR_NO_ROW, bad_val = CSR_NO_ROW;
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t a = indptr[i], b = indptr[i + 1];
        if (a < 0 || b < a || b > nnz) { if (bad_ptr == CSR_NO_ROW) bad_ptr = (unsigned long long)i; continue; }
        if (b - a > M) { if (bad_idx == CSR_NO_ROW) bad_idx = (unsigned long long)i; continue; }
        for (int64_t k = a + lane; k < b; k += 64) {
            const int c = indices[k];
            const bool in = c >= 0 && c < M;
            if (!in || (k > a && indices[k - 1] >= c)) { if (bad_idx == CSR_NO_ROW) bad_idx = (unsigned long long)i; }
            if (!csr_finite(values[k])) { if (bad_val == CSR_NO_ROW) bad_val = (unsigned long long)i; }
            if (wcnt && in) atomicAdd(&hist[c], 1u);
        }
    }
    if (bad_ptr != CSR_NO_ROW) atomicMin(&err[0], bad_ptr);
    if (bad_idx != CSR_NO_ROW) atomicMin(&err[1], bad_idx);
    if (bad_val != CSR_NO_ROW) atomicMin(&err[2], bad_val);
    if (wcnt && i0 < N) {
        __builtin_amdgcn_wave_barrier();
        for (int m = lane; m < M; m += 64) wcnt[(size_t)g * M + m] = hist[m];
    }
}

// Per column m (one thread each): wcnt[g][m] -> the exclusive prefix over the waves g (in place: where wave g's entries of column m begin
// inside the column) and cnt[m] = the column's total.
__global__ __launch_bounds__(256) void csr_wave_scan_kernel(unsigned *__restrict__ wcnt, int W, int M, unsigned long long *__restrict__ cnt)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    unsigned run = 0;
    for (int g = 0; g < W; ++g) {
        const unsigned v = wcnt[(size_t)g * M + m];
        wcnt[(size_t)g * M + m] = run;
        run += v;
    }
    cnt[m] = run;
}

// colptr[0 .. M] = exclusive scan of cnt[0 .. M) (one workgroup; M <= 1022: four columns per thread, one tree over the threads)
__global__ __launch_bounds__(256) void csr_colptr_kernel(const unsigned long long *__restrict__ cnt, int M, int64_t *__restrict__ colptr)
{
    __shared__ unsigned long long tot[256];
    const int t = threadIdx.x;
    unsigned long long v[4], s = 0;
    for (int u = 0; u < 4; ++u) { const int m = 4 * t + u; v[u] = m < M ? cnt[m] : 0ULL; s += v[u]; }
    tot[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // inclusive scan (Hillis-Steele; integers: any order is exact)
        const unsigned long long add = t >= off ? tot[t - off] : 0ULL;
        __syncthreads();
        tot[t] += add;
        __syncthreads();
    }
    unsigned long long run = tot[t] - s;
    for (int u = 0; u < 4; ++u) { const int m = 4 * t + u; if (m < M) colptr[m] = (int64_t)run; run += v[u]; }
    if (t == 255) colptr[M] = (int64_t)tot[255];
}

// Placement: wave g walks its rows in order once more; the lanes take a row's nonzeros (distinct columns: distinct LDS words) and each
// appends its entry at colptr[c] + (wave g's offset in column c) + (entries of column c the wave has placed so far).  Rows ascend inside
// a wave's range and the ranges ascend with g, so every column ends up in row order whichever wave runs first.
__global__ __launch_bounds__(64 * CSR_WPB) void csr_place_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                 const double *__restrict__ values, int64_t N, int M, int64_t R,
                                                                 const unsigned *__restrict__ wcnt, const int64_t *__restrict__ colptr,
                                                                 int32_t *__restrict__ crow, double *__restrict__ cval)
{
    extern __shared__ unsigned csr_hist[];               // [CSR_WPB][M]: entries of column m placed so far by this wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned *pos = csr_hist + (size_t)wave * M;
    const int64_t g = (int64_t)blockIdx.x * CSR_WPB + wave;
    const int64_t i0 = g * R, i1 = (i0 + R < N) ? i0 + R : N;
    if (i0 >= N) return;
    for (int m = lane; m < M; m += 64) pos[m] = wcnt[(size_t)g * M + m];
    __builtin_amdgcn_wave_barrier();
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t a = indptr[i], b = indptr[i + 1];
        for (int64_t k = a + lane; k < b; k += 64) {
            const int c = indices[k];
            const unsigned p = pos[c];
            pos[c] = p + 1u;
            const int64_t at = colptr[c] + (int64_t)p;
            crow[at] = (int32_t)i;
            cval[at] = values[k];
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// The 2 x 2 corner of the augmented Gram: corner[0..2] = sum_i w_i, sum_i w_i y_i, sum_i w_i y_i^2 (w = 1 without weights).  One
// workgroup, rows strided over its threads, one tree: a fixed order.
template <bool WT>
__global__ __launch_bounds__(256) void csr_corner_kernel(const double *__restrict__ y, const double *__restrict__ wt, int64_t N,
                                                         double *__restrict__ corner)
{
    __shared__ double red[3][256];
    double v[3] = {0.0, 0.0, 0.0};                      // sums of w, w y, w y^2
    for (int64_t i = threadIdx.x; i < N; i += 256) {
        const double yi = y[i];
        if constexpr (WT) { const double wi = wt[i], wy = wi * yi; v[0] += wi; v[1] += wy; v[2] = fma(wy, yi, v[2]); }
        else { v[0] += 1.0; v[1] += yi; v[2] = fma(yi, yi, v[2]); }
    }
    block_tree_256<3>(red, v);
    if (threadIdx.x == 0) { corner[0] = v[0]; corner[1] = v[1]; corner[2] = v[2]; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Gram (the hot path).  Work item (q, s) = one wave: column q of G, the nonzeros [colptr[q] + s seg, ... + seg) of column q in the CSC
// copy, i.e. in row order.  The wave keeps a dense accumulator of the column — acc[p], p <= q (the lower triangle; the mirror entry is
// the same number) — in LDS.  For each nonzero (i, v) of its range it adds (w_i) v x_ip for the nonzeros p <= q of CSR row i, lanes
// across p: distinct words within a step, and the steps of a wave reach the LDS in program order, so an entry is summed over the rows in
// ascending order.  The ones and y entries (X'1, X'y) are carried in registers, the same value in every lane.  The row heads
// (indptr, y, w) of 64 nonzeros are fetched by the 64 lanes at once and handed out by lane index.
// part[(s M + q)(M + 2) + p]: p <= q, p = M (ones), p = M + 1 (y).  Items beyond a column's last range write nothing (the reduction
// reads csr_parts(count, seg) of them).
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int csr_parts(int64_t count, int64_t seg) { return count > 0 ? (int)((count + seg - 1) / seg) : 1; }

template <bool WT>
__global__ __launch_bounds__(64 * CSR_WPB) void csr_gram_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                const double *__restrict__ values, const int64_t *__restrict__ colptr,
                                                                const int32_t *__restrict__ crow, const double *__restrict__ cval,
                                                                const double *__restrict__ y, const double *__restrict__ wt, int M,
                                                                int64_t seg, int S, double *__restrict__ part)
{
    extern __shared__ double csr_acc[];                  // [CSR_WPB][M]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *acc = csr_acc + (size_t)wave * M;
    const int64_t item = (int64_t)blockIdx.x * CSR_WPB + wave;
    // column-major over the items, heaviest triangle rows first: item -> (q = M - 1 - item / S, s = item % S)
    if (item >= (int64_t)M * S) return;
    const int q = M - 1 - (int)(item / S), s = (int)(item % S);
    const int64_t c0 = colptr[q], c1 = colptr[q + 1];
    if (s >= csr_parts(c1 - c0, seg)) return;
    const int64_t k0 = c0 + (int64_t)s * seg, k1 = (k0 + seg < c1) ? k0 + seg : c1;
    for (int p = lane; p <= q; p += 64) acc[p] = 0.0;
    __builtin_amdgcn_wave_barrier();
    double ones = 0.0, ysum = 0.0;
    for (int64_t base = k0; base < k1; base += 64) {
        const int64_t k = base + lane;
        const bool have = k < k1;
        const int64_t i = have ? (int64_t)crow[k] : 0;
        const double v = have ? cval[k] : 0.0;
        const int64_t a_l = have ? indptr[i] : 0;
        const int len_l = have ? (int)(indptr[i + 1] - a_l) : 0;
        const double y_l = have ? y[i] : 0.0;
        double wv_l = v;
        if constexpr (WT) wv_l = have ? wt[i] * v : 0.0;
        const int cnt = (int)((k1 - base < 64) ? k1 - base : 64);
        for (int j = 0; j < cnt; ++j) {
            const int64_t a = __shfl(a_l, j);
            const int len = __shfl(len_l, j);
            const double wv = __shfl(wv_l, j), yi = __shfl(y_l, j);
            for (int o = lane; o < len; o += 64) {
                const int p = indices[a + o];
                if (p > q) break;                       // sorted row: nothing of the lower triangle beyond
                acc[p] = fma(wv, values[a + o], acc[p]);
            }
            ones += wv;
            ysum = fma(wv, yi, ysum);
        }
    }
    double *out = part + ((size_t)s * M + q) * (size_t)(M + 2);
    for (int p = lane; p <= q; p += 64) out[p] = acc[p];
    if (lane == 0) { out[M] = ones; out[M + 1] = ysum; }
}

// G (ldg x ldg, full symmetric, zero beyond M + 1) from the partial columns: entry (i, j) of two features is column max(i, j)'s
// accumulator at min(i, j), its ranges added in range order; both mirror entries are computed by the same additions.
__global__ __launch_bounds__(256) void csr_gram_reduce_kernel(const double *__restrict__ part, const int64_t *__restrict__ colptr,
                                                              const double *__restrict__ corner, int M, int64_t seg, int ldg,
                                                              double *__restrict__ G)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ldg * ldg) return;
    const int i = idx / ldg, j = idx % ldg;
    double g = 0.0;
    if (i <= M + 1 && j <= M + 1) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        if (lo >= M) g = corner[(lo - M) + (hi - M)];    // (M, M) -> 0, (M, M + 1) -> 1, (M + 1, M + 1) -> 2
        else {
            const int q = hi < M ? hi : lo, p = hi < M ? lo : hi;          // column of the accumulator, entry inside it
            const int np = csr_parts(colptr[q + 1] - colptr[q], seg);
            for (int s = 0; s < np; ++s) g += part[((size_t)s * M + q) * (size_t)(M + 2) + p];
        }
    }
    G[idx] = g;
}

// ---------------------------------------------------------------------------------------------------------------------
// Residual / predict: the outputs and fold rules of residual_kernel (misc.hip).  One thread per row: yhat_i = (sum over the row's
// nonzeros in ascending column order of x_im w_m) + t — one fma chain, so an empty row gives exactly t; the weight vector is staged in
// LDS once per workgroup.  partial[b] = the workgroup's sum of (wt_i) r_i^2, a tree over its threads; the host adds the blocks in order.
// ---------------------------------------------------------------------------------------------------------------------
template <bool WT>
__global__ __launch_bounds__(256) void csr_residual_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                           const double *__restrict__ values, int64_t N, int M,
                                                           const double *__restrict__ y, const double *__restrict__ w, double t,
                                                           double *__restrict__ partial, double *__restrict__ yhat,
                                                           const double *__restrict__ wt)
{
    extern __shared__ double csr_sw[];
    for (int m = threadIdx.x; m < M; m += blockDim.x) csr_sw[m] = w[m];
    __syncthreads();
    double acc2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = indptr[i], b = indptr[i + 1];
        double s = 0.0;
        for (int64_t k = a; k < b; ++k) s = fma(values[k], csr_sw[indices[k]], s);
        const double p = s + t;
        if (yhat) yhat[i] = p;
        if (y) {
            const double r = p - y[i];
            if constexpr (WT) acc2 = fma(wt[i] * r, r, acc2);
            else acc2 = fma(r, r, acc2);
        }
    }
    __shared__ double red[256];
    acc2 = block_sum_256(red, acc2);
    if (threadIdx.x == 0 && partial) partial[blockIdx.x] = acc2;
}

// ---------------------------------------------------------------------------------------------------------------------
// X'r: the output of xtr_kernel (misc.hip), gpart[r (M + 1) + m], row slices r of xtr_slices(N) added in slice order by the caller.
// Workgroup (m, r): the nonzeros of column m whose row lies in slice r — a contiguous stretch of the CSC column, found by two binary
// searches — strided over the threads, one tree.  Column M is the ones column: the (weighted) residual summed over the slice's rows.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t csr_lower_bound(const int32_t *__restrict__ rows, int64_t lo, int64_t hi, int64_t row)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)rows[mid] < row) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool WT>
__global__ __launch_bounds__(256) void csr_xtr_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ crow,
                                                      const double *__restrict__ cval, int64_t N, int M, const double *__restrict__ y,
                                                      const double *__restrict__ yhat, double *__restrict__ gpart, int R,
                                                      const double *__restrict__ wt)
{
    const int m = blockIdx.x, r = blockIdx.y;
    const int64_t rows = (N + R - 1) / R, r0 = (int64_t)r * rows, r1 = (r0 + rows < N) ? r0 + rows : N;
    double acc = 0.0;
    if (m < M) {
        const int64_t c0 = colptr[m], c1 = colptr[m + 1];
        const int64_t k0 = csr_lower_bound(crow, c0, c1, r0), k1 = csr_lower_bound(crow, k0, c1, r1);
        for (int64_t k = k0 + threadIdx.x; k < k1; k += 256) {
            const int64_t i = crow[k];
            double d = y[i] - yhat[i];
            if constexpr (WT) d = wt[i] * d;
            acc = fma(cval[k], d, acc);
        }
    } else {
        for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) {
            if constexpr (WT) acc += wt[i] * (y[i] - yhat[i]);
            else acc += y[i] - yhat[i];
        }
    }
    __shared__ double red[256];
    const double g = block_sum_256(red, acc);
    if (threadIdx.x == 0) gpart[(size_t)r * (M + 1) + m] = g;
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_csr_check(const CsrView &A, int64_t nnz, unsigned long long *err, unsigned *wcnt, hipStream_t s)
{
    const int64_t R = csr_rows_per_wave(A.N);
    const int W = csr_row_waves(A.N);
    hipError_t e = hipMemsetAsync(err, 0xff, 3 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(csr_check_kernel, dim3((W + CSR_WPB - 1) / CSR_WPB), dim3(64 * CSR_WPB), (size_t)CSR_WPB * A.M * sizeof(unsigned), s,
                       A.indptr, A.indices, A.values, A.N, (int)A.M, nnz, R, err, wcnt);
    return hipGetLastError();
}

hipError_t launch_csr_colptr(const CsrView &A, unsigned *wcnt, unsigned long long *cnt, int64_t *colptr, hipStream_t s)
{
    const int W = csr_row_waves(A.N), M = (int)A.M;
    hipLaunchKernelGGL(csr_wave_scan_kernel, dim3((M + 63) / 64), dim3(64), 0, s, wcnt, W, M, cnt);
    hipLaunchKernelGGL(csr_colptr_kernel, dim3(1), dim3(256), 0, s, cnt, M, colptr);
    return hipGetLastError();
}

hipError_t launch_csr_place(const CsrView &A, const unsigned *wcnt, const int64_t *colptr, int32_t *crow, double *cval, hipStream_t s)
{
    const int64_t R = csr_rows_per_wave(A.N);
    const int W = csr_row_waves(A.N), M = (int)A.M;
    hipLaunchKernelGGL(csr_place_kernel, dim3((W + CSR_WPB - 1) / CSR_WPB), dim3(64 * CSR_WPB), (size_t)CSR_WPB * M * sizeof(unsigned), s,
                       A.indptr, A.indices, A.values, A.N, M, R, wcnt, colptr, crow, cval);
    return hipGetLastError();
}

// seg: nonzeros of a column one wave sums — at least 256, and large enough that the longest column has at most csr_max_parts(M) ranges
// (which bounds the partial columns, S M (M + 2) doubles, to about 128 MB).  A function of the data alone.
static int csr_max_parts(int64_t M) { const int64_t s = 16384 / M; return (int)(s < 16 ? 16 : (s > 64 ? 64 : s)); }
void csr_gram_plan(int64_t M, int64_t longest, int64_t *seg_out, int *S_out)
{
    const int smax = csr_max_parts(M);
    int64_t seg = (longest + smax - 1) / smax;
    if (seg < 256) seg = 256;
    *seg_out = seg;
    *S_out = csr_parts(longest, seg);
}
size_t csr_gram_part_doubles(int64_t M, int S) { return (size_t)S * (size_t)M * (size_t)(M + 2); }

hipError_t launch_csr_gram(const CsrView &A, const CscView &T, const double *y, const double *wt, int64_t seg, int S, double *part,
                           double *corner, int ldg, double *G, hipStream_t s)
{
    const int M = (int)A.M;
    const int64_t items = (int64_t)M * S;
    const dim3 grid((unsigned)((items + CSR_WPB - 1) / CSR_WPB)), block(64 * CSR_WPB);
    const size_t lds = (size_t)CSR_WPB * M * sizeof(double);
    if (wt) {
        hipLaunchKernelGGL(csr_corner_kernel<true>, dim3(1), dim3(256), 0, s, y, wt, A.N, corner);
        hipLaunchKernelGGL(csr_gram_kernel<true>, grid, block, lds, s, A.indptr, A.indices, A.values, T.colptr, T.rows, T.values, y, wt, M, seg, S, part);
    } else {
        hipLaunchKernelGGL(csr_corner_kernel<false>, dim3(1), dim3(256), 0, s, y, wt, A.N, corner);
        hipLaunchKernelGGL(csr_gram_kernel<false>, grid, block, lds, s, A.indptr, A.indices, A.values, T.colptr, T.rows, T.values, y, wt, M, seg, S, part);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(csr_gram_reduce_kernel, dim3((ldg * ldg + 255) / 256), dim3(256), 0, s, part, T.colptr, corner, M, seg, ldg, G);
    return hipGetLastError();
}

hipError_t launch_csr_residual(const CsrView &A, const double *y, const double *w, double t, double *partial, int nblocks, double *yhat,
                               hipStream_t s, const double *wt)
{
    const size_t lds = (size_t)A.M * sizeof(double);
    if (wt && y)
        hipLaunchKernelGGL(csr_residual_kernel<true>, dim3(nblocks), dim3(256), lds, s, A.indptr, A.indices, A.values, A.N, (int)A.M, y, w, t,
                           partial, yhat, wt);
    else
        hipLaunchKernelGGL(csr_residual_kernel<false>, dim3(nblocks), dim3(256), lds, s, A.indptr, A.indices, A.values, A.N, (int)A.M, y, w, t,
                           partial, yhat, nullptr);
    return hipGetLastError();
}

hipError_t launch_csr_xtr(const CscView &T, int64_t N, int64_t M, const double *y, const double *yhat, double *gpart, hipStream_t s,
                          const double *wt)
{
    const int R = xtr_slices(N);
    const dim3 grid((unsigned)(M + 1), (unsigned)R);
    if (wt) hipLaunchKernelGGL(csr_xtr_kernel<true>, grid, dim3(256), 0, s, T.colptr, T.rows, T.values, N, (int)M, y, yhat, gpart, R, wt);
    else hipLaunchKernelGGL(csr_xtr_kernel<false>, grid, dim3(256), 0, s, T.colptr, T.rows, T.values, N, (int)M, y, yhat, gpart, R, wt);
    return hipGetLastError();
}

}  // namespace partls
