// rescue.hip — patterns that hit the pivot cap of the sweeps, solved again by Lawson-Hanson on the device (PARTLS_OPT_RESCUE_CAPPED;
// DESIGN.md §4.14).
//
// Block principal pivoting with the largest-index backup (sweep_rules.h: ExchangeRule) is finite but no descent method: on designs
// that are correlated throughout it wanders until the cap of 20 (n + 1) rounds.  Lawson-Hanson lowers the objective at every main
// pass, and it runs as a pivoting rule on the same scaled tableau with the same rank-1 sweep (sweep_generic.hip's formula), so what it
// leaves is a basis of the sweeps' own kind: the rhs is the solution on the basic variables and the gradient on the others, the corner
// the objective^2, and "converged" is kkt_violates == false for every variable under the context's tol.
//
// One workgroup solves one subproblem from the fresh tableau Tfull and the empty basis, on a private copy in global scratch (the whole
// symmetric (n+1)^2 image, rows contiguous: the pivot ROW is what a step reads, coalesced, and keeps in LDS as the pivot column).  The
// grid is bounded (rescue_shape); workgroup b takes the entries b, b + grid, ... of a device list, so the scratch is grid tableaus
// whatever the list's length, which only the device knows (rescue_list_kernel compacts the NaN rows of an export piece).
//
// The rule (tests/rescue_reference.py states it in numpy).  q: the rhs, sgn: the sign the pattern asks of a variable, x: the last
// feasible iterate in the pattern's signs (LDS):
//     main pass:  candidates = non-basic, code != 0, not blocked, sgn q > tol;  none: converged
//                 k = the candidate of the largest sgn q (lowest index on ties)
//                 T[k][k] <= piv_eps: blocked += k, a veto, next main pass      (the sweeps' leave-one-out rule)
//                 pivot k in
//     inner loop: s = sgn q over the basic variables
//                 every s > 0: x = s, blocked cleared, next main pass
//                 alpha = min over the wrong-signed i of x_i / (x_i - s_i);  x += alpha (s - x)
//                 pivot out the minimiser and every basic i with x_i <= 0
// Main passes are bounded by max_passes (3 n, the oracle's itmax; PARTLS_RESCUE_MAX_PASSES); an inner iteration that does not end the
// loop removes at least the minimiser from a basis of at most n variables, and the loop is cut at n + 1 iterations besides.  A
// subproblem that runs out of main passes keeps its NaN row and counts as failed.
#include "ctx.h"
#include "sweep_rules.h"
#include <algorithm>
#include <cstring>

namespace partls {

static constexpr int RS_MAXTHREADS = 1024, RS_MAXWAVES = RS_MAXTHREADS / 64;
static constexpr int RS_NONE = 0x7fffffff;

struct RescueParams {
    int n;
    const uint64_t *mask;        // [n] group masks in the bit order of the patterns below
    const double *T0;            // Tfull: (n+1)^2, fresh
    double *scratch;             // [gridDim.x][(n+1)^2]
    double tol, piv_eps;
    int max_passes;
    const int64_t *list;         // entry e: gray ? the row of the piece (Gray index g0 + list[e]) : the pattern itself
    const unsigned *count;       // entries of the list (device)
    int64_t g0;
    int gray;
    double *rows;                // row r (leading dimension n): scaled solution, 0 for non-basic variables; r = gray ? list[e] : e
    double *obj;                 // [r] objective (sqrt of the corner); both untouched for a subproblem that fails
    unsigned long long *stats;   // [rescued | pivots | failed | vetoes], added to
};

// (value, index) maximum over the workgroup, the lowest index among equal values; every thread gets the result.  red_v / red_i: one
// slot per wave.  (-inf, RS_NONE) from every thread: nothing to pick.
__device__ __forceinline__ void rs_argmax(double &v, int &i, double *red_v, int *red_i, int tid, int nwaves)
{
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    __syncthreads();                                              // the slots' previous readers are done
    if ((tid & 63) == 0) { red_v[tid >> 6] = v; red_i[tid >> 6] = i; }
    __syncthreads();
    v = red_v[0]; i = red_i[0];
    for (int w = 1; w < nwaves; ++w) {
        const double ov = red_v[w];
        const int oi = red_i[w];
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// the symmetric rank-1 sweep on variable k (sweep_generic.hip: T_ij -= T_ik T_kj / d, T_ik = T_ik / |d|, T_kk = -1 / d; the same
// formula enters and removes), one wave per row.  col / wcol: the pivot row and the pivot row / d, in LDS.
__device__ __forceinline__ void rs_pivot(double *T, int ld, int k, double *col, double *wcol, int tid, int nthreads)
{
    const double d = T[(size_t)k * ld + k];
    const double inv = 1.0 / d, ainv = fabs(inv);
    __syncthreads();                                              // col / wcol: the previous step's readers are done
    for (int j = tid; j < ld; j += nthreads) {
        const double c = T[(size_t)k * ld + j];
        col[j] = c;
        wcol[j] = c * inv;
    }
    __syncthreads();
    // (a form with four rows of a wave in flight together was measured on the MI355X: 3.01 against 2.98 ms on the n = 176 design of
    // DESIGN.md §4.14, 4.84 against 4.67 ms at n = 297 — a step is bound by its chain of dependent round trips, not by this loop)
    const int lane = tid & 63, nwaves = nthreads >> 6;
    for (int i = tid >> 6; i < ld; i += nwaves) {
        double *row = T + (size_t)i * ld;
        if (i == k) {
            for (int j = lane; j < ld; j += 64) row[j] = (j == k) ? -inv : col[j] * ainv;
        } else {
            const double ci = col[i];
            for (int j = lane; j < ld; j += 64) row[j] = (j == k) ? ci * ainv : row[j] - ci * wcol[j];
        }
    }
    __threadfence_block();
    __syncthreads();
}

__global__ __launch_bounds__(RS_MAXTHREADS) void rescue_kernel(RescueParams p)
{
    const int n = p.n, ld = n + 1;
    const int tid = threadIdx.x, nthreads = blockDim.x, nwaves = nthreads >> 6;
    extern __shared__ double rs_smem[];
    double *col = rs_smem;                                        // [ld]
    double *wcol = col + ld;                                      // [ld]
    double *x = wcol + ld;                                        // [n]
    double *red_v = x + n;                                        // [RS_MAXWAVES]
    int *red_i = reinterpret_cast<int *>(red_v + RS_MAXWAVES);    // [RS_MAXWAVES]
    int8_t *s_code = reinterpret_cast<int8_t *>(red_i + RS_MAXWAVES);   // [n] -1 / 0 / +1
    uint8_t *s_basic = reinterpret_cast<uint8_t *>(s_code + n);   // [n]
    uint8_t *s_blocked = s_basic + n;                             // [n]
    uint8_t *s_out = s_blocked + n;                               // [n] leaves in this inner iteration

    double *T = p.scratch + (size_t)blockIdx.x * (size_t)ld * (size_t)ld;
    const double *q = T + (size_t)n * ld;                         // the rhs: row n of the symmetric image
    const unsigned cnt = *p.count;
    unsigned long long nresc = 0, npiv = 0, nfail = 0, nveto = 0;

    for (unsigned e = blockIdx.x; e < cnt; e += gridDim.x) {
        const int64_t le = p.list[e];
        const uint64_t g = (uint64_t)(p.g0 + le);
        const uint64_t pat = p.gray ? (g ^ (g >> 1)) : (uint64_t)le;
        const size_t row = p.gray ? (size_t)le : (size_t)e;
        __syncthreads();                                          // the previous subproblem's LDS state has been read
        for (int idx = tid; idx < ld * ld; idx += nthreads) T[idx] = p.T0[idx];
        for (int i = tid; i < n; i += nthreads) {
            const int f = sign_of_var(p.mask[i], pat);
            s_code[i] = (int8_t)((f > 0) - (f < 0));
            s_basic[i] = 0; s_blocked[i] = 0; s_out[i] = 0;
            x[i] = 0.0;
        }
        __threadfence_block();
        __syncthreads();

        int passes = 0;
        bool solved = false;
        for (;;) {
            // ---- main pass: the most violated multiplier
            double bv = -__builtin_inf();
            int bi = RS_NONE;
            for (int i = tid; i < n; i += nthreads) {
                const int c = s_code[i];
                if (s_basic[i] || c == 0 || s_blocked[i]) continue;
                const double v = (double)c * q[i];
                if (v > p.tol && v > bv) { bv = v; bi = i; }      // ascending i: the lowest index of the thread's maximum
            }
            rs_argmax(bv, bi, red_v, red_i, tid, nwaves);
            if (bi == RS_NONE) { solved = true; break; }
            if (passes >= p.max_passes) break;
            ++passes;
            const int k = bi;
            if (!(T[(size_t)k * ld + k] > p.piv_eps)) {           // dependent on the current basis: the leave-one-out rule
                __syncthreads();                                  // the scan's readers of s_blocked are done
                if (tid == 0) s_blocked[k] = 1;
                ++nveto;
                __syncthreads();
                continue;
            }
            rs_pivot(T, ld, k, col, wcol, tid, nthreads);
            ++npiv;
            if (tid == 0) { s_basic[k] = 1; x[k] = 0.0; }
            __syncthreads();
            // ---- inner loop: back to a feasible point, then on to the basis' own solution
            for (int it = 0; it <= n; ++it) {
                double rv = -__builtin_inf();                     // maximum of -ratio = minimum of the ratio
                int ri = RS_NONE;
                for (int i = tid; i < n; i += nthreads) {
                    if (!s_basic[i]) continue;
                    const double s = (double)s_code[i] * q[i];
                    if (s > 0.0) continue;
                    const double xi = x[i], den = xi - s;
                    const double r = den > 0.0 ? xi / den : 0.0;
                    if (-r > rv) { rv = -r; ri = i; }
                }
                rs_argmax(rv, ri, red_v, red_i, tid, nwaves);
                if (ri == RS_NONE) {                              // the basis' solution is feasible: it is the new iterate
                    for (int i = tid; i < n; i += nthreads) {
                        x[i] = s_basic[i] ? (double)s_code[i] * q[i] : 0.0;
                        s_blocked[i] = 0;
                    }
                    __syncthreads();
                    break;
                }
                const double alpha = -rv;
                for (int i = tid; i < n; i += nthreads) {
                    uint8_t out = 0;
                    if (s_basic[i]) {
                        const double s = (double)s_code[i] * q[i];
                        const double xn = x[i] + alpha * (s - x[i]);
                        x[i] = xn;
                        out = (xn <= 0.0 || i == ri) ? 1 : 0;
                    }
                    s_out[i] = out;
                }
                __syncthreads();
                for (int i = 0; i < n; ++i) {                     // ascending, workgroup-uniform
                    if (!s_out[i]) continue;
                    rs_pivot(T, ld, i, col, wcol, tid, nthreads);
                    ++npiv;
                    if (tid == 0) { s_basic[i] = 0; x[i] = 0.0; }
                }
                __syncthreads();
            }
        }
        if (solved) {
            const double o2 = T[(size_t)n * ld + n];
            for (int i = tid; i < n; i += nthreads) p.rows[row * (size_t)n + i] = s_basic[i] ? q[i] : 0.0;
            if (tid == 0) p.obj[row] = sqrt(o2 > 0.0 ? o2 : 0.0);
            ++nresc;
        } else {
            ++nfail;
        }
    }
    if (tid == 0) {
        if (nresc) atomicAdd(p.stats + 0, nresc);
        if (npiv) atomicAdd(p.stats + 1, npiv);
        if (nfail) atomicAdd(p.stats + 2, nfail);
        if (nveto) atomicAdd(p.stats + 3, nveto);
    }
}

// the rows of a piece whose objective is NaN (the export's mark of a capped pattern) -> list, in any order; *count: their number
__global__ __launch_bounds__(256) void rescue_list_kernel(const double *__restrict__ obj, int64_t cnt, int64_t *__restrict__ list, unsigned *count)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * 256) {
        const double o = obj[i];
        if (o != o) list[atomicAdd(count, 1u)] = i;
    }
}

// A few workgroups per CU, and never more than 256 MiB of tableaus: 1024 threads (16 waves: one row of the update each) from n = 128 on,
// 256 below.
static void rescue_shape(const partls_ctx *c, int64_t upper, int *grid, int *threads)
{
    const size_t ld = (size_t)c->n + 1;
    *threads = c->n >= 128 ? RS_MAXTHREADS : 256;
    int64_t g = (int64_t)c->ncu * (*threads == RS_MAXTHREADS ? 2 : 4);
    g = std::min<int64_t>(g, (int64_t)std::max<size_t>(1, ((size_t)256 << 20) / (ld * ld * sizeof(double))));
    g = std::min<int64_t>(g, upper);
    *grid = (int)std::max<int64_t>(1, g);
}

static int rescue_max_passes(const partls_ctx *c) { return c->knobs.rescue_max_passes >= 1 ? c->knobs.rescue_max_passes : 3 * c->n; }

// head of c->rescueList, 8-byte words: [count | rescued | pivots | failed | vetoes | - | - | -], then the list
static constexpr size_t RS_HEAD = 8;

static partls_status rescue_launch(partls_ctx *c, int64_t upper, const uint64_t *mask, int64_t g0, bool gray, double *rows, double *obj)
{
    int grid = 1, threads = 256;
    rescue_shape(c, upper, &grid, &threads);
    const size_t ld = (size_t)c->n + 1;
    PARTLS_HIP_CHECK(c->rescueScratch.ensure((size_t)grid * ld * ld * sizeof(double)));
    unsigned long long *head = c->rescueList.as<unsigned long long>();
    RescueParams p{};
    p.n = c->n; p.mask = mask; p.T0 = c->Tfull.as<double>(); p.scratch = c->rescueScratch.as<double>();
    p.tol = c->tol; p.piv_eps = SWEEP_PIV_EPS; p.max_passes = rescue_max_passes(c);
    p.list = reinterpret_cast<const int64_t *>(head + RS_HEAD); p.count = reinterpret_cast<const unsigned *>(head);
    p.g0 = g0; p.gray = gray ? 1 : 0;
    p.rows = rows; p.obj = obj; p.stats = head + 1;
    const size_t shmem = ((size_t)2 * ld + (size_t)c->n + RS_MAXWAVES) * sizeof(double) + RS_MAXWAVES * sizeof(int) + (size_t)4 * c->n + 16;
    t_begin(c, PARTLS_T_RESCUE);
    hipLaunchKernelGGL(rescue_kernel, dim3(grid), dim3(threads), shmem, c->stream, p);
    PARTLS_HIP_CHECK(hipGetLastError());
    t_end(c, PARTLS_T_RESCUE);
    return PARTLS_OK;
}

partls_status rescue_piece(partls_ctx *c, int64_t p0, int64_t cnt, double *rows, double *obj)
{
    PARTLS_HIP_CHECK(c->rescueList.ensure((RS_HEAD + (size_t)cnt) * 8));
    PARTLS_HIP_CHECK(c->rescueStage.resize(RS_HEAD));
    PARTLS_HIP_CHECK(hipMemsetAsync(c->rescueList.p, 0, RS_HEAD * 8, c->stream));
    unsigned long long *head = c->rescueList.as<unsigned long long>();
    const int lgrid = (int)std::min<int64_t>((cnt + 255) / 256, 1024);
    hipLaunchKernelGGL(rescue_list_kernel, dim3(lgrid), dim3(256), 0, c->stream, obj, cnt, reinterpret_cast<int64_t *>(head + RS_HEAD),
                       reinterpret_cast<unsigned *>(head));
    PARTLS_HIP_CHECK(hipGetLastError());
    // the export's patterns are Gray indices in the visiting order of the sweep: its masks (sweep_params)
    const SweepParams sp = sweep_params(c, /*internal_order=*/true);
    const partls_status st = rescue_launch(c, cnt, sp.mask, p0, true, rows, obj);
    if (st != PARTLS_OK) return st;
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->rescueStage.data(), c->rescueList.p, RS_HEAD * 8, hipMemcpyDeviceToHost, c->stream));
    return PARTLS_OK;
}

void rescue_begin_call(partls_ctx *c)
{
    c->rescue_rescued = c->rescue_pivots = c->rescue_failed = 0;
    c->ms[PARTLS_T_RESCUE] = 0.0;
}

// all_opt of a sweep's second pass: the objective of row i (Gray index p0 + i) to its entry, indexed by the internal pattern
__global__ __launch_bounds__(256) void rescue_all_opt_kernel(const double *__restrict__ obj, int64_t p0, int64_t cnt, double *__restrict__ all_opt)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * 256) {
        const uint64_t g = (uint64_t)(p0 + i);
        all_opt[g ^ (g >> 1)] = obj[i];
    }
}

partls_status rescue_all_opt(partls_ctx *c, const double *obj, int64_t p0, int64_t cnt, double *all_opt)
{
    const int grid = (int)std::min<int64_t>((cnt + 255) / 256, 1024);
    hipLaunchKernelGGL(rescue_all_opt_kernel, dim3(grid), dim3(256), 0, c->stream, obj, p0, cnt, all_opt);
    PARTLS_HIP_CHECK(hipGetLastError());
    return PARTLS_OK;
}

void rescue_collect(partls_ctx *c, unsigned long long *unconv, unsigned long long *vetoes)
{
    t_collect(c);
    unsigned long long h[RS_HEAD];
    std::memcpy(h, c->rescueStage.data(), sizeof(h));
    const unsigned long long listed = h[0] & 0xffffffffULL;
    c->rescue_rescued += h[1]; c->rescue_pivots += h[2]; c->rescue_failed += h[3];
    if (unconv) *unconv = (*unconv >= listed ? *unconv - listed : 0) + h[3];
    if (vetoes) *vetoes += h[4];
}

partls_status rescue_pattern(partls_ctx *c, uint64_t pattern, std::vector<double> &sol, double *obj2, unsigned long long *unconv)
{
    const int n = c->n;
    PARTLS_HIP_CHECK(c->rescueList.ensure((RS_HEAD + 1 + (size_t)n + 1) * 8));
    PARTLS_HIP_CHECK(c->rescueStage.resize(RS_HEAD + 1 + (size_t)n + 1));
    // [head | the pattern | row (n) | objective], the objective NaN until the kernel solves the pattern
    double *st = c->rescueStage.data();
    unsigned long long h[RS_HEAD] = {1, 0, 0, 0, 0, 0, 0, 0};
    std::memcpy(st, h, sizeof(h));
    const int64_t pat = (int64_t)pattern;
    std::memcpy(st + RS_HEAD, &pat, sizeof(pat));
    for (int i = 0; i <= n; ++i) st[RS_HEAD + 1 + i] = __builtin_nan("");
    const size_t words = RS_HEAD + 1 + (size_t)n + 1;
    PARTLS_HIP_CHECK(hipMemcpyAsync(c->rescueList.p, st, words * 8, hipMemcpyHostToDevice, c->stream));
    double *drow = c->rescueList.as<double>() + RS_HEAD + 1;
    const partls_status ls = rescue_launch(c, 1, c->maskTabP, 0, false, drow, drow + n);
    if (ls != PARTLS_OK) return ls;
    PARTLS_HIP_CHECK(hipMemcpyAsync(st, c->rescueList.p, words * 8, hipMemcpyDeviceToHost, c->stream));
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    t_collect(c);
    std::memcpy(h, st, sizeof(h));
    c->rescue_rescued += h[1]; c->rescue_pivots += h[2]; c->rescue_failed += h[3];
    c->last_pivots = h[2]; c->last_vetoes = h[4];
    sol.assign(st + RS_HEAD + 1, st + RS_HEAD + 1 + n);
    const double o = st[RS_HEAD + 1 + n];
    if (obj2) *obj2 = o * o;
    if (unconv) *unconv = h[3] ? 1 : 0;
    if (h[3]) sol.assign((size_t)n, 0.0);
    return PARTLS_OK;
}

}  // namespace partls
