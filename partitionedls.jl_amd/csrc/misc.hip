// misc.hip — the small kernels either side of the sweep: synthetic inputs, tableau preparation, residual from the data.
#include "sweep_rules.h"
#include "prepare_rules.h"

namespace partls {

// (block_sum_256, the fixed-order block sum of the 256-thread kernels below: common.h)

// Prediction of row i of column-major X (widened as it is loaded) under the weights sw[0..M) and intercept t: four chains over m mod 4,
// ((a0 + a1) + (a2 + a3)) + t — the one order in which a row is predicted, so that a model's residual and its out-of-bag error agree
// bit for bit on a row.  residual_kernel keeps a hand-written copy (see there).
template <class XT>
__device__ __forceinline__ double row_predict(const XT *X, int64_t i, int64_t M, int64_t ldX, const double *sw, double t)
{
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t m = 0;
    for (; m + 3 < M; m += 4) {
        a0 = fma((double)X[i + m * ldX], sw[m], a0);
        a1 = fma((double)X[i + (m + 1) * ldX], sw[m + 1], a1);
        a2 = fma((double)X[i + (m + 2) * ldX], sw[m + 2], a2);
        a3 = fma((double)X[i + (m + 3) * ldX], sw[m + 3], a3);
    }
    for (; m < M; ++m) a0 = fma((double)X[i + m * ldX], sw[m], a0);
    return ((a0 + a1) + (a2 + a3)) + t;
}

// ---------------------------------------------------------------------------------------------------------------------
// Synthetic inputs: integer-exact counter-based generator — the device twin of oracle_synth().
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ static inline uint64_t sm64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__host__ __device__ static inline uint64_t rnd64_hd(uint64_t seed, uint64_t stream, uint64_t idx)
{
    return sm64(sm64(seed ^ (stream * 0xD6E8FEB86659FD93ULL)) + idx);
}
uint64_t rnd64(uint64_t seed, uint64_t stream, uint64_t idx) { return rnd64_hd(seed, stream, idx); }

__device__ static inline double gauss12(uint64_t seed, uint64_t stream, uint64_t idx)
{
    uint64_t s = 0;
#pragma unroll
    for (uint64_t r = 0; r < 3; ++r) {
        const uint64_t h = rnd64_hd(seed, stream, idx * 3 + r);
        s += (h & 0xFFFF) + ((h >> 16) & 0xFFFF) + ((h >> 32) & 0xFFFF) + (h >> 48);
    }
    return ((double)(int64_t)s - 393210.0) * 0x1.0p-16;
}

__global__ void synth_x_kernel(uint64_t seed, int64_t total, double *__restrict__ X)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        X[i] = gauss12(seed, 1, (uint64_t)i);
}

__global__ void synth_y_kernel(uint64_t seed, int64_t N, int64_t D, const double *__restrict__ X,
                               const double *__restrict__ wstar, double *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double acc = 0.0;
    for (int64_t j = 0; j < D; ++j) acc = fma(X[i + j * N], wstar[j], acc);      // same order as oracle_synth
    y[i] = fma(0.1, gauss12(seed, 4, (uint64_t)i), acc + 1.0);
}

hipError_t launch_synth(uint64_t seed, int64_t N, int64_t D, const double *wstar_dev, double *X, double *y, hipStream_t s)
{
    const int64_t total = N * D;
    int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(synth_x_kernel, dim3(blocks), dim3(256), 0, s, seed, total, X);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(synth_y_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, seed, N, D, X, wstar_dev, y);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Tableau preparation.  Input: G_aug ((M+2)^2, variables [features, intercept, y]).
//   1. regularisation, PartitionedLS.jl:108-123 in Gram form: G[a][b] += eta * #(groups containing both a and b)
//      (the K' extra rows sqrt(eta)*1_{group k}; y is padded with zeros so c and yy are unchanged);
//   2. free-intercept mode: eliminate the (always passive) intercept by a Schur complement;
//   3. scale to unit diagonal, s_i = 1/sqrt(B_ii) (sign constraints are invariant under positive scaling);
//   4. emit the full symmetric tableau  T = [[B~, c~], [c~', yy]]  ((n+1)^2, ld = n+1).
// ---------------------------------------------------------------------------------------------------------------------
__device__ static inline double reg_entry(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, int a, int b)
{
    double v = G[(size_t)a * ldg + b];
    if (eta != 0.0 && a <= M && b <= M) v += eta * (double)__popcll(mask_aug[a] & mask_aug[b]);
    return v;
}

__device__ static inline double base_entry(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug,
                                           int free_intercept, const int *perm, int n, int i, int j)
{
    // tableau index -> augmented Gram index: variables perm[0..n-1] (grouped by partition) then the rhs (y) at index n
    const int a = (i < n) ? perm[i] : M + 1, b = (j < n) ? perm[j] : M + 1;
    double v = reg_entry(G, ldg, M, eta, mask_aug, a, b);
    if (free_intercept) {
        const double gII = reg_entry(G, ldg, M, eta, mask_aug, M, M);
        v -= reg_entry(G, ldg, M, eta, mask_aug, a, M) * reg_entry(G, ldg, M, eta, mask_aug, M, b) / gII;
    }
    return v;
}

// The two steps, one entry per thread: the bodies of the single kernels and of the batched ones alike.  The tableau reads the scale.
__device__ __forceinline__ void prep_scale_entry(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, int free_intercept,
                                                 const int *perm, int n, double *scale)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = base_entry(G, ldg, M, eta, mask_aug, free_intercept, perm, n, i, i);
    const double ref = G[(size_t)perm[i] * ldg + perm[i]];
    scale[i] = column_is_live(d, ref) ? 1.0 / sqrt(d) : 0.0;
}

__device__ __forceinline__ void prep_tableau_entry(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, int free_intercept,
                                                   const int *perm, int n, const double *scale, double *Tfull)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int ld = n + 1;
    if (idx >= ld * ld) return;
    const int i = idx / ld, j = idx % ld;
    const double si = (i < n) ? scale[i] : 1.0, sj = (j < n) ? scale[j] : 1.0;
    double v = base_entry(G, ldg, M, eta, mask_aug, free_intercept, perm, n, i, j) * si * sj;
    if (i == j && i < n && si == 0.0) v = 1.0;          // dead variable: harmless unit pivot, never selected
    Tfull[idx] = v;
}

// One problem: G and eta as passed (eta is a kernel argument: the single prepare pays no copy for it; a C2 fit is 0.58 ms end to end).
__global__ void prep_scale_kernel(const double *__restrict__ G, int ldg, int M, double eta, const uint64_t *__restrict__ mask_aug,
                                  int free_intercept, const int *__restrict__ perm, int n, double *__restrict__ scale)
{
    prep_scale_entry(G, ldg, M, eta, mask_aug, free_intercept, perm, n, scale);
}

__global__ void prep_tableau_kernel(const double *__restrict__ G, int ldg, int M, double eta, const uint64_t *__restrict__ mask_aug, int free_intercept,
                                    const int *__restrict__ perm, int n, const double *__restrict__ scale, double *__restrict__ Tfull)
{
    prep_tableau_entry(G, ldg, M, eta, mask_aug, free_intercept, perm, n, scale, Tfull);
}

hipError_t launch_prep(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, int free_intercept,
                       const int *perm, double *scale, double *Tfull, int n, hipStream_t s)
{
    hipLaunchKernelGGL(prep_scale_kernel, dim3((n + 255) / 256), dim3(256), 0, s, G, ldg, M, eta, mask_aug,
                       free_intercept, perm, n, scale);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int tot = (n + 1) * (n + 1);
    hipLaunchKernelGGL(prep_tableau_kernel, dim3((tot + 255) / 256), dim3(256), 0, s, G, ldg, M, eta, mask_aug,
                       free_intercept, perm, n, scale, Tfull);
    return hipGetLastError();
}

// Batched: problem q = q0 + blockIdx.y reads the Gram G + (q / E) * gstride with eta[q % E] and writes slot blockIdx.y of the outputs;
// the scale step also writes the problem's tolerance from its own y'y (problem_tol, the host's rule).
__global__ void prep_scale_batch_kernel(const double *__restrict__ G, int64_t gstride, int E, int64_t q0, const double *__restrict__ eta, int ldg, int M,
                                        const uint64_t *__restrict__ mask_aug, int free_intercept, const int *__restrict__ perm, int n,
                                        double tol_rel, double *__restrict__ scale, double *__restrict__ tol)
{
    const int64_t qq = q0 + blockIdx.y;
    const double *Gq = G + (qq / E) * gstride;
    if (blockIdx.x == 0 && threadIdx.x == 0) tol[blockIdx.y] = problem_tol(tol_rel, Gq[(size_t)(M + 1) * ldg + (M + 1)]);
    prep_scale_entry(Gq, ldg, M, eta[qq % E], mask_aug, free_intercept, perm, n, scale + (int64_t)blockIdx.y * n);
}

__global__ void prep_tableau_batch_kernel(const double *__restrict__ G, int64_t gstride, int E, int64_t q0, const double *__restrict__ eta, int ldg,
                                          int M, const uint64_t *__restrict__ mask_aug, int free_intercept, const int *__restrict__ perm,
                                          int n, const double *__restrict__ scale, double *__restrict__ Tfull)
{
    const int64_t qq = q0 + blockIdx.y;
    prep_tableau_entry(G + (qq / E) * gstride, ldg, M, eta[qq % E], mask_aug, free_intercept, perm, n, scale + (int64_t)blockIdx.y * n,
                       Tfull + (int64_t)blockIdx.y * (n + 1) * (n + 1));
}

hipError_t launch_prep_batch(const double *G, int64_t gstride, int E, int64_t q0, const double *eta, int ldg, int M, const uint64_t *mask_aug,
                             int free_intercept, const int *perm, double tol_rel, double *scale, double *Tfull, double *tol, int n,
                             int batch, hipStream_t s)
{
    if (batch < 1 || batch > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prep_scale_batch_kernel, dim3((n + 255) / 256, batch), dim3(256), 0, s, G, gstride, E, q0, eta, ldg, M, mask_aug,
                       free_intercept, perm, n, tol_rel, scale, tol);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int tot = (n + 1) * (n + 1);
    hipLaunchKernelGGL(prep_tableau_batch_kernel, dim3((tot + 255) / 256, batch), dim3(256), 0, s, G, gstride, E, q0, eta, ldg, M, mask_aug,
                       free_intercept, perm, n, scale, Tfull);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Bit-order calibration of the Opt sweep (api.hip: calibrate_bit_order).  Bit b of the Gray index flips in 2^-(b+1) of all
// transitions, so which group sits on which bit decides how many variables the sweep exchanges: measured on C3, the same 2^20
// subproblems cost 16.9 M pivots / 74.9 ms in one order and 13.5 M / 52.2 ms in another.  The flip cost of a group is measured,
// not guessed: chain c starts from a pseudo-random pattern and flips the groups of its segment one after the other.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ static inline uint64_t walk_base(int chain, int kbits)
{
    return sm64(0xB17C0DE5ULL + (uint64_t)chain) & ((kbits >= 64) ? ~0ULL : ((1ULL << kbits) - 1));
}
int walk_flipped_bit(int chain, int step, int kbits, int seg_len, int nseg)       // step >= 1 flips this group
{
    return ((chain % nseg) * seg_len + step - 1) % kbits;
}
// codes[(c * L + i) * n + v]: constraint of tableau variable v at step i of chain c (sign of its multiplier, Opt.jl:28-29)
__global__ void walk_codes_kernel(const uint64_t *__restrict__ mask, int n, int kbits, int L, int seg_len, int nseg,
                                  int8_t *__restrict__ codes)
{
    const int c = blockIdx.x / L, i = blockIdx.x - c * L;
    uint64_t pat = walk_base(c, kbits);
    for (int j = 1; j <= i; ++j) pat ^= 1ULL << (((c % nseg) * seg_len + j - 1) % kbits);
    for (int v = threadIdx.x; v < n; v += blockDim.x) {
        const int f = sign_of_var(mask[v], pat);
        codes[(size_t)blockIdx.x * n + v] = (int8_t)((f > 0) - (f < 0));
    }
}
hipError_t launch_walk_codes(const uint64_t *mask, int n, int kbits, int chains, int L, int seg_len, int nseg, int8_t *codes, hipStream_t s)
{
    hipLaunchKernelGGL(walk_codes_kernel, dim3(chains * L), dim3(256), 0, s, mask, n, kbits, L, seg_len, nseg, codes);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// BnB node batches (solvers.hip), both ends of a batch on the device so that only (pat, free) goes up and (bound, branch) comes back:
//   codes: constraint of tableau variable v in node i — its branched groups each contribute alpha >= 0 or <= 0 (the Sigma of
//          BnB.jl:120-121 accumulates them); none -> free (2), both kinds -> forced to 0 (BnB.jl:74-79);
//   nu:    lb = sqrt(objective^2) (BnB.jl:69-92) and branch = argmax_k nu_k, nu_k = sum_{i<j in group k} max(0, -w_i w_j) =
//          (sum of the positive w)(sum of the |negative w|) over the variables of group k (BnB.jl:42-57,107,117); only groups that
//          are still free can mix signs; -1 when every nu_k is 0: the relaxed solution is feasible (BnB.jl:109-115).
//          Lane k walks the variables in tableau order (fixed summation order: run-to-run reproducible).
// ---------------------------------------------------------------------------------------------------------------------
__global__ void bnb_codes_kernel(const uint64_t *__restrict__ mask_tab, int n, const uint64_t *__restrict__ pat,
                                 const uint64_t *__restrict__ free_, int8_t *__restrict__ codes)
{
    const uint64_t pt = pat[blockIdx.x], fr = free_[blockIdx.x];
    for (int v = threadIdx.x; v < n; v += blockDim.x) {
        const uint64_t br = mask_tab[v] & ~fr;
        const bool pos = (br & pt) != 0, neg = (br & ~pt) != 0;
        codes[(size_t)blockIdx.x * n + v] = (int8_t)(!br ? 2 : (pos && neg ? 0 : (pos ? 1 : -1)));
    }
}

// One workgroup of 256 threads per node: the unscaled solution and the group masks are staged in LDS by all threads (one coalesced
// pass), then lane k of wave 0 adds group k's positive and negative parts in VARIABLE ORDER from LDS — the summation order of round 3's
// kernel (bit-identical bounds and branching decisions), without its 257 dependent global-memory round trips per lane (43 us per
// batch whatever its size: a fifth of a 1024-node round once the snapshots stopped dominating it).
__global__ __launch_bounds__(256) void bnb_nu_kernel(const double *__restrict__ sol, const double *__restrict__ obj2, int n,
                                                     const double *__restrict__ scale, const uint64_t *__restrict__ mask_tab, int Kp,
                                                     const uint64_t *__restrict__ free_, double *__restrict__ lb, int *__restrict__ branch)
{
    __shared__ double sw[1024];
    __shared__ uint64_t sm[1024];
    __shared__ double nu[64];
    const int i = blockIdx.x, k = threadIdx.x;
    const uint64_t fr = free_[i];
    const double *w = sol + (size_t)i * n;
    for (int v = threadIdx.x; v < n; v += 256) { sw[v] = w[v] * scale[v]; sm[v] = mask_tab[v]; }
    __syncthreads();
    if (k < 64) {
        double pos = 0.0, neg = 0.0;
        if (k < Kp && ((fr >> k) & 1ULL)) {
            for (int v = 0; v < n; ++v) {
                if (!((sm[v] >> k) & 1ULL)) continue;
                const double wv = sw[v];
                if (wv > 0.0) pos += wv; else neg -= wv;
            }
        }
        nu[k] = pos * neg;
    }
    __syncthreads();
    if (k == 0) {
        int kbest = -1;
        double nubest = 0.0;
        for (int g = 0; g < Kp; ++g) if (nu[g] > nubest) { nubest = nu[g]; kbest = g; }     // argmax: first maximal index
        const double o2 = obj2[i];
        lb[i] = sqrt(o2 > 0.0 ? o2 : 0.0);
        branch[i] = kbest;
    }
}

// Gershgorin radii of the scaled Gram block (unit diagonal): out[i] = sum_{j != i, j < n} |T[i][j]|.  max_i out[i] = r proves
// lambda_min >= 1 - r and lambda_max <= 1 + r for the matrix every solve of the prepared problem works on (solvers.hip: fit(Alt) skips
// its extra pass over X when that bound alone guarantees the Gram form's accuracy).
__global__ __launch_bounds__(256) void gersh_kernel(const double *__restrict__ T, int n, int ld, double *__restrict__ out)
{
    __shared__ double red[256];
    const int i = blockIdx.x;
    double s = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) if (j != i) s += fabs(T[(size_t)i * ld + j]);
    s = block_sum_256(red, s);
    if (threadIdx.x == 0) out[i] = s;
}
hipError_t launch_gersh(const double *Tfull, int n, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(gersh_kernel, dim3(n), dim3(256), 0, s, Tfull, n, n + 1, out);
    return hipGetLastError();
}

hipError_t launch_bnb_codes(const uint64_t *mask_tab, int n, const uint64_t *pat, const uint64_t *free_, int cnt, int8_t *codes, hipStream_t s)
{
    hipLaunchKernelGGL(bnb_codes_kernel, dim3(cnt), dim3(256), 0, s, mask_tab, n, pat, free_, codes);
    return hipGetLastError();
}
hipError_t launch_bnb_nu(const double *sol, const double *obj2, int n, const double *scale, const uint64_t *mask_tab, int Kp,
                         const uint64_t *free_, int cnt, double *lb, int *branch, hipStream_t s)
{
    hipLaunchKernelGGL(bnb_nu_kernel, dim3(cnt), dim3(256), 0, s, sol, obj2, n, scale, mask_tab, Kp, free_, lb, branch);
    return hipGetLastError();
}

// all_opt leaves the sweep indexed by the INTERNAL pattern (group k on bit gbit[k]); the boundary indexes it by the reference's
__global__ void pattern_gather_kernel(const double *__restrict__ in, int64_t npat, int kbits, BitOrder order, double *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // reference pattern
    if (r >= npat) return;
    uint64_t q = 0;
    for (int k = 0; k < kbits; ++k) q |= (((uint64_t)r >> k) & 1ULL) << order.gbit[k];
    out[r] = in[q];
}
hipError_t launch_pattern_gather(const double *in, int64_t npat, int kbits, const BitOrder &order, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(pattern_gather_kernel, dim3((unsigned)((npat + 255) / 256)), dim3(256), 0, s, in, npat, kbits, order, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// beta-step system of fit(Alt) in Gram form (Alt.jl:109-110):  H = A' Greg A,  g = A' c  with  A = Po o alpha  ((M+1) x K').
// Two tiny kernels with fixed summation orders (run-to-run reproducible, no atomics):
//   1. GA[m][k2] = sum_{m2 in group k2} Greg[m][m2] alpha_m2          (one workgroup per row m, lane = k2)
//   2. H[k][k2]  = sum_{m in group k} alpha_m GA[m][k2],   g[k] = sum_{m in group k} alpha_m Greg[m][y]
// On the host this was an M^2 loop per Alt iteration (0.3 ms at D = 512, a quarter of an iteration).
// ---------------------------------------------------------------------------------------------------------------------
// both kernels: lane = group index (K' <= 64), the 16 waves of the workgroup take the variables m = wave, wave + 16, ...; the 16
// partial sums of a lane are added in wave order by wave 0 (fixed order).  (One thread walking all M + 1 variables: 75 us per
// kernel at D = 512 — latency of 513 dependent steps.)
static constexpr int ALT_WAVES = 16;

// PP (partls_cv_alt): start blockIdx.y belongs to problem q = pp.q0 + pp.prob[blockIdx.y] of a batch and reads that
// problem's Gram G + (q / E) gstride with eta[q % E]; nothing else differs, and the PP = false instantiation ignores pp altogether.
struct AltProblemOf { const int *prob; int64_t q0, gstride; int E; const double *eta; };
#define ALT_PROBLEM_OPERANDS()                                                                                                        \
    if constexpr (PP) {                                                                                                               \
        const int64_t q = pp.q0 + pp.prob[blockIdx.y];                                                                                \
        G += (q / pp.E) * pp.gstride;                                                                                                 \
        eta = pp.eta[q % pp.E];                                                                                                       \
    }

template <bool PP>
__global__ __launch_bounds__(64 * ALT_WAVES) void alt_ga_kernel(const double *__restrict__ G, int ldg, int M, double eta,
                                                               const uint64_t *__restrict__ mask_aug, const double *__restrict__ a, int Kp,
                                                               double *__restrict__ GA, const int *__restrict__ slot, AltProblemOf pp)
{
    __shared__ double part[ALT_WAVES][64];
    const int m = blockIdx.x, k2 = threadIdx.x & 63, wave = threadIdx.x >> 6, Mp = M + 1;
    ALT_PROBLEM_OPERANDS()
    if (slot) { a += (size_t)slot[blockIdx.y] * Mp; GA += (size_t)blockIdx.y * Mp * Kp; }      // start blockIdx.y of a batch (see below)
    // branch-free and unrolled: the loads of a step are wave-uniform (row m of G, alpha and the mask of variable m2), eight steps
    // are in flight together; a lane adds the product when variable m2 belongs to ITS group
    const int wu = __builtin_amdgcn_readfirstlane(wave);
    double s = 0.0;
    int m2 = wu;
    for (; m2 + 7 * ALT_WAVES < Mp; m2 += 8 * ALT_WAVES) {
        double v[8];
        uint64_t mk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int mm = m2 + u * ALT_WAVES;
            mk[u] = mask_aug[mm];
            v[u] = reg_entry(G, ldg, M, eta, mask_aug, m, mm) * a[mm];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += ((mk[u] >> k2) & 1ULL) ? v[u] : 0.0;
    }
    for (; m2 < Mp; m2 += ALT_WAVES) s += ((mask_aug[m2] >> k2) & 1ULL) ? reg_entry(G, ldg, M, eta, mask_aug, m, m2) * a[m2] : 0.0;
    if (k2 >= Kp) s = 0.0;
    part[wave][k2] = s;
    __syncthreads();
    if (wave == 0 && k2 < Kp) {
        double t = 0.0;
        for (int w = 0; w < ALT_WAVES; ++w) t += part[w][k2];
        GA[(size_t)m * Kp + k2] = t;
    }
}

template <bool PP>
__global__ __launch_bounds__(64 * ALT_WAVES) void alt_h_kernel(const double *__restrict__ G, int ldg, int M, double eta,
                                                              const uint64_t *__restrict__ mask_aug, const double *__restrict__ a, int Kp,
                                                              const double *__restrict__ GA, double *__restrict__ Hg,
                                                              const int *__restrict__ slot, AltProblemOf pp)
{
    __shared__ double part[ALT_WAVES][65];
    ALT_PROBLEM_OPERANDS()
    if (slot) { a += (size_t)slot[blockIdx.y] * (M + 1); GA += (size_t)blockIdx.y * (M + 1) * Kp; Hg += (size_t)blockIdx.y * Kp * (Kp + 1); }
    const int k = blockIdx.x, k2 = threadIdx.x & 63, wave = threadIdx.x >> 6, Mp = M + 1;     // column Kp of row k holds g[k] (Kp <= 64: lane Kp <= 64 ... handled by lane 63 when Kp == 64)
    // lanes 0..Kp-1: H[k][k2]; the g column is computed by lane Kp when Kp < 64, else by a second pass of lane 0
    auto term = [&](int m, int col) { return col < Kp ? GA[(size_t)m * Kp + col] : reg_entry(G, ldg, M, eta, mask_aug, m, M + 1); };
    double s = 0.0, sg = 0.0;
    for (int m = wave; m < Mp; m += ALT_WAVES) {
        if (!((mask_aug[m] >> k) & 1ULL)) continue;
        const double am = a[m];
        if (k2 < Kp) s = fma(am, term(m, k2), s);
        if (k2 == 0) sg = fma(am, term(m, Kp), sg);
    }
    part[wave][k2] = s;
    if (k2 == 0) part[wave][64] = sg;
    __syncthreads();
    if (wave == 0) {
        if (k2 < Kp) {
            double t = 0.0;
            for (int w = 0; w < ALT_WAVES; ++w) t += part[w][k2];
            Hg[(size_t)k * (Kp + 1) + k2] = t;
        }
        if (k2 == 0) {
            double t = 0.0;
            for (int w = 0; w < ALT_WAVES; ++w) t += part[w][64];
            Hg[(size_t)k * (Kp + 1) + Kp] = t;
        }
    }
}

hipError_t launch_alt_beta_system(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, const double *a, int Kp,
                                  double *GA, double *Hg, hipStream_t s)
{
    hipLaunchKernelGGL(alt_ga_kernel<false>, dim3(M + 1), dim3(64 * ALT_WAVES), 0, s, G, ldg, M, eta, mask_aug, a, Kp, GA, (const int *)nullptr,
                       AltProblemOf{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(alt_h_kernel<false>, dim3(Kp), dim3(64 * ALT_WAVES), 0, s, G, ldg, M, eta, mask_aug, a, Kp, GA, Hg, (const int *)nullptr,
                       AltProblemOf{});
    return hipGetLastError();
}

// The same for `cnt` starts at once (partls_alt_multistart): start j of the batch = blockIdx.y reads alpha from a + slot[j] (M + 1) and
// writes GA + j (M + 1) Kp and Hg + j Kp (Kp + 1).  Every start is summed exactly as a single one is: same workgroup shape, same orders.
template <bool PP>
static hipError_t alt_beta_system_batch(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, const double *a, int Kp,
                                        const int *slot, int cnt, double *GA, double *Hg, AltProblemOf pp, hipStream_t s)
{
    for (int j0 = 0; j0 < cnt; j0 += 65535) {                     // gridDim.y <= 65535
        const int nb = cnt - j0 < 65535 ? cnt - j0 : 65535;
        double *ga = GA + (size_t)j0 * (M + 1) * Kp, *hg = Hg + (size_t)j0 * Kp * (Kp + 1);
        AltProblemOf pj = pp;
        if (PP) pj.prob += j0;
        hipLaunchKernelGGL(alt_ga_kernel<PP>, dim3(M + 1, nb), dim3(64 * ALT_WAVES), 0, s, G, ldg, M, eta, mask_aug, a, Kp, ga, slot + j0, pj);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(alt_h_kernel<PP>, dim3(Kp, nb), dim3(64 * ALT_WAVES), 0, s, G, ldg, M, eta, mask_aug, a, Kp, ga, hg, slot + j0, pj);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_alt_beta_system_batch(const double *G, int ldg, int M, double eta, const uint64_t *mask_aug, const double *a, int Kp,
                                        const int *slot, int cnt, double *GA, double *Hg, hipStream_t s)
{
    return alt_beta_system_batch<false>(G, ldg, M, eta, mask_aug, a, Kp, slot, cnt, GA, Hg, AltProblemOf{}, s);
}

// ... of starts that belong to different problems of a batch (partls_cv_alt): start j is of problem q0 + prob[j], which reads the Gram
// G + (q / E) gstride with eta[q % E] (device array)
hipError_t launch_alt_beta_system_problems(const double *G, int64_t gstride, int E, int64_t q0, const double *eta, const int *prob, int ldg,
                                           int M, const uint64_t *mask_aug, const double *a, int Kp, const int *slot, int cnt, double *GA,
                                           double *Hg, hipStream_t s)
{
    return alt_beta_system_batch<true>(G, ldg, M, 0.0, mask_aug, a, Kp, slot, cnt, GA, Hg, AltProblemOf{prob, q0, gstride, E, eta}, s);
}

// ---------------------------------------------------------------------------------------------------------------------
// Residual from the data (Opt.jl:90 / predict PartitionedLS.jl:132-134): one coalesced pass over column-major X.
//   partial[b] = sum over the block's rows of (sum_m X[i,m] w[m] + t - y[i])^2 ;  yhat (optional) = X w + t
// WT (sample weights): row i contributes wt[i] r_i^2, accumulated as fma(wt_i r_i, r_i, acc) — the unweighted order
// with one exact factor when wt_i = 1.
// Blocks are summed on the host in index order (reproducible).
// ---------------------------------------------------------------------------------------------------------------------
template <class XT, bool WT>
__global__ __launch_bounds__(256) void residual_kernel(const XT *__restrict__ X, int64_t N, int64_t M, int64_t ldX,
                                                       const double *__restrict__ y, const double *__restrict__ w, double t,
                                                       double *__restrict__ partial, double *__restrict__ yhat,
                                                       const double *__restrict__ wt)
{
    extern __shared__ double sw[];                       // w staged once per block
    for (int64_t m = threadIdx.x; m < M; m += blockDim.x) sw[m] = w[m];
    __syncthreads();
    double acc2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        // (row_predict), written out: through the helper this kernel — the data pass of C3 / C4 — is allocated one SGPR more (45 for 44;
        // the same instructions in another allocation, profiles/prepare_path_resource_usage.txt).  A change is made in both.
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int64_t m = 0;
        for (; m + 3 < M; m += 4) {
            a0 = fma((double)X[i + m * ldX], sw[m], a0);
            a1 = fma((double)X[i + (m + 1) * ldX], sw[m + 1], a1);
            a2 = fma((double)X[i + (m + 2) * ldX], sw[m + 2], a2);
            a3 = fma((double)X[i + (m + 3) * ldX], sw[m + 3], a3);
        }
        for (; m < M; ++m) a0 = fma((double)X[i + m * ldX], sw[m], a0);
        const double p = ((a0 + a1) + (a2 + a3)) + t;
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

template <class XT>
static void launch_residual_kernel(const XT *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w, double t,
                                   double *partial, int nblocks, double *yhat, hipStream_t s, const double *wt)
{
    if (wt && y)
        hipLaunchKernelGGL((residual_kernel<XT, true>), dim3(nblocks), dim3(256), (size_t)M * sizeof(double), s, X, N, M, ldX, y, w, t,
                           partial, yhat, wt);
    else
        hipLaunchKernelGGL((residual_kernel<XT, false>), dim3(nblocks), dim3(256), (size_t)M * sizeof(double), s, X, N, M, ldX, y, w, t,
                           partial, yhat, nullptr);
}

hipError_t launch_residual(const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *w, double t,
                           double *partial, int nblocks, double *yhat, hipStream_t s, const double *wt, bool x_f32)
{
    if (x_f32) launch_residual_kernel(static_cast<const float *>(X), N, M, ldX, y, w, t, partial, nblocks, yhat, s, wt);
    else launch_residual_kernel(static_cast<const double *>(X), N, M, ldX, y, w, t, partial, nblocks, yhat, s, wt);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// g = Xo' (y - yhat) for iterative refinement of one solution in data space (corrected semi-normal equations).
// Grid (column, row slice): workgroup (m, r) reduces rows [r0, r1) of column m (the last column is the ones column) with four
// loads of X in flight per thread, coalesced along the column, fixed-order block reduction; the XTR_R partial sums of a column are
// added in slice order by the caller (reproducible).  One workgroup per whole column (round 1) left each CU with a handful of loads
// in flight: 100 us for 205 MB at C3.
// WT (sample weights): the residual of row i enters as wt[i] (y_i - yhat_i), i.e. g = Xo' W (y - yhat).
// ---------------------------------------------------------------------------------------------------------------------
template <class XT, bool WT>
__global__ __launch_bounds__(256) void xtr_kernel(const XT *__restrict__ X, int64_t N, int64_t M, int64_t ldX,
                                                  const double *__restrict__ y, const double *__restrict__ yhat,
                                                  double *__restrict__ gpart, int R, const double *__restrict__ wt)
{
    const int64_t m = blockIdx.x;
    const int r = blockIdx.y;
    const int64_t rows = (N + R - 1) / R, r0 = (int64_t)r * rows, r1 = (r0 + rows < N) ? r0 + rows : N;
    const XT *col = X + m * ldX;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t i = r0 + threadIdx.x;
    if (m < M) {
        for (; i + 768 < r1; i += 1024) {
            XT x[4];
            double d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                x[u] = col[i + 256 * u];
                if constexpr (WT) d[u] = wt[i + 256 * u] * (y[i + 256 * u] - yhat[i + 256 * u]);
                else d[u] = y[i + 256 * u] - yhat[i + 256 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = fma((double)x[u], d[u], acc[u]);
        }
        if constexpr (WT) for (; i < r1; i += 256) acc[0] = fma((double)col[i], wt[i] * (y[i] - yhat[i]), acc[0]);
        else for (; i < r1; i += 256) acc[0] = fma((double)col[i], y[i] - yhat[i], acc[0]);
    } else {
        if constexpr (WT) for (; i < r1; i += 256) acc[0] += wt[i] * (y[i] - yhat[i]);
        else for (; i < r1; i += 256) acc[0] += y[i] - yhat[i];
    }
    __shared__ double red[256];
    const double g = block_sum_256(red, (acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (threadIdx.x == 0) gpart[(size_t)r * (M + 1) + m] = g;
}

int xtr_slices(int64_t N)
{
    int R = (int)((N + 16383) / 16384);
    if (R < 1) R = 1;
    if (R > 16) R = 16;
    return R;
}

template <class XT>
static void launch_xtr_kernel(const XT *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *yhat, double *gpart,
                              hipStream_t s, const double *wt)
{
    const int R = xtr_slices(N);
    if (wt) hipLaunchKernelGGL((xtr_kernel<XT, true>), dim3((unsigned)(M + 1), (unsigned)R), dim3(256), 0, s, X, N, M, ldX, y, yhat, gpart, R, wt);
    else hipLaunchKernelGGL((xtr_kernel<XT, false>), dim3((unsigned)(M + 1), (unsigned)R), dim3(256), 0, s, X, N, M, ldX, y, yhat, gpart, R, wt);
}

hipError_t launch_xtr(const void *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *yhat, double *gpart,
                      hipStream_t s, const double *wt, bool x_f32)
{
    if (x_f32) launch_xtr_kernel(static_cast<const float *>(X), N, M, ldX, y, yhat, gpart, s, wt);
    else launch_xtr_kernel(static_cast<const double *>(X), N, M, ldX, y, yhat, gpart, s, wt);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Sample weights: one pass over the columns of W (N x batch, leading dimension ldW) on the device, for host and
// device weights alike; a single weighted fit is the batch of one.  Column b = blockIdx.y -> column b of S = sqrt(W) (leading
// dimension N; what the Gram kernel stages; sqrt is correctly rounded, so sqrt(1) = 1 and sqrt(4) = 2 exactly) and, per block (b, x),
// four partials at part[4 (b gridDim.x + x) ..]:
//   [0] 1 if some w_i < 0,   [1] 1 if some w_i is NaN / Inf,   [2] the sum of the block's finite w_i,
//   [3] the number of rows whose weight is exactly 0 (the out-of-bag rows of a weighting; a count below 2^53 is exact in a double)
// (grid-stride rows, fixed-order trees over the block: a column's sum depends on N and the column alone).  The host folds a column's
// blocks in index order (fold_weight_partials, prepare_rules.h) and turns them into a status.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void weight_prep_kernel(const double *__restrict__ W, int64_t N, int64_t ldW, double *__restrict__ S,
                                                          double *__restrict__ part)
{
    __shared__ double red[4][256];
    const int64_t b = blockIdx.y;
    const double *w = W + b * ldW;
    double *s = S + b * N;
    double neg = 0.0, bad = 0.0, sum = 0.0, zero = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = w[i];
        const bool fin = isfinite(v);
        if (!fin) bad = 1.0;
        if (v < 0.0) neg = 1.0;
        if (v == 0.0) zero += 1.0;
        sum += fin ? v : 0.0;
        s[i] = (fin && v >= 0.0) ? sqrt(v) : 0.0;
    }
    double v[4] = {neg, bad, sum, zero};                // the two flags by max, the two sums by +: one tree
    block_tree_256<4, 0x3u>(red, v);
    if (threadIdx.x == 0) {
        double *p = part + 4 * (b * gridDim.x + blockIdx.x);
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}

int weight_prep_blocks(int64_t N)
{
    const int64_t b = (N + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

hipError_t launch_weightings_prep(const double *W, int64_t N, int64_t ldW, int batch, double *S, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(weight_prep_kernel, dim3(weight_prep_blocks(N), batch), dim3(256), 0, st, W, N, ldW, S, part);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Out-of-bag error of `batch` models at once (partls_opt_weightings): problem b = blockIdx.y has the model wv + b (M + 1) (features, then
// the intercept) and the weights W + b ldW; part[b gridDim.x + x] = sum over the block's rows i with W[i, b] == 0 of
// (sum_m X[i,m] w_m + t - y_i)^2, unweighted.  A row's prediction is residual_kernel's (row_predict), the rows of a block and its tree
// are fixed by N alone, and the host adds the blocks in index order: a problem's value does not depend on what else is in the batch.
// No atomics.  Every workgroup of a column reads the rows of X it owns once per problem; the problems of one launch share them through
// the caches.
// Dynamic LDS only: [tree (256) | model (M + 1)].
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void oob_sse_kernel(const double *__restrict__ X, int64_t N, int64_t M, int64_t ldX,
                                                      const double *__restrict__ y, const double *__restrict__ W, int64_t ldW,
                                                      const double *__restrict__ wv, double *__restrict__ part)
{
    extern __shared__ double oob_lds[];
    double *red = oob_lds, *sw = oob_lds + 256;
    const int64_t b = blockIdx.y;
    const double *wb = wv + b * (M + 1);
    for (int64_t m = threadIdx.x; m <= M; m += blockDim.x) sw[m] = wb[m];
    __syncthreads();
    const double t = sw[M];
    const double *wt = W + b * ldW;
    double acc2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        if (wt[i] != 0.0) continue;
        const double r = row_predict(X, i, M, ldX, sw, t) - y[i];
        acc2 = fma(r, r, acc2);
    }
    acc2 = block_sum_256(red, acc2);
    if (threadIdx.x == 0) part[b * gridDim.x + blockIdx.x] = acc2;
}

hipError_t launch_oob_sse(const double *X, int64_t N, int64_t M, int64_t ldX, const double *y, const double *W, int64_t ldW,
                          const double *wv, int batch, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(oob_sse_kernel, dim3(weight_prep_blocks(N), batch), dim3(256), (size_t)(256 + M + 1) * sizeof(double), st, X, N, M,
                       ldX, y, W, ldW, wv, part);
    return hipGetLastError();
}

}  // namespace partls
