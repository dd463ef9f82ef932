// alt_multi.hip — partls_alt_multistart: fit(Alt) from many starting points in one batched device call.
//
// Every start runs the iteration of partls_alt_prepared (solvers.hip) — alpha-step, checkalpha, renormalisation, beta-step, loss,
// stop rule — but all active starts of a chunk advance together and their state stays in HBM:
//   codes    f = Po beta, sign(f) in tableau order straight into the node-code buffer               (alt_multi_codes_kernel)
//   alpha    the sweep kernels in node mode, one node per start, from the fresh tableau            (solve_nodes_device, sweep_setup.hip)
//   alpha    unscale, alpha = max(w / f, 0), checkalpha, renormalise, beta o= sum alpha            (alt_multi_alpha_kernel)
//   beta     H = A'G_reg A, g = A'c per start                                                      (launch_alt_beta_system_batch, misc.hip)
//   beta     Gaussian elimination in LDS, loss, stop rule, one record per start                    (alt_multi_beta_kernel)
// The host reads one block of records per iteration (one copy, one synchronisation for the whole chunk) and builds the next active
// list from it.  A start's arithmetic touches only its own rows and is summed in fixed orders (no atomics on values): its result
// does not depend on the batch, its position or the chunking, bit for bit.
#include "ctx.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

using namespace partls;

namespace {

// state of a chunk in HBM, one row per slot (slot s of the chunk = start r0 + s)
struct AltMultiState {
    int n, Mp, Kp;
    double *a;             // [C x Mp]   alpha over [features, intercept]
    double *b;             // [C x Kp]   beta
    double *wv;            // [C x Mp]   raw solution w = f o alpha of the last alpha-step
    double *hdiag;         // [C x Kp]   diag(H) of the last beta-step
    double *opt;           // [C x 2]    oldopt, optval
    int *iters;            // [C]        completed iterations
    int8_t *vcode;         // [C x Mp]   constraint codes of the last alpha-step over [features, intercept]
    const uint64_t *mask_aug;
    const int *perm;
    const double *scale;
};

// what the host reads per active start and iteration
struct AltMultiRec { double optval; int32_t cont; int32_t status; };

// One workgroup per active start: f_m = sum_k Po[m,k] beta_k with k ascending as on the host (Alt.jl:80); the code of tableau variable v
// is the sign of f at perm[v] (0: zero multiplier, the variable stays out of the basis).
__global__ __launch_bounds__(256) void alt_multi_codes_kernel(AltMultiState st, const int *__restrict__ slot, int8_t *__restrict__ code)
{
    __shared__ double sb[64];
    const int s = slot[blockIdx.x];
    if ((int)threadIdx.x < st.Kp) sb[threadIdx.x] = st.b[(size_t)s * st.Kp + threadIdx.x];
    __syncthreads();
    for (int v = threadIdx.x; v < st.n; v += 256) {
        const int m = st.perm[v];
        double f = 0.0;
        for (uint64_t bits = st.mask_aug[m]; bits; bits &= bits - 1) f += sb[__builtin_ctzll(bits)];
        const int8_t cd = (int8_t)((f > 0.0) - (f < 0.0));
        code[(size_t)blockIdx.x * st.n + v] = cd;
        st.vcode[(size_t)s * st.Mp + m] = cd;
    }
}

// One workgroup per active start, the rest of the alpha-step (Alt.jl:86-98) in the order of the host loop of partls_alt_prepared:
// w[perm[i]] = sol[i] scale[i]; alpha = max(w / f, 0); checkalpha (a group whose alphas sum to exactly 0 becomes uniform, sums taken
// before any group is rewritten); alpha /= Po sum-alpha (a feature of no group stays 0); beta o= sum-alpha.  Lane k walks the variables
// in order for group k's sums (fixed summation order).
// PP (partls_cv_alt): the start belongs to problem prob[blockIdx.x] of a batch and st.scale holds one row of n per problem.
template <bool PP>
__global__ __launch_bounds__(256) void alt_multi_alpha_kernel(AltMultiState st, const int *__restrict__ slot, const double *__restrict__ sol,
                                                              const int *__restrict__ prob)
{
    __shared__ double sw[1024], sa[1024];
    __shared__ uint64_t sm[1024];
    __shared__ double sb[64], ssum[64];
    __shared__ int scnt[64];
    const int s = slot[blockIdx.x], Mp = st.Mp, Kp = st.Kp, tid = threadIdx.x;
    const double *x = sol + (size_t)blockIdx.x * st.n;
    const double *scale = st.scale;
    if constexpr (PP) scale += (size_t)prob[blockIdx.x] * st.n;
    for (int m = tid; m < Mp; m += 256) { sw[m] = 0.0; sm[m] = st.mask_aug[m]; }
    if (tid < Kp) sb[tid] = st.b[(size_t)s * Kp + tid];
    __syncthreads();
    for (int i = tid; i < st.n; i += 256) sw[st.perm[i]] = x[i] * scale[i];
    __syncthreads();
    for (int m = tid; m < Mp; m += 256) {
        double f = 0.0;
        for (uint64_t bits = sm[m]; bits; bits &= bits - 1) f += sb[__builtin_ctzll(bits)];
        const double am = (f != 0.0) ? sw[m] / f : 0.0;
        sa[m] = am > 0.0 ? am : 0.0;
        st.wv[(size_t)s * Mp + m] = sw[m];
    }
    __syncthreads();
    if (tid < Kp) {
        double t = 0.0;
        int cnt = 0;
        for (int m = 0; m < Mp; ++m) if ((sm[m] >> tid) & 1ULL) { t += sa[m]; ++cnt; }
        ssum[tid] = t; scnt[tid] = cnt;
    }
    __syncthreads();
    for (int m = tid; m < Mp; m += 256) {                      // checkalpha: the last empty group of a variable decides, as in the host's loop over k
        double am = sa[m];
        for (uint64_t bits = sm[m]; bits; bits &= bits - 1) {
            const int k = __builtin_ctzll(bits);
            if (ssum[k] == 0.0) am = 1.0 / (double)scnt[k];
        }
        sa[m] = am;
    }
    __syncthreads();
    if (tid < Kp) {
        double t = 0.0;
        for (int m = 0; m < Mp; ++m) if ((sm[m] >> tid) & 1ULL) t += sa[m];
        ssum[tid] = t;
    }
    __syncthreads();
    for (int m = tid; m < Mp; m += 256) {
        double poa = 0.0;
        for (uint64_t bits = sm[m]; bits; bits &= bits - 1) poa += ssum[__builtin_ctzll(bits)];
        st.a[(size_t)s * Mp + m] = sm[m] ? sa[m] / poa : 0.0;
    }
    if (tid < Kp) st.b[(size_t)s * Kp + tid] = sb[tid] * ssum[tid];
}

// One wave per active start.  The K' x (K' + 1) system [H | g] of the beta-step (K' <= 62) sits in LDS and is solved by Gaussian
// elimination with partial pivoting in solve_dense's pivot and operation order (solvers.hip): lane i owns row i of an elimination
// step; the back substitution runs on lane 0.  Then the loss beta'H beta - 2 g'beta + y'y (Alt.jl:112-113) from the unmodified system
// in global memory, the stop rule of Alt.jl:76 and the record the host reads.  PP: y'y is the start's problem's, yyp[prob[blockIdx.x]].
template <bool PP>
__global__ __launch_bounds__(64) void alt_multi_beta_kernel(AltMultiState st, const int *__restrict__ slot, const double *__restrict__ Hg,
                                                            double yy, double eps, long long T, AltMultiRec *__restrict__ rec,
                                                            const int *__restrict__ prob, const double *__restrict__ yyp)
{
    __shared__ double H[62 * 63];
    __shared__ double term[64];
    const int s = slot[blockIdx.x], Kp = st.Kp, W = Kp + 1, lane = threadIdx.x;
    const double *H0 = Hg + (size_t)blockIdx.x * Kp * W;
    if constexpr (PP) yy = yyp[prob[blockIdx.x]];
    for (int i = lane; i < Kp * W; i += 64) H[i] = H0[i];
    __syncthreads();
    // groups without members get a unit diagonal so that H stays regular
    if (lane < Kp && H[lane * W + lane] == 0.0) H[lane * W + lane] = 1.0;
    __syncthreads();
    bool singular = false;
    for (int k = 0; k < Kp; ++k) {
        int p = k;
        double best = fabs(H[k * W + k]);
        for (int i = k + 1; i < Kp; ++i) { const double v = fabs(H[i * W + k]); if (v > best) { best = v; p = i; } }
        if (H[p * W + k] == 0.0) { singular = true; break; }                  // the same for every lane
        if (p != k) {
            if (lane < W) { const double t = H[p * W + lane]; H[p * W + lane] = H[k * W + lane]; H[k * W + lane] = t; }
            __syncthreads();
        }
        if (lane > k && lane < Kp) {
            const double f = H[lane * W + k] / H[k * W + k];
            if (f != 0.0) {
                for (int j = k; j < Kp; ++j) H[lane * W + j] -= f * H[k * W + j];
                H[lane * W + Kp] -= f * H[k * W + Kp];
            }
        }
        __syncthreads();
    }
    if (singular) {
        if (lane == 0) { rec[blockIdx.x].optval = st.opt[2 * (size_t)s + 1]; rec[blockIdx.x].cont = 0; rec[blockIdx.x].status = PARTLS_ERR_NOT_CONVERGED; }
        return;
    }
    if (lane == 0)
        for (int i = Kp - 1; i >= 0; --i) {
            double t = H[i * W + Kp];
            for (int j = i + 1; j < Kp; ++j) t -= H[i * W + j] * H[j * W + Kp];
            H[i * W + Kp] = t / H[i * W + i];
        }
    __syncthreads();
    if (lane < Kp) {
        const double bk = H[lane * W + Kp];
        double hb = 0.0, hd = 0.0;
        for (int k2 = 0; k2 < Kp; ++k2) {
            double h = H0[lane * W + k2];
            if (k2 == lane) { if (h == 0.0) h = 1.0; hd = h; }
            hb += h * H[k2 * W + Kp];
        }
        term[lane] = bk * (hb - 2.0 * H0[lane * W + Kp]);
        st.b[(size_t)s * Kp + lane] = bk;
        st.hdiag[(size_t)s * Kp + lane] = hd;
    }
    __syncthreads();
    if (lane == 0) {
        double o2 = yy;
        for (int k = 0; k < Kp; ++k) o2 += term[k];
        const double oldopt = st.opt[2 * (size_t)s + 1], optval = sqrt(o2 > 0.0 ? o2 : 0.0);
        const int it = st.iters[s] + 1;
        st.opt[2 * (size_t)s] = oldopt;
        st.opt[2 * (size_t)s + 1] = optval;
        st.iters[s] = it;
        rec[blockIdx.x].optval = optval;
        rec[blockIdx.x].cont = ((long long)it < T && fabs(oldopt - optval) > eps * oldopt) ? 1 : 0;
        rec[blockIdx.x].status = PARTLS_OK;
    }
}

// bump allocator over one device buffer (256-byte aligned pieces)
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *p) : base(static_cast<char *>(p)) {}
    template <class T> T *take(size_t count)
    {
        T *q = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return q;
    }
};

struct ChunkBuffers {
    AltMultiState st;
    int *slot;                     // [2 C] the active slots of an iteration, then (a batch of problems) the problem of each
    int8_t *code;
    unsigned long long *redo;      // [C x 4] counters of the one-start launches that find the starts at the pivot cap
    double *out;                   // [4 counters per problem of the chunk | C records]: what the host reads per iteration
    double *obj2, *sol, *GA, *Hg;
};

// carve the state and the work buffers of a chunk of C slots that touches at most NP problems (base pointers may be null: sizes only)
void carve(const partls_ctx *c, const AltProblems *pp, size_t C, size_t NP, void *state, void *work, ChunkBuffers &cb, size_t *state_bytes,
           size_t *work_bytes)
{
    const size_t n = (size_t)c->n, Mp = (size_t)c->M + 1, Kp = (size_t)c->K + 1;
    Carver s(state), w(work);
    cb.st.n = c->n; cb.st.Mp = (int)Mp; cb.st.Kp = (int)Kp;
    cb.st.a = s.take<double>(C * Mp);
    cb.st.b = s.take<double>(C * Kp);
    cb.st.wv = s.take<double>(C * Mp);
    cb.st.hdiag = s.take<double>(C * Kp);
    cb.st.opt = s.take<double>(C * 2);
    cb.st.iters = s.take<int>(C);
    cb.st.vcode = s.take<int8_t>(C * Mp);
    cb.st.mask_aug = c->maskAugD.as<uint64_t>();
    cb.st.perm = c->permP;
    cb.st.scale = pp ? pp->scale : c->scale.as<double>();
    cb.slot = w.take<int>(2 * C);
    cb.code = w.take<int8_t>(C * n);
    cb.redo = w.take<unsigned long long>(C * 4);
    cb.out = w.take<double>(4 * NP + 2 * C);
    cb.obj2 = w.take<double>(C);
    cb.sol = w.take<double>(C * n);
    cb.GA = w.take<double>(C * Mp * Kp);
    cb.Hg = w.take<double>(C * Kp * (Kp + 1));
    *state_bytes = s.off; *work_bytes = w.off;
}

}  // namespace

namespace partls {

// The multistart itself, for the context's own problem (pp == nullptr: partls_alt_multistart, and partls_cv_alt's serial route) or for
// the B problems of pp at once (partls_cv_alt).  A slot is a (problem, start) pair, s = p R + r; start r of every
// problem begins at row r of alpha0 / beta0.  Slots advance together in chunks of consecutive slots; the active list stays in slot
// order, so the active starts of a problem are neighbours in it and their alpha-steps are one node-mode launch on that problem's
// tableau.  tb: per-slot tables (each optional); win[p]: the winner of problem p and what alt_finish needs of its last iteration.
partls_status alt_multistart_core(partls_ctx *c, const AltProblems *pp, double eps, int64_t T, int64_t R,
                                  const double *alpha0, int64_t ld_alpha0, const double *beta0, int64_t ld_beta0,
                                  const AltTables &tb, AltWinner *win)
{
    const int64_t M = c->M, K = c->K, B = pp ? pp->B : 1, S = B * R;
    const size_t Mp = (size_t)M + 1, Kp = (size_t)K + 1, n = (size_t)c->n;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int max_rounds = c->knobs.alt_ms_max_rounds > 0 ? c->knobs.alt_ms_max_rounds : 20 * (c->n + 1);
    const int Y = (int)M + 1;
    const double yy = pp ? 0.0 : h_reg(c, Y, Y);

    // slots per chunk: the per-slot scratch (GA dominates: (M+1)(K+1) doubles) of a chunk stays within 256 MB
    ChunkBuffers cb{};
    const size_t per_start = 8 * (3 * Mp + 3 * Kp + 5 + n + Mp * Kp + Kp * (Kp + 1)) + 2 * n + 24;
    size_t C = c->knobs.alt_ms_chunk > 0 ? (size_t)c->knobs.alt_ms_chunk : std::max<size_t>(1, ((size_t)256 << 20) / per_start);
    C = std::min<size_t>(std::min<size_t>(C, (size_t)S), (size_t)1 << 20);
    const size_t NP = (size_t)std::min<int64_t>(B, ((int64_t)C + R - 1) / R + 1);      // problems a chunk of consecutive slots can touch
    size_t state_bytes = 0, work_bytes = 0;
    carve(c, pp, C, NP, nullptr, nullptr, cb, &state_bytes, &work_bytes);
    PARTLS_HIP_CHECK(c->amsState.ensure(state_bytes));
    PARTLS_HIP_CHECK(c->amsWork.ensure(work_bytes));
    carve(c, pp, C, NP, c->amsState.p, c->amsWork.p, cb, &state_bytes, &work_bytes);
    const AltMultiState &st = cb.st;
    // page-locked staging: [a0 (C x Mp) | b0 (C x Kp) | opt (C x 2) | slot and problem lists (2 C ints)] up, [counters | records] or the final state back
    const size_t in_words = C * (Mp + Kp + 2) + C;
    const size_t out_words = std::max<size_t>(std::max<size_t>(4 * NP + 2 * C, 4 * C), C * (Mp + Kp + 2) + (C + 1) / 2);
    PARTLS_HIP_CHECK(c->amsHostIn.resize(in_words));
    PARTLS_HIP_CHECK(c->amsHostOut.resize(out_words));
    double *hin = c->amsHostIn.data(), *hout = c->amsHostOut.data();
    int *hslot = reinterpret_cast<int *>(hin + C * (Mp + Kp + 2));

    const bool runs = std::fabs(1e20 - 1e10) > eps * 1e20;       // the stop rule before the first iteration (Alt.jl:73-76); T >= 1
    for (int64_t p = 0; p < B; ++p) {
        AltWinner &w = win[p];
        w.start = -1; w.iters = 0; w.opt = 0.0;
        w.a.assign(Mp, 0.0); w.b.assign(Kp, 0.0); w.wv.assign(Mp, 0.0); w.hdiag.assign(Kp, 0.0); w.vcode.assign(Mp, 0);
    }
    std::vector<int32_t> status(C);
    std::vector<int> active, next, pidx;
    std::vector<char> capped;
    std::vector<unsigned long long> cap;
    std::vector<std::pair<int64_t, size_t>> fresh;               // (problem, slot of the chunk) of the winners this chunk brought
    unsigned long long pivots = 0, vetoes = 0;

    for (int64_t s0 = 0; s0 < S; s0 += (int64_t)C) {
        const size_t cnt0 = (size_t)std::min<int64_t>((int64_t)C, S - s0);
        const int64_t p_first = s0 / R;
        const size_t np = (size_t)((s0 + (int64_t)cnt0 - 1) / R - p_first) + 1;
        // ---- the chunk's starting points: checked on the host, uploaded once ------------------------------------------------
        active.clear();
        for (size_t s = 0; s < cnt0; ++s) {
            const size_t r = (size_t)((s0 + (int64_t)s) % R);
            const double *a0 = alpha0 + r * (size_t)ld_alpha0, *b0 = beta0 + r * (size_t)ld_beta0;
            bool finite = true;
            for (size_t m = 0; m < Mp; ++m) finite = finite && std::isfinite(a0[m]);
            for (size_t k = 0; k < Kp; ++k) finite = finite && std::isfinite(b0[k]);
            status[s] = finite ? PARTLS_OK : PARTLS_ERR_NONFINITE;
            std::memcpy(hin + s * Mp, a0, Mp * sizeof(double));
            std::memcpy(hin + C * Mp + s * Kp, b0, Kp * sizeof(double));
            hin[C * (Mp + Kp) + 2 * s] = 1e20;                   // oldopt, optval (Alt.jl:73-74)
            hin[C * (Mp + Kp) + 2 * s + 1] = 1e10;
            if (finite && runs) active.push_back((int)s);
        }
        PARTLS_HIP_CHECK(hipMemcpyAsync(st.a, hin, cnt0 * Mp * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(st.b, hin + C * Mp, cnt0 * Kp * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(st.opt, hin + C * (Mp + Kp), cnt0 * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PARTLS_HIP_CHECK(hipMemsetAsync(st.iters, 0, cnt0 * sizeof(int), c->stream));
        PARTLS_HIP_CHECK(hipMemsetAsync(st.vcode, 0, cnt0 * Mp, c->stream));
        PARTLS_HIP_CHECK(hipMemsetAsync(st.wv, 0, cnt0 * Mp * sizeof(double), c->stream));
        PARTLS_HIP_CHECK(hipMemsetAsync(st.hdiag, 0, cnt0 * Kp * sizeof(double), c->stream));

        // ---- iterations: every active slot advances by one, then the host reads their records -------------------------------
        while (!active.empty()) {
            const size_t cnt = active.size();
            pidx.resize(cnt);
            for (size_t j = 0; j < cnt; ++j) pidx[j] = (int)((s0 + active[j]) / R);          // the slot's problem (0 without pp)
            std::memcpy(hslot, active.data(), cnt * sizeof(int));
            if (pp) std::memcpy(hslot + cnt, pidx.data(), cnt * sizeof(int));
            PARTLS_HIP_CHECK(hipMemcpyAsync(cb.slot, hslot, (pp ? 2 : 1) * cnt * sizeof(int), hipMemcpyHostToDevice, c->stream));
            const int *dprob = cb.slot + cnt;
            unsigned long long *dctr = reinterpret_cast<unsigned long long *>(cb.out);
            AltMultiRec *drec = reinterpret_cast<AltMultiRec *>(cb.out + 4 * np);
            PARTLS_HIP_CHECK(hipMemsetAsync(cb.out, 0, 4 * np * sizeof(double), c->stream));
            hipLaunchKernelGGL(alt_multi_codes_kernel, dim3((unsigned)cnt), dim3(256), 0, c->stream, st, cb.slot, cb.code);
            PARTLS_HIP_CHECK(hipGetLastError());
            // alpha-steps: one node-mode launch per problem that still has active starts, back to back on the stream
            auto alpha_steps = [&](size_t j0, size_t j1, unsigned long long *ctr) {
                if (!pp) return solve_nodes_device(c, j1 - j0, cb.code + j0 * n, cb.obj2 + j0, cb.sol + j0 * n, ctr, max_rounds);
                const size_t p = (size_t)pidx[j0];
                return solve_nodes_device_at(c, pp->T0reg + p * pp->t0d, pp->tol[p], j1 - j0, cb.code + j0 * n, cb.obj2 + j0, cb.sol + j0 * n, ctr,
                                             max_rounds);
            };
            for (size_t j0 = 0, j1; j0 < cnt; j0 = j1) {
                for (j1 = j0 + 1; j1 < cnt && pidx[j1] == pidx[j0]; ++j1) {}
                const partls_status ss = alpha_steps(j0, j1, dctr + 4 * (size_t)(pidx[j0] - p_first));
                if (ss != PARTLS_OK) return ss;
            }
            if (pp) {
                hipLaunchKernelGGL(alt_multi_alpha_kernel<true>, dim3((unsigned)cnt), dim3(256), 0, c->stream, st, cb.slot, cb.sol, dprob);
                PARTLS_HIP_CHECK(hipGetLastError());
                PARTLS_HIP_CHECK(launch_alt_beta_system_problems(pp->G, pp->gs, (int)pp->E, pp->q0, pp->eta, dprob, c->ldg, (int)M,
                                                                 c->maskAugD.as<uint64_t>(), st.a, (int)Kp, cb.slot, (int)cnt, cb.GA, cb.Hg, c->stream));
                hipLaunchKernelGGL(alt_multi_beta_kernel<true>, dim3((unsigned)cnt), dim3(64), 0, c->stream, st, cb.slot, cb.Hg, 0.0, eps, (long long)T,
                                   drec, dprob, pp->yy);
            } else {
                hipLaunchKernelGGL(alt_multi_alpha_kernel<false>, dim3((unsigned)cnt), dim3(256), 0, c->stream, st, cb.slot, cb.sol, (const int *)nullptr);
                PARTLS_HIP_CHECK(hipGetLastError());
                PARTLS_HIP_CHECK(launch_alt_beta_system_batch(c->G.as<double>(), c->ldg, (int)M, c->eta, c->maskAugD.as<uint64_t>(), st.a, (int)Kp,
                                                              cb.slot, (int)cnt, cb.GA, cb.Hg, c->stream));
                hipLaunchKernelGGL(alt_multi_beta_kernel<false>, dim3((unsigned)cnt), dim3(64), 0, c->stream, st, cb.slot, cb.Hg, yy, eps, (long long)T,
                                   drec, (const int *)nullptr, (const double *)nullptr);
            }
            PARTLS_HIP_CHECK(hipGetLastError());
            PARTLS_HIP_CHECK(hipMemcpyAsync(hout, cb.out, (4 * np + 2 * cnt) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
            cap.assign(np, 0);
            bool any_cap = false;
            for (size_t i = 0; i < np; ++i) {
                unsigned long long ctr[4];
                std::memcpy(ctr, hout + 4 * i, sizeof(ctr));
                cap[i] = ctr[0]; pivots += ctr[1]; vetoes += ctr[2];
                any_cap = any_cap || ctr[0] != 0;
            }
            const AltMultiRec *rec = reinterpret_cast<const AltMultiRec *>(hout + 4 * np);
            next.clear();
            capped.assign(cnt, 0);
            if (any_cap) {
                // node mode counts pivot-cap hits per launch: the alpha-steps of the launches that counted one again (their codes are still
                // there), one start per launch with counters of its own, tell which starts they were.  The others' iteration stands: no
                // start reads another's rows.
                std::vector<AltMultiRec> keep(rec, rec + cnt);
                PARTLS_HIP_CHECK(hipMemsetAsync(cb.redo, 0, cnt * 4 * sizeof(unsigned long long), c->stream));
                for (size_t j = 0; j < cnt; ++j) {
                    if (!cap[(size_t)(pidx[j] - p_first)]) continue;
                    const partls_status ss = alpha_steps(j, j + 1, cb.redo + 4 * j);
                    if (ss != PARTLS_OK) return ss;
                }
                PARTLS_HIP_CHECK(hipMemcpyAsync(hout, cb.redo, cnt * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
                PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
                const unsigned long long *rc = reinterpret_cast<const unsigned long long *>(hout);
                for (size_t j0 = 0, j1; j0 < cnt; j0 = j1) {                              // problem by problem
                    for (j1 = j0 + 1; j1 < cnt && pidx[j1] == pidx[j0]; ++j1) {}
                    if (!cap[(size_t)(pidx[j0] - p_first)]) continue;
                    bool any = false;
                    for (size_t j = j0; j < j1; ++j) { capped[j] = rc[4 * j] != 0; any = any || capped[j]; }
                    if (!any) std::fill(capped.begin() + (ptrdiff_t)j0, capped.begin() + (ptrdiff_t)j1, 1);   // cannot tell them apart: none of this launch is trusted
                }
                for (size_t j = 0; j < cnt; ++j) {
                    if (capped[j]) status[(size_t)active[j]] = PARTLS_ERR_NOT_CONVERGED;
                    else if (keep[j].status != PARTLS_OK) status[(size_t)active[j]] = keep[j].status;
                    else if (keep[j].cont) next.push_back(active[j]);
                }
            } else {
                for (size_t j = 0; j < cnt; ++j) {
                    if (rec[j].status != PARTLS_OK) status[(size_t)active[j]] = rec[j].status;
                    else if (rec[j].cont) next.push_back(active[j]);
                }
            }
            active.swap(next);
        }

        // ---- the chunk's results -----------------------------------------------------------------------------------------------
        double *ha = hout, *hb = hout + C * Mp, *ho = hout + C * (Mp + Kp);
        int *hit = reinterpret_cast<int *>(hout + C * (Mp + Kp + 2));
        PARTLS_HIP_CHECK(hipMemcpyAsync(ha, st.a, cnt0 * Mp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(hb, st.b, cnt0 * Kp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(ho, st.opt, cnt0 * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipMemcpyAsync(hit, st.iters, cnt0 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
        fresh.clear();
        for (size_t s = 0; s < cnt0; ++s) {
            const int64_t g = s0 + (int64_t)s, p = g / R, r = g % R;
            const bool ok = status[s] == PARTLS_OK;
            const double *as = ha + s * Mp, *bs = hb + s * Kp;
            if (tb.alpha_all) for (int64_t m = 0; m < M; ++m) tb.alpha_all[(size_t)g * (size_t)tb.ld_alpha_all + (size_t)m] = ok ? as[m] : nan;
            if (tb.beta_all) for (int64_t k = 0; k < K; ++k) tb.beta_all[(size_t)g * (size_t)tb.ld_beta_all + (size_t)k] = ok ? bs[k] : nan;
            if (tb.t_all) tb.t_all[g] = ok ? bs[K] * as[M] : nan;                  // Alt.jl:119
            if (tb.opt_all) tb.opt_all[g] = ok ? ho[2 * s + 1] : nan;
            if (tb.iters_all) tb.iters_all[g] = ok ? hit[s] : 0;
            if (tb.status_all) tb.status_all[g] = status[s];
            // the winner: smallest final loss, lowest index on an exact tie; a NaN loss wins only against nothing
            const double o = ho[2 * s + 1];
            AltWinner &w = win[p];
            if (ok && (w.start < 0 || o < w.opt || (std::isnan(w.opt) && !std::isnan(o)))) {
                w.start = r; w.opt = o;
                if (!fresh.empty() && fresh.back().first == p) fresh.back().second = s; else fresh.emplace_back(p, s);
            }
        }
        for (const auto &ps : fresh) {
            AltWinner &w = win[ps.first];
            const size_t s = ps.second;
            w.iters = hit[s];
            std::memcpy(w.a.data(), ha + s * Mp, Mp * sizeof(double));
            std::memcpy(w.b.data(), hb + s * Kp, Kp * sizeof(double));
            // what the data-space check of the ending needs of the winner's last iteration
            PARTLS_HIP_CHECK(hipMemcpyAsync(w.wv.data(), st.wv + s * Mp, Mp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            PARTLS_HIP_CHECK(hipMemcpyAsync(w.hdiag.data(), st.hdiag + s * Kp, Kp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            PARTLS_HIP_CHECK(hipMemcpyAsync(w.vcode.data(), st.vcode + s * Mp, Mp, hipMemcpyDeviceToHost, c->stream));
        }
        if (!fresh.empty()) PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    c->last_pivots = pivots; c->last_vetoes = vetoes; c->last_blocks = 0;
    return PARTLS_OK;
}

}  // namespace partls

extern "C" {

partls_status partls_alt_multistart(partls_ctx *c, double eps, int64_t T, int64_t R,
                                    const double *alpha0, int64_t ld_alpha0, const double *beta0, int64_t ld_beta0,
                                    double *alpha, double *beta, double *t, double *opt, int64_t *iters, int64_t *best_start,
                                    double *alpha_all, int64_t ld_alpha_all, double *beta_all, int64_t ld_beta_all,
                                    double *t_all, double *opt_all, int64_t *iters_all, int32_t *status_all)
try {
    if (!c || !c->prepared || !c->faithful) { set_error("partls_alt_multistart: needs a context prepared with PARTLS_OPT_FAITHFUL_INTERCEPT"); return PARTLS_ERR_STATE; }
    if (!alpha0 || !beta0 || !alpha || !beta || !t || !opt || !iters || !best_start) { set_error("partls_alt_multistart: NULL argument"); return PARTLS_ERR_BAD_ARG; }
    if (!(eps > 0.0) || T < 1 || R < 1) { set_error("partls_alt_multistart: need eps > 0, T >= 1 and R >= 1"); return PARTLS_ERR_BAD_ARG; }
    const int64_t M = c->M, K = c->K;
    if (ld_alpha0 < M + 1 || ld_beta0 < K + 1 || (alpha_all && ld_alpha_all < M) || (beta_all && ld_beta_all < K)) {
        set_error("partls_alt_multistart: leading dimension smaller than the row count");
        return PARTLS_ERR_BAD_ARG;
    }
    PARTLS_HIP_CHECK(hipSetDevice(c->device));
    // Gershgorin radii for the winner's ending (alt_finish), read back with the first iteration's records
    std::vector<double> gersh((size_t)c->n, 0.0);
    PARTLS_HIP_CHECK(c->altGersh.ensure((size_t)c->n * sizeof(double)));
    PARTLS_HIP_CHECK(launch_gersh(c->Tfull.as<double>(), c->n, c->altGersh.as<double>(), c->stream));
    PARTLS_HIP_CHECK(hipMemcpyAsync(gersh.data(), c->altGersh.p, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    const AltTables tb{alpha_all, ld_alpha_all, beta_all, ld_beta_all, t_all, opt_all, iters_all, status_all};
    AltWinner w;
    const partls_status st = alt_multistart_core(c, nullptr, eps, T, R, alpha0, ld_alpha0, beta0, ld_beta0, tb, &w);
    if (st != PARTLS_OK) return st;
    PARTLS_HIP_CHECK(hipStreamSynchronize(c->stream));               // the Gershgorin radii, when no chunk synchronised
    if (w.start < 0) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        *best_start = -1; *iters = 0; *t = nan; *opt = nan;
        for (int64_t m = 0; m < M; ++m) alpha[m] = nan;
        for (int64_t k = 0; k < K; ++k) beta[k] = nan;
        set_error("partls_alt_multistart: no start finished (non-finite starting point, pivot cap or singular beta-step in every one)");
        return PARTLS_ERR_NOT_CONVERGED;
    }
    *best_start = w.start;
    return alt_finish(c, w.a, w.b, w.wv, w.vcode, w.hdiag, gersh, w.opt, w.iters, 0, alpha, beta, t, opt, iters);
}
PARTLS_ABI_GUARD

}  // extern "C"
