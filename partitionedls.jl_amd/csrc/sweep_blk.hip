// sweep_blk.hip — production sign-pattern sweep, BLOCKED principal pivots on a register-resident tableau (n <= 320).
//
// Replaces the loop body of fit(Opt), Opt.jl:87-90 (indextobeta + bmatrix + nonneg_lsq + objective), for every pattern of a
// Gray-code chain, and serves the node solves of Alt (Alt.jl:80-90) and BnB (BnB.jl:69-92); same mathematics and the same
// per-pattern decisions as the other tableau kernels: the rules of sweep_rules.h.
//
// Data layout (one workgroup = 512 threads = 8 waves = 2 waves/SIMD on one CU, one tableau, one chain):
//   * variables are padded to 16*T; the symmetric tableau is cut into 16x16 tiles (rho, gamma), rho <= gamma only;
//   * thread (a, b) = (t & 15, (t >> 4) & 15) owns element (16 rho + a, 16 gamma + b) of EVERY stored tile — a tile-cyclic
//     layout, so a pivot is an outer-product update in registers with static register indices only;
//   * v_fma_f64 can address only the 256 architectural VGPRs, so the T(T+1)/2 tile slots (153 at n = 257) are split
//     between the two halves of the workgroup by tile COLUMN (threads 0..255: gamma < G, threads 256..511: gamma >= G);
//   * rhs column q: thread v owns q_v (v < n); the objective (corner) is replicated; KKT scan = one ballot per wave.
// The violators of one KKT scan are exchanged one TILE COLUMN at a time as a block pivot of m <= 8 variables
//     T'_RR = T_RR - sum_s z_s z_s' / d_s          (z_s = pivot column as of its own step, d_s its pivot):
//   1. gather   : the pivot columns go from registers to an LDS panel P[m cols][rows] (+ rhs row), compacted;
//   2. panel    : thread t owns ROW t of the panel in registers (<= 8 pivot columns); m sequential Gauss–Jordan steps, each
//                 exchanging only the m pivot-row entries of the CURRENT pivot column and 1/d through LDS (one barrier per
//                 step); z_s and 1/d_s are recorded for the update;
//   3. update   : all 512 threads: S(rho,gamma) -= x_s[rho] * y_s[gamma] for s = 1..m (x resident, y streamed from LDS);
//   4. scatter  : rows/columns of the pivoted variables are overwritten from the final panel (one if-chain per tile).
//
// Dependent columns.  An entering variable k is refused (Lawson–Hanson's rejection; re-examined after any exchange) when the
// basis B + k would be numerically dependent at the 1e-11 level on the unit-diagonal scale: with c_j = T[j][k] the regression
// coefficients of column k on the basic columns, the leave-one-out pivot of EVERY member of B + k must stay above piv_eps —
//     d_k > piv_eps                      (k itself:  relative residual norm of x_k after regression on B)
//     d_k > piv_eps * c_j^2  (j in B)    (1 / d_j(B + k) = 1 / d_j(B) + c_j^2 / d_k)
// The second line is what a Gram-based method needs on top of the textbook rule: the computed d_k carries an error of
// eps * (1 + |c|)^2, so with large coefficients (an exactly dependent column next to a nearly collinear pair) a true zero
// comes out at 1e-11..1e-10 and the fixed threshold alone accepts it (round-1 fuzz blocks 9 and 24).  The panel is computed
// optimistically; a thread that sees the second condition violated in its own row reports the step, the block is abandoned
// before the register tableau is touched, the offender is marked rejected and the rest of the block is redone.
// The test needs no basis bookkeeping: for a NONBASIC row j the Schur complement is positive semidefinite, T_jk^2 <= T_jj T_kk
// <= d_k, so d_k > piv_eps * T_jk^2 holds with a margin of 1e11 and every row can simply test its own entry; a leaving pivot
// has 1/d < 0 and a rejected one 1/d = 0, which fail the test by sign.  Only the rhs row (no variable) must not report.
#include "sweep_rules.h"
#include <atomic>
#include <type_traits>

namespace partls {
namespace blk {

static constexpr int THREADS = 512;
static constexpr int MAXT = 20;                 // n <= 320 compiled (T = 21: 1500 spilled VGPRs); the library switches to sweep_lazy.hip beyond T = 18 (ctx.h: reg_maxt)
#ifndef PARTLS_UPD_UNROLL
#define PARTLS_UPD_UNROLL 1
#endif
static constexpr int MB = 8;                    // pivots per block (a tile column with more violators takes two blocks): the 256-thread kernel
#ifndef PARTLS_EXPORT_BIG
#define PARTLS_EXPORT_BIG 1      // the 512-thread kernel leaves the solution of every workgroup's best pattern behind (round 4: C3 finish 0.54 -> 0.16 ms, sweep 49.1 -> 48.6)
#endif
#ifndef PARTLS_MERGED_SCAN
#define PARTLS_MERGED_SCAN 1     // 0: every pattern starts with a KKT scan of its own (A/B of the two round-5 pieces apart: profiles/r05_ab_c3.txt)
#endif
#ifndef PARTLS_LANE_MASKS
#define PARTLS_LANE_MASKS 1      // 0: a tile column's masks come from LDS
#endif
#ifndef PARTLS_MB_BIG
#define PARTLS_MB_BIG 8
#endif
#ifndef PARTLS_PAIR
#define PARTLS_PAIR 1            // 0: the pair walk of the 512-thread chain kernel is not compiled (every Gray flip is exchanged on the tableau)
#endif
static constexpr int EXPORT_MAXT = 17;          // ... up to this tile count (beyond it the two live registers of the export start spilling: 22 -> 32 spilled VGPRs at T = 18)
static constexpr int MBB = PARTLS_MB_BIG;       // ... of the 512-thread kernel (8..16; experiments: tools/experiments/README.md)
static constexpr int NO_VETO = 99;
static constexpr int PAIR_MAXC = 16;            // pair walk: most violators a twin is priced with (the two panel buffers hold 2 MBB >= 16 columns)
static constexpr int PAIR_PIV_MIN_HI = 0x3f1a36e2;   // ... and the smallest entering pivot (unit-diagonal scale) it is priced with: the high word of 1e-4
                                                // (0x3f1a36e2eb1c432d) — a pivot is accepted when its high word, as a signed integer, is ABOVE this one, i.e.
                                                // d >= 1.00000000055e-4: a scalar compare with a literal, where the double constant costs two VGPRs the
                                                // compiler keeps live through the whole kernel.  The rounds' dependent-column rule, d <= 1e-11 max(1, cmax^2),
                                                // needs the whole panel; a twin below the guard is left to the rounds
static constexpr int PAIR_XCH = 40;             // ... and where, in doubles behind pair_solve's `out`, its 16 doubles of lane exchange lie (16-byte aligned)
static constexpr int F64_EXP_HI = 0x7ff00000;   // the exponent bits of a double's high word: all set = inf or NaN (whose high word lies ABOVE the guard's)

constexpr int nslots(int T) { return T * (T + 1) / 2; }
constexpr int tri(int g) { return g * (g + 1) / 2; }
constexpr int split(int T)
{
    int best = 1, bestmax = 1 << 30;
    for (int g = 1; g < T; ++g) {
        int a = tri(g), b = nslots(T) - tri(g);
        int m = a > b ? a : b;
        if (m < bestmax) { bestmax = m; best = g; }
    }
    return T == 1 ? 1 : best;
}
constexpr int rstride(int T) { return (T % 2) ? T : T + 1; }      // odd row stride: 16 lanes x 8 B hit 32 distinct banks
constexpr int colw(int T) { return 513; }                          // panel column: one slot per thread (16*RS rows + rhs + dummies), odd
// Small tableaus (T <= MAXT_S tile columns, n <= 160): ONE group of 256 threads owns every tile slot (<= 55 doubles per thread), so a
// workgroup is 4 waves and a CU holds three of them — three independent chains whose latency chains (panel steps, scans, barriers)
// interleave on the same SIMDs instead of one chain leaving them idle (BASELINE config 2: n = 128).
static constexpr int MAXT_S = 10;
static constexpr int CW_S = 257;                                   // one panel slot per thread of the 256-thread workgroup, odd
template <class PT> __device__ __forceinline__ PT *uniform_ptr(PT *p)     // a wave-uniform pointer the compiler cannot prove uniform -> SGPR pair
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (PT *)(((unsigned long long)hi << 32) | lo);
}

// Diagnostic build only (-DPARTLS_STAMPS): per-phase cycle shares of workgroup 0 / thread 0, written to p.scratch[0..23]
// (a buffer no other code of the kernel reads).  Never quote this build's run time (cdna_hip_programming.md §7).
#ifdef PARTLS_STAMPS
#define STAMP_DECL unsigned long long st_acc[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long st_t = __builtin_amdgcn_s_memtime();
#define STAMP(ph) do { __builtin_amdgcn_sched_barrier(0); unsigned long long _n = __builtin_amdgcn_s_memtime(); \
                       st_acc[ph] += _n - st_t; st_t = _n; __builtin_amdgcn_sched_barrier(0); } while (0)
#ifndef PARTLS_STAMP_TID
#define PARTLS_STAMP_TID 0
#endif
#define STAMP_FLUSH do { if (tid == PARTLS_STAMP_TID && blockIdx.x == 0 && p.scratch) { for (int _i = 0; _i < 24; ++_i) p.scratch[_i] = (double)st_acc[_i]; \
                                p.scratch[24] = (double)bc; p.scratch[25] = (double)sc; p.scratch[26] = (double)npiv; } } while (0)   /* + blocks, scans, pivots of workgroup 0 */
#define STAMP_PARAMS , unsigned long long (&st_acc)[24], unsigned long long &st_t       /* a helper that stamps: the caller's accumulators */
#define STAMP_ARGS , st_acc, st_t
#else
#define STAMP_DECL
#define STAMP(ph) do { } while (0)
#define STAMP_FLUSH do { } while (0)
#define STAMP_PARAMS
#define STAMP_ARGS
#endif

// LDS image, statically allocated at namespace scope (one copy per kernel, shared by the two half instantiations): every
// address is a link-time constant that folds into the ds_* immediates — with a dynamic base the compiler kept ~20 slot
// addresses in SGPRs and spilled them to VGPR lanes inside the panel steps.  ~100 KB of the CU's 160 KB.
static constexpr int CWMAX = colw(MAXT);
template <int CWX, int MAXTX>
struct LdsImageT {
    double Z[MB * CWX];
    double U[2 * (MB + 64)];
    double Dinv[MB + 64];
    unsigned long long s_inf[32];
    unsigned long long s_bas[16];
    unsigned long long s_sum[16];
    int s_veto[2];
    double s_best[4];
    unsigned char s_rbit[64];
    unsigned long long s_vmask[16 * MAXTX];
    double Pbase[2 * MB * CWX];
};
// One struct, so that the order is ours: everything the update and the panel steps address with per-thread offsets (Z, U, Dinv,
// the masks) sits in the first 64 KB, where base + element offset fits the 16-bit immediate of the ds_* instructions; with Z
// behind the two panel buffers every operand read of the update loop needed its own v_add for the address.
struct LdsImage {
    double Z[MBB * CWMAX];                     // [MB][CW] pivot column s as of its own step
    double U[2 * (MBB + 64)];                  // [2][MB+64] pivot-row entries of the current column (+ per-lane dummies)
    double Dinv[MBB + 64];                     // 1/d_s
    unsigned long long s_inf[32];              // [2][2][8] violator masks of the scan: [0] of the pattern being solved, [1] ("s_inf2") of the NEXT pattern of the chain on the same rhs column
    unsigned long long s_bas[16];              // [2][8] basis mask of the scan
    unsigned long long s_sum[16];              // [2][8] per-wave summaries, count | tile bits << 8: of s_inf in the low word, of s_inf2 in the high word (one read)
    int s_veto[2];                             // first vetoed step of a block (by block parity)
    // per-thread state that is touched once per pattern lives in LDS, not in VGPRs (the register file holds the tableau):
    double s_best[4];                          // running minimum: obj^2, pattern (as bits); runner-up: obj^2, pattern
    unsigned char s_rbit[64];                  // reference bit of internal pattern bit b (exact ties only)
    unsigned long long s_vmask[16 * MAXT];     // group mask of variable v
    double Pbase[2 * MBB * CWMAX];             // [2][MB][CW] panel, double buffered by block parity
};
static_assert(2 * MBB >= PAIR_MAXC, "the pair walk gathers up to PAIR_MAXC columns into the two panel buffers");
__shared__ LdsImage lds_image;
__shared__ LdsImageT<CW_S, MAXT_S> lds_small;              // the 256-thread kernel's image (~51 KB: three workgroups per CU)

template <int W>
__device__ __forceinline__ auto *image_of()
{
    if constexpr (W == 1) return &lds_small; else return &lds_image;
}

// W = 2: the tile slots are split between the two halves H = 0 / 1 of a 512-thread workgroup; W = 1: one group of 256 threads owns all
template <int T, int H, int W = 2>
struct Half {
    static constexpr int G = W == 1 ? T : split(T);
    static constexpr int GLO = H ? G : 0;
    static constexpr int GHI = H ? T : G;
    static constexpr int OFF = H ? tri(G) : 0;
    static constexpr int CNT = (H ? nslots(T) - tri(G) : tri(G)) > 0 ? (H ? nslots(T) - tri(G) : tri(G)) : 1;
    static constexpr int XN = GHI;
    static constexpr int RS = rstride(T);
    static constexpr int CW = W == 1 ? CW_S : colw(T);
    static constexpr int NT = W == 1 ? 256 : THREADS;              // threads of the workgroup
    __device__ static constexpr int idx(int rho, int gam) { return tri(gam) + rho - OFF; }
};

// ---- the thread's tile slots -> a tableau image in global memory (snapshots, node_tab) ----------------------------------
// The address loop of the chain start in sweep_body (see the comment there), storing.  The load stays written out where it is
// used: as a helper the same loop compiles to the same registers but reschedules the chain-mode kernels.
template <class L>
__device__ __forceinline__ void tiles_store(double *dst, const double (&S)[L::CNT], int t8)
{
    double *bp = uniform_ptr(dst) + (size_t)L::OFF * 256;
#pragma unroll
    for (int s = 0; s < L::CNT; ++s) {
        if ((s & 1) == 0) asm volatile("" : "+s"(bp));
        bp[(s & 1) * 256 + t8] = S[s];
        if (s & 1) bp += 512;
    }
}

// ---- tile-column gather ------------------------------------------------------------------------------------------------
// Element (16 rho + a, 16 KAPPA + b) belongs to column b of the tile, row position a*RS + rho.  Only the pivot columns are
// gathered, COMPACTED: the j-th pivot of the block (ascending local index) becomes panel column j = popc(pm below it).
template <int T, int H, int W, int KAPPA, class SA>
__device__ __forceinline__ void gather_tile(const SA &S, double *P, int a, int b, unsigned pm)
{
    using L = Half<T, H, W>;
    if constexpr (KAPPA >= L::GLO && KAPPA < L::GHI) {
        if ((pm >> b) & 1u) {
            double *col = P + __builtin_popcount(pm & ((1u << b) - 1u)) * L::CW + a * L::RS;
#pragma unroll
            for (int rho = 0; rho <= KAPPA; ++rho) col[rho] = S[L::idx(rho, KAPPA)];
        }
    }
    // row KAPPA of the stored triangle = column (16 KAPPA + a) by symmetry, row position b*RS + gamma
    if ((pm >> a) & 1u) {
        double *col = P + __builtin_popcount(pm & ((1u << a) - 1u)) * L::CW + b * L::RS;
#pragma unroll
        for (int gam = (KAPPA + 1 > L::GLO ? KAPPA + 1 : L::GLO); gam < L::GHI; ++gam) col[gam] = S[L::idx(KAPPA, gam)];
    }
}

template <int T, int H, int W, int KAPPA, class SA>
__device__ __forceinline__ void scatter_tile(SA &S, const double *P, int a, int b, unsigned pm)
{
    using L = Half<T, H, W>;
    if constexpr (KAPPA >= L::GLO && KAPPA < L::GHI) {
        if ((pm >> b) & 1u) {
            const double *col = P + __builtin_popcount(pm & ((1u << b) - 1u)) * L::CW + a * L::RS;
#pragma unroll
            for (int rho = 0; rho <= KAPPA; ++rho) S[L::idx(rho, KAPPA)] = col[rho];
        }
    }
    if ((pm >> a) & 1u) {
        const double *col = P + __builtin_popcount(pm & ((1u << a) - 1u)) * L::CW + b * L::RS;
#pragma unroll
        for (int gam = (KAPPA > L::GLO ? KAPPA : L::GLO); gam < L::GHI; ++gam) S[L::idx(KAPPA, gam)] = col[gam];
    }
}

// ---- panel elimination for a block of exactly M pivots (M = 1..MB); straight-line code, no guards ------------------------
// Thread t owns row position `prow` (= t for the real positions) of the M (compacted) pivot columns in registers pv[0..M);
// threads beyond the rhs row work on dummy positions: computed, stored, never read.  Step s: the pivot-row threads publish
// their entry of column s through U, the thread that IS pivot row s also publishes 1/d (0 for a dependent column, Lawson–
// Hanson's rejection) — both as unconditional stores, non-owners hit a dummy slot — one barrier, one batch of broadcast
// reads, then every thread updates its own row with  T_ij -= T_is T_sj / d,  T_is = T_is / |d|,  T_ss = -1/d.
// NUMERICS: the factor T_sj is taken from the pivot COLUMN s (its entry at pivot row j, u[j]) — never from column j at pivot
// row s, which is the same number only in exact arithmetic.  With u from column s the panel receives exactly the symmetric
// rank-1 term z_s z_s' / d_s that the register tableau receives in the update; mixing the two breaks that consistency and
// loses the solution on ill-conditioned data (pivots ~1e-8: measured, tools/tableau_emul.py --block).
// `my_basic`: this thread is a pivot row and its variable is basic (leaves).
// Returns the first step whose entering pivot this thread's row vetoes under the leave-one-out rule (file header), M if none.
template <int M, int CW, int MBK>
__device__ __forceinline__ int panel_block(double *P, double *Z, double *U, double *Dinv, int myj, bool my_basic,
                                           double piv_eps, int tid, int prow, bool idle_wave)
{
    // A wave whose 64 row positions all lie beyond the rhs row owns no panel row.  Two waves share a SIMD's issue slots, so
    // such a wave only keeps the barrier count instead of competing with a real wave.
    if (idle_wave) {
#pragma unroll
        for (int s = 0; s < M; ++s) __syncthreads();
        return M;
    }
    constexpr int US = MBK + 64;                            // U row stride; slots MB.. are per-lane dummies (no same-address stores)
    const int dummy = MBK + (tid & 63);
    double pv[M];
#pragma unroll
    for (int j = 0; j < M; ++j) pv[j] = P[j * CW + prow];
    const int uslot = myj >= 0 ? myj : dummy;
    int veto = M;
#pragma unroll
    for (int s = 0; s < M; ++s) {
        Z[s * CW + prow] = pv[s];
        U[(s & 1) * US + uslot] = pv[s];
        if (myj == s) {                                     // the one pivot-row thread (its wave only: the others branch over)
            const double d = pv[s];
            Dinv[s] = (my_basic || d > piv_eps) ? rcp_newton(d) : 0.0;
        }
        __syncthreads();
        double inv = Dinv[s];
        double u[M];
#pragma unroll
        for (int j = 0; j < M; ++j) u[j] = U[(s & 1) * US + j];
        // all reads of the step are issued together, right after the barrier: left alone, the compiler sinks the u[j] loads into the
        // "pivot accepted" branch, i.e. behind a second LDS round trip (wait for 1/d, branch, then load and wait again)
        asm volatile("" : "+v"(inv));
#pragma unroll
        for (int j = 0; j < M; ++j) asm volatile("" : "+v"(u[j]));
        // leave-one-out veto: T_js^2 >= d / piv_eps  (inv = 1/d; negative for a leaving pivot, 0 for a rejected one)
        if ((pv[s] * pv[s]) * (inv * piv_eps) >= 1.0) veto = veto < s ? veto : s;
        // inv is the same in every lane: a scalar branch skips a rejected pivot (1/d = 0: exponent field 0)
        if (__builtin_amdgcn_readfirstlane(__double2hiint(inv)) & 0x7ff00000) {
            const double ainv = fabs(inv), fz = -pv[s] * inv;
            if (myj == s) {                                 // pivot row: T_sj / |d| from the pivot COLUMN's entries, T_ss = -1/d
#pragma unroll
                for (int j = 0; j < M; ++j) pv[j] = (j == s) ? -inv : u[j] * ainv;
            } else {
#pragma unroll
                for (int j = 0; j < M; ++j) pv[j] = (j == s) ? pv[s] * ainv : fma(fz, u[j], pv[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < M; ++j) P[j * CW + prow] = pv[j];
    return veto;
}

// ---- pair walk: the twin's |C| x |C| solve on ONE wave, no workgroup barrier inside ------------------------------------------
// The m columns of C (ascending variable index; where they lie in the panel: below) are eliminated by the m sequential pivots of
// panel_block, restricted to what decides: the m pivot rows and, as a column of its own, their rhs entries q_C (the panel's rhs row,
// by symmetry).  The rhs column ends as the twin's rhs entries q'_C of the pivot rows (what scatter takes from the final panel), and
// these ARE the coefficients of the rank-m update of every other row: with T_ik / |d|, T_kk = -1/d a single pivot gives
// q_i - T_ik q_k / d and q'_k = q_k / |d|, i.e. q_i - T_ik a_k with a_k = +q'_k for an entering and -q'_k for a leaving variable, and
// so for the block (the sweeps of distinct variables commute); the rhs row itself is such a row: corner' = corner - sum_k q_k a_k.
// Checked against sequential pivots in tools/pair_emul.py.
// Layout, DENSE: the panel holds ALL 16 columns of the pair column KC (sweep_body: the static gather), panel column k = variable 16 KC + k,
// whose row position is k RS + KC.  Lane = r + 16 h holds row r of the four columns 4 h .. 4 h + 3 of that 16 x 16 block, loaded from
// fixed addresses.  The steps run over k = 0 .. 15 in ascending order and a wave-uniform bit test of the violator mask `cm` skips every
// column outside C: exactly |C| steps execute, in the order of the compacted solve.  All 16 steps are written out, so the step, its
// quarter k >> 2 and its register k & 3 are constants.  The pivot column of step k lies in the 16 lanes of quarter k >> 2: they store it
// to a 16-double exchange in LDS (one masked ds_write_b64), and every lane reads its own row's entry (ds_read_b64) and the pivot row's
// entries of its four columns (two broadcast ds_read_b128) from there — the same doubles ten ds_bpermute_b32 carried before.  The exchange
// lies in U behind `out` (PAIR_XCH: in the first 64 KB, so its offsets are immediates; a field of its own would cost an address register).
// Every lane does the step's five FMAs; the pivot column (quarter k >> 2) and the pivot row (the four lanes r == k) are then overwritten
// under EXEC.  Rows and columns outside C carry whatever the tableau holds there and are updated along with the rest; an
// entry (r, c) with r and c in C only ever takes its factors from rows r and c of a pivot column of C, so none of that reaches C, and the
// guard tests the steps of C only.  The guard takes no branch: the steps behind a bad pivot execute, on values nobody reads — the solve
// writes nothing but `out`, and the caller reads nothing of `out` once the flag is set.  8 VGPRs of matrix per lane: with a whole row
// per lane (32) the chain kernel of T = 16 spilled.
// basm: the basis flags of the 16 variables (bit k: variable 16 KC + k is basic).
// out, indexed by k: [0..16) a_k (0 outside C), [16..32) q'_k (meaningful on C), [33] != 0: an entering pivot at or below the guard, or a
// pivot that is not finite (nothing else of `out` is then meaningful); [PAIR_XCH, PAIR_XCH + 16): the exchange
// The lanes of ONE wave exchange through LDS: the hardware executes a wave's LDS operations in order, so a store is seen by the loads
// behind it without a wait; the fences only keep the compiler from moving a lane's load above another lane's store, or the next step's
// store above this step's loads (they emit no s_waitcnt).  No __syncthreads() here: the barrier invariant above batch_select
#define PAIR_XCH_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                             __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
template <int CW, int RS, int KC>
__device__ __forceinline__ void pair_solve(const double *P, unsigned cm, unsigned basm, int lane, int rhspos, double *out STAMP_PARAMS)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    const int r = lane & 15, h = lane >> 4;
    const int pos = r * RS + KC;
    double pv[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) pv[jj] = P[(4 * h + jj) * CW + pos];
    double qc = P[r * CW + rhspos];
    // the exchange's two addresses, opaque: one VGPR each through the steps (else the compiler forms them again at every use)
    int xro = 8 * r, xuo = 32 * h;
    asm volatile("" : "+v"(xro), "+v"(xuo));
    double *const xr = reinterpret_cast<double *>(reinterpret_cast<char *>(out + PAIR_XCH) + xro);               // this row's entry of the pivot column
    const d2 *const xu = reinterpret_cast<const d2 *>(reinterpret_cast<char *>(out + PAIR_XCH) + xuo);           // the pivot row's entries of this lane's four columns
    // the guard, without a branch: the smallest high word of an entering pivot and the largest exponent field of any pivot, judged once
    // behind the steps.  The steps behind a bad pivot compute on values nobody reads (`out` is not read once the flag is set)
    int dlo = 0x7fffffff, dex = 0;
    STAMP(16);
#pragma unroll
    for (int s = 0; s < PAIR_MAXC; ++s) {
        const int hq = s >> 2, jj = s & 3;
        if (!((cm >> s) & 1u)) continue;                        // (wave-uniform: a scalar branch)
        const double d = readlane_f64(pv[jj], 16 * hq + s);
        const int dh = __double2hiint(d);                       // (wave-uniform: scalar arithmetic)
        dlo = min(dlo, ((basm >> s) & 1u) ? 0x7fffffff : dh);
        dex = max(dex, dh & F64_EXP_HI);
        if (h == hq) *xr = pv[jj];
        PAIR_XCH_SYNC();
        const double pvs = *xr;
        const d2 u01 = xu[0], u23 = xu[1];                      // from the pivot COLUMN (panel_block's NUMERICS)
        PAIR_XCH_SYNC();
        const double u[4] = {u01.x, u01.y, u23.x, u23.y};
        const double inv = rcp_newton(d), ainv = fabs(inv);
        const double fz = -pvs * inv;
        const double qs = readlane_f64(qc, s);
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) pv[j2] = fma(fz, u[j2], pv[j2]);
        qc = fma(fz, qs, qc);
        // the pivot column and the pivot row, as fix-ups under EXEC (the empty asm keeps the compiler from turning them into selects)
        if (h == hq) { asm volatile(""); pv[jj] = pvs * ainv; }
        if (r == s) {
            asm volatile("");
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) pv[j2] = u[j2] * ainv;
            qc = qs * ainv;
            if (h == hq) pv[jj] = -inv;
        }
    }
    const bool hard = !(dlo > PAIR_PIV_MIN_HI) || dex == F64_EXP_HI;
    STAMP(17);
    if (lane < PAIR_MAXC) {
        const bool in_c = (cm >> lane) & 1u;
        out[PAIR_MAXC + lane] = qc;
        out[lane] = in_c ? (((basm >> lane) & 1u) ? -qc : qc) : 0.0;
    }
    if (lane == 0) out[2 * PAIR_MAXC + 1] = hard ? 1.0 : 0.0;
}

#define PARTLS_CASES(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16) M(17) M(18) M(19)

// NODE: node mode (Alt alpha-steps, BnB bounds: one subproblem per chain, free / zero groups) is a separate instantiation, so
// that the chain-mode sweep carries neither the node pointers nor the per-thread `free` flag through its loops.
// MODELS (chain mode only, partls_opt_models): every finished pattern leaves its scaled solution (basic ? q : 0, node_sol's format) in
// row g - g_begin of p.node_sol (leading dimension p.node_ld) and sqrt(obj2) in p.node_obj2[g - g_begin]; a pattern that hit the pivot
// cap leaves NaN in both.  The row follows from the chain and pattern counters alone (no live register beyond the default build's); the
// export instantiation writes no best_sol.  A separate instantiation: the default ones keep their code.
template <int T, int H, bool NODE, int W = 2, bool MODELS = false, bool BATCH = false, bool PAIRK = false>
__device__ __forceinline__ void sweep_body(const SweepParams &p)
{
    using L = Half<T, H, W>;
    constexpr int RS = L::RS, CW = L::CW, RHSPOS = 16 * RS, NW = (T + 3) / 4;      // NW: 64-bit mask words that can be non-empty
    constexpr int THREADS = L::NT;                                                  // shadows the namespace constant
    constexpr int MB = W == 1 ? blk::MB : MBB;                                      // pivots per block of this kernel (shadows the namespace constant)
    // MERGED: the merged KKT scan (below); LANE_MASKS: the round's tile-column masks live in a VGPR (see the exchange).  Both only where the
    // allocation takes them without new spills (profiles/r05_sweep_resource_usage.txt): with the merged scan the chain kernel of T = 18 spills
    // 25 VGPRs instead of 22 and the batch instantiations spill at T = 7, 8 and from 17 on, with the masks the chain kernel of T = 17 spills 2
    // — those keep the one-scan-per-decision loop and the LDS reads, and with them their former allocation.
    static_assert(!(NODE && MODELS), "node mode exports no per-pattern models (finish_pattern's capped flag is chain mode's)");
    constexpr bool MERGED = PARTLS_MERGED_SCAN && !NODE && !BATCH && T <= 17;
    constexpr bool LANE_MASKS = PARTLS_LANE_MASKS && !BATCH && T <= 16;
    // PAIR: the pair walk — chain mode of the 512-thread kernel wherever both of the above are on, i.e. up to T = 16 (T = 17
    // has no lane-held masks; from T = 18 on the chain kernel spills as it is and stays unpaired).  An instantiation of its own (PAIRK),
    // launched when SweepParams::pair is set: compiled into the one chain kernel and switched at run time, the walk costs the plain one
    // 3 % (C3 sweep 49.3 against 47.8 ms with the pairing off: the pricing's edges in the round loop move its code and 5 VGPRs).
    constexpr bool PAIR = PAIRK && PARTLS_PAIR && MERGED && LANE_MASKS && W == 2 && !MODELS;
    static_assert(PAIR == PAIRK, "the pair walk is launched only where it is compiled (pair_compiled)");
    static_assert(W == 2 || RHSPOS < 256, "the 256-thread kernel needs every panel row position (and the rhs row) below 256");
    auto &lds_image = *image_of<W>();
    const int tid = threadIdx.x, t8 = tid & 255, a = t8 & 15, b = t8 >> 4, lane = tid & 63, wave = tid >> 6;
    const int n = p.n;
    const int nwords = (n + 63) >> 6;

    // link-time constant addresses into the LDS image
    double *const Pbase = lds_image.Pbase, *const Z = lds_image.Z, *const U = lds_image.U, *const Dinv = lds_image.Dinv;
    unsigned long long *const s_inf = lds_image.s_inf, *const s_bas = lds_image.s_bas, *const s_vmask = lds_image.s_vmask;
    unsigned long long *const s_sum = lds_image.s_sum;
    int *const s_veto = lds_image.s_veto;
    double *const s_best = lds_image.s_best;
    // pair walk: U and Dinv are idle while a twin is priced (the panel steps rewrite what they read) and lie in the first 64 KB — fields of
    // their own behind the panel each cost an address register that lives through the whole kernel.  s_pair: the solve's results (pair_solve's
    // `out`); s_tw[w]: wave w still sees a violator; s_cm: the twin's violators, one bit per variable of the pair column, in the low half and
    // the basis flags of the column's variables in the high half
    [[maybe_unused]] double *const s_pair = U;
    [[maybe_unused]] int *const s_tw = reinterpret_cast<int *>(Dinv);
    [[maybe_unused]] int *const s_cm = s_tw + 8;
    static_assert(PAIR_MAXC == 16, "the pair column is one tile column: 16 variables, one mask bit each");
    static_assert(2 * (MB + 64) >= PAIR_XCH + PAIR_MAXC && PAIR_XCH >= 2 * PAIR_MAXC + 2, "pair_solve's `out` and its exchange (doubles) fit U");
    static_assert((sizeof(lds_image.Z) + PAIR_XCH * sizeof(double)) % 16 == 0, "the exchange is read 16 bytes at a time");
    static_assert(2 * (MB + 64) >= 9, "s_tw and s_cm (9 ints) fit Dinv (MB + 64 doubles)");
    for (int i = tid; i < 2 * MB * CW; i += THREADS) Pbase[i] = 0.0;                   // padding rows are never gathered
    for (int i = tid; i < MB * CW; i += THREADS) Z[i] = 0.0;
    if (tid < 2 * (MB + 64)) U[tid] = 0.0;
    if (tid < MB + 64) Dinv[tid] = 0.0;
    if (tid < 32) s_inf[tid] = 0;                                                      // both sets
    if (tid < 16) { s_bas[tid] = 0; s_sum[tid] = 0; }
    if (tid < 2) s_veto[tid] = NO_VETO;
    if (tid == 0) {
        s_best[0] = __builtin_inf(); reinterpret_cast<long long *>(s_best)[1] = -1;
        s_best[2] = __builtin_inf(); reinterpret_cast<long long *>(s_best)[3] = -1;
    }
    if (tid < 16 * T) s_vmask[tid] = tid < p.n ? p.mask[tid] : 0ULL;
    if (tid < 64) lds_image.s_rbit[tid] = tid < 40 ? p.rbit.gbit[tid] : 0;
    __syncthreads();

    double S[L::CNT];
    double q = 0.0, corner = 0.0;
    double mybest = __builtin_inf();                      // chain mode: objective^2 of the pattern whose solution sits in p.best_sol
    const bool has_var = tid < n;
    bool basic = false, blocked = false;
    const int mypos = (tid & 15) * RS + (tid >> 4);       // panel row position of variable `tid` (tid < 16 T)
    // panel phase: this thread owns row position `tid`, i.e. variable 16*rowrho + rowc (valid when rowc < 16)
    const int rowc = tid / RS, rowrho = tid - rowc * RS;
    const bool idle_wave = __builtin_amdgcn_readfirstlane((tid & ~63) > RHSPOS ? 1 : 0) != 0;   // no panel row in this wave

    unsigned npiv = 0, nunconv = 0, nveto = 0;            // per workgroup: far below 2^32
    unsigned bc = 0, sc = 0;                              // block / scan counters (double-buffer parity)

    // 32-bit loop state (the host guarantees nchains < 2^31 and chain_len < 2^31): every 64-bit scalar held across the pattern loop is
    // an SGPR pair the allocator spills to a VGPR lane and reloads
    const int clen = (int)p.chain_len;
    const int nchains = (int)((p.g_end - p.g_begin + clen - 1) / clen);

    STAMP_DECL
    for (int chain = blockIdx.x; chain < nchains; chain += gridDim.x) {
        const int64_t g0 = p.g_begin + (int64_t)chain * clen;
        const int glen = (int)((g0 + clen < p.g_end) ? clen : p.g_end - g0);
        STAMP(5);
        const double *src = p.T0;
        if constexpr (NODE) {                                         // warm start from a snapshot (BnB children), wave-uniform
            if (p.node_src) {
                const double *snap = p.node_src[chain];
                if (snap) src = snap;
            }
        }
        // One wave-uniform base per PAIR of slots, opaque to the optimiser, + the thread's constant element offset + an immediate: left
        // alone, LLVM hoists the CNT per-slot address offsets out of the chain loop as CNT live VGPRs, spills them, and every load / store of
        // a chain start or snapshot then waits for its own scratch reload (`scratch_load; s_waitcnt vmcnt(0); global_store` 76 times: 35 us
        // per snapshot, 85 % of a warm-started BnB node — found in the round-4 kernel trace of the node batches)
        {
            const double *bp = uniform_ptr(src) + (size_t)L::OFF * 256;
#pragma unroll
            for (int s = 0; s < L::CNT; ++s) {
                if ((s & 1) == 0) asm volatile("" : "+s"(bp));
                S[s] = bp[(s & 1) * 256 + t8];
                if (s & 1) bp += 512;
            }
        }
        q = (tid < 16 * T) ? src[(size_t)nslots(T) * 256 + tid] : 0.0;
        corner = src[(size_t)nslots(T) * 256 + 16 * T];
        basic = false;
        if constexpr (NODE) {
            if (src != p.T0 && tid < 16 * T) basic = reinterpret_cast<const int8_t *>(src + (nslots(T) * 256 + 16 * T + 8))[tid] != 0;
        }
        STAMP(6);

        // ONE loop over the exchange rounds of the whole chain.  In chain mode every KKT scan evaluates two predicates on the same rhs column
        // and basis: `bad` under the signs f of the pattern being solved and `nxt` under the signs fn of its successor in the chain, with no
        // column rejected — what the successor's first scan would see, since nothing touches the tableau between the scan that finds a
        // pattern solved and the first scan of the next one.  The confirming scan of pattern g therefore IS the first scan of g + 1: its
        // second summary and mask words (s_inf set 1) start the exchange of g + 1 directly, one scan (two ballots' worth of LDS words, a
        // barrier and a reduction) less per pattern, the same violators round for round.  Node mode takes its codes per node from global
        // memory and keeps one scan per decision (!MERGED, as do the instantiations listed at MERGED above): there the second predicate is
        // not compiled and every pattern starts with a scan — the round loop ends with the pattern and the loop around it starts the next one
        // (with MERGED that outer loop runs once; with a node's bookkeeping and the next node's codes inside the round loop the node-mode
        // kernel spills 421 VGPRs at T = 16).
        // bookkeeping of a finished pattern (converged, or capped: it hit the pivot cap); touches no tile slot
        auto finish_pattern = [&](int gi, [[maybe_unused]] bool capped) {
            const uint64_t g = (uint64_t)g0 + (unsigned)gi;
            const uint64_t pat = NODE ? (uint64_t)chain : g ^ (g >> 1);
            // patterns are ranked on objective^2 (the tableau corner; sqrt is monotone): one sqrt per workgroup instead of one per
            // pattern, unless every pattern's objective is wanted
            const double obj2 = corner > 0.0 ? corner : 0.0;
            // bookkeeping of the finished pattern: by the last thread — its wave owns no panel row and has slack, wave 0 has none
            if constexpr (NODE) {                                     // chain of nodes (bit-order calibration): pivots, blocks, scans so far
                if (p.node_piv && tid == 0) {
                    unsigned *o = p.node_piv + 3 * ((size_t)chain * clen + gi);
                    o[0] = npiv; o[1] = bc; o[2] = sc;
                }
            }
            if (p.all_opt && tid == THREADS - 1) p.all_opt[pat] = sqrt(obj2);
            if constexpr (MODELS) {
                const size_t row = (size_t)chain * (size_t)clen + (size_t)gi;
                if (has_var) p.node_sol[row * p.node_ld + tid] = capped ? __builtin_nan("") : (basic ? q : 0.0);
                if (tid == THREADS - 1) p.node_obj2[row] = capped ? __builtin_nan("") : sqrt(obj2);
            }
            if constexpr (!NODE && !MODELS && (W == 1 || (PARTLS_EXPORT_BIG && T <= EXPORT_MAXT))) {
                // (round 3: 256-thread kernel only — in the 512-thread kernel the two extra live registers moved 8 spills and cost 1.8 % of the
                // C3 sweep.  Round 4: the spills turned out to be hoisted address offsets and are gone; -DPARTLS_EXPORT_BIG=1 measures it again)
                // the workgroup's best pattern so far leaves its solution behind (rhs column of the basic variables, as node mode's
                // node_sol): the host takes the winner's from here instead of solving that pattern again from the empty basis.  Every
                // thread decides for itself on the replicated corner; on exact objective ties the FIRST pattern's solution stays (the
                // host checks the solution against the winning pattern's signs and re-solves if they disagree).
                if (p.best_sol && obj2 < mybest) {
                    mybest = obj2;
                    if (has_var) p.best_sol[(size_t)blockIdx.x * p.node_ld + tid] = basic ? q : 0.0;
                }
            }
            // the ranking of rank_pattern (sweep_rules.h) on objective^2 held in LDS, in this kernel's own form: it has no `best_pat >= 0` guard
            // lexicographic (objective, pattern) minimum and runner-up: argmin's first-index rule for both.  The minimum is never above the
            // runner-up, so a pattern above the runner-up — nearly every one — is done after one comparison
            if (tid == THREADS - 1 && obj2 <= s_best[2]) {
                const double bo = s_best[0];
                const long long bp = reinterpret_cast<long long *>(s_best)[1];
                if (obj2 < bo || (obj2 == bo && ref_index_less(pat, (unsigned long long)bp, lds_image.s_rbit))) {
                    s_best[2] = bo; reinterpret_cast<long long *>(s_best)[3] = bp;             // the old minimum becomes the runner-up
                    s_best[0] = obj2; reinterpret_cast<long long *>(s_best)[1] = (long long)pat;
                } else if (obj2 < s_best[2] || ref_index_less(pat, (unsigned long long)reinterpret_cast<long long *>(s_best)[3], lds_image.s_rbit)) {
                    s_best[2] = obj2; reinterpret_cast<long long *>(s_best)[3] = (long long)pat;     // (equal to the runner-up's here)
                }
            }
        };
        // the same bookkeeping for a pattern the tableau does not hold — a twin of the pair walk (PAIR: chain mode, no export of models): its
        // objective^2, this thread's rhs entry and basis flag come as values (the twin's temporaries, or the tableau's own where C is empty).
        // A recorder of its own: with these three as parameters of finish_pattern the node-mode kernels, which never price, lose their allocation
        [[maybe_unused]] auto record_twin = [&](int gi, double cornerv, double qv, bool bv) {
            const uint64_t g = (uint64_t)g0 + (unsigned)gi;
            const uint64_t pat = g ^ (g >> 1);
            const double obj2 = cornerv > 0.0 ? cornerv : 0.0;
            if (p.all_opt && tid == THREADS - 1) p.all_opt[pat] = sqrt(obj2);
            if constexpr (PARTLS_EXPORT_BIG && T <= EXPORT_MAXT) {
                if (p.best_sol && obj2 < mybest) {
                    mybest = obj2;
                    if (has_var) p.best_sol[(size_t)blockIdx.x * p.node_ld + tid] = bv ? qv : 0.0;
                }
            }
            if (tid == THREADS - 1 && obj2 <= s_best[2]) {           // finish_pattern's ranking
                const double bo = s_best[0];
                const long long bp = reinterpret_cast<long long *>(s_best)[1];
                if (obj2 < bo || (obj2 == bo && ref_index_less(pat, (unsigned long long)bp, lds_image.s_rbit))) {
                    s_best[2] = bo; reinterpret_cast<long long *>(s_best)[3] = bp;
                    s_best[0] = obj2; reinterpret_cast<long long *>(s_best)[1] = (long long)pat;
                } else if (obj2 < s_best[2] || ref_index_less(pat, (unsigned long long)reinterpret_cast<long long *>(s_best)[3], lds_image.s_rbit)) {
                    s_best[2] = obj2; reinterpret_cast<long long *>(s_best)[3] = (long long)pat;
                }
            }
        };
        int gi = 0;
        // ---- pair walk (PAIR) ----------------------------------------------------------------------------------------
        // Patterns g and g ^ 1 (Gray indices) differ in internal bit 0 only: a PAIR when both lie in the chain.  The tableau visits ONE
        // member per pair — the one whose bit 0 is the committed state's, so a step from pair to pair flips one group on a bit >= 1 — and
        // once that member is confirmed its twin is PRICED from the columns of its violators C: nothing of the tableau is written.  A twin
        // that pricing cannot finish (a small entering pivot, violators left after the block pivot on C; more than PAIR_MAXC violators do not
        // occur: C lies in the one tile column the host gave the group on bit 0, and with a wider group the walk is off) is
        // solved by the ordinary rounds from the current tableau instead; a pattern without its partner in the chain (odd chain ends) is
        // an ordinary pattern.  All of this state is wave-uniform and the same in both halves (the barrier invariant below).
        [[maybe_unused]] bool tw_pending = false;                         // the pattern being solved has a twin that is still to come
        // index of the partner of chain pattern i, -1 if it has none
        [[maybe_unused]] auto pair_partner = [&](int i) -> int {
            const int j = (((unsigned)g0 + (unsigned)i) & 1u) ? i - 1 : i + 1;
            return (PAIR && j >= 0 && j < glen) ? j : -1;
        };
        [[maybe_unused]] auto pair_unit_end = [&](int i) -> int { const int j = pair_partner(i); return (j > i ? j : i) + 1; };
        // the pattern the tableau visits of the unit that starts at chain index u, with the committed state at chain pattern i
        [[maybe_unused]] auto pair_target = [&](int u, int i) -> int {
            const unsigned gu = (unsigned)g0 + (unsigned)u, gc = (unsigned)g0 + (unsigned)i;
            if (pair_partner(u) < 0 || (gu & 1u)) return u;
            return (((gu >> 1) ^ gu ^ (gc >> 1) ^ gc) & 1u) ? u + 1 : u;      // bit 0 of gray(g) = bit 0 of g ^ (g >> 1)
        };
        // after pattern gi: on to its twin (`to_twin`: by the ordinary rounds), or to the next unit; false: the chain is finished
        [[maybe_unused]] auto pair_next = [&](bool to_twin, int &f, int &fn) -> bool {
            if (to_twin) gi = pair_partner(gi);
            else {
                const int u = pair_unit_end(gi);
                if (u >= glen) return false;
                gi = pair_target(u, gi);
            }
            tw_pending = !to_twin && pair_partner(gi) >= 0;
            const uint64_t vmask = s_vmask[tid < 16 * T ? tid : 0] & (has_var ? ~0ULL : 0ULL);
            const uint64_t g = (uint64_t)g0 + (unsigned)gi;
            f = sign_of_var(vmask, g ^ (g >> 1));
            const int u2 = pair_unit_end(gi);                             // the merged scan looks ahead to the next pattern the TABLEAU visits
            fn = f;
            if (u2 < glen) { const uint64_t gn = (uint64_t)g0 + (unsigned)pair_target(u2, gi); fn = sign_of_var(vmask, gn ^ (gn >> 1)); }
            return true;
        };
        for (;;) {                                                    // !MERGED: one turn per pattern; MERGED: one turn
            [[maybe_unused]] const unsigned nunconv0 = nunconv;           // !MERGED: did this pattern hit the pivot cap?
            bool isfree = false;
            int f = 0;
            [[maybe_unused]] int fn = 0;                                  // chain mode: the sign of this variable under pattern gi + 1 (the last pattern of a chain: f)
            if constexpr (NODE) {                                         // node mode: chain index = node index, per-variable codes
                const int code = has_var ? (int)p.node_code[((size_t)chain * clen + gi) * p.node_ld + tid] : 0;   // a chain of nodes: warm start
                isfree = code == 2;
                f = isfree ? 0 : code;
            } else {
                const uint64_t vmask = s_vmask[tid < 16 * T ? tid : 0] & (has_var ? ~0ULL : 0ULL);
                const uint64_t g = (uint64_t)g0 + (unsigned)gi, gn = g + 1;                 // MERGED: gi = 0 here
                f = sign_of_var(vmask, g ^ (g >> 1));
                if constexpr (MERGED) fn = glen > 1 ? sign_of_var(vmask, gn ^ (gn >> 1)) : f;
                if constexpr (PAIR) {                                     // gi = 0: the chain's first pattern is visited whatever its bit 0
                    tw_pending = pair_partner(0) >= 0;
                    const int u2 = pair_unit_end(0);
                    fn = f;
                    if (u2 < glen) { const uint64_t g2 = (uint64_t)g0 + (unsigned)pair_target(u2, 0); fn = sign_of_var(vmask, g2 ^ (g2 >> 1)); }
                }
            }
            blocked = false;
            int ninf_best = n + 1, patience = 3, rounds = 0;
            bool progress = false;                                        // did the previous round change the basis?
            for (;;) {
                // ---- KKT scan of the rhs column (registers) ------------------------------------------------------------
                // a column rejected as dependent is only dependent on the basis it was tested against (Lawson–Hanson
                // re-examines it after any exchange): forget the rejections once the basis has changed
                if (progress) blocked = false;
                progress = false;
                const int par = sc & 1;
                ++sc;
                bool bad = false;
                [[maybe_unused]] bool nxt = false;
                if (has_var) {                                            // kkt_violates<NODE> (sweep_rules.h), written out: see the exchange rule below
                    const double fq = q * (double)(f > 1 ? 1 : (f < -1 ? -1 : f));     // sign(f) * q  (|f| = 2: feature of two groups)
                    if (NODE && isfree) bad = !basic && !blocked && (fabs(q) > p.tol);     // free: stationarity only
                    else if (basic) bad = (f == 0) || (fq < -p.tol);
                    else bad = (fq > p.tol) && !blocked;
                    if constexpr (MERGED) {                               // the same test under the next pattern's signs; a pattern starts with no rejections
                        const double fqn = q * (double)(fn > 1 ? 1 : (fn < -1 ? -1 : fn));
                        nxt = basic ? ((fn == 0) || (fqn < -p.tol)) : (fqn > p.tol);
                    }
                }
                const unsigned long long bb = __ballot(bad), bs = __ballot(basic);
                // every wave condenses ITS mask word before the barrier (count in bits 0..7, one bit per 16-variable tile column in
                // bits 8..11), so that after it each wave combines NW small words instead of re-deriving everything from NW masks
                unsigned summ = (unsigned)__popcll(bb);
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
                    if ((bb >> (16 * sub)) & 0xFFFFull) summ |= 0x100u << sub;
                if constexpr (!MERGED) {
                    if (lane == 0 && wave < nwords) { s_inf[par * 8 + wave] = bb; s_bas[par * 8 + wave] = bs; s_sum[par * 8 + wave] = summ; }
                } else {
                    const unsigned long long bn = __ballot(nxt);
                    unsigned summ2 = (unsigned)__popcll(bn);
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub)
                        if ((bn >> (16 * sub)) & 0xFFFFull) summ2 |= 0x100u << sub;
                    if (lane == 0 && wave < nwords) {
                        s_inf[par * 8 + wave] = bb; s_inf[16 + par * 8 + wave] = bn; s_bas[par * 8 + wave] = bs;
                        s_sum[par * 8 + wave] = ((unsigned long long)summ2 << 32) | summ;
                    }
                }
                STAMP(9);
                __syncthreads();
                STAMP(10);
                int count = 0;
                unsigned tiles = 0;
                [[maybe_unused]] int count2 = 0;
                [[maybe_unused]] unsigned tiles2 = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const unsigned long long sw2 = s_sum[par * 8 + w];                                       // 0 for w >= nwords
                    const unsigned sw = (unsigned)__builtin_amdgcn_readfirstlane((int)sw2);
                    count += (int)(sw & 0xFFu);
                    tiles |= (sw >> 8) << (4 * w);
                    if constexpr (MERGED) {
                        const unsigned sn = (unsigned)__builtin_amdgcn_readfirstlane((int)(sw2 >> 32));
                        count2 += (int)(sn & 0xFFu);
                        tiles2 |= (sn >> 8) << (4 * w);
                    }
                }
                STAMP(0);
                // ExchangeRule::next (sweep_rules.h), written out: through the helpers the same rules compile to the same VGPR count but
                // move 2-4 spilled SGPRs, and this kernel is tuned to the register.  Keep both in step with sweep_rules.h by hand.
                // Everything below up to the exchange is decided from count / count2 / rounds / gi: LDS words and kernel arguments that are the
                // same for all threads of both halves (the barrier invariant above batch_select).
                int soff = par * 8;                                       // the mask words this round exchanges: s_inf set 0 (+ 16: set 1)
                bool all = true;
                bool done = count == 0;
                if (!done) {
                    if (count < ninf_best) { ninf_best = count; patience = 3; }
                    else if (patience > 0) --patience;
                    else all = false;                                     // backup rule: only the largest violator
                    if (++rounds > p.max_rounds) { ++nunconv; done = true; }
                }
                if (done) {
                    // ---- pattern gi is finished (converged, or the pivot cap: count != 0) ---------------------------------------
                    if constexpr (!MERGED) break;                         // the turn of the outer loop ends
                    finish_pattern(gi, count != 0);
                    if constexpr (PAIR) {
                        // 0: no twin to come (second member of a pair, a pattern without partner), or the twin is priced and recorded
                        // 2: the twin goes to the ordinary rounds
                        int tw = 0;
                        if (tw_pending) {
                            tw = 2;                                   // (a capped pattern's pair is finished by the ordinary path)
                            if (count == 0) {
                                // ---- pricing the twin of pattern gi: a routine of its own, outside the exchange loop --------------------------
                                // The host has laid every live variable of the group on bit 0 into tile column KC (pair_relayout, sweep_setup.hip),
                                // so the twin's violators C — variables whose sign bit 0 changes — are among the 16 variables of that column: the
                                // tile slots to gather are the same in every pattern (static register indices, immediate LDS offsets) and the
                                // twin's scan is 16 lanes' worth of rhs entries.  ALL 16 columns go to the two panel buffers (both idle at a
                                // confirmed pattern), the rhs row with them, under the barrier that publishes the violator mask; the solve, the
                                // rows and the confirming scan then restrict themselves to C.  Nothing of the tableau is written.
                                constexpr int KC = T - 2, WQ = (16 * KC) >> 6, SHQ = (16 * KC) & 63;
                                static_assert(KC >= L::G, "the pair column's tile slots all lie in half 1");
                                // the thread's coordinates once more, opaque: everything derived from `tid` itself is hoisted out of the chain loop
                                // and held in registers through the whole kernel (lane masks, row positions: 8 spilled VGPRs at T = 16)
                                int tidp = tid;
                                asm volatile("" : "+v"(tidp));
                                const int lanep = tidp & 63, wavep = __builtin_amdgcn_readfirstlane(tidp >> 6), kp = tidp & 15;
                                const bool mine = (tidp >> 4) == KC;      // this thread holds the rhs entry of variable 16 KC + kp
                                const uint64_t vmask = s_vmask[tidp < 16 * T ? tidp : 0] & (has_var ? ~0ULL : 0ULL);
                                const uint64_t gt = (uint64_t)g0 + (unsigned)pair_partner(gi);
                                const int ft = sign_of_var(vmask, gt ^ (gt >> 1));
                                gather_tile<T, H, W, KC>(S, Pbase, a, b, 0xFFFFu);
                                if (mine) Pbase[kp * CW + RHSPOS] = q;
                                if (H == 0 && wavep == WQ) {              // the one wave that holds the pair column's rhs entries
                                    const double fqt = q * (double)(ft > 1 ? 1 : (ft < -1 ? -1 : ft));
                                    const bool badt = mine && has_var && (basic ? ((ft == 0) || (fqt < -p.tol)) : (fqt > p.tol));   // kkt_violates (sweep_rules.h), written out
                                    const unsigned cmw = (unsigned)(__ballot(badt) >> SHQ) & 0xFFFFu;
                                    const unsigned basw = (unsigned)(__ballot(basic) >> SHQ) & 0xFFFFu;     // this wave's word of s_bas, at the column
                                    if (lanep == 0) s_cm[0] = (int)(cmw | (basw << 16));
                                }
                                __syncthreads();
                                STAMP(15);
                                const unsigned cmb = (unsigned)__builtin_amdgcn_readfirstlane(s_cm[0]);
                                const unsigned cm = cmb & 0xFFFFu;
                                if (cm == 0) {                        // C is empty: the twin's optimum is the current corner
                                    record_twin(pair_partner(gi), corner, q, basic);
                                    tw = 0;
                                } else {
                                    // One wave solves while the other seven wait at the barrier: nothing else of the pricing can start before the
                                    // coefficients exist (every row's FMAs need all of them).  Wave 3, of half 0 rather than the blocks' idle wave of
                                    // half 1: half 0 holds fewer tile slots (66 against 70 at T = 16), so the solve's live registers land where the
                                    // allocation has room.
                                    if (H == 0 && wavep == 3) pair_solve<CW, RS, KC>(Pbase, cm, cmb >> 16, lanep, RHSPOS, s_pair STAMP_ARGS);
                                    else STAMP(16);               // (the other waves' stamps: all of the solve is their wait, 18)
                                    __syncthreads();
                                    STAMP(18);
                                    const bool guard = __builtin_amdgcn_readfirstlane(__double2hiint(s_pair[2 * PAIR_MAXC + 1])) != 0;
                                    // Every thread forms its twin rhs entry: the pivot rows take the solve's, the others 16 FMAs on their own panel row, in
                                    // ascending k — a term outside C has a_k = 0 and leaves the sum as it is, bit for bit.  The objective (the rhs row's
                                    // own entry) is a second chain of the same form.  The coefficients are wave-uniform: lane k of every row of 16
                                    // lanes reads -a_k and the rhs row's q_k ONCE, and the FMAs take them as DPP row broadcasts (sweep_lazy.hip's
                                    // lz_fmac_bcast); each thread's own 16 panel entries are reads at immediate offsets of one address.
                                    const bool in_c = mine && ((cm >> kp) & 1u);
                                    double qt = q, cornert = corner;
                                    {
                                        const double *prow = Pbase + (tidp < 16 * T ? kp * RS + (tidp >> 4) : RHSPOS);
                                        const double na = -s_pair[kp], qk = Pbase[kp * CW + RHSPOS];
                                        double tq;
                                        // (inline asm: the compiler pads no hazard of a DPP operand — a VGPR written by the VALU needs two wait states
                                        // before a DPP instruction reads it, an EXEC written by the VALU five)
#define PARTLS_ROW(K, PAD) asm volatile("s_nop " #PAD "\n\t" \
                                          "v_mov_b64_dpp %2, %4 row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n\t" \
                                          "v_fmac_f64_dpp %0, %3, %5 row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n\t" \
                                          "s_nop 0\n\t" \
                                          "v_fmac_f64_dpp %1, %3, %2 row_newbcast:" #K " row_mask:0xf bank_mask:0xf" \
                                          : "+v"(qt), "+v"(cornert), "=&v"(tq) : "v"(na), "v"(qk), "v"(pk[K]));
                                        // (an asm statement is a barrier to the scheduler: all 16 reads are issued ahead of the FMAs, one round trip; the
                                        // allocation takes the 32 registers — they are dead again before the tableau is touched)
                                        double pk[PAIR_MAXC];
#pragma unroll
                                        for (int k = 0; k < PAIR_MAXC; ++k) pk[k] = prow[k * CW];
                                        PARTLS_ROW(0, 4) PARTLS_ROW(1, 1) PARTLS_ROW(2, 1) PARTLS_ROW(3, 1) PARTLS_ROW(4, 1) PARTLS_ROW(5, 1)
                                        PARTLS_ROW(6, 1) PARTLS_ROW(7, 1) PARTLS_ROW(8, 1) PARTLS_ROW(9, 1) PARTLS_ROW(10, 1) PARTLS_ROW(11, 1)
                                        PARTLS_ROW(12, 1) PARTLS_ROW(13, 1) PARTLS_ROW(14, 1) PARTLS_ROW(15, 1)
#undef PARTLS_ROW
                                    }
                                    if (in_c) qt = s_pair[PAIR_MAXC + kp];
                                    STAMP(19);
                                    const bool bt = basic != in_c;
                                    const double fqt = qt * (double)(ft > 1 ? 1 : (ft < -1 ? -1 : ft));
                                    const bool bad2 = has_var && (bt ? ((ft == 0) || (fqt < -p.tol)) : (fqt > p.tol));   // kkt_violates (sweep_rules.h), written out
                                    const unsigned long long b2 = __ballot(bad2);
                                    if (lanep == 0) s_tw[wavep] = b2 != 0ull;
                                    __syncthreads();
                                    int left = guard ? 1 : 0;
#pragma unroll
                                    for (int w = 0; w < 8; ++w) left |= s_tw[w];
                                    left = __builtin_amdgcn_readfirstlane(left);
                                    // easy: the block pivot on C is the whole story — recorded as finish_pattern records; else nothing of the pricing
                                    // is kept.  Either way the confirming scan's look-ahead still holds: the next pattern starts from it below
                                    if (!left) { record_twin(pair_partner(gi), cornert, qt, bt); tw = 0; }
                                }
                                STAMP(20);                            // (16 .. 20: the pricing behind the scan, STAMP 14 of the earlier records)
                            }
                        }
                        if (tw == 2) {                                // a fresh scan starts the twin
                            if (!pair_next(true, f, fn)) break;
                            blocked = false;
                            ninf_best = n + 1; patience = 3; rounds = 0;
                            continue;
                        }
                    }
                    {
                    // ---- ... and the next one starts: from this very scan where it can ---------------------------------------------
                    if constexpr (PAIR) { if (!pair_next(false, f, fn)) break; }       // (f and fn: the next visited pattern's and its successor's)
                    else if (++gi >= glen) break;
                    blocked = false;
                    ninf_best = n + 1; patience = 3; rounds = 0;
                    if constexpr (MERGED) {
                        if constexpr (!PAIR) {
                        const uint64_t vmask = s_vmask[tid < 16 * T ? tid : 0] & (has_var ? ~0ULL : 0ULL);
                        const uint64_t gn = (uint64_t)g0 + (unsigned)gi + 1;
                        f = fn;
                        fn = gi + 1 < glen ? sign_of_var(vmask, gn ^ (gn >> 1)) : f;
                        }
                        // count2 == 0: the new pattern is optimal as it stands — the next scan records it (and looks one pattern further)
                        if (count2 == 0 || p.max_rounds < 1) continue;
                        ninf_best = count2; rounds = 1;                   // ExchangeRule::next of a first round: count2 < n + 1, 1 <= max_rounds
                        all = true;
                        tiles = tiles2;
                        soff += 16;
                    }
                    }
                }
                int single_k = -1;
                if (!all) {                                               // rare: the largest violator, from the mask words themselves
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        unsigned long long ww = s_inf[par * 8 + w];
                        ww = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(ww >> 32)) << 32) |
                             (unsigned)__builtin_amdgcn_readfirstlane((int)ww);
                        if (ww) single_k = (w << 6) + 63 - __builtin_clzll(ww);
                    }
                    tiles = 1u << (single_k >> 4);
                }
                tiles = (unsigned)__builtin_amdgcn_readfirstlane((int)tiles);
                // lane t of every wave keeps the violator and basis masks of tile column t (16 + 16 bits) for the round: one v_readlane per
                // tile column instead of two LDS reads, a wait and 64-bit shifts (LANE_MASKS: up to T = 16 — with the extra live register the
                // chain-mode kernel of T = 17 would spill 2 VGPRs, so from there on the masks come from LDS per tile column)
                [[maybe_unused]] unsigned tmask = 0;
                if constexpr (LANE_MASKS) {
                    const int tl = lane < T ? lane : 0, wl = tl >> 2, shl = 16 * (tl & 3);
                    tmask = (unsigned)((s_inf[soff + wl] >> shl) & 0xFFFFull) | ((unsigned)((s_bas[par * 8 + wl] >> shl) & 0xFFFFull) << 16);
                }

                while (tiles) {
                    const int kappa = __builtin_ctz(tiles);
                    unsigned pmall, basm;
                    if constexpr (LANE_MASKS) {
                        const unsigned tm = (unsigned)__builtin_amdgcn_readlane((int)tmask, kappa);
                        pmall = tm & 0xFFFFu;
                        if (!all) pmall = 1u << (single_k & 15);
                        basm = tm >> 16;
                    } else {
                        const int wsel = kappa >> 2, sh = 16 * (kappa & 3);
                        pmall = (unsigned)((s_inf[soff + wsel] >> sh) & 0xFFFFull);
                        if (!all) pmall = 1u << (single_k & 15);
                        basm = (unsigned)__builtin_amdgcn_readfirstlane((int)((s_bas[par * 8 + wsel] >> sh) & 0xFFFFull));
                        pmall = (unsigned)__builtin_amdgcn_readfirstlane((int)pmall);
                    }
                    while (pmall) {
                        // ---- block: the lowest <= MB violators of tile column kappa -------------------------------------
                        unsigned rest = 0;
                        if (__builtin_expect(__builtin_popcount(pmall) > MB, 0)) {
                            rest = pmall;
#pragma unroll
                            for (int i = 0; i < MB; ++i) rest &= rest - 1;
                        }
                        const unsigned pm = pmall & ~rest;
                        pmall = rest;
                        const int m = __builtin_popcount(pm);
                        const int bpar = bc & 1;
                        double *P = Pbase + bpar * MB * CW;
                        ++bc;
                        // the tile index is invariant in this loop: left alone, the compiler hoists all 17 `kappa == i` tests out of it
                        // as 64-bit lane masks (34 SGPRs, spilled to VGPR lanes and reloaded per block); the opaque copy keeps each
                        // test a plain s_cmp at its use (C3 sweep 93.0 -> 85.3 ms)
                        int kap = kappa;
                        asm volatile("" : "+s"(kap));
                        STAMP(12);
                        // ---- 1. gather the pivot columns (compacted) into the LDS panel ------------------------------------
#define PARTLS_G(i) if constexpr (i < T) { if (__builtin_expect(kap == i, 0)) gather_tile<T, H, W, i>(S, P, a, b, pm); }
                        PARTLS_CASES(PARTLS_G)                 // flat chain of independent ifs: the only form the register allocator keeps spill-free
#undef PARTLS_G
                        STAMP(13);
                        if (tid < 16 * T && (tid >> 4) == kappa && ((pm >> (tid & 15)) & 1u))
                            P[__builtin_popcount(pm & ((1u << (tid & 15)) - 1u)) * CW + RHSPOS] = q;
                        // is this thread's panel row a pivot row?  row position t <-> variable 16*rowrho + rowc
                        int myj = -1;
                        bool my_basic = false;
                        if (rowrho == kappa && rowc < 16 && ((pm >> rowc) & 1u)) {
                            myj = __builtin_popcount(pm & ((1u << rowc) - 1u));
                            my_basic = (basm >> rowc) & 1u;
                        }
                        STAMP(8);
                        __syncthreads();
                        STAMP(1);
                        if (tid == 0) s_veto[bpar ^ 1] = NO_VETO;              // the other slot: last read before this barrier
                        // ---- 2. panel elimination -----------------------------------------------------------------------
                        {
                            int veto;
                            switch (m) {
#define PARTLS_PB(i) case i: if constexpr (i <= MB) veto = panel_block<(i <= MB ? i : 1), CW, MB>(P, Z, U, Dinv, myj, my_basic, p.piv_eps, tid, tid, idle_wave); else veto = 0; break;
                                PARTLS_PB(1) PARTLS_PB(2) PARTLS_PB(3) PARTLS_PB(4) PARTLS_PB(5) PARTLS_PB(6) PARTLS_PB(7) PARTLS_PB(8)
                                PARTLS_PB(9) PARTLS_PB(10) PARTLS_PB(11) PARTLS_PB(12) PARTLS_PB(13) PARTLS_PB(14) PARTLS_PB(15)
#undef PARTLS_PB
                                default: veto = panel_block<MB, CW, MB>(P, Z, U, Dinv, myj, my_basic, p.piv_eps, tid, tid, idle_wave); break;
                            }
                            if (veto < m && tid != RHSPOS) atomicMin(&s_veto[bpar], veto);     // the rhs row is no variable
                        }
                        STAMP(11);
                        __syncthreads();
                        STAMP(2);
                        // leave-one-out veto at step vs: nothing of this block has touched the register tableau yet.  The offender
                        // is rejected for the current basis and the other pivots of the block are redone; the rest of the block body
                        // runs with ZERO pivots (no extra control-flow edge in the block loop: the allocator keeps the tableau put)
                        const int vs = __builtin_amdgcn_readfirstlane(s_veto[bpar]);
                        unsigned pmx = pm;
                        int mx = m;
                        if (__builtin_expect(vs < m, 0)) {
                            unsigned r = pm;
                            for (int i = 0; i < vs; ++i) r &= r - 1;
                            const unsigned vbit = r & (0u - r);
                            blocked = blocked || (tid == 16 * kappa + __builtin_ctz(vbit));
                            pmall |= pm & ~vbit;
                            pmx = 0;
                            mx = 0;
                            ++nveto;
                        }
                        // ---- 3. fused rank-m update of the register tableau ------------------------------------------------
                        bool blk_ok = false;
#pragma unroll PARTLS_UPD_UNROLL
                        for (int s = 0; s < mx; ++s) {
                            const double inv = Dinv[s];
                            blk_ok = blk_ok || (inv != 0.0);
                            const double *Zs = Z + s * CW;
                            double x[L::XN];
#pragma unroll
                            for (int rho = 0; rho < L::XN; ++rho) x[rho] = Zs[a * RS + rho];
#pragma unroll
                            for (int gam = L::GLO; gam < L::GHI; ++gam) {
                                const double yg = -Zs[b * RS + gam] * inv;
#pragma unroll
                                for (int rho = 0; rho <= gam; ++rho)
                                    S[L::idx(rho, gam)] = fma(x[rho], yg, S[L::idx(rho, gam)]);
                            }
                            const double zr = Zs[RHSPOS], zri = zr * inv;
                            if (tid < 16 * T) q = fma(-Zs[mypos], zri, q);
                            corner = fma(-zr, zri, corner);
                        }
                        STAMP(3);
                        // ---- 4. rows / columns of the pivoted variables come from the final panel ----------------------------
#define PARTLS_F(i) if constexpr (i < T) { if (__builtin_expect(kap == i, 0)) scatter_tile<T, H, W, i>(S, P, a, b, pmx); }
                        PARTLS_CASES(PARTLS_F)
#undef PARTLS_F
                        if (tid < 16 * T && (tid >> 4) == kappa && ((pmx >> (tid & 15)) & 1u)) {
                            const int j = __builtin_popcount(pmx & ((1u << (tid & 15)) - 1u));
                            q = P[j * CW + RHSPOS];
                            if (Dinv[j] != 0.0) basic = !basic;
                            else blocked = true;
                        }
                        progress = progress || blk_ok;
                        npiv += (unsigned)mx;
                        STAMP(4);
                    }
                    tiles &= tiles - 1;
                }
            }
            if constexpr (!MERGED) {
                finish_pattern(gi, nunconv != nunconv0);
                if (++gi >= glen) break;
            } else break;
        }
        if constexpr (NODE) {
            if (has_var) p.node_sol[(size_t)chain * p.node_ld + tid] = basic ? q : 0.0;
            if (tid == 0) p.node_obj2[chain] = corner;
            if (p.node_dst) {                                     // snapshot of the final state: what a child node starts from
                double *snap = p.node_dst[chain];
                if (snap && (H == 0 || T > 1)) {
                    tiles_store<L>(snap, S, t8);
                    if (tid < 16 * T) {
                        snap[(size_t)nslots(T) * 256 + tid] = q;
                        reinterpret_cast<int8_t *>(snap + (nslots(T) * 256 + 16 * T + 8))[tid] = basic ? 1 : 0;
                    }
                    if (tid == 0) snap[(size_t)nslots(T) * 256 + 16 * T] = corner;
                }
            }
            if (p.node_tab && (H == 0 || T > 1)) {                // final tableau + basis, same layout as T0 (half 1 of T = 1 owns nothing)
                double *tab = p.node_tab + (size_t)chain * (nslots(T) * 256 + 16 * T + 8);
                tiles_store<L>(tab, S, t8);
                if (tid < 16 * T) p.node_basic[(size_t)chain * 16 * T + tid] = basic ? 1 : 0;
            }
        }
    }
    STAMP_FLUSH;
    __syncthreads();                                      // s_best was last written by thread THREADS - 1
    if (tid == 0) {
        p.best_obj[blockIdx.x] = sqrt(s_best[0]);
        p.best_pat[blockIdx.x] = reinterpret_cast<long long *>(s_best)[1];
        if (p.second_obj) { p.second_obj[blockIdx.x] = sqrt(s_best[2]); p.second_pat[blockIdx.x] = reinterpret_cast<long long *>(s_best)[3]; }
        if (p.n_pivots && npiv) atomicAdd(p.n_pivots, (unsigned long long)npiv);
        if (p.n_unconverged && nunconv) atomicAdd(p.n_unconverged, (unsigned long long)nunconv);
        if (p.n_vetoes && nveto) atomicAdd(p.n_vetoes, (unsigned long long)nveto);
    }
}

// Barrier invariant.  The two halves of the workgroup run DIFFERENT instantiations (sweep_body<T,0> / <T,1>) and meet at
// workgroup barriers issued from different program counters.  That is only sound because every barrier of the body is reached
// under wave-uniform control flow whose conditions (count, tiles, pmall, m, vs, rounds, patience, chain and pattern counters)
// are computed from LDS words or kernel arguments that are identical for all 512 threads — never from a half's own registers —
// so both instantiations execute the same barrier sequence: per scan 1, per block 2 + m (the m panel steps; idle waves only
// count them).  Any edit that makes a barrier conditional on per-half or per-wave data deadlocks the CU.
// BATCH (chain mode only, partls_cv_opt): blockIdx.y selects one problem of a stacked batch; its tableau, tolerance and result slots
// replace the launch's before the body runs (SweepParams::batch_t0).  A separate instantiation: the default ones keep their code.
__device__ __forceinline__ void batch_select(SweepParams &p)
{
    const int64_t q = blockIdx.y;
    p.T0 += q * p.batch_t0;
    p.tol = p.batch_tol[q];
    const int64_t o = q * p.batch_out;
    p.best_obj += o;
    p.best_pat += o;
    if (p.second_obj) { p.second_obj += o; p.second_pat += o; }
    if (p.n_unconverged) p.n_unconverged += o;
    if (p.n_pivots) p.n_pivots += o;
    if (p.n_vetoes) p.n_vetoes += o;
    if (p.best_sol) p.best_sol += q * (int64_t)gridDim.x * p.node_ld;
}

template <int T, bool NODE, bool MODELS = false, bool BATCH = false, bool PAIRK = false>
__global__ __launch_bounds__(THREADS, 2) void sweep_blk_kernel(SweepParams p)
{
    if constexpr (BATCH) batch_select(p);
    const int half = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    if (half == 0) sweep_body<T, 0, NODE, 2, MODELS, BATCH, PAIRK>(p);
    else sweep_body<T, 1, NODE, 2, MODELS, BATCH, PAIRK>(p);
}
constexpr bool pair_compiled(int T) { return PARTLS_PAIR && PARTLS_MERGED_SCAN && PARTLS_LANE_MASKS && T > MAXT_S && T <= 16; }

#ifndef PARTLS_SMALL_OCC
#define PARTLS_SMALL_OCC(T) ((T) <= 8 ? 3 : 2)          // waves per SIMD = workgroups per CU the allocator is asked to leave room for
#endif
template <int T, bool NODE, bool MODELS = false, bool BATCH = false>
__global__ __launch_bounds__(256, PARTLS_SMALL_OCC(T)) void sweep_small_kernel(SweepParams p)
{
    if constexpr (BATCH) batch_select(p);
    sweep_body<T, 0, NODE, 1, MODELS, BATCH>(p);
}

// Tfull ((n+1)^2) -> tile-cyclic initial state: [slot = tri(gamma) + rho][256 = a + 16 b], then q0[16 T], then the corner.
// blockIdx.y selects one problem of a stacked batch; in_stride / out_stride: doubles from one problem to the next
__global__ void layout_reg_kernel(const double *__restrict__ Tfull, int n, int T, double *__restrict__ out, int64_t in_stride, int64_t out_stride)
{
    const int64_t q = blockIdx.y;
    const int ld = n + 1;
    const int ns = T * (T + 1) / 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int tot = ns * 256 + 16 * T + 1;
    if (idx >= tot) return;
    const double *Tq = Tfull + q * in_stride;
    double *oq = out + q * out_stride;
    if (idx < ns * 256) {
        const int s = idx >> 8, t8 = idx & 255, a = t8 & 15, b = t8 >> 4;
        int gam = 0;
        while ((gam + 1) * (gam + 2) / 2 <= s) ++gam;
        const int rho = s - gam * (gam + 1) / 2;
        const int i = 16 * rho + a, j = 16 * gam + b;
        oq[idx] = (i < n && j < n) ? Tq[(size_t)i * ld + j] : ((i == j) ? 1.0 : 0.0);
    } else if (idx < ns * 256 + 16 * T) {
        const int v = idx - ns * 256;
        oq[idx] = (v < n) ? Tq[(size_t)v * ld + n] : 0.0;
    } else {
        oq[idx] = Tq[(size_t)n * ld + n];
    }
}

}  // namespace blk

bool sweep_reg_supported(int n) { return n >= 1 && n <= 16 * blk::MAXT; }
int sweep_reg_tiles(int n) { return (n + 15) / 16; }
bool sweep_reg_exports(int T) { return PARTLS_EXPORT_BIG != 0 && T <= blk::EXPORT_MAXT; }
bool sweep_reg_small(int T) { return T <= blk::MAXT_S; }   // the 256-thread kernel (several chains per CU) runs this tile count
size_t sweep_reg_t0_doubles(int T) { return (size_t)T * (T + 1) / 2 * 256 + 16 * (size_t)T + 8; }

// every problem of the batch writes tot = ns * 256 + 16 T + 1 doubles; the batch strides by sweep_reg_t0_doubles(T)
hipError_t launch_layout_reg_batch(const double *Tfull, int n, int T, int batch, double *T0reg, hipStream_t s)
{
    const int tot = T * (T + 1) / 2 * 256 + 16 * T + 1;
    hipLaunchKernelGGL(blk::layout_reg_kernel, dim3((tot + 255) / 256, batch), dim3(256), 0, s, Tfull, n, T, T0reg,
                       (int64_t)(n + 1) * (n + 1), (int64_t)sweep_reg_t0_doubles(T));
    return hipGetLastError();
}

hipError_t launch_layout_reg(const double *Tfull, int n, int T, double *T0reg, hipStream_t s)
{
    return launch_layout_reg_batch(Tfull, n, T, 1, T0reg, s);
}

// f(std::integral_constant<int, T>{}) for a compiled tile count T (PARTLS_ONLY_T: that one only), `none` for any other
template <class R, class F>
static R dispatch_T(int T, R none, F f)
{
    switch (T) {
#ifdef PARTLS_ONLY_T
        case PARTLS_ONLY_T: return f(std::integral_constant<int, PARTLS_ONLY_T>{});
#else
#define PARTLS_L(i) case i + 1: return f(std::integral_constant<int, i + 1>{});
        PARTLS_CASES(PARTLS_L)
#undef PARTLS_L
#endif
        default: return none;
    }
}

template <int T>
static hipError_t launch_blk_batch_T(const SweepParams &p, int grid, int batch, hipStream_t s)
{
    if constexpr (T <= blk::MAXT_S) hipLaunchKernelGGL((blk::sweep_small_kernel<T, false, false, true>), dim3(grid, batch), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((blk::sweep_blk_kernel<T, false, false, true>), dim3(grid, batch), dim3(blk::THREADS), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_sweep_blk_batch(const SweepParams &p, int T, int grid, int batch, hipStream_t s)
{
    if (p.node_code || batch < 1 || batch > 65535) return hipErrorInvalidValue;
    return dispatch_T(T, hipErrorInvalidValue, [&](auto t) { return launch_blk_batch_T<decltype(t)::value>(p, grid, batch, s); });
}

template <int T>
static hipError_t launch_blk_T(const SweepParams &p, int grid, hipStream_t s, bool models)
{
    if constexpr (T <= blk::MAXT_S) {                        // small tableau: 256-thread workgroups, several per CU
        if (p.node_code) hipLaunchKernelGGL((blk::sweep_small_kernel<T, true>), dim3(grid), dim3(256), 0, s, p);
        else if (models) hipLaunchKernelGGL((blk::sweep_small_kernel<T, false, true>), dim3(grid), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((blk::sweep_small_kernel<T, false>), dim3(grid), dim3(256), 0, s, p);
    } else {
        if (p.node_code) hipLaunchKernelGGL((blk::sweep_blk_kernel<T, true>), dim3(grid), dim3(blk::THREADS), 0, s, p);     // ~100 KB of static LDS
        else if (models) hipLaunchKernelGGL((blk::sweep_blk_kernel<T, false, true>), dim3(grid), dim3(blk::THREADS), 0, s, p);
        else if (blk::pair_compiled(T) && p.pair) hipLaunchKernelGGL((blk::sweep_blk_kernel<T, false, false, false, blk::pair_compiled(T)>), dim3(grid), dim3(blk::THREADS), 0, s, p);
        else hipLaunchKernelGGL((blk::sweep_blk_kernel<T, false>), dim3(grid), dim3(blk::THREADS), 0, s, p);
    }
    return hipGetLastError();
}

// chains (workgroups) of the chain-mode sweep a CU runs at the same time: 1 for the 512-thread kernel, the occupancy of the 256-thread one
template <int T>
static int concurrency_T()
{
    if constexpr (T <= blk::MAXT_S) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void *>(&blk::sweep_small_kernel<T, false>), 256, 0) != hipSuccess || n < 1) n = 1;
        return n;
    }
    return 1;
}
int sweep_reg_concurrency_query(int T);
int sweep_reg_concurrency(int T)
{
    // the occupancy query costs tens of microseconds — as much as a tenth of a whole C2-sized fit: asked once per tile count
    // (atomic: the rank threads of partls_fit_opt_multi call this concurrently; every thread would store the same value)
    static std::atomic<int> cached[blk::MAXT + 2];
    if (T >= 0 && T <= blk::MAXT) { const int v = cached[T].load(std::memory_order_relaxed); if (v > 0) return v; }
    const int v = sweep_reg_concurrency_query(T);
    if (T >= 0 && T <= blk::MAXT) cached[T].store(v, std::memory_order_relaxed);
    return v;
}
int sweep_reg_concurrency_query(int T)
{
    return dispatch_T(T, 1, [](auto t) { return concurrency_T<decltype(t)::value>(); });
}

hipError_t launch_sweep_blk(const SweepParams &p, int T, int grid, hipStream_t s, bool models)
{
    return dispatch_T(T, hipErrorInvalidValue, [&](auto t) { return launch_blk_T<decltype(t)::value>(p, grid, s, models); });
}

}  // namespace partls
