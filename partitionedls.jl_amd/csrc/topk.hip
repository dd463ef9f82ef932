// topk.hip — the k best patterns of a piece of an export sweep, selected on the device (partls_opt_top, partls_opt_top_select;
// DESIGN.md §4.13).
//
// The export instantiation of the sweep kernels leaves obj[i], the objective of Gray index g0 + i, for the cnt patterns of a piece.  The
// order is total: a before b iff obj_a < obj_b, or obj_a == obj_b as doubles (-0 = +0) and reference index a < reference index b; a NaN
// objective (pivot cap) is never selected.  Every pattern gets the 128-bit composite key
//     hi = order-preserving image of the double (-0 folded to +0: sign bit set for x >= 0, all bits flipped for x < 0)
//     lo = reference index b = g ^ (g >> 1) through the visiting order (as models_cleanup_kernel computes it)
// which is unique, so "the k smallest" is a set.  All of it runs on one stream without a host round trip:
//   1. radix select, 8 bits a pass, most significant digit first: 8 passes over hi, then ceil(kbits / 8) over lo among the entries whose
//      hi equals the threshold's.  A pass is a histogram kernel (integer atomics only; its pieces are radix_select.h's, shared with
//      robust.hip) and a one-workgroup scan that fixes the next digit of the threshold key, the k still to find below it, and `done` as
//      soon as the threshold's bucket is taken whole — the remaining passes then return at once.  Counts do not depend on arrival order.
//   2. compaction: every non-NaN entry with key <= threshold claims a slot by an integer atomic (any order: the next step sorts);
//   3. a bitonic sort of the at most k survivors by the composite key in the LDS of one workgroup (4096 x 24 B = 96 KiB);
//   4. gather: the survivors' scaled rows, objectives and Gray indices into a compact buffer in sorted order, one wave per row, 16-byte
//      loads along the row when the rows are 16-byte aligned (n even).  Rows at and beyond the count get a NaN objective, which
//      models_cleanup_kernel (run on the compact buffer with the Gray-index list) answers with NaN outputs that the host never reads.
#include "sweep_rules.h"
#include "radix_select.h"

namespace partls {

static constexpr int TK_THREADS = 256, TK_BINS = 257 /* 256 digits + NaN (first pass) */, TK_SORT_THREADS = 1024;

struct TopState {
    uint64_t thr_hi, thr_lo;     // threshold key: the digits fixed so far, all ones below them
    uint64_t k_rem;              // entries still to take among those that match the fixed digits
    uint64_t count;              // min(k, non-NaN entries): fixed by the first scan
    unsigned done, nsel;         // the threshold's bucket is taken whole; slots claimed by the compaction
    unsigned hist[TK_BINS + 1];
};
static_assert(sizeof(TopState) <= TOPK_STATE_BYTES, "TopState outgrew its slot in the work buffer");

__device__ __forceinline__ uint64_t tk_value_key(double o)
{
    uint64_t u = (o == 0.0) ? 0ULL : (uint64_t)__double_as_longlong(o);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ uint64_t tk_ref_pattern(uint64_t g, int kbits, const BitOrder &order, int order_identity)
{
    const uint64_t q = g ^ (g >> 1);
    if (order_identity) return q;
    uint64_t b = 0;
    for (int k = 0; k < kbits; ++k) b |= ((q >> order.gbit[k]) & 1ULL) << k;
    return b;
}
__device__ __forceinline__ uint64_t tk_above(uint64_t x, int s) { return s >= 64 ? 0ULL : x >> s; }

__global__ void topk_init_kernel(TopState *st, int64_t k, int nlo)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < TK_BINS + 1; i += blockDim.x) st->hist[i] = 0;
    // the threshold starts at the largest key: all ones in hi and in the 8 nlo bits of lo that the passes walk (lo < 2^kbits <= 2^(8 nlo))
    if (tid == 0) { st->thr_hi = ~0ULL; st->thr_lo = nlo >= 8 ? ~0ULL : (1ULL << (8 * nlo)) - 1; st->k_rem = (uint64_t)k; st->count = 0; st->done = 0; st->nsel = 0; }
}

// pass p < 8: digit 7 - p of hi; pass 8 + j: digit nlo - 1 - j of lo
__global__ __launch_bounds__(TK_THREADS) void topk_hist_kernel(const double *__restrict__ obj, int64_t cnt, int64_t g0, int kbits,
                                                               BitOrder order, int order_identity, TopState *st, int pass, int nlo)
{
    __shared__ unsigned h[TK_BINS];
    if (st->done) return;                                         // grid-uniform: written by the previous kernel of the stream
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < TK_BINS; i += TK_THREADS) h[i] = 0;
    __syncthreads();
    const uint64_t thi = st->thr_hi, tlo = st->thr_lo;
    const bool on_hi = pass < 8;
    const int shift = on_hi ? 56 - 8 * pass : 8 * (nlo - 1 - (pass - 8));
    for (int64_t base = (int64_t)blockIdx.x * TK_THREADS; base < cnt; base += (int64_t)gridDim.x * TK_THREADS) {   // block-uniform trip count
        const int64_t i = base + tid;
        bool part = false;
        int d = 0;
        if (i < cnt) {
            const double o = obj[i];
            if (o != o) {
                if (pass == 0) { part = true; d = 256; }
            } else {
                const uint64_t hi = tk_value_key(o);
                if (on_hi) {
                    part = tk_above(hi, shift + 8) == tk_above(thi, shift + 8);
                    d = (int)((hi >> shift) & 255ULL);
                } else if (hi == thi) {
                    const uint64_t lo = tk_ref_pattern((uint64_t)(g0 + i), kbits, order, order_identity);
                    part = tk_above(lo, shift + 8) == tk_above(tlo, shift + 8);
                    d = (int)((lo >> shift) & 255ULL);
                }
            }
        }
        radix_wave_add(h, part, d, lane);
    }
    __syncthreads();
    radix_flush(h, st->hist, TK_BINS, tid, TK_THREADS);
}

__global__ __launch_bounds__(TK_THREADS) void topk_scan_kernel(TopState *st, int pass, int nlo)
{
    __shared__ unsigned h[TK_BINS];
    if (st->done) return;
    const int tid = threadIdx.x;
    radix_take(h, st->hist, TK_BINS, tid, TK_THREADS);
    __syncthreads();
    if (tid != 0) return;
    uint64_t krem = st->k_rem;
    if (pass == 0) {
        uint64_t valid = 0;
        for (int d = 0; d < 256; ++d) valid += h[d];
        if (krem > valid) krem = valid;
        st->count = krem;
        if (krem == 0) { st->k_rem = 0; st->done = 1; return; }
    }
    uint64_t cum = 0;
    const int d = radix_digit(h, krem, &cum);
    krem -= cum;
    const bool on_hi = pass < 8;
    const int shift = on_hi ? 56 - 8 * pass : 8 * (nlo - 1 - (pass - 8));
    const uint64_t clr = ~(255ULL << shift), dig = (uint64_t)d << shift;
    if (on_hi) st->thr_hi = (st->thr_hi & clr) | dig;
    else st->thr_lo = (st->thr_lo & clr) | dig;
    st->k_rem = krem;
    if ((uint64_t)h[d] == krem) st->done = 1;                     // the whole bucket is taken: key <= threshold (ones below) selects it
}

__global__ __launch_bounds__(TK_THREADS) void topk_compact_kernel(const double *__restrict__ obj, int64_t cnt, int64_t g0, int kbits,
                                                                  BitOrder order, int order_identity, TopState *st, int64_t cap,
                                                                  uint64_t *__restrict__ sel_hi, uint64_t *__restrict__ sel_lo,
                                                                  int64_t *__restrict__ sel_idx)
{
    if (st->count == 0) return;
    const uint64_t thi = st->thr_hi, tlo = st->thr_lo;
    for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * TK_THREADS) {
        const double o = obj[i];
        if (o != o) continue;
        const uint64_t hi = tk_value_key(o);
        if (hi > thi) continue;
        const uint64_t lo = tk_ref_pattern((uint64_t)(g0 + i), kbits, order, order_identity);
        if (hi == thi && lo > tlo) continue;
        const unsigned slot = atomicAdd(&st->nsel, 1u);
        if ((int64_t)slot < cap) { sel_hi[slot] = hi; sel_lo[slot] = lo; sel_idx[slot] = i; }
    }
}

// one workgroup: bitonic sort of the survivors (padded to p2, a power of two, with keys of all ones) -> out_idx, out_pat [count]
__global__ __launch_bounds__(TK_SORT_THREADS) void topk_sort_kernel(TopState *st, const uint64_t *__restrict__ sel_hi,
                                                                    const uint64_t *__restrict__ sel_lo, const int64_t *__restrict__ sel_idx,
                                                                    int p2, int64_t *__restrict__ out_idx, int64_t *__restrict__ out_pat)
{
    extern __shared__ __align__(16) unsigned char tk_smem[];
    uint64_t *khi = reinterpret_cast<uint64_t *>(tk_smem), *klo = khi + p2;
    int64_t *kix = reinterpret_cast<int64_t *>(klo + p2);
    const int tid = threadIdx.x;
    int count = (int)st->count;
    if (count > p2) count = p2;
    if ((unsigned)count > st->nsel) count = (int)st->nsel;        // (never: exactly `count` entries lie at or below the threshold)
    __syncthreads();
    if (tid == 0) st->count = (uint64_t)count;
    for (int i = tid; i < p2; i += TK_SORT_THREADS) {
        const bool in = i < count;
        khi[i] = in ? sel_hi[i] : ~0ULL;
        klo[i] = in ? sel_lo[i] : ~0ULL;
        kix[i] = in ? sel_idx[i] : -1;
    }
    __syncthreads();
    for (int size = 2; size <= p2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (p2 >> 1); t += TK_SORT_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const uint64_t ah = khi[i], al = klo[i], bh = khi[j], bl = klo[j];
                const bool a_gt_b = ah > bh || (ah == bh && al > bl);
                if (a_gt_b == up) {
                    khi[i] = bh; klo[i] = bl; khi[j] = ah; klo[j] = al;
                    const int64_t x = kix[i]; kix[i] = kix[j]; kix[j] = x;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < count; i += TK_SORT_THREADS) { out_idx[i] = kix[i]; out_pat[i] = (int64_t)klo[i]; }
}

// one wave per output row i < kk: row out_idx[i] of the piece -> row i of the compact buffer, with its objective and Gray index
__global__ __launch_bounds__(64) void topk_gather_kernel(const double *__restrict__ rows, const double *__restrict__ obj, int n, int64_t g0,
                                                         int64_t cnt, const TopState *st, const int64_t *__restrict__ out_idx, double *__restrict__ crow,
                                                         double *__restrict__ cobj, int64_t *__restrict__ glist)
{
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t src = i < (int64_t)st->count ? out_idx[i] : -1;
    if (src < 0 || src >= cnt) {                                  // no such row: the cleanup writes NaN there, nobody reads it
        if (lane == 0) { cobj[i] = __builtin_nan(""); glist[i] = g0; }
        return;
    }
    const double *s = rows + (size_t)src * n;
    double *d = crow + (size_t)i * n;
    if ((n & 1) == 0) {                                           // both rows start on 16 bytes
        const double2 *s2 = reinterpret_cast<const double2 *>(s);
        double2 *d2 = reinterpret_cast<double2 *>(d);
        for (int v = lane; v < (n >> 1); v += 64) d2[v] = s2[v];
    } else {
        for (int v = lane; v < n; v += 64) d[v] = s[v];
    }
    if (lane == 0) { cobj[i] = obj[src]; glist[i] = g0 + src; }
}

static int tk_pow2(int64_t x)
{
    int p = 2;
    while (p < x) p <<= 1;
    return p;
}

size_t topk_work_bytes(int64_t kk) { return TOPK_STATE_BYTES + (size_t)5 * (size_t)kk * 8; }

hipError_t launch_topk_select(const double *obj, int64_t cnt, int64_t g0, int64_t k, int kbits, const BitOrder &order, bool order_identity,
                              void *work, hipStream_t s)
{
    const int64_t kk = k < cnt ? k : cnt;
    TopState *st = static_cast<TopState *>(work);
    const TopkWork w = topk_work(work, kk);
    const int ident = order_identity ? 1 : 0, nlo = (kbits + 7) / 8;
    const int64_t blocks = (cnt + TK_THREADS - 1) / TK_THREADS;
    const int grid = (int)(blocks < 1024 ? blocks : 1024);
    hipLaunchKernelGGL(topk_init_kernel, dim3(1), dim3(TK_THREADS), 0, s, st, kk, nlo);
    for (int pass = 0; pass < 8 + nlo; ++pass) {
        hipLaunchKernelGGL(topk_hist_kernel, dim3(grid), dim3(TK_THREADS), 0, s, obj, cnt, g0, kbits, order, ident, st, pass, nlo);
        hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(TK_THREADS), 0, s, st, pass, nlo);
    }
    hipLaunchKernelGGL(topk_compact_kernel, dim3(grid), dim3(TK_THREADS), 0, s, obj, cnt, g0, kbits, order, ident, st, kk, w.sel_hi, w.sel_lo,
                       w.sel_idx);
    const int p2 = tk_pow2(kk);
    const size_t shmem = (size_t)p2 * 24;
    if (shmem > ((size_t)48 << 10)) {                             // k > 2048 (the attribute is per device: set whenever it is needed)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&topk_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)shmem);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(topk_sort_kernel, dim3(1), dim3(TK_SORT_THREADS), shmem, s, st, w.sel_hi, w.sel_lo, w.sel_idx, p2, w.out_idx, w.out_pat);
    return hipGetLastError();
}

hipError_t launch_topk_gather(const double *rows, const double *obj, int n, int64_t g0, int64_t cnt, int64_t kk, const void *work, double *crow,
                              double *cobj, int64_t *glist, hipStream_t s)
{
    const TopkWork w = topk_work(const_cast<void *>(work), kk);
    hipLaunchKernelGGL(topk_gather_kernel, dim3((unsigned)kk), dim3(64), 0, s, rows, obj, n, g0, cnt, static_cast<const TopState *>(work), w.out_idx,
                       crow, cobj, glist);
    return hipGetLastError();
}

}  // namespace partls
