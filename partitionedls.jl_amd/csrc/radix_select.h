// radix_select.h — what the two radix selects (topk.hip, robust.hip) share of a pass, 8 bits at a time over an `unsigned` histogram:
// device only, integer only (a count does not depend on the order of arrival).  The keys, thresholds and states stay with each file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace partls {

// A wave's entries of a step into the workgroup's LDS histogram h (every lane calls it; `part`: this lane has an entry, of digit d).
// A wave whose participants all share a digit, the usual case in the leading digits, adds its count once.
__device__ __forceinline__ void radix_wave_add(unsigned *h, bool part, int d, int lane)
{
    const unsigned long long mask = __ballot(part);              // 64 lanes
    if (!mask) return;
    const int first = __ffsll((long long)mask) - 1;
    const int d0 = __shfl(d, first);
    const unsigned long long same = __ballot(part && d == d0);
    if (same == mask) {
        if (lane == first) atomicAdd(&h[d0], (unsigned)__popcll(mask));
    } else if (part) atomicAdd(&h[d], 1u);
}

// the workgroup's histogram h[0 .. bins) into the global one g: one integer add per non-empty bin
__device__ __forceinline__ void radix_flush(const unsigned *h, unsigned *g, int bins, int tid, int threads)
{
    for (int i = tid; i < bins; i += threads)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

// the scan's side: g[0 .. bins) into LDS, and zeroed for the next pass (the caller's barrier follows)
__device__ __forceinline__ void radix_take(unsigned *h, unsigned *g, int bins, int tid, int threads)
{
    for (int i = tid; i < bins; i += threads) { h[i] = g[i]; g[i] = 0; }
}

// the first digit d < 255 whose cumulative count reaches k (255 when none does); *below = the count of the digits under it
__device__ __forceinline__ int radix_digit(const unsigned *h, uint64_t k, uint64_t *below)
{
    uint64_t cum = 0;
    int d = 0;
    for (; d < 255; ++d) {
        if (cum + h[d] >= k) break;
        cum += h[d];
    }
    *below = cum;
    return d;
}

}  // namespace partls
