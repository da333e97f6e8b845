// search.h -- the two searches over ascending u64 arrays (read offsets, scans, position lists) that more than one kernel file uses.
#pragma once
#include "device_common.h"

namespace drprg {
namespace dev {

// smallest i in [0, n) with a[i] >= target, n if there is none; a is ascending.  Wave-uniform result; every lane of the wave calls it.
// A 64-way search: every round the 64 lanes probe evenly spaced entries of what is left of the range and a ballot keeps the one gap the
// answer lies in, so the range shrinks 64-fold per round (five rounds for 2^28 entries; a binary search by one lane would be 28 dependent loads).
__device__ inline uint64_t first_at_least(const uint64_t* __restrict__ a, uint64_t n, uint64_t target, int lane)
{
    uint64_t lo = 0, hi = n; // the answer is in [lo, hi]; a[hi] >= target or hi == n
    while (lo < hi) {
        const uint64_t step = (hi - lo + 63) >> 6; // >= 1: the probes lo + step * lane cover [lo, hi)
        const uint64_t p = lo + step * (uint64_t)lane;
        const bool ge = p < hi && a[p] >= target; // (p < hi <= n: inside the array)
        const uint64_t m = __ballot(ge);
        if (!m) { // every probe is below the target, the last one at >= hi - step: what is left lies behind it
            const uint64_t last = lo + step * (uint64_t)((hi - lo - 1) / step);
            lo = last + 1;
            continue;
        }
        const int f = __ffsll((long long)m) - 1;
        hi = lo + step * (uint64_t)f;                 // a[hi] >= target
        if (f) lo = lo + step * (uint64_t)(f - 1) + 1; // a[probe f - 1] < target
    }
    return lo;
}

// (host code as well, so that a CPU build can walk a kernel's index arithmetic under a sanitizer)
// the largest r in [lo, hi] with offsets[r] <= p (offsets[lo] <= p): the read that holds base p when p < offsets[hi + 1]
DRPRG_HD inline uint64_t read_holding(const uint64_t* __restrict__ offsets, uint64_t lo, uint64_t hi, uint64_t p)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

} // namespace dev
} // namespace drprg
