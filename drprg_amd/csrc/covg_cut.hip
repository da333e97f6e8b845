// covg_cut.hip -- where a device batch crosses the depth cap (drprg_hip_set_max_covg; DESIGN.md section 4 "depth cap").
//
// A device batch's read offsets exist only in HBM.  The host knows the batch's n_bases, so it knows WHETHER the batch reaches the cap
// without asking the device; only the one batch that does is looked at here: the smallest i with offsets[i] >= target, and -- for a
// packed batch -- how many of its listed non-ACGT positions lie below offsets[i].  One wave, a 64-way search: every round the 64 lanes
// probe evenly spaced entries of what is left of the range and a ballot keeps the one gap the answer lies in, so the range shrinks
// 64-fold per round (five rounds for 2^28 reads; a binary search by one lane would be 28 dependent loads).  Latency-bound: <= 5 + 5
// rounds of one 8-byte load per lane, no LDS, nothing to tune.  Launched at most once per context between resets.
#include "device_common.h"

namespace drprg {
namespace dev {

// smallest i in [0, n) with a[i] >= target, n if there is none; a is ascending.  Wave-uniform result; every lane of the wave calls it.
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

// out[0] = i, out[1] = offsets[i], out[2] = positions of npos below offsets[i]  (out: page-locked host memory, written by lane 0 with
// ordinary vector stores).  No entry reaches the target (the caller's n_bases was not offsets[n_reads]): i = n_reads.
__global__ __launch_bounds__(64) void covg_cut_kernel(const uint64_t* __restrict__ offsets, uint64_t n_reads, uint64_t target,
    const uint64_t* __restrict__ npos, uint64_t n_npos, unsigned long long* __restrict__ out)
{
    const int lane = (int)threadIdx.x;
    uint64_t i = first_at_least(offsets + 1, n_reads, target, lane) + 1;
    if (i > n_reads) i = n_reads;
    const uint64_t cut = offsets[i];
    const uint64_t below = n_npos ? first_at_least(npos, n_npos, cut, lane) : 0;
    if (lane == 0) {
        out[0] = i;
        out[1] = cut;
        out[2] = below;
    }
}

hipError_t launch_covg_cut(const uint64_t* offsets, uint64_t n_reads, uint64_t target, const uint64_t* npos, uint64_t n_npos, unsigned long long* out,
    hipStream_t stream)
{
    hipLaunchKernelGGL(covg_cut_kernel, dim3(1), dim3(64), 0, stream, offsets, n_reads, target, npos, n_npos, out);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
