// covg_cut.hip -- where a device batch crosses the depth cap (drprg_hip_set_max_covg; DESIGN.md section 4 "depth cap").
//
// A device batch's read offsets exist only in HBM.  The host knows the batch's n_bases, so it knows WHETHER the batch reaches the cap
// without asking the device; only the one batch that does is looked at here: the smallest i with offsets[i] >= target, and -- for a
// packed batch -- how many of its listed non-ACGT positions lie below offsets[i].  One wave, a 64-way search (first_at_least, search.h: the
// range shrinks 64-fold per round, five rounds for 2^28 reads).  Latency-bound: <= 5 + 5
// rounds of one 8-byte load per lane, no LDS, nothing to tune.  Launched at most once per context between resets.
#include "search.h"

namespace drprg {
namespace dev {

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
