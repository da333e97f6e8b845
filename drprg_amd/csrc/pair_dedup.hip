// pair_dedup.hip -- duplicate read PAIRS dropped from the resident sample (drprg_hip_dedup_pairs; the rule: include/drprg_hip.h
// "duplicate pairs").  Driven by Mapper::dedup_pairs_kept and Mapper::dedup_pairs_device, which own every buffer named
// here.  The per-read content keys are dedup_keys_kernel's (dedup.hip), the places of the reads dedup_loc_kernel's, the sort the hit
// list's radix sort, the compaction behind the flags keep_flagged's.  What is new is the unit: a source pair (A_s, B_s).
//
// Units.  pd_scatter_kernel, one thread per resident read: unit[2 s + side] = the read's resident number, s its source pair.
// pd_unit_kernel, one thread per source pair: both reads' DedupLoc and keys are gathered (two 32-byte and two 8-byte loads at unrelated
// places), the mates are checked to name each other, U = fin(ka + G) + fin(kb + 2 G) is written with its masked copy for the sort.
// Meant to be bound by the latency of those gathers: 80 bytes of useful data per pair.
//
// Exact check.  pd_check_kernel, one thread per sorted entry, walks back through its run of equal masked keys, predecessor first: both
// lengths, then the words of A, then of B (dd_read_word).  It records the identical predecessor it found (root[s] = h, else s).  A true
// duplicate costs one comparison -- its nearest copy stands right in front of it --, only key collisions walk further.  Meant to be bound
// by the gathers of the two reads' words (2 x 40 bytes per 150-base mate and unit compared, each read by one lane: no coalescing).
//
// The class's first unit.  The links point at the NEAREST copy, so a stack of c copies is a chain of c - 1 links.  pd_jump_kernel is
// pointer doubling in place: root[s] = root[root[s]], PD_ROUNDS rounds at the most; a round in which the one before it changed nothing
// returns at once (a word per round in device memory: no read-back between the rounds).  Links only ever point at smaller numbers
// (pd_check_kernel refuses any other), so there is no cycle and a lane that reads a link another lane is moving reads an ancestor
// either way.  Meant to be bound by 4-byte gathers: two per unit and live round.
//
// Copies, levels, flags.  pd_copies_kernel runs over the SORTED entries, where the copies of one class stand together: the lanes of a wave
// that hold one first unit in a row add their count once (a ballot, the distance to the next run's head), so the deep stack costs one
// atomic per wave and not one per copy.  pd_finish_kernel, one thread per unit: keep[s], the four counts and the 32 levels through the
// workgroup's words in LDS, and the flags of the unit's reads with bases cleared (pd_reads_kernel has set every read's to 1); then the two
// exclusive scans keep_flagged reads.
//
// Measured (tools/pair_dedup_bench.py and one kernel trace), 5 M pairs of 150-base mates: pd_unit_kernel 0.13 ms,
// pd_check_kernel 0.41 ms without duplicates and 0.67 ms with one stack of 1 M copies, the 32 pd_jump_kernel launches 0.24 ms together,
// pd_copies_kernel 0.24 to 0.34 ms, pd_finish_kernel 0.24 ms; with the keys (0.85 ms), the sort (0.5 ms) and the scans 3.3 ms of kernels in
// a call of 6.7 ms, the rest being the call's allocations, memsets and launch gaps.  Which bound holds in any of the kernels is UNMEASURED
// (no counter run).
//
// Every index that comes from device data (source numbers, mates, sorted unit numbers, links) is compared with the size of what it
// indexes before it is used; a mismatch sets the error word the host looks at and writes nothing out of bounds.
#include "search.h"
#include "dedup_word.h"
#include <rocprim/device/device_scan.hpp>

namespace drprg {
namespace dev {

constexpr int PD_THREADS = 256;
constexpr uint32_t PD_NONE = ~0u;

__global__ __launch_bounds__(PD_THREADS) void pd_source_numbers_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ res, uint32_t m, uint64_t n,
    uint32_t* __restrict__ srcno, uint32_t* __restrict__ err)
{
    const uint64_t k = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x;
    if (k >= m) return;
    const uint32_t r = res[k];
    if (r >= n) {
        *err = 1;
        return;
    }
    srcno[r] = src[k];
}

__global__ __launch_bounds__(PD_THREADS) void pd_scatter_kernel(PairDedupArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t s = a.srcno[i];
    if (s == PD_NONE) return;
    if (s >= a.pairs) {
        *a.err = 1;
        return;
    }
    a.unit[2ull * s + (i >= a.n1 ? 1 : 0)] = (uint32_t)i;
}

// the resident number of one side of unit s, PD_NONE for none; a number that is not one of its side's sets the error word
__device__ inline uint32_t pd_side(const PairDedupArgs& a, uint64_t s, int side)
{
    const uint32_t r = a.unit[2 * s + side];
    if (r == PD_NONE) return r;
    if (r >= a.n || (side == 0) != (r < a.n1)) {
        *a.err = 1;
        return PD_NONE;
    }
    return r;
}

__device__ inline DedupLoc pd_loc(const PairDedupArgs& a, uint32_t r)
{
    if (r == PD_NONE) return DedupLoc { nullptr, nullptr, 0, 0 };
    return a.loc[r];
}

__global__ __launch_bounds__(PD_THREADS) void pd_unit_kernel(PairDedupArgs a, uint64_t mask)
{
    const uint64_t s = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x;
    if (s >= a.pairs) return;
    const uint32_t ra = pd_side(a, s, 0), rb = pd_side(a, s, 1);
    if (ra != PD_NONE && rb != PD_NONE && (a.mate[ra] != rb || a.mate[rb] != ra)) *a.err = 1;
    const uint64_t la = ra == PD_NONE ? 0 : a.loc[ra].len, lb = rb == PD_NONE ? 0 : a.loc[rb].len;
    const uint64_t ka = la ? a.rkey[ra] : 0, kb = lb ? a.rkey[rb] : 0;
    const uint64_t U = dd_fin(ka + DD_GOLDEN) + dd_fin(kb + 2 * DD_GOLDEN);
    a.ukey[s] = U;
    a.skey[s] = U & mask;
    a.idx[s] = (uint32_t)s;
    a.ubases[s] = (uint8_t)((la ? 1 : 0) | (lb ? 2 : 0));
}

__device__ inline bool pd_identical(const DedupLoc& x, const DedupLoc& y)
{
    const uint64_t n_words = (x.len + 15) >> 4; // (the lengths are equal: the caller has looked)
    for (uint64_t j = 0; j < n_words; ++j)
        if (dd_read_word(x.words, x.bits, x.start, x.len, j) != dd_read_word(y.words, y.bits, y.start, y.len, j)) return false;
    return true;
}

// The sort is stable and idx ascends going in, so the entries of one masked key stand in ascending order of unit: every unit in front of p
// in its run has a smaller number.
__global__ __launch_bounds__(PD_THREADS) void pd_check_kernel(PairDedupArgs a)
{
    const uint64_t p = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x;
    if (p >= a.pairs) return;
    const uint32_t s = a.idx_sorted[p];
    if (s >= a.pairs) {
        *a.err = 1;
        return;
    }
    uint32_t pred = s;
    const DedupLoc A = pd_loc(a, pd_side(a, s, 0)), B = pd_loc(a, pd_side(a, s, 1));
    if (A.len | B.len) { // (a unit of no bases is never a duplicate and never makes one)
        const uint64_t k = a.skey_sorted[p];
        for (uint64_t q = p; q-- > 0 && a.skey_sorted[q] == k;) {
            const uint32_t h = a.idx_sorted[q];
            if (h >= s) { // (h >= pairs among them; a link must point at a smaller number, or the doubling below could run in a circle)
                *a.err = 1;
                break;
            }
            const DedupLoc Ah = pd_loc(a, pd_side(a, h, 0)), Bh = pd_loc(a, pd_side(a, h, 1));
            if (Ah.len != A.len || Bh.len != B.len) continue;
            if (pd_identical(Ah, A) && pd_identical(Bh, B)) {
                pred = h;
                break;
            }
        }
    }
    a.root[s] = pred;
}

__global__ __launch_bounds__(PD_THREADS) void pd_jump_kernel(uint32_t* root, uint64_t pairs, uint32_t* changed, int round, uint32_t* err)
{
    if (round > 0 && changed[round - 1] == 0) return; // (uniform: the round before this one moved no link, so none is left to move)
    const uint64_t s = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x;
    if (s >= pairs) return;
    const uint32_t r = root[s];
    if (r > s) {
        *err = 1;
        return;
    }
    const uint32_t rr = root[r];
    if (rr > r) {
        *err = 1;
        return;
    }
    if (rr != r) {
        root[s] = rr;
        changed[round] = 1;
    }
}

__global__ __launch_bounds__(PD_THREADS) void pd_copies_kernel(PairDedupArgs a)
{
    const uint64_t p = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t r = PD_NONE; // (no lane leaves before the ballot)
    if (p < a.pairs) {
        const uint32_t s = a.idx_sorted[p];
        if (s >= a.pairs) *a.err = 1;
        else if (a.ubases[s]) {
            r = a.root[s];
            if (r > s || a.root[r] != r) { // (r <= s < pairs) a link that has not reached its class's first unit
                *a.err = 1;
                r = PD_NONE;
            }
        }
    }
    const uint32_t before = __shfl_up(r, 1);
    const bool head = lane == 0 || before != r;
    const unsigned long long heads = __ballot(head);
    if (head && r != PD_NONE) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const uint32_t run = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
        atomicAdd(&a.copies[r], run);
    }
}

// flag[i] = 1, flag32[i] = 1, klen[i] = the read's length for every resident read; entry n of the two the scans read: 0
__global__ __launch_bounds__(PD_THREADS) void pd_reads_kernel(PairDedupArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x;
    if (i > a.n) return;
    if (i == a.n) {
        a.flag32[i] = 0;
        a.klen[i] = 0;
        return;
    }
    a.flag[i] = 1;
    a.flag32[i] = 1;
    a.klen[i] = a.loc[i].len;
}

__global__ __launch_bounds__(PD_THREADS) void pd_finish_kernel(PairDedupArgs a)
{
    __shared__ uint32_t s_cnt[PD_WORDS];
    if (threadIdx.x < PD_WORDS) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t s = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x;
    if (s < a.pairs) {
        const uint32_t hb = a.ubases[s], r = a.root[s];
        bool dup = false;
        if (hb) {
            atomicAdd(&s_cnt[PD_WITH_BASES], 1u);
            if (hb == 3) atomicAdd(&s_cnt[PD_BOTH], 1u);
            if (r > s) *a.err = 1;
            else dup = r != s;
            if (dup) {
                atomicAdd(&s_cnt[PD_DROPPED], 1u);
                for (int side = 0; side < 2; ++side) {
                    if (!(hb >> side & 1)) continue; // (a read of no bases is always kept)
                    const uint32_t i = pd_side(a, s, side);
                    if (i == PD_NONE) continue;
                    a.flag[i] = 0;
                    a.flag32[i] = 0;
                    a.klen[i] = 0;
                }
            } else {
                const uint32_t c = a.copies[s];
                if (c == 0) *a.err = 1;
                else atomicAdd(&s_cnt[PD_LEVELS + (c > 32 ? 32 : c) - 1], 1u);
            }
        }
        a.keep[s] = dup ? 0 : 1;
    }
    __syncthreads();
    if (threadIdx.x < PD_WORDS && s_cnt[threadIdx.x]) atomicAdd(&a.out[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

hipError_t launch_pair_source_numbers(const uint32_t* src, const uint32_t* res, uint32_t m, uint64_t n, uint32_t* srcno, uint32_t* err, hipStream_t stream)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(pd_source_numbers_kernel, dim3((m + PD_THREADS - 1) / PD_THREADS), dim3(PD_THREADS), 0, stream, src, res, m, n, srcno, err);
    return hipGetLastError();
}

hipError_t launch_pair_dedup(const PairDedupArgs& a, hipStream_t stream)
{
    const uint64_t n = a.n, P = a.pairs;
    if (!P || P >= (1ull << 32) || n >= (1ull << 32) || a.n1 > n || a.key_bits < 1 || a.key_bits > 64) return hipErrorInvalidValue;
    size_t temp_bytes = a.temp_bytes; // (rocPRIM takes it by reference)
    const dim3 block(PD_THREADS), grid_p((uint32_t)((P + PD_THREADS - 1) / PD_THREADS)), grid_n1((uint32_t)((n + 1 + PD_THREADS - 1) / PD_THREADS));
    const uint64_t mask = a.key_bits == 64 ? ~0ull : (1ull << a.key_bits) - 1;
    HIP_TRY(hipMemsetAsync(a.unit, 0xFF, 2 * P * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(a.copies, 0, P * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(a.changed, 0, (PD_ROUNDS + 1) * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(a.out, 0, PD_WORDS * sizeof(unsigned long long), stream));
    if (n) {
        hipLaunchKernelGGL(pd_scatter_kernel, dim3((uint32_t)((n + PD_THREADS - 1) / PD_THREADS)), block, 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pd_unit_kernel, grid_p, block, 0, stream, a, mask);
    HIP_TRY(hipGetLastError());
    // (masked key, s) ascending: idx ascends going in and the sort is stable -- pd_check_kernel relies on it
    HIP_TRY(sort_hits(a.temp, a.temp_bytes, a.skey, a.skey_sorted, a.idx, a.idx_sorted, (uint32_t)P, stream));
    hipLaunchKernelGGL(pd_check_kernel, grid_p, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    for (int round = 0; round < PD_ROUNDS; ++round) {
        hipLaunchKernelGGL(pd_jump_kernel, grid_p, block, 0, stream, a.root, P, a.changed, round, a.err);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pd_copies_kernel, grid_p, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pd_reads_kernel, grid_n1, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pd_finish_kernel, grid_p, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::exclusive_scan(a.temp, temp_bytes, a.flag32, a.rank, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), stream));
    HIP_TRY(rocprim::exclusive_scan(a.temp, temp_bytes, a.klen, a.boff, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), stream));
    return hipSuccess;
}

} // namespace dev
} // namespace drprg
