// pair_overlap.hip -- read-through adapters cut by mate overlap (drprg_hip_pair_overlap; the rule: include/drprg_hip.h "mate overlap",
// DESIGN.md section 4).  Driven by Mapper::pair_overlap_device, which owns every buffer named here.
//
// Mates.  pair_mates_kernel: the reads of either side that lie in resident blocks come as two ascending lists of source numbers with the
// resident number of each beside it; one thread per read of side 1 looks its source number up in side 2's list (a binary search) and
// writes both mate entries.  A read without a partner keeps ~0u (the caller fills the array with it).
//
// Overlap.  pair_overlap_kernel: one wave per PAIR, that is per side-1 read: it judges the pair when the mate is present, else it passes its
// read on (an orphan, a read of no bases); pair_side2_kernel, one thread per side-2 read, passes on the side-2 reads no wave writes.  The
// waves of a workgroup share nothing but the twelve counters, so they meet at two barriers only (the counters zeroed, the counters added);
// between the stages of one pair a wave waits for its own LDS writes alone.  A judged pair is staged once in LDS (pair_stage.h, which
// pair_merge.hip stages its pairs with too):
// a's read-aligned 16-base words with a mask of its known bases (one bit per base, at the even bit of its letter: the same funnel shift
// moves letters and mask), and B = the reverse complement of b in the same form (b's words staged first, then every word of B is one
// window of b taken backwards: a bit reversal, the two bits of every letter swapped back, the complement an XOR).  Bases outside a read
// are unknown in the mask, so a shift needs no edge case: the shifts d = -(Lb-1) .. La-1 are spread over the lanes, a shift is a loop
// over the 16-base words of its columns -- two LDS words funnel-shifted at the phase of d against one aligned word of the other mate, XOR,
// AND with both masks, two popcounts -- and shifts with fewer than O columns are skipped.  Lanes of one round read neighbouring LDS words
// (16 consecutive shifts share theirs), so the loop was meant to be bound by VALU issue.  Measured (tools/pair_overlap_bench.py and one
// kernel trace): 15.4 ms per 5 M pairs of 150-base mates, 3.1 ns per pair -- five times the arithmetic guess (a
// first form with one wave per resident READ and barriers between the stages took 30.7 ms); a lane's loop still runs as long as the
// longest shift of its round and is not unrolled.  Which bound holds is UNMEASURED (no counter run).
// A lane keeps the best key (c, -x, d) of its shifts as one 64-bit word; one xor-shuffle reduction picks the wave's.  Lane 0 writes the
// shift and both kept lengths and adds the pair's counts to the workgroup's words in LDS; a workgroup adds every non-zero word once.
//
// Every index that comes from device data (mate numbers, where a read lies) is what the caller built from its own blocks; a mate number
// that is out of range or on the read's own side sets the error word and the read passes unchanged.
#include "device_common.h"
#include "pair_stage.h"
#include <rocprim/device/device_scan.hpp>

namespace drprg {
namespace dev {

constexpr int PO_THREADS = 256;
constexpr int PO_WAVES = PO_THREADS / 64;

__global__ __launch_bounds__(PO_THREADS) void pair_overlap_kernel(PairOverlapArgs a)
{
    __shared__ uint32_t s_rows[PO_WAVES][PO_ROWS][PO_ROW];
    __shared__ unsigned long long s_cnt[PO_WORDS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * PO_WAVES + wave;
    uint32_t (*s)[PO_ROW] = s_rows[wave];
    if (threadIdx.x < PO_WORDS) s_cnt[threadIdx.x] = 0;
    __syncthreads();

    // ---- what this wave does (all of it uniform in the wave) ----
    DedupLoc me {}, other {};
    uint32_t mt = ~0u;
    bool judged = false, too_long = false, passes = false; // passes: this wave writes keep[i] = the read's length
    if (i < a.n1) {
        me = a.loc[i];
        mt = a.mate[i];
        bool partner = false;
        if (mt != ~0u) {
            if (mt >= a.n || mt < a.n1) {
                if (lane == 0) *a.err = 1;
                mt = ~0u;
            } else {
                other = a.loc[mt];
                partner = other.len != 0;
            }
        }
        if (me.len == 0 || !partner) passes = true;
        else {
            too_long = me.len > PO_MAX_LEN || other.len > PO_MAX_LEN;
            judged = !too_long;
        }
    }
    const uint32_t La = judged ? (uint32_t)me.len : 0, Lb = judged ? (uint32_t)other.len : 0;

    po_stage_rows(s, me, other, judged, lane); // (pair_stage.h)
    // ---- the shifts ----
    unsigned long long best = 0;
    if (judged) {
        const uint32_t total = La + Lb - 1;
        for (uint32_t sidx = lane; sidx < total; sidx += 64) {
            const int32_t d = (int32_t)sidx - (int32_t)(Lb - 1);
            // the mate that is read at an offset (`up`) and the one that is read from its first base
            const uint32_t up = d >= 0 ? PO_A : PO_B, low = d >= 0 ? PO_B : PO_A;
            const uint32_t off = d >= 0 ? (uint32_t)d : (uint32_t)-d;
            const uint32_t ncol = d >= 0 ? min(La - off, Lb) : min(La, Lb - off);
            if (ncol < a.min_overlap) continue;
            const uint32_t nw = (ncol + 15) >> 4, base = off >> 4, sh = 2 * (off & 15u); // base + nw + 1 < PO_ROW: off + ncol <= PO_MAX_LEN
            uint32_t c = 0, x = 0;
            uint32_t lw = s[up][base], lk = s[up + 1][base];
            for (uint32_t t = 0; t < nw; ++t) {
                const uint32_t hw = s[up][base + t + 1], hk = s[up + 1][base + t + 1];
                const uint32_t k = po_funnel(lk, hk, sh) & s[low + 1][t];
                const uint32_t df = po_funnel(lw, hw, sh) ^ s[low][t];
                c += __popc(k);
                x += __popc((df | df >> 1) & k);
                lw = hw; lk = hk;
            }
            if (c >= a.min_overlap && 1000ull * x <= (unsigned long long)a.error_milli * c) {
                const unsigned long long key = (unsigned long long)c << 40 | (unsigned long long)(2047u - x) << 20 | (unsigned long long)(d + 2048);
                if (key > best) best = key;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long v = __shfl_xor(best, o);
            if (v > best) best = v;
        }
    }
    // ---- what comes of it ----
    if (lane == 0 && i < a.n1) {
        int32_t shift = PO_NOT_JUDGED;
        atomicAdd(&s_cnt[PO_BASES_BEFORE], (unsigned long long)me.len);
        if (passes) {
            a.keep[i] = me.len;
            if (me.len) {
                atomicAdd(&s_cnt[PO_ORPHANS], 1ull);
                atomicAdd(&s_cnt[PO_BASES_KEPT], (unsigned long long)me.len);
            }
        } else if (too_long) {
            a.keep[i] = me.len;
            a.keep[mt] = other.len;
            atomicAdd(&s_cnt[PO_TOO_LONG], 1ull);
            atomicAdd(&s_cnt[PO_BASES_KEPT], (unsigned long long)(me.len + other.len));
        } else if (judged) {
            uint32_t ka = La, kb = Lb;
            shift = PO_NO_SHIFT;
            atomicAdd(&s_cnt[PO_JUDGED], 1ull);
            if (best) {
                shift = (int32_t)(best & 0xFFFFFu) - 2048;
                const uint32_t ins = (uint32_t)((int32_t)Lb + shift); // 1 .. La + Lb - 1
                ka = min(La, ins);
                const uint32_t rtb = min(Lb, ins);
                kb = a.clip || a.merge ? (ins > La ? ins - La : 0u) : rtb;
                atomicAdd(&s_cnt[PO_OVERLAPPING], 1ull);
                if (ka < La || rtb < Lb) atomicAdd(&s_cnt[PO_READ_THROUGH], 1ull);
                if (La - ka + Lb - rtb) atomicAdd(&s_cnt[PO_BASES_CUT], (unsigned long long)(La - ka + Lb - rtb));
                if (rtb - kb) atomicAdd(&s_cnt[PO_BASES_CLIPPED], (unsigned long long)(rtb - kb));
                if (kb == 0 || a.merge) atomicAdd(&s_cnt[PO_READS_EMPTIED], 1ull); // (ka >= 1: ins >= 1)
                if (a.merge) { // mate merging: the clip's counts; a's place takes the merged read of `ins` bases (pair_merge.hip), b none
                    ka = ins;
                    kb = 0;
                }
            }
            a.keep[i] = ka;
            a.keep[mt] = kb;
            atomicAdd(&s_cnt[PO_BASES_KEPT], (unsigned long long)(ka + kb));
        }
        a.shift[i] = shift;
    }
    __syncthreads();
    if (threadIdx.x < PO_WORDS && s_cnt[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], s_cnt[threadIdx.x]);
}

// The side-2 reads no wave of pair_overlap_kernel writes: a read of no bases keeps none, a read without a present mate passes as an orphan.
// One thread per side-2 read; the three counts it touches go through the workgroup's words in LDS.
__global__ __launch_bounds__(PO_THREADS) void pair_side2_kernel(PairOverlapArgs a)
{
    __shared__ unsigned long long s_cnt[3]; // bases before, orphans, bases kept
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = a.n1 + (uint64_t)blockIdx.x * PO_THREADS + threadIdx.x;
    if (i < a.n) {
        const uint64_t len = a.loc[i].len;
        const uint32_t mt = a.mate[i];
        bool partner = false;
        if (mt != ~0u) {
            if (mt >= a.n1) *a.err = 1;
            else partner = a.loc[mt].len != 0;
        }
        if (len) atomicAdd(&s_cnt[0], (unsigned long long)len);
        if (len == 0) a.keep[i] = 0;
        else if (!partner) {
            a.keep[i] = len;
            atomicAdd(&s_cnt[1], 1ull);
            atomicAdd(&s_cnt[2], (unsigned long long)len);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt[0]) atomicAdd(&a.counts[PO_BASES_BEFORE], s_cnt[0]);
    if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(&a.counts[PO_ORPHANS], s_cnt[1]);
    if (threadIdx.x == 2 && s_cnt[2]) atomicAdd(&a.counts[PO_BASES_KEPT], s_cnt[2]);
}

// first index in s[0 .. n) whose value is not below key
__device__ inline uint32_t po_lower_bound(const uint32_t* __restrict__ s, uint32_t n, uint32_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PO_THREADS) void pair_mates_kernel(const uint32_t* __restrict__ src1, const uint32_t* __restrict__ res1, uint32_t m1,
    const uint32_t* __restrict__ src2, const uint32_t* __restrict__ res2, uint32_t m2, uint64_t n, uint32_t* __restrict__ mate, uint32_t* __restrict__ err)
{
    const uint64_t k = (uint64_t)blockIdx.x * PO_THREADS + threadIdx.x;
    if (k >= m1) return;
    const uint32_t key = src1[k];
    const uint32_t j = po_lower_bound(src2, m2, key);
    if (j >= m2 || src2[j] != key) return;
    const uint32_t r = res1[k], q = res2[j];
    if (r >= n || q >= n) {
        *err = 1;
        return;
    }
    mate[r] = q;
    mate[q] = r;
}

// out[rank of read i among the kept] = base + i for every read of a block that stays (flag null: all of them; take: only reads below it)
__global__ __launch_bounds__(PO_THREADS) void pair_numbers_kernel(const uint8_t* __restrict__ flag, const uint32_t* __restrict__ rank, uint64_t n_reads, uint64_t take,
    uint32_t base, uint64_t out_cap, uint32_t* __restrict__ out, uint32_t* __restrict__ err)
{
    const uint64_t i = (uint64_t)blockIdx.x * PO_THREADS + threadIdx.x;
    if (i >= n_reads || i >= take) return;
    if (flag && !flag[i]) return;
    const uint64_t at = flag ? rank[i] : i;
    if (at >= out_cap) {
        if (err) *err = 1;
        return;
    }
    out[at] = base + (uint32_t)i;
}

hipError_t launch_pair_numbers(const uint8_t* flag, const uint32_t* rank, uint64_t n_reads, uint64_t take, uint32_t base, uint64_t out_cap, uint32_t* out, uint32_t* err,
    hipStream_t stream)
{
    if (!n_reads || !out_cap) return hipSuccess;
    hipLaunchKernelGGL(pair_numbers_kernel, dim3((uint32_t)((n_reads + PO_THREADS - 1) / PO_THREADS)), dim3(PO_THREADS), 0, stream, flag, rank, n_reads, take, base,
        out_cap, out, err);
    return hipGetLastError();
}

hipError_t launch_pair_mates(const uint32_t* src1, const uint32_t* res1, uint32_t m1, const uint32_t* src2, const uint32_t* res2, uint32_t m2, uint64_t n, uint32_t* mate,
    uint32_t* err, hipStream_t stream)
{
    if (!m1 || !m2) return hipSuccess;
    hipLaunchKernelGGL(pair_mates_kernel, dim3((m1 + PO_THREADS - 1) / PO_THREADS), dim3(PO_THREADS), 0, stream, src1, res1, m1, src2, res2, m2, n, mate, err);
    return hipGetLastError();
}

hipError_t launch_pair_offsets(const uint64_t* keep, uint64_t n_reads, uint64_t* noff, void* temp, size_t temp_bytes, hipStream_t stream)
{
    return rocprim::exclusive_scan(temp, temp_bytes, keep, noff, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_pair_overlap(const PairOverlapArgs& a, hipStream_t stream)
{
    if (!a.n) return hipSuccess;
    if (a.n >= (1ull << 32) || a.n1 > a.n || a.min_overlap < 1 || a.min_overlap > PO_MAX_LEN || a.error_milli > 1000) return hipErrorInvalidValue;
    if (a.n1) {
        hipLaunchKernelGGL(pair_overlap_kernel, dim3((uint32_t)((a.n1 + PO_WAVES - 1) / PO_WAVES)), dim3(PO_THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (a.n > a.n1) {
        hipLaunchKernelGGL(pair_side2_kernel, dim3((uint32_t)((a.n - a.n1 + PO_THREADS - 1) / PO_THREADS)), dim3(PO_THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

} // namespace dev
} // namespace drprg
