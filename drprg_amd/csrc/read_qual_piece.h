// read_qual_piece.h -- the read filter's mean-quality test in integer arithmetic (include/drprg_hip.h "read filter"):
// the table E, the threshold T, and what read_qual_kernel (read_qual.hip) does with the up to 16 quality bytes one lane loads.  Host code
// as well (nothing here needs the HIP headers), so that a CPU build can walk the index arithmetic under a sanitizer with the buffers at
// their exact sizes (tools/read_qual_walk.cpp).
#pragma once
#include <cstdint>

#ifndef DRPRG_HD
#if defined(__HIPCC__)
#define DRPRG_HD __host__ __device__
#else
#define DRPRG_HD
#endif
#endif

namespace drprg {
namespace dev {

constexpr uint32_t RQ_MAX_QUAL = 93;
constexpr uint32_t RQ_MAX_QUAL_MILLI = 93000;
// E[q] = round(2^31 * 10^(-q / 10)), q = 0 .. 93: the error probability of Phred quality q in units of 2^-31
constexpr uint32_t RQ_E[RQ_MAX_QUAL + 1] = {
    2147483648u, 1705806895u, 1354970580u, 1076291389u, 854928639u, 679093957u, 539423504u, 428479319u,
    340353221u, 270352174u, 214748365u, 170580690u, 135497058u, 107629139u, 85492864u, 67909396u,
    53942350u, 42847932u, 34035322u, 27035217u, 21474836u, 17058069u, 13549706u, 10762914u,
    8549286u, 6790940u, 5394235u, 4284793u, 3403532u, 2703522u, 2147484u, 1705807u,
    1354971u, 1076291u, 854929u, 679094u, 539424u, 428479u, 340353u, 270352u,
    214748u, 170581u, 135497u, 107629u, 85493u, 67909u, 53942u, 42848u,
    34035u, 27035u, 21475u, 17058u, 13550u, 10763u, 8549u, 6791u,
    5394u, 4285u, 3404u, 2704u, 2147u, 1706u, 1355u, 1076u,
    855u, 679u, 539u, 428u, 340u, 270u, 215u, 171u,
    135u, 108u, 85u, 68u, 54u, 43u, 34u, 27u,
    21u, 17u, 14u, 11u, 9u, 7u, 5u, 4u,
    3u, 3u, 2u, 2u, 1u, 1u,
};
static_assert(RQ_E[0] == 0x80000000u && RQ_E[RQ_MAX_QUAL] == 1u, "the table's ends");

// T of the rule: a read of L bases whose E sum to S is kept iff S <= L * T.  Host only.
inline uint64_t rq_threshold(uint32_t min_qual_milli)
{
    if (min_qual_milli % 1000 == 0) return RQ_E[min_qual_milli / 1000];
    return (uint64_t)__builtin_floor(2147483648.0 * __builtin_pow(10.0, -(double)min_qual_milli / 10000.0) + 0.5);
}

// The bytes [p, p + n) of a batch's quality buffer (1 <= n <= 16, p + n <= offsets[n_reads]); e[j]: E of byte p + j.  r: a read at or
// before the one that holds byte p; moved on to the read that holds the LAST of the bytes.  Returns the sum of the bytes that belong to
// the read that holds byte p -- head_read receives that read -- and calls rest(read, sum) for every further read that has bytes here, in
// ascending order.  Empty reads own no byte and are stepped over.  (One loop of constant trip count and constant indices into e: on the
// device the sixteen values stay in registers.)
template <typename Rest>
DRPRG_HD inline uint64_t rq_piece(const uint64_t* offsets, uint64_t n_reads, uint64_t p, uint32_t n, const uint32_t (&e)[16], uint64_t& r, uint64_t& head_read,
    Rest&& rest)
{
    while (r + 1 < n_reads && offsets[r + 1] <= p) ++r;
    head_read = r;
    uint64_t end = r + 1 < n_reads ? offsets[r + 1] : ~0ull; // (the last read takes whatever is left: nothing is indexed by it)
    uint64_t head_sum = 0, acc = 0;
    if (n == 16 && end - p >= 16) { // all sixteen bytes inside the head read -- nearly every piece of a batch of long reads: no test per byte
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) acc += e[j];
        return acc;
    }
    bool in_head = true;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        if (j >= n) continue;
        if (p + j >= end) { // byte p + j belongs to a later read
            if (in_head) head_sum = acc;
            else rest(r, acc);
            in_head = false;
            acc = 0;
            while (r + 1 < n_reads && offsets[r + 1] <= p + j) ++r;
            end = r + 1 < n_reads ? offsets[r + 1] : ~0ull;
        }
        acc += e[j];
    }
    if (in_head) return acc;
    rest(r, acc);
    return head_sum;
}

} // namespace dev
} // namespace drprg
