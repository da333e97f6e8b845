// read_trim_piece.h -- read trimming (include/drprg_hip.h "read trimming") in integer arithmetic: the fixed crop, the
// window test, and what trim_points_kernel (read_trim.hip) does with the 16 window starts one lane takes per round.  Host code as well
// (nothing here needs the HIP headers), so that a CPU build can walk the index arithmetic under a sanitizer with the buffers at their exact
// sizes (tools/read_trim_walk.cpp).
//
// Everything is stated in STORED order: the order of the quality bytes.  A BAM record with flag 0x10 stores its qualities mirrored, and the
// rule is mirror-symmetric, so such a read is trimmed in stored order with `front` and `tail` swapped and its range is mirrored at the end
// (rt_crop below, trim_tables_kernel).
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

constexpr uint32_t RT_MAX_QUAL = 93;
constexpr uint32_t RT_MAX_QUAL_MILLI = 93000;
constexpr uint32_t RT_MAX_WINDOW = 32;
constexpr uint32_t RT_DEFAULT_WINDOW = 4;
constexpr uint32_t RT_LANE_STARTS = 16;                                  // window starts per lane and round
constexpr uint32_t RT_LANE_WORDS = (RT_LANE_STARTS + RT_MAX_WINDOW) / 4; // 12: the 16 bytes and up to 31 behind them, rounded up to words
constexpr uint32_t RT_NONE = 0xFFFFFFFFu;                                // "no good window" in the array of smallest starts (0 in the array of largest start + 1)
constexpr uint64_t RT_MAX_READ = 1ull << 31;                             // starts are 32-bit words: a longer read is refused with the offsets

// The fixed crop of a read of L bases, in stored order: [lo, hi).  In read orientation a0 = min(front, L), b0 = L - min(tail, L - a0).
DRPRG_HD inline void rt_crop(uint64_t L, uint64_t front, uint64_t tail, bool rev, uint64_t& lo, uint64_t& hi)
{
    const uint64_t a0 = front < L ? front : L;
    const uint64_t t = tail < L - a0 ? tail : L - a0;
    const uint64_t b0 = L - t;
    lo = rev ? L - b0 : a0;
    hi = rev ? L - a0 : b0;
}

// What a window sum of RAW bytes is compared with: good iff 1000 * (sum of q) >= qual_milli * W, q = byte - bias, which is
// 1000 * (sum of bytes) >= (qual_milli + 1000 * bias) * W, which is sum of bytes >= the ceiling of that over 1000.  Below 2^13.
DRPRG_HD inline uint32_t rt_window_threshold(uint32_t qual_milli, uint32_t bias, uint32_t W) { return ((qual_milli + 1000u * bias) * W + 999u) / 1000u; }
// the same for one base (the narrowing of the range's two ends)
DRPRG_HD inline bool rt_base_good(uint32_t byte, uint32_t bias, uint32_t qual_milli) { return 1000u * byte >= qual_milli + 1000u * bias; }

// Bit 7 of byte k of the result is set iff byte k of x lies outside [bias, bias + 93] (bias <= 34: the upper end stays below 128): four
// range tests in six operations, no carry or borrow crosses a byte.  The kernel looks for the first bad byte only where this is non-zero.
DRPRG_HD inline uint32_t rt_bad_bytes(uint32_t x, uint32_t bias)
{
    const uint32_t x7 = x & 0x7F7F7F7Fu;
    const uint32_t at_least = (x7 | 0x80808080u) - bias * 0x01010101u;               // bit 7 stays iff the byte's low seven bits are >= bias
    const uint32_t above = x7 + (0x7Fu - (bias + RT_MAX_QUAL)) * 0x01010101u;        // bit 7 comes up iff they are > bias + 93
    return (x | ~at_least | above) & 0x80808080u;
}

DRPRG_HD inline uint32_t rt_byte_sum(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(x, 0u, 0u);
#else
    return (x & 0xFFu) + ((x >> 8) & 0xFFu) + ((x >> 16) & 0xFFu) + (x >> 24);
#endif
}

// w: the 48 bytes from a lane's first window start on, little-endian words.  Bit j of the result: the W bytes from byte j on sum to at
// least thr (rt_window_threshold).  1 <= W <= 32.  A running sum: the first window by masked byte sums, every further one adds the byte
// that enters and takes off the byte that leaves; the entering bytes are the 16 bytes at byte W, funnel-shifted out of five words picked
// by a uniform W / 4 (constant indices everywhere: on the device the twelve words stay in registers).
DRPRG_HD inline uint32_t rt_good_bits(const uint32_t (&w)[RT_LANE_WORDS], uint32_t W, uint32_t thr)
{
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < RT_MAX_WINDOW / 4; ++k) {
        const uint32_t m = 4 * k + 4 <= W ? 0xFFFFFFFFu : (4 * k >= W ? 0u : (1u << (8 * (W - 4 * k))) - 1u);
        s += rt_byte_sum(w[k] & m);
    }
    uint32_t u[5] = { 0, 0, 0, 0, 0 };
    const uint32_t wq = W >> 2, sh = (W & 3u) * 8u;
#pragma unroll
    for (uint32_t c = 0; c <= RT_MAX_WINDOW / 4; ++c)
        if (c == wq) {
#pragma unroll
            for (uint32_t k = 0; k < 5; ++k) u[k] = c + k < RT_LANE_WORDS ? w[c + k] : 0u;
        }
    uint32_t t[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) t[k] = (uint32_t)(((((uint64_t)u[k + 1]) << 32) | u[k]) >> sh);
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t j = 0; j < RT_LANE_STARTS; ++j) {
        bits |= (s >= thr ? 1u : 0u) << j;
        s += (t[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        s -= (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
    }
    return bits;
}

// The window starts [p, p + n) of a batch's quality buffer (1 <= n <= 16, p + n <= n_bases) and `good`, their bits from rt_good_bits.
// r: a read at or before the one that holds byte p; moved on to the read that holds the last of the bytes.  Calls emit(read, first, last1)
// for every read that has a good AND valid start here, in ascending order: first = the smallest such start, last1 = the largest + 1, both
// counted from the read's cropped start (rt_crop's lo).  A start i is valid for its read iff lo <= i and i + W <= hi.  Reads whose offsets
// do not ascend inside n_bases are stepped over (trim_tables_kernel refuses the batch); nothing is indexed by what they hold.
template <typename Emit>
DRPRG_HD inline void rt_piece(const uint64_t* offsets, const uint8_t* rev, uint64_t n_reads, uint64_t n_bases, uint64_t p, uint32_t n, uint32_t good, uint32_t W,
    uint64_t front, uint64_t tail, uint64_t& r, Emit&& emit)
{
    while (r + 1 < n_reads && offsets[r + 1] <= p) ++r;
    while (true) {
        const uint64_t s = offsets[r], e = r + 1 < n_reads ? offsets[r + 1] : n_bases;
        if (s <= e && e <= n_bases && e - s < RT_MAX_READ) {
            uint64_t lo, hi;
            rt_crop(e - s, front, tail, rev && rev[r], lo, hi);
            lo += s;
            hi += s;
            if (hi - lo >= W) {
                const uint64_t from = lo > p ? lo : p, to = hi - W < p + n - 1 ? hi - W : p + n - 1; // the valid starts among ours: [from, to]
                if (from <= to) {
                    const uint32_t f = (uint32_t)(from - p), t = (uint32_t)(to - p); // 0 <= f <= t <= 15
                    const uint32_t m = good & ((0xFFFFu >> (15u - t)) & (0xFFFFu << f));
                    if (m) emit(r, (uint32_t)(p + (uint32_t)__builtin_ctz(m) - lo), (uint32_t)(p + (31u - (uint32_t)__builtin_clz(m)) - lo) + 1u);
                }
            }
        }
        if (r + 1 < n_reads && offsets[r + 1] < p + n) ++r;
        else break;
    }
}

// The kept range of one read in stored order from what the windows said (first, last1: the smallest good start and the largest + 1,
// counted from lo; RT_NONE / 0: none), narrowed from either end while the end base is below Q.  q: the read's quality bytes in stored order
// (indexed 0 .. L - 1).  [a, b) on return; empty ranges are [0, 0).  A good window holds a base at or above Q, so each walk ends inside its
// edge window; both are bounded by the range all the same.
DRPRG_HD inline void rt_range(const uint8_t* q, uint64_t lo, uint64_t hi, uint32_t first, uint32_t last1, uint32_t W, uint32_t bias, uint32_t qual_milli,
    uint64_t& a, uint64_t& b)
{
    a = b = 0;
    if (first == RT_NONE || last1 == 0 || last1 - 1 < first) return;
    uint64_t x = lo + first, y = lo + (last1 - 1) + W;
    if (y > hi || x >= y) return; // (what the points kernel cannot have written)
    while (x < y && !rt_base_good(q[x], bias, qual_milli)) ++x;
    while (y > x && !rt_base_good(q[y - 1], bias, qual_milli)) --y;
    if (x < y) {
        a = x;
        b = y;
    }
}

} // namespace dev
} // namespace drprg
