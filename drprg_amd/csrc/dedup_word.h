// dedup_word.h -- the word arithmetic of duplicate removal (include/drprg_hip.h "duplicate reads"): the read-aligned
// words x_j of a read made from the packed words of the batch it lies in, the content key, and what dedup_keys_kernel (dedup.hip) does
// with one 16-base window of the batch.  Host code as well (nothing here needs the HIP headers), so that a CPU build can walk the index
// arithmetic under a sanitizer with the buffers at their exact sizes (tools/dedup_walk.cpp).
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

constexpr uint64_t DD_GOLDEN = 0x9E3779B97F4A7C15ull;

// the splitmix64 finaliser ("random subsample" in the header states it)
DRPRG_HD inline uint64_t dd_fin(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// bit t of m -> bits 2t and 2t + 1 (m < 2^16): the letter bits under the mask bits
DRPRG_HD inline uint32_t dd_spread(uint32_t m)
{
    m = (m | m << 8) & 0x00FF00FFu;
    m = (m | m << 4) & 0x0F0F0F0Fu;
    m = (m | m << 2) & 0x33333333u;
    m = (m | m << 1) & 0x55555555u;
    return m * 3u;
}

// x_j of the rule for the `len` (1..16) bases that start at phase `phase` (0..15) of the batch word lo and run on into hi: a funnel shift
// of the two words and of their two 16-bit rows of the bitmap, bases beyond the read's end cleared, letters under mask bits forced to 0
DRPRG_HD inline uint64_t dd_x(uint32_t lo, uint32_t hi, uint32_t mlo, uint32_t mhi, uint32_t phase, uint32_t len)
{
    uint32_t v = (uint32_t)(((uint64_t)hi << 32 | lo) >> (2 * phase));
    uint32_t m = (((mhi & 0xFFFFu) << 16 | (mlo & 0xFFFFu)) >> phase) & 0xFFFFu;
    if (len < 16) {
        v &= (1u << (2 * len)) - 1u;
        m &= (1u << len) - 1u;
    }
    if (m) v &= ~dd_spread(m);
    return (uint64_t)v | (uint64_t)m << 32;
}

// what word j of a read adds to its key; word 0 carries the length L as well
DRPRG_HD inline uint64_t dd_term(uint64_t x, uint64_t j) { return dd_fin(x + DD_GOLDEN * (j + 1)); }
DRPRG_HD inline uint64_t dd_length_term(uint64_t L) { return dd_fin(DD_GOLDEN * L); }

// A packed batch as the key kernel sees it.  words: ceil(n_bases / 16); bits: the bitmap launch_mark_npos makes of the listed positions,
// one u16 per word, or null when the batch lists none.
struct DedupBatch {
    const uint32_t* words;
    const uint16_t* bits;
    const uint64_t* offsets; // n_reads + 1
    uint64_t n_reads, n_bases;
};

// x_j of the read that starts at base `start` of the batch and is `len` bases long (16 j < len; start + len <= n_bases), straight from
// memory: what the exact check compares.  The second word is touched only when the 16 (or fewer) bases reach into it.
DRPRG_HD inline uint64_t dd_read_word(const uint32_t* words, const uint16_t* bits, uint64_t start, uint64_t len, uint64_t j)
{
    const uint64_t b = start + 16 * j;
    const uint32_t n = (uint32_t)(len - 16 * j < 16 ? len - 16 * j : 16);
    const uint64_t w = b >> 4;
    const uint32_t phase = (uint32_t)(b & 15u);
    const bool two = phase + n > 16;
    return dd_x(words[w], two ? words[w + 1] : 0u, bits ? bits[w] : 0u, bits && two ? bits[w + 1] : 0u, phase, n);
}

// The window of bases [P, P + 16) of the batch (P a multiple of 16, P < n_bases); lo / hi: the batch words P / 16 and P / 16 + 1 (hi: 0
// when there is none), mlo / mhi their rows of the bitmap.  Every read-aligned word whose FIRST base lies in the window is handled here and
// nowhere else: for the read that holds base P that is the one word j = ceil((P - start) / 16) -- if the read reaches that far --, and
// every read that starts behind P inside the window adds its word 0.  emit(read, term) is called once per such word, in ascending order of
// read.  r: a read at or before the one that holds base P; moved on to the last read looked at.  bad is set, and the read skipped, when
// its offsets do not ascend or leave the batch.
template <typename Emit>
DRPRG_HD inline void dd_window(const DedupBatch& b, uint64_t P, uint32_t lo, uint32_t hi, uint32_t mlo, uint32_t mhi, uint64_t& r, bool& bad, Emit&& emit)
{
    while (r + 1 < b.n_reads && b.offsets[r + 1] <= P) ++r;
    const uint64_t wend = P + 16;
    {
        const uint64_t s = b.offsets[r], e = b.offsets[r + 1];
        if (s > P || e < s || e > b.n_bases) bad = true;
        else {
            const uint64_t j = (P - s + 15) >> 4, at = s + 16 * j; // P <= at < P + 16
            if (at < e) {
                const uint32_t n = (uint32_t)(e - at < 16 ? e - at : 16);
                uint64_t t = dd_term(dd_x(lo, hi, mlo, mhi, (uint32_t)(at - P), n), j);
                if (j == 0) t += dd_length_term(e - s);
                emit(r, t);
            }
        }
    }
    while (r + 1 < b.n_reads && b.offsets[r + 1] < wend) {
        ++r;
        const uint64_t s = b.offsets[r], e = b.offsets[r + 1];
        if (s <= P || e < s || e > b.n_bases) { // (s <= P: behind a read that starts later -- the offsets do not ascend)
            bad = true;
            continue;
        }
        if (e == s) continue; // a read of no bases has no word
        const uint32_t n = (uint32_t)(e - s < 16 ? e - s : 16);
        emit(r, dd_term(dd_x(lo, hi, mlo, mhi, (uint32_t)(s - P), n), 0) + dd_length_term(e - s));
    }
}

} // namespace dev
} // namespace drprg
