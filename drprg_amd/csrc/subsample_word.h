// subsample_word.h -- the word assembly of the packed compaction (subsample.hip): one output word of a batch that holds only the kept
// reads, made from the packed words of the batch they came from.  Host code as well (nothing here needs the HIP headers), so that a CPU
// build can walk the index arithmetic under a sanitizer with the buffers at their exact sizes (tools/subsample_walk.cpp).
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

// The kept reads of one resident packed batch, as the compaction sees them: read r of the new batch is bases [new_offsets[r],
// new_offsets[r + 1]) of it and bases [src_start[r], ..) of the old one.  src_words: the old batch's ceil(src_bases / 16) words.
struct CompactBatch {
    const uint32_t* src_words;
    uint64_t src_bases;
    const uint64_t* new_offsets; // n_reads + 1, ascending, [0] = 0, [n_reads] = n_bases
    const uint64_t* src_start;   // n_reads
    uint64_t n_reads, n_bases;
};

// the 16 bases from base s of the old batch on, all of them inside it (s + 16 <= src_bases): funnel shift of the one or two words that
// hold them at the phase s & 15
DRPRG_HD inline uint32_t ss_fetch16(const CompactBatch& b, uint64_t s)
{
    const uint64_t w = s >> 4;
    const uint32_t phase = (uint32_t)(s & 15u);
    const uint64_t lo = b.src_words[w];
    const uint64_t hi = phase ? b.src_words[w + 1] : 0; // (bases s .. s + 15 end in word (s + 15) >> 4 = w + 1 when phase != 0)
    return (uint32_t)((hi << 32 | lo) >> (2 * phase));
}

// The word of bases [pw, pw + 16) of the new batch (pw < n_bases, pw a multiple of 16); r: a read at or before the one that holds pw,
// moved on to it.  Bits of bases at or beyond n_bases stay clear, as pack.cpp leaves them.  bad is set when a source position computed from
// the tables lies outside the old batch (the word's bases from there are left clear): tables that do not belong to the batch.
DRPRG_HD inline uint32_t ss_word(const CompactBatch& b, uint64_t pw, uint64_t& r, bool& bad)
{
    while (r + 1 < b.n_reads && b.new_offsets[r + 1] <= pw) ++r;
    const uint64_t start = b.new_offsets[r], end = b.new_offsets[r + 1];
    if (start <= pw && pw + 16 <= end) { // wholly inside one read: all but a few words of a batch of long reads
        const uint64_t s = b.src_start[r] + (pw - start);
        if (s + 16 <= b.src_bases && s + 16 > s) return ss_fetch16(b, s);
        bad = true;
        return 0;
    }
    // a word that crosses a read boundary (or the last word of the batch): stitched base by base
    uint64_t rr = r, st = start, e = end;
    const uint32_t valid = (uint32_t)(b.n_bases - pw < 16 ? b.n_bases - pw : 16);
    uint32_t x = 0;
    for (uint32_t i = 0; i < valid; ++i) {
        const uint64_t p = pw + i;
        while (rr + 1 < b.n_reads && e <= p) {
            ++rr;
            st = e;
            e = b.new_offsets[rr + 1];
        }
        if (p < st || p >= e) { // (the offsets do not cover p: not ascending, or they end before n_bases)
            bad = true;
            break;
        }
        const uint64_t s = b.src_start[rr] + (p - st);
        if (s >= b.src_bases) {
            bad = true;
            break;
        }
        x |= ((b.src_words[s >> 4] >> (2 * (uint32_t)(s & 15u))) & 3u) << (2 * i);
    }
    return x;
}

} // namespace dev
} // namespace drprg
