// read_stats_words.h -- the layout of one read-statistics snapshot (include/drprg_hip.h "read statistics"): a flat
// array of RS_WORDS u64 words, shared by the kernels (read_stats.hip), the C entries (capi_prep.cpp), the JSON writer (qc_json.cpp) and --
// through drprg_hip_read_stats_layout -- the Python binding.  Host code as well: nothing here needs the HIP headers.
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

constexpr uint32_t RS_LEN_BINS = 2432; // exact below 1024, 64 per octave from 2^10 to 2^32
constexpr uint32_t RS_CYCLES = 512;    // cycle bin RS_CYCLES takes every position at or beyond it
constexpr uint32_t RS_COLS = 5;        // A, C, G, T, U
constexpr uint32_t RS_QUALS = 94;      // Phred 0 .. 93
constexpr uint32_t RS_GC_BINS = 101;   // floor(100 (G + C) / V)
enum : uint32_t {
    RS_READS = 0, RS_BASES = 1, RS_MIN_LEN = 2 /* 0 without a read */, RS_MAX_LEN = 3,
    RS_LEN_READS = 4,                                        // [RS_LEN_BINS]
    RS_LEN_BASES = RS_LEN_READS + RS_LEN_BINS,               // [RS_LEN_BINS]: the exact sum of the lengths of the bin's reads
    RS_CYC_BASE = RS_LEN_BASES + RS_LEN_BINS,                // [RS_CYCLES + 1][RS_COLS]
    RS_CYC_QSUM = RS_CYC_BASE + (RS_CYCLES + 1) * RS_COLS,   // [RS_CYCLES + 1]: the sum of the Phred values
    RS_QUAL_HIST = RS_CYC_QSUM + RS_CYCLES + 1,              // [RS_QUALS]: bases per Phred value
    RS_READQ_HIST = RS_QUAL_HIST + RS_QUALS,                 // [RS_QUALS]: reads per quality of their mean error probability
    RS_GC_HIST = RS_READQ_HIST + RS_QUALS,                   // [RS_GC_BINS]
    RS_WORDS = RS_GC_HIST + RS_GC_BINS,
    // behind the snapshot in a device accumulator only: what the kernels refuse
    RS_DEV_BAD_AT = RS_WORDS /* first bad quality byte + 1 of a block, or ~0: none */, RS_DEV_OFFSETS = RS_WORDS + 1, RS_DEV_WORDS = RS_WORDS + 2
};

// the length histogram's bin of a read of L bases (L < 2^32), and the smallest length of a bin
DRPRG_HD inline uint32_t rs_len_bin(uint64_t L)
{
    if (L < 1024) return (uint32_t)L;
    const uint32_t e = 63u - (uint32_t)__builtin_clzll(L); // floor(log2 L), 10 .. 31
    return 1024u + (e - 10u) * 64u + (uint32_t)((L >> (e - 6u)) & 63u);
}
DRPRG_HD inline uint64_t rs_bin_low(uint32_t bin)
{
    if (bin < 1024) return bin;
    const uint32_t e = 10u + (bin - 1024u) / 64u, m = (bin - 1024u) % 64u;
    return (uint64_t)(64u + m) << (e - 6u);
}

} // namespace dev
} // namespace drprg
