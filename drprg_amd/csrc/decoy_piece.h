// decoy_piece.h -- the decoy screen (include/drprg_hip.h "decoy screen") in integer arithmetic: the settings as the
// kernels hold them, a k-mer's canonical form, the table's slot and the verdict.  Host code as well (nothing here needs the HIP headers):
// drprg_hip_decoy_lookup canonicalises on the host, and the verdict is stated once for the two kernels that apply it.
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

constexpr uint32_t DC_MIN_K = 9, DC_MAX_K = 31, DC_DEFAULT_K = 31;
constexpr uint32_t DC_MAX_FILES = 8;
constexpr uint32_t DC_DEFAULT_FRAC_MILLI = 500, DC_DEFAULT_MIN_KMERS = 1;
constexpr uint64_t DC_MAX_WINDOWS = 0x7FFFFFFFull;
constexpr uint64_t DC_MIN_SLOTS = 8;
constexpr uint64_t DC_EMPTY = ~0ull; // never a k-mer: K <= 31 keeps every code below 2^62

// What the kernels are told of a decoy set: k == 0: none.  table: n_slots (a power of two) 64-bit slots in device memory, DC_EMPTY or a
// canonical k-mer; linear probing from dc_slot, wrapping; at most half of the slots are taken.
struct DecoySet {
    const unsigned long long* table;
    uint64_t n_slots;
    uint32_t k, frac_milli, min_kmers;
};

// the reverse complement of a k-mer code (A 0, C 1, G 2, T 3, first base in the high bits)
DRPRG_HD inline uint64_t dc_revcomp(uint64_t x, uint32_t k)
{
    x = ~x; // the complement of a letter is 3 - letter
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    x = (x >> 32) | (x << 32);
    return x >> (64u - 2u * k);
}

DRPRG_HD inline uint64_t dc_mask(uint32_t k) { return (1ull << (2u * k)) - 1ull; }

DRPRG_HD inline uint64_t dc_canonical(uint64_t x, uint32_t k)
{
    x &= dc_mask(k);
    const uint64_t r = dc_revcomp(x, k);
    return r < x ? r : x;
}

// where a canonical k-mer's probe sequence starts: hash64 (the minimizer hash, HashTraits<uint64_t>::mix at full width) folded once
DRPRG_HD inline uint64_t dc_slot(uint64_t key, uint64_t slot_mask)
{
    key = ~key + (key << 21);
    key = key ^ (key >> 24);
    key = key + (key << 3) + (key << 8);
    key = key ^ (key >> 14);
    key = key + (key << 2) + (key << 4);
    key = key ^ (key >> 28);
    key = key + (key << 31);
    return (key ^ (key >> 32)) & slot_mask;
}

// the verdict: a read with V valid windows, H of them in the set, is dropped as DECOY iff H >= M and 1000 * H >= f * V (V, H < 2^32)
DRPRG_HD inline bool dc_drops(uint32_t V, uint32_t H, uint32_t frac_milli, uint32_t min_kmers)
{
    return H >= min_kmers && 1000ull * H >= (uint64_t)frac_milli * V;
}

} // namespace dev
} // namespace drprg
