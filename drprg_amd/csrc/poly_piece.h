// poly_piece.h -- the integer arithmetic of poly-tail trimming and of the low-complexity filter (the rules: include/drprg_hip.h "poly
// tails" and "read complexity"), as poly_tail.hip, read_complexity.hip and read_flags_kernel use it.  Host code as
// well (nothing here needs the HIP headers).
#pragma once
#include "adapter_piece.h"

namespace drprg {
namespace dev {

constexpr uint32_t PT_MIN_LEN_LO = 2, PT_MIN_LEN_HI = 255, PT_DEFAULT_MIN_LEN = 10;
constexpr uint32_t PT_MAX_MISS = 5;         // a suffix holds at most min(floor(n / 8), 5) bases that are not X
constexpr uint64_t CX_MAX_READ = 1ull << 32; // D is a 32-bit word per read

// bases not X a suffix of n bases may hold
DRPRG_HD inline uint32_t pt_allowance(uint32_t n) { return (n >> 3) < PT_MAX_MISS ? (n >> 3) : PT_MAX_MISS; }

// the read-complexity verdict: dropped iff L >= 2 and 100 D < P (L - 1)
DRPRG_HD inline bool cx_drops(uint64_t D, uint64_t len, uint32_t percent) { return len >= 2 && 100ull * D < (uint64_t)percent * (len - 1); }

} // namespace dev
} // namespace drprg
