// mask_args.h -- --mask-qual as both executables take it (include/drprg_hip.h "base masking").
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>

namespace drprg {

// Q, an integer in 1..93, into q; what is wrong with `v` otherwise (a usage error: exit 2)
inline std::string parse_mask_qual(const char* v, uint32_t& q)
{
    char* end = nullptr;
    const unsigned long n = std::strtoul(v, &end, 10);
    if (end == v || *end || *v < '0' || *v > '9' || n < 1 || n > 93) return std::string("--mask-qual needs a whole Phred quality from 1 to 93, not ") + v;
    q = (uint32_t)n;
    return std::string();
}

} // namespace drprg
