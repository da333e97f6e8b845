// load16.h -- 16 bases in adapter_points_kernel's common form (adapter_piece.h) from either input form, for adapter_trim.hip,
// decoy_screen.hip, poly_tail.hip and read_complexity.hip: a 32-bit word of 2-bit letters, first base in the LOWEST bits, A0 C1 T2 G3, and a 16-bit mask of the bases that are
// not ACGT -- the rules' one unknown base U.
#pragma once
#include "device_common.h"

namespace drprg {
namespace dev {

// The 16 bases from base p on (p a multiple of 16) in the common form.  A word
// whose first base is not below n_bases is not loaded: it reads as sixteen unknown bases.  Text at an address that is not 16-byte aligned is
// read byte by byte and never behind n_bases; aligned text has its 64 bytes of padding, so the 16 bytes at p < n_bases are readable.
__device__ inline void load16_common(const uint8_t* __restrict__ text, const uint32_t* __restrict__ words, const uint16_t* __restrict__ nbits, uint64_t n_bases,
    bool aligned, uint64_t p, uint32_t& code, uint32_t& nmask)
{
    code = 0;
    nmask = 0xFFFFu;
    if (p >= n_bases) return;
    if (words) {
        code = words[p >> 4]; // (p < n_bases: below ceil(n_bases / 16))
        nmask = nbits ? nbits[p >> 4] : 0u;
        return;
    }
    uint32_t w[4] = { 0, 0, 0, 0 };
    if (aligned) {
        const uint4 v = load_once_16(text + p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        const uint32_t n = (uint32_t)(n_bases - p < 16 ? n_bases - p : 16);
        for (uint32_t j = 0; j < n; ++j) w[j >> 2] |= (uint32_t)text[p + j] << (8 * (j & 3));
    }
    ad_text16(w, code, nmask);
}

} // namespace dev
} // namespace drprg
