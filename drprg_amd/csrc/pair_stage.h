// pair_stage.h -- a judged pair staged in LDS, as pair_overlap.hip and pair_merge.hip both read it: a's read-aligned 16-base words with the
// mask of its known bases (one bit per base, at the even bit of its letter) and B = the reverse complement of b in the same form.  See
// pair_overlap.hip's header for the layout; one wave owns one set of rows.
#pragma once
#include "device_common.h"

namespace drprg {
namespace dev {

constexpr uint32_t PO_ROW = PO_MAX_LEN / 16 + 4; // words of one staged row: 64 of a mate, zero words around them
enum { PO_A = 0, PO_KA = 1, PO_B = 2, PO_KB = 3, PO_T = 4, PO_KT = 5, PO_ROWS = 6 };

// bit t of m (m < 2^16) -> bit 2t
__device__ inline uint32_t po_even(uint32_t m)
{
    m = (m | m << 8) & 0x00FF00FFu;
    m = (m | m << 4) & 0x0F0F0F0Fu;
    m = (m | m << 2) & 0x33333333u;
    m = (m | m << 1) & 0x55555555u;
    return m;
}

// bits [shift, shift + 32) of hi:lo (shift: 0..30): one v_alignbit_b32, where the 64-bit shift is two slower instructions
__device__ inline uint32_t po_funnel(uint32_t lo, uint32_t hi, uint32_t shift) { return __builtin_amdgcn_alignbit(hi, lo, shift); }

// word j of the read at l (16 j < l.len): its letters (those behind the read's end are not defined) and the mask of its known bases.  The
// second batch word is touched only when the bases reach into it, as dd_read_word does.
__device__ inline void po_read_word(const DedupLoc& l, uint32_t j, uint32_t& letters, uint32_t& known)
{
    const uint64_t at = l.start + 16ull * j;
    const uint32_t n = (uint32_t)(l.len - 16ull * j < 16 ? l.len - 16ull * j : 16);
    const uint64_t w = at >> 4;
    const uint32_t phase = (uint32_t)(at & 15u);
    const bool two = phase + n > 16;
    const uint32_t lo = l.words[w], hi = two ? l.words[w + 1] : 0u;
    const uint32_t mlo = l.bits ? l.bits[w] : 0u, mhi = l.bits && two ? l.bits[w + 1] : 0u;
    letters = po_funnel(lo, hi, 2 * phase);
    const uint32_t m = ((mhi << 16 | mlo) >> phase) & 0xFFFFu;
    known = po_even(~m & (n < 16 ? (1u << n) - 1u : 0xFFFFu));
}

// a wave's own LDS writes before its reads of what other lanes wrote: no other wave touches its rows
__device__ __forceinline__ void po_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The rows of one wave filled from the pair (a at `me`, b at `other`, both 1 .. PO_MAX_LEN bases; `staged` is uniform in the wave, and a
// wave that stages nothing only keeps step): a and b as they lie (b one word up: the windows of B reach 15 bases in front of it), then
// B[16 k + f] = complement(b[Lb - 1 - 16 k - f]): the window of b that ends at p = Lb - 1 - 16 k, backwards.
__device__ inline void po_stage_rows(uint32_t (*s)[PO_ROW], const DedupLoc& me, const DedupLoc& other, bool staged, uint32_t lane)
{
    const uint32_t La = staged ? (uint32_t)me.len : 0, Lb = staged ? (uint32_t)other.len : 0;
    const uint32_t nwa = (La + 15) >> 4, nwb = (Lb + 15) >> 4;
    if (staged) {
        for (uint32_t k = lane; k < PO_ROW; k += 64) {
            uint32_t v = 0, m = 0, bv = 0, bm = 0;
            if (k < nwa) po_read_word(me, k, v, m);
            if (k >= 1 && k - 1 < nwb) po_read_word(other, k - 1, bv, bm);
            s[PO_A][k] = v; s[PO_KA][k] = m;
            s[PO_T][k] = bv; s[PO_KT][k] = bm;
        }
    }
    po_wave_sync();
    if (staged) {
        for (uint32_t k = lane; k < PO_ROW; k += 64) {
            uint32_t v = 0, m = 0;
            if (k < nwb) {
                const uint32_t at = Lb - 16 * k; // (p - 15) + 16: where the window starts in the row (1 .. 1024)
                const uint32_t w = at >> 4, sh = 2 * (at & 15u);
                v = __brev(po_funnel(s[PO_T][w], s[PO_T][w + 1], sh));
                v = (((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1)) ^ 0xAAAAAAAAu; // letters: A 0, C 1, T 2, G 3 -- the complement flips bit 1
                m = __brev(po_funnel(s[PO_KT][w], s[PO_KT][w + 1], sh)) >> 1;
            }
            s[PO_B][k] = v; s[PO_KB][k] = m;
        }
    }
    po_wave_sync();
}

} // namespace dev
} // namespace drprg
