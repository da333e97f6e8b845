// adapter_piece.h -- adapter trimming (include/drprg_hip.h "adapter trimming") in integer arithmetic: the settings as
// the kernels hold them, the two loads' common form, and what adapter_points_kernel (adapter_trim.hip) does with the 16 starts one lane
// takes per round.  Host code as well (nothing here needs the HIP headers), so that a CPU build can walk the index arithmetic under a
// sanitizer with the buffers at their exact sizes (tools/adapter_walk.cpp).
//
// One form behind either load: 16 bases are a 32-bit word of 2-bit letters, first base in the LOWEST bits, A0 C1 T2 G3 -- (byte >> 1) & 3
// of the text, in either case, and the packed batch's own word -- and a 16-bit mask of the bases that are not ACGT (bit i = base i: what
// launch_mark_npos makes of a packed block's position list).  An adapter is held the same way in two 64-bit words.
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

constexpr uint32_t AD_MAX_ADAPTERS = 4;
constexpr uint32_t AD_MAX_LEN = 64;
constexpr uint32_t AD_MAX_ERROR_MILLI = 500;
constexpr uint32_t AD_DEFAULT_ERROR_MILLI = 100;
constexpr uint32_t AD_DEFAULT_MIN_OVERLAP = 3;
constexpr uint32_t AD_LANE_STARTS = 16;                                         // starts per lane and round: one word
constexpr uint32_t AD_LANE_WORDS = (AD_LANE_STARTS + AD_MAX_LEN + 15) / 16;     // 5: the lane's own word and the up to 63 bases behind it
constexpr uint32_t AD_NONE = 0xFFFFFFFFu;                                       // "no match" in the array of smallest starts
constexpr uint64_t AD_MAX_READ = 1ull << 31;                                    // starts are 32-bit words (as RT_MAX_READ)

struct AdapterSet { // n == 0: no adapter trimming
    uint64_t lo[AD_MAX_ADAPTERS], hi[AD_MAX_ADAPTERS]; // letters 0..31 and 32..63, 2 bits each, first letter lowest; zero behind the last
    uint32_t len[AD_MAX_ADAPTERS];
    uint32_t n, error_milli, min_overlap, max_len;
};

// letter code of an adapter letter, or 4
DRPRG_HD inline uint32_t ad_letter(uint8_t c)
{
    const uint32_t u = c & 0xDFu;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T' ? (u >> 1) & 3u : 4u;
}

// 16 text bytes (four little-endian words) -> the common form.  A byte is a base iff, upper-cased, it is the letter its code stands for.
DRPRG_HD inline void ad_text16(const uint32_t (&w)[4], uint32_t& code, uint32_t& nmask)
{
    code = 0;
    nmask = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t u = w[q] & 0xDFDFDFDFu, sel = (u >> 1) & 0x03030303u;
#if defined(__HIP_DEVICE_COMPILE__)
        code |= (__builtin_amdgcn_udot4(sel, 0x40100401u, 0u, false) & 0xFFu) << (8 * q); // byte weights 1, 4, 16, 64
        const uint32_t diff = u ^ __builtin_amdgcn_perm(0u, 0x47544341u, sel);            // "ACTG"[code]
#else
        uint32_t expect = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t l = (sel >> (8 * b)) & 3u;
            code |= l << (8 * q + 2 * b);
            expect |= ((0x47544341u >> (8 * l)) & 0xFFu) << (8 * b);
        }
        const uint32_t diff = u ^ expect;
#endif
        if (diff) { // rare: bit 7 of every non-zero byte, gathered into four bits
            const uint32_t bad = (((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff) & 0x80808080u;
            nmask |= ((((bad >> 7) * 0x01020408u) >> 24) & 0xFu) << (4 * q);
        }
    }
}

// bit i of a 16-bit mask -> bit 2 i
DRPRG_HD inline uint32_t ad_spread16(uint32_t m)
{
    if (!m) return 0;
    m &= 0xFFFFu;
    m = (m | (m << 8)) & 0x00FF00FFu;
    m = (m | (m << 4)) & 0x0F0F0F0Fu;
    m = (m | (m << 2)) & 0x33333333u;
    m = (m | (m << 1)) & 0x55555555u;
    return m;
}

// the low c letters (c <= 32) of a 64-bit word of bit pairs, as a mask over their low bits
DRPRG_HD inline uint64_t ad_pairs(uint32_t c) { return c >= 32u ? 0x5555555555555555ull : ((1ull << (2u * c)) - 1ull) & 0x5555555555555555ull; }

// A lane's window: the 80 bases from the start it stands at on, as five words of letters (c) and five of non-ACGT bits spread to the
// pairs' low bits (n; any_n: one of them is set, which is rare).  ad_window makes it of the five loaded words; ad_step moves it on by one
// base, five funnel shifts by a constant.
struct AdWindow {
    uint32_t c[AD_LANE_WORDS], n[AD_LANE_WORDS];
    bool any_n;
};
DRPRG_HD inline AdWindow ad_window(const uint32_t (&c)[AD_LANE_WORDS], const uint32_t (&n)[AD_LANE_WORDS])
{
    AdWindow w;
    uint32_t any = 0;
#pragma unroll
    for (uint32_t k = 0; k < AD_LANE_WORDS; ++k) {
        w.c[k] = c[k];
        w.n[k] = ad_spread16(n[k]);
        any |= w.n[k];
    }
    w.any_n = any != 0;
    return w;
}
DRPRG_HD inline void ad_step(AdWindow& w)
{
#pragma unroll
    for (uint32_t k = 0; k + 1 < AD_LANE_WORDS; ++k) w.c[k] = (w.c[k] >> 2) | (w.c[k + 1] << 30);
    w.c[AD_LANE_WORDS - 1] >>= 2;
    if (w.any_n) {
#pragma unroll
        for (uint32_t k = 0; k + 1 < AD_LANE_WORDS; ++k) w.n[k] = (w.n[k] >> 2) | (w.n[k + 1] << 30);
        w.n[AD_LANE_WORDS - 1] >>= 2;
    }
}

DRPRG_HD inline uint32_t ad_popc64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }

// Is the start the window stands at a match of one of the adapters, when `avail` bases (>= 1) lie between it and the end of its read's
// range?  c = min(m, avail); a match iff c >= O and at most floor(c * e / 1000) of the first c letters differ.  Bases behind `avail` are
// masked off before they are counted: what lies there (the next read, the padding, a word that was never loaded) does not matter.
// Nearly every start has every adapter's full length in front of it: there c, the masks and the limit are the same for every lane and
// stay in scalar registers (the first loop); the few starts near a range's end take the second.
DRPRG_HD inline bool ad_match(const AdWindow& w, uint64_t avail, const AdapterSet& ad)
{
    const bool wide = ad.max_len > 32u; // (uniform)
    const uint64_t lo = (uint64_t)w.c[0] | ((uint64_t)w.c[1] << 32), hi = wide ? (uint64_t)w.c[2] | ((uint64_t)w.c[3] << 32) : 0ull;
    const uint64_t nlo = w.any_n ? (uint64_t)w.n[0] | ((uint64_t)w.n[1] << 32) : 0ull, nhi = wide && w.any_n ? (uint64_t)w.n[2] | ((uint64_t)w.n[3] << 32) : 0ull;
    if (avail >= ad.max_len) {
        for (uint32_t a = 0; a < ad.n && a < AD_MAX_ADAPTERS; ++a) {
            const uint32_t m = ad.len[a];
            if (m < ad.min_overlap || m == 0) continue;
            const uint64_t x = lo ^ ad.lo[a];
            uint32_t miss = ad_popc64(((x | (x >> 1)) | nlo) & ad_pairs(m));
            if (m > 32u) {
                const uint64_t y = hi ^ ad.hi[a];
                miss += ad_popc64(((y | (y >> 1)) | nhi) & ad_pairs(m - 32u));
            }
            if (miss <= m * ad.error_milli / 1000u) return true;
        }
        return false;
    }
    for (uint32_t a = 0; a < ad.n && a < AD_MAX_ADAPTERS; ++a) {
        const uint32_t m = ad.len[a];
        const uint32_t c = avail < m ? (uint32_t)avail : m;
        if (c < ad.min_overlap || c == 0) continue;
        const uint64_t x = lo ^ ad.lo[a];
        uint32_t miss = ad_popc64(((x | (x >> 1)) | nlo) & ad_pairs(c));
        if (c > 32u) {
            const uint64_t y = hi ^ ad.hi[a];
            miss += ad_popc64(((y | (y >> 1)) | nhi) & ad_pairs(c - 32u));
        }
        if (miss <= c * ad.error_milli / 1000u) return true;
    }
    return false;
}

// The starts [p, p + n) of a batch's concatenated bases (1 <= n <= 16, p + n <= n_bases) and the lane's window from base p on.  r: a read
// at or before the one that holds base p; moved on to the read that holds the last of the starts, and never behind r_last (< n_reads: a
// read at or behind the one that holds the last start -- the walk over reads is bounded by it whatever the offsets hold).  Calls emit(read, cut) for every read
// that has a matching start here, in ascending order: cut = the smallest such start counted from the read's range's first base.  A start
// belongs to read i iff it lies in [offsets[i] + begin[i], offsets[i] + end[i]).  Reads whose offsets do not ascend inside n_bases, or
// whose range does not lie inside them, are stepped over (adapter_apply_kernel refuses the batch); nothing is indexed by what they hold.
// The starts are taken in order, the window moving on by one base each, and the read under a start is followed as they go.
template <typename Emit>
DRPRG_HD inline void ad_piece(const uint64_t* offsets, const uint64_t* begin, const uint64_t* end, uint64_t n_reads, uint64_t n_bases, uint64_t p, uint32_t n,
    AdWindow w, const AdapterSet& ad, uint64_t& r, uint64_t r_last, Emit&& emit)
{
    if (r_last >= n_reads) r_last = n_reads - 1;
    while (r < r_last && offsets[r + 1] <= p) ++r;
    uint64_t x = 0, y = 0, next = 0; // the range of read r, [0, 0) when it has none; where the read behind it starts (~0: there is none)
    bool found = false;
    auto enter = [&]() {
        const uint64_t s = offsets[r], e = r + 1 < n_reads ? offsets[r + 1] : n_bases;
        next = r + 1 < n_reads ? e : ~0ull;
        x = y = 0;
        found = false;
        if (s <= e && e <= n_bases && e - s < AD_MAX_READ) {
            const uint64_t b = begin[r], t = end[r];
            if (b < t && t <= e - s) {
                x = s + b;
                y = s + t;
            }
        }
    };
    enter();
    if (n == AD_LANE_STARTS && x <= p && p + (AD_LANE_STARTS - 1) + ad.max_len <= y) {
        // All sixteen starts lie in this read's range with every adapter's full length in front of them: nearly every piece.  A match of
        // adapter a has at most its limit of mismatches among its first 16 letters too, so a start is looked at in full only where one
        // 32-bit word passes that test -- next to never on bases that hold no adapter.  Constant shifts, scalar masks and limits.
        uint32_t maybe = 0;
#pragma unroll
        for (uint32_t j = 0; j < AD_LANE_STARTS; ++j) {
            const uint32_t w0 = j ? (w.c[0] >> (2u * j)) | (w.c[1] << (32u - 2u * j)) : w.c[0];
            const uint32_t n0 = !w.any_n ? 0u : (j ? (w.n[0] >> (2u * j)) | (w.n[1] << (32u - 2u * j)) : w.n[0]);
            for (uint32_t a = 0; a < ad.n && a < AD_MAX_ADAPTERS; ++a) {
                const uint32_t m = ad.len[a], d = w0 ^ (uint32_t)ad.lo[a];
                const uint32_t miss = (uint32_t)__builtin_popcount(((d | (d >> 1)) | n0) & (uint32_t)ad_pairs(m < 16u ? m : 16u));
                maybe |= (miss <= m * ad.error_milli / 1000u ? 1u : 0u) << j;
            }
        }
        while (maybe) { // (rare) ascending: the first start that matches in full is the read's smallest here
            const uint32_t j = (uint32_t)__builtin_ctz(maybe);
            maybe &= maybe - 1u;
            AdWindow v = w;
            for (uint32_t k = 0; k < j; ++k) ad_step(v);
            if (ad_match(v, y - (p + j), ad)) {
                emit(r, (uint32_t)(p + j - x));
                break;
            }
        }
        return;
    }
    for (uint32_t j = 0; j < AD_LANE_STARTS; ++j) {
        if (j >= n) break;
        const uint64_t at = p + j;
        while (next <= at && r < r_last) { // (reads of no bases are stepped over)
            ++r;
            enter();
        }
        if (!found && at >= x && at < y && ad_match(w, y - at, ad)) {
            emit(r, (uint32_t)(at - x));
            found = true;
        }
        ad_step(w);
    }
}

} // namespace dev
} // namespace drprg
