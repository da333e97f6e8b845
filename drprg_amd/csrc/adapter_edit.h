// adapter_edit.h -- adapter trimming with indels and at the 5' end (include/drprg_hip.h "adapter trimming", the indel rule; DESIGN.md
// section 4) in integer arithmetic: Myers' bit-vector recurrence for the edit distance of an adapter against every stretch of a read that
// starts (3' side) or ends (5' side) at a base, and what one lane of adapter_edit_points_kernel (adapter_edit.hip) does with the stretch
// of the batch's concatenated bases it owns.  Host code as well (nothing here needs the HIP headers), so that a CPU build can walk the
// index arithmetic under a sanitizer with the buffers at their exact sizes (tools/adapter_edit_walk.cpp).
//
// One scan serves both sides.  The 3' side walks the bases right to left with the adapter reversed: behind base p the score is
// full(p) = min over q of ed(A, r[p..q)), the score of the step before it full(p + 1).  The 5' side walks left to right with the adapter
// as given: behind base q - 1 the score is g(q) = min over p of ed(A, r[p..q)).  The 5' side is the 3' side on the reversed read with the
// reversed adapter, so its AdapterSet holds the adapters letter-reversed and everything behind the direction of the walk is one code path:
// the pattern of the recurrence is the set's adapter read backwards, and the partial overlaps of clause (a) compare the window of the
// bases walked last, newest base in the lowest bits, against the set's letters as adapter_piece.h's ad_match does.
#pragma once
#include "adapter_piece.h"

namespace drprg {
namespace dev {

constexpr uint32_t AE_THREADS = 256;
constexpr uint32_t AE_STRETCH = 64;                      // starts (3') or ends (5') one lane owns
constexpr uint32_t AE_WAVE = 64 * AE_STRETCH;            // bases under one wave
constexpr uint32_t AE_TILE = AE_THREADS * AE_STRETCH;    // 16384 bases per workgroup, as adapter_points_kernel
constexpr uint32_t AE_SLOTS = 1024;                      // per-workgroup words in LDS: reads first .. first + 1023 of the tile
constexpr uint32_t AE_FLAG_INDELS = 1u;                  // drprg_hip_set_adapters2's flags

// the recurrence's match masks: eq[a][l] bit i is set iff letter len - 1 - i of adapter a of the set is l (A0 C1 T2 G3)
struct AdapterEq {
    uint64_t eq[AD_MAX_ADAPTERS][4];
};

DRPRG_HD inline uint32_t ae_limit(uint32_t c, uint32_t error_milli) { return c * error_milli / 1000u; }

// How far from the first base it owns a lane starts its walk with a fresh column.  A score of at most L(m) is reached inside m + L(m)
// bases, and clause (b) looks at the score of one base further: m + L(m) + 1 bases decide every verdict, one more is the margin the rule
// was checked with.  The longest adapter's figure serves every adapter of the set.
DRPRG_HD inline uint32_t ae_warmup(const AdapterSet& ad) { return ad.max_len + ae_limit(ad.max_len, ad.error_milli) + 2u; }

DRPRG_HD inline uint32_t ae_letter_of(const AdapterSet& ad, uint32_t a, uint32_t j) { return (uint32_t)((j < 32u ? ad.lo[a] >> (2u * j) : ad.hi[a] >> (2u * (j - 32u))) & 3u); }

inline AdapterEq ae_make_eq(const AdapterSet& ad)
{
    AdapterEq q {};
    for (uint32_t a = 0; a < ad.n && a < AD_MAX_ADAPTERS; ++a)
        for (uint32_t i = 0; i < ad.len[a] && i < AD_MAX_LEN; ++i) q.eq[a][ae_letter_of(ad, a, ad.len[a] - 1u - i)] |= 1ull << i;
    return q;
}

// the set with every adapter read backwards (the 5' side's)
inline AdapterSet ae_reversed(const AdapterSet& ad)
{
    AdapterSet r = ad;
    for (uint32_t a = 0; a < ad.n && a < AD_MAX_ADAPTERS; ++a) {
        r.lo[a] = r.hi[a] = 0;
        for (uint32_t j = 0; j < ad.len[a] && j < AD_MAX_LEN; ++j)
            (j < 32u ? r.lo[a] : r.hi[a]) |= (uint64_t)ae_letter_of(ad, a, ad.len[a] - 1u - j) << (2u * (j & 31u));
    }
    return r;
}

// The bases of a batch in either form (kernels.h AdapterPoints): text, or packed words with the bitmap of the bases that are not ACGT.
struct AeBases {
    const uint8_t* text;
    const uint32_t* words;
    const uint16_t* nbits;
    uint64_t n_bases;
    bool aligned; // text at a 16-byte aligned address: n_bases + 64 bytes are readable
};

// The 16 bases from base p on (p a multiple of 16) in adapter_piece.h's common form.  A word whose first base is not below n_bases is not
// loaded; text that is not aligned is read byte by byte and never behind n_bases.
DRPRG_HD inline void ae_load16(const AeBases& b, uint64_t p, uint32_t& code, uint32_t& nmask)
{
    code = 0;
    nmask = 0xFFFFu;
    if (p >= b.n_bases) return;
    if (b.words) {
        code = b.words[p >> 4]; // (p < n_bases: below ceil(n_bases / 16))
        nmask = b.nbits ? b.nbits[p >> 4] : 0u;
        return;
    }
    uint32_t w[4] = { 0, 0, 0, 0 };
    if (b.aligned) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(b.text + p);
        w[0] = t[0]; w[1] = t[1]; w[2] = t[2]; w[3] = t[3];
    } else {
        const uint32_t n = (uint32_t)(b.n_bases - p < 16 ? b.n_bases - p : 16);
        for (uint32_t j = 0; j < n; ++j) w[j >> 2] |= (uint32_t)b.text[p + j] << (8 * (j & 3));
    }
    ad_text16(w, code, nmask);
}

// the largest r in [0, n_reads) with offsets[r] <= p (offsets[0] <= p)
DRPRG_HD inline uint64_t ae_read_holding(const uint64_t* offsets, uint64_t n_reads, uint64_t p)
{
    uint64_t lo = 0, hi = n_reads - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One lane's walk.  It owns the bases [a, b) of the batch's concatenated bases (a < b <= n_bases, n_reads >= 1) as starts (DIR < 0, the 3'
// side: right to left) or as the last base in front of an end (DIR > 0, the 5' side: left to right), begins at most ae_warmup bases
// outside them with a fresh column D[i] = i, takes a fresh column again at the first base of every range it walks into, and steps over
// bases outside every range.  Word: uint32_t when every adapter has at most 32 letters, uint64_t otherwise.  emit(read, v) once for
// every read that has a match among the owned bases: DIR < 0: v = the smallest matching start here, DIR > 0: v = the largest matching
// end here, both counted from the range's first base.  A base belongs to read i iff it lies in [offsets[i] + begin[i], offsets[i] +
// end[i]).  Reads whose offsets do not ascend inside n_bases, or whose range does not lie inside them, have no range here (the apply
// kernel refuses the batch); nothing is indexed by what they hold, and no base at or behind n_bases is looked at.
template <int DIR, typename Word, typename Emit>
DRPRG_HD inline void ae_scan(const AeBases& bs, const uint64_t* offsets, const uint64_t* begin, const uint64_t* end, uint64_t n_reads, uint64_t a, uint64_t b,
    const AdapterSet& ad, const AdapterEq& q, Emit&& emit)
{
    constexpr bool wide = sizeof(Word) > 4;
    const uint32_t W = ae_warmup(ad);
    uint64_t pos;
    if (DIR < 0) pos = bs.n_bases - b >= W ? b - 1 + W : bs.n_bases - 1;
    else pos = a >= W ? a - W : 0;
    uint64_t steps = DIR < 0 ? pos - a + 1 : b - pos;

    Word pv[AD_MAX_ADAPTERS], mv[AD_MAX_ADAPTERS];
    uint32_t sc[AD_MAX_ADAPTERS];
    auto fresh = [&]() {
#pragma unroll
        for (uint32_t k = 0; k < AD_MAX_ADAPTERS; ++k) {
            pv[k] = (Word)~(Word)0;
            mv[k] = 0;
            sc[k] = ad.len[k];
        }
    };
    fresh();
    uint64_t lo = 0, hi = 0, nlo = 0, nhi = 0; // the bases walked last, newest lowest: letters, and the bits of those that are not ACGT

    uint64_t r = ae_read_holding(offsets, n_reads, pos);
    uint64_t S0 = 0, E0 = ~0ull, X = 0, Y = 0; // read r's bases and its range, absolute ([0, 0): none)
    auto enter = [&]() {
        const uint64_t s = offsets[r], e = r + 1 < n_reads ? offsets[r + 1] : bs.n_bases;
        S0 = 0;
        E0 = ~0ull;
        X = Y = 0;
        if (s <= pos && pos < e && e <= bs.n_bases && e - s < AD_MAX_READ) {
            S0 = s;
            E0 = e;
            const uint64_t x = begin[r], t = end[r];
            if (x < t && t <= e - s) {
                X = s + x;
                Y = s + t;
            }
        }
    };
    enter();
    uint32_t best = 0;
    bool has = false;
    uint32_t code = 0, nm = 0xFFFFu;
    bool loaded = false;
    for (; steps; --steps, pos += (uint64_t)(int64_t)DIR) {
        if (!loaded || (pos & 15u) == (DIR < 0 ? 15u : 0u)) {
            ae_load16(bs, pos & ~15ull, code, nm);
            loaded = true;
        }
        if (DIR < 0 ? pos < S0 : pos >= E0) { // the next read that has bases
            if (has) emit(r, best);
            has = false;
            if (DIR < 0) while (r > 0 && offsets[r] > pos) --r;
            else while (r + 1 < n_reads && offsets[r + 1] <= pos) ++r;
            enter();
        }
        if (pos < X || pos >= Y) continue;
        if (pos == (DIR < 0 ? Y - 1 : X)) fresh();
        const uint32_t sh = (uint32_t)(pos & 15u);
        const uint32_t base = (code >> (2u * sh)) & 3u;
        const bool isn = (nm >> sh) & 1u;
        if (wide) {
            hi = (hi << 2) | (lo >> 62);
            nhi = (nhi << 2) | (nlo >> 62);
        }
        lo = (lo << 2) | base;
        nlo = (nlo << 2) | (isn ? 1u : 0u);
        const bool own = DIR < 0 ? pos < b : pos >= a;
        const uint64_t c = DIR < 0 ? Y - pos : pos + 1 - X; // bases between here and where the range begins for this walk
        bool match = false;
#pragma unroll
        for (uint32_t k = 0; k < AD_MAX_ADAPTERS; ++k) {
            if (k >= ad.n) break; // (uniform)
            const uint32_t m = ad.len[k];
            const Word e0 = (Word)q.eq[k][0], e1 = (Word)q.eq[k][1], e2 = (Word)q.eq[k][2], e3 = (Word)q.eq[k][3];
            const Word eq = isn ? (Word)0 : (base == 0 ? e0 : base == 1 ? e1 : base == 2 ? e2 : e3);
            const Word top = (Word)1 << (m - 1u);
            const uint32_t before = sc[k];
            const Word xv = eq | mv[k];
            const Word xh = (Word)((((eq & pv[k]) + pv[k]) ^ pv[k]) | eq);
            Word ph = mv[k] | (Word)~(xh | pv[k]);
            Word mh = pv[k] & xh;
            sc[k] += (ph & top) ? 1u : 0u;
            sc[k] -= (mh & top) ? 1u : 0u;
            ph <<= 1;
            mh <<= 1;
            pv[k] = mh | (Word)~(xv | ph);
            mv[k] = ph & xv;
            if (!own) continue;
            if (sc[k] <= ae_limit(m, ad.error_milli) && before >= sc[k]) match = true; // clause (b)
            if (c < m && c >= ad.min_overlap) {                                        // clause (a): the adapter runs off the range's end
                const uint32_t cc = (uint32_t)c;
                const uint64_t x = lo ^ ad.lo[k];
                uint32_t miss = ad_popc64(((x | (x >> 1)) | nlo) & ad_pairs(cc < 32u ? cc : 32u));
                if (wide && cc > 32u) {
                    const uint64_t y = hi ^ ad.hi[k];
                    miss += ad_popc64(((y | (y >> 1)) | nhi) & ad_pairs(cc - 32u));
                }
                if (miss <= ae_limit(cc, ad.error_milli)) match = true;
            }
        }
        if (match) { // (the walk goes towards smaller starts, or larger ends: the last match is the one to keep)
            best = (uint32_t)(DIR < 0 ? pos - X : pos + 1 - X);
            has = true;
        }
    }
    if (has) emit(r, best);
}

} // namespace dev
} // namespace drprg
