// poly_tail.hip -- poly-tail trimming (drprg_hip_set_poly_trim; the rule: include/drprg_hip.h "poly tails"): every
// read loses its longest suffix of n >= M bases that begins with a letter X of the set and holds at most min(floor(n / 8), 5) bases that
// are not X.  Launched by launch_read_trim (read_trim.hip) behind whichever adapter rule ran, on the ranges it left, in front of the scan
// of the new lengths; the compaction that follows is the trim stage's own.
//
// poly_tail_kernel walks every read's range from its END, one thread per read, 16 bases at a time in adapter_points_kernel's common form
// (load16_common, load16.h: a packed block's word and its bitmap piece, or ad_text16 of one 16-byte load).  Per word and letter: an XOR
// against the letter in every pair, a fold of the two bit planes, an OR of the bases that are not ACGT, a mask to the bases inside the range
// and a popcount.  The number of bases that are not X only grows with n, so a letter is done at its sixth such base: a read without a tail
// costs one or two words whatever its length.  A word that is all X is settled by its far end alone (the allowance only grows), any other
// word base by base.
//
// A thread takes at most PT_SOLO_WORDS words this way.  Reads still under way then -- tails beyond 64 bases -- are taken one after the
// other by the whole wave: lane k loads the k-th word from where the scan stands, an inclusive scan by shuffles gives every lane the bases
// not X behind its word, every lane settles its own word and a maximum over the wave is the longest suffix so far: 1024 bases per step,
// until every letter is done or the range's first base is reached.  So the bound per read is its tail's length plus, at most, the six
// bases that end every letter's scan, rounded up to 16-base words under 64 bases and to 64 words beyond.
//
// "Longest" is a maximum over independent tests: the result does not depend on who took which word.  The thread that owns the read
// applies the cut -- end[i] -= cut, klen[i] -- and counts.  Every index that comes from device data is bounded before it is used: a range
// that does not lie inside its read, or a read that does not lie below n_bases, sets work[RT_OFFSETS] and is left alone.
#include "load16.h"

namespace drprg {
namespace dev {

constexpr int PT_THREADS = 256;
constexpr uint32_t PT_SOLO_WORDS = 4;

// the pairs' low bits of the bases lo .. hi - 1 of a word (0 <= lo < hi <= 16)
__device__ inline uint32_t pt_valid(uint32_t lo, uint32_t hi)
{
    const uint32_t up = hi >= 16u ? 0xFFFFFFFFu : (1u << (2u * hi)) - 1u;
    return up & ~((1u << (2u * lo)) - 1u) & 0x55555555u;
}

// bit 2 j: base j of the word is inside the range and is not X (x: the letter's code; nspread: the unknown bases, ad_spread16)
__device__ inline uint32_t pt_miss(uint32_t code, uint32_t nspread, uint32_t x, uint32_t valid)
{
    const uint32_t d = code ^ (x * 0x55555555u);
    return ((d | (d >> 1)) | nspread) & valid;
}

// The longest qualifying suffix that begins at one of the word's bases lo .. hi - 1, or 0: n bases lie behind the word, mm of them not X.
__device__ inline uint32_t pt_scan(uint32_t miss, uint32_t lo, uint32_t hi, uint32_t n, uint32_t mm, uint32_t min_len)
{
    if (!miss) { // all X: mm stays and the allowance only grows, so the word's first base decides
        const uint32_t nn = n + (hi - lo);
        return nn >= min_len && mm <= pt_allowance(nn) ? nn : 0u;
    }
    uint32_t best = 0;
    for (uint32_t j = hi; j > lo && mm <= PT_MAX_MISS; --j) {
        const uint32_t bit = (miss >> (2u * (j - 1u))) & 1u;
        mm += bit;
        ++n;
        if (!bit && n >= min_len && mm <= pt_allowance(n)) best = n;
    }
    return best;
}

// letters: bit x set for the letter with code x (A0 C1 T2 G3).  end[i] -= the cut; klen[i] (may be null) the new length; the counts ADDED
// to work[RT_PT_*].
__global__ __launch_bounds__(PT_THREADS) void poly_tail_kernel(AdapterPoints a, uint32_t letters, uint32_t min_len, uint64_t* __restrict__ end,
    uint64_t* __restrict__ klen, unsigned long long* __restrict__ work)
{
    __shared__ unsigned long long s_n[4];
    if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    const bool aligned = (reinterpret_cast<uintptr_t>(a.text) & 15u) == 0;
    if (i == a.n_reads && a.offsets[i] != a.n_bases) work[RT_OFFSETS] = 1;
    // the read's range in the block: [lo_at, pos)
    uint64_t lo_at = 0, pos = 0, y = 0;
    bool ok = false;
    if (i < a.n_reads) {
        const uint64_t s = a.offsets[i], e = a.offsets[i + 1], x = a.begin[i];
        y = end[i];
        if (e < s || e > a.n_bases || e - s >= AD_MAX_READ || x > y || y > e - s) work[RT_OFFSETS] = 1;
        else {
            ok = true;
            lo_at = s + x;
            pos = s + y;
        }
    }
    const uint32_t L = (uint32_t)(pos - lo_at);
    uint32_t n = 0, best = 0, alive = ok && L >= min_len ? letters & 0xFu : 0u, mmp = 0; // mmp: the bases not X behind, 8 bits per letter
    for (uint32_t w = 0; w < PT_SOLO_WORDS && alive && pos > lo_at; ++w) {
        const uint64_t p0 = (pos - 1) & ~15ull; // (below pos <= n_bases)
        uint32_t code, nm;
        load16_common(a.text, a.words, a.nbits, a.n_bases, aligned, p0, code, nm);
        const uint32_t lo = lo_at > p0 ? (uint32_t)(lo_at - p0) : 0u, hi = (uint32_t)(pos - p0), valid = pt_valid(lo, hi), nsp = ad_spread16(nm);
#pragma unroll
        for (uint32_t x = 0; x < 4; ++x) {
            if (!((alive >> x) & 1u)) continue;
            const uint32_t miss = pt_miss(code, nsp, x, valid), mm = (mmp >> (8u * x)) & 0xFFu;
            const uint32_t c = pt_scan(miss, lo, hi, n, mm, min_len);
            best = c > best ? c : best;
            const uint32_t now = mm + __popc(miss);
            if (now > PT_MAX_MISS) alive &= ~(1u << x);
            else mmp = (mmp & ~(0xFFu << (8u * x))) | (now << (8u * x));
        }
        n += hi - lo;
        pos = p0 + lo;
    }
    // the reads still under way, one after the other, by the whole wave (every lane of the wave is here: nothing above returns)
    uint64_t todo = __ballot(alive != 0 && pos > lo_at);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t ra = __shfl(lo_at, src);
        uint64_t rpos = __shfl(pos, src);
        uint32_t rn = __shfl(n, src), ralive = __shfl(alive, src), rmm = __shfl(mmp, src), rbest = 0;
        while (ralive && rpos > ra) { // (uniform)
            const uint64_t qtop = (rpos - 1) >> 4;
            const bool has = qtop >= (uint64_t)lane && ((qtop - lane) << 4) + 16 > ra; // lane k: the k-th word down from the scan's place
            const uint64_t p0 = has ? (qtop - lane) << 4 : 0;
            uint32_t code = 0, nm = 0, lo = 0, hi = 0, valid = 0, behind = 0;
            if (has) {
                load16_common(a.text, a.words, a.nbits, a.n_bases, aligned, p0, code, nm); // (p0 < rpos <= n_bases)
                lo = ra > p0 ? (uint32_t)(ra - p0) : 0u;
                hi = lane == 0 ? (uint32_t)(rpos - p0) : 16u;
                valid = pt_valid(lo, hi);
                behind = rn + (lane ? (uint32_t)(rpos - (p0 + 16)) : 0u);
            }
            const uint32_t nsp = ad_spread16(nm);
            for (uint32_t x = 0; x < 4; ++x) {
                if (!((ralive >> x) & 1u)) continue; // (uniform)
                const uint32_t miss = pt_miss(code, nsp, x, valid), cnt = __popc(miss);
                uint32_t inc = cnt;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t v = __shfl_up(inc, off);
                    if (lane >= off) inc += v;
                }
                const uint32_t before = ((rmm >> (8u * x)) & 0xFFu) + inc - cnt, total = ((rmm >> (8u * x)) & 0xFFu) + __shfl(inc, 63);
                if (has && before <= PT_MAX_MISS) {
                    const uint32_t c = pt_scan(miss, lo, hi, behind, before, min_len);
                    rbest = c > rbest ? c : rbest;
                }
                if (total > PT_MAX_MISS) ralive &= ~(1u << x);
                else rmm = (rmm & ~(0xFFu << (8u * x))) | (total << (8u * x));
            }
            const uint64_t low = qtop >= 63 ? (qtop - 63) << 4 : 0, next = low > ra ? low : ra;
            rn += (uint32_t)(rpos - next);
            rpos = next;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_xor(rbest, off);
            rbest = o > rbest ? o : rbest;
        }
        if (lane == src) {
            best = rbest > best ? rbest : best;
            alive = 0;
        }
    }
    if (ok) {
        if (L) atomicAdd(&s_n[0], (unsigned long long)L);
        if (best) { // (best <= L: no more bases were taken than the range holds)
            end[i] = y - best;
            if (klen) klen[i] = L - best;
            atomicAdd(&s_n[1], 1ull);
            atomicAdd(&s_n[2], (unsigned long long)best);
            if (best == L) atomicAdd(&s_n[3], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_n[threadIdx.x]) atomicAdd(&work[RT_PT_BASES_SEEN + threadIdx.x], s_n[threadIdx.x]);
}

hipError_t launch_poly_tail(const AdapterPoints& a, uint32_t letters, uint32_t min_len, uint64_t* end, uint64_t* klen, unsigned long long* work, hipStream_t stream,
    KernelTimer timer)
{
    if (!a.n_reads || a.n_reads > MAX_BATCH_READS) return hipErrorInvalidValue;
    if (!letters || letters > 0xFu || min_len < PT_MIN_LEN_LO || min_len > PT_MIN_LEN_HI) return hipErrorInvalidValue;
    if (!a.offsets || !a.begin || !end || !work || (a.n_bases && !a.text && !a.words)) return hipErrorInvalidValue;
    // the set by letter code (A0 C1 T2 G3) from the set by letter (bit 0 A, 1 C, 2 G, 3 T)
    const uint32_t by_code = (letters & 3u) | ((letters & 4u) << 1) | ((letters & 8u) >> 1);
    launch_timed(timer, poly_tail_kernel, dim3((uint32_t)((a.n_reads + 1 + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, stream, a, by_code, min_len, end, klen, work);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
