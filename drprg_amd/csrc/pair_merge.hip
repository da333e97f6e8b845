// pair_merge.hip -- overlapping mates merged into one read (drprg_hip_set_pair_merge; the rule: include/drprg_hip.h "mate merging",
// DESIGN.md section 4).  Driven by Mapper::pair_overlap_kept and Mapper::pair_merge_device, which own every buffer named here.
//
// pair_merge_kernel runs behind pair_overlap_kernel and reads its shift[] and the DedupLoc table it read.  One wave per side-1 read of the
// launch's range.  A pair with a chosen shift d is staged in LDS exactly as the overlap kernel stages it (pair_stage.h: a and B =
// revcomp(b) as read-aligned 16-base words, the known masks at the even bits); lane t then builds word j = t, t + 64 of the merged read M
// (I = Lb + d bases, at most 128 words): a's aligned word j against B's window at 16 j - d -- one funnel shift of two LDS words, zero words
// where the window leaves B -- agree = ~(df | df >> 1) at the even bits, letters = ka ? a : B, known = (ka ^ kb) | (ka & kb & agree), both
// cut at p < I, and a base that is not known gets letter 3, which is what an N packs to.  The five column counts are popcounts of the same
// masks under the mask of the columns both mates cover; they are summed over the wave by shuffles, over the workgroup in LDS, and a
// workgroup makes one global atomic per non-zero word (a maximum for the longest merged read).  With `all` set the wave of any other read
// places the bases that read keeps, word by word from po_read_word, letters as they lie.
//
// Alignment: a read starts at any of the 16 phases of a destination word, so a word of M falls on two destination words and shares them
// with its neighbours.  The choice here is ATOMIC OR INTO ZEROED WORDS (the caller clears words and bitmap) for the words reads can share,
// ONE WRITER for the rest: a lane builds a destination word of its read from two of the read's words (one shuffle), the read's first and
// last destination word are ORed in atomically, and every word between them, which no other read touches, takes a plain store.  (A first
// form ORed every word in as two parts: 28.8 ms for 2.75 M merged pairs in a kernel trace, twice the overlap kernel.)  Unknown bases go
// by atomic OR into the bitmap (one bit per base, as launch_mark_npos lays it out), from which the ascending list is made by
// base_mask.hip's emit.  A text destination takes plain byte stores.
// Only vector stores and ordinary atomics; no inline assembly.
//
// Every index that comes from device data is checked against the sizes the caller gave: a shift, a mate number, a length or an offset that
// does not fit sets the error word and the read writes nothing.
#include "device_common.h"
#include "pair_stage.h"

namespace drprg {
namespace dev {

constexpr int PM_THREADS = 256;
constexpr int PM_WAVES = PM_THREADS / 64;
constexpr uint32_t PM_TILE = BASE_MASK_TILE; // the bases under one chunk count, as launch_base_mask_emit reads them
static_assert(PM_TILE == PM_THREADS * 64, "a lane of the count kernel takes 64 bases");

// the even bits of the bases lo <= p < hi of the 16-base word that starts at base p0
__device__ inline uint32_t pm_range(uint32_t p0, int64_t lo, int64_t hi)
{
    const int64_t x = lo - (int64_t)p0, y = hi - (int64_t)p0;
    const uint32_t nx = x <= 0 ? 0u : (x >= 16 ? 16u : (uint32_t)x), ny = y <= 0 ? 0u : (y >= 16 ? 16u : (uint32_t)y);
    if (ny <= nx) return 0u;
    const uint32_t below_y = ny == 16 ? 0xFFFFFFFFu : (1u << (2 * ny)) - 1u, below_x = (1u << (2 * nx)) - 1u; // (nx < 16 here)
    return (below_y & ~below_x) & 0x55555555u;
}

// bit 2t of m -> bit t (the inverse of po_even)
__device__ inline uint32_t pm_odd_out(uint32_t m)
{
    m &= 0x55555555u;
    m = (m | m >> 1) & 0x33333333u;
    m = (m | m >> 2) & 0x0F0F0F0Fu;
    m = (m | m >> 4) & 0x00FF00FFu;
    m = (m | m >> 8) & 0x0000FFFFu;
    return m;
}

// Word k of a read of `len` bases that lies at base `at` of the destination (letters clear behind the read's end, known at the even
// bits; both zero for k at or beyond the read's words), called by all lanes of the wave with k = 64 r + lane, r = 0, 1, ...: `carry` hands
// lane 63's letters to lane 0 of the next round.  Text: the word's bytes.  Packed: lane k writes DESTINATION word k of the read, its own
// letters shifted up by the read's phase under the top of word k - 1 (one shuffle); the read's first and last destination word, which a
// neighbour may share, are ORed in atomically, every word between them is this read's alone and takes a plain store.  Unknown bases are
// few: they go into the bitmap by atomic OR.
__device__ inline void pm_place(const PairMergeArgs& a, uint64_t at, uint64_t len, uint64_t k, uint32_t lane, uint32_t letters, uint32_t known, uint32_t& carry)
{
    const uint64_t nw = (len + 15) >> 4;
    const uint32_t nv = k < nw ? (uint32_t)(len - 16 * k < 16 ? len - 16 * k : 16) : 0u;
    if (a.text) {
        for (uint32_t t = 0; t < nv; ++t) a.text[at + 16 * k + t] = (known >> (2 * t)) & 1u ? "ACTG"[(letters >> (2 * t)) & 3u] : 'N';
        return;
    }
    const uint32_t phase = (uint32_t)(at & 15u);
    uint32_t prev = __shfl_up(letters, 1);
    if (lane == 0) prev = carry;
    carry = __shfl(letters, 63);
    const uint64_t nwd = (phase + len + 15) >> 4; // destination words the read touches (nw or nw + 1)
    if (k < nwd) {
        const uint32_t v = phase ? (letters << (2 * phase)) | (prev >> (32 - 2 * phase)) : letters;
        uint32_t* const w = a.words + (at >> 4) + k;
        if (k == 0 || k == nwd - 1) {
            if (v) atomicOr(w, v);
        } else *w = v;
    }
    const uint32_t unknown = nv ? ~pm_odd_out(known) & (nv < 16 ? (1u << nv) - 1u : 0xFFFFu) : 0u;
    if (unknown) {
        uint32_t* const bits = reinterpret_cast<uint32_t*>(a.nbits);
        const uint64_t p = at + 16 * k, q = p >> 5;
        const uint32_t sh = (uint32_t)(p & 31u);
        atomicOr(&bits[q], unknown << sh);
        if (sh > 16 && unknown >> (32 - sh)) atomicOr(&bits[q + 1], unknown >> (32 - sh));
    }
}

__device__ inline uint32_t pm_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(PM_THREADS) void pair_merge_kernel(PairMergeArgs a)
{
    __shared__ uint32_t s_rows[PM_WAVES][PO_ROWS][PO_ROW];
    __shared__ unsigned long long s_cnt[PM_WORDS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t j = (uint64_t)blockIdx.x * PM_WAVES + wave; // the read's number in the launch's range
    uint32_t (*s)[PO_ROW] = s_rows[wave];
    if (threadIdx.x < PM_WORDS) s_cnt[threadIdx.x] = 0;
    __syncthreads();

    // ---- what this wave does (all of it uniform in the wave) ----
    DedupLoc me {}, other {};
    bool merged = false, plain = false, bad = false;
    int32_t d = 0;
    uint64_t at = 0, room = 0;
    const uint64_t i = a.first + j;
    if (j < a.n_reads && i < a.n1) {
        me = a.loc[i];
        at = a.noff[j];
        const uint64_t end = a.noff[j + 1];
        if (end < at || end > a.new_bases) bad = true;
        else {
            room = end - at;
            d = a.shift[i];
            if (d > PO_NOT_JUDGED) {
                const uint32_t mt = a.mate[i];
                if (mt >= a.n || mt < a.n1) bad = true;
                else {
                    other = a.loc[mt];
                    const int64_t La = (int64_t)me.len, Lb = (int64_t)other.len;
                    if (La < 1 || Lb < 1 || La > (int64_t)PO_MAX_LEN || Lb > (int64_t)PO_MAX_LEN || d <= -Lb || d >= La || (int64_t)room != Lb + d) bad = true;
                    else merged = true;
                }
            } else if (a.all && room) {
                if (room > me.len || a.text) bad = true;
                else plain = true;
            }
        }
    } else if (j < a.n_reads) bad = true;
    if (bad && lane == 0) *a.err = 1;

    po_stage_rows(s, me, other, merged, lane);

    uint32_t n_agree = 0, n_dis = 0, n_fill = 0, n_unk = 0;
    if (merged) {
        const uint32_t La = (uint32_t)me.len, I = (uint32_t)room;
        const uint32_t nw = (I + 15) >> 4;
        uint32_t carry = 0;
        for (uint32_t k = lane; k - lane <= nw; k += 64) { // (uniform: one word more than M has, for the word its phase spills into)
            uint32_t letters = 0, known = 0;
            if (k < nw) {
                const uint32_t p0 = 16 * k;
                const uint32_t av = k < PO_ROW ? s[PO_A][k] : 0u, ka = k < PO_ROW ? s[PO_KA][k] : 0u;
                // B's window at q = 16 k - d (-1024 < q < Lb): rows b0 and b0 + 1, zero words in front of B
                const int32_t q = (int32_t)p0 - d, b0 = q >> 4;
                const uint32_t sh = 2 * ((uint32_t)q & 15u);
                const uint32_t lw = b0 >= 0 ? s[PO_B][b0] : 0u, lk = b0 >= 0 ? s[PO_KB][b0] : 0u;
                const uint32_t hw = b0 >= -1 ? s[PO_B][b0 + 1] : 0u, hk = b0 >= -1 ? s[PO_KB][b0 + 1] : 0u; // (b0 + 1 <= 64 < PO_ROW: q < Lb)
                const uint32_t bv = po_funnel(lw, hw, sh), kb = po_funnel(lk, hk, sh);
                const uint32_t in = pm_range(p0, 0, I);
                const uint32_t df = av ^ bv, agree = ~(df | df >> 1) & 0x55555555u;
                const uint32_t both = ka & kb;
                known = ((ka ^ kb) | (both & agree)) & in;
                const uint32_t from_a = ka | ka << 1, kn2 = known | known << 1, in2 = in | in << 1;
                letters = ((((av & from_a) | (bv & ~from_a)) & kn2) | ~kn2) & in2;
                const uint32_t covered = pm_range(p0, 0, La) & pm_range(p0, d, I) & in;
                n_agree += __popc(both & agree & covered);
                n_dis += __popc(both & ~agree & covered);
                n_fill += __popc((ka ^ kb) & covered);
                n_unk += __popc(~(ka | kb) & covered);
            }
            pm_place(a, at, I, k, lane, letters, known, carry); // (every lane of the wave: it shuffles)
        }
    } else if (plain) {
        const uint64_t nw = (room + 15) >> 4;
        uint32_t carry = 0;
        for (uint64_t k = lane; k - lane <= nw; k += 64) { // (uniform, as above)
            uint32_t v = 0, m = 0;
            if (k < nw) {
                po_read_word(me, (uint32_t)k, v, m);
                const uint32_t nv = (uint32_t)(room - 16 * k < 16 ? room - 16 * k : 16);
                const uint32_t in = nv < 16 ? (1u << (2 * nv)) - 1u : 0xFFFFFFFFu;
                v &= in;
                m &= in;
            }
            pm_place(a, at, room, k, lane, v, m, carry);
        }
    }
    n_agree = pm_wave_sum(n_agree);
    n_dis = pm_wave_sum(n_dis);
    n_fill = pm_wave_sum(n_fill);
    n_unk = pm_wave_sum(n_unk);
    if (merged && lane == 0) {
        atomicAdd(&s_cnt[PM_MERGED], 1ull);
        atomicAdd(&s_cnt[PM_BOTH], (unsigned long long)(n_agree + n_dis + n_fill + n_unk));
        if (n_agree) atomicAdd(&s_cnt[PM_AGREE], (unsigned long long)n_agree);
        if (n_dis) atomicAdd(&s_cnt[PM_DISAGREE], (unsigned long long)n_dis);
        if (n_fill) atomicAdd(&s_cnt[PM_FILLED], (unsigned long long)n_fill);
        if (n_unk) atomicAdd(&s_cnt[PM_UNKNOWN_BOTH], (unsigned long long)n_unk);
        atomicAdd(&s_cnt[PM_BASES], (unsigned long long)room);
        atomicMax(&s_cnt[PM_LONGEST], (unsigned long long)room);
    }
    __syncthreads();
    if (threadIdx.x < PM_WORDS && s_cnt[threadIdx.x]) {
        if (threadIdx.x == PM_LONGEST) atomicMax(&a.counts[PM_LONGEST], s_cnt[PM_LONGEST]);
        else atomicAdd(&a.counts[threadIdx.x], s_cnt[threadIdx.x]);
    }
}

__global__ __launch_bounds__(PM_THREADS) void pair_merge_lengths_kernel(const int32_t* __restrict__ shift, const uint64_t* __restrict__ keep, uint64_t n1,
    uint64_t* __restrict__ len)
{
    const uint64_t i = (uint64_t)blockIdx.x * PM_THREADS + threadIdx.x;
    if (i > n1) return;
    len[i] = i < n1 && shift[i] > PO_NOT_JUDGED ? keep[i] : 0;
}

__global__ __launch_bounds__(PM_THREADS) void pair_merge_table_kernel(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets, uint64_t n_reads,
    uint64_t n_bases, uint64_t first, uint64_t n1, const int32_t* __restrict__ shift, const uint64_t* __restrict__ keep, const uint64_t* __restrict__ noff,
    uint64_t new_bases, GatherEntry* __restrict__ table, uint32_t* __restrict__ err)
{
    const uint64_t j = (uint64_t)blockIdx.x * PM_THREADS + threadIdx.x;
    if (j >= n_reads) return;
    const uint64_t s = offsets[j], e = offsets[j + 1], k = keep[first + j], at = noff[j];
    const bool merged = first + j < n1 && shift[first + j] > PO_NOT_JUDGED;
    const bool ok = s <= e && e <= n_bases && noff[j + 1] == at + k && at + k <= new_bases && (merged || (k <= e - s && k <= 0xFFFFFFFFull));
    if (!ok) *err = 1;
    table[j] = GatherEntry { bases + (ok ? s : 0), ok ? at : 0, ok && !merged ? (uint32_t)k : 0u, 0 };
}

// one workgroup per PM_TILE bases, a lane per 64 of them, as base_mask_emit_kernel reads the bitmap
__global__ __launch_bounds__(PM_THREADS) void pair_merge_bits_count_kernel(const uint16_t* __restrict__ nbits, uint64_t n_bases, uint32_t* __restrict__ chunk_count,
    unsigned long long* __restrict__ total)
{
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint64_t p0 = (uint64_t)blockIdx.x * PM_TILE + (uint64_t)threadIdx.x * 64;
    uint64_t bits = 0;
    if (p0 < n_bases) {
        bits = *reinterpret_cast<const uint64_t*>(nbits + (p0 >> 4));
        if (n_bases - p0 < 64) bits &= (1ull << (n_bases - p0)) - 1ull;
    }
    const uint32_t n = pm_wave_sum((uint32_t)__popcll(bits));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        chunk_count[blockIdx.x] = s_n;
        if (s_n) atomicAdd(total, (unsigned long long)s_n);
    }
}

hipError_t launch_pair_merge(const PairMergeArgs& a, hipStream_t stream)
{
    if (!a.n_reads) return hipSuccess;
    if (a.n >= (1ull << 32) || a.n1 > a.n || a.first + a.n_reads > a.n1 || (a.text != nullptr) == (a.words != nullptr) || (a.words && !a.nbits) || (a.text && a.all))
        return hipErrorInvalidValue;
    const uint64_t grid = (a.n_reads + PM_WAVES - 1) / PM_WAVES;
    if (grid >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pair_merge_kernel, dim3((uint32_t)grid), dim3(PM_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_pair_merge_lengths(const int32_t* shift, const uint64_t* keep, uint64_t n1, uint64_t* len, hipStream_t stream)
{
    hipLaunchKernelGGL(pair_merge_lengths_kernel, dim3((uint32_t)((n1 + 1 + PM_THREADS - 1) / PM_THREADS)), dim3(PM_THREADS), 0, stream, shift, keep, n1, len);
    return hipGetLastError();
}

hipError_t launch_pair_merge_table(const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t n_bases, uint64_t first, uint64_t n1, const int32_t* shift,
    const uint64_t* keep, const uint64_t* noff, uint64_t new_bases, GatherEntry* table, uint32_t* err, hipStream_t stream)
{
    if (!n_reads) return hipSuccess;
    hipLaunchKernelGGL(pair_merge_table_kernel, dim3((uint32_t)((n_reads + PM_THREADS - 1) / PM_THREADS)), dim3(PM_THREADS), 0, stream, bases, offsets, n_reads, n_bases, first,
        n1, shift, keep, noff, new_bases, table, err);
    return hipGetLastError();
}

hipError_t launch_pair_merge_bits_count(const uint16_t* nbits, uint64_t n_bases, uint32_t* chunk_count, unsigned long long* total, hipStream_t stream)
{
    const uint32_t n_tiles = base_mask_tiles(n_bases);
    if (!n_tiles) return hipSuccess;
    hipLaunchKernelGGL(pair_merge_bits_count_kernel, dim3(n_tiles), dim3(PM_THREADS), 0, stream, nbits, n_bases, chunk_count, total);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
