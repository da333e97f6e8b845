// bam_pack.hip -- BAM's 4-bit sequence fields -> the 2-bit packed form (kernels.h SketchArgs::packed) on the device: what a block of a BAM
// file becomes before it is mapped (include/drprg_hip.h "BAM input"; the rule: bam.h).
//
// Gather form: a lane makes four whole output words (64 bases, one 16-byte store), so a word that two reads share has one writer and no
// atomics touch the words.  The read that holds a workgroup's first and last base comes from two binary searches over `offsets`, a lane's
// own read from a search between the two (a handful of steps for short reads), every further read by walking forward.  A word that lies
// wholly inside one forward read -- all but a few words of an unaligned BAM -- is one unaligned 8-byte load (and one byte more when the
// word starts on a low nibble) with the nibbles put in base order by shifts and masks; anything else is gathered base by base.  The 16
// codes of a word are then looked up in two register constants: the 2-bit letters (bits 2:1 of the ASCII code of the upper-case letter,
// as pack_kernel takes them from text) and the non-ACGT bits.
//
// The non-ACGT positions come out ascending without a sort: the first launch leaves every workgroup's count, one scan turns the counts
// into starts, and a second launch -- whose workgroups without such a position return at once, i.e. nearly all of them -- makes the
// masks of its 16384 bases again and writes the positions in order.  HBM-bound by design: n / 2 bytes read, n / 4 written.
#include "search.h"

namespace drprg {
namespace dev {

constexpr int BP_THREADS = 256;
constexpr int BP_LANE_WORDS = 4;                              // one 16-byte store per lane
constexpr uint32_t BP_CHUNK_WORDS = BP_THREADS * BP_LANE_WORDS; // 16384 bases per workgroup

constexpr uint32_t bp_letters()
{
    const char s[17] = "=ACMGRSVTWYHKDBN";
    uint32_t l = 0;
    for (int c = 0; c < 16; ++c) l |= (((uint32_t)s[c] >> 1) & 3u) << (2 * c);
    return l;
}
constexpr uint64_t bp_complements()
{
    uint64_t t = 0;
    for (uint64_t c = 0; c < 16; ++c) t |= ((c & 1) << 3 | (c & 2) << 1 | (c & 4) >> 1 | (c & 8) >> 3) << (4 * c);
    return t;
}
constexpr uint32_t BP_LETTERS = bp_letters();       // letter of code c in bits [2 c + 1 : 2 c]
constexpr uint32_t BP_NON_ACGT = 0xFEE9u;           // bit c: code c is not A (1), C (2), G (4) or T (8)
constexpr uint64_t BP_COMPLEMENT = bp_complements(); // the 4-bit reversal of code c in bits [4 c + 3 : 4 c]

uint32_t bam_pack_chunks(uint64_t n_bases) { return (uint32_t)((((n_bases + 15) >> 4) + BP_CHUNK_WORDS - 1) / BP_CHUNK_WORDS); }

// (the two functions below, and read_holding of search.h, are host code as well, so that a CPU build can walk the kernel's index arithmetic
// under a sanitizer)
struct BamBatch {
    const uint8_t* seq;
    const uint64_t* seq_start;
    const uint64_t* offsets;
    const uint8_t* reverse; // may be null: every read forward
    uint64_t n_reads, n_bases;
};

// 16 codes (code i in bits [4 i + 3 : 4 i]) -> their letters; mask: bit i set when code i is not a base
DRPRG_HD inline uint32_t bp_letters_of(uint64_t x, uint32_t& mask)
{
    uint32_t w = 0, m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t c = (uint32_t)(x >> (4 * i)) & 15u;
        w |= ((BP_LETTERS >> (2 * c)) & 3u) << (2 * i);
        m |= ((BP_NON_ACGT >> c) & 1u) << i;
    }
    mask = m;
    return w;
}

// The word of bases [pw, pw + 16) (pw < n_bases) and its non-ACGT mask; r: a read at or before the one that holds pw, moved on to it.
DRPRG_HD inline uint32_t bp_word(const BamBatch& b, uint64_t pw, uint64_t& r, uint32_t& mask)
{
    while (r + 1 < b.n_reads && b.offsets[r + 1] <= pw) ++r;
    const uint64_t start = b.offsets[r], end = b.offsets[r + 1];
    uint64_t x = 0;
    uint32_t valid = 16;
    if (pw + 16 <= end && !(b.reverse && b.reverse[r])) {
        const uint64_t q0 = pw - start;
        const uint8_t* a = b.seq + b.seq_start[r] + (q0 >> 1);
        uint64_t v;
        __builtin_memcpy(&v, a, 8); // (the eight bytes lie inside the read's field: its bases q0 .. q0 + 15 end in byte (q0 + 15) / 2)
        v = (v & 0x0F0F0F0F0F0F0F0Full) << 4 | (v >> 4 & 0x0F0F0F0F0F0F0F0Full); // high nibble first -> base order
        x = (q0 & 1) ? (v >> 4 | (uint64_t)(a[8] >> 4) << 60) : v;
    } else {
        uint64_t rr = r, s = start, e = end;
        valid = (uint32_t)(b.n_bases - pw < 16 ? b.n_bases - pw : 16);
        for (uint32_t i = 0; i < valid; ++i) {
            const uint64_t p = pw + i;
            while (rr + 1 < b.n_reads && e <= p) {
                ++rr;
                s = e;
                e = b.offsets[rr + 1];
            }
            const bool rev = b.reverse && b.reverse[rr];
            const uint64_t q = rev ? e - 1 - p : p - s;
            const uint32_t byte = b.seq[b.seq_start[rr] + (q >> 1)];
            uint32_t c = (q & 1) ? byte & 15u : byte >> 4;
            if (rev) c = (uint32_t)(BP_COMPLEMENT >> (4 * c)) & 15u;
            x |= (uint64_t)c << (4 * i);
        }
    }
    uint32_t w = bp_letters_of(x, mask);
    if (valid < 16) { // the last word: its tail bits stay clear, as pack_kernel leaves them
        w &= (1u << (2 * valid)) - 1u;
        mask &= (1u << valid) - 1u;
    }
    return w;
}

// EMIT == false: the words, and chunk_count[workgroup] = its non-ACGT positions.  EMIT == true: those positions, ascending, from
// chunk_prefix[workgroup] on (entries at or beyond npos_cap are dropped).
template <bool EMIT>
__global__ __launch_bounds__(BP_THREADS) void bam_pack_kernel(BamBatch b, uint32_t* __restrict__ words, uint32_t* __restrict__ chunk_count,
    const uint32_t* __restrict__ chunk_prefix, uint64_t* __restrict__ npos, uint64_t npos_cap)
{
    __shared__ uint64_t s_read[2];
    __shared__ uint32_t s_w[BP_THREADS / 64 + 1];
    const uint64_t n_words = (b.n_bases + 15) >> 4;
    const uint64_t chunk_word = (uint64_t)blockIdx.x * BP_CHUNK_WORDS;
    if (EMIT && chunk_prefix[blockIdx.x + 1] == chunk_prefix[blockIdx.x]) return; // (uniform) nothing to list here
    if (threadIdx.x == 0 || threadIdx.x == 64) {
        const uint64_t chunk_end = chunk_word + BP_CHUNK_WORDS < n_words ? (chunk_word + BP_CHUNK_WORDS) << 4 : b.n_bases;
        s_read[threadIdx.x >> 6] = read_holding(b.offsets, 0, b.n_reads - 1, threadIdx.x == 0 ? chunk_word << 4 : chunk_end - 1);
    }
    __syncthreads();
    const uint64_t w0 = chunk_word + (uint64_t)threadIdx.x * BP_LANE_WORDS;
    uint32_t w[BP_LANE_WORDS], mask[BP_LANE_WORDS], n_bad = 0;
    if (w0 < n_words) {
        uint64_t r = read_holding(b.offsets, s_read[0], s_read[1], w0 << 4);
#pragma unroll
        for (int j = 0; j < BP_LANE_WORDS; ++j) {
            w[j] = 0;
            mask[j] = 0;
            if (w0 + j < n_words) w[j] = bp_word(b, (w0 + j) << 4, r, mask[j]);
            n_bad += (uint32_t)__popc(mask[j]);
        }
        if (!EMIT) {
            if (w0 + BP_LANE_WORDS <= n_words && (reinterpret_cast<uintptr_t>(words) & 15u) == 0)
                *reinterpret_cast<uint4*>(words + w0) = make_uint4(w[0], w[1], w[2], w[3]);
            else
                for (int j = 0; j < BP_LANE_WORDS; ++j)
                    if (w0 + j < n_words) words[w0 + j] = w[j];
        }
    }
    uint32_t total = 0;
    const uint32_t before = block_exclusive_scan<BP_THREADS / 64>(n_bad, s_w, &total);
    if (!EMIT) {
        if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
        return;
    }
    if (!n_bad) return;
    uint64_t at = (uint64_t)chunk_prefix[blockIdx.x] + before;
#pragma unroll
    for (int j = 0; j < BP_LANE_WORDS; ++j)
        for (uint32_t m = mask[j]; m; m &= m - 1, ++at)
            if (at < npos_cap) npos[at] = ((w0 + j) << 4) + (uint64_t)(__ffs(m) - 1);
}

hipError_t launch_bam_pack(const uint8_t* seq, const uint64_t* seq_start, const uint64_t* offsets, const uint8_t* reverse, uint64_t n_reads, uint64_t n_bases,
    uint32_t* words, uint64_t* npos, uint64_t npos_cap, bool list, uint32_t* chunk_count, uint32_t* chunk_prefix, void* temp, size_t temp_bytes, hipStream_t stream)
{
    const uint32_t n_chunks = bam_pack_chunks(n_bases);
    if (!n_chunks || !n_reads) return hipSuccess;
    const BamBatch b { seq, seq_start, offsets, reverse, n_reads, n_bases };
    hipLaunchKernelGGL(bam_pack_kernel<false>, dim3(n_chunks), dim3(BP_THREADS), 0, stream, b, words, chunk_count, (const uint32_t*)nullptr, (uint64_t*)nullptr, 0ull);
    HIP_TRY(hipGetLastError());
    if (!list) return hipSuccess;
    HIP_TRY(hipMemsetAsync(chunk_count + n_chunks, 0, sizeof(uint32_t), stream));
    HIP_TRY(exclusive_scan_u32(temp, temp_bytes, chunk_count, chunk_prefix, n_chunks + 1, stream));
    if (!npos || !npos_cap) return hipSuccess;
    hipLaunchKernelGGL(bam_pack_kernel<true>, dim3(n_chunks), dim3(BP_THREADS), 0, stream, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)chunk_prefix, npos, npos_cap);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
