// base_mask.hip -- base masking (drprg_hip_set_base_mask; the rule: include/drprg_hip.h "base masking"): every base of a
// ragged batch whose Phred quality is below Q becomes an unknown base, in place, in either form of the batch.  Driven by
// Mapper::run_base_mask, which owns every buffer.
//
// base_mask_kernel tiles the BUFFER, not the reads -- 16 384 bases per workgroup, 64 per lane, as bam_pack_kernel does -- so that every
// 16-byte group of text, every packed word and every 64-bit piece of the bitmap has ONE writer: no atomic touches the bases.  A lane's
// qualities are four 16-byte loads at its own positions (quality byte = base position for a forward read).  Only a block with
// reverse-strand reads (rev != null: BAM, whose QUAL stays in stored order while bam_pack_kernel reversed the bases) needs the read that
// holds a position: the reads of a tile's first and last base come from two searches, a lane's own from a search between the two, every
// further one by walking; a 16-base group that touches a reversed read is gathered byte by byte from quality byte s + e - 1 - p.  The
// mapping is a permutation inside every read, so each quality byte is range-checked exactly once; a byte outside [bias, bias + 93] sends
// its position + 1 to the error word by an atomic min.
//
// Text: the byte becomes 'N' (16-byte stores for whole groups, byte stores for the block's last piece: the pad behind n_bases is never
// written).  Packed: the 2-bit letter becomes 3 -- what pack_kernel makes of 'N' -- and the position is ORed into the bitmap
// launch_mark_npos made of the block's list; the workgroup leaves the set bits of its chunk in chunk_count and adds them to
// work[BM_LISTED], so the host knows the new list's length with the counts and launches the scan and base_mask_emit_kernel (positions
// ascending, without a sort and without a duplicate: the two-pass shape of bam_pack.hip) only for a block whose list changed.
// reads_masked wants every read once: a lane with a masked base walks the reads under its bits and claims each in read_flag (one atomicOr
// per read and lane).  The counts are reduced per wave and leave the workgroup in one atomic each.  HBM-bound by design: n bytes read;
// written only where a base was masked.  Every index that comes from device data is bounded before it is used.
#include "search.h"

namespace drprg {
namespace dev {

constexpr int BM_THREADS = 256;
constexpr uint32_t BM_LANE_BASES = 64;
constexpr uint32_t BM_TILE = BM_THREADS * BM_LANE_BASES; // 16384 bases per workgroup
static_assert(BM_TILE == BASE_MASK_TILE, "kernels.h states the tile that other files count chunks by");
constexpr uint32_t BM_MAX_QUAL = 93;

uint32_t base_mask_tiles(uint64_t n_bases) { return (uint32_t)((n_bases + BM_TILE - 1) / BM_TILE); }

// bit i of a 16-bit mask -> bits 2 i and 2 i + 1
__device__ inline uint32_t bm_spread2(uint32_t x)
{
    x = (x | x << 8) & 0x00FF00FFu;
    x = (x | x << 4) & 0x0F0F0F0Fu;
    x = (x | x << 2) & 0x33333333u;
    x = (x | x << 1) & 0x55555555u;
    return x * 3u;
}

// one quality byte: low = below the threshold, bad = outside 0..93 (a byte below the bias wraps to a large value: bad, never low)
__device__ inline void bm_judge(uint32_t byte, uint32_t bias, uint32_t min_qual, uint32_t& low, uint32_t& bad)
{
    const uint32_t q = byte - bias;
    bad = q > BM_MAX_QUAL ? 1u : 0u;
    low = q < min_qual ? 1u : 0u;
}

__device__ inline unsigned long long bm_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <bool TEXT> __global__ __launch_bounds__(BM_THREADS) void base_mask_kernel(BaseMaskArgs a)
{
    __shared__ uint64_t s_read[2];
    __shared__ uint32_t s_w[BM_THREADS / 64 + 1];
    __shared__ unsigned long long s_n[3];
    const uint64_t tile = (uint64_t)blockIdx.x * BM_TILE;
    if (tile >= a.n_bases) return; // (uniform)
    const uint64_t tile_end = a.n_bases - tile > BM_TILE ? tile + BM_TILE : a.n_bases;
    if (threadIdx.x < 3) s_n[threadIdx.x] = 0;
    if (threadIdx.x == 0 || threadIdx.x == 64) s_read[threadIdx.x >> 6] = read_holding(a.offsets, 0, a.n_reads - 1, threadIdx.x == 0 ? tile : tile_end - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0 && (a.offsets[0] != 0 || a.offsets[a.n_reads] != a.n_bases)) a.work[BM_OFFSETS] = 1;
    __syncthreads();
    const uint64_t p0 = tile + (uint64_t)threadIdx.x * BM_LANE_BASES;
    const bool aligned_q = (reinterpret_cast<uintptr_t>(a.qual) & 15u) == 0;
    uint64_t mask = 0, bad_at = ~0ull; // mask: bit i set when base p0 + i is below the threshold
    bool odd = false;                  // the offsets and n_bases do not fit each other
    unsigned long long n_reads_masked = 0, n_masked = 0, n_already = 0;
    uint32_t n_listed = 0;
    if (p0 < tile_end) {
        const uint32_t n = (uint32_t)(tile_end - p0 < BM_LANE_BASES ? tile_end - p0 : BM_LANE_BASES);
        uint4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) // (the buffer is padded: the 16 bytes at a position below n_bases are readable when it is aligned)
            v[j] = aligned_q && p0 + 16u * j < tile_end ? load_once_16(a.qual + p0 + 16u * j) : make_uint4(0, 0, 0, 0);
        uint64_t r = 0, s = 0, e = 0;
        if (a.rev) {
            r = read_holding(a.offsets, s_read[0], s_read[1], p0);
            s = a.offsets[r];
            e = a.offsets[r + 1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t g0 = p0 + 16u * j;
            if (g0 >= tile_end) break;
            const uint32_t ng = (uint32_t)(tile_end - g0 < 16 ? tile_end - g0 : 16);
            bool direct = true; // quality byte = base position for the whole group
            if (a.rev) {
                while (r + 1 < a.n_reads && e <= g0) {
                    ++r;
                    s = e;
                    e = a.offsets[r + 1];
                }
                direct = s <= g0 && g0 + ng <= e && !a.rev[r];
            }
            uint32_t low16 = 0;
            if (direct) {
                uint32_t w[4] = { v[j].x, v[j].y, v[j].z, v[j].w }, bad16 = 0;
                if (!aligned_q) { // byte by byte, and never behind n_bases: such a buffer promises no padding
                    w[0] = w[1] = w[2] = w[3] = 0;
                    for (uint32_t i = 0; i < ng; ++i) w[i >> 2] |= (uint32_t)a.qual[g0 + i] << (8 * (i & 3));
                }
#pragma unroll
                for (uint32_t i = 0; i < 16; ++i) {
                    uint32_t low, bad;
                    bm_judge((w[i >> 2] >> (8 * (i & 3))) & 0xFFu, a.bias, a.min_qual, low, bad);
                    low16 |= low << i;
                    bad16 |= bad << i;
                }
                low16 &= (1u << ng) - 1u; // (ng == 16: the shift gives 0x10000)
                bad16 &= (1u << ng) - 1u;
                if (bad16) {
                    const uint64_t at = g0 + (uint64_t)(__ffs(bad16) - 1);
                    if (at < bad_at) bad_at = at;
                }
            } else {
                uint64_t rr = r, ss = s, ee = e;
                for (uint32_t i = 0; i < ng; ++i) {
                    const uint64_t p = g0 + i;
                    while (rr + 1 < a.n_reads && ee <= p) {
                        ++rr;
                        ss = ee;
                        ee = a.offsets[rr + 1];
                    }
                    if (p < ss || p >= ee || ee > a.n_bases) { // (offsets that do not ascend)
                        odd = true;
                        continue;
                    }
                    const uint64_t at = a.rev[rr] ? ss + (ee - 1 - p) : p; // ss <= at < ee <= n_bases
                    uint32_t low, bad;
                    bm_judge(a.qual[at], a.bias, a.min_qual, low, bad);
                    low16 |= low << i;
                    if (bad && at < bad_at) bad_at = at;
                }
            }
            mask |= (uint64_t)low16 << (16 * j);
        }
        // the bases
        if (TEXT) {
            const bool aligned_t = (reinterpret_cast<uintptr_t>(a.text) & 15u) == 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t low16 = (uint32_t)(mask >> (16 * j)) & 0xFFFFu;
                const uint64_t g0 = p0 + 16u * j;
                if (!low16) continue;
                uint32_t unknown16 = 0;
                if (aligned_t && g0 + 16 <= a.n_bases) {
                    uint4 t = *reinterpret_cast<const uint4*>(a.text + g0);
                    uint32_t w[4] = { t.x, t.y, t.z, t.w };
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t nb = encode4(w[k]) & 0x04040404u, lk = (low16 >> (4 * k)) & 15u;
                        unknown16 |= ((nb >> 2 & 1u) | (nb >> 9 & 2u) | (nb >> 16 & 4u) | (nb >> 23 & 8u)) << (4 * k);
                        const uint32_t bm = ((lk & 1u) * 0xFFu) | ((lk >> 1 & 1u) * 0xFF00u) | ((lk >> 2 & 1u) * 0xFF0000u) | ((lk >> 3 & 1u) * 0xFF000000u);
                        w[k] = (w[k] & ~bm) | (0x4E4E4E4Eu & bm); // 'N'
                    }
                    *reinterpret_cast<uint4*>(a.text + g0) = make_uint4(w[0], w[1], w[2], w[3]);
                } else {
                    for (uint32_t m = low16; m; m &= m - 1) {
                        const uint32_t i = (uint32_t)__ffs(m) - 1u;
                        if (g0 + i >= a.n_bases) break;
                        if (encode_base(a.text[g0 + i]) > 3u) unknown16 |= 1u << i;
                        a.text[g0 + i] = 'N';
                    }
                }
                n_masked += (uint32_t)__popc(low16 & ~unknown16);
                n_already += (uint32_t)__popc(low16 & unknown16);
            }
        } else {
            const uint64_t w0 = p0 >> 4, n_words = (a.n_bases + 15) >> 4;
            uint64_t* const bits = reinterpret_cast<uint64_t*>(a.nbits + w0); // (p0 is a multiple of 64: 8-byte aligned; the bitmap has 8 words behind its last)
            const uint64_t old = *bits, now = old | mask;
            if (now != old) *bits = now;
            n_masked = (uint32_t)__popcll(mask & ~old);
            n_already = (uint32_t)__popcll(mask & old);
            n_listed = (uint32_t)__popcll(n < 64 ? now & ((1ull << n) - 1ull) : now);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t low16 = (uint32_t)(mask >> (16 * j)) & 0xFFFFu;
                if (low16 && w0 + j < n_words) a.words[w0 + j] |= bm_spread2(low16);
            }
        }
        // the reads that hold a masked base, each claimed once
        if (mask) {
            uint64_t rr = read_holding(a.offsets, s_read[0], s_read[1], p0 + (uint64_t)(__ffsll((long long)mask) - 1));
            for (uint64_t m = mask; m;) {
                const uint64_t p = p0 + (uint64_t)(__ffsll((long long)m) - 1);
                while (rr + 1 < a.n_reads && a.offsets[rr + 1] <= p) ++rr;
                const uint64_t ee = a.offsets[rr + 1];
                m &= m - 1;
                if (ee > p0) m = ee - p0 >= 64 ? 0 : m & (~0ull << (ee - p0)); // the read's other bits under this lane
                if (atomicOr(&a.read_flag[rr], 1u) == 0) ++n_reads_masked;
            }
        }
    }
    if (bad_at != ~0ull) atomicMin(&a.work[BM_BAD_AT], (unsigned long long)(bad_at + 1));
    if (odd) a.work[BM_OFFSETS] = 1;
    n_reads_masked = bm_wave_sum(n_reads_masked);
    n_masked = bm_wave_sum(n_masked);
    n_already = bm_wave_sum(n_already);
    if ((threadIdx.x & 63) == 0) {
        if (n_reads_masked) atomicAdd(&s_n[0], n_reads_masked);
        if (n_masked) atomicAdd(&s_n[1], n_masked);
        if (n_already) atomicAdd(&s_n[2], n_already);
    }
    uint32_t total = 0;
    if (!TEXT) (void)block_exclusive_scan<BM_THREADS / 64>(n_listed, s_w, &total);
    __syncthreads();
    if (threadIdx.x < 3 && s_n[threadIdx.x]) atomicAdd(&a.work[BM_READS_MASKED + threadIdx.x], s_n[threadIdx.x]);
    if (!TEXT && threadIdx.x == 0) {
        a.chunk_count[blockIdx.x] = total;
        if (total) atomicAdd(&a.work[BM_LISTED], (unsigned long long)total);
    }
}

// the set bits of the bitmap below n_bases as positions, ascending, from chunk_prefix[workgroup] on (entries at or beyond out_cap are dropped)
__global__ __launch_bounds__(BM_THREADS) void base_mask_emit_kernel(const uint16_t* __restrict__ nbits, uint64_t n_bases, const uint32_t* __restrict__ chunk_prefix,
    uint64_t* __restrict__ out, uint64_t out_cap)
{
    __shared__ uint32_t s_w[BM_THREADS / 64 + 1];
    if (chunk_prefix[blockIdx.x + 1] == chunk_prefix[blockIdx.x]) return; // (uniform) nothing to list here
    const uint64_t p0 = (uint64_t)blockIdx.x * BM_TILE + (uint64_t)threadIdx.x * BM_LANE_BASES;
    uint64_t bits = 0;
    if (p0 < n_bases) {
        bits = *reinterpret_cast<const uint64_t*>(nbits + (p0 >> 4));
        if (n_bases - p0 < 64) bits &= (1ull << (n_bases - p0)) - 1ull;
    }
    uint32_t total = 0;
    const uint32_t before = block_exclusive_scan<BM_THREADS / 64>((uint32_t)__popcll(bits), s_w, &total);
    uint64_t at = (uint64_t)chunk_prefix[blockIdx.x] + before;
    for (; bits; bits &= bits - 1, ++at)
        if (at < out_cap) out[at] = p0 + (uint64_t)(__ffsll((long long)bits) - 1);
}

hipError_t launch_base_mask(const BaseMaskArgs& a, hipStream_t stream, KernelTimer timer)
{
    if (!a.n_reads || a.n_reads > MAX_BATCH_READS || a.min_qual < 1 || a.min_qual > BM_MAX_QUAL || (a.bias != 0 && a.bias != 33)) return hipErrorInvalidValue;
    if ((a.text != nullptr) == (a.words != nullptr) || (a.words && (!a.nbits || !a.chunk_count))) return hipErrorInvalidValue;
    HIP_TRY(hipMemsetAsync(a.work, 0, BM_WORDS * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(a.work + BM_BAD_AT, 0xFF, sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(a.read_flag, 0, a.n_reads * sizeof(uint32_t), stream));
    const uint32_t n_tiles = base_mask_tiles(a.n_bases);
    if (!n_tiles) return hipSuccess;
    if (a.text) launch_timed(timer, base_mask_kernel<true>, dim3(n_tiles), dim3(BM_THREADS), 0, stream, a);
    else launch_timed(timer, base_mask_kernel<false>, dim3(n_tiles), dim3(BM_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_base_mask_emit(const uint16_t* nbits, uint64_t n_bases, uint32_t* chunk_count, uint32_t* chunk_prefix, void* temp, size_t temp_bytes, uint64_t* out,
    uint64_t out_cap, hipStream_t stream)
{
    const uint32_t n_tiles = base_mask_tiles(n_bases);
    if (!n_tiles || !out_cap) return hipSuccess;
    HIP_TRY(hipMemsetAsync(chunk_count + n_tiles, 0, sizeof(uint32_t), stream));
    HIP_TRY(exclusive_scan_u32(temp, temp_bytes, chunk_count, chunk_prefix, n_tiles + 1, stream));
    hipLaunchKernelGGL(base_mask_emit_kernel, dim3(n_tiles), dim3(BM_THREADS), 0, stream, nbits, n_bases, (const uint32_t*)chunk_prefix, out, out_cap);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
