// read_complexity.hip -- the low-complexity filter (drprg_hip_set_min_complexity; the rule: include/drprg_hip.h "read complexity",
// DESIGN.md section 4): per read D, the number of neighbouring base pairs inside it that differ.  The verdict -- dropped iff L >= 2 and
// 100 D < P (L - 1) -- is read_flags_kernel's (read_qual.hip), which takes D as it takes the decoy screen's V and H; the verdict kernel
// here serves the device entry alone.  Driven by Mapper::run_read_complexity, which owns every buffer.
//
// read_diff_kernel is a segmented count over the batch's concatenated bases.  The BUFFER is tiled, not the reads -- 16 384 bases per
// workgroup, a lane takes 64 consecutive bases, as decoy_screen_kernel does --, so 150-base reads and 50 kb reads run the same code.  The
// bases come 16 at a time in adapter_points_kernel's common form from either input form (load16_common, load16.h).  Per word: the word
// shifted down by one base with the next word's first base on top, an XOR, a fold of the two bit planes; the same shift on the mask of
// unknown bases; a pair differs iff exactly one of its bases is unknown, or neither is and the letters differ.  Four words make one 64-bit
// mask, bit j: the pair (p + j, p + j + 1) differs.  The pair across a word, a 16-byte group, a lane and a tile boundary is an ordinary bit
// of that mask: its second base is the fifth word's first.
//
// The lane then follows the reads under its 64 bases (first_at_least for the tile's first and last read, read_holding for the lane's, then
// a walk bounded by the tile's last read): read r gets the popcount of the bits from its first base under the lane up to, and without, its
// LAST base -- the pair (last base of r, first base of r + 1) is never counted --, one atomicAdd per read the lane touched.  Integer adds
// commute: D is bit-exact whatever the launch geometry.  Nothing is indexed out of bounds whatever `offsets` holds.
#include "load16.h"
#include "search.h"

namespace drprg {
namespace dev {

constexpr int CX_THREADS = 256;
constexpr uint32_t CX_LANE_BASES = 64;
constexpr uint32_t CX_TILE = CX_THREADS * CX_LANE_BASES; // 16384 bases per workgroup

uint32_t read_complexity_tiles(uint64_t n_bases) { return (uint32_t)((n_bases + CX_TILE - 1) / CX_TILE); }

// the even bits of m, gathered into the low 16
__device__ inline uint32_t cx_even_bits(uint32_t m)
{
    m &= 0x55555555u;
    m = (m | (m >> 1)) & 0x33333333u;
    m = (m | (m >> 2)) & 0x0F0F0F0Fu;
    m = (m | (m >> 4)) & 0x00FF00FFu;
    m = (m | (m >> 8)) & 0x0000FFFFu;
    return m;
}

// bits lo .. hi - 1 (0 <= lo < hi <= 64)
__device__ inline uint64_t cx_bits(uint32_t lo, uint32_t hi) { return (hi >= 64u ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull); }

__global__ __launch_bounds__(CX_THREADS) void read_diff_kernel(ComplexityArgs a)
{
    __shared__ uint64_t s_read[2];
    const uint64_t tile = (uint64_t)blockIdx.x * CX_TILE;
    if (tile >= a.n_bases) return; // (uniform)
    const uint64_t tile_end = a.n_bases - tile > CX_TILE ? tile + CX_TILE : a.n_bases;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 128) { // (two whole waves) the reads that hold the tile's first and last base, as decoy_screen_kernel finds them
        const uint64_t at = threadIdx.x < 64 ? tile : tile_end - 1;
        const uint64_t i = first_at_least(a.offsets, a.n_reads, at + 1, lane);
        if (lane == 0) s_read[threadIdx.x >> 6] = i ? i - 1 : 0;
    }
    __syncthreads();
    const uint64_t first = s_read[0], last = s_read[1] < a.n_reads ? s_read[1] : a.n_reads - 1;
    const uint64_t p = tile + (uint64_t)threadIdx.x * CX_LANE_BASES;
    if (p >= tile_end || first > last) return;
    const uint32_t nst = (uint32_t)(tile_end - p < CX_LANE_BASES ? tile_end - p : CX_LANE_BASES);
    const bool aligned = (reinterpret_cast<uintptr_t>(a.text) & 15u) == 0;
    uint64_t differ = 0;
    uint32_t code, nm;
    load16_common(a.text, a.words, a.nbits, a.n_bases, aligned, p, code, nm);
#pragma unroll
    for (uint32_t w = 0; w < CX_LANE_BASES / 16; ++w) {
        if (16u * w >= nst) break;
        uint32_t ncode, nnm; // the next word: behind the buffer sixteen unknown bases, whose pairs lie behind every read
        load16_common(a.text, a.words, a.nbits, a.n_bases, aligned, p + 16ull * (w + 1), ncode, nnm);
        const uint32_t up = (code >> 2) | (ncode << 30), x = code ^ up;
        const uint32_t u = nm & 0xFFFFu, un = (u >> 1) | ((nnm & 1u) << 15);
        const uint32_t d = ((u ^ un) | (~(u | un) & cx_even_bits(x | (x >> 1)))) & 0xFFFFu;
        differ |= (uint64_t)d << (16u * w);
        code = ncode;
        nm = nnm;
    }
    const uint64_t pend = p + nst;
    uint64_t r = read_holding(a.offsets, first, last, p), pos = p; // r in [first, last]: below n_reads
    for (;;) {
        const uint64_t e = a.offsets[r + 1];
        if (e > pos && a.offsets[r] <= pos) { // read r holds the bases pos .. min(e, pend) - 1 under this lane; its last base starts no pair
            const uint64_t hi = e - 1 < pend ? e - 1 : pend;
            if (hi > pos) {
                const uint32_t cnt = (uint32_t)__popcll(differ & cx_bits((uint32_t)(pos - p), (uint32_t)(hi - p)));
                if (cnt) atomicAdd(&a.diff[r], cnt);
            }
            pos = e;
        }
        if (pos >= pend || r >= last) break;
        ++r;
    }
}

// the verdict alone (drprg_hip_complexity_device): one thread per read
__global__ __launch_bounds__(CX_THREADS) void complexity_verdict_kernel(ComplexityArgs a, uint32_t percent, uint8_t* __restrict__ flag,
    unsigned long long* __restrict__ work, uint32_t* __restrict__ err)
{
    __shared__ unsigned long long s_n[2];
    if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * CX_THREADS + threadIdx.x;
    if (i == 0 && a.offsets[0] != 0) *err = 1;
    if (i == a.n_reads && a.offsets[i] != a.n_bases) *err = 1;
    if (i < a.n_reads) {
        const uint64_t s = a.offsets[i], e = a.offsets[i + 1];
        uint64_t len = 0;
        if (e < s || e > a.n_bases || e - s >= CX_MAX_READ) *err = 1;
        else len = e - s;
        const bool drop = cx_drops(a.diff[i], len, percent);
        flag[i] = drop ? 0 : 1;
        if (drop) {
            atomicAdd(&s_n[0], 1ull);
            atomicAdd(&s_n[1], (unsigned long long)len);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_n[threadIdx.x]) atomicAdd(&work[threadIdx.x], s_n[threadIdx.x]);
}

static bool complexity_args_ok(const ComplexityArgs& a)
{
    return a.n_reads && a.n_reads <= MAX_BATCH_READS && a.offsets && a.diff && (!a.n_bases || a.text || a.words);
}

hipError_t launch_read_diff(const ComplexityArgs& a, hipStream_t stream, KernelTimer timer)
{
    if (!complexity_args_ok(a)) return hipErrorInvalidValue;
    HIP_TRY(hipMemsetAsync(a.diff, 0, a.n_reads * sizeof(uint32_t), stream));
    const uint32_t n_tiles = read_complexity_tiles(a.n_bases);
    if (!n_tiles) return hipSuccess;
    launch_timed(timer, read_diff_kernel, dim3(n_tiles), dim3(CX_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_complexity_verdict(const ComplexityArgs& a, uint32_t percent, uint8_t* flag, unsigned long long* work, uint32_t* err, hipStream_t stream)
{
    if (!complexity_args_ok(a) || percent < 1 || percent > 100 || !flag || !work || !err) return hipErrorInvalidValue;
    hipLaunchKernelGGL(complexity_verdict_kernel, dim3((uint32_t)((a.n_reads + 1 + CX_THREADS - 1) / CX_THREADS)), dim3(CX_THREADS), 0, stream, a, percent, flag, work, err);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
