// adapter_trim.hip -- adapter trimming (drprg_hip_set_adapters; the rule: include/drprg_hip.h "adapter trimming"):
// where the leftmost match of an adapter starts in every read's range, and the cut.  Launched by launch_read_trim (read_trim.hip) between
// trim_tables_kernel, which leaves every read's range behind the crops and the quality trim, and the scan of the new lengths; the
// compaction that follows is the trim stage's own.
//
// adapter_points_kernel is a segmented leftmost-match search over the batch's concatenated bases.  The BUFFER is tiled, not the reads --
// 16 384 bases per workgroup, as trim_points_kernel tiles the quality bytes --, so 150-base reads and 50 kb reads run the same code.  A lane
// takes 16 starts per round, four rounds: one word of 2-bit letters and a 16-bit mask of the bases that are not ACGT, made of 16 text bytes
// in registers (ad_text16) or loaded as they lie (a packed block's words, and the bitmap launch_mark_npos makes of its position list):
// load16_common, load16.h.
// Behind the load there is one code path.  The up to 63 bases behind a lane's own come by shuffle from the next four lanes, on the last
// lanes of a wave from memory -- never from behind the buffer: a word whose first base is not below n_bases is not loaded, and what a
// window holds behind its read's range is masked off before it is counted (ad_match, adapter_piece.h: host code as well).  Per start and
// adapter: an XOR against the adapter's letters, which ride in scalar registers, a fold of the bit pairs, an OR of the non-ACGT bits, a
// mask to the compared length and a popcount; one 64-bit step up to 32 letters, two up to 64.  A lane takes its starts in order and moves
// its window on by one base each (five funnel shifts by a constant); where every adapter's full length lies in front of a start -- nearly
// everywhere -- the compared length, the masks and the limit are the same in every lane and stay scalar.  The starts are split by read and held
// against each read's range (ad_piece), and every read gets ONE 32-bit word, the smallest matching start counted from its range's first
// base: a wave that lies under one read reduces in registers, whatever is left goes to a per-workgroup array in LDS indexed by read minus
// the workgroup's first read and from there by one atomicMin per read to global memory (a tile of more than AD_SLOTS reads sends the reads
// beyond the array straight there).  A minimum commutes: the result is bit-exact whatever the launch geometry.  Every index that comes from
// device data is bounded before it is used.
//
// adapter_apply_kernel: one thread per read -- end = begin + cut, the new length, and the counts.
#include "adapter_piece.h"
#include "load16.h"
#include "search.h"

namespace drprg {
namespace dev {

constexpr int AD_THREADS = 256;
constexpr int AD_ROUNDS = 4;
constexpr uint32_t AD_TILE = AD_THREADS * AD_ROUNDS * AD_LANE_STARTS; // 16384 bases per workgroup
constexpr uint32_t AD_SLOTS = 1024;                                   // per-workgroup words in LDS: reads first .. first + 1023 of the tile

uint32_t adapter_trim_tiles(uint64_t n_bases) { return (uint32_t)((n_bases + AD_TILE - 1) / AD_TILE); }

struct AdLds {
    uint32_t mn[AD_SLOTS];
    uint64_t read[2];
};

__device__ inline void ad_put(AdLds& s, uint32_t* __restrict__ gcut, uint64_t n_reads, uint64_t first, uint64_t read, uint32_t cut)
{
    if (read >= n_reads || read < first) return;
    if (read - first < AD_SLOTS) atomicMin(&s.mn[read - first], cut);
    else atomicMin(&gcut[read], cut);
}

// (the 16 bases from base p on in the common form: load16_common, load16.h)
__global__ __launch_bounds__(AD_THREADS) void adapter_points_kernel(AdapterPoints a, AdapterSet ad)
{
    __shared__ AdLds s;
    const uint64_t tile = (uint64_t)blockIdx.x * AD_TILE;
    if (tile >= a.n_bases) return; // (uniform)
    const uint64_t tile_end = a.n_bases - tile > AD_TILE ? tile + AD_TILE : a.n_bases;
    for (uint32_t i = threadIdx.x; i < AD_SLOTS; i += AD_THREADS) s.mn[i] = AD_NONE;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 128) { // (two whole waves) the reads that hold the tile's first and last base, as trim_points_kernel finds them
        const uint64_t at = threadIdx.x < 64 ? tile : tile_end - 1;
        const uint64_t i = first_at_least(a.offsets, a.n_reads, at + 1, lane);
        if (lane == 0) s.read[threadIdx.x >> 6] = i ? i - 1 : 0;
    }
    __syncthreads();
    const uint64_t first = s.read[0], last = s.read[1];
    const bool aligned = (reinterpret_cast<uintptr_t>(a.text) & 15u) == 0;
    const uint32_t extra = (ad.max_len + 14u) / 16u; // (uniform) words behind the lane's own that a window can reach into: 0..4
    uint32_t code[AD_ROUNDS], nm[AD_ROUNDS];
#pragma unroll
    for (int round = 0; round < AD_ROUNDS; ++round) {
        const uint64_t p = tile + ((uint64_t)round * AD_THREADS + threadIdx.x) * AD_LANE_STARTS;
        code[round] = 0;
        nm[round] = 0xFFFFu;
        if (p < tile_end) load16_common(a.text, a.words, a.nbits, a.n_bases, aligned, p, code[round], nm[round]);
    }
#pragma unroll
    for (int round = 0; round < AD_ROUNDS; ++round) {
        const uint64_t p = tile + ((uint64_t)round * AD_THREADS + threadIdx.x) * AD_LANE_STARTS;
        const bool live = p < tile_end;
        uint32_t c[AD_LANE_WORDS], n[AD_LANE_WORDS];
        c[0] = code[round];
        n[0] = nm[round];
#pragma unroll
        for (uint32_t k = 1; k < AD_LANE_WORDS; ++k) {
            c[k] = 0;
            n[k] = 0; // (a word no window reaches into: never counted, and it must not look like a base that is not ACGT to the lane's shortcut)
            if (k <= extra) { // (uniform) the next lanes' words; on the wave's last lanes the buffer itself, the next tile's bases included
                c[k] = __shfl_down(code[round], k);
                n[k] = __shfl_down(nm[round], k);
                if (lane + (int)k > 63) {
                    c[k] = 0;
                    n[k] = 0xFFFFu;
                    if (live) load16_common(a.text, a.words, a.nbits, a.n_bases, aligned, p + (uint64_t)k * AD_LANE_STARTS, c[k], n[k]);
                }
            }
        }
        uint32_t key = AD_NONE, cut = AD_NONE;
        if (live) {
            const uint32_t nst = (uint32_t)(tile_end - p < AD_LANE_STARTS ? tile_end - p : AD_LANE_STARTS);
            const AdWindow w = ad_window(c, n);
            uint64_t r = read_holding(a.offsets, first, last, p);
            ad_piece(a.offsets, a.begin, a.end, a.n_reads, a.n_bases, p, nst, w, ad, r, last, [&](uint64_t read, uint32_t at) {
                if (read < first || read - first >= 0xFFFFFFFFull) return;
                if (key == AD_NONE) { // the lane's first read with a match: kept for the wave's reduction
                    key = (uint32_t)(read - first);
                    cut = at;
                } else ad_put(s, a.cut, a.n_reads, first, read, at);
            });
        }
        // One read under every lane of the wave that found a match (every wave inside a long read): the minimum in registers, one lane hands
        // it over.  Otherwise every lane hands over its own.
        uint32_t kmin = key;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_xor(kmin, off);
            kmin = o < kmin ? o : kmin;
        }
        if (kmin == AD_NONE) continue; // (uniform: no lane found a match)
        if (__all(key == kmin || key == AD_NONE)) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = __shfl_xor(cut, off);
                cut = o < cut ? o : cut;
            }
            if (lane == 0) ad_put(s, a.cut, a.n_reads, first, first + kmin, cut);
            continue;
        }
        if (key != AD_NONE) ad_put(s, a.cut, a.n_reads, first, first + key, cut);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < AD_SLOTS; i += AD_THREADS) {
        const uint32_t v = s.mn[i];
        if (v != AD_NONE && first + i < a.n_reads) atomicMin(&a.cut[first + i], v);
    }
}

// end[i] = begin[i] + cut[i] where the points kernel found a match; klen[i] (may be null) = the new length; the counts into
// work[RT_AD_*]; work[RT_OFFSETS] is set when a range does not lie inside its read or the offsets do not ascend to n_bases.
__global__ __launch_bounds__(AD_THREADS) void adapter_apply_kernel(AdapterPoints a, uint64_t* __restrict__ end, uint64_t* __restrict__ klen,
    unsigned long long* __restrict__ work)
{
    __shared__ unsigned long long s_n[4];
    if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * AD_THREADS + threadIdx.x;
    if (i == a.n_reads && a.offsets[i] != a.n_bases) work[RT_OFFSETS] = 1;
    if (i < a.n_reads) {
        const uint64_t s = a.offsets[i], e = a.offsets[i + 1], x = a.begin[i], y = end[i];
        if (e < s || e > a.n_bases || e - s >= AD_MAX_READ || x > y || y > e - s) work[RT_OFFSETS] = 1;
        else {
            const uint64_t n = y - x;
            const uint32_t cut = a.cut[i];
            if (n) atomicAdd(&s_n[0], (unsigned long long)n);
            if (cut != AD_NONE && cut < n) {
                end[i] = x + cut;
                if (klen) klen[i] = cut;
                atomicAdd(&s_n[1], 1ull);
                atomicAdd(&s_n[2], (unsigned long long)(n - cut));
                if (cut == 0) atomicAdd(&s_n[3], 1ull);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_n[threadIdx.x]) atomicAdd(&work[RT_AD_BASES_SEEN + threadIdx.x], s_n[threadIdx.x]);
}

hipError_t launch_adapter_trim(const AdapterPoints& a, const AdapterSet& ad, uint64_t* end, uint64_t* klen, unsigned long long* work, hipStream_t stream,
    KernelTimer timer)
{
    if (!a.n_reads || a.n_reads > MAX_BATCH_READS) return hipErrorInvalidValue;
    if (!ad.n || ad.n > AD_MAX_ADAPTERS || ad.max_len < 1 || ad.max_len > AD_MAX_LEN || ad.error_milli > AD_MAX_ERROR_MILLI || ad.min_overlap < 1)
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < ad.n; ++k)
        if (ad.len[k] < 1 || ad.len[k] > ad.max_len) return hipErrorInvalidValue;
    if (!a.cut || !a.offsets || !a.begin || !end || (a.n_bases && !a.text && !a.words)) return hipErrorInvalidValue;
    HIP_TRY(hipMemsetAsync(a.cut, 0xFF, a.n_reads * sizeof(uint32_t), stream));
    const uint32_t n_tiles = adapter_trim_tiles(a.n_bases);
    if (n_tiles) {
        launch_timed(timer, adapter_points_kernel, dim3(n_tiles), dim3(AD_THREADS), 0, stream, a, ad);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(adapter_apply_kernel, dim3((uint32_t)((a.n_reads + 1 + AD_THREADS - 1) / AD_THREADS)), dim3(AD_THREADS), 0, stream, a, end, klen, work);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
