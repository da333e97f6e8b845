// decoy_screen.hip -- the decoy screen (drprg_hip_set_decoy; the rule: include/drprg_hip.h "decoy screen"): a set of
// canonical k-mers in an open-addressing table in HBM, and per read how many of its k-mers are valid (V) and how many are in the set (H).
// Driven by Mapper::set_decoy and Mapper::run_decoy_screen, which own every buffer.
//
// One inner loop (dc_roll) serves the build and the screen, and both input forms of the screen.  The BUFFER is tiled, not the reads --
// 16 384 starts per workgroup, as adapter_points_kernel tiles the bases --, so 150-base reads and 50 kb reads run the same code.  A lane
// takes a run of 64 consecutive starts and the K - 1 bases behind them, 16 bases at a time in adapter_points_kernel's common form: a word of
// 2-bit letters (A0 C1 T2 G3, the packed batch's own word; text: ad_text16 of one 16-byte load) and a 16-bit mask of the bases that are not
// ACGT (text: from the bytes; packed: the bitmap launch_mark_npos makes of the position list).  It rolls the forward and the
// reverse-complement code in two 64-bit registers (the rule's letters, A0 C1 G2 T3, are letter ^ letter >> 1) with the length of the
// run of ACGT bases that ends at the newest base: a window is all ACGT iff that run is at least K.  A word whose first base is not below
// n_bases is not loaded and reads as sixteen bases that are not ACGT.
//
// The screen follows the read under its starts (first_at_least for the tile's first and last read, read_holding for the lane's, then a
// walk bounded by the tile's last read): a window counts iff it ends inside the read its start lies in.  V and H stay in registers while
// the start stays in one read and go out with one atomicAdd each per read the lane touched, so a read that crosses lane, wave and tile
// edges needs no special case and the sums are order-free.  One 8-byte probe per valid window, linear and wrapping: at most half of the
// slots are taken, and the loop is bounded by the table's size whatever it holds.
//
// The build inserts with a 64-bit compare-and-swap: the slot a k-mer ends in depends on who came first, membership does not.
#include "load16.h"
#include "search.h"

namespace drprg {
namespace dev {

constexpr int DC_THREADS = 256;
constexpr uint32_t DC_LANE_STARTS = 64;
constexpr uint32_t DC_TILE = DC_THREADS * DC_LANE_STARTS; // 16384 starts per workgroup

uint32_t decoy_screen_tiles(uint64_t n_bases) { return (uint32_t)((n_bases + DC_TILE - 1) / DC_TILE); }

// The starts p .. p + nst - 1 (p a multiple of 16, 1 <= nst <= DC_LANE_STARTS): visit(j, canon) for every j < nst whose window [p + j,
// p + j + k) is all ACGT and lies below n_bases of the loader, in ascending order; canon: the window's canonical k-mer.
template <typename Visit>
__device__ inline void dc_roll(const DecoyScreenArgs& a, bool aligned, uint64_t p, uint32_t nst, uint32_t k, Visit&& visit)
{
    const uint64_t mask = dc_mask(k);
    const uint32_t top = 2u * (k - 1u), n_take = nst + k - 1u; // the bases the starts' windows hold
    uint64_t fwd = 0, rev = 0;
    uint32_t run = 0;
    for (uint32_t w = 0; 16u * w < n_take; ++w) {
        uint32_t code, nm;
        load16_common(a.text, a.words, a.nbits, a.n_bases, aligned, p + 16ull * w, code, nm);
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t l = (code >> (2u * j)) & 3u, c = l ^ (l >> 1);
            fwd = ((fwd << 2) | c) & mask;
            rev = (rev >> 2) | ((uint64_t)(3u - c) << top);
            run = (nm >> j) & 1u ? 0u : run + 1u;
            const uint32_t at = 16u * w + j; // the newest base, counted from p: the last base of the window that starts at at - (k - 1)
            if (at + 1u >= k && at + 1u - k < nst && run >= k) visit(at + 1u - k, fwd < rev ? fwd : rev);
        }
    }
}

// true: `key` is in the table
__device__ inline bool dc_find(const DecoySet& d, uint64_t key)
{
    const uint64_t smask = d.n_slots - 1;
    uint64_t sl = dc_slot(key, smask);
    for (uint64_t i = 0; i < d.n_slots; ++i) { // (ends at the first empty slot: at most half are taken)
        const uint64_t v = d.table[sl];
        if (v == key) return true;
        if (v == DC_EMPTY) return false;
        sl = (sl + 1) & smask;
    }
    return false;
}

__global__ __launch_bounds__(DC_THREADS) void decoy_build_kernel(DecoyScreenArgs a, uint32_t k, unsigned long long* __restrict__ table, uint64_t n_slots,
    unsigned long long* __restrict__ distinct)
{
    const uint64_t p = ((uint64_t)blockIdx.x * DC_THREADS + threadIdx.x) * DC_LANE_STARTS;
    if (p >= a.n_bases) return;
    const uint32_t nst = (uint32_t)(a.n_bases - p < DC_LANE_STARTS ? a.n_bases - p : DC_LANE_STARTS);
    const uint64_t smask = n_slots - 1;
    uint32_t fresh = 0;
    dc_roll(a, true, p, nst, k, [&](uint32_t, uint64_t key) {
        uint64_t sl = dc_slot(key, smask);
        for (uint64_t i = 0; i < n_slots; ++i) {
            const unsigned long long was = atomicCAS(&table[sl], (unsigned long long)DC_EMPTY, (unsigned long long)key);
            if (was == DC_EMPTY) {
                ++fresh;
                return;
            }
            if (was == key) return;
            sl = (sl + 1) & smask;
        }
    });
    if (fresh) atomicAdd(distinct, (unsigned long long)fresh);
}

__global__ __launch_bounds__(DC_THREADS) void decoy_lookup_kernel(DecoySet d, const unsigned long long* __restrict__ kmers, uint64_t n, uint8_t* __restrict__ found)
{
    const uint64_t i = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    if (i < n) found[i] = dc_find(d, kmers[i]) ? 1 : 0;
}

__global__ __launch_bounds__(DC_THREADS) void decoy_screen_kernel(DecoyScreenArgs a, DecoySet d)
{
    __shared__ uint64_t s_read[2];
    const uint64_t tile = (uint64_t)blockIdx.x * DC_TILE;
    if (tile >= a.n_bases) return; // (uniform)
    const uint64_t tile_end = a.n_bases - tile > DC_TILE ? tile + DC_TILE : a.n_bases;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 128) { // (two whole waves) the reads that hold the tile's first and last base, as adapter_points_kernel finds them
        const uint64_t at = threadIdx.x < 64 ? tile : tile_end - 1;
        const uint64_t i = first_at_least(a.offsets, a.n_reads, at + 1, lane);
        if (lane == 0) s_read[threadIdx.x >> 6] = i ? i - 1 : 0;
    }
    __syncthreads();
    const uint64_t first = s_read[0], last = s_read[1] < a.n_reads ? s_read[1] : a.n_reads - 1;
    const uint64_t p = tile + (uint64_t)threadIdx.x * DC_LANE_STARTS;
    if (p >= tile_end || first > last) return;
    const uint32_t nst = (uint32_t)(tile_end - p < DC_LANE_STARTS ? tile_end - p : DC_LANE_STARTS);
    const bool aligned = (reinterpret_cast<uintptr_t>(a.text) & 15u) == 0;
    uint64_t r = read_holding(a.offsets, first, last, p); // in [first, last]: below n_reads
    uint64_t end = a.offsets[r + 1];
    uint32_t V = 0, H = 0;
    auto flush = [&]() {
        if (V) atomicAdd(&a.valid[r], V);
        if (H) atomicAdd(&a.hits[r], H);
        V = H = 0;
    };
    dc_roll(a, aligned, p, nst, d.k, [&](uint32_t j, uint64_t key) {
        const uint64_t s = p + j;
        if (s >= end && r < last) { // the start has left read r: its counts go out, and the read under the start is found by walking
            flush();
            do end = a.offsets[++r + 1];
            while (s >= end && r < last);
        }
        if (s + d.k > end || end > a.n_bases) return; // the window runs past its read's end: no window of the rule
        ++V;
        if (dc_find(d, key)) ++H;
    });
    flush();
}

// the verdict alone (drprg_hip_decoy_screen_device): one thread per read
__global__ __launch_bounds__(DC_THREADS) void decoy_verdict_kernel(DecoyScreenArgs a, DecoySet d, uint8_t* __restrict__ flag, unsigned long long* __restrict__ work,
    uint32_t* __restrict__ err)
{
    __shared__ unsigned long long s_n[4];
    if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    if (i == 0 && a.offsets[0] != 0) *err = 1;
    if (i == a.n_reads && a.offsets[i] != a.n_bases) *err = 1;
    if (i < a.n_reads) {
        const uint64_t s = a.offsets[i], e = a.offsets[i + 1];
        if (e < s || e > a.n_bases) *err = 1;
        const uint32_t V = a.valid[i], H = a.hits[i];
        const bool drop = dc_drops(V, H, d.frac_milli, d.min_kmers);
        flag[i] = drop ? 0 : 1;
        if (drop) {
            atomicAdd(&s_n[0], 1ull);
            if (e >= s) atomicAdd(&s_n[1], (unsigned long long)(e - s));
        }
        if (V) atomicAdd(&s_n[2], (unsigned long long)V);
        if (H) atomicAdd(&s_n[3], (unsigned long long)H);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_n[threadIdx.x]) atomicAdd(&work[threadIdx.x], s_n[threadIdx.x]);
}

static bool decoy_set_ok(const DecoySet& d)
{
    return d.table && d.k >= DC_MIN_K && d.k <= DC_MAX_K && d.n_slots >= DC_MIN_SLOTS && (d.n_slots & (d.n_slots - 1)) == 0;
}

hipError_t launch_decoy_build(const uint8_t* text, uint64_t n_text, uint32_t k, unsigned long long* table, uint64_t n_slots, unsigned long long* distinct,
    hipStream_t stream)
{
    if (!text || !n_text || !decoy_set_ok(DecoySet { table, n_slots, k, 1, 1 }) || !distinct || (reinterpret_cast<uintptr_t>(text) & 15u)) return hipErrorInvalidValue;
    HIP_TRY(hipMemsetAsync(table, 0xFF, n_slots * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(distinct, 0, sizeof(unsigned long long), stream));
    const DecoyScreenArgs a { text, nullptr, nullptr, nullptr, 0, n_text, nullptr, nullptr };
    hipLaunchKernelGGL(decoy_build_kernel, dim3(decoy_screen_tiles(n_text)), dim3(DC_THREADS), 0, stream, a, k, table, n_slots, distinct);
    return hipGetLastError();
}

hipError_t launch_decoy_lookup(const DecoySet& d, const unsigned long long* kmers, uint64_t n, uint8_t* found, hipStream_t stream)
{
    if (!decoy_set_ok(d) || n > 0xFFFFFFFFull * DC_THREADS) return hipErrorInvalidValue;
    if (!n) return hipSuccess;
    if (!kmers || !found) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoy_lookup_kernel, dim3((uint32_t)((n + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, stream, d, kmers, n, found);
    return hipGetLastError();
}

static bool decoy_args_ok(const DecoyScreenArgs& a)
{
    return a.n_reads && a.n_reads <= MAX_BATCH_READS && a.offsets && a.valid && a.hits && (!a.n_bases || a.text || a.words);
}

hipError_t launch_decoy_screen(const DecoyScreenArgs& a, const DecoySet& d, hipStream_t stream, KernelTimer timer)
{
    if (!decoy_set_ok(d) || !decoy_args_ok(a)) return hipErrorInvalidValue;
    const uint32_t n_tiles = decoy_screen_tiles(a.n_bases);
    if (!n_tiles) return hipSuccess;
    launch_timed(timer, decoy_screen_kernel, dim3(n_tiles), dim3(DC_THREADS), 0, stream, a, d);
    return hipGetLastError();
}

hipError_t launch_decoy_verdict(const DecoyScreenArgs& a, const DecoySet& d, uint8_t* flag, unsigned long long* work, uint32_t* err, hipStream_t stream)
{
    if (!decoy_args_ok(a) || !flag || !work || !err) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoy_verdict_kernel, dim3((uint32_t)((a.n_reads + 1 + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, stream, a, d, flag, work, err);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
