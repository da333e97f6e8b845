// adapter_edit.hip -- adapter trimming with indels and at the 5' end (drprg_hip_set_adapters2; the rule: include/drprg_hip.h "adapter
// trimming", the indel rule).  Launched by launch_read_trim (read_trim.hip) in place of adapter_trim.hip's kernels
// when the indel flag is set: the 3' side first, then the 5' side on what the 3' cut left.
//
// adapter_edit_points_kernel<DIR, Word> is a segmented approximate search over the batch's concatenated bases with Myers' bit-vector
// recurrence.  The BUFFER is tiled, not the reads -- 16 384 bases per workgroup --, so 150-base reads and 50 kb reads run the same code.
// A lane owns a stretch of 64 bases and walks it one base a step (ae_scan, adapter_edit.h: host code as well): right to left with the
// reversed adapter for the 3' side, which leaves the score of every START behind each base, left to right with the adapter as given for
// the 5' side, which leaves the score of every END.  The walk begins at most m + L(m) + 2 bases outside the stretch with the column
// D[i] = i, takes that column again at every range end it crosses, and never looks at a base at or behind n_bases; the bases come sixteen
// at a time in adapter_trim.hip's common form, from text (aligned or byte by byte) or from packed words and the bitmap.  The adapters' four
// match masks, their letters, lengths and limits are kernel arguments and ride in scalar registers; a lane holds Pv, Mv and the score
// per adapter (the score of the step before is a temporary of the step), 32-bit words when every adapter has at most 32 letters (Word: chosen by the host, a uniform branch).  Every read gets ONE
// 32-bit word -- the smallest matching start (3', atomicMin) or the largest matching end (5', atomicMax), counted from its range's first
// base -- through a per-workgroup array in LDS indexed by read minus the workgroup's first read (a tile of more than AE_SLOTS reads sends
// the reads beyond the array straight to global memory).  Minimum and maximum commute, and a verdict depends on the bases inside the
// warm-up distance alone: the result is bit-exact whatever the launch geometry.  Every index that comes from device data is bounded
// before it is used.
//
// adapter_edit_apply_kernel<FRONT>: one thread per read -- end = begin + cut (3'), then begin = begin + cut (5'), the new length, and
// the counts; bad offsets are refused as adapter_apply_kernel refuses them.
#include "adapter_edit.h"
#include "search.h"

namespace drprg {
namespace dev {

uint32_t adapter_edit_tiles(uint64_t n_bases) { return (uint32_t)((n_bases + AE_TILE - 1) / AE_TILE); }

struct AeLds {
    uint32_t v[AE_SLOTS];
    uint64_t first;
};

template <int DIR, typename Word>
__global__ __launch_bounds__(AE_THREADS) void adapter_edit_points_kernel(AdapterPoints a, AdapterSet ad, AdapterEq q)
{
    __shared__ AeLds s;
    constexpr uint32_t none = DIR < 0 ? AD_NONE : 0u;
    const uint64_t tile = (uint64_t)blockIdx.x * AE_TILE;
    if (tile >= a.n_bases) return; // (uniform)
    const uint64_t tile_end = a.n_bases - tile > AE_TILE ? tile + AE_TILE : a.n_bases;
    for (uint32_t i = threadIdx.x; i < AE_SLOTS; i += AE_THREADS) s.v[i] = none;
    if (threadIdx.x < 64) { // (one whole wave) the read that holds the tile's first base
        const uint64_t i = first_at_least(a.offsets, a.n_reads, tile + 1, (int)threadIdx.x);
        if (threadIdx.x == 0) s.first = i ? i - 1 : 0;
    }
    __syncthreads();
    const uint64_t first = s.first;
    const uint64_t from = tile + (uint64_t)threadIdx.x * AE_STRETCH;
    if (from < tile_end) {
        const uint64_t to = tile_end - from > AE_STRETCH ? from + AE_STRETCH : tile_end;
        const AeBases bs { a.text, a.words, a.nbits, a.n_bases, (reinterpret_cast<uintptr_t>(a.text) & 15u) == 0 };
        ae_scan<DIR, Word>(bs, a.offsets, a.begin, a.end, a.n_reads, from, to, ad, q, [&](uint64_t read, uint32_t v) {
            if (read >= a.n_reads || read < first) return;
            if (read - first < AE_SLOTS) {
                if (DIR < 0) atomicMin(&s.v[read - first], v);
                else atomicMax(&s.v[read - first], v);
            } else {
                if (DIR < 0) atomicMin(&a.cut[read], v);
                else atomicMax(&a.cut[read], v);
            }
        });
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < AE_SLOTS; i += AE_THREADS) {
        const uint32_t v = s.v[i];
        if (v != none && first + i < a.n_reads) {
            if (DIR < 0) atomicMin(&a.cut[first + i], v);
            else atomicMax(&a.cut[first + i], v);
        }
    }
}

// FRONT == false: end[i] = begin[i] + cut[i] where the 3' side found a match (cut: smallest matching start, or AD_NONE), the counts
// into work[RT_AD_*].  FRONT == true: begin[i] += cut[i] where the 5' side found one (cut: largest matching end, or 0), the counts into
// work[RT_FA_*].  klen[i] (may be null) = the new length.  work[RT_OFFSETS] is set when a range does not lie inside its read or the
// offsets do not ascend to n_bases.
template <bool FRONT>
__global__ __launch_bounds__(AE_THREADS) void adapter_edit_apply_kernel(AdapterPoints a, uint64_t* __restrict__ begin, uint64_t* __restrict__ end,
    uint64_t* __restrict__ klen, unsigned long long* __restrict__ work)
{
    __shared__ unsigned long long s_n[4];
    if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * AE_THREADS + threadIdx.x;
    if (i == a.n_reads && a.offsets[i] != a.n_bases) work[RT_OFFSETS] = 1;
    if (i < a.n_reads) {
        const uint64_t s = a.offsets[i], e = a.offsets[i + 1], x = begin[i], y = end[i];
        if (e < s || e > a.n_bases || e - s >= AD_MAX_READ || x > y || y > e - s) work[RT_OFFSETS] = 1;
        else {
            const uint64_t n = y - x;
            const uint32_t cut = a.cut[i];
            if (n) atomicAdd(&s_n[0], (unsigned long long)n);
            if (!FRONT && cut != AD_NONE && cut < n) {
                end[i] = x + cut;
                if (klen) klen[i] = cut;
                atomicAdd(&s_n[1], 1ull);
                atomicAdd(&s_n[2], (unsigned long long)(n - cut));
                if (cut == 0) atomicAdd(&s_n[3], 1ull);
            }
            if (FRONT && cut != 0 && cut <= n) {
                begin[i] = x + cut;
                if (klen) klen[i] = n - cut;
                atomicAdd(&s_n[1], 1ull);
                atomicAdd(&s_n[2], (unsigned long long)cut);
                if (cut == n) atomicAdd(&s_n[3], 1ull);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_n[threadIdx.x]) atomicAdd(&work[(FRONT ? RT_FA_BASES_SEEN : RT_AD_BASES_SEEN) + threadIdx.x], s_n[threadIdx.x]);
}

static bool ae_set_ok(const AdapterSet& ad)
{
    if (ad.n > AD_MAX_ADAPTERS || (ad.n && (ad.max_len < 1 || ad.max_len > AD_MAX_LEN || ad.error_milli > AD_MAX_ERROR_MILLI || ad.min_overlap < 1))) return false;
    for (uint32_t k = 0; k < ad.n; ++k)
        if (ad.len[k] < 1 || ad.len[k] > ad.max_len) return false;
    return true;
}

template <int DIR>
static hipError_t ae_side(const AdapterPoints& a, const AdapterSet& ad, const AdapterEq& q, uint64_t* begin, uint64_t* end, uint64_t* klen, unsigned long long* work,
    hipStream_t stream, KernelTimer timer)
{
    HIP_TRY(hipMemsetAsync(a.cut, DIR < 0 ? 0xFF : 0, a.n_reads * sizeof(uint32_t), stream));
    const uint32_t n_tiles = adapter_edit_tiles(a.n_bases);
    if (n_tiles) {
        if (ad.max_len <= 32u) launch_timed(timer, adapter_edit_points_kernel<DIR, uint32_t>, dim3(n_tiles), dim3(AE_THREADS), 0, stream, a, ad, q);
        else launch_timed(timer, adapter_edit_points_kernel<DIR, uint64_t>, dim3(n_tiles), dim3(AE_THREADS), 0, stream, a, ad, q);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(adapter_edit_apply_kernel<(DIR > 0)>, dim3((uint32_t)((a.n_reads + 1 + AE_THREADS - 1) / AE_THREADS)), dim3(AE_THREADS), 0, stream, a, begin, end,
        klen, work);
    return hipGetLastError();
}

hipError_t launch_adapter_edit(const AdapterPoints& a, const AdapterSet& ad3, const AdapterEq& eq3, const AdapterSet& ad5, const AdapterEq& eq5, uint64_t* begin,
    uint64_t* end, uint64_t* klen, unsigned long long* work, hipStream_t stream, KernelTimer timer3, KernelTimer timer5)
{
    if (!a.n_reads || a.n_reads > MAX_BATCH_READS) return hipErrorInvalidValue;
    if ((!ad3.n && !ad5.n) || !ae_set_ok(ad3) || !ae_set_ok(ad5)) return hipErrorInvalidValue;
    if (!a.cut || !a.offsets || !begin || !end || a.begin != begin || a.end != end || (a.n_bases && !a.text && !a.words)) return hipErrorInvalidValue;
    if (ad3.n) HIP_TRY(ae_side<-1>(a, ad3, eq3, begin, end, klen, work, stream, timer3));
    if (ad5.n) HIP_TRY(ae_side<1>(a, ad5, eq5, begin, end, klen, work, stream, timer5));
    return hipSuccess;
}

} // namespace dev
} // namespace drprg
