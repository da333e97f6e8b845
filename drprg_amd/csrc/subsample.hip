// subsample.hip -- a resident sample cut to a target depth at random (drprg_hip_subsample; the rule: include/drprg_hip.h "random
// subsample").  Two halves, both driven by Mapper::subsample_kept, which owns every buffer named here.
//
// Selection.  Read i of the sample (numbered through the resident blocks) gets key(i) = splitmix64(seed + GOLDEN * (i + 1)); the reads are
// ordered by (key, i) with the radix sort the hit list uses (no two reads share a key), their lengths are gathered in that order and summed by a u64 inclusive
// scan, one wave finds the first sum that reaches the target (first_at_least, search.h) and every read whose (key, i) is not above that
// read's is kept: one byte per read.  Two exclusive scans over the flags (kept reads before i, kept bases before i) then give every kept
// read its number and its first base in the new set.  Streams of 4 to 16 bytes per read; nothing here touches a base.
//
// Compaction.  Per resident block: the new offsets and a table of where each kept read starts in the old block, then
//   packed blocks: one workgroup per 16 384 output bases, a lane makes four whole output words (a word two reads share has one writer, no
//     atomics); its first read comes from a binary search of the new offsets between the workgroup's first and last read, further reads by
//     walking; a word inside one read is a funnel shift of the one or two source words at the read's source phase, a word that crosses a
//     read boundary is stitched base by base (subsample_word.h).  The listed non-ACGT positions inside kept reads move with them and stay
//     ascending without a sort: per-workgroup counts, one scan, a second launch (as bam_pack.hip).
//   ASCII blocks: gather_reads_kernel (anchor_scan.hip) from a table the same kernel fills.
// Expected to be bound by the HBM reads of the kept bases (n / 4 bytes in and out, packed); UNMEASURED.
// Every index that comes from device data (offsets of the old block, the scans) is compared with the size of what it indexes before it is
// used; a mismatch sets the error word the host looks at and writes nothing.
#include "search.h"
#include "subsample_word.h"
#include <rocprim/device/device_scan.hpp>

namespace drprg {
namespace dev {

constexpr int SS_THREADS = 256;
constexpr int SS_LANE_WORDS = 4;                                 // one 16-byte store per lane
constexpr uint32_t SS_CHUNK_WORDS = SS_THREADS * SS_LANE_WORDS;  // 16384 bases per workgroup
constexpr uint64_t SS_GOLDEN = 0x9E3779B97F4A7C15ull;

DRPRG_HD inline uint64_t ss_key(uint64_t seed, uint64_t i)
{
    uint64_t z = seed + SS_GOLDEN * (i + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

uint32_t subsample_chunks(uint64_t n_bases) { return (uint32_t)((((n_bases + 15) >> 4) + SS_CHUNK_WORDS - 1) / SS_CHUNK_WORDS); }
uint32_t subsample_npos_chunks(uint64_t n_npos) { return (uint32_t)((n_npos + SS_THREADS - 1) / SS_THREADS); }

// ---- selection ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_THREADS) void ss_keys_kernel(uint64_t seed, uint64_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ idx)
{
    const uint64_t i = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (i >= n) return;
    key[i] = ss_key(seed, i);
    idx[i] = (uint32_t)i;
}

// len[first + j] = length of read j of one resident block (len: n entries, the block's reads lie inside: first + n_reads <= n)
__global__ __launch_bounds__(SS_THREADS) void ss_lengths_kernel(const uint64_t* __restrict__ offsets, uint64_t n_reads, uint64_t first, uint64_t n,
    uint64_t* __restrict__ len)
{
    const uint64_t j = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (j >= n_reads || first + j >= n) return;
    const uint64_t a = offsets[j], b = offsets[j + 1];
    len[first + j] = b >= a ? b - a : 0;
}

__global__ __launch_bounds__(SS_THREADS) void ss_gather_lengths_kernel(const uint64_t* __restrict__ len, const uint32_t* __restrict__ order, uint64_t n,
    uint64_t* __restrict__ out)
{
    const uint64_t p = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = order[p];
    out[p] = i < n ? len[i] : 0;
}

// cut[0] = key, cut[1] = number of the read at which the running sum of lengths (csum, key order) first reaches target -- the last read
// in key order if it never does.  One wave; n >= 1.
__global__ __launch_bounds__(64) void ss_cut_kernel(const uint64_t* __restrict__ csum, const uint64_t* __restrict__ key_sorted,
    const uint32_t* __restrict__ order, uint64_t n, uint64_t target, unsigned long long* __restrict__ cut)
{
    uint64_t p = first_at_least(csum, n, target, (int)threadIdx.x);
    if (p >= n) p = n - 1;
    if (threadIdx.x == 0) {
        cut[0] = key_sorted[p];
        cut[1] = order[p];
    }
}

// flag[i] = (key(i), i) <= (cut[0], cut[1]); flag32[i] and klen[i] = the same as a word, and the read's length if it is kept: what the
// two exclusive scans read (entry n of both: 0)
__global__ __launch_bounds__(SS_THREADS) void ss_flags_kernel(uint64_t seed, uint64_t n, const unsigned long long* __restrict__ cut,
    const uint64_t* __restrict__ len, uint8_t* __restrict__ flag, uint32_t* __restrict__ flag32, uint64_t* __restrict__ klen)
{
    const uint64_t i = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        flag32[i] = 0;
        klen[i] = 0;
        return;
    }
    const uint64_t k = ss_key(seed, i), kc = cut[0], ic = cut[1];
    const bool keep = k < kc || (k == kc && i <= ic);
    const uint64_t l = len[i]; // (read before klen[i] is written: the two may be one array)
    flag[i] = keep ? 1 : 0;
    flag32[i] = keep ? 1u : 0u;
    klen[i] = keep ? l : 0;
}

// out[2 b] = rank[first[b]], out[2 b + 1] = boff[first[b]] for the n_bounds block boundaries (first[b] <= n: the scans hold n + 1 entries)
__global__ __launch_bounds__(SS_THREADS) void ss_bounds_kernel(const uint64_t* __restrict__ first, uint32_t n_bounds, uint64_t n, const uint32_t* __restrict__ rank,
    const uint64_t* __restrict__ boff, unsigned long long* __restrict__ out)
{
    const uint32_t b = blockIdx.x * SS_THREADS + threadIdx.x;
    if (b >= n_bounds) return;
    const uint64_t f = first[b] <= n ? first[b] : n;
    out[2 * b] = rank[f];
    out[2 * b + 1] = boff[f];
}

hipError_t launch_subsample_lengths(const uint64_t* offsets, uint64_t n_reads, uint64_t first, uint64_t n, uint64_t* len, hipStream_t stream)
{
    if (!n_reads) return hipSuccess;
    hipLaunchKernelGGL(ss_lengths_kernel, dim3((uint32_t)((n_reads + SS_THREADS - 1) / SS_THREADS)), dim3(SS_THREADS), 0, stream, offsets, n_reads, first, n, len);
    return hipGetLastError();
}

size_t subsample_scan_temp_bytes(uint64_t n)
{
    size_t a = 0, b = 0;
    (void)rocprim::inclusive_scan(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n + 1, rocprim::plus<uint64_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), (hipStream_t)0);
    const size_t c = sort_temp_bytes((uint32_t)n);
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

hipError_t launch_subsample_select(const SubsampleSelect& s, hipStream_t stream)
{
    const uint64_t n = s.n;
    if (!n || n >= (1ull << 32)) return hipErrorInvalidValue;
    size_t temp_bytes = s.temp_bytes; // (rocPRIM takes it by reference)
    const dim3 grid((uint32_t)((n + SS_THREADS - 1) / SS_THREADS)), grid1((uint32_t)((n + 1 + SS_THREADS - 1) / SS_THREADS)), block(SS_THREADS);
    // (key, i) ascending.  The keys of different reads differ -- the finaliser is a bijection and seed + GOLDEN * (i + 1) takes every value
    // once, GOLDEN being odd --, so the order by key alone is the order by (key, i)
    hipLaunchKernelGGL(ss_keys_kernel, grid, block, 0, stream, s.seed, n, s.key, s.idx);
    HIP_TRY(hipGetLastError());
    HIP_TRY(sort_hits(s.temp, s.temp_bytes, s.key, s.key_sorted, s.idx, s.idx_sorted, (uint32_t)n, stream));
    // lengths in key order into s.key (its keys are in key_sorted by now), their running sum into csum
    hipLaunchKernelGGL(ss_gather_lengths_kernel, grid, block, 0, stream, (const uint64_t*)s.len, (const uint32_t*)s.idx_sorted, n, s.key);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::inclusive_scan(s.temp, temp_bytes, s.key, s.csum, (size_t)n, rocprim::plus<uint64_t>(), stream));
    hipLaunchKernelGGL(ss_cut_kernel, dim3(1), dim3(64), 0, stream, (const uint64_t*)s.csum, (const uint64_t*)s.key_sorted, (const uint32_t*)s.idx_sorted, n, s.target, s.cut);
    HIP_TRY(hipGetLastError());
    // flags; the words the scans read go into idx and key (n + 1 entries each), the scans into rank and boff
    hipLaunchKernelGGL(ss_flags_kernel, grid1, block, 0, stream, s.seed, n, (const unsigned long long*)s.cut, (const uint64_t*)s.len, s.flag, s.idx, s.key);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::exclusive_scan(s.temp, temp_bytes, s.idx, s.rank, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), stream));
    HIP_TRY(rocprim::exclusive_scan(s.temp, temp_bytes, s.key, s.boff, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), stream));
    return hipSuccess;
}

hipError_t launch_subsample_bounds(const uint64_t* first, uint32_t n_bounds, uint64_t n, const uint32_t* rank, const uint64_t* boff, unsigned long long* out,
    hipStream_t stream)
{
    if (!n_bounds) return hipSuccess;
    hipLaunchKernelGGL(ss_bounds_kernel, dim3((n_bounds + SS_THREADS - 1) / SS_THREADS), dim3(SS_THREADS), 0, stream, first, n_bounds, n, rank, boff, out);
    return hipGetLastError();
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------------
// The kept reads of one block: new_offsets[r] and where read r starts in the old block -- src_start[r] (packed) or a GatherEntry (ASCII).
// One thread per old read; thread 0 closes the offsets.  *err is set when the scans and the block's offsets do not fit each other.
__global__ __launch_bounds__(SS_THREADS) void ss_tables_kernel(SubsampleBlock b, uint64_t* __restrict__ new_offsets, uint64_t* __restrict__ src_start,
    GatherEntry* __restrict__ table, uint32_t* __restrict__ err)
{
    const uint64_t j = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x;
    const uint32_t rank0 = b.rank[b.first];
    const uint64_t boff0 = b.boff[b.first];
    if (j == 0) {
        const uint64_t total = b.boff[b.first + b.n_reads] - boff0;
        if (b.rank[b.first + b.n_reads] - rank0 != b.new_reads || total != b.new_bases) *err = 1;
        else new_offsets[b.new_reads] = total;
    }
    if (j >= b.n_reads || !b.flag[b.first + j]) return;
    const uint64_t r = b.rank[b.first + j] - rank0, at = b.boff[b.first + j] - boff0;
    const uint64_t s = b.offsets[j], e = b.offsets[j + 1];
    if (r >= b.new_reads || e < s || e > b.n_bases || at + (e - s) > b.new_bases || e - s > 0xFFFFFFFFull) {
        *err = 1;
        return;
    }
    new_offsets[r] = at;
    if (src_start) src_start[r] = s;
    if (table) {
        GatherEntry g;
        g.src = b.bases + s;
        g.dst = at;
        g.len = (uint32_t)(e - s);
        g.pad = 0;
        table[r] = g;
    }
}

__global__ __launch_bounds__(SS_THREADS) void ss_pack_kernel(CompactBatch b, uint32_t* __restrict__ words, uint32_t* __restrict__ err)
{
    __shared__ uint64_t s_read[2];
    const uint64_t n_words = (b.n_bases + 15) >> 4;
    const uint64_t chunk_word = (uint64_t)blockIdx.x * SS_CHUNK_WORDS;
    if (threadIdx.x == 0 || threadIdx.x == 64) {
        const uint64_t chunk_end = chunk_word + SS_CHUNK_WORDS < n_words ? (chunk_word + SS_CHUNK_WORDS) << 4 : b.n_bases;
        s_read[threadIdx.x >> 6] = read_holding(b.new_offsets, 0, b.n_reads - 1, threadIdx.x == 0 ? chunk_word << 4 : chunk_end - 1);
    }
    __syncthreads();
    const uint64_t w0 = chunk_word + (uint64_t)threadIdx.x * SS_LANE_WORDS;
    if (w0 >= n_words) return;
    uint64_t r = read_holding(b.new_offsets, s_read[0], s_read[1], w0 << 4);
    uint32_t w[SS_LANE_WORDS];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < SS_LANE_WORDS; ++j) w[j] = w0 + j < n_words ? ss_word(b, (w0 + j) << 4, r, bad) : 0;
    if (bad) *err = 1;
    if (w0 + SS_LANE_WORDS <= n_words && (reinterpret_cast<uintptr_t>(words) & 15u) == 0)
        *reinterpret_cast<uint4*>(words + w0) = make_uint4(w[0], w[1], w[2], w[3]);
    else
        for (int j = 0; j < SS_LANE_WORDS; ++j)
            if (w0 + j < n_words) words[w0 + j] = w[j];
}

// The block's listed positions that lie inside kept reads, at their new places.  EMIT == false: chunk_count[workgroup] = how many of its
// SS_THREADS entries are kept.  EMIT == true: they are written, ascending, from chunk_prefix[workgroup] on (below out_cap).
template <bool EMIT>
__global__ __launch_bounds__(SS_THREADS) void ss_npos_kernel(SubsampleBlock b, const uint64_t* __restrict__ npos, uint64_t n_npos, uint32_t* __restrict__ chunk_count,
    const uint32_t* __restrict__ chunk_prefix, uint64_t* __restrict__ out, uint64_t out_cap)
{
    __shared__ uint32_t s_w[SS_THREADS / 64 + 1];
    if (EMIT && chunk_prefix[blockIdx.x + 1] == chunk_prefix[blockIdx.x]) return; // (uniform)
    const uint64_t t = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x;
    uint32_t keep = 0;
    uint64_t to = 0;
    if (t < n_npos) {
        const uint64_t q = npos[t];
        if (q < b.n_bases) {
            const uint64_t j = read_holding(b.offsets, 0, b.n_reads - 1, q);
            const uint64_t s = b.offsets[j];
            if (s <= q && q < b.offsets[j + 1] && b.flag[b.first + j]) {
                keep = 1;
                to = (b.boff[b.first + j] - b.boff[b.first]) + (q - s);
            }
        }
    }
    uint32_t total = 0;
    const uint32_t before = block_exclusive_scan<SS_THREADS / 64>(keep, s_w, &total);
    if (!EMIT) {
        if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
        return;
    }
    const uint64_t at = (uint64_t)chunk_prefix[blockIdx.x] + before;
    if (keep && at < out_cap && to < b.new_bases) out[at] = to;
}

hipError_t launch_subsample_tables(const SubsampleBlock& b, uint64_t* new_offsets, uint64_t* src_start, GatherEntry* table, uint32_t* err, hipStream_t stream)
{
    const uint64_t threads = b.n_reads ? b.n_reads : 1;
    hipLaunchKernelGGL(ss_tables_kernel, dim3((uint32_t)((threads + SS_THREADS - 1) / SS_THREADS)), dim3(SS_THREADS), 0, stream, b, new_offsets, src_start, table, err);
    return hipGetLastError();
}

hipError_t launch_subsample_pack(const SubsampleBlock& b, const uint64_t* new_offsets, const uint64_t* src_start, uint32_t* words, uint32_t* err, hipStream_t stream)
{
    const uint32_t n_chunks = subsample_chunks(b.new_bases);
    if (!n_chunks || !b.new_reads) return hipSuccess;
    const CompactBatch c { reinterpret_cast<const uint32_t*>(b.bases), b.n_bases, new_offsets, src_start, b.new_reads, b.new_bases };
    hipLaunchKernelGGL(ss_pack_kernel, dim3(n_chunks), dim3(SS_THREADS), 0, stream, c, words, err);
    return hipGetLastError();
}

hipError_t launch_subsample_npos_count(const SubsampleBlock& b, const uint64_t* npos, uint64_t n_npos, uint32_t* chunk_count, uint32_t* chunk_prefix, void* temp,
    size_t temp_bytes, hipStream_t stream)
{
    const uint32_t n_chunks = subsample_npos_chunks(n_npos);
    if (!n_chunks || !b.n_reads) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ss_npos_kernel<false>, dim3(n_chunks), dim3(SS_THREADS), 0, stream, b, npos, n_npos, chunk_count, (const uint32_t*)nullptr, (uint64_t*)nullptr, 0ull);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(chunk_count + n_chunks, 0, sizeof(uint32_t), stream));
    return exclusive_scan_u32(temp, temp_bytes, chunk_count, chunk_prefix, n_chunks + 1, stream);
}

hipError_t launch_subsample_npos_emit(const SubsampleBlock& b, const uint64_t* npos, uint64_t n_npos, const uint32_t* chunk_prefix, uint64_t* out, uint64_t out_cap,
    hipStream_t stream)
{
    const uint32_t n_chunks = subsample_npos_chunks(n_npos);
    if (!n_chunks || !b.n_reads || !out_cap) return hipSuccess;
    hipLaunchKernelGGL(ss_npos_kernel<true>, dim3(n_chunks), dim3(SS_THREADS), 0, stream, b, npos, n_npos, (uint32_t*)nullptr, chunk_prefix, out, out_cap);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
