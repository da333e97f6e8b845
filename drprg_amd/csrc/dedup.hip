// dedup.hip -- exact duplicate reads dropped from the resident sample (drprg_hip_dedup; the rule: include/drprg_hip.h "duplicate reads",
// DESIGN.md section 4).  Driven by Mapper::dedup_kept, which owns every buffer named here; the compaction and the fresh mapping behind the
// flags are the random subsample's (subsample.hip).
//
// Keys.  dedup_keys_kernel is a segmented sum over the packed base stream of one resident block: key(read) = fin(G L) + sum_j fin(x_j + G (j + 1))
// over the read-aligned words x_j (dedup_word.h: host code as well).  The BUFFER is tiled, not the reads -- 65 536 bases = 16 KB of words
// per workgroup, as read_qual_kernel tiles the quality bytes --, so 150-base reads and 50 kb reads run the same code at the same rate.  A lane
// loads 16 bytes (four words, 64 bases) four times, every round a coalesced 4 KB of the workgroup, with the bitmap rows of the listed
// positions beside them (8 bytes; no load at all for a block that lists none); all loads are issued before the first is used.  The word
// behind a lane's four comes from the next lane by a shuffle (lane 63 loads it).  Each of the lane's four 16-base windows handles every
// read-aligned word whose first base lies in it (dd_window): a funnel shift of two adjacent batch words at the read's phase.  A lane adds
// up the terms of one read in registers; the sums of the lanes whose first base lies in one read are added inside the wave (a segmented
// scan by shuffles), the wave's runs and the terms of reads that start inside a lane go
// to a per-workgroup array of 64-bit sums in LDS, and every read the workgroup touched gets ONE 64-bit atomic add to key[read].  Integer
// adds commute: the key is the same bits whatever the launch geometry and the order of the atomics.
// Meant to be bound by reading n_bases / 4 bytes from HBM.  Measured (kernel time, one batch): 0.069 of 8 TB/s on 10 M x 150 bp, 0.10 on
// 2 M x 4 kb; which bound holds is UNMEASURED (no counter run yet).  On a resident sample the kernel runs once per block, and a block of
// 3.9 M bases is 60 workgroups: the 382 launches of 10 M x 150 bp take 13 ms together (DESIGN.md section 6 has the numbers and the remedy).
//
// Order and exact check.  (key & mask(key_bits), i) ascending by the hit list's radix sort; then one thread per sorted entry walks back
// through the entries of its masked key and compares length, then words (dd_read_word), with each: identical to one of them -- dropped.
// Equal keys decide nothing.  One flag byte per read, then the two exclusive scans launch_subsample_select leaves (rank, boff).
//
// Every index that comes from device data (offsets, sorted read numbers) is compared with the size of what it indexes before it is used; a
// mismatch sets the error word the host looks at and writes nothing out of bounds.
#include "search.h"
#include "dedup_word.h"
#include <rocprim/device/device_scan.hpp>

namespace drprg {
namespace dev {

constexpr int DD_THREADS = 256;
constexpr int DD_ROUNDS = 4;
constexpr uint32_t DD_LANE_WORDS = 4;                                           // one 16-byte load per lane and round
constexpr uint32_t DD_TILE_WORDS = DD_THREADS * DD_ROUNDS * DD_LANE_WORDS;      // 4096 words = 65 536 bases per workgroup
constexpr uint32_t DD_SLOTS = 1024;                                             // per-workgroup sums in LDS: reads first .. first + 1023 of the tile

uint32_t dedup_tiles(uint64_t n_bases) { return (uint32_t)((((n_bases + 15) >> 4) + DD_TILE_WORDS - 1) / DD_TILE_WORDS); }

struct DdLds {
    unsigned long long sum[DD_SLOTS];
    uint64_t read[2];
};

__device__ inline void dd_add(DdLds& s, unsigned long long* __restrict__ key, uint64_t n_reads, uint64_t first, uint64_t read, uint64_t v)
{
    if (read >= n_reads || read < first) return;
    if (read - first < DD_SLOTS) atomicAdd(&s.sum[read - first], (unsigned long long)v);
    else atomicAdd(&key[read], (unsigned long long)v);
}

__global__ __launch_bounds__(DD_THREADS) void dedup_keys_kernel(DedupBatch b, unsigned long long* __restrict__ key, uint32_t* __restrict__ err)
{
    __shared__ DdLds s;
    const uint64_t n_words = (b.n_bases + 15) >> 4;
    const uint64_t tile_word = (uint64_t)blockIdx.x * DD_TILE_WORDS;
    if (tile_word >= n_words) return; // (uniform)
    const uint64_t tile = tile_word << 4;
    const uint64_t tile_end = n_words - tile_word > DD_TILE_WORDS ? (tile_word + DD_TILE_WORDS) << 4 : b.n_bases;
    for (uint32_t i = threadIdx.x; i < DD_SLOTS; i += DD_THREADS) s.sum[i] = 0;
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0 && (b.offsets[0] != 0 || b.offsets[b.n_reads] != b.n_bases)) *err = 1;
    if (threadIdx.x < 128) { // (two whole waves) the reads that hold the tile's first and last base
        const uint64_t at = threadIdx.x < 64 ? tile : tile_end - 1;
        const uint64_t i = first_at_least(b.offsets, b.n_reads, at + 1, lane); // the first read that starts behind `at`: the one before it holds it
        if (lane == 0) s.read[threadIdx.x >> 6] = i ? i - 1 : 0;
    }
    __syncthreads();
    const uint64_t first = s.read[0], last = s.read[1]; // (both below n_reads)
    const bool aligned = (reinterpret_cast<uintptr_t>(b.words) & 15u) == 0;
    const bool bits_aligned = (reinterpret_cast<uintptr_t>(b.bits) & 7u) == 0;
    // all loads of the lane are issued before the first is used
    uint4 v[DD_ROUNDS];
    uint2 mv[DD_ROUNDS];
    uint32_t next[DD_ROUNDS], mnext[DD_ROUNDS];
#pragma unroll
    for (int round = 0; round < DD_ROUNDS; ++round) {
        const uint64_t w0 = tile_word + ((uint64_t)round * DD_THREADS + threadIdx.x) * DD_LANE_WORDS;
        v[round] = make_uint4(0, 0, 0, 0);
        mv[round] = make_uint2(0, 0);
        next[round] = mnext[round] = 0;
        if (w0 >= n_words) continue;
        if (aligned && w0 + DD_LANE_WORDS <= n_words) v[round] = load_once_16(b.words + w0);
        else {
            v[round].x = b.words[w0];
            if (w0 + 1 < n_words) v[round].y = b.words[w0 + 1];
            if (w0 + 2 < n_words) v[round].z = b.words[w0 + 2];
            if (w0 + 3 < n_words) v[round].w = b.words[w0 + 3];
        }
        if (lane == 63 && w0 + DD_LANE_WORDS < n_words) next[round] = b.words[w0 + DD_LANE_WORDS];
        if (b.bits) {
            if (bits_aligned && w0 + DD_LANE_WORDS <= n_words) mv[round] = *reinterpret_cast<const uint2*>(b.bits + w0);
            else {
                uint32_t m[4] = { 0, 0, 0, 0 };
                for (uint32_t j = 0; j < DD_LANE_WORDS; ++j)
                    if (w0 + j < n_words) m[j] = b.bits[w0 + j];
                mv[round] = make_uint2(m[0] | m[1] << 16, m[2] | m[3] << 16);
            }
            if (lane == 63 && w0 + DD_LANE_WORDS < n_words) mnext[round] = b.bits[w0 + DD_LANE_WORDS];
        }
    }
    bool bad = false;
#pragma unroll
    for (int round = 0; round < DD_ROUNDS; ++round) {
        const uint64_t w0 = tile_word + ((uint64_t)round * DD_THREADS + threadIdx.x) * DD_LANE_WORDS;
        // the word behind the lane's four: the next lane's first (it is inside the batch whenever a base of this lane's windows needs it)
        const uint32_t nx = __shfl_down(v[round].x, 1), mnx = __shfl_down(mv[round].x, 1) & 0xFFFFu;
        const uint32_t w[DD_LANE_WORDS + 1] = { v[round].x, v[round].y, v[round].z, v[round].w, lane == 63 ? next[round] : nx };
        const uint32_t m[DD_LANE_WORDS + 1] = { mv[round].x & 0xFFFFu, mv[round].x >> 16, mv[round].y & 0xFFFFu, mv[round].y >> 16, lane == 63 ? mnext[round] : mnx };
        uint64_t head = ~0ull, sum = 0;
        if (w0 < n_words) {
            uint64_t r = read_holding(b.offsets, first, last, w0 << 4);
            head = r;
            // the terms of one read are added up in registers; a read behind the lane's first goes to the workgroup's array when it is done
            uint64_t cur = r, acc = 0;
            auto emit = [&](uint64_t read, uint64_t t) {
                if (read == cur) {
                    acc += t;
                    return;
                }
                if (cur == head) sum += acc;
                else dd_add(s, key, b.n_reads, first, cur, acc);
                cur = read;
                acc = t;
            };
#pragma unroll
            for (uint32_t j = 0; j < DD_LANE_WORDS; ++j) {
                const uint64_t P = (w0 + j) << 4;
                if (P < b.n_bases) dd_window(b, P, w[j], w[j + 1], m[j], m[j + 1], r, bad, emit);
            }
            if (cur == head) sum += acc;
            else dd_add(s, key, b.n_reads, first, cur, acc);
        }
        // The heads of one read are adjacent lanes: a segmented inclusive scan by shuffles, keyed by the read's place in the tile, and the
        // last lane of every run hands its read's sum over.  (k < 2^32: a sample has fewer than 2^32 reads, which the callers hold.)
        const uint32_t k = head == ~0ull ? 0xFFFFFFFFu : (uint32_t)(head - first);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t ko = __shfl_up(k, off);
            const uint64_t vo = __shfl_up(sum, off);
            if (lane >= off && ko == k) sum += vo;
        }
        const uint32_t kn = __shfl_down(k, 1);
        if (k != 0xFFFFFFFFu && (lane == 63 || kn != k)) dd_add(s, key, b.n_reads, first, head, sum);
    }
    if (bad) *err = 1;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < DD_SLOTS; i += DD_THREADS) {
        const unsigned long long t = s.sum[i];
        if (t && first + i < b.n_reads) atomicAdd(&key[first + i], t);
    }
}

// loc[first + j] = where read j of one resident block lies (loc: n entries; reads of the sample that no block holds keep length 0)
__global__ __launch_bounds__(DD_THREADS) void dedup_loc_kernel(DedupBatch b, uint64_t first, uint64_t n, DedupLoc* __restrict__ loc, uint32_t* __restrict__ err)
{
    const uint64_t j = (uint64_t)blockIdx.x * DD_THREADS + threadIdx.x;
    if (j >= b.n_reads || first + j >= n) return;
    const uint64_t s = b.offsets[j], e = b.offsets[j + 1];
    DedupLoc l { b.words, b.bits, s, 0 };
    if (e < s || e > b.n_bases) *err = 1;
    else l.len = e - s;
    loc[first + j] = l;
}

// what the sort sees: key[i] &= mask, idx[i] = i
__global__ __launch_bounds__(DD_THREADS) void dedup_sort_keys_kernel(uint64_t mask, uint64_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ idx)
{
    const uint64_t i = (uint64_t)blockIdx.x * DD_THREADS + threadIdx.x;
    if (i >= n) return;
    key[i] &= mask;
    idx[i] = (uint32_t)i;
}

__device__ inline bool dd_identical(const DedupLoc& a, const DedupLoc& c)
{
    if (a.len != c.len) return false;
    const uint64_t n_words = (a.len + 15) >> 4;
    for (uint64_t j = 0; j < n_words; ++j)
        if (dd_read_word(a.words, a.bits, a.start, a.len, j) != dd_read_word(c.words, c.bits, c.start, c.len, j)) return false;
    return true;
}

// The exact check: one thread per sorted entry p.  The sort is stable (rocPRIM documents radix_sort_pairs so), so the entries of one masked
// key stand in ascending order of read: every read in front of p in its run has a smaller number, and read order[p] is a duplicate iff it is
// identical to one of them.  The predecessor comes first: a true duplicate costs one comparison, only key collisions walk further.
// flag32[i] and klen[i]: the flag as a word and the read's length if it is kept -- what the two exclusive scans read (entry n of both: 0).
__global__ __launch_bounds__(DD_THREADS) void dedup_check_kernel(const uint64_t* __restrict__ key_sorted, const uint32_t* __restrict__ order, uint64_t n,
    const DedupLoc* __restrict__ loc, uint8_t* __restrict__ flag, uint32_t* __restrict__ flag32, uint64_t* __restrict__ klen, uint32_t* __restrict__ err)
{
    const uint64_t p = (uint64_t)blockIdx.x * DD_THREADS + threadIdx.x;
    if (p > n) return;
    if (p == n) {
        flag32[n] = 0;
        klen[n] = 0;
        return;
    }
    const uint64_t i = order[p];
    if (i >= n) {
        *err = 1;
        return;
    }
    const DedupLoc me = loc[i];
    bool keep = true;
    if (me.len) { // (a read of no bases is never a duplicate and never makes one)
        const uint64_t k = key_sorted[p];
        for (uint64_t q = p; q-- > 0 && key_sorted[q] == k;) {
            const uint64_t h = order[q];
            if (h >= n) {
                *err = 1;
                break;
            }
            if (dd_identical(loc[h], me)) {
                keep = false;
                break;
            }
        }
    }
    flag[i] = keep ? 1 : 0;
    flag32[i] = keep ? 1u : 0u;
    klen[i] = keep ? me.len : 0;
}

hipError_t launch_dedup_keys(const DedupBatch& b, unsigned long long* key, uint32_t* err, hipStream_t stream)
{
    const uint32_t n_tiles = dedup_tiles(b.n_bases);
    if (!n_tiles || !b.n_reads) return hipSuccess;
    hipLaunchKernelGGL(dedup_keys_kernel, dim3(n_tiles), dim3(DD_THREADS), 0, stream, b, key, err);
    return hipGetLastError();
}

hipError_t launch_dedup_loc(const DedupBatch& b, uint64_t first, uint64_t n, DedupLoc* loc, uint32_t* err, hipStream_t stream)
{
    if (!b.n_reads) return hipSuccess;
    hipLaunchKernelGGL(dedup_loc_kernel, dim3((uint32_t)((b.n_reads + DD_THREADS - 1) / DD_THREADS)), dim3(DD_THREADS), 0, stream, b, first, n, loc, err);
    return hipGetLastError();
}

hipError_t launch_dedup_select(const DedupSelect& s, hipStream_t stream)
{
    const uint64_t n = s.n;
    if (!n || n >= (1ull << 32) || s.key_bits < 1 || s.key_bits > 64) return hipErrorInvalidValue;
    size_t temp_bytes = s.temp_bytes; // (rocPRIM takes it by reference)
    const dim3 grid((uint32_t)((n + DD_THREADS - 1) / DD_THREADS)), grid1((uint32_t)((n + 1 + DD_THREADS - 1) / DD_THREADS)), block(DD_THREADS);
    const uint64_t mask = s.key_bits == 64 ? ~0ull : (1ull << s.key_bits) - 1;
    hipLaunchKernelGGL(dedup_sort_keys_kernel, grid, block, 0, stream, mask, n, s.key, s.idx);
    HIP_TRY(hipGetLastError());
    // (masked key, i) ascending: idx ascends going in and the sort is stable, so equal keys stay in read order -- dedup_check_kernel relies on it
    HIP_TRY(sort_hits(s.temp, s.temp_bytes, s.key, s.key_sorted, s.idx, s.idx_sorted, (uint32_t)n, stream));
    // flags; the words the scans read go into idx and key (n + 1 entries each; the sort has left them), the scans into rank and boff
    hipLaunchKernelGGL(dedup_check_kernel, grid1, block, 0, stream, (const uint64_t*)s.key_sorted, (const uint32_t*)s.idx_sorted, n, (const DedupLoc*)s.loc, s.flag, s.idx,
        s.key, s.err);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::exclusive_scan(s.temp, temp_bytes, s.idx, s.rank, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), stream));
    HIP_TRY(rocprim::exclusive_scan(s.temp, temp_bytes, s.key, s.boff, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), stream));
    return hipSuccess;
}

} // namespace dev
} // namespace drprg
