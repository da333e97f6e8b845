// read_stats.hip -- read statistics (drprg_hip_set_read_stats; the rule: include/drprg_hip.h "read statistics"; the
// layout: read_stats_words.h): the reads of a ragged batch, in either form, counted into one snapshot's device accumulators.  Nothing of
// the batch is written.  Driven by Mapper::run_read_stats, which owns every buffer.
//
// read_stats_pos_kernel tiles the BUFFER, as base_mask_kernel does -- 16 384 bases per workgroup, 64 per lane: four 16-base loads in the
// common form (load16.h) and, with qualities, four 16-byte loads beside them.  A lane walks the reads under its 64 positions (the reads of
// the tile's ends come from two searches, the lane's first from a search between the two), so that it knows every base's cycle, whether
// the read counts (keep flag, `take`) and -- a reverse-strand BAM read -- the mirrored quality byte.  It adds to three histograms that are
// private to the workgroup, in LDS, as 32-bit counters (a tile holds 16 384 bases: none can overflow):
//   cycle x {A, C, G, T, U} and the cycle's Phred sum: a wave's lanes stand 64 bases apart, so for reads that are not a power of two long
//     they hit different cycles; everything at or beyond cycle 512 is ONE bin, which every lane of a long read would hit at once: those
//     counts stay in registers and leave the wave through shuffles, one atomic per wave and column;
//   bases per Phred value: NovaSeq qualities take four values, so one counter per value would serialise a wave 64-fold: every lane has a
//     column of its own (94 x 64 words), which no other lane of its wave touches; the columns are summed, rotated against the banks, at the end.
// What a read needs from its bases -- G + C, valid bases and the sum of E -- is summed per lane and read and leaves with one 64-bit global
// atomic each when the lane's read changes.  Non-zero LDS entries are flushed with 64-bit global atomics.
//
// read_stats_read_kernel: one thread per read, 2048 reads per workgroup.  Length from the offsets, the three per-read words the first
// kernel left; length, read-quality and GC histograms again in LDS.  All reads of an Illumina run share one length bin: equal bins of a
// wave are found by ballots and added once.
//
// Every index that comes from device data is bounded before it is used; offsets that do not ascend to n_bases set RS_DEV_OFFSETS, a
// quality byte outside [bias, bias + 93] sends its index + 1 to RS_DEV_BAD_AT by an atomic min and is not counted.
#include "load16.h"
#include "read_qual_piece.h"
#include "search.h"

namespace drprg {
namespace dev {

constexpr int RS_THREADS = 256;
constexpr uint32_t RS_LANE_BASES = 64;
constexpr uint32_t RS_TILE = RS_THREADS * RS_LANE_BASES; // 16384 bases per workgroup
constexpr uint32_t RS_WG_READS = RS_THREADS * 8;         // reads per workgroup of read_stats_read_kernel

uint32_t read_stats_tiles(uint64_t n_bases) { return (uint32_t)((n_bases + RS_TILE - 1) / RS_TILE); }

__device__ inline unsigned long long rs_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <bool QUAL> __global__ __launch_bounds__(RS_THREADS) void read_stats_pos_kernel(ReadStatsArgs a)
{
    __shared__ uint32_t s_cyc[(RS_CYCLES + 1) * RS_COLS];
    __shared__ uint32_t s_qs[RS_CYCLES + 1];
    __shared__ uint32_t s_qh[QUAL ? RS_QUALS * 64 : 1];
    __shared__ uint32_t s_e[RS_QUALS];
    __shared__ uint64_t s_read[2];
    const uint64_t take = a.take < a.n_reads ? a.take : a.n_reads;
    uint64_t lim = a.offsets[take]; // nothing behind the last read that can count is looked at
    if (lim > a.n_bases) lim = a.n_bases;
    const uint64_t tile = (uint64_t)blockIdx.x * RS_TILE;
    if (tile >= lim) return; // (uniform)
    const uint64_t tile_end = lim - tile > RS_TILE ? tile + RS_TILE : lim;
    for (uint32_t i = threadIdx.x; i < (RS_CYCLES + 1) * RS_COLS; i += RS_THREADS) s_cyc[i] = 0;
    for (uint32_t i = threadIdx.x; i < RS_CYCLES + 1; i += RS_THREADS) s_qs[i] = 0;
    if (QUAL) {
        for (uint32_t i = threadIdx.x; i < RS_QUALS * 64; i += RS_THREADS) s_qh[i] = 0;
        if (threadIdx.x < RS_QUALS) s_e[threadIdx.x] = RQ_E[threadIdx.x];
    }
    if (threadIdx.x == 0 || threadIdx.x == 64) s_read[threadIdx.x >> 6] = read_holding(a.offsets, 0, a.n_reads - 1, threadIdx.x == 0 ? tile : tile_end - 1);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p0 = tile + (uint64_t)threadIdx.x * RS_LANE_BASES;
    uint32_t ov[RS_COLS] = { 0, 0, 0, 0, 0 }; // the bin of every cycle from RS_CYCLES on
    unsigned long long ovq = 0;
    uint64_t bad_at = ~0ull;
    bool odd = false; // the offsets and n_bases do not fit each other
    if (p0 < tile_end) {
        const bool aligned_t = (reinterpret_cast<uintptr_t>(a.text) & 15u) == 0;
        const bool aligned_q = QUAL && (reinterpret_cast<uintptr_t>(a.qual) & 15u) == 0;
        uint64_t r = read_holding(a.offsets, s_read[0], s_read[1], p0);
        uint64_t s = a.offsets[r], e = a.offsets[r + 1];
        bool counted = false, mirrored = false;
        auto enter = [&]() { // the read the walk has arrived at: does it count, and are its quality bytes stored mirrored?
            const bool ok = s <= e && e <= a.n_bases;
            if (!ok) odd = true;
            counted = ok && r < take && (!a.flags || a.flags[r]);
            mirrored = counted && a.rev && a.rev[r];
        };
        enter();
        unsigned long long gc = 0, valid = 0, es = 0; // of read r, under this lane
        bool dirty = false;
        auto leave = [&]() {
            if (dirty) {
                atomicAdd(&a.gcv[r], (gc << 32) | valid);
                if (QUAL) atomicAdd(&a.esum[r], es);
            }
            gc = valid = es = 0;
            dirty = false;
        };
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t g0 = p0 + 16u * j;
            if (g0 >= tile_end) break;
            const uint32_t ng = (uint32_t)(tile_end - g0 < 16 ? tile_end - g0 : 16);
            uint32_t code, nmask;
            load16_common(a.text, a.words, a.nbits, a.n_bases, aligned_t, g0, code, nmask);
            uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0; // the group's quality bytes at their own positions (aligned buffers are padded)
            if (aligned_q) {
                const uint4 v = load_once_16(a.qual + g0);
                q0 = v.x; q1 = v.y; q2 = v.z; q3 = v.w;
            }
            for (uint32_t k = 0; k < ng; ++k) {
                const uint64_t p = g0 + k;
                const uint32_t letter = code & 3u, unk = nmask & 1u, direct = q0 & 0xFFu;
                code >>= 2; nmask >>= 1;
                q0 = (q0 >> 8) | (q1 << 24); q1 = (q1 >> 8) | (q2 << 24); q2 = (q2 >> 8) | (q3 << 24); q3 >>= 8;
                if (p >= e) {
                    leave();
                    while (r + 1 < a.n_reads && e <= p) {
                        ++r;
                        s = e;
                        e = a.offsets[r + 1];
                    }
                    enter();
                }
                if (p < s || p >= e) { // (offsets that do not ascend)
                    odd = true;
                    continue;
                }
                if (!counted) continue;
                const uint64_t cyc = p - s;
                const uint32_t col = unk ? 4u : letter ^ (letter >> 1); // common form A0 C1 T2 G3 -> columns A C G T
                uint32_t q = 0;
                if (QUAL) {
                    const uint64_t at = mirrored ? s + (e - 1 - p) : p; // s <= at < e <= n_bases
                    q = (aligned_q && !mirrored ? direct : (uint32_t)a.qual[at]) - a.bias;
                    if (q > RQ_MAX_QUAL) {
                        if (at < bad_at) bad_at = at;
                        continue;
                    }
                    atomicAdd(&s_qh[q * 64u + lane], 1u);
                    es += s_e[q];
                }
                if (cyc < RS_CYCLES) {
                    atomicAdd(&s_cyc[(uint32_t)cyc * RS_COLS + col], 1u);
                    if (QUAL) atomicAdd(&s_qs[cyc], q);
                } else {
#pragma unroll
                    for (uint32_t c = 0; c < RS_COLS; ++c) ov[c] += col == c ? 1u : 0u;
                    ovq += q;
                }
                valid += unk ^ 1u;
                gc += (unk ^ 1u) & letter; // C = 1, G = 3
                dirty = true;
            }
        }
        leave();
    }
    if (bad_at != ~0ull) atomicMin(&a.acc[RS_DEV_BAD_AT], (unsigned long long)(bad_at + 1));
    if (odd) a.acc[RS_DEV_OFFSETS] = 1;
#pragma unroll
    for (uint32_t c = 0; c < RS_COLS; ++c) {
        const uint32_t n = (uint32_t)rs_wave_sum(ov[c]);
        if (lane == 0 && n) atomicAdd(&s_cyc[RS_CYCLES * RS_COLS + c], n);
    }
    if (QUAL) {
        const uint32_t n = (uint32_t)rs_wave_sum(ovq); // (at most 16 384 x 93)
        if (lane == 0 && n) atomicAdd(&s_qs[RS_CYCLES], n);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (RS_CYCLES + 1) * RS_COLS; i += RS_THREADS)
        if (s_cyc[i]) atomicAdd(&a.acc[RS_CYC_BASE + i], (unsigned long long)s_cyc[i]);
    if (QUAL) {
        for (uint32_t i = threadIdx.x; i < RS_CYCLES + 1; i += RS_THREADS)
            if (s_qs[i]) atomicAdd(&a.acc[RS_CYC_QSUM + i], (unsigned long long)s_qs[i]);
        if (threadIdx.x < RS_QUALS) {
            uint32_t n = 0;
            for (uint32_t j = 0; j < 64; ++j) n += s_qh[threadIdx.x * 64u + ((j + threadIdx.x) & 63u)]; // (rotated: the threads read different banks)
            if (n) atomicAdd(&a.acc[RS_QUAL_HIST + threadIdx.x], (unsigned long long)n);
        }
    }
}

// hist[bin] += the number of lanes with `on` and this bin, one atomic per distinct bin of the wave.  Every lane of the wave calls it.
__device__ inline void rs_wave_count(uint32_t* hist, uint32_t bin, bool on, uint32_t lane)
{
    uint64_t todo = __ballot(on);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t b = __shfl(bin, leader);
        const uint64_t m = __ballot(on && bin == b);
        if ((int)lane == leader) atomicAdd(&hist[b], (uint32_t)__popcll(m));
        todo &= ~m;
    }
}

template <bool QUAL> __global__ __launch_bounds__(RS_THREADS) void read_stats_read_kernel(ReadStatsArgs a)
{
    __shared__ uint32_t s_lr[RS_LEN_BINS];
    __shared__ unsigned long long s_lb[RS_LEN_BINS];
    __shared__ uint32_t s_rq[RS_QUALS], s_gc[RS_GC_BINS], s_e[RS_QUALS];
    __shared__ unsigned long long s_tot[4];
    for (uint32_t i = threadIdx.x; i < RS_LEN_BINS; i += RS_THREADS) {
        s_lr[i] = 0;
        s_lb[i] = 0;
    }
    if (threadIdx.x < RS_QUALS) {
        s_rq[threadIdx.x] = 0;
        s_e[threadIdx.x] = RQ_E[threadIdx.x];
    }
    if (threadIdx.x < RS_GC_BINS) s_gc[threadIdx.x] = 0;
    if (threadIdx.x < 4) s_tot[threadIdx.x] = threadIdx.x == 2 ? ~0ull : 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t take = a.take < a.n_reads ? a.take : a.n_reads;
    unsigned long long n_reads = 0, n_bases = 0, shortest = ~0ull, longest = 0;
    bool odd = blockIdx.x == 0 && threadIdx.x == 0 && (a.offsets[0] != 0 || a.offsets[a.n_reads] != a.n_bases);
    for (uint32_t it = 0; it < RS_WG_READS / RS_THREADS; ++it) { // (uniform trip count: the ballots below want whole waves)
        const uint64_t r = (uint64_t)blockIdx.x * RS_WG_READS + (uint64_t)it * RS_THREADS + threadIdx.x;
        uint64_t L = 0;
        bool counted = false;
        if (r < a.n_reads) {
            const uint64_t s = a.offsets[r], e = a.offsets[r + 1];
            if (s <= e && e <= a.n_bases) {
                L = e - s;
                counted = r < take && (!a.flags || a.flags[r]);
            } else odd = true;
        }
        if (counted) {
            ++n_reads;
            n_bases += L;
            if (L < shortest) shortest = L;
            if (L > longest) longest = L;
        }
        // the length histogram: reads, and the exact sum of their lengths (L <= n_bases < 2^32: the bin is below RS_LEN_BINS)
        const uint32_t bin = rs_len_bin(L & 0xFFFFFFFFull);
        uint64_t todo = __ballot(counted);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t b = __shfl(bin, leader);
            const bool mine = counted && bin == b;
            const uint64_t m = __ballot(mine);
            unsigned long long sum = (unsigned long long)__popcll(m) * b; // (an exact bin: every read of it is b bases long)
            if (b >= 1024u) sum = rs_wave_sum(mine ? L : 0ull);
            if ((int)lane == leader) {
                atomicAdd(&s_lr[b], (uint32_t)__popcll(m));
                if (sum) atomicAdd(&s_lb[b], sum);
            }
            todo &= ~m;
        }
        unsigned long long g = 0;
        if (counted && L) g = a.gcv[r];
        const uint64_t V = g & 0xFFFFFFFFull, GC = g >> 32;
        uint32_t gbin = V ? (uint32_t)(100ull * GC / V) : 0u;
        if (gbin > 100u) gbin = 100u; // (never: G + C <= V)
        rs_wave_count(s_gc, gbin, counted && V != 0, lane);
        if (QUAL) {
            uint32_t lo = 0, hi = RQ_MAX_QUAL; // the largest q with S <= E[q] L (E descends; q = 0 always holds: S <= 2^31 L)
            if (counted && L) {
                const unsigned long long S = a.esum[r];
                while (lo < hi) {
                    const uint32_t mid = (lo + hi + 1) >> 1;
                    if (S <= (unsigned long long)s_e[mid] * L) lo = mid;
                    else hi = mid - 1;
                }
            }
            rs_wave_count(s_rq, lo, counted && L != 0, lane);
        }
    }
    if (odd) a.acc[RS_DEV_OFFSETS] = 1;
    n_reads = rs_wave_sum(n_reads);
    n_bases = rs_wave_sum(n_bases);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long lo = __shfl_xor(shortest, off), hi = __shfl_xor(longest, off);
        if (lo < shortest) shortest = lo;
        if (hi > longest) longest = hi;
    }
    if (lane == 0 && n_reads) {
        atomicAdd(&s_tot[0], n_reads);
        atomicAdd(&s_tot[1], n_bases);
        atomicMin(&s_tot[2], shortest);
        atomicMax(&s_tot[3], longest);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_tot[0]) {
        atomicAdd(&a.acc[RS_READS], s_tot[0]);
        if (s_tot[1]) atomicAdd(&a.acc[RS_BASES], s_tot[1]);
        atomicMin(&a.acc[RS_MIN_LEN], s_tot[2]);
        atomicMax(&a.acc[RS_MAX_LEN], s_tot[3]);
    }
    for (uint32_t i = threadIdx.x; i < RS_LEN_BINS; i += RS_THREADS) {
        if (s_lr[i]) atomicAdd(&a.acc[RS_LEN_READS + i], (unsigned long long)s_lr[i]);
        if (s_lb[i]) atomicAdd(&a.acc[RS_LEN_BASES + i], s_lb[i]);
    }
    if (threadIdx.x < RS_GC_BINS && s_gc[threadIdx.x]) atomicAdd(&a.acc[RS_GC_HIST + threadIdx.x], (unsigned long long)s_gc[threadIdx.x]);
    if (QUAL && threadIdx.x < RS_QUALS && s_rq[threadIdx.x]) atomicAdd(&a.acc[RS_READQ_HIST + threadIdx.x], (unsigned long long)s_rq[threadIdx.x]);
}

hipError_t launch_read_stats_clear(unsigned long long* acc, hipStream_t stream)
{
    HIP_TRY(hipMemsetAsync(acc, 0, RS_DEV_WORDS * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(acc + RS_MIN_LEN, 0xFF, sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(acc + RS_DEV_BAD_AT, 0xFF, sizeof(unsigned long long), stream));
    return hipSuccess;
}

hipError_t launch_read_stats(const ReadStatsArgs& a, hipStream_t stream, KernelTimer timer)
{
    if (!a.n_reads) return hipSuccess;
    if (a.n_reads > MAX_BATCH_READS || a.n_bases >= RS_MAX_BASES || (a.bias != 0 && a.bias != 33) || !a.offsets || !a.gcv || !a.acc) return hipErrorInvalidValue;
    if (a.n_bases && ((a.text != nullptr) == (a.words != nullptr) || (a.qual && !a.esum))) return hipErrorInvalidValue;
    HIP_TRY(hipMemsetAsync(a.gcv, 0, a.n_reads * sizeof(unsigned long long), stream));
    if (a.qual) HIP_TRY(hipMemsetAsync(a.esum, 0, a.n_reads * sizeof(unsigned long long), stream));
    const uint32_t n_tiles = read_stats_tiles(a.n_bases), n_groups = (uint32_t)((a.n_reads + RS_WG_READS - 1) / RS_WG_READS);
    if (n_tiles) {
        if (a.qual) launch_timed(timer, read_stats_pos_kernel<true>, dim3(n_tiles), dim3(RS_THREADS), 0, stream, a);
        else launch_timed(timer, read_stats_pos_kernel<false>, dim3(n_tiles), dim3(RS_THREADS), 0, stream, a);
    }
    if (a.qual) hipLaunchKernelGGL(read_stats_read_kernel<true>, dim3(n_groups), dim3(RS_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(read_stats_read_kernel<false>, dim3(n_groups), dim3(RS_THREADS), 0, stream, a);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
