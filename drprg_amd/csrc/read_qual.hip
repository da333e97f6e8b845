// read_qual.hip -- the read filter (drprg_hip_set_read_filter; the rule: include/drprg_hip.h "read filter"): one exact
// number per read from a ragged batch of quality bytes, then one flag per read.  Driven by Mapper::run_read_filter, which owns every buffer.
//
// read_qual_kernel is a segmented sum over the batch's concatenated quality buffer.  The BUFFER is tiled, not the reads -- 16 384 bytes per
// workgroup, as bam_pack_kernel tiles the bases --, so a batch of 150-base reads and one of 50 kb reads run the same code at the same rate.
// A lane loads 16 bytes four times (four rounds, each a coalesced 4 KB of the workgroup, all four loads issued up front), looks every byte up in the 94-entry table E, which
// lies in LDS, and splits its 16 values by read (rq_piece, read_qual_piece.h: host code as well).  The read that holds a workgroup's first
// and last byte comes from two 64-way searches over `offsets` (first_at_least, search.h: one wave each), a lane's own read from a search between the two, further reads by walking.
// The sums of the lanes whose first byte lies in one read are added up inside the wave (one read under the whole wave: a reduction in
// registers; otherwise a segmented scan by shuffles -- the read numbers ascend along the wave), the wave's runs and the few pieces behind a read boundary go to a per-workgroup array of 64-bit sums in LDS,
// indexed by read minus the workgroup's first read, and every read the workgroup touched gets ONE 64-bit atomic add to qsum[read].  (A
// tile of more than RQ_SLOTS reads -- reads of under 16 bases on average -- sends the runs beyond the array straight to qsum.)  Integer
// adds commute: qsum is bit-exact whatever the launch geometry and the order of the atomics.
//
// The table: u32[94] in LDS, read with ds_read_b32 (32 banks, conflicts counted per 32-lane half): lanes with the same quality broadcast,
// lanes whose qualities differ by 32 or 64 share a bank.  Real quality strings keep most bytes of a half inside a span of 32, so the
// lookup mostly runs conflict-free; uniform random qualities over 0..93 cost about three LDS cycles per half instead of one -- and take the
// same kernel time to 1 % (measured): the lookup is not what the kernel waits for.  The sums never wait for a lookup of another byte: 16
// independent lookups are in flight per lane and round.
//
// Meant to be bound by reading n_bases bytes from HBM; measured at 0.20 of 8 TB/s on 2 M x 4 kb, bound by the instructions issued per byte
// (about ten vector instructions and the lookup): DESIGN.md section 6 has the numbers and the first remedy.
// A byte outside [bias, bias + 93] sends its position + 1 to the error word by an atomic min (the sums of such a batch mean nothing); every index that comes
// from device data is bounded by n_reads before it is used, so nothing is written out of bounds whatever `offsets` holds.
#include "read_qual_piece.h"
#include "search.h"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/warp/warp_reduce.hpp>

namespace drprg {
namespace dev {

constexpr int RQ_THREADS = 256;
constexpr int RQ_ROUNDS = 4;
constexpr uint32_t RQ_LANE_BYTES = 16;
constexpr uint32_t RQ_TILE = RQ_THREADS * RQ_ROUNDS * RQ_LANE_BYTES; // 16384 bytes per workgroup
constexpr uint32_t RQ_SLOTS = 1024;                                  // per-workgroup sums in LDS: reads first .. first + 1023 of the tile

uint32_t read_qual_tiles(uint64_t n_bases) { return (uint32_t)((n_bases + RQ_TILE - 1) / RQ_TILE); }

struct RqLds {
    unsigned long long sum[RQ_SLOTS];
    uint32_t e[128];
    uint64_t read[2];
};

__device__ inline void rq_add(RqLds& s, unsigned long long* __restrict__ qsum, uint64_t n_reads, uint64_t first, uint64_t read, uint64_t v)
{
    if (read >= n_reads || read < first) return;
    if (read - first < RQ_SLOTS) atomicAdd(&s.sum[read - first], (unsigned long long)v);
    else atomicAdd(&qsum[read], (unsigned long long)v);
}

__global__ __launch_bounds__(RQ_THREADS) void read_qual_kernel(const uint8_t* __restrict__ qual, uint32_t bias, const uint64_t* __restrict__ offsets, uint64_t n_reads,
    uint64_t n_bases, unsigned long long* __restrict__ qsum, unsigned long long* __restrict__ bad_at)
{
    using WaveReduce = rocprim::warp_reduce<unsigned long long, 64>;
    __shared__ RqLds s;
    __shared__ typename WaveReduce::storage_type s_wr[RQ_THREADS / 64]; // one per wave
    const uint64_t tile = (uint64_t)blockIdx.x * RQ_TILE;
    if (tile >= n_bases) return; // (uniform)
    const uint64_t tile_end = n_bases - tile > RQ_TILE ? tile + RQ_TILE : n_bases;
    for (uint32_t i = threadIdx.x; i < RQ_SLOTS; i += RQ_THREADS) s.sum[i] = 0;
    if (threadIdx.x < 128) s.e[threadIdx.x] = threadIdx.x <= RQ_MAX_QUAL ? RQ_E[threadIdx.x] : 0u;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 128) { // (two whole waves) the reads that hold the tile's first and last byte: the 64-way search, four dependent loads
        // for 2^24 reads where one lane's binary search takes 24 -- a workgroup has 16 KB to read, and waited longer for that search
        const uint64_t at = threadIdx.x < 64 ? tile : tile_end - 1;
        const uint64_t i = first_at_least(offsets, n_reads, at + 1, lane); // the first read that starts behind `at`: the one before it holds it
        if (lane == 0) s.read[threadIdx.x >> 6] = i ? i - 1 : 0;
    }
    __syncthreads();
    const uint64_t first = s.read[0], last = s.read[1];
    const bool aligned = (reinterpret_cast<uintptr_t>(qual) & 15u) == 0;
    uint64_t bad = ~0ull;
    // all four loads of the lane are issued before the first is used: 64 bytes in flight per lane instead of 16 (one load at a time left the
    // kernel waiting for HBM latency at a fifth of the bandwidth)
    uint4 v[RQ_ROUNDS];
#pragma unroll
    for (int round = 0; round < RQ_ROUNDS; ++round) {
        const uint64_t p = tile + ((uint64_t)round * RQ_THREADS + threadIdx.x) * RQ_LANE_BYTES;
        v[round] = aligned && p < tile_end ? load_once_16(qual + p) : make_uint4(0, 0, 0, 0); // (the buffer is padded: the 16 bytes at p < n_bases are readable)
    }
#pragma unroll
    for (int round = 0; round < RQ_ROUNDS; ++round) {
        const uint64_t p = tile + ((uint64_t)round * RQ_THREADS + threadIdx.x) * RQ_LANE_BYTES;
        uint64_t head = ~0ull, sum = 0;
        if (p < tile_end) {
            const uint32_t n = (uint32_t)(tile_end - p < RQ_LANE_BYTES ? tile_end - p : RQ_LANE_BYTES);
            uint32_t w[4] = { 0, 0, 0, 0 };
            if (aligned) {
                w[0] = v[round].x; w[1] = v[round].y; w[2] = v[round].z; w[3] = v[round].w;
            } else {
#pragma unroll
                for (uint32_t j = 0; j < RQ_LANE_BYTES; ++j)
                    if (j < n) w[j >> 2] |= (uint32_t)qual[p + j] << (8 * (j & 3));
            }
            uint32_t e[RQ_LANE_BYTES], bad_bits = 0;
#pragma unroll
            for (uint32_t j = 0; j < RQ_LANE_BYTES; ++j) {
                const uint32_t q = ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) - bias; // (below the bias: wraps to a large value)
                bad_bits |= (q > RQ_MAX_QUAL ? 1u : 0u) << j;
                e[j] = s.e[q & 127u]; // (entries 94 .. 127 are zero; the sums of a batch with a byte out of range mean nothing: the call fails)
            }
            bad_bits &= (1u << n) - 1u; // (n <= 16; bytes behind the tile's end are padding)
            if (bad_bits) {
                const uint64_t at = p + (uint64_t)(__ffs(bad_bits) - 1);
                if (at < bad) bad = at;
            }
            uint64_t r = read_holding(offsets, first, last, p);
            sum = rq_piece(offsets, n_reads, p, n, e, r, head, [&](uint64_t read, uint64_t v) { rq_add(s, qsum, n_reads, first, read, v); });
        }
        // The heads of one read are adjacent lanes.  One read under the whole wave (every wave of a tile inside a long read): a reduction
        // in registers (DPP).  Otherwise a segmented inclusive scan by shuffles, keyed by the read's place in the tile, and the last lane of
        // every run hands its read's sum over.
        const uint32_t key = head == ~0ull ? 0xFFFFFFFFu : (uint32_t)(head - first);
        if (__all(key == (uint32_t)__builtin_amdgcn_readfirstlane((int)key))) {
            if (key == 0xFFFFFFFFu) continue; // (uniform: the wave lies behind the tile's end)
            unsigned long long total = 0;
            WaveReduce().reduce((unsigned long long)sum, total, s_wr[threadIdx.x >> 6]);
            if (lane == 0) rq_add(s, qsum, n_reads, first, head, total);
            continue;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t k = __shfl_up(key, off);
            const uint64_t v = __shfl_up(sum, off);
            if (lane >= off && k == key) sum += v;
        }
        const uint32_t next = __shfl_down(key, 1);
        if (key != 0xFFFFFFFFu && (lane == 63 || next != key)) rq_add(s, qsum, n_reads, first, head, sum);
    }
    if (bad != ~0ull) atomicMin(bad_at, (unsigned long long)(bad + 1));
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < RQ_SLOTS; i += RQ_THREADS) {
        const unsigned long long v = s.sum[i];
        if (v && first + i < n_reads) atomicAdd(&qsum[first + i], v);
    }
}

// flag[i] = read i passes the rule; flag32[i] and klen[i]: the same as a word, and the read's length if it is kept -- what the two
// exclusive scans read (entry n_reads of both: 0).  work[RF_SHORT .. RF_LOWQ] count the dropped reads, work[RF_OFFSETS] is set when the
// offsets do not ascend or end at n_bases.  Under a decoy set (a.decoy_valid != null) a read that passed these tests is held against the
// decoy screen's verdict (dc_drops) and counted in work[RF_DECOY_*]; under a complexity threshold (a.cplx_diff != null) it is held
// against that verdict first (cx_drops, poly_piece.h), counted in work[RF_CPLX_*], and the decoy verdict sees only what it kept.
__global__ __launch_bounds__(RQ_THREADS) void read_flags_kernel(ReadFilterArgs a)
{
    __shared__ uint32_t s_n[3];
    __shared__ unsigned long long s_d[6], s_c[4];
    if (threadIdx.x < 3) s_n[threadIdx.x] = 0;
    if (threadIdx.x < 6) s_d[threadIdx.x] = 0;
    if (threadIdx.x < 4) s_c[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * RQ_THREADS + threadIdx.x;
    if (i == a.n_reads) {
        a.flag32[i] = 0;
        a.klen[i] = 0;
        if (a.offsets[i] != a.n_bases) a.work[RF_OFFSETS] = 1;
    }
    if (i < a.n_reads) {
        const uint64_t s = a.offsets[i], e = a.offsets[i + 1];
        uint64_t len = 0;
        if (e < s || e > a.n_bases) a.work[RF_OFFSETS] = 1;
        else len = e - s;
        int why = -1;
        if (len < a.min_len) why = 0;
        else if (a.max_len && len > a.max_len) why = 1;
        else if (a.use_qual) {
            // kept iff S <= L * T (a product beyond 64 bits is above every sum)
            const uint64_t S = a.qsum[i];
            if (__umul64hi(len, a.T) == 0 && S > len * a.T) why = 2;
        }
        if (why >= 0) atomicAdd(&s_n[why], 1u);
        else if (a.cplx_diff) { // the low-complexity verdict, on what the length and quality tests kept
            atomicAdd(&s_c[0], 1ull);
            atomicAdd(&s_c[1], (unsigned long long)len);
            if (cx_drops(a.cplx_diff[i], len, a.cplx_percent)) {
                why = 4;
                atomicAdd(&s_c[2], 1ull);
                atomicAdd(&s_c[3], (unsigned long long)len);
            }
        }
        if (why < 0 && a.decoy_valid) {
            const uint32_t V = a.decoy_valid[i], H = a.decoy_hits[i];
            atomicAdd(&s_d[0], 1ull);
            atomicAdd(&s_d[1], (unsigned long long)len);
            if (V) atomicAdd(&s_d[4], (unsigned long long)V);
            if (H) atomicAdd(&s_d[5], (unsigned long long)H);
            if (dc_drops(V, H, a.decoy_frac_milli, a.decoy_min_kmers)) {
                why = 3;
                atomicAdd(&s_d[2], 1ull);
                atomicAdd(&s_d[3], (unsigned long long)len);
            }
        }
        a.flag[i] = why < 0 ? 1 : 0;
        a.flag32[i] = why < 0 ? 1u : 0u;
        a.klen[i] = why < 0 ? len : 0;
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_n[threadIdx.x]) atomicAdd(&a.work[RF_SHORT + threadIdx.x], (unsigned long long)s_n[threadIdx.x]);
    if (threadIdx.x < 6 && s_d[threadIdx.x]) atomicAdd(&a.work[RF_DECOY_READS + threadIdx.x], s_d[threadIdx.x]);
    if (threadIdx.x < 4 && s_c[threadIdx.x]) atomicAdd(&a.work[RF_CPLX_READS + threadIdx.x], s_c[threadIdx.x]);
}

// the totals of the two scans beside the counts, and everything into `out` (page-locked host memory, or device memory)
__global__ void read_filter_result_kernel(ReadFilterArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    a.out[RF_KEPT_READS] = a.rank[a.n_reads];
    a.out[RF_KEPT_BASES] = a.boff[a.n_reads];
    a.out[RF_SHORT] = a.work[RF_SHORT];
    a.out[RF_LONG] = a.work[RF_LONG];
    a.out[RF_LOWQ] = a.work[RF_LOWQ];
    a.out[RF_BAD_AT] = a.work[RF_BAD_AT] == ~0ull ? 0ull : a.work[RF_BAD_AT];
    a.out[RF_OFFSETS] = a.work[RF_OFFSETS];
    a.out[RF_ERR] = 0;
    for (int i = RF_DECOY_READS; i < RF_WORDS; ++i) a.out[i] = a.work[i];
}

size_t read_filter_temp_bytes(uint64_t n_reads)
{
    size_t a = 0, b = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n_reads + 1, rocprim::plus<uint32_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>(), (hipStream_t)0);
    return a > b ? a : b;
}

hipError_t launch_read_qual(const uint8_t* qual, uint32_t bias, const uint64_t* offsets, uint64_t n_reads, uint64_t n_bases, unsigned long long* qsum,
    unsigned long long* bad_at, hipStream_t stream, KernelTimer timer)
{
    const uint32_t n_tiles = read_qual_tiles(n_bases);
    if (!n_tiles || !n_reads) return hipSuccess;
    launch_timed(timer, read_qual_kernel, dim3(n_tiles), dim3(RQ_THREADS), 0, stream, qual, bias, offsets, n_reads, n_bases, qsum, bad_at);
    return hipGetLastError();
}

hipError_t launch_read_filter(const ReadFilterArgs& a, hipStream_t stream, KernelTimer timer)
{
    if (!a.n_reads || a.n_reads > MAX_BATCH_READS) return hipErrorInvalidValue;
    size_t temp_bytes = a.temp_bytes; // (rocPRIM takes it by reference)
    HIP_TRY(hipMemsetAsync(a.work, 0, RF_WORDS * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(a.work + RF_BAD_AT, 0xFF, sizeof(unsigned long long), stream));
    if (a.use_qual) {
        HIP_TRY(hipMemsetAsync(a.qsum, 0, a.n_reads * sizeof(unsigned long long), stream));
        HIP_TRY(launch_read_qual(a.qual, a.bias, a.offsets, a.n_reads, a.n_bases, a.qsum, a.work + RF_BAD_AT, stream, timer));
    }
    hipLaunchKernelGGL(read_flags_kernel, dim3((uint32_t)((a.n_reads + 1 + RQ_THREADS - 1) / RQ_THREADS)), dim3(RQ_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::exclusive_scan(a.temp, temp_bytes, a.flag32, a.rank, 0u, (size_t)a.n_reads + 1, rocprim::plus<uint32_t>(), stream));
    HIP_TRY(rocprim::exclusive_scan(a.temp, temp_bytes, a.klen, a.boff, (uint64_t)0, (size_t)a.n_reads + 1, rocprim::plus<uint64_t>(), stream));
    hipLaunchKernelGGL(read_filter_result_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
