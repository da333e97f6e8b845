// read_trim.hip -- read trimming (drprg_hip_set_read_trim; the rule: include/drprg_hip.h "read trimming"): the kept
// range of every read of a ragged batch from its quality bytes and two fixed crops, then the tables the compaction kernels of
// subsample.hip and anchor_scan.hip make the trimmed block from.  Driven by Mapper::run_read_trim, which owns every buffer.
//
// trim_points_kernel (only under a quality threshold) is a segmented first/last search over the batch's concatenated quality buffer.  The
// BUFFER is tiled, not the reads -- 16 384 bytes per workgroup, as read_qual_kernel tiles it --, so 150-base reads and 50 kb reads run the
// same code.  A lane takes 16 window starts per round, four rounds, all four 16-byte loads issued before the first is used.  A window of W
// <= 32 bytes needs up to 31 bytes behind the lane's own: they come by shuffle from the next one or two lanes, and by a global load on the
// last two lanes of a wave (the buffer's 64 zero bytes behind n_bases make every such load legal; a window that runs past its read is
// invalid anyway).  The 16 window sums are a running sum over those bytes (rt_good_bits, read_trim_piece.h: host code as well), the
// starts are split by read and held against each read's cropped range (rt_piece), and every read gets the smallest good start and the
// largest + 1, counted from its cropped start: 32-bit words, min and max.  A wave that lies under one read reduces in registers; whatever
// is left goes to two per-workgroup arrays in LDS indexed by read minus the workgroup's first read, and every read the workgroup found a
// window for gets ONE atomicMin and ONE atomicMax in global memory (a tile of more than RT_SLOTS reads sends the reads beyond the arrays
// straight there).  Min and max commute: the result is bit-exact whatever the launch geometry.  A byte outside [bias, bias + 93] sends its
// position + 1 to the error word by an atomic min; every index that comes from device data is bounded before it is used.
// Measured at 0.14 of 8 TB/s on 2 M x 4 kb (6.90 ms beside read_qual_kernel's 4.87 in the same run), bound like it by the instructions
// issued per byte: DESIGN.md section 6 has the numbers and the first remedy.
//
// trim_tables_kernel: one thread per read -- the crop, the two narrowing walks of at most W bytes each, the mirror for reversed records,
// the read's new length and the counts.  One rocPRIM u64 exclusive scan of the lengths gives the new offsets; trim_fill_kernel then writes
// where every trimmed read starts in the old block (what launch_subsample_pack and launch_gather_reads take), and trim_npos_kernel moves
// the listed non-ACGT positions that stay (count, scan, emit: ascending without a sort).  Under adapters (drprg_hip_set_adapters) the two
// kernels of adapter_trim.hip -- under the indel rule (drprg_hip_set_adapters2) those of adapter_edit.hip, for either end -- run between
// the tables and the scan and shorten the ranges once more.
#include "read_trim_piece.h"
#include "search.h"
#include <rocprim/device/device_scan.hpp>

namespace drprg {
namespace dev {

constexpr int RT_THREADS = 256;
constexpr int RT_ROUNDS = 4;
constexpr uint32_t RT_TILE = RT_THREADS * RT_ROUNDS * RT_LANE_STARTS; // 16384 bytes per workgroup
constexpr uint32_t RT_SLOTS = 1024;                                   // per-workgroup words in LDS: reads first .. first + 1023 of the tile

uint32_t read_trim_tiles(uint64_t n_bases) { return (uint32_t)((n_bases + RT_TILE - 1) / RT_TILE); }

struct RtLds {
    uint32_t mn[RT_SLOTS], mx[RT_SLOTS];
    uint64_t read[2];
};

__device__ inline void rt_put(RtLds& s, uint32_t* __restrict__ gmin, uint32_t* __restrict__ gmax, uint64_t n_reads, uint64_t first, uint64_t read, uint32_t lo, uint32_t hi1)
{
    if (read >= n_reads || read < first) return;
    if (read - first < RT_SLOTS) {
        atomicMin(&s.mn[read - first], lo);
        atomicMax(&s.mx[read - first], hi1);
    } else {
        atomicMin(&gmin[read], lo);
        atomicMax(&gmax[read], hi1);
    }
}

__global__ __launch_bounds__(RT_THREADS) void trim_points_kernel(const uint8_t* __restrict__ qual, uint32_t bias, const uint64_t* __restrict__ offsets,
    const uint8_t* __restrict__ rev, uint64_t n_reads, uint64_t n_bases, uint64_t front, uint64_t tail, uint32_t qual_milli, uint32_t W, uint32_t* __restrict__ gmin,
    uint32_t* __restrict__ gmax, unsigned long long* __restrict__ bad_at)
{
    __shared__ RtLds s;
    const uint64_t tile = (uint64_t)blockIdx.x * RT_TILE;
    if (tile >= n_bases) return; // (uniform)
    const uint64_t tile_end = n_bases - tile > RT_TILE ? tile + RT_TILE : n_bases;
    for (uint32_t i = threadIdx.x; i < RT_SLOTS; i += RT_THREADS) {
        s.mn[i] = RT_NONE;
        s.mx[i] = 0;
    }
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 128) { // (two whole waves) the reads that hold the tile's first and last byte, as read_qual_kernel finds them
        const uint64_t at = threadIdx.x < 64 ? tile : tile_end - 1;
        const uint64_t i = first_at_least(offsets, n_reads, at + 1, lane);
        if (lane == 0) s.read[threadIdx.x >> 6] = i ? i - 1 : 0;
    }
    __syncthreads();
    const uint64_t first = s.read[0], last = s.read[1];
    const bool aligned = (reinterpret_cast<uintptr_t>(qual) & 15u) == 0;
    const uint32_t thr = rt_window_threshold(qual_milli, bias, W);
    uint64_t bad = ~0ull;
    uint4 v[RT_ROUNDS];
#pragma unroll
    for (int round = 0; round < RT_ROUNDS; ++round) {
        const uint64_t p = tile + ((uint64_t)round * RT_THREADS + threadIdx.x) * RT_LANE_STARTS;
        v[round] = aligned && p < tile_end ? load_once_16(qual + p) : make_uint4(0, 0, 0, 0); // (the buffer is padded: the 16 bytes at p < n_bases are readable)
    }
#pragma unroll
    for (int round = 0; round < RT_ROUNDS; ++round) {
        const uint64_t p = tile + ((uint64_t)round * RT_THREADS + threadIdx.x) * RT_LANE_STARTS;
        const bool live = p < tile_end;
        uint32_t w[RT_LANE_WORDS];
        if (aligned) {
            // the 32 bytes behind the lane's own: the next two lanes' loads; on the wave's last two lanes, the buffer itself (p < n_bases, so
            // p + 48 <= n_bases + 47: inside the padding)
            const uint4 a = v[round];
            uint4 b, c;
            b.x = __shfl_down(a.x, 1); b.y = __shfl_down(a.y, 1); b.z = __shfl_down(a.z, 1); b.w = __shfl_down(a.w, 1);
            if (lane == 63 && live && W > 1) b = *reinterpret_cast<const uint4*>(qual + p + 16);
            c = make_uint4(0, 0, 0, 0);
            if (W > 17) { // (uniform)
                c.x = __shfl_down(b.x, 1); c.y = __shfl_down(b.y, 1); c.z = __shfl_down(b.z, 1); c.w = __shfl_down(b.w, 1);
                if (lane == 63 && live) c = *reinterpret_cast<const uint4*>(qual + p + 32);
            }
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
            w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < RT_LANE_WORDS; ++k) w[k] = 0;
            if (live)
                for (uint32_t j = 0; j < RT_LANE_STARTS + W - 1; ++j) // byte by byte, and never behind n_bases: such a buffer promises no padding
                    if (p + j < n_bases) w[j >> 2] |= (uint32_t)qual[p + j] << (8 * (j & 3));
        }
        uint32_t key = RT_NONE, lo = RT_NONE, hi1 = 0;
        if (live) {
            const uint32_t n = (uint32_t)(tile_end - p < RT_LANE_STARTS ? tile_end - p : RT_LANE_STARTS);
            // the range test on four bytes at once; the first bad byte is looked for only where there is one (and in the buffer's last piece,
            // whose padding fails the test under a bias)
            if (rt_bad_bytes(w[0], bias) | rt_bad_bytes(w[1], bias) | rt_bad_bytes(w[2], bias) | rt_bad_bytes(w[3], bias)) {
                uint32_t bad_bits = 0;
#pragma unroll
                for (uint32_t j = 0; j < RT_LANE_STARTS; ++j) {
                    const uint32_t q = ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) - bias; // (below the bias: wraps to a large value)
                    bad_bits |= (q > RT_MAX_QUAL ? 1u : 0u) << j;
                }
                bad_bits &= (1u << n) - 1u;
                if (bad_bits) {
                    const uint64_t at = p + (uint64_t)(__ffs(bad_bits) - 1);
                    if (at < bad) bad = at;
                }
            }
            const uint32_t good = rt_good_bits(w, W, thr);
            uint64_t r = read_holding(offsets, first, last, p);
            rt_piece(offsets, rev, n_reads, n_bases, p, n, good, W, front, tail, r, [&](uint64_t read, uint32_t f, uint32_t l1) {
                if (read < first || read - first >= 0xFFFFFFFFull) return;
                if (key == RT_NONE) { // the lane's first read with a window: kept for the wave's reduction
                    key = (uint32_t)(read - first);
                    lo = f;
                    hi1 = l1;
                } else rt_put(s, gmin, gmax, n_reads, first, read, f, l1);
            });
        }
        // One read under every lane of the wave that found a window (every wave inside a long read): min and max in registers, one lane
        // hands them over.  Otherwise every lane hands over its own.
        uint32_t kmin = key;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_xor(kmin, off);
            kmin = o < kmin ? o : kmin;
        }
        if (kmin == RT_NONE) continue; // (uniform: no lane found a window)
        if (__all(key == kmin || key == RT_NONE)) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t a = __shfl_xor(lo, off), b = __shfl_xor(hi1, off);
                lo = a < lo ? a : lo;
                hi1 = b > hi1 ? b : hi1;
            }
            if (lane == 0) rt_put(s, gmin, gmax, n_reads, first, first + kmin, lo, hi1);
            continue;
        }
        if (key != RT_NONE) rt_put(s, gmin, gmax, n_reads, first, first + key, lo, hi1);
    }
    if (bad != ~0ull) atomicMin(bad_at, (unsigned long long)(bad + 1));
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < RT_SLOTS; i += RT_THREADS) {
        const uint32_t a = s.mn[i], b = s.mx[i];
        if (b && first + i < n_reads) {
            atomicMin(&gmin[first + i], a);
            atomicMax(&gmax[first + i], b);
        }
    }
}

// begin[i], end[i]: the kept range of read i in READ orientation; klen[i] = its length (entry n_reads: 0); the counts into work[RT_*];
// work[RT_OFFSETS] is set when the offsets do not ascend to n_bases or a read is too long for the 32-bit starts.
__global__ __launch_bounds__(RT_THREADS) void trim_tables_kernel(ReadTrimArgs a)
{
    __shared__ unsigned long long s_n[6];
    if (threadIdx.x < 6) s_n[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (i == a.n_reads) {
        a.klen[i] = 0;
        if (a.offsets[i] != a.n_bases) a.work[RT_OFFSETS] = 1;
    }
    if (i < a.n_reads) {
        const uint64_t s = a.offsets[i], e = a.offsets[i + 1];
        uint64_t x = 0, y = 0; // the kept range, read orientation
        if (e < s || e > a.n_bases || e - s >= RT_MAX_READ) a.work[RT_OFFSETS] = 1;
        else {
            const uint64_t L = e - s;
            const bool rev = a.rev && a.rev[i];
            uint64_t lo, hi; // stored order
            rt_crop(L, a.front, a.tail, rev, lo, hi);
            uint64_t p = lo, q = hi;
            if (a.qual_milli) rt_range(a.qual + s, lo, hi, a.first[i], a.last[i], a.window, a.bias, a.qual_milli, p, q);
            else if (p >= q) p = q = 0;
            // the counts, in read orientation: what the crop took at either end, and what the quality took inside the cropped range (a read
            // without a good window: all of it, counted at the front)
            const uint64_t a0 = rev ? L - hi : lo, b0 = rev ? L - lo : hi;
            x = rev ? (q > p ? L - q : 0) : p;
            y = rev ? (q > p ? L - p : 0) : q;
            const uint64_t qf = y > x ? x - a0 : b0 - a0, qt = y > x ? b0 - y : 0;
            if (y - x != L) atomicAdd(&s_n[0], 1ull);
            if (a0) atomicAdd(&s_n[1], (unsigned long long)a0);
            if (L - b0) atomicAdd(&s_n[2], (unsigned long long)(L - b0));
            if (qf) atomicAdd(&s_n[3], (unsigned long long)qf);
            if (qt) atomicAdd(&s_n[4], (unsigned long long)qt);
            if (L && y == x) atomicAdd(&s_n[5], 1ull);
        }
        a.begin[i] = x;
        a.end[i] = y;
        a.klen[i] = y - x;
    }
    __syncthreads();
    if (threadIdx.x < 6 && s_n[threadIdx.x]) atomicAdd(&a.work[RT_LOST_READS + threadIdx.x], s_n[threadIdx.x]);
}

// everything into `out` (page-locked host memory, or device memory); n_kept_npos: null, or the count trim_npos_kernel's scan left
__global__ void read_trim_result_kernel(ReadTrimArgs a, const uint32_t* __restrict__ n_kept_npos)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    a.out[RT_KEPT_BASES] = a.noff[a.n_reads];
    for (int k = RT_LOST_READS; k <= RT_EMPTIED; ++k) a.out[k] = a.work[k];
    for (int k = RT_AD_BASES_SEEN; k <= RT_PT_EMPTIED; ++k) a.out[k] = a.work[k];
    a.out[RT_BAD_AT] = a.work[RT_OFFSETS] ? ~0ull : (a.work[RT_BAD_AT] == ~0ull ? 0ull : a.work[RT_BAD_AT]);
    a.out[RT_KEPT_NPOS] = n_kept_npos ? *n_kept_npos : 0;
}

// Where every trimmed read starts in the old block: src_start (packed blocks: launch_subsample_pack), a GatherEntry for its bases (ASCII
// blocks) and one for its quality bytes, which stay in stored order; each may be null.
__global__ __launch_bounds__(RT_THREADS) void trim_fill_kernel(ReadTrimFill f)
{
    const uint64_t i = (uint64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (i >= f.n_reads) return;
    const uint64_t s = f.offsets[i], e = f.offsets[i + 1], x = f.begin[i], y = f.end[i], at = f.noff[i];
    const bool ok = s <= e && e <= f.n_bases && x <= y && y <= e - s && y - x < RT_MAX_READ && at + (y - x) <= f.new_bases && f.noff[i + 1] == at + (y - x);
    if (!ok) *f.err = 1;
    const uint64_t L = ok ? e - s : 0;
    const uint32_t len = ok ? (uint32_t)(y - x) : 0u;
    if (f.src_start) f.src_start[i] = ok ? s + x : 0;
    if (f.btable) f.btable[i] = GatherEntry { f.bases + (ok ? s + x : 0), ok ? at : 0, len, 0 };
    if (f.qtable) {
        const uint64_t sb = f.rev && f.rev[i] ? L - y : x; // the range's first byte in stored order
        f.qtable[i] = GatherEntry { f.qual + (ok && len ? s + sb : 0), ok ? at : 0, len, 0 };
    }
}

// The block's listed positions that lie inside kept ranges, at their new places.  EMIT == false: chunk_count[workgroup] = how many of its
// RT_THREADS entries stay.  EMIT == true: they are written, ascending, from chunk_prefix[workgroup] on (below out_cap).
template <bool EMIT>
__global__ __launch_bounds__(RT_THREADS) void trim_npos_kernel(ReadTrimFill f, const uint64_t* __restrict__ npos, uint64_t n_npos, uint32_t* __restrict__ chunk_count,
    const uint32_t* __restrict__ chunk_prefix, uint64_t* __restrict__ out, uint64_t out_cap)
{
    __shared__ uint32_t s_w[RT_THREADS / 64 + 1];
    if (EMIT && chunk_prefix[blockIdx.x + 1] == chunk_prefix[blockIdx.x]) return; // (uniform)
    const uint64_t t = (uint64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    uint32_t keep = 0;
    uint64_t to = 0;
    if (t < n_npos) {
        const uint64_t q = npos[t];
        if (q < f.n_bases) {
            const uint64_t j = read_holding(f.offsets, 0, f.n_reads - 1, q);
            const uint64_t s = f.offsets[j];
            if (s <= q && q < f.offsets[j + 1]) {
                const uint64_t x = f.begin[j], y = f.end[j];
                if (q - s >= x && q - s < y) {
                    keep = 1;
                    to = f.noff[j] + (q - s - x);
                }
            }
        }
    }
    uint32_t total = 0;
    const uint32_t before = block_exclusive_scan<RT_THREADS / 64>(keep, s_w, &total);
    if (!EMIT) {
        if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
        return;
    }
    const uint64_t at = (uint64_t)chunk_prefix[blockIdx.x] + before;
    if (keep && at < out_cap && to < f.new_bases) out[at] = to;
}

size_t read_trim_temp_bytes(uint64_t n_reads)
{
    size_t a = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>(), (hipStream_t)0);
    return a;
}

uint32_t read_trim_npos_chunks(uint64_t n_npos) { return (uint32_t)((n_npos + RT_THREADS - 1) / RT_THREADS); }

hipError_t launch_read_trim(const ReadTrimArgs& a, const ReadTrimNpos& np, hipStream_t stream, KernelTimer timer, const AdapterEditSets* edit)
{
    if (!a.n_reads || a.n_reads > MAX_BATCH_READS) return hipErrorInvalidValue;
    if (a.qual_milli && (a.window < 1 || a.window > RT_MAX_WINDOW || a.qual_milli > RT_MAX_QUAL_MILLI)) return hipErrorInvalidValue;
    size_t temp_bytes = a.temp_bytes; // (rocPRIM takes it by reference)
    HIP_TRY(hipMemsetAsync(a.work, 0, RT_WORDS * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(a.work + RT_BAD_AT, 0xFF, sizeof(unsigned long long), stream));
    const uint32_t n_tiles = read_trim_tiles(a.n_bases);
    if (a.qual_milli) {
        HIP_TRY(hipMemsetAsync(a.first, 0xFF, a.n_reads * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(a.last, 0, a.n_reads * sizeof(uint32_t), stream));
        if (n_tiles) {
            launch_timed(timer, trim_points_kernel, dim3(n_tiles), dim3(RT_THREADS), 0, stream, a.qual, a.bias, a.offsets, a.rev, a.n_reads, a.n_bases, a.front, a.tail,
                a.qual_milli, a.window, a.first, a.last, a.work + RT_BAD_AT);
            HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(trim_tables_kernel, dim3((uint32_t)((a.n_reads + 1 + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    if (edit || a.ad.n || a.poly_letters) { // adapter trimming, then poly tails: on the ranges the tables kernel left, before the new lengths are scanned
        AdapterPoints pts = a.pts;
        pts.offsets = a.offsets; pts.begin = a.begin; pts.end = a.end; pts.n_reads = a.n_reads; pts.n_bases = a.n_bases;
        if (edit) HIP_TRY(launch_adapter_edit(pts, edit->ad3, edit->eq3, edit->ad5, edit->eq5, a.begin, a.end, a.klen, a.work, stream)); // (adapter_edit.hip: 3', then 5')
        else if (a.ad.n) HIP_TRY(launch_adapter_trim(pts, a.ad, a.end, a.klen, a.work, stream));                            // (adapter_trim.hip)
        if (a.poly_letters) HIP_TRY(launch_poly_tail(pts, a.poly_letters, a.poly_min_len, a.end, a.klen, a.work, stream));  // (poly_tail.hip)
    }
    HIP_TRY(rocprim::exclusive_scan(a.temp, temp_bytes, a.klen, a.noff, (uint64_t)0, (size_t)a.n_reads + 1, rocprim::plus<uint64_t>(), stream));
    const uint32_t* kept_npos = nullptr;
    if (np.n_npos) { // how many listed positions stay: counted before the host looks, so that the block costs one read-back
        const ReadTrimFill f { a.offsets, a.rev, a.begin, a.end, a.noff, a.n_reads, a.n_bases, ~0ull, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
        HIP_TRY(launch_read_trim_npos_count(f, np, stream));
        kept_npos = np.chunk_prefix + read_trim_npos_chunks(np.n_npos);
    }
    hipLaunchKernelGGL(read_trim_result_kernel, dim3(1), dim3(64), 0, stream, a, kept_npos);
    return hipGetLastError();
}

hipError_t launch_read_trim_npos_count(const ReadTrimFill& f, const ReadTrimNpos& np, hipStream_t stream)
{
    const uint32_t n_chunks = read_trim_npos_chunks(np.n_npos);
    if (!n_chunks || !f.n_reads) return hipErrorInvalidValue;
    hipLaunchKernelGGL(trim_npos_kernel<false>, dim3(n_chunks), dim3(RT_THREADS), 0, stream, f, np.npos, np.n_npos, np.chunk_count, (const uint32_t*)nullptr,
        (uint64_t*)nullptr, 0ull);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(np.chunk_count + n_chunks, 0, sizeof(uint32_t), stream));
    return exclusive_scan_u32(np.temp, np.temp_bytes, np.chunk_count, np.chunk_prefix, n_chunks + 1, stream);
}

hipError_t launch_read_trim_fill(const ReadTrimFill& f, hipStream_t stream)
{
    if (!f.n_reads) return hipSuccess;
    hipLaunchKernelGGL(trim_fill_kernel, dim3((uint32_t)((f.n_reads + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, stream, f);
    return hipGetLastError();
}

hipError_t launch_read_trim_npos_emit(const ReadTrimFill& f, const ReadTrimNpos& np, uint64_t* out, uint64_t out_cap, hipStream_t stream)
{
    const uint32_t n_chunks = read_trim_npos_chunks(np.n_npos);
    if (!n_chunks || !f.n_reads || !out_cap) return hipSuccess;
    hipLaunchKernelGGL(trim_npos_kernel<true>, dim3(n_chunks), dim3(RT_THREADS), 0, stream, f, np.npos, np.n_npos, (uint32_t*)nullptr, (const uint32_t*)np.chunk_prefix, out,
        out_cap);
    return hipGetLastError();
}

} // namespace dev
} // namespace drprg
