// mapper.cpp -- device context and per-batch launch sequence.  See mapper.h.
#include "mapper.h"
#include <algorithm>
#include <cmath>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <set>
#include <hip/hip_runtime.h>
#include <sys/mman.h>

namespace drprg {

// counter slots
enum { C_HITS = 0, C_MINIMIZERS = 1, C_CLUSTERS_KEPT = 2, C_HITS_KEPT = 3, C_OVERFLOW = 4, C_MAXLEN = 5, C_UNSORTED = 6, C_COMPLEX = 7, C_N = 8 };
// reads up to this length get their hits reordered per read (read_inversion_kernel, read_fix_kernel); longer ones take the radix sort
constexpr uint64_t READ_SORT_MAX_LEN = 512;
// candidate buffers of the filtered sequence: one entry per this many bases of the batch.  One per 64 is laid out by the tile; the quarter
// added on top is kept for the small chunks of a dynamic schedule's last round (sketch_filter.hip launch_sketch_filter)
constexpr uint64_t FILTER_BASES_PER_ENTRY = 48;

void Mapper::IndexTables::fill(const FlatIndex& idx, bool wide_hash, uint64_t mid_max_records)
{
    const size_t nslot = idx.slot_key.size(), nrec = idx.rec_prg.size();
    // what the kernels cannot address is refused here, on the host index, before the first allocation
    if (idx.min_path_len.size() > dev::MAX_PRGS) throw Error(DRPRG_EOVERFLOW, "more than " + std::to_string(dev::MAX_PRGS) + " PRGs");
    for (size_t i = 0; i < nslot; ++i)
        if (idx.slot_cnt[i] && idx.min_path_len[idx.rec_prg[idx.slot_off[i]]] >= (1u << 20))
            throw Error(DRPRG_EOVERFLOW, "a PRG's shortest k-mer path has 2^20 nodes or more");
    if (idx.total_knodes() >= (1u << 31)) throw Error(DRPRG_EOVERFLOW, "too many k-mer nodes");
    table_bits = idx.table_bits;
    if (wide_hash) {
        std::vector<uint64_t> k64(nslot);
        for (size_t i = 0; i < nslot; ++i) k64[i] = idx.slot_cnt[i] ? idx.slot_key[i] : ~0ULL; // empty-slot sentinel
        slot_key.upload(reinterpret_cast<const unsigned char*>(k64.data()), nslot * sizeof(uint64_t));
    } else {
        std::vector<uint32_t> k32(nslot);
        for (size_t i = 0; i < nslot; ++i) k32[i] = idx.slot_cnt[i] ? (uint32_t)idx.slot_key[i] : 0xFFFFFFFFu; // empty-slot sentinel
        slot_key.upload(reinterpret_cast<const unsigned char*>(k32.data()), nslot * sizeof(uint32_t));
    }
    std::vector<uint2> rec(nslot);
    std::vector<uint4> first(nslot);
    for (size_t i = 0; i < nslot; ++i) {
        rec[i] = make_uint2(idx.slot_off[i], idx.slot_cnt[i]);
        first[i] = make_uint4(idx.slot_off[i], idx.slot_cnt[i], 0u, 0u);
        if (idx.slot_cnt[i]) {
            const uint32_t r = idx.slot_off[i], prg = idx.rec_prg[r];
            first[i].z = (idx.rec_knode_global[r] << 1) | idx.rec_strand[r];
            first[i].w = prg | (idx.min_path_len[prg] << 12);
        }
    }
    slot_rec.upload(rec);
    slot_first.upload(first);
    std::vector<uint32_t> rk(nrec);
    std::vector<uint16_t> rp(nrec);
    for (size_t i = 0; i < nrec; ++i) {
        rk[i] = (idx.rec_knode_global[i] << 1) | idx.rec_strand[i];
        rp[i] = (uint16_t)idx.rec_prg[i];
    }
    rec_knode.upload(rk);
    rec_prg.upload(rp);
    min_path_len.upload(idx.min_path_len);
    h_min_path_len = idx.min_path_len;
    prg_thr.alloc(idx.min_path_len.size()); // (filled by set_params)
    // Bloom tier of the direct kernel: only when keys + slot records outgrow an XCD's 4 MB L2 (<= ~4 keys per 32-bit word)
    if (nslot * (size_t)(wide_hash ? 16 : 12) > ((size_t)2 << 20)) {
        pbloom_wbits = 10;
        while (((size_t)4 << pbloom_wbits) < idx.keys.size()) ++pbloom_wbits;
        std::vector<uint32_t> pb((size_t)1 << pbloom_wbits, 0);
        for (uint64_t key : idx.keys) {
            const uint32_t m = dev::pbloom_mix(key);
            pb[dev::pbloom_word(m, pbloom_wbits)] |= dev::pbloom_bits(m);
        }
        pbloom.upload(pb);
    }
    bloom_wbits = idx.bloom_wbits;
    if (bloom_wbits) bloom.upload(idx.bloom);
    bloom0_wbits = bloom_wbits ? idx.bloom0_wbits : 0;
    if (bloom0_wbits) {
        bloom0.upload(idx.bloom0);
        bloom0f.upload(idx.bloom0f);
        bloomr.upload(idx.bloomr);
        if (idx.blkc_wbits) { // the second stage for the L2 (round 6)
            blkc_wbits = idx.blkc_wbits;
            blkc.upload(idx.blkc);
        }
    }
    if (idx.midc_wbits && nrec <= mid_max_records) { // (switches.h: where the direct sequence takes over)
        midc_wbits = idx.midc_wbits;
        mid0_bits = idx.mid0_bits;
        mid0.upload(idx.mid0);
        mid_bitmap.upload(idx.mid_bitmap);
        midc.upload(idx.midc);
    }
    HIPCHK(hipStreamSynchronize(nullptr)); // every table is on the device before a kernel of a non-blocking stream can ask for it
}

dev::BloomTables Mapper::IndexTables::bloom_tables(bool mid) const
{
    dev::BloomTables bt { bloom.data(), bloom_wbits, bloom0.data(), bloom0_wbits, bloomr.data(), bloom0f.data() };
    bt.blkc = blkc.data();
    bt.blkc_wbits = blkc_wbits;
    if (mid) {
        bt.mid0 = mid0.data();
        bt.mid_bitmap = mid_bitmap.data();
        bt.midc = midc.data();
        bt.midc_wbits = midc_wbits;
        bt.mid0_bits = mid0_bits;
    }
    return bt;
}

Mapper::Mapper(const FlatIndex& idx, const MapParams& p, int device) : device_(device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        throw Error(DRPRG_ENODEV, "no HIP device is visible: the drprg hot path has no CPU fallback");
    if (device < 0 || device >= ndev) throw Error(DRPRG_ENODEV, "HIP device " + std::to_string(device) + " does not exist");
    HIPCHK(hipSetDevice(device_));
    n_prgs_ = (uint32_t)idx.min_path_len.size();
    n_knodes_ = idx.total_knodes();
    tables_.fill(idx, p.k > 15, sw_.mid_max_records);
    stream_.create();
    HIPCHK(hipDeviceGetAttribute(&n_cus_, hipDeviceAttributeMultiprocessorCount, device_));
    set_params(p); // (behind the tables: the kernel choice depends on the filter being available)
    if (sw_.min_capacity) // (tests: small batches at the production ratio, or below it to force regrows)
        min_capacity_ = std::max<uint64_t>(MIN_CAPACITY_CLAMP, std::min<uint64_t>(*sw_.min_capacity, 1ull << 30));
    // ONE allocation [coverage | reads per PRG]: the sample's whole additive state is one contiguous u32 vector, so the
    // collective of the path is a single ncclAllReduce / ncclReduce over it (capi_reduce.cpp)
    d_covg_.alloc(2 * (size_t)n_knodes_ + (size_t)n_prgs_);
    d_counters_.alloc(C_N);
    h_counters_.alloc(C_N);
    ev0_.create(true);
    ev1_.create(true);
    reset_coverage();
}

// The owners free everything; what is left to say is the order: nothing is in flight when they do.
Mapper::~Mapper()
{
    (void)hipSetDevice(device_);
    try {
        sync();
    } catch (...) { // (nothing to report to from a destructor)
    }
    (void)hipDeviceSynchronize();
}

// Zeroes device memory and returns when it IS zero.  hipMemset on device memory runs on the null stream and may return before it
// has run; this class's streams are non-blocking, so nothing they do waits for the null stream -- a freshly allocated cand_pos1
// was zeroed AFTER the verification kernel had written the first batch into it (cold start, several contexts busy on one device:
// one run in ten lost 5 % of its clusters; tools/stress_multi.py).
void Mapper::zero_now(void* p, size_t bytes)
{
    HIPCHK(hipMemsetAsync(p, 0, bytes, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
}

static std::mutex g_pinned_mu;
static std::set<void*> g_pinned_by_runtime; // blocks that came from hipHostMalloc (pinned_alloc's second choice)

// Page-locked memory for the ingest's parser threads.  Portable: they call this with whatever device is current on their
// thread, and a portable registration is page-locked for every device, so the copy engine of the mapper's device takes it at
// DMA speed.  Ordinary memory (2 MB aligned, transparent huge pages asked for), touched by the calling thread and THEN
// registered: measured on the MI355X box for 32 threads x 32 MB, hipHostMalloc pins at 6.7 GB/s (161 ms), touch +
// hipHostRegister takes 5 + 13 ms, and host -> device copies run at the same 56 GB/s from both (tools/mb_pin.cpp,
// profiles/r03/mb_pin.txt).
void* Mapper::pinned_alloc(size_t bytes)
{
    constexpr size_t HUGE = 2u << 20;
    const size_t n = (bytes + HUGE - 1) / HUGE * HUGE;
    void* p = std::aligned_alloc(HUGE, n);
    if (!p) return nullptr;
    (void)madvise(p, n, MADV_HUGEPAGE);
    for (size_t i = 0; i < n; i += 4096) static_cast<volatile char*>(p)[i] = 0;
    if (hipHostRegister(p, n, hipHostRegisterPortable) != hipSuccess) {
        // (a host that refuses the registration -- a limit on locked pages, an old driver --: the runtime's own allocation, slower to get)
        (void)hipGetLastError();
        std::free(p);
        p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        std::lock_guard<std::mutex> g(g_pinned_mu);
        g_pinned_by_runtime.insert(p);
    }
    return p;
}

void Mapper::pinned_free(void* p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_pinned_mu);
        if (g_pinned_by_runtime.erase(p)) {
            (void)hipHostFree(p);
            return;
        }
    }
    (void)hipHostUnregister(p);
    std::free(p);
}

// First HIP call of a process: tens to hundreds of milliseconds of runtime start-up.  drprg_hip_open runs this on a thread of
// its own while the index files are read; errors are left to the Mapper constructor, which reports them.
void Mapper::warm_device(int device)
{
    if (hipSetDevice(device) == hipSuccess) (void)hipFree(nullptr);
}

void Mapper::set_params(const MapParams& p)
{
    sync(); // (a batch in flight was launched with the previous parameters)
    // validate everything before any state changes: a refused call leaves the previous parameters in force
    PrgIndex::check_wk(p.w, p.k);
    const bool filter_ok = (tables_.bloom_wbits != 0 || tables_.midc_wbits != 0) && p.k <= 15 && p.w <= 16;
    if (p.kernel_mode < 0 || p.kernel_mode > 3) throw Error(DRPRG_EINVAL, "kernel must be 0 (auto), 1, 2 or 3");
    if (p.kernel_mode == 2 && !filter_ok)
        throw Error(DRPRG_EINVAL, "the Bloom-prefiltered kernel needs k <= 15, w <= 16 and an index small enough for its filter tiers");
    params_ = p;
    wide_hash_ = p.k > 15;
    halo_ = std::max(16, ((p.w - 1 + 15) / 16) * 16);
    { // the PRG's share of the cluster size threshold, in the oracle's own arithmetic
        std::vector<uint32_t> thr(n_prgs_);
        const double fraction = params_.cluster_fraction();
        for (uint32_t i = 0; i < n_prgs_; ++i) thr[i] = (uint32_t)((double)tables_.h_min_path_len[i] * fraction);
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipMemcpy(tables_.prg_thr.data(), thr.data(), n_prgs_ * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(hipStreamSynchronize(nullptr)); // (the copies of this file run on the null stream, which the non-blocking streams do not wait for)
    }
    use_filter_ = p.kernel_mode == 2 || (p.kernel_mode == 0 && filter_ok);
    use_mid_ = use_filter_ && tables_.bloom_wbits == 0;
    use_direct_cands_ = p.kernel_mode == 3 || (p.kernel_mode == 0 && !filter_ok);
}

void Mapper::reset_coverage(bool new_sample)
{
    sync();
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipMemsetAsync(d_covg_.data(), 0, d_covg_.bytes(), stream_)); // [coverage | reads per PRG]
    HIPCHK(hipMemsetAsync(d_counters_.data(), 0, d_counters_.bytes(), stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    tot_reads_ = tot_bases_ = tot_hits_ = tot_leftover_ = tot_minimizers_ = 0;
    bam_blocks_ = 0;
    for (auto& sh : ft_share_) // (a reset context starts from the launcher's built-in tile shares again: ADVICE r05)
        for (uint32_t& v : sh) v = 0;
    sw_ = read_switches(); // (those that only shape construction keep their effect from the open)
    if (new_sample) {
        drop_kept();
        for (int w = 0; w < 2; ++w) { // the read statistics are the sample's
            if (stats_.acc[w]) HIPCHK(dev::launch_read_stats_clear(stats_.acc[w].data(), stream_));
            stats_.empty_reads[w] = 0;
        }
        HIPCHK(hipStreamSynchronize(stream_));
    }
}

void Mapper::ensure_workspace(uint64_t cap)
{
    if (cap <= hit_capacity()) return;
    if (cap >= (1ull << 31)) throw Error(DRPRG_EOVERFLOW, "more than 2^31 minimizer hits in one batch; map smaller batches");
    d_key_a_.alloc(cap); d_key_b_.alloc(cap); d_val_a_.alloc(cap); d_val_b_.alloc(cap);
    d_head_.alloc(cap); d_scan_.alloc(cap); d_cstart_.alloc(cap + 1); d_order_.alloc(cap);
    d_clusters_.alloc(cap);
    d_temp_.alloc(std::max(dev::sort_temp_bytes((uint32_t)cap), dev::scan_temp_bytes((uint32_t)cap)));
}

void Mapper::grow_lane(Lane& lane, uint64_t cap)
{
    if (cap <= lane.capacity()) return;
    if (cap >= (1ull << 31)) throw Error(DRPRG_EOVERFLOW, "more than 2^31 candidate k-mers in one batch; map smaller batches");
    lane.raw_pos.alloc(cap); lane.cand_info.alloc(cap); lane.cand_pos1.alloc(cap); lane.cand_rec.alloc(cap);
    // the slices form of the direct sequence uses cand_pos1 as an array of "handled" marks (mark = a batch's epoch): fresh device
    // memory may hold anything, including a value some later epoch of this or an earlier Mapper takes
    zero_now(lane.cand_pos1.data(), lane.cand_pos1.bytes());
}

// Both lanes' events, counters and their pinned mirror; the candidate buffers grow with the batches (grow_lane).
void Mapper::ensure_lanes()
{
    for (Lane& lane : lanes_) {
        if (lane.h_scratch) continue; // (the last thing a lane gets)
        lane.done.create(false);
        lane.t0.create(true);
        lane.t1.create(true);
        lane.small.alloc(dev::filter_small_words());
        zero_now(lane.small.data(), lane.small.bytes()); // (the superblock counts start at zero; every sequence leaves them so)
        lane.d_scratch.alloc(L_N);
        zero_now(lane.d_scratch.data(), lane.d_scratch.bytes());
        lane.scratch_zero = true;
        lane.h_scratch.alloc(L_N);
    }
}

Mapper::Batch Mapper::make_batch(int lane, const DeviceBatch& batch, uint32_t* covg, uint32_t* prg_reads, hipStream_t stream) const
{
    return Batch { batch, true, !use_filter_, lane, covg, prg_reads, stream }; // (direct: the callers run only the two candidate sequences)
}

void Mapper::launch(const Batch& b)
{
    ensure_lanes();
    if (b.direct) direct_launch(b);
    else filter_launch(b);
    HIPCHK(hipEventRecord(lanes_[b.lane].done, b.stream));
}

void Mapper::count_on_lane(dev::SketchArgs& a, const Lane& lane) const
{
    a.n_hits = lane.d_scratch.data() + L_HITS;
    a.n_minimizers = lane.d_scratch.data() + L_MINIMIZERS;
    a.overflow = reinterpret_cast<uint32_t*>(lane.d_scratch.data() + L_OVERFLOW);
}

dev::FilterBuffers Mapper::filter_buffers(const Lane& lane) const
{
    return dev::FilterBuffers { lane.raw_pos.data(), lane.cand_info.data(), lane.cand_pos1.data(), lane.cand_rec.data(), lane.capacity(), lane.small.data(),
        lane.d_scratch.data() + L_MAXLEN };
}

dev::ReadClusterArgs Mapper::read_cluster_args(const Batch& b) const
{
    const Lane& lane = lanes_[b.lane];
    dev::ReadClusterArgs rc {};
    rc.prg_min_path_len = tables_.min_path_len.data();
    rc.fraction = params_.cluster_fraction();
    rc.min_cluster_size = params_.min_cluster_size;
    rc.max_diff = params_.max_diff;
    rc.n_prgs = n_prgs_;
    rc.covg = b.covg;
    rc.prg_reads = b.prg_reads;
    rc.n_clusters_kept = d_counters_.data() + C_CLUSTERS_KEPT;
    rc.n_hits_kept = d_counters_.data() + C_HITS_KEPT;
    rc.n_complex = lane.d_scratch.data() + L_COMPLEX;
    rc.chunk_counter = reinterpret_cast<uint32_t*>(lane.d_scratch.data() + L_CHUNK);
    return rc;
}

dev::KernelTimer Mapper::kernel_timer(hipEvent_t t0, hipEvent_t t1) const
{
    dev::KernelTimer timer;
    if (timing_) { // events bracket the dominant kernel only
        timer.begin = t0;
        timer.end = t1;
    }
    return timer;
}

// One filtered sequence, asynchronous on the batch's stream: kernels, then the lane's counters to its pinned mirror, then the counters
// cleared again behind the copy (so that the next batch starts with its first kernel instead of a memset).
void Mapper::filter_launch(const Batch& b)
{
    Lane& lane = lanes_[b.lane];
    // (a deferred batch: this lane's previous batch was completed by the call before this one; growing frees its buffers, which waits for the device)
    grow_lane(lane, std::max<uint64_t>(min_capacity_, b.batch.n_bases / FILTER_BASES_PER_ENTRY));
    if (!lane.scratch_zero) HIPCHK(hipMemsetAsync(lane.d_scratch.data(), 0, lane.d_scratch.bytes(), b.stream));
    lane.scratch_zero = false;
    dev::SketchArgs a = sketch_args(b.batch, nullptr);
    count_on_lane(a, lane);
    dev::FilterBuffers fb = filter_buffers(lane);
    fb.class_clock = lane.d_scratch.data() + L_FT_CLOCK; // (unused when DRPRG_FT_SHARE pins the shares: then nothing adapts them)
    if (ft_share_[b.batch.packed ? 1 : 0][0]) fb.wave_share = ft_share_[b.batch.packed ? 1 : 0];
    HIPCHK(dev::launch_sketch_filter(a, tables_.bloom_tables(use_mid_), n_cus_, fb, read_cluster_args(b), lane.fw, sw_, b.stream, kernel_timer(lane.t0, lane.t1)));
    // the counters to the pinned mirror and zero again behind it: one small kernel (rounds 1-4: a copy and two memsets)
    HIPCHK(dev::launch_counters_home(lane.d_scratch.data(), lane.h_scratch.device_ptr(), L_N, b.stream, dev::filter_super_counts(lane.small.data()), dev::filter_super_words()));
    lane.scratch_zero = true;
}

// Waits for `event` (recorded on `stream`), or -- event null -- for everything queued on `stream`.  The wait polls for a short while first:
// an interrupt-driven synchronise wakes up tens of microseconds late, which is visible at 0.7 ms per batch.  Only for a short while (~2 ms
// of polls): a longer batch does not notice the late wake-up, and a host core that spins for it is a core the FASTQ parser threads (or the
// other ranks of a node) do not have.
static void wait_stream(hipStream_t stream, hipEvent_t event = nullptr)
{
    for (int spins = 0; spins < 2048; ++spins) {
        const hipError_t e = event ? hipEventQuery(event) : hipStreamQuery(stream);
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) HIPCHK(e);
    }
    HIPCHK(event ? hipEventSynchronize(event) : hipStreamSynchronize(stream));
}

// hits in d_key_a_/d_val_a_ -> clusters -> coverage (the generic pipeline).  ordered: the hits are ordered by
// (read, position) already and no read is longer than READ_SORT_MAX_LEN, so a per-read reorder replaces the radix sort.
void Mapper::cluster_hits(const uint64_t* d_offsets, uint32_t n_hits, bool ordered, unsigned long long* d_unsorted, uint32_t* covg,
    uint32_t* prg_reads, hipStream_t stream)
{
    if (n_hits == 0) return;
    const uint64_t* s_key = d_key_b_.data();
    const uint32_t* s_val = d_val_b_.data();
    if (ordered) {
        HIPCHK(dev::launch_read_sort(d_key_a_.data(), d_val_a_.data(), d_key_b_.data(), d_val_b_.data(), n_hits, d_order_.data(), hit_capacity(), d_unsorted, stream));
        s_key = d_key_a_.data();
        s_val = d_val_a_.data();
    } else HIPCHK(dev::sort_hits(d_temp_.data(), d_temp_.size(), d_key_a_.data(), d_key_b_.data(), d_val_a_.data(), d_val_b_.data(), n_hits, stream));
    HIPCHK(dev::launch_cluster_flags(s_key, n_hits, params_.max_diff, d_head_.data(), d_scan_.data(), d_temp_.data(), d_temp_.size(), stream));
    HIPCHK(dev::launch_cluster_starts(d_head_.data(), d_scan_.data(), n_hits, d_cstart_.data(), stream));
    dev::ClusterArgs c {};
    c.key = s_key;
    c.val = s_val;
    c.scan = d_scan_.data();
    c.cstart = d_cstart_.data();
    c.d_n_clusters = d_scan_.data() + (n_hits - 1);
    c.offsets = d_offsets;
    c.prg_min_path_len = tables_.min_path_len.data();
    c.clusters = d_clusters_.data();
    c.order = d_order_.data();
    c.w = params_.w;
    c.fraction = params_.cluster_fraction();
    c.min_cluster_size = params_.min_cluster_size;
    c.covg = covg;
    c.prg_reads = prg_reads;
    c.n_clusters_kept = d_counters_.data() + C_CLUSTERS_KEPT;
    c.n_hits_kept = d_counters_.data() + C_HITS_KEPT;
    HIPCHK(dev::launch_cluster_pipeline(c, n_hits, n_prgs_, stream));
}

dev::SketchArgs Mapper::sketch_args(const DeviceBatch& batch, const TileSet* tiles) const
{
    dev::SketchArgs a {};
    a.bases = batch.d_bases;
    a.offsets = batch.d_offsets;
    a.n_bases = batch.n_bases;
    a.n_reads = (uint32_t)batch.n_reads; // (check: at most 2^28)
    a.w = params_.w;
    a.k = params_.k;
    a.halo = halo_;
    a.slot_key = tables_.slot_key.data();
    a.slot_rec = tables_.slot_rec.data();
    a.slot_first = tables_.slot_first.data();
    a.table_bits = tables_.table_bits;
    a.rec_knode = tables_.rec_knode.data();
    a.rec_prg = tables_.rec_prg.data();
    a.tile_first_read = tiles ? tiles->d_tile_first.data() : nullptr;
    a.pbloom = tables_.pbloom.data();
    a.pbloom_wbits = tables_.pbloom_wbits;
    a.hit_key = d_key_a_.data();
    a.hit_val = d_val_a_.data();
    a.hit_capacity = hit_capacity();
    a.n_hits = d_counters_.data() + C_HITS;
    a.n_minimizers = d_counters_.data() + C_MINIMIZERS;
    a.overflow = reinterpret_cast<uint32_t*>(d_counters_.data() + C_OVERFLOW);
    a.packed = batch.packed ? 1 : 0; // (said by the caller, carried with the batch -- not looked up by its address)
    a.npos = batch.d_npos;
    a.n_npos = batch.n_npos;
    return a;
}

Mapper::DeviceBatch Mapper::ascii_view(int slot, const DeviceBatch& batch, hipStream_t stream)
{
    if (!batch.packed) return batch;
    const uint64_t need = (batch.n_bases + 15) / 16 * 16 + 64;
    if (need > d_unpacked_[slot].size()) {
        sync(); // (a batch in flight may still read the old buffer)
        HIPCHK(hipStreamSynchronize(stream));
        d_unpacked_[slot].alloc(need + need / 4);
    }
    HIPCHK(dev::launch_unpack(reinterpret_cast<const uint32_t*>(batch.d_bases), batch.n_bases, batch.d_npos, batch.n_npos, d_unpacked_[slot].data(), stream));
    return DeviceBatch { d_unpacked_[slot].data(), batch.d_offsets, batch.n_reads, batch.n_bases };
}

void Mapper::read_counters(hipStream_t stream)
{
    HIPCHK(hipMemcpyAsync(h_counters_.data(), d_counters_.data(), d_counters_.bytes(), hipMemcpyDeviceToHost, stream));
    wait_stream(stream);
}

void Mapper::note_kernel_time(hipEvent_t t0, hipEvent_t t1)
{
    if (!timing_) return;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, t0, t1));
    sketch_ms_ += ms;
    sketch_launches_ += 1;
}

// The reads read_cluster_kernel left over in the batch's candidate list: their hits -> the generic cluster pipeline.
void Mapper::leftovers(const Batch& b)
{
    Lane& lane = lanes_[b.lane];
    if (lane.h_scratch[L_COMPLEX] == 0) return;
    const hipStream_t stream = b.stream;
    dev::SketchArgs a = sketch_args(b.batch, b.direct ? &tsets_[b.lane] : nullptr);
    count_on_lane(a, lane); // (the recount pass does not count minimizers again)
    lane.scratch_zero = false; // the leftover pass uses the lane's counters again
    HIPCHK(dev::launch_filter_recount(a, lane.fw, stream));
    HIPCHK(hipMemcpyAsync(lane.h_scratch.data(), lane.d_scratch.data(), lane.d_scratch.bytes(), hipMemcpyDeviceToHost, stream));
    wait_stream(stream);
    const uint64_t n_left = lane.h_scratch[L_HITS];
    if (n_left == 0) return;
    ensure_workspace(std::max<uint64_t>(min_capacity_, n_left + n_left / 8));
    a.hit_key = d_key_a_.data(); // the hit buffers may have moved
    a.hit_val = d_val_a_.data();
    a.hit_capacity = hit_capacity();
    HIPCHK(dev::launch_filter_expand(a, lane.fw, stream));
    cluster_hits(b.batch.d_offsets, (uint32_t)n_left, lane.h_scratch[L_MAXLEN] <= READ_SORT_MAX_LEN, lane.d_scratch.data() + L_UNSORTED, b.covg, b.prg_reads, stream);
}

void Mapper::ensure_tile_workspace(TileSet& t, uint32_t n_tiles, uint32_t tile_cap)
{
    if (n_tiles <= t.ws_tiles && tile_cap <= t.ws_cap) return;
    const uint32_t ws_tiles = std::max(t.ws_tiles, n_tiles + n_tiles / 8 + 32), ws_cap = std::max(t.ws_cap, tile_cap);
    const size_t n = (size_t)ws_tiles * ws_cap, per_tile = (size_t)ws_tiles + 1;
    t.d_tile_info.alloc(n); t.d_tile_pos1.alloc(n); t.d_tile_rec.alloc(n);
    t.d_tile_count.alloc(per_tile); t.d_tile_hits.alloc(per_tile); t.d_tile_nmin.alloc(per_tile); t.d_tile_prefix.alloc(per_tile);
    t.d_tile_temp.alloc(dev::scan_temp_bytes(ws_tiles + 1));
    t.ws_tiles = ws_tiles; // (said last: a set whose allocation failed half-way is still known as too small)
    t.ws_cap = ws_cap;
}

// the first read of every tile: one entry per tile of the sketch that fills it, a quarter more when it has to grow
void Mapper::reserve_tile_first(TileSet& t, uint32_t n_tiles)
{
    t.d_tile_first.reserve(n_tiles, n_tiles + n_tiles / 4 + 16);
}

// Direct sequence, candidate form: every k-mer hashed (any k, any w, any index size); each tile leaves its index minimizers
// as candidate records in position order, a scan orders the slices and read_cluster_kernel takes the candidates from them -- no hit
// list, no radix sort, no cluster kernels for the reads that fit it.
// One attempt, asynchronous on `stream`: the launches, the lane's counters to their pinned mirror, the counters cleared behind the copy.
void Mapper::direct_launch(const Batch& b)
{
    const int set = b.lane;
    const uint64_t n_bases = b.batch.n_bases;
    const hipStream_t stream = b.stream;
    TileSet& t = tsets_[set];
    const uint32_t n_tiles = dev::direct_candidate_tiles(n_bases, halo_, params_.k, params_.w, wide_hash_, sw_.direct_lds); // = slices
    reserve_tile_first(t, dev::direct_first_read_tiles(n_bases, halo_, params_.k, params_.w, wide_hash_, sw_.direct_lds));
    Lane& lane = lanes_[set]; // (only this set's lane may grow: the other one may belong to a batch in flight)
    grow_lane(lane, std::min<uint64_t>(std::max<uint64_t>(min_capacity_, n_bases / 16), (1ull << 31) - 1));
    // read_cluster_kernel takes the candidates straight from the tile slices (no gathered list unless reads are left over); what it
    // handled is marked in the dense cand_pos1 array with a value no other batch used (the gather-first sequence of rounds 1-3 lost to
    // this one: DESIGN.md section 6).  The mark is never a value a position + 1 can have, never 0; one sequence of epochs per process,
    // so that no two Mappers that follow each other in recycled device memory ever use the same mark.
    static std::atomic<uint32_t> process_epoch { 0x80000000u };
    slices_epoch_ = process_epoch.fetch_add(1) + 1;
    if (slices_epoch_ < 0x80000000u) { // wrapped after 2^31 batches: marks of old batches may still be around, clear them
        HIPCHK(hipMemsetAsync(lane.cand_pos1.data(), 0, lane.cand_pos1.bytes(), stream));
        process_epoch.store(0x80000001u);
        slices_epoch_ = 0x80000001u;
    }
    const uint32_t mark = slices_epoch_;
    ensure_tile_workspace(t, n_tiles, t.slice_cap);
    if (!lane.scratch_zero) HIPCHK(hipMemsetAsync(lane.d_scratch.data(), 0, lane.d_scratch.bytes(), stream));
    lane.scratch_zero = false;
    HIPCHK(hipMemsetAsync(t.d_tile_count.data() + n_tiles, 0, sizeof(uint32_t), stream)); // the scan's closing zero
    // a packed batch: sketch_wave_kernel reads the words themselves (round 4; the positions of its npos as one bit per base, set here);
    // the general direct kernel reads an ASCII expansion made on the same stream (packed.hip)
    const bool native_packed = b.batch.packed && dev::direct_uses_wave_form(params_.k, params_.w, wide_hash_, sw_.direct_lds);
    dev::SketchArgs a = sketch_args(native_packed ? b.batch : ascii_view(set, b.batch, stream), &t);
    if (native_packed && a.n_npos) {
        const uint64_t words16 = ((n_bases + 15) / 16 + 1) & ~1ull; // (an even number of u16 words: the marks are 32-bit atomics)
        const uint64_t grown = words16 + words16 / 4;
        if (t.d_nbits.reserve(words16, grown + (grown & 1))) t.nbits_dirty = true; // (fresh memory)
        if (t.nbits_dirty) HIPCHK(hipMemsetAsync(t.d_nbits.data(), 0, t.d_nbits.bytes(), stream));
        HIPCHK(dev::launch_mark_npos(a.npos, a.n_npos, n_bases, t.d_nbits.data(), stream));
        t.nbits_dirty = true;
        a.nbits = t.d_nbits.data();
    }
    count_on_lane(a, lane);
    a.tile_cap = t.ws_cap;
    a.tile_info = t.d_tile_info.data();
    a.tile_pos1 = t.d_tile_pos1.data();
    a.tile_rec = t.d_tile_rec.data();
    a.tile_count = t.d_tile_count.data();
    a.tile_hits = t.d_tile_hits.data();
    a.tile_nmin = t.d_tile_nmin.data();
    a.prg_min_path_len = tables_.min_path_len.data();
    a.prg_thr = tables_.prg_thr.data();
    a.fraction = params_.cluster_fraction();
    a.min_cluster_size = params_.min_cluster_size;
    lane.fw = dev::FilterWork {};
    lane.fw.read_begin = 0;
    lane.fw.read_end = (uint32_t)b.batch.n_reads;
    dev::init_candidate_work(lane.fw, filter_buffers(lane), n_cus_);
    HIPCHK(dev::launch_direct_candidates(a, wide_hash_, sw_.direct_lds, t.d_tile_prefix.data(), t.d_tile_temp.data(), t.d_tile_temp.size(), lane.capacity(),
        read_cluster_args(b), n_cus_, lane.fw, stream, kernel_timer(lane.t0, lane.t1), mark));
    t.a_done = a;
    t.mark = mark;
    t.n_tiles = n_tiles;
    HIPCHK(hipMemcpyAsync(lane.h_scratch.data(), lane.d_scratch.data(), lane.d_scratch.bytes(), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemsetAsync(lane.d_scratch.data(), 0, lane.d_scratch.bytes(), stream));
    lane.scratch_zero = true;
}

// The read-back of such an attempt has arrived.  false: a tile slice or the dense list was too small -- nothing was counted except the
// minimizers, and those only in this attempt's scratch block --, the buffers have been grown and the caller runs the batch again.
// true: totals taken, reads left to the generic pipeline queued on the batch's stream.
bool Mapper::direct_finish(const Batch& b, int attempt)
{
    TileSet& t = tsets_[b.lane];
    Lane& lane = lanes_[b.lane];
    const uint32_t ovf = (uint32_t)lane.h_scratch[L_OVERFLOW];
    if (ovf & 2u) throw Error(DRPRG_EOVERFLOW, "a read is longer than 2^" + std::to_string(dev::HIT_POS_BITS) + " bases");
    if (ovf & 4u) {
        if (attempt > 6) throw Error(DRPRG_EOVERFLOW, "candidate buffer overflow after regrow");
        HIPCHK(hipStreamSynchronize(b.stream)); // (the buffers are about to be freed)
        ++reruns_direct_;
        t.slice_cap = std::min<uint32_t>(t.slice_cap * 2, 4096);
        grow_lane(lane, std::min<uint64_t>(lane.capacity() * 2, (1ull << 31) - 1));
        return false;
    }
    tot_minimizers_ += lane.h_scratch[L_MINIMIZERS];
    tot_hits_ += lane.h_scratch[L_HITS];
    tot_leftover_ += lane.h_scratch[L_COMPLEX];
    if (lane.h_scratch[L_COMPLEX]) // reads were left over: the generic pipeline wants the gathered list after all
        HIPCHK(dev::launch_tile_gather_marked(t.a_done, lane.fw, t.d_tile_prefix.data(), t.n_tiles, lane.capacity(), t.mark, b.stream));
    leftovers(b);
    return true;
}

// The same for the filtered sequence: a candidate slice that was too small -> false, the lane grown; else the totals, and the reads
// read_cluster_kernel left over -> the generic pipeline on their hits.
bool Mapper::filter_finish(const Batch& b, int attempt)
{
    Lane& lane = lanes_[b.lane];
    const uint32_t ovf = (uint32_t)lane.h_scratch[L_OVERFLOW];
    if (ovf & 8u) throw Error(DRPRG_EIO, "sketch_filter_kernel: dynamic LDS does not start at address 0");
    if (ovf & 16u) throw Error(DRPRG_EIO, "sketch_filter_kernel: a chunk of its schedule holds too few whole tiles");
    if (ovf & 32u) throw Error(DRPRG_EINVAL, "the batch's read offsets do not span its bases: offsets[0] must be 0 and offsets[n_reads] must be n_bases");
    if (ovf & 2u) throw Error(DRPRG_EOVERFLOW, "a read is longer than 2^" + std::to_string(dev::HIT_POS_BITS) + " bases");
    if (ovf & 4u) {
        // a candidate slice was too small: the sequence counted nothing and touched no coverage (hit_scan_kernel / read_cluster_kernel
        // check the flag)
        if (attempt > 8) throw Error(DRPRG_EOVERFLOW, "candidate buffer overflow after regrow");
        grow_lane(lane, lane.capacity() * 4);
        ++reruns_filter_;
        return false;
    }
    tot_minimizers_ += lane.h_scratch[L_MINIMIZERS];
    tot_hits_ += lane.h_scratch[L_HITS];
    tot_leftover_ += lane.h_scratch[L_COMPLEX];
    tune_filter_shares(lane, b.batch.packed, b.batch.n_bases);
    leftovers(b);
    return true;
}

void Mapper::filter_schedule(uint64_t out[20])
{
    sync();
    for (int i = 0; i < 20; ++i) out[i] = ft_last_[i];
}

void Mapper::buffer_info(uint64_t out[6])
{
    sync(); // (a deferred batch that overflowed is run again when it is completed)
    uint64_t raw = 0;
    for (const Lane& lane : lanes_) raw = std::max(raw, lane.capacity());
    out[0] = reruns_filter_;
    out[1] = reruns_direct_;
    out[2] = regrows_hits_;
    out[3] = raw;
    out[4] = hit_capacity();
    out[5] = sketch_form();
}

// which sketch form serves this context: 1 sketch_wave_kernel, 2 / 3 / 4 sketch_probe_kernel with its compile-time window / its sequential
// scan on u32 / u64 keys; the filtered sequence: 10 small tier (level 0 on 12-mers), 11 levels 1+2 alone (k < 15), 12 middle tier
int Mapper::sketch_form() const
{
    if (use_filter_) return use_mid_ ? 12 : (tables_.bloom0_wbits ? 10 : 11);
    if (use_direct_cands_ && dev::direct_uses_wave_form(params_.k, params_.w, wide_hash_, sw_.direct_lds)) return 1;
    return wide_hash_ ? 4 : (dev::probe_compile_time_window(params_.k, params_.w) ? 2 : 3);
}

// sketch_filter_kernel's four wave classes should end together (sketch_filter.hip: a SIMD issues for its oldest wave first).  How far apart they
// ended in the batch just read back moves the next batch's shares: share_c *= (mean end / end_c)^0.6, every share kept within 0.35 .. 2.2 of an
// even one, the sum at 1024.  Any shares give the same candidates; batches too small to time (under 64 M bases) change nothing.
void Mapper::tune_filter_shares(const Lane& lane, bool packed, uint64_t n_bases)
{
    {   // what the batch just completed ran with (whatever its size)
        const dev::FilterSched& sc = lane.fw.sched;
        const unsigned long long* ck = &lane.h_scratch[L_FT_CLOCK];
        ft_last_[0] = sc.n_rounds;
        ft_last_[1] = lane.fw.n_slices;
        ft_last_[2] = sc.tpw0;
        for (int c = 0; c < 4; ++c) {
            ft_last_[3 + c] = lane.fw.wave_share[c];
            ft_last_[7 + c] = ck[0] && ck[1 + c] > ~ck[0] ? ck[1 + c] - ~ck[0] : 0;
        }
        ft_last_[11] = sc.per_wg;
        for (int r = 0; r < dev::FT_MAX_ROUNDS; ++r) ft_last_[12 + r] = r && r < (int)sc.n_rounds ? sc.size[r] : 0;
    }
    if (lane.fw.sched.n_rounds > 1) return; // a dynamic schedule balances itself: the shares of round 0 stay what they are
    if (n_bases < (64ull << 20)) return;
    const unsigned long long* ck = &lane.h_scratch[L_FT_CLOCK];
    if (!ck[0] || !ck[1] || !ck[2] || !ck[3] || !ck[4]) return; // (a launch without the level-0 form, or with DRPRG_FT_SHARE)
    const unsigned long long t0 = ~ck[0];
    double end[4], mean = 0;
    for (int c = 0; c < 4; ++c) {
        if (ck[1 + c] <= t0) return;
        end[c] = (double)(ck[1 + c] - t0);
        mean += end[c] / 4;
    }
    uint32_t* s = ft_share_[packed ? 1 : 0];
    if (!s[0]) { // the launcher's built-in shares were in use
        const uint32_t* from = dev::filter_builtin_shares(use_mid_, packed);
        for (int c = 0; c < 4; ++c) s[c] = from[c];
    }
    double v[4], sum = 0;
    for (int c = 0; c < 4; ++c) {
        v[c] = (double)s[c] * std::pow(mean / end[c], 0.6);
        v[c] = std::min(std::max(v[c], 0.35 * 256), 2.2 * 256);
        sum += v[c];
    }
    uint32_t acc = 0;
    for (int c = 0; c < 3; ++c) acc += s[c] = (uint32_t)(1024.0 * v[c] / sum + 0.5);
    s[3] = 1024u - acc;
}

void Mapper::check(const DeviceBatch& b)
{
    if (b.n_npos && !b.d_npos) throw Error(DRPRG_EINVAL, "n_npos > 0 without the positions");
    if (b.n_reads == 0) return;
    if (!b.d_bases || !b.d_offsets) throw Error(DRPRG_EINVAL, "null device pointer");
    if ((reinterpret_cast<uintptr_t>(b.d_bases) & 15u) != 0)
        throw Error(DRPRG_EINVAL, std::string(b.packed ? "d_words" : "d_bases") + " must be 16-byte aligned");
    if (b.n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
}

void Mapper::map(const DeviceBatch& batch, uint32_t* covg, uint32_t* prg_reads, hipStream_t stream, bool deferred)
{
    check(batch);
    if (batch.n_reads == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (resident_.cap && !in_keep_call_) resident_.broken = true; // reads of the caller's own buffers: not among the kept ones
    if (!covg) covg = d_covg();
    if (!prg_reads) prg_reads = d_prg_reads();
    if (!stream) stream = stream_;
    if (!deferred || (!use_filter_ && !use_direct_cands_) || batch.n_bases == 0) {
        complete_pending();
        run_batch(batch, covg, prg_reads, stream);
        tot_reads_ += batch.n_reads;
        tot_bases_ += batch.n_bases;
        // (no deferred form of the other sequences, or of a batch of empty reads: the batch is complete on return, including what its tail
        // queued for the leftover reads)
        if (deferred) wait_stream(stream);
        return;
    }
    // the two lanes take the batches in turn: a batch's read-back is looked at while the next batch runs (a batch whose candidate buffers
    // overflowed, or that left reads to the generic pipeline, is finished then -- from its own lane, which the batch in flight does not touch)
    const Batch cur = make_batch(pipe_next_, batch, covg, prg_reads, stream);
    launch(cur);
    // the batch just queued is registered before the previous one is completed: if completing that one throws (a read too long,
    // an overflow that does not go away, a HIP error) the queued batch is still known to sync() and to the next call
    const Batch prev = pending_;
    pending_ = cur;
    pipe_next_ ^= 1;
    tot_reads_ += batch.n_reads;
    tot_bases_ += batch.n_bases;
    if (prev.active) complete_batch(prev); // the batch before this one, while this one runs
}

void Mapper::complete_pending()
{
    if (!pending_.active) return;
    const Batch b = pending_;
    pending_.active = false;
    complete_batch(b);
}

// The batch's first attempt has been launched.  Wait for its read-back, then finish -> (buffers grown) launch again -> wait ... until it
// fit.  Only the first attempt's kernel time is counted (sketch_ms_total).  A batch that needed the host afterwards (run again, reads left
// to the generic pipeline) has just had more work queued for its accumulators: "completed" means that work is done too -- the caller may
// touch the buffers of a completed batch from any stream.
void Mapper::complete_batch(const Batch& b)
{
    HIPCHK(hipSetDevice(device_));
    const Lane& lane = lanes_[b.lane];
    const uint64_t leftover_before = tot_leftover_;
    for (int attempt = 0;; ++attempt) {
        if (attempt) launch(b); // (nothing of the last attempt was counted: again, alone, behind whatever is queued on its stream)
        wait_stream(b.stream, lane.done);
        if (attempt == 0) note_kernel_time(lane.t0, lane.t1);
        if (b.direct ? direct_finish(b, attempt) : filter_finish(b, attempt)) {
            if (attempt || tot_leftover_ != leftover_before) wait_stream(b.stream);
            return;
        }
    }
}

void Mapper::sync()
{
    const hipStream_t last = pending_.active ? pending_.stream : nullptr;
    complete_pending();
    if (last) HIPCHK(hipStreamSynchronize(last));
}

void Mapper::run_batch(const DeviceBatch& batch, uint32_t* covg, uint32_t* prg_reads, hipStream_t stream)
{
    const uint64_t n_bases = batch.n_bases;
    if (n_bases == 0) return; // only empty reads: no k-mers, no hits
    if (use_filter_ || use_direct_cands_) {
        // ---- the candidate sequences (filtered; direct in its candidate form): the hits of short reads never leave the chip
        // (read_cluster_kernel).  Lane 0: complete_pending() has left nothing in flight on it ----
        const Batch b = make_batch(0, batch, covg, prg_reads, stream);
        launch(b);
        complete_batch(b);
        return;
    }
    // ---- direct sequence, generic form: every k-mer hashed, hits in tile order, global radix sort ----
    ensure_workspace(std::max<uint64_t>(min_capacity_, n_bases / 64));
    reserve_tile_first(tsets_[0], dev::sketch_n_tiles(n_bases, halo_));
    const DeviceBatch ascii = ascii_view(2, batch, stream); // (a packed batch: expanded on the device for this kernel)
    for (int attempt = 0;; ++attempt) {
        HIPCHK(hipMemsetAsync(d_counters_.data() + C_HITS, 0, 2 * sizeof(unsigned long long), stream)); // hits + minimizers of this attempt
        HIPCHK(hipMemsetAsync(d_counters_.data() + C_OVERFLOW, 0, sizeof(unsigned long long), stream));
        const dev::SketchArgs a = sketch_args(ascii, &tsets_[0]);
        HIPCHK(dev::launch_sketch_probe(a, wide_hash_, stream, kernel_timer(ev0_, ev1_)));
        read_counters(stream);
        if (attempt == 0) note_kernel_time(ev0_, ev1_); // (as complete_batch: a batch's first attempt)
        if ((uint32_t)h_counters_[C_OVERFLOW] & 2u)
            throw Error(DRPRG_EOVERFLOW, "a read is longer than 2^" + std::to_string(dev::HIT_POS_BITS) + " bases");
        if (h_counters_[C_HITS] > hit_capacity()) {
            if (attempt > 6) throw Error(DRPRG_EOVERFLOW, "hit buffer overflow after regrow");
            ensure_workspace(h_counters_[C_HITS] + h_counters_[C_HITS] / 8 + 1024);
            ++regrows_hits_;
            continue;
        }
        break;
    }
    tot_minimizers_ += h_counters_[C_MINIMIZERS];
    tot_hits_ += h_counters_[C_HITS];
    cluster_hits(batch.d_offsets, (uint32_t)h_counters_[C_HITS], false, nullptr, covg, prg_reads, stream);
}

Mapper::CutPoint Mapper::find_cut(const DeviceBatch& b, uint64_t target, hipStream_t stream)
{
    check(b);
    if (b.n_reads == 0) return CutPoint { 0, 0, 0 };
    sync(); // (a batch in flight comes before this one in the running total: it is complete before this one is cut)
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!h_cut_) h_cut_.alloc(4);
    HIPCHK(dev::launch_covg_cut(b.d_offsets, b.n_reads, target, b.d_npos, b.n_npos, h_cut_.device_ptr(), stream));
    wait_stream(stream);
    return CutPoint { h_cut_[0], h_cut_[1], h_cut_[2] };
}

void Mapper::add_vectors_from(Mapper& other)
{
    if (other.n_knodes_ != n_knodes_ || other.n_prgs_ != n_prgs_) throw Error(DRPRG_EINVAL, "coverage size mismatch");
    other.sync();
    HIPCHK(hipSetDevice(other.device_));
    HIPCHK(hipStreamSynchronize(other.stream_));
    sync();
    HIPCHK(hipSetDevice(device_));
    const size_t nc = 2 * (size_t)n_knodes_, np = n_prgs_;
    const uint32_t* src = other.d_covg(); // [coverage | reads per PRG], one vector on either side
    if (other.device_ != device_) {
        if (!d_peer_tmp_) d_peer_tmp_.alloc(nc + np);
        HIPCHK(hipMemcpyPeerAsync(d_peer_tmp_.data(), device_, other.d_covg(), other.device_, (nc + np) * sizeof(uint32_t), stream_));
        src = d_peer_tmp_.data();
    }
    HIPCHK(dev::launch_vector_add_u32(d_covg(), src, nc + np, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
}

void Mapper::download(std::vector<uint32_t>& covg, std::vector<uint32_t>& prg_reads)
{
    sync();
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipStreamSynchronize(stream_));
    covg.resize(2 * (size_t)n_knodes_);
    prg_reads.resize(n_prgs_);
    HIPCHK(hipMemcpy(covg.data(), d_covg(), covg.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(prg_reads.data(), d_prg_reads(), prg_reads.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

void Mapper::upload(const std::vector<uint32_t>& covg, const std::vector<uint32_t>& prg_reads)
{
    if (resident_.cap) resident_.broken = true; // coverage that came without its reads

    if (covg.size() != 2 * (size_t)n_knodes_ || prg_reads.size() != n_prgs_) throw Error(DRPRG_EINVAL, "coverage size mismatch");
    sync();
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipMemcpy(d_covg(), covg.data(), covg.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_prg_reads(), prg_reads.data(), prg_reads.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
}

void Mapper::device_tables(uint64_t out[6]) const
{
    const IndexTables& t = tables_;
    out[4] = use_mid_ ? (uint64_t)MID_BITMAP_WORDS * 4 + ((uint64_t)16 << t.midc_wbits) : 0; // global-memory (L2) tiers of the filter
    if (!use_mid_ && use_filter_ && t.blkc) out[4] = (uint64_t)16 << t.blkc_wbits; // (small tier: the second stage's block filter, what packed batches are tested against)
    out[5] = sketch_form();
    out[0] = t.pbloom ? (uint64_t)1 << t.pbloom_wbits : 0;
    out[1] = ((uint64_t)1 << t.table_bits) * (wide_hash_ ? 16 : 12);
    out[2] = t.bloom_wbits ? ((uint64_t)4 << t.bloom_wbits) + (t.bloom0_wbits ? ((uint64_t)4 << t.bloom0_wbits) + ((uint64_t)4 << BLOOMR_WBITS) : 0) : 0;
    if (use_mid_) out[2] = (uint64_t)4 << 15;
    out[3] = use_filter_ ? 2 : (use_direct_cands_ ? 3 : 1);
}

MapCounters Mapper::counters()
{
    sync();
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipStreamSynchronize(stream_));
    unsigned long long c[C_N];
    HIPCHK(hipMemcpy(c, d_counters_.data(), sizeof(c), hipMemcpyDeviceToHost));
    MapCounters m;
    m.reads = tot_reads_;
    m.bases = tot_bases_;
    m.minimizers = tot_minimizers_;
    m.hits = tot_hits_;
    m.clusters_kept = c[C_CLUSTERS_KEPT];
    m.hits_kept = c[C_HITS_KEPT];
    m.kernel = use_filter_ ? 2 : (use_direct_cands_ ? 3 : 1);
    m.leftover_reads = tot_leftover_;
    return m;
}

} // namespace drprg
