// mapper.cpp -- device context and per-batch launch sequence.  See mapper.h.
#include "mapper.h"
#include <algorithm>
#include <cmath>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    // collective of the path is a single ncclAllReduce / ncclReduce over it (capi.cpp)
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
    if (new_sample) drop_kept();
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
    Batch b;
    b.batch = batch;
    b.active = true;
    b.direct = !use_filter_; // (the callers run only the two candidate sequences)
    b.lane = lane;
    b.covg = covg;
    b.prg_reads = prg_reads;
    b.stream = stream;
    return b;
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
    DeviceBatch ascii;
    ascii.d_bases = d_unpacked_[slot].data();
    ascii.d_offsets = batch.d_offsets;
    ascii.n_reads = batch.n_reads;
    ascii.n_bases = batch.n_bases;
    return ascii;
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
    if (kept_cap_ && !in_keep_call_) kept_broken_ = true; // reads of the caller's own buffers: not among the kept ones
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

void Mapper::ensure_stage(Stage& st, uint64_t payload_bytes, uint64_t n_reads, uint64_t n_npos)
{
    if (payload_bytes + 64 > st.d_bases.size() || n_reads + 1 > st.d_offsets.size() || n_npos > st.d_npos.size())
        sync(); // (freeing device memory waits for the device; be explicit about the batch in flight)
    st.d_bases.reserve(payload_bytes + 64, payload_bytes + payload_bytes / 4 + 64);
    st.d_offsets.reserve(n_reads + 1, n_reads + n_reads / 4 + 1);
    st.d_npos.reserve(n_npos, n_npos + n_npos / 4 + 16);
}

Mapper::DeviceBatch Mapper::copy_in(const HostBatch& hb, uint8_t* d_bases, uint64_t* d_offsets, uint64_t* d_npos, hipStream_t stream)
{
    DeviceBatch b;
    b.d_bases = d_bases;
    b.d_offsets = d_offsets;
    b.n_reads = hb.n_reads;
    b.n_bases = hb.n_bases();
    b.packed = hb.packed;
    b.n_npos = hb.packed ? hb.n_npos : 0;
    b.d_npos = b.n_npos ? d_npos : nullptr;
    HIPCHK(hipMemcpyAsync(d_bases, hb.bases, hb.payload_bytes(), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_offsets, hb.offsets, (hb.n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    if (b.n_npos) HIPCHK(hipMemcpyAsync(d_npos, hb.npos, b.n_npos * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    return b;
}

void Mapper::ensure_bam_scratch(BamScratch& s, uint64_t n_bases)
{
    const uint64_t n = (uint64_t)dev::bam_pack_chunks(n_bases) + 1;
    const size_t temp = dev::scan_temp_bytes((uint32_t)n);
    if (n > s.d_count.size() || n > s.d_prefix.size() || temp > s.d_temp.size()) sync(); // (as ensure_stage)
    s.d_count.reserve(n, n + n / 4);
    s.d_prefix.reserve(n, n + n / 4);
    s.d_temp.reserve(temp, temp + temp / 4);
}

Mapper::DeviceBatch Mapper::copy_in_bam(const HostBatch& hb, Stage& st, uint8_t* d_words, uint64_t* d_offsets, uint64_t* d_npos, hipStream_t copy_stream,
    hipStream_t stream)
{
    if (!hb.seq_start || (hb.seq_bytes && !hb.bases)) throw Error(DRPRG_EINVAL, "null buffer");
    if (hb.seq_bytes + 16 > st.d_seq.size() || hb.n_reads > st.d_seq_start.size() || hb.n_reads > st.d_reverse.size()) sync();
    st.d_seq.reserve(hb.seq_bytes + 16, hb.seq_bytes + hb.seq_bytes / 4 + 16);
    st.d_seq_start.reserve(hb.n_reads, hb.n_reads + hb.n_reads / 4);
    st.d_reverse.reserve(hb.n_reads, hb.n_reads + hb.n_reads / 4);
    ensure_bam_scratch(st.bam, hb.n_bases());
    DeviceBatch b;
    b.d_bases = d_words;
    b.d_offsets = d_offsets;
    b.n_reads = hb.n_reads;
    b.n_bases = hb.n_bases();
    b.packed = true;
    b.n_npos = hb.n_npos; // (counted by the parser thread that copied the fields: no read-back, no wait)
    b.d_npos = b.n_npos ? d_npos : nullptr;
    if (hb.seq_bytes) HIPCHK(hipMemcpyAsync(st.d_seq.data(), hb.bases, hb.seq_bytes, hipMemcpyHostToDevice, copy_stream));
    HIPCHK(hipMemcpyAsync(st.d_seq_start.data(), hb.seq_start, hb.n_reads * sizeof(uint64_t), hipMemcpyHostToDevice, copy_stream));
    if (hb.reverse) HIPCHK(hipMemcpyAsync(st.d_reverse.data(), hb.reverse, hb.n_reads, hipMemcpyHostToDevice, copy_stream));
    HIPCHK(hipMemcpyAsync(d_offsets, hb.offsets, (hb.n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, copy_stream));
    if (copy_stream != stream) {
        HIPCHK(hipEventRecord(st.copied, copy_stream));
        HIPCHK(hipStreamWaitEvent(stream, st.copied, 0));
    }
    HIPCHK(dev::launch_bam_pack(st.d_seq.data(), st.d_seq_start.data(), d_offsets, hb.reverse ? st.d_reverse.data() : nullptr, hb.n_reads, b.n_bases,
        reinterpret_cast<uint32_t*>(d_words), d_npos, b.n_npos, b.n_npos != 0, st.bam.d_count.data(), st.bam.d_prefix.data(), st.bam.d_temp.data(),
        st.bam.d_temp.size(), stream));
    ++bam_blocks_;
    return b;
}

void Mapper::map_host(const HostBatch& hb)
{
    if (hb.n_reads == 0) return;
    sync();
    HIPCHK(hipSetDevice(device_));
    if (hb.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
    Stage& st = stage_sync_;
    ensure_stage(st, hb.payload_bytes(), hb.n_reads, hb.packed || hb.bam ? hb.n_npos : 0);
    if (hb.bam) map(copy_in_bam(hb, st, st.d_bases.data(), st.d_offsets.data(), st.d_npos.data(), stream_, stream_), nullptr, nullptr, stream_, false);
    else map(copy_in(hb, st.d_bases.data(), st.d_offsets.data(), st.d_npos.data(), stream_), nullptr, nullptr, stream_, false);
    HIPCHK(hipStreamSynchronize(stream_)); // the staging buffers are reused by the next call
}

uint64_t Mapper::pack_on_device(const uint8_t* d_bases, uint64_t n_bases, uint32_t* d_words, uint64_t* d_npos, uint64_t npos_cap, hipStream_t stream)
{
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (n_bases == 0) return 0;
    if (!d_bases || !d_words) throw Error(DRPRG_EINVAL, "null device pointer");
    if (!d_pack_count_) d_pack_count_.alloc(1); // (one counter word per Mapper: an allocation per call synchronises the device)
    unsigned long long n = 0;
    HIPCHK(hipMemsetAsync(d_pack_count_.data(), 0, sizeof(unsigned long long), stream));
    HIPCHK(dev::launch_pack(d_bases, n_bases, d_words, d_npos, d_npos ? npos_cap : 0, d_pack_count_.data(), stream));
    HIPCHK(hipMemcpyAsync(&n, d_pack_count_.data(), sizeof n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (n && !d_npos) throw Error(DRPRG_EINVAL, "the batch holds bases that are not ACGT and no buffer for their positions was given");
    if (d_npos && n > 1 && n <= npos_cap) { // the positions come out in any order: sorted on the host (few; the harness path)
        std::vector<uint64_t> h(n);
        HIPCHK(hipMemcpy(h.data(), d_npos, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        std::sort(h.begin(), h.end());
        HIPCHK(hipMemcpy(d_npos, h.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    return n;
}

uint64_t Mapper::pack_bam_on_device(const uint8_t* d_seq, const uint64_t* d_seq_start, const uint64_t* d_offsets, const uint8_t* d_reverse, uint64_t n_reads,
    uint64_t n_bases, uint32_t* d_words, uint64_t* d_npos, uint64_t npos_cap, hipStream_t stream)
{
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (n_bases == 0) return 0;
    if (n_reads == 0) throw Error(DRPRG_EINVAL, "bases without reads");
    if (!d_seq || !d_seq_start || !d_offsets || !d_words) throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
    ensure_bam_scratch(bam_api_, n_bases);
    const uint32_t n_chunks = dev::bam_pack_chunks(n_bases);
    HIPCHK(dev::launch_bam_pack(d_seq, d_seq_start, d_offsets, d_reverse, n_reads, n_bases, d_words, d_npos, d_npos ? npos_cap : 0, true,
        bam_api_.d_count.data(), bam_api_.d_prefix.data(), bam_api_.d_temp.data(), bam_api_.d_temp.size(), stream));
    uint32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, bam_api_.d_prefix.data() + n_chunks, sizeof n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (n && !d_npos) throw Error(DRPRG_EINVAL, "the batch holds bases that are not ACGT and no buffer for their positions was given");
    return n;
}

void* Mapper::arena_take(size_t bytes)
{
    bytes = (bytes + 255) / 256 * 256;
    if (kept_bytes_ + bytes > kept_cap_) return nullptr;
    if (bytes > arena_left_) {
        // (what is left of the current piece is not used: pieces are 256 MB, blocks ~25 MB)
        const size_t piece = std::max<size_t>(bytes, std::min<uint64_t>(256ull << 20, kept_cap_ - kept_bytes_));
        DeviceBuffer<uint8_t> arena;
        try {
            arena.alloc(piece);
        } catch (const Error&) { // (the device is full: the caller goes on without resident reads)
            (void)hipGetLastError();
            return nullptr;
        }
        kept_arenas_.push_back(std::move(arena));
        arena_at_ = kept_arenas_.back().data();
        arena_left_ = piece;
    }
    void* r = arena_at_;
    arena_at_ += bytes;
    arena_left_ -= bytes;
    kept_bytes_ += bytes;
    return r;
}

void Mapper::keep_reads(uint64_t max_bytes)
{
    drop_kept();
    kept_cap_ = max_bytes;
    // reads mapped before this call are not resident: kept_complete() must not claim them (map_resident would map a subset)
    kept_broken_ = tot_reads_ != 0;
}

void Mapper::drop_kept()
{
    if (!kept_arenas_.empty()) {
        sync();
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));
    }
    kept_arenas_.clear();
    kept_.clear();
    kept_first_.clear();
    kept_seen_ = 0;
    arena_at_ = nullptr;
    arena_left_ = 0;
    kept_bytes_ = 0;
    kept_broken_ = false;
}

uint64_t Mapper::map_kept_from(const Mapper& other)
{
    if (other.device_ != device_) throw Error(DRPRG_EINVAL, "the kept reads live on another device");
    if (!other.kept_complete()) throw Error(DRPRG_ENODATA, "the other context does not hold all of its reads");
    uint64_t n = 0;
    for (const DeviceBatch& b : other.kept_) {
        map(b, nullptr, nullptr, stream_, true);
        n += b.n_reads;
    }
    sync();
    HIPCHK(hipStreamSynchronize(stream_));
    return n;
}

Mapper::SubsampleResult Mapper::subsample_kept(uint64_t target_bases, uint64_t seed, std::vector<uint8_t>& flags)
{
    if (!kept_complete())
        throw Error(DRPRG_ENODATA, "random subsample: not every read of the sample is resident in device memory (drprg_hip_keep_reads is off, or the "
                                   "sample is larger than its limit; the executables take the limit from DRPRG_HIP_KEEP_READS_GB)");
    sync();
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipStreamSynchronize(stream_));
    flags.clear();
    const uint64_t n = kept_seen_;
    uint64_t bases = 0;
    for (const DeviceBatch& b : kept_) bases += b.n_bases;
    SubsampleResult res { n, bases, n, bases };
    if (bases <= target_bases) return res;
    if (n >= (1ull << 32)) throw Error(DRPRG_EOVERFLOW, "random subsample: 2^32 reads or more in one sample");
    // ---- selection (device scratch of this call) ----
    DeviceBuffer<uint64_t> d_len, d_key, d_key_sorted, d_csum, d_boff;
    DeviceBuffer<uint32_t> d_idx, d_idx_sorted, d_rank;
    DeviceBuffer<uint8_t> d_flag;
    DeviceBuffer<unsigned long long> d_cut; // d_cut: [0..1] the cut, [2] the compaction's error word
    DeviceBuffer<unsigned char> d_temp;
    d_len.alloc(n); d_key.alloc(n + 1); d_key_sorted.alloc(n); d_csum.alloc(n); d_boff.alloc(n + 1);
    d_idx.alloc(n + 1); d_idx_sorted.alloc(n); d_rank.alloc(n + 1); d_flag.alloc(n); d_cut.alloc(4);
    d_temp.alloc(dev::subsample_scan_temp_bytes(n));
    HIPCHK(hipMemsetAsync(d_len.data(), 0, d_len.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_cut.data(), 0, d_cut.bytes(), stream_));
    for (size_t b = 0; b < kept_.size(); ++b)
        HIPCHK(dev::launch_subsample_lengths(kept_[b].d_offsets, kept_[b].n_reads, kept_first_[b], n, d_len.data(), stream_));
    dev::SubsampleSelect sel {};
    sel.n = n; sel.target = target_bases; sel.seed = seed;
    sel.len = d_len.data(); sel.key = d_key.data(); sel.key_sorted = d_key_sorted.data(); sel.csum = d_csum.data(); sel.boff = d_boff.data();
    sel.idx = d_idx.data(); sel.idx_sorted = d_idx_sorted.data(); sel.rank = d_rank.data(); sel.flag = d_flag.data(); sel.cut = d_cut.data();
    sel.temp = d_temp.data(); sel.temp_bytes = d_temp.size();
    HIPCHK(dev::launch_subsample_select(sel, stream_));
    uint32_t* const d_err = reinterpret_cast<uint32_t*>(d_cut.data() + 2);
    keep_flagged(d_flag.data(), d_rank.data(), d_boff.data(), d_err, "random subsample", res, flags);
    return res;
}

// What both selections of resident reads end in (subsample_kept, dedup_kept): flag[i] = 1 for the reads that stay, rank[i] / boff[i] = kept
// reads / bases before read i (n + 1 entries, n = kept_seen_; device memory).  Every resident block is compacted into a block of its kept
// reads in arenas of their own, the old set comes back if that fails, coverage and counters are cleared and the new set is mapped.  d_err:
// a zeroed device word.  res.reads_kept / bases_kept and flags (the device flags, or empty after a failure) are filled here.
void Mapper::keep_flagged(const uint8_t* d_flag, const uint32_t* d_rank, const uint64_t* d_boff, uint32_t* d_err, const char* what, SubsampleResult& res,
    std::vector<uint8_t>& flags)
{
    const uint64_t n = kept_seen_;
    DeviceBuffer<uint64_t> d_first;
    DeviceBuffer<unsigned long long> d_bounds;
    // kept reads and bases in front of every block's first read, behind its last one, and in all
    std::vector<uint64_t> first;
    for (size_t b = 0; b < kept_.size(); ++b) {
        first.push_back(kept_first_[b]);
        first.push_back(kept_first_[b] + kept_[b].n_reads);
    }
    first.push_back(n);
    std::vector<unsigned long long> bounds(2 * first.size());
    d_first.alloc(first.size());
    d_bounds.alloc(bounds.size());
    HIPCHK(hipMemcpyAsync(d_first.data(), first.data(), first.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream_));
    HIPCHK(dev::launch_subsample_bounds(d_first.data(), (uint32_t)first.size(), n, d_rank, d_boff, d_bounds.data(), stream_));
    HIPCHK(hipMemcpyAsync(bounds.data(), d_bounds.data(), bounds.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_));
    flags.resize(n);
    HIPCHK(hipMemcpyAsync(flags.data(), d_flag, n, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    res.reads_kept = bounds[bounds.size() - 2];
    res.bases_kept = bounds[bounds.size() - 1];
    // ---- compaction: the new set in arenas of its own; the old ones are released by their owners when this scope is left ----
    std::vector<DeviceBuffer<uint8_t>> old_arenas = std::move(kept_arenas_);
    std::vector<DeviceBatch> old_kept = std::move(kept_);
    std::vector<uint64_t> old_first = std::move(kept_first_);
    uint8_t* const old_at = arena_at_;
    const size_t old_left = arena_left_;
    const uint64_t old_bytes = kept_bytes_;
    kept_arenas_.clear(); kept_.clear(); kept_first_.clear();
    arena_at_ = nullptr; arena_left_ = 0; kept_bytes_ = 0;
    try {
        uint64_t max_reads = 0, max_npos = 0;
        for (size_t b = 0; b < old_kept.size(); ++b) {
            max_reads = std::max<uint64_t>(max_reads, bounds[4 * b + 2] - bounds[4 * b]);
            max_npos = std::max(max_npos, old_kept[b].n_npos);
        }
        DeviceBuffer<uint64_t> d_src;
        DeviceBuffer<dev::GatherEntry> d_table;
        DeviceBuffer<uint32_t> d_count, d_prefix;
        DeviceBuffer<unsigned char> d_ntemp;
        d_src.alloc(max_reads);
        d_table.alloc(max_reads);
        if (max_npos) {
            const uint64_t chunks = (uint64_t)dev::subsample_npos_chunks(max_npos) + 1;
            d_count.alloc(chunks); d_prefix.alloc(chunks); d_ntemp.alloc(dev::scan_temp_bytes((uint32_t)chunks));
        }
        for (size_t b = 0; b < old_kept.size(); ++b) {
            const DeviceBatch& ob = old_kept[b];
            const uint64_t nr = bounds[4 * b + 2] - bounds[4 * b], nb = bounds[4 * b + 3] - bounds[4 * b + 1];
            if (nb == 0) continue; // (nothing of the block is kept, or empty reads only: they are counted below, as map_host_async counts them)
            const uint64_t payload = ob.packed ? (nb + 15) / 16 * 4 : nb;
            uint8_t* db = static_cast<uint8_t*>(arena_take(payload + 64));
            uint64_t* doff = db ? static_cast<uint64_t*>(arena_take((nr + 1) * sizeof(uint64_t))) : nullptr;
            if (!db || !doff) throw Error(DRPRG_ENOMEM, std::string(what) + ": no device memory for the kept reads beside the resident sample");
            HIPCHK(hipMemsetAsync(db + payload, 0, 64, stream_));
            const dev::SubsampleBlock sb { ob.d_bases, ob.d_offsets, ob.n_reads, ob.n_bases, old_first[b], d_flag, d_rank, d_boff, nr, nb };
            DeviceBatch kb;
            kb.d_bases = db; kb.d_offsets = doff; kb.n_reads = nr; kb.n_bases = nb; kb.packed = ob.packed;
            if (ob.packed) {
                HIPCHK(dev::launch_subsample_tables(sb, doff, d_src.data(), nullptr, d_err, stream_));
                HIPCHK(dev::launch_subsample_pack(sb, doff, d_src.data(), reinterpret_cast<uint32_t*>(db), d_err, stream_));
                if (ob.n_npos) {
                    const uint32_t chunks = dev::subsample_npos_chunks(ob.n_npos);
                    HIPCHK(dev::launch_subsample_npos_count(sb, ob.d_npos, ob.n_npos, d_count.data(), d_prefix.data(), d_ntemp.data(), d_ntemp.size(), stream_));
                    uint32_t cnt = 0;
                    HIPCHK(hipMemcpyAsync(&cnt, d_prefix.data() + chunks, sizeof cnt, hipMemcpyDeviceToHost, stream_));
                    HIPCHK(hipStreamSynchronize(stream_));
                    if (cnt) {
                        uint64_t* dnp = static_cast<uint64_t*>(arena_take((uint64_t)cnt * sizeof(uint64_t)));
                        if (!dnp) throw Error(DRPRG_ENOMEM, std::string(what) + ": no device memory for the kept reads beside the resident sample");
                        HIPCHK(dev::launch_subsample_npos_emit(sb, ob.d_npos, ob.n_npos, d_prefix.data(), dnp, cnt, stream_));
                        kb.d_npos = dnp;
                        kb.n_npos = cnt;
                    }
                }
            } else {
                HIPCHK(hipMemsetAsync(d_table.data(), 0, nr * sizeof(dev::GatherEntry), stream_)); // (an entry the kernel refuses to fill copies nothing)
                HIPCHK(dev::launch_subsample_tables(sb, doff, nullptr, d_table.data(), d_err, stream_));
                HIPCHK(dev::launch_gather_reads(d_table.data(), (uint32_t)nr, db, stream_));
            }
            kept_.push_back(kb);
            kept_first_.push_back(bounds[4 * b]);
        }
        uint32_t err = 0;
        HIPCHK(hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_)); // (nothing reads the old blocks any more)
        if (err) throw Error(DRPRG_EIO, std::string(what) + ": the resident blocks' offsets and the selection do not fit each other");
    } catch (...) { // the sample as it was
        (void)hipStreamSynchronize(stream_);
        kept_arenas_ = std::move(old_arenas);
        kept_ = std::move(old_kept);
        kept_first_ = std::move(old_first);
        arena_at_ = old_at; arena_left_ = old_left; kept_bytes_ = old_bytes;
        flags.clear();
        throw;
    }
    kept_seen_ = res.reads_kept;
    // ---- the kept reads mapped afresh ----
    HIPCHK(hipMemsetAsync(d_covg_.data(), 0, d_covg_.bytes(), stream_)); // [coverage | reads per PRG]
    HIPCHK(hipMemsetAsync(d_counters_.data(), 0, d_counters_.bytes(), stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    tot_reads_ = tot_bases_ = tot_hits_ = tot_leftover_ = tot_minimizers_ = 0;
    uint64_t in_blocks = 0;
    in_keep_call_ = true;
    try {
        for (const DeviceBatch& b : kept_) {
            map(b, nullptr, nullptr, stream_, true);
            in_blocks += b.n_reads;
        }
        sync();
    } catch (...) {
        in_keep_call_ = false;
        throw;
    }
    in_keep_call_ = false;
    HIPCHK(hipStreamSynchronize(stream_));
    tot_reads_ += res.reads_kept - in_blocks; // (kept empty reads of blocks that hold no base any more)
}

// One resident block as the key kernel reads it: a packed block as it lies there (the bitmap of its listed positions beside it), an ASCII
// block packed into scratch first.  The scratch lives as long as this object.
struct Mapper::DedupBlock {
    DeviceBuffer<uint32_t> words;
    DeviceBuffer<uint64_t> npos;
    DeviceBuffer<uint16_t> bits;
    dev::DedupBatch batch {};
};

void Mapper::dedup_block(const DeviceBatch& kb, DedupBlock& out, unsigned long long* d_count)
{
    const uint64_t n_words = (kb.n_bases + 15) / 16;
    const uint64_t* d_npos = kb.d_npos;
    uint64_t n_npos = kb.n_npos;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(kb.d_bases);
    if (!kb.packed) {
        // launch_pack counts every position it meets and writes those below the capacity: one pass with room for a modest number of them,
        // a second one only for a block that holds more
        const uint64_t room = std::min<uint64_t>(kb.n_bases, 1u << 16);
        out.words.alloc(n_words + 4);
        out.npos.alloc(room);
        unsigned long long cnt = 0;
        HIPCHK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream_));
        HIPCHK(dev::launch_pack(kb.d_bases, kb.n_bases, out.words.data(), out.npos.data(), room, d_count, stream_));
        HIPCHK(hipMemcpyAsync(&cnt, d_count, sizeof cnt, hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        if (cnt > room) {
            out.npos.alloc(cnt);
            HIPCHK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream_));
            HIPCHK(dev::launch_pack(kb.d_bases, kb.n_bases, out.words.data(), out.npos.data(), cnt, d_count, stream_));
        }
        words = out.words.data();
        d_npos = out.npos.data();
        n_npos = cnt;
    }
    if (n_npos) {
        out.bits.alloc(n_words + 8);
        HIPCHK(hipMemsetAsync(out.bits.data(), 0, out.bits.bytes(), stream_));
        HIPCHK(dev::launch_mark_npos(d_npos, n_npos, kb.n_bases, out.bits.data(), stream_));
    }
    out.batch = dev::DedupBatch { words, n_npos ? out.bits.data() : nullptr, kb.d_offsets, kb.n_reads, kb.n_bases };
}

Mapper::SubsampleResult Mapper::dedup_kept(uint32_t key_bits, std::vector<uint8_t>& flags)
{
    if (key_bits < 1 || key_bits > 64) throw Error(DRPRG_EINVAL, "duplicate removal: key_bits must be 1..64");
    if (!kept_complete())
        throw Error(DRPRG_ENODATA, "duplicate removal: not every read of the sample is resident in device memory (drprg_hip_keep_reads is off, or the "
                                   "sample is larger than its limit; the executables take the limit from DRPRG_HIP_KEEP_READS_GB)");
    sync();
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipStreamSynchronize(stream_));
    flags.clear();
    const uint64_t n = kept_seen_;
    uint64_t bases = 0, with_bases = 0;
    for (const DeviceBatch& b : kept_) {
        bases += b.n_bases;
        with_bases += b.n_bases ? b.n_reads : 0; // (an upper bound: two reads with bases need two reads in blocks that hold bases)
    }
    SubsampleResult res { n, bases, n, bases };
    if (n >= (1ull << 32)) throw Error(DRPRG_EOVERFLOW, "duplicate removal: 2^32 reads or more in one sample");
    if (with_bases < 2) return res;
    // ---- selection (device scratch of this call) ----
    DeviceBuffer<uint64_t> d_key, d_key_sorted, d_boff;
    DeviceBuffer<uint32_t> d_idx, d_idx_sorted, d_rank, d_err;
    DeviceBuffer<uint8_t> d_flag;
    DeviceBuffer<dev::DedupLoc> d_loc;
    DeviceBuffer<unsigned long long> d_count;
    DeviceBuffer<unsigned char> d_temp;
    d_key.alloc(n + 1); d_key_sorted.alloc(n); d_boff.alloc(n + 1); d_idx.alloc(n + 1); d_idx_sorted.alloc(n); d_rank.alloc(n + 1);
    d_flag.alloc(n); d_loc.alloc(n); d_err.alloc(4); d_count.alloc(1);
    d_temp.alloc(dev::subsample_scan_temp_bytes(n));
    HIPCHK(hipMemsetAsync(d_key.data(), 0, d_key.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_loc.data(), 0, d_loc.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_err.data(), 0, d_err.bytes(), stream_));
    std::vector<DedupBlock> blocks(kept_.size()); // (the exact check reads every block: the scratch of all of them lives until it is done)
    for (size_t b = 0; b < kept_.size(); ++b) {
        if (!kept_[b].n_reads || !kept_[b].n_bases) continue;
        if (kept_first_[b] + kept_[b].n_reads > n) throw Error(DRPRG_EIO, "duplicate removal: the resident blocks hold more reads than the sample");
        dedup_block(kept_[b], blocks[b], d_count.data());
        HIPCHK(dev::launch_dedup_keys(blocks[b].batch, reinterpret_cast<unsigned long long*>(d_key.data()) + kept_first_[b], d_err.data(), stream_));
        HIPCHK(dev::launch_dedup_loc(blocks[b].batch, kept_first_[b], n, d_loc.data(), d_err.data(), stream_));
    }
    dev::DedupSelect sel {};
    sel.n = n; sel.key_bits = key_bits; sel.loc = d_loc.data();
    sel.key = d_key.data(); sel.key_sorted = d_key_sorted.data(); sel.boff = d_boff.data();
    sel.idx = d_idx.data(); sel.idx_sorted = d_idx_sorted.data(); sel.rank = d_rank.data(); sel.flag = d_flag.data(); sel.err = d_err.data();
    sel.temp = d_temp.data(); sel.temp_bytes = d_temp.size();
    HIPCHK(dev::launch_dedup_select(sel, stream_));
    uint32_t err = 0, kept = 0;
    HIPCHK(hipMemcpyAsync(&err, d_err.data(), sizeof err, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(&kept, d_rank.data() + n, sizeof kept, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    if (err) throw Error(DRPRG_EIO, "duplicate removal: a resident block's offsets do not fit its bases");
    if (kept == n) return res; // no read dropped: nothing else happens
    keep_flagged(d_flag.data(), d_rank.data(), d_boff.data(), d_err.data() + 1, "duplicate removal", res, flags);
    return res;
}

void Mapper::dedup_keys_device(const uint32_t* d_words, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, const uint64_t* d_npos, uint64_t n_npos,
    unsigned long long* d_keys, hipStream_t stream)
{
    if (n_reads == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!d_offsets || !d_keys || (n_bases && !d_words) || (n_npos && !d_npos)) throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_reads >= (1ull << 32)) throw Error(DRPRG_EOVERFLOW, "duplicate keys: 2^32 reads or more in one batch");
    const uint64_t n_words = (n_bases + 15) / 16;
    DeviceBuffer<uint16_t> d_bits;
    DeviceBuffer<uint32_t> d_err;
    d_err.alloc(1);
    HIPCHK(hipMemsetAsync(d_err.data(), 0, d_err.bytes(), stream));
    HIPCHK(hipMemsetAsync(d_keys, 0, n_reads * sizeof(unsigned long long), stream));
    if (n_npos) {
        d_bits.alloc(n_words + 8);
        HIPCHK(hipMemsetAsync(d_bits.data(), 0, d_bits.bytes(), stream));
        HIPCHK(dev::launch_mark_npos(d_npos, n_npos, n_bases, d_bits.data(), stream));
    }
    const dev::DedupBatch b { d_words, n_npos ? d_bits.data() : nullptr, d_offsets, n_reads, n_bases };
    HIPCHK(dev::launch_dedup_keys(b, d_keys, d_err.data(), stream));
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, d_err.data(), sizeof err, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (err) throw Error(DRPRG_EINVAL, "duplicate keys: the offsets do not ascend from 0 to n_bases");
}

void Mapper::select_reads_with_anchors(std::vector<uint64_t> anchors, uint32_t A, std::vector<uint8_t>& bases, std::vector<uint64_t>& offsets,
    std::vector<uint64_t>* ids, uint64_t window_bytes)
{
    if (!kept_complete()) throw Error(DRPRG_ENODATA, "not every read of the sample is resident");
    if (A == 0 || A > 31) throw Error(DRPRG_EINVAL, "anchor length must be 1..31");
    if (offsets.empty()) offsets.push_back(0);
    std::sort(anchors.begin(), anchors.end());
    anchors.erase(std::unique(anchors.begin(), anchors.end()), anchors.end());
    if (anchors.empty() || kept_.empty()) return;
    sync();
    HIPCHK(hipSetDevice(device_));
    std::vector<uint32_t> pf(2048, 0);
    for (uint64_t a : anchors) pf[(a & 0xFFFF) >> 5] |= 1u << (a & 31);
    uint64_t total_reads = 0, max_reads = 0;
    for (const DeviceBatch& b : kept_) {
        total_reads += b.n_reads;
        max_reads = std::max(max_reads, b.n_reads);
    }
    // device scratch of this call
    DeviceBuffer<uint64_t> d_anchors;
    DeviceBuffer<uint32_t> d_pf, d_flags;
    DeviceBuffer<unsigned long long> d_count;
    DeviceBuffer<dev::SelectedRead> d_list;
    DeviceBuffer<uint8_t> d_ascii;
    d_anchors.alloc(anchors.size()); d_pf.alloc(pf.size()); d_flags.alloc(max_reads); d_count.alloc(1); d_list.alloc(total_reads);
    HIPCHK(hipMemcpyAsync(d_anchors.data(), anchors.data(), anchors.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemcpyAsync(d_pf.data(), pf.data(), pf.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemsetAsync(d_count.data(), 0, sizeof(unsigned long long), stream_));
    // Batches kept in the packed form: the scan and the gather read an ASCII expansion.  It is made a WINDOW of batches at a time -- as
    // many consecutive batches as expand into <= 1 GB (a larger batch alone) --, scanned, and its selected reads gathered before the next
    // window's expansion takes the scratch: the scratch is the largest window, not the sample (up to 128 Gbases can stay
    // resident packed; expanding all of them at once needed that much memory again, with no way back to the file pass).
    auto expanded = [](const DeviceBatch& kb) -> uint64_t { return kb.packed ? (kb.n_bases + 15) / 16 * 16 + 64 : 0; };
    const uint64_t WINDOW_BYTES = window_bytes ? window_bytes : SELECT_WINDOW_BYTES;
    std::vector<std::pair<size_t, size_t>> windows; // [first batch, one past the last)
    uint64_t scratch_need = 0;
    for (size_t b = 0; b < kept_.size();) {
        size_t e = b;
        uint64_t need = 0;
        do need += expanded(kept_[e++]);
        while (e < kept_.size() && need + expanded(kept_[e]) <= WINDOW_BYTES);
        windows.emplace_back(b, e);
        scratch_need = std::max(scratch_need, need);
        b = e;
    }
    if (scratch_need) d_ascii.alloc(scratch_need);
    std::vector<const uint8_t*> ascii(kept_.size(), nullptr);
    unsigned long long done = 0; // entries of d_list the windows before this one left
    for (const auto& win : windows) {
        uint64_t at = 0;
        for (size_t b = win.first; b < win.second; ++b) {
            const DeviceBatch& kb = kept_[b];
            if (!kb.packed) {
                ascii[b] = kb.d_bases;
                continue;
            }
            HIPCHK(dev::launch_unpack(reinterpret_cast<const uint32_t*>(kb.d_bases), kb.n_bases, kb.d_npos, kb.n_npos, d_ascii.data() + at, stream_));
            ascii[b] = d_ascii.data() + at;
            at += expanded(kb);
        }
        for (size_t b = win.first; b < win.second; ++b) {
            const DeviceBatch& kb = kept_[b];
            HIPCHK(hipMemsetAsync(d_flags.data(), 0, kb.n_reads * sizeof(uint32_t), stream_));
            HIPCHK(dev::launch_anchor_scan(ascii[b], kb.d_offsets, (uint32_t)kb.n_reads, kb.n_bases, d_anchors.data(), (uint32_t)anchors.size(), A, d_pf.data(),
                (uint32_t)b, d_flags.data(), d_count.data(), d_list.data(), total_reads, n_cus_, stream_));
        }
        unsigned long long count = 0;
        HIPCHK(hipMemcpyAsync(&count, d_count.data(), sizeof count, hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        if (count > total_reads) throw Error(DRPRG_EIO, "read selection: more reads than the batches hold"); // (each read is appended once)
        if (count == done) continue;
        std::vector<dev::SelectedRead> list(count - done);
        HIPCHK(hipMemcpy(list.data(), d_list.data() + done, (count - done) * sizeof(dev::SelectedRead), hipMemcpyDeviceToHost));
        done = count;
        std::sort(list.begin(), list.end(), [](const dev::SelectedRead& x, const dev::SelectedRead& y) { return x.batch != y.batch ? x.batch < y.batch : x.read < y.read; });
        std::vector<dev::GatherEntry> table(list.size());
        uint64_t out_bytes = 0;
        for (size_t i = 0; i < list.size(); ++i) {
            table[i].src = ascii[list[i].batch] + list[i].offset;
            table[i].dst = out_bytes;
            table[i].len = list[i].len;
            table[i].pad = 0;
            out_bytes += list[i].len;
        }
        // (device memory of this window only: freed before the next one)
        DeviceBuffer<dev::GatherEntry> d_table;
        DeviceBuffer<uint8_t> d_out;
        d_table.alloc(list.size());
        d_out.alloc(out_bytes);
        const size_t base0 = bases.size();
        bases.resize(base0 + out_bytes);
        HIPCHK(hipMemcpyAsync(d_table.data(), table.data(), list.size() * sizeof(dev::GatherEntry), hipMemcpyHostToDevice, stream_));
        HIPCHK(dev::launch_gather_reads(d_table.data(), (uint32_t)list.size(), d_out.data(), stream_));
        if (out_bytes) HIPCHK(hipMemcpyAsync(bases.data() + base0, d_out.data(), out_bytes, hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        for (size_t i = 0; i < list.size(); ++i) offsets.push_back(offsets.back() + list[i].len);
        if (ids)
            for (size_t i = 0; i < list.size(); ++i) ids->push_back((uint64_t)list[i].batch << 32 | list[i].read);
    }
}

// over the limit (or the device is full): nothing is kept from here on, and what was kept is of no use without the rest
void Mapper::stop_keeping()
{
    const uint64_t cap = kept_cap_;
    drop_kept();
    kept_cap_ = cap;
    kept_broken_ = true;
    // (said once per context, always: the run takes a different, slower route from here -- results are the same)
    std::fprintf(stderr, "[drprg-hip] the sample is larger than the %.1f GB of device memory set aside for resident reads (device %d): reads are "
                         "not kept, later passes read the file again (DRPRG_HIP_KEEP_READS_GB raises the limit)\n", (double)cap / 1e9, device_);
}

void Mapper::map_host_async(const HostBatch& hb)
{
    const uint64_t n_reads = hb.n_reads;
    if (n_reads == 0) return;
    if (kept_cap_ && !kept_broken_) {
        // the block goes into device memory of its own and stays there
        HIPCHK(hipSetDevice(device_));
        if (hb.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
        if (hb.n_bases() == 0) {
            tot_reads_ += n_reads; // (only empty reads: nothing to keep)
            kept_seen_ += n_reads;
            return;
        }
        const uint64_t n_npos = hb.packed || hb.bam ? hb.n_npos : 0;
        uint8_t* db = static_cast<uint8_t*>(arena_take(hb.payload_bytes() + 64));
        uint64_t* doff = db ? static_cast<uint64_t*>(arena_take((n_reads + 1) * sizeof(uint64_t))) : nullptr;
        uint64_t* dnp = doff && n_npos ? static_cast<uint64_t*>(arena_take(n_npos * sizeof(uint64_t))) : nullptr;
        if (db && doff && (dnp || !n_npos)) {
            if (!copy_stream_) copy_stream_.create();
            if (!kept_copied_) kept_copied_.create(false);
            // (a BAM block is kept in the packed form: its raw fields go through a staging set, taken in turn as below)
            Stage* raw = hb.bam ? &stage_[stage_next_] : nullptr;
            if (raw) {
                stage_next_ ^= 1;
                if (!raw->copied) raw->copied.create(false);
            }
            const DeviceBatch kb = raw ? copy_in_bam(hb, *raw, db, doff, dnp, copy_stream_, stream_) : copy_in(hb, db, doff, dnp, copy_stream_);
            HIPCHK(hipEventRecord(kept_copied_, copy_stream_));
            HIPCHK(hipStreamWaitEvent(stream_, kept_copied_, 0));
            kept_.push_back(kb);
            kept_first_.push_back(kept_seen_);
            kept_seen_ += n_reads;
            in_keep_call_ = true;
            try {
                map(kb, nullptr, nullptr, stream_, true);
            } catch (...) {
                in_keep_call_ = false;
                throw;
            }
            in_keep_call_ = false;
            HIPCHK(hipEventSynchronize(kept_copied_)); // the caller's block is free again
            return;
        }
        stop_keeping();
    }
    if (!use_filter_) { // no deferred form of this sequence
        map_host(hb);
        return;
    }
    HIPCHK(hipSetDevice(device_));
    if (hb.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
    if (hb.n_bases() == 0) { // only empty reads: nothing to copy, nothing to map (the counters still see them)
        tot_reads_ += n_reads;
        return;
    }
    if (!copy_stream_) copy_stream_.create();
    // the batch that used this staging set two calls ago was completed by the previous call (a deferred map completes the batch
    // before the one it queues), so the set is free
    Stage& st = stage_[stage_next_];
    stage_next_ ^= 1;
    if (!st.copied) st.copied.create(false);
    ensure_stage(st, hb.payload_bytes(), n_reads, hb.packed || hb.bam ? hb.n_npos : 0);
    const DeviceBatch b = hb.bam ? copy_in_bam(hb, st, st.d_bases.data(), st.d_offsets.data(), st.d_npos.data(), copy_stream_, stream_)
                                 : copy_in(hb, st.d_bases.data(), st.d_offsets.data(), st.d_npos.data(), copy_stream_);
    HIPCHK(hipEventRecord(st.copied, copy_stream_));
    HIPCHK(hipStreamWaitEvent(stream_, st.copied, 0));
    map(b, nullptr, nullptr, stream_, true);
    HIPCHK(hipEventSynchronize(st.copied)); // the caller's block is free again; the kernels run on
}

// ---- the read filter ---------------------------------------------------------------------------------------------------------------
void Mapper::ensure_filter_scratch(FilterScratch& fs, uint64_t n_reads, uint64_t qual_bytes, bool own_flags, bool own_sums)
{
    auto room = [&](auto& buf, uint64_t need) {
        if (need <= buf.size()) return;
        sync(); // (as ensure_stage: freeing device memory waits for the device)
        buf.alloc(need + need / 4);
    };
    if (qual_bytes) room(fs.d_qual, qual_bytes + 64);
    if (own_flags) room(fs.d_flag, n_reads);
    if (own_sums) room(fs.d_qsum, n_reads);
    room(fs.d_flag32, n_reads + 1);
    room(fs.d_rank, n_reads + 1);
    room(fs.d_klen, n_reads + 1);
    room(fs.d_boff, n_reads + 1);
    room(fs.d_temp, dev::read_filter_temp_bytes(n_reads));
    if (!fs.d_work) fs.d_work.alloc(8);
    if (!fs.h_out) fs.h_out.alloc(8);
}

void Mapper::run_read_filter(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, uint64_t n_reads,
    uint64_t n_bases, unsigned long long* d_sums, uint8_t* d_flags, hipStream_t stream)
{
    dev::ReadFilterArgs a {};
    a.qual = d_qual; a.bias = bias; a.offsets = d_offsets; a.n_reads = n_reads; a.n_bases = n_bases;
    a.min_len = f.min_len; a.max_len = f.max_len; a.T = f.T; a.use_qual = f.use_qual(); // (a batch of empty reads launches no tile, and its sums are still cleared)
    a.qsum = d_sums; a.flag = d_flags; a.flag32 = fs.d_flag32.data(); a.rank = fs.d_rank.data(); a.klen = fs.d_klen.data(); a.boff = fs.d_boff.data();
    a.work = fs.d_work.data(); a.out = fs.h_out.device_ptr(); a.temp = fs.d_temp.data(); a.temp_bytes = fs.d_temp.size();
    HIPCHK(dev::launch_read_filter(a, stream));
}

void Mapper::read_filter_device(const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases,
    unsigned long long* d_sums, uint8_t* d_flags, uint64_t res[8], hipStream_t stream)
{
    for (int i = 0; i < 8; ++i) res[i] = 0;
    if (n_reads == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!d_offsets || !d_flags || (f.use_qual() && n_bases && !d_qual)) throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
    FilterScratch& fs = filter_api_;
    ensure_filter_scratch(fs, n_reads, 0, false, f.use_qual() && !d_sums);
    if (f.use_qual() && !d_sums) d_sums = fs.d_qsum.data();
    run_read_filter(fs, f, d_qual, bias, d_offsets, n_reads, n_bases, d_sums, d_flags, stream);
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < 8; ++i) res[i] = fs.h_out[i];
}

// ---- read trimming -------------------------------------------------------------------------------------------------------------------
void Mapper::ensure_trim_scratch(FilterScratch& fs, uint64_t n_reads, uint64_t n_npos, bool use_qual, bool own_ranges, bool adapters, uint64_t bitmap_bases)
{
    auto room = [&](auto& buf, uint64_t need) {
        if (need <= buf.size()) return;
        sync(); // (as ensure_stage: freeing device memory waits for the device)
        buf.alloc(need + need / 4);
    };
    if (use_qual) {
        room(fs.t_first, n_reads);
        room(fs.t_last, n_reads);
    }
    if (own_ranges) {
        room(fs.t_begin, n_reads);
        room(fs.t_end, n_reads);
    }
    room(fs.t_klen, n_reads + 1);
    room(fs.t_offsets, n_reads + 1);
    room(fs.t_temp, dev::read_trim_temp_bytes(n_reads));
    if (n_npos) {
        const uint64_t chunks = (uint64_t)dev::read_trim_npos_chunks(n_npos) + 1;
        room(fs.t_count, chunks);
        room(fs.t_prefix, chunks);
        room(fs.t_ntemp, dev::scan_temp_bytes((uint32_t)chunks));
    }
    if (adapters) {
        room(fs.t_cut, n_reads);
        if (bitmap_bases) room(fs.t_nbits, (bitmap_bases + 15) / 16 + 8); // (launch_mark_npos writes 32-bit words)
    }
    if (!fs.t_work) fs.t_work.alloc(dev::RT_WORDS);
    if (!fs.t_out) fs.t_out.alloc(dev::RT_WORDS);
}

dev::AdapterPoints Mapper::adapter_points(FilterScratch& fs, const uint8_t* d_bases, bool packed, const uint64_t* d_npos, uint64_t n_npos, uint64_t n_bases,
    hipStream_t stream)
{
    dev::AdapterPoints p {};
    p.cut = fs.t_cut.data();
    if (!packed) {
        p.text = d_bases;
        return p;
    }
    p.words = reinterpret_cast<const uint32_t*>(d_bases);
    if (n_npos) {
        const uint64_t n16 = (n_bases + 15) / 16 + 8;
        HIPCHK(hipMemsetAsync(fs.t_nbits.data(), 0, n16 * sizeof(uint16_t), stream));
        HIPCHK(dev::launch_mark_npos(d_npos, n_npos, n_bases, fs.t_nbits.data(), stream));
        p.nbits = fs.t_nbits.data();
    }
    return p;
}

void Mapper::run_read_trim(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, const uint8_t* d_rev,
    uint64_t n_reads, uint64_t n_bases, uint64_t* d_begin, uint64_t* d_end, const uint64_t* d_npos, uint64_t n_npos, hipStream_t stream,
    const dev::AdapterPoints* pts)
{
    dev::ReadTrimArgs a {};
    dev::AdapterEditSets edit {};
    const bool indels = pts && f.adapter_indels && f.any_adapters();
    if (pts && f.any_adapters()) {
        a.pts = *pts;
        if (indels) edit = dev::AdapterEditSets { f.adapters, f.front_adapters, f.eq3, f.eq5 };
        else a.ad = f.adapters;
    }
    a.qual = d_qual; a.bias = bias; a.offsets = d_offsets; a.rev = d_rev; a.n_reads = n_reads; a.n_bases = n_bases;
    a.front = f.trim_front; a.tail = f.trim_tail; a.qual_milli = f.trim_qual_milli; a.window = f.trim_window;
    a.first = fs.t_first.data(); a.last = fs.t_last.data(); a.begin = d_begin; a.end = d_end; a.klen = fs.t_klen.data(); a.noff = fs.t_offsets.data();
    a.work = fs.t_work.data(); a.out = fs.t_out.device_ptr(); a.temp = fs.t_temp.data(); a.temp_bytes = fs.t_temp.size();
    dev::ReadTrimNpos np {};
    if (n_npos) np = dev::ReadTrimNpos { d_npos, n_npos, fs.t_count.data(), fs.t_prefix.data(), fs.t_ntemp.data(), fs.t_ntemp.size() };
    HIPCHK(dev::launch_read_trim(a, np, stream, {}, indels ? &edit : nullptr));
}

void Mapper::read_trim_device(const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, const uint8_t* d_rev, uint64_t n_reads,
    uint64_t n_bases, uint64_t* d_begin, uint64_t* d_end, uint64_t res[9], hipStream_t stream)
{
    for (int i = 0; i < 9; ++i) res[i] = 0;
    if (n_reads == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!d_offsets || !d_begin || !d_end || (f.trim_qual_milli && n_bases && !d_qual)) throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
    FilterScratch& fs = filter_api_;
    ensure_trim_scratch(fs, n_reads, 0, f.trim_qual_milli != 0, false);
    run_read_trim(fs, f, d_qual, bias, d_offsets, d_rev, n_reads, n_bases, d_begin, d_end, nullptr, 0, stream);
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < 9; ++i) res[i] = fs.t_out[i];
}

void Mapper::adapter_trim_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos,
    const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, const uint64_t* d_begin, uint64_t* d_end, uint64_t res[6], hipStream_t stream, dev::KernelTimer timer)
{
    for (int i = 0; i < 6; ++i) res[i] = 0;
    if (n_reads == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!f.adapters.n) throw Error(DRPRG_EINVAL, "adapter trimming: no adapter is set (drprg_hip_set_adapters)");
    if (f.adapter_indels) throw Error(DRPRG_EINVAL, "adapter trimming: the indel rule is set (drprg_hip_set_adapters2); it runs through drprg_hip_adapter_trim_device2");
    if (!d_offsets || !d_begin || !d_end || (n_bases && !d_text && !d_words) || (n_npos && !d_npos)) throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
    FilterScratch& fs = filter_api_;
    ensure_trim_scratch(fs, n_reads, 0, false, false, true, d_words && n_npos ? n_bases : 0);
    dev::AdapterPoints p = adapter_points(fs, d_words ? reinterpret_cast<const uint8_t*>(d_words) : d_text, d_words != nullptr, d_npos, n_npos, n_bases, stream);
    p.offsets = d_offsets; p.begin = d_begin; p.end = d_end; p.n_reads = n_reads; p.n_bases = n_bases;
    HIPCHK(hipMemsetAsync(fs.t_work.data(), 0, dev::RT_WORDS * sizeof(unsigned long long), stream));
    HIPCHK(dev::launch_adapter_trim(p, f.adapters, d_end, nullptr, fs.t_work.data(), stream, timer));
    HIPCHK(hipMemcpyAsync(fs.t_out.data(), fs.t_work.data(), dev::RT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    res[0] = n_reads;
    for (int i = 0; i < 4; ++i) res[1 + i] = fs.t_out[dev::RT_AD_BASES_SEEN + i];
    res[5] = fs.t_out[dev::RT_OFFSETS];
}

void Mapper::adapter_trim_device2(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos,
    const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t* d_begin, uint64_t* d_end, uint64_t res[11], hipStream_t stream, dev::KernelTimer timer3,
    dev::KernelTimer timer5)
{
    for (int i = 0; i < 11; ++i) res[i] = 0;
    if (n_reads == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!f.any_adapters()) throw Error(DRPRG_EINVAL, "adapter trimming: no adapter is set (drprg_hip_set_adapters, drprg_hip_set_adapters2)");
    if (!d_offsets || !d_begin || !d_end || (n_bases && !d_text && !d_words) || (n_npos && !d_npos)) throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
    FilterScratch& fs = filter_api_;
    ensure_trim_scratch(fs, n_reads, 0, false, false, true, d_words && n_npos ? n_bases : 0);
    dev::AdapterPoints p = adapter_points(fs, d_words ? reinterpret_cast<const uint8_t*>(d_words) : d_text, d_words != nullptr, d_npos, n_npos, n_bases, stream);
    p.offsets = d_offsets; p.begin = d_begin; p.end = d_end; p.n_reads = n_reads; p.n_bases = n_bases;
    HIPCHK(hipMemsetAsync(fs.t_work.data(), 0, dev::RT_WORDS * sizeof(unsigned long long), stream));
    if (f.adapter_indels)
        HIPCHK(dev::launch_adapter_edit(p, f.adapters, f.eq3, f.front_adapters, f.eq5, d_begin, d_end, nullptr, fs.t_work.data(), stream, timer3, timer5));
    else HIPCHK(dev::launch_adapter_trim(p, f.adapters, d_end, nullptr, fs.t_work.data(), stream, timer3));
    HIPCHK(hipMemcpyAsync(fs.t_out.data(), fs.t_work.data(), dev::RT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (f.adapters.n) res[0] = n_reads;
    if (f.front_adapters.n) res[5] = n_reads;
    for (int i = 0; i < 4; ++i) {
        res[1 + i] = fs.t_out[dev::RT_AD_BASES_SEEN + i];
        res[6 + i] = fs.t_out[dev::RT_FA_BASES_SEEN + i];
    }
    res[10] = fs.t_out[dev::RT_OFFSETS];
}

void Mapper::map_host_filtered(const HostBatch& hb, const ReadFilter& f, uint64_t cap_need, FilterOutcome& o)
{
    o = FilterOutcome {};
    const uint64_t n_reads = hb.n_reads;
    if (n_reads == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (hb.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
    uint64_t n_bases = hb.n_bases(); // (of the block as it goes on: the trimmed block's, once the trim stage has replaced it)
    o.reads_seen = n_reads;
    o.bases_seen = n_bases;
    bool keeping = kept_cap_ && !kept_broken_;
    if (n_bases == 0) { // only empty reads: the lower bound decides, there is nothing to copy and nothing to map (the counters still see them)
        o.dropped_short = f.min_len ? n_reads : 0;
        o.reads_kept = o.mapped_reads = n_reads - o.dropped_short;
        tot_reads_ += o.reads_kept;
        if (keeping) kept_seen_ += o.reads_kept;
        return;
    }
    if (f.trim_qual_milli && !hb.qual) throw Error(DRPRG_EINVAL, "--trim-qual: the reads came without base qualities");
    if (f.use_qual() && !hb.qual) throw Error(DRPRG_EINVAL, "--min-read-qual: the reads came without base qualities");
    if (n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
    if (!copy_stream_) copy_stream_.create();
    const hipStream_t cs = copy_stream_;
    // (the batch that used this staging set two calls ago was completed by the previous call: map_host_async)
    Stage& st = stage_[stage_next_];
    stage_next_ ^= 1;
    if (!st.copied) st.copied.create(false);
    FilterScratch& fs = st.filt;
    uint64_t n_npos = hb.packed || hb.bam ? hb.n_npos : 0;
    ensure_stage(st, hb.payload_bytes(), n_reads, n_npos);
    ensure_filter_scratch(fs, n_reads, f.wants_qual() ? n_bases : 0, true, f.use_qual());
    if (f.trims()) ensure_trim_scratch(fs, n_reads, n_npos, f.trim_qual_milli != 0, true, f.any_adapters(), n_npos ? n_bases : 0);
    DeviceBatch src = hb.bam ? copy_in_bam(hb, st, st.d_bases.data(), st.d_offsets.data(), st.d_npos.data(), cs, cs)
                             : copy_in(hb, st.d_bases.data(), st.d_offsets.data(), st.d_npos.data(), cs);
    if (f.wants_qual()) {
        HIPCHK(hipMemcpyAsync(fs.d_qual.data(), hb.qual, n_bases, hipMemcpyHostToDevice, cs));
        HIPCHK(hipMemsetAsync(fs.d_qual.data() + n_bases, 0, 64, cs));
    }
    const uint8_t* d_q = fs.d_qual.data();
    uint32_t trim_err = 0;
    if (f.trims()) {
        // The trim stage: the kept range of every read, the new offsets and the counts, one read-back; a block that lost a base is compacted
        // into the set's t_* buffers (launch_subsample_pack for words, launch_gather_reads for text and for the quality bytes) and `src`
        // and the quality pointer are REPLACED: the filter, the depth cut, the compaction and keep_reads below see a block of trimmed reads.
        const uint8_t* d_rev = hb.bam && hb.reverse ? st.d_reverse.data() : nullptr; // (BAM: QUAL stays in stored order; the bases were reversed by bam_pack_kernel)
        dev::AdapterPoints pts {}; // (adapters: sought in what the crops and the quality trim leave, bases in read orientation; a packed block's bitmap first)
        if (f.any_adapters()) pts = adapter_points(fs, src.d_bases, src.packed, src.d_npos, src.n_npos, n_bases, cs);
        run_read_trim(fs, f, d_q, hb.qual_bias, src.d_offsets, d_rev, n_reads, n_bases, fs.t_begin.data(), fs.t_end.data(), src.d_npos, src.n_npos, cs, &pts);
        HIPCHK(hipStreamSynchronize(cs)); // the trim's read-back: the trimmed sizes are known before the filter is launched
        const unsigned long long* t = fs.t_out.data();
        if (t[dev::RT_BAD_AT] == ~0ull) throw Error(DRPRG_EINVAL, "read trimming: the block's offsets do not ascend to its number of bases");
        if (t[dev::RT_BAD_AT])
            throw Error(DRPRG_EFORMAT, "a base quality outside 0..93 (quality byte " + std::to_string(t[dev::RT_BAD_AT] - 1) + " of an ingest block of "
                    + std::to_string(n_bases) + " bases, " + (hb.qual_bias ? "FASTQ: bytes 33..126" : "BAM: bytes 0..93") + ")");
        if (f.crops()) {
            o.trim.reads_seen = n_reads; o.trim.bases_seen = n_bases; o.trim.reads_lost_base = t[dev::RT_LOST_READS];
            o.trim.cut_front = t[dev::RT_CUT_FRONT]; o.trim.cut_tail = t[dev::RT_CUT_TAIL]; o.trim.qcut_front = t[dev::RT_QCUT_FRONT];
            o.trim.qcut_tail = t[dev::RT_QCUT_TAIL]; o.trim.emptied = t[dev::RT_EMPTIED];
        }
        if (f.adapters.n) {
            o.adapter.reads_seen = n_reads; o.adapter.bases_seen = t[dev::RT_AD_BASES_SEEN]; o.adapter.reads_cut = t[dev::RT_AD_READS_CUT];
            o.adapter.bases_cut = t[dev::RT_AD_BASES_CUT]; o.adapter.reads_emptied = t[dev::RT_AD_EMPTIED];
        }
        if (f.front_adapters.n) {
            o.front.reads_seen = n_reads; o.front.bases_seen = t[dev::RT_FA_BASES_SEEN]; o.front.reads_cut = t[dev::RT_FA_READS_CUT];
            o.front.bases_cut = t[dev::RT_FA_BASES_CUT]; o.front.reads_emptied = t[dev::RT_FA_EMPTIED];
        }
        if (t[dev::RT_LOST_READS] || t[dev::RT_AD_READS_CUT] || t[dev::RT_FA_READS_CUT]) { // the block lost a base to any cause
            const uint64_t nb = t[dev::RT_KEPT_BASES], n_list = src.n_npos ? t[dev::RT_KEPT_NPOS] : 0;
            o.bases_seen = nb;
            if (nb == 0) { // every base of the block is gone: reads of no bases, nothing to map; the set is handed back (see below)
                stage_next_ ^= 1;
                o.dropped_short = f.min_len ? n_reads : 0;
                o.reads_kept = o.mapped_reads = n_reads - o.dropped_short;
                tot_reads_ += o.reads_kept;
                if (keeping) kept_seen_ += o.reads_kept;
                return;
            }
            const uint64_t payload = src.packed ? (nb + 15) / 16 * 4 : nb;
            auto room = [&](auto& buf, uint64_t need) {
                if (need <= buf.size()) return;
                sync();
                buf.alloc(need + need / 4);
            };
            room(fs.t_bases, payload + 64);
            if (n_list) room(fs.t_npos, n_list);
            if (f.use_qual()) room(fs.t_qual, nb + 64);
            if (src.packed) room(fs.t_src, n_reads);
            if (!src.packed) room(fs.t_btable, n_reads);
            if (f.use_qual()) room(fs.t_qtable, n_reads);
            uint32_t* const d_err = reinterpret_cast<uint32_t*>(fs.t_work.data() + dev::RT_KEPT_NPOS); // (zeroed with the trim's words, unused on the device)
            dev::ReadTrimFill tf { src.d_offsets, d_rev, fs.t_begin.data(), fs.t_end.data(), fs.t_offsets.data(), n_reads, n_bases, nb, src.d_bases, d_q,
                src.packed ? fs.t_src.data() : nullptr, src.packed ? nullptr : fs.t_btable.data(), f.use_qual() ? fs.t_qtable.data() : nullptr, d_err };
            HIPCHK(dev::launch_read_trim_fill(tf, cs));
            HIPCHK(hipMemsetAsync(fs.t_bases.data() + payload, 0, 64, cs));
            if (src.packed) {
                const dev::SubsampleBlock sb { src.d_bases, src.d_offsets, n_reads, n_bases, 0, nullptr, nullptr, nullptr, n_reads, nb };
                HIPCHK(dev::launch_subsample_pack(sb, fs.t_offsets.data(), fs.t_src.data(), reinterpret_cast<uint32_t*>(fs.t_bases.data()), d_err, cs));
                if (n_list) {
                    const dev::ReadTrimNpos np { src.d_npos, src.n_npos, fs.t_count.data(), fs.t_prefix.data(), fs.t_ntemp.data(), fs.t_ntemp.size() };
                    HIPCHK(dev::launch_read_trim_npos_emit(tf, np, fs.t_npos.data(), n_list, cs));
                }
            } else HIPCHK(dev::launch_gather_reads(fs.t_btable.data(), (uint32_t)n_reads, fs.t_bases.data(), cs));
            if (f.use_qual()) {
                HIPCHK(dev::launch_gather_reads(fs.t_qtable.data(), (uint32_t)n_reads, fs.t_qual.data(), cs));
                HIPCHK(hipMemsetAsync(fs.t_qual.data() + nb, 0, 64, cs));
                d_q = fs.t_qual.data();
            }
            HIPCHK(hipMemcpyAsync(&trim_err, d_err, sizeof trim_err, hipMemcpyDeviceToHost, cs)); // (queued behind the compaction; waited for with the filter's read-back)
            src.d_bases = fs.t_bases.data();
            src.d_offsets = fs.t_offsets.data();
            src.n_bases = n_bases = nb;
            src.d_npos = n_list ? fs.t_npos.data() : nullptr;
            src.n_npos = n_npos = n_list;
        }
    }
    run_read_filter(fs, f, d_q, hb.qual_bias, src.d_offsets, n_reads, n_bases, fs.d_qsum.data(), fs.d_flag.data(), cs);
    HIPCHK(hipStreamSynchronize(cs)); // the caller's block is free again; the filter's read-back is here
    if (trim_err) throw Error(DRPRG_EIO, "read trimming: the block's offsets and the trimmed ranges do not fit each other");
    const unsigned long long* h = fs.h_out.data();
    if (h[dev::RF_OFFSETS]) throw Error(DRPRG_EINVAL, "read filter: the block's offsets do not ascend to its number of bases");
    if (h[dev::RF_BAD_AT])
        throw Error(DRPRG_EFORMAT, "a base quality outside 0..93 (quality byte " + std::to_string(h[dev::RF_BAD_AT] - 1) + " of an ingest block of "
                + std::to_string(n_bases) + " bases, " + (hb.qual_bias ? "FASTQ: bytes 33..126" : "BAM: bytes 0..93") + ")");
    o.dropped_short = h[dev::RF_SHORT];
    o.dropped_long = h[dev::RF_LONG];
    o.dropped_lowq = h[dev::RF_LOWQ];
    o.reads_kept = h[dev::RF_KEPT_READS];
    o.bases_kept = h[dev::RF_KEPT_BASES];
    uint64_t take = n_reads, nr = o.reads_kept, nb = o.bases_kept; // the block's first `take` reads hold the nr reads and nb bases that go on
    if (cap_need && nb >= cap_need) {
        // the cut, in the block's own numbering: boff is the running total of the kept bases (covg_cut.hip on the scan instead of the offsets)
        if (!h_cut_) h_cut_.alloc(4);
        HIPCHK(dev::launch_covg_cut(fs.d_boff.data(), n_reads, cap_need, nullptr, 0, h_cut_.device_ptr(), cs));
        HIPCHK(hipStreamSynchronize(cs));
        take = h_cut_[0];
        nb = h_cut_[1];
        uint32_t rk = 0;
        HIPCHK(hipMemcpyAsync(&rk, fs.d_rank.data() + take, sizeof rk, hipMemcpyDeviceToHost, cs));
        HIPCHK(hipStreamSynchronize(cs));
        o.cut = true;
        o.cut_dropped = nr - rk;
        nr = rk;
    }
    o.mapped_reads = nr;
    o.mapped_bases = nb;
    if (nb == 0) { // nothing of the block is left, or empty reads only
        // No map call follows, so nothing completes the batch in flight -- whose kernels read the OTHER staging set.  This set is handed back:
        // the next block takes it again, and the sets keep their rule (the batch that used a set before was completed by the map call
        // between).  Were the turn kept, the next block's copies would overwrite what the batch in flight is still reading.
        stage_next_ ^= 1;
        tot_reads_ += nr;
        if (keeping) kept_seen_ += nr;
        return;
    }
    const bool compact = nr != n_reads;
    const uint64_t payload = src.packed ? (nb + 15) / 16 * 4 : nb;
    const dev::SubsampleBlock sb { src.d_bases, src.d_offsets, take, src.n_bases, 0, fs.d_flag.data(), fs.d_rank.data(), fs.d_boff.data(), nr, nb };
    // how many of the block's listed positions go on: all of them, or -- counted before any room is taken for them -- those in kept reads
    uint64_t n_list = n_npos;
    if (compact && src.n_npos) {
        const uint64_t chunks = (uint64_t)dev::subsample_npos_chunks(src.n_npos) + 1;
        const size_t temp = dev::scan_temp_bytes((uint32_t)chunks);
        if (chunks > fs.d_count.size()) fs.d_count.alloc(chunks + chunks / 4);
        if (chunks > fs.d_prefix.size()) fs.d_prefix.alloc(chunks + chunks / 4);
        if (temp > fs.d_ntemp.size()) fs.d_ntemp.alloc(temp + temp / 4);
        HIPCHK(dev::launch_subsample_npos_count(sb, src.d_npos, src.n_npos, fs.d_count.data(), fs.d_prefix.data(), fs.d_ntemp.data(), fs.d_ntemp.size(), cs));
        uint32_t cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, fs.d_prefix.data() + (chunks - 1), sizeof cnt, hipMemcpyDeviceToHost, cs));
        HIPCHK(hipStreamSynchronize(cs));
        n_list = cnt;
    } else if (compact) n_list = 0;
    uint8_t* db = nullptr;
    uint64_t *doff = nullptr, *dnp = nullptr;
    if (keeping) {
        db = static_cast<uint8_t*>(arena_take(payload + 64));
        doff = db ? static_cast<uint64_t*>(arena_take((nr + 1) * sizeof(uint64_t))) : nullptr;
        dnp = doff && n_list ? static_cast<uint64_t*>(arena_take(n_list * sizeof(uint64_t))) : nullptr;
        if (!db || !doff || (n_list && !dnp)) {
            stop_keeping();
            keeping = false;
        }
    }
    DeviceBatch cur = src;
    if (compact || keeping) {
        if (!keeping) {
            if (payload + 64 > fs.c_bases.size() || nr + 1 > fs.c_offsets.size() || n_list > fs.c_npos.size()) sync();
            fs.c_bases.reserve(payload + 64, payload + payload / 4 + 64);
            fs.c_offsets.reserve(nr + 1, nr + nr / 4 + 1);
            fs.c_npos.reserve(n_list, n_list + n_list / 4 + 16);
            db = fs.c_bases.data();
            doff = fs.c_offsets.data();
            dnp = fs.c_npos.data();
        }
        cur.d_bases = db;
        cur.d_offsets = doff;
        cur.n_reads = nr;
        cur.n_bases = nb;
        HIPCHK(hipMemsetAsync(db + payload, 0, 64, cs));
        if (!compact) { // the whole block, copied on the device to where it stays
            HIPCHK(hipMemcpyAsync(db, src.d_bases, payload, hipMemcpyDeviceToDevice, cs));
            HIPCHK(hipMemcpyAsync(doff, src.d_offsets, (nr + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, cs));
            if (src.n_npos) HIPCHK(hipMemcpyAsync(dnp, src.d_npos, src.n_npos * sizeof(uint64_t), hipMemcpyDeviceToDevice, cs));
            cur.d_npos = src.n_npos ? dnp : nullptr;
            HIPCHK(hipStreamSynchronize(cs)); // (the block is whole before anything on the mapping stream reads it)
        } else {
            uint32_t* const d_err = reinterpret_cast<uint32_t*>(fs.d_work.data() + 7); // (zeroed with the filter's words)
            cur.d_npos = nullptr;
            cur.n_npos = 0;
            if (src.packed) {
                if (nr > fs.d_src.size()) fs.d_src.alloc(nr + nr / 4);
                HIPCHK(dev::launch_subsample_tables(sb, doff, fs.d_src.data(), nullptr, d_err, cs));
                HIPCHK(dev::launch_subsample_pack(sb, doff, fs.d_src.data(), reinterpret_cast<uint32_t*>(db), d_err, cs));
                if (n_list) { // (counted above; the scan of the counts is still in d_prefix)
                    HIPCHK(dev::launch_subsample_npos_emit(sb, src.d_npos, src.n_npos, fs.d_prefix.data(), dnp, n_list, cs));
                    cur.d_npos = dnp;
                    cur.n_npos = n_list;
                }
            } else {
                if (nr > fs.d_table.size()) fs.d_table.alloc(nr + nr / 4);
                HIPCHK(hipMemsetAsync(fs.d_table.data(), 0, nr * sizeof(dev::GatherEntry), cs)); // (an entry the kernel refuses to fill copies nothing)
                HIPCHK(dev::launch_subsample_tables(sb, doff, nullptr, fs.d_table.data(), d_err, cs));
                HIPCHK(dev::launch_gather_reads(fs.d_table.data(), (uint32_t)nr, db, cs));
            }
            uint32_t err = 0;
            HIPCHK(hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, cs));
            HIPCHK(hipStreamSynchronize(cs));
            if (err) throw Error(DRPRG_EIO, "read filter: the block's offsets and the filter's scans do not fit each other");
        }
    }
    if (keeping) {
        kept_.push_back(cur);
        kept_first_.push_back(kept_seen_);
        kept_seen_ += nr;
    }
    in_keep_call_ = keeping;
    try {
        map(cur, nullptr, nullptr, stream_, true);
    } catch (...) {
        in_keep_call_ = false;
        throw;
    }
    in_keep_call_ = false;
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
    if (kept_cap_) kept_broken_ = true; // coverage that came without its reads

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
