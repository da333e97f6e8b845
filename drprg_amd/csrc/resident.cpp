// resident.cpp -- the reads that stay in device memory (keep_reads): the arenas, the one compaction by flags, random subsample, duplicate
// removal and the read selection for discover.  See mapper.h.
#include "mapper.h"
#include <algorithm>
#include <cstdio>
#include <hip/hip_runtime.h>

namespace drprg {

void* Mapper::ResidentSet::arena_take(size_t n)
{
    n = (n + 255) / 256 * 256;
    if (bytes + n > cap) return nullptr;
    if (n > left) {
        // (what is left of the current piece is not used: pieces are 256 MB, blocks ~25 MB)
        const size_t piece = std::max<size_t>(n, std::min<uint64_t>(256ull << 20, cap - bytes));
        DeviceBuffer<uint8_t> arena;
        try {
            arena.alloc(piece);
        } catch (const Error&) { // (the device is full: the caller goes on without resident reads)
            (void)hipGetLastError();
            return nullptr;
        }
        arenas.push_back(std::move(arena));
        at = arenas.back().data();
        left = piece;
    }
    void* r = at;
    at += n;
    left -= n;
    bytes += n;
    return r;
}

std::optional<Mapper::BlockRoom> Mapper::ResidentSet::take_block(uint64_t payload_bytes, uint64_t n_reads, uint64_t n_npos)
{
    BlockRoom r {};
    if (!(r.bases = static_cast<uint8_t*>(arena_take(payload_bytes + 64)))) return std::nullopt;
    if (!(r.offsets = static_cast<uint64_t*>(arena_take((n_reads + 1) * sizeof(uint64_t))))) return std::nullopt;
    if (n_npos && !(r.npos = static_cast<uint64_t*>(arena_take(n_npos * sizeof(uint64_t))))) return std::nullopt;
    return r;
}

void Mapper::keep_reads(uint64_t max_bytes)
{
    drop_kept();
    resident_.cap = max_bytes;
    // reads mapped before this call are not resident: kept_complete() must not claim them (map_resident would map a subset)
    resident_.broken = tot_reads_ != 0;
}

void Mapper::drop_kept()
{
    if (!resident_.arenas.empty()) {
        sync();
        HIPCHK(hipSetDevice(device_));
        HIPCHK(hipStreamSynchronize(stream_));
    }
    resident_.clear();
    const bool record = pair_.record, dedup = pair_.dedup;
    pair_ = PairState {};
    pair_.record = record;
    pair_.dedup = dedup;
}

// The map call on a block of the resident set.  in_keep_call_ is set for as long as it runs and on no other path: map() takes every other
// batch for reads of the caller's own buffers and marks the set broken.
void Mapper::map_resident_block(const DeviceBatch& b)
{
    struct Guard {
        bool& flag;
        explicit Guard(bool& f) : flag(f) { flag = true; }
        ~Guard() { flag = false; }
    } guard(in_keep_call_);
    map(b, nullptr, nullptr, stream_, true);
}

uint64_t Mapper::map_kept_from(const Mapper& other)
{
    if (other.device_ != device_) throw Error(DRPRG_EINVAL, "the kept reads live on another device");
    if (!other.kept_complete()) throw Error(DRPRG_ENODATA, "the other context does not hold all of its reads");
    uint64_t n = 0;
    for (const DeviceBatch& b : other.resident_.kept) {
        map(b, nullptr, nullptr, stream_, true);
        n += b.n_reads;
    }
    sync();
    HIPCHK(hipStreamSynchronize(stream_));
    return n;
}

// over the limit (or the device is full): nothing is kept from here on, and what was kept is of no use without the rest
void Mapper::stop_keeping()
{
    const uint64_t cap = resident_.cap;
    drop_kept(); // (the cap stays)
    resident_.broken = true;
    // (said once per context, always: the run takes a different, slower route from here -- results are the same)
    std::fprintf(stderr, "[drprg-hip] the sample is larger than the %.1f GB of device memory set aside for resident reads (device %d): reads are "
                         "not kept, later passes read the file again (DRPRG_HIP_KEEP_READS_GB raises the limit)\n", (double)cap / 1e9, device_);
}

// What subsample_kept and dedup_kept begin with: the whole sample is resident, nothing is in flight, and what the sample holds.
Mapper::SubsampleResult Mapper::resident_sample(const char* what, std::vector<uint8_t>& flags)
{
    if (!kept_complete())
        throw Error(DRPRG_ENODATA, std::string(what) + ": not every read of the sample is resident in device memory (drprg_hip_keep_reads is off, or the "
                                   "sample is larger than its limit; the executables take the limit from DRPRG_HIP_KEEP_READS_GB)");
    sync();
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipStreamSynchronize(stream_));
    flags.clear();
    uint64_t bases = 0;
    for (const DeviceBatch& b : resident_.kept) bases += b.n_bases;
    return SubsampleResult { resident_.seen, bases, resident_.seen, bases };
}

Mapper::SubsampleResult Mapper::subsample_kept(uint64_t target_bases, uint64_t seed, std::vector<uint8_t>& flags)
{
    SubsampleResult res = resident_sample("random subsample", flags);
    const uint64_t n = res.reads_before;
    if (res.bases_before <= target_bases) return res;
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
    for (size_t b = 0; b < resident_.kept.size(); ++b)
        HIPCHK(dev::launch_subsample_lengths(resident_.kept[b].d_offsets, resident_.kept[b].n_reads, resident_.first[b], n, d_len.data(), stream_));
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
// reads / bases before read i (n + 1 entries, n = resident_.seen; device memory).  Every resident block is compacted into a block of its kept
// reads in arenas of their own, the old set stays where it is if that fails, coverage and counters are cleared and the new set is mapped.  d_err:
// a zeroed device word.  res.reads_kept / bases_kept and flags (the device flags, or empty after a failure) are filled here.
void Mapper::keep_flagged(const uint8_t* d_flag, const uint32_t* d_rank, const uint64_t* d_boff, uint32_t* d_err, const char* what, SubsampleResult& res,
    std::vector<uint8_t>& flags)
{
    const uint64_t n = resident_.seen;
    DeviceBuffer<uint64_t> d_first;
    DeviceBuffer<unsigned long long> d_bounds;
    // kept reads and bases in front of every block's first read, behind its last one, and in all
    std::vector<uint64_t> first;
    for (size_t b = 0; b < resident_.kept.size(); ++b) {
        first.push_back(resident_.first[b]);
        first.push_back(resident_.first[b] + resident_.kept[b].n_reads);
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
    // ---- compaction: a new set under the same cap, in arenas of its own.  It takes the old one's place only once the error word has read
    // back clean: a failure before that leaves the sample as it was.  The old arenas are released by their owners when this scope is left ----
    ResidentSet fresh;
    fresh.cap = resident_.cap;
    try {
        const std::vector<DeviceBatch>& old = resident_.kept;
        CompactScratch scratch;
        for (size_t b = 0; b < old.size(); ++b) // (room for the largest block first: no block below waits for a regrow)
            compact_room(scratch, old[b].packed, bounds[4 * b + 2] - bounds[4 * b], old[b].packed ? old[b].n_npos : 0);
        for (size_t b = 0; b < old.size(); ++b) {
            const DeviceBatch& ob = old[b];
            const uint64_t nr = bounds[4 * b + 2] - bounds[4 * b], nb = bounds[4 * b + 3] - bounds[4 * b + 1];
            if (nb == 0) continue; // (nothing of the block is kept, or empty reads only: they are numbered below, as map_host_async counts them)
            const uint64_t payload = ob.packed ? (nb + 15) / 16 * 4 : nb;
            const dev::SubsampleBlock sb { ob.d_bases, ob.d_offsets, ob.n_reads, ob.n_bases, resident_.first[b], d_flag, d_rank, d_boff, nr, nb };
            fresh.count_empty(bounds[4 * b] - fresh.seen); // (kept reads in front of the block that lie in no block)
            const DeviceBatch kb = compact_block(sb, ob, scratch, d_err, stream_, [&](uint64_t n_list) {
                const std::optional<BlockRoom> room = fresh.take_block(payload, nr, n_list);
                if (!room) throw Error(DRPRG_ENOMEM, std::string(what) + ": no device memory for the kept reads beside the resident sample");
                return *room;
            });
            fresh.add(kb, nr);
        }
        fresh.count_empty(res.reads_kept - fresh.seen);
        compaction_clean(d_err, std::string(what) + ": the resident blocks' offsets and the selection do not fit each other");
    } catch (...) {
        (void)hipStreamSynchronize(stream_); // (nothing writes the new arenas any more when their owners release them)
        flags.clear();
        throw;
    }
    adopt_kept(fresh, res.reads_kept);
}

void Mapper::compaction_clean(uint32_t* d_err, const std::string& what)
{
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_)); // (nothing reads the old blocks any more)
    if (err) throw Error(DRPRG_EIO, what);
}

void Mapper::adopt_kept(ResidentSet& fresh, uint64_t reads_kept)
{
    std::swap(resident_, fresh);
    pair_.src.clear(); // (mate overlap: the numbers lay in the old arenas and stood for the old blocks)
    pair_.spent = true;
    pair_.release_record(); // (duplicate pairs: pair_overlap_kept, whose compaction keeps every read's number, hands its record over behind this call)
    // ---- the kept reads mapped afresh ----
    HIPCHK(hipMemsetAsync(d_covg_.data(), 0, d_covg_.bytes(), stream_)); // [coverage | reads per PRG]
    HIPCHK(hipMemsetAsync(d_counters_.data(), 0, d_counters_.bytes(), stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    tot_reads_ = tot_bases_ = tot_hits_ = tot_leftover_ = tot_minimizers_ = 0;
    uint64_t in_blocks = 0;
    for (const DeviceBatch& b : resident_.kept) {
        map_resident_block(b);
        in_blocks += b.n_reads;
    }
    sync();
    HIPCHK(hipStreamSynchronize(stream_));
    tot_reads_ += reads_kept - in_blocks; // (kept empty reads of blocks that hold no base any more)
}

void Mapper::compact_room(CompactScratch& cs, bool packed, uint64_t n_kept, uint64_t n_npos)
{
    if (packed) grow(cs.d_src, n_kept);
    else grow(cs.d_table, n_kept);
    if (!n_npos) return;
    const uint64_t chunks = (uint64_t)dev::subsample_npos_chunks(n_npos) + 1;
    grow(cs.d_count, chunks);
    grow(cs.d_prefix, chunks);
    grow(cs.d_ntemp, dev::scan_temp_bytes((uint32_t)chunks));
}

Mapper::DeviceBatch Mapper::compact_block(const dev::SubsampleBlock& sb, const DeviceBatch& src, CompactScratch& cs, uint32_t* d_err, hipStream_t stream,
    const std::function<BlockRoom(uint64_t n_list)>& room)
{
    const uint64_t nr = sb.new_reads, nb = sb.new_bases;
    const uint64_t n_npos = src.packed ? src.n_npos : 0; // (a text block lists none)
    compact_room(cs, src.packed, nr, n_npos);
    // how many of the block's listed positions lie in kept reads: counted before any room is taken for them (the scan of the counts stays
    // in d_prefix for the emit below)
    uint32_t n_list = 0;
    if (n_npos) {
        HIPCHK(dev::launch_subsample_npos_count(sb, src.d_npos, n_npos, cs.d_count.data(), cs.d_prefix.data(), cs.d_ntemp.data(), cs.d_ntemp.size(), stream));
        HIPCHK(hipMemcpyAsync(&n_list, cs.d_prefix.data() + dev::subsample_npos_chunks(n_npos), sizeof n_list, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    const BlockRoom dst = room(n_list);
    HIPCHK(hipMemsetAsync(dst.bases + (src.packed ? (nb + 15) / 16 * 4 : nb), 0, 64, stream));
    if (!src.packed) HIPCHK(hipMemsetAsync(cs.d_table.data(), 0, nr * sizeof(dev::GatherEntry), stream)); // (an entry the kernel refuses to fill copies nothing)
    HIPCHK(dev::launch_subsample_tables(sb, dst.offsets, src.packed ? cs.d_src.data() : nullptr, src.packed ? nullptr : cs.d_table.data(), d_err, stream));
    if (!src.packed) HIPCHK(dev::launch_gather_reads(cs.d_table.data(), (uint32_t)nr, dst.bases, stream));
    else HIPCHK(dev::launch_subsample_pack(sb, dst.offsets, cs.d_src.data(), reinterpret_cast<uint32_t*>(dst.bases), d_err, stream));
    if (n_list) HIPCHK(dev::launch_subsample_npos_emit(sb, src.d_npos, n_npos, cs.d_prefix.data(), dst.npos, n_list, stream));
    return DeviceBatch { dst.bases, dst.offsets, nr, nb, src.packed, n_list ? dst.npos : nullptr, n_list };
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
    SubsampleResult res = resident_sample("duplicate removal", flags);
    const uint64_t n = res.reads_before;
    uint64_t with_bases = 0; // (an upper bound: two reads with bases need two reads in blocks that hold bases)
    for (const DeviceBatch& b : resident_.kept) with_bases += b.n_bases ? b.n_reads : 0;
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
    std::vector<DedupBlock> blocks(resident_.kept.size()); // (the exact check reads every block: the scratch of all of them lives until it is done)
    for (size_t b = 0; b < resident_.kept.size(); ++b) {
        if (!resident_.kept[b].n_reads || !resident_.kept[b].n_bases) continue;
        if (resident_.first[b] + resident_.kept[b].n_reads > n) throw Error(DRPRG_EIO, "duplicate removal: the resident blocks hold more reads than the sample");
        dedup_block(resident_.kept[b], blocks[b], d_count.data());
        HIPCHK(dev::launch_dedup_keys(blocks[b].batch, reinterpret_cast<unsigned long long*>(d_key.data()) + resident_.first[b], d_err.data(), stream_));
        HIPCHK(dev::launch_dedup_loc(blocks[b].batch, resident_.first[b], n, d_loc.data(), d_err.data(), stream_));
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

// ---- mate overlap on the resident sample (the rule: include/drprg_hip.h "mate overlap") ------------------------------------------------
bool Mapper::pair_number_block(uint64_t n_reads, const uint8_t* d_flag, const uint32_t* d_rank, uint64_t src_reads, uint64_t take, uint64_t base, hipStream_t stream)
{
    uint32_t* const numbers = resident_.take_numbers(n_reads);
    if (!numbers) return false;
    // (a side of 2^32 reads or more is refused by the stage: the numbers of such a sample are never looked at)
    HIPCHK(dev::launch_pair_numbers(d_flag, d_rank, src_reads, take, (uint32_t)base, n_reads, numbers, nullptr, stream));
    pair_.src.push_back(numbers);
    return true;
}

void Mapper::begin_mates()
{
    if (!pair_.record) throw Error(DRPRG_EINVAL, "drprg_hip_begin_mates: no mate-overlap setting (drprg_hip_set_pair_overlap)");
    if (pair_.begun) throw Error(DRPRG_EINVAL, "drprg_hip_begin_mates: called twice for one sample (side 2 has begun already)");
    sync();
    pair_.begun = 1;
    pair_.side = 1;
    pair_.block2 = resident_.kept.size();
    pair_.n1 = resident_.seen;
}

void Mapper::pair_overlap_kept(const PairSetting& set, std::vector<int32_t>& shifts, uint64_t counts[dev::PO_WORDS], uint64_t* merged)
{
    if (set.merge && (set.clip || !merged)) throw Error(DRPRG_EINVAL, "mate merging: not beside the clip (drprg_hip_set_pair_merge)");
    if (merged)
        for (int i = 0; i < dev::PM_WORDS; ++i) merged[i] = 0;
    std::vector<uint8_t> unused;
    const SubsampleResult before = resident_sample("mate overlap", unused);
    if (copy_stream_) HIPCHK(hipStreamSynchronize(copy_stream_)); // (the numbers of filtered blocks were written there)
    const uint64_t n = before.reads_before, n1 = pair_.n1;
    const std::vector<DeviceBatch>& old = resident_.kept;
    if (!set.on()) throw Error(DRPRG_EINVAL, "mate overlap: no setting (drprg_hip_set_pair_overlap)");
    if (!pair_.begun) throw Error(DRPRG_EINVAL, "mate overlap: drprg_hip_begin_mates was not called: the sample has no second side");
    if (pair_.spent || pair_.src.size() != old.size())
        throw Error(DRPRG_EINVAL, "mate overlap: the resident reads are not numbered by side (they were compacted by an earlier stage, or mapped before "
                                  "drprg_hip_set_pair_overlap)");
    if (pair_.seen[0] != pair_.seen[1])
        throw Error(DRPRG_EFORMAT, "mate overlap: the two sides hold different numbers of reads (" + std::to_string(pair_.seen[0]) + " and " +
                                       std::to_string(pair_.seen[1]) + "): the files are not mates of each other");
    if (n >= (1ull << 32) || pair_.seen[0] >= (1ull << 32)) throw Error(DRPRG_EOVERFLOW, "mate overlap: 2^32 reads or more in one sample");
    const uint64_t pairs = pair_.seen[0];
    shifts.assign(pairs, dev::PO_NOT_JUDGED);
    for (int i = 0; i < dev::PO_WORDS; ++i) counts[i] = 0;
    counts[dev::PO_PAIRS] = pairs;
    counts[dev::PO_READS] = n;
    counts[dev::PO_BASES_BEFORE] = counts[dev::PO_BASES_KEPT] = before.bases_before;
    if (n == 0) return;
    // ---- mates and kept lengths (device scratch of this call) ----
    uint64_t m[2] = { 0, 0 }, max_reads = 0, max_npos = 0;
    for (size_t b = 0; b < old.size(); ++b) {
        if (resident_.first[b] + old[b].n_reads > n || (b < pair_.block2) != (resident_.first[b] < n1))
            throw Error(DRPRG_EIO, "mate overlap: the resident blocks and the sides do not fit each other");
        m[b >= pair_.block2] += old[b].n_reads;
        max_reads = std::max(max_reads, old[b].n_reads);
        if (old[b].packed) max_npos = std::max(max_npos, old[b].n_npos);
    }
    DeviceBuffer<uint32_t> d_src, d_res, d_mate, d_err;
    DeviceBuffer<int32_t> d_shift;
    DeviceBuffer<uint64_t> d_keep;
    DeviceBuffer<dev::DedupLoc> d_loc;
    DeviceBuffer<unsigned long long> d_counts, d_count;
    d_src.alloc(m[0] + m[1] + 1); d_res.alloc(m[0] + m[1] + 1); d_mate.alloc(n); d_err.alloc(4); d_shift.alloc(n1 + 1); d_keep.alloc(n + 1); d_loc.alloc(n);
    d_counts.alloc(dev::PO_WORDS); d_count.alloc(1);
    HIPCHK(hipMemsetAsync(d_loc.data(), 0, d_loc.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_mate.data(), 0xFF, d_mate.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_err.data(), 0, d_err.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_keep.data(), 0, d_keep.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_counts.data(), 0, d_counts.bytes(), stream_));
    std::vector<DedupBlock> blocks(old.size()); // (the overlap kernel reads every block: the scratch of all of them lives until it is done)
    uint64_t at = 0;
    for (size_t b = 0; b < old.size(); ++b) {
        const uint64_t nr = old[b].n_reads;
        if (!nr) continue;
        HIPCHK(hipMemcpyAsync(d_src.data() + at, pair_.src[b], nr * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream_));
        HIPCHK(dev::launch_pair_numbers(nullptr, nullptr, nr, ~0ull, (uint32_t)resident_.first[b], nr, d_res.data() + at, nullptr, stream_));
        at += nr;
        if (!old[b].n_bases) continue;
        dedup_block(old[b], blocks[b], d_count.data());
        HIPCHK(dev::launch_dedup_loc(blocks[b].batch, resident_.first[b], n, d_loc.data(), d_err.data(), stream_));
    }
    HIPCHK(dev::launch_pair_mates(d_src.data(), d_res.data(), (uint32_t)m[0], d_src.data() + m[0], d_res.data() + m[0], (uint32_t)m[1], n, d_mate.data(), d_err.data(),
        stream_));
    DeviceBuffer<uint32_t> d_srcno; // duplicate pairs: the source number of every resident read, kept with d_mate when that stage is switched on
    if (pair_.dedup) {
        d_srcno.alloc(n);
        HIPCHK(hipMemsetAsync(d_srcno.data(), 0xFF, d_srcno.bytes(), stream_));
        HIPCHK(dev::launch_pair_source_numbers(d_src.data(), d_res.data(), (uint32_t)(m[0] + m[1]), n, d_srcno.data(), d_err.data(), stream_));
    }
    const auto hand_over = [&] {
        if (!pair_.dedup) return;
        pair_.d_mate = std::move(d_mate);
        pair_.d_srcno = std::move(d_srcno);
        pair_.pairs = pairs;
        pair_.ready = true;
    };
    dev::PairOverlapArgs args {};
    args.loc = d_loc.data(); args.mate = d_mate.data(); args.n = n; args.n1 = n1;
    args.min_overlap = set.min_overlap; args.error_milli = set.error_milli; args.clip = set.clip ? 1 : 0; args.merge = set.merge ? 1 : 0;
    args.shift = d_shift.data(); args.keep = d_keep.data(); args.counts = d_counts.data(); args.err = d_err.data();
    HIPCHK(dev::launch_pair_overlap(args, stream_));
    uint32_t err = 0;
    unsigned long long got[dev::PO_WORDS];
    std::vector<int32_t> shift(n1);
    std::vector<uint32_t> src1(m[0]);
    std::vector<uint64_t> keep(n);
    HIPCHK(hipMemcpyAsync(&err, d_err.data(), sizeof err, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(got, d_counts.data(), sizeof got, hipMemcpyDeviceToHost, stream_));
    if (n1) HIPCHK(hipMemcpyAsync(shift.data(), d_shift.data(), n1 * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    if (m[0]) HIPCHK(hipMemcpyAsync(src1.data(), d_src.data(), m[0] * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(keep.data(), d_keep.data(), n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    if (err) throw Error(DRPRG_EIO, "mate overlap: a resident block's offsets do not fit its bases, or its source numbers do not fit the sample");
    at = 0;
    for (size_t b = 0; b < pair_.block2 && b < old.size(); ++b)
        for (uint64_t j = 0; j < old[b].n_reads; ++j, ++at) {
            if (src1[at] >= pairs) throw Error(DRPRG_EIO, "mate overlap: a source number beyond the side's reads");
            shifts[src1[at]] = shift[resident_.first[b] + j];
        }
    for (int i = 0; i < dev::PO_WORDS; ++i)
        if (i != dev::PO_PAIRS && i != dev::PO_READS) counts[i] = got[i];
    // no read lost a base (every merged pair loses the columns both mates covered): nothing else happens
    if (counts[dev::PO_BASES_KEPT] == counts[dev::PO_BASES_BEFORE]) {
        pair_.src.clear(); // (the numbers are dropped after the stage)
        pair_.spent = true;
        hand_over();
        return;
    }
    // ---- compaction by the ranges [0, keep): a new set under the same cap, as keep_flagged makes one by flags ----
    DeviceBuffer<uint64_t> d_zero, d_noff, d_start;
    DeviceBuffer<dev::GatherEntry> d_table;
    DeviceBuffer<uint32_t> d_ccount, d_cprefix;
    DeviceBuffer<unsigned char> d_temp, d_ntemp;
    d_zero.alloc(max_reads + 1); d_noff.alloc(max_reads + 1); d_start.alloc(max_reads + 1); d_table.alloc(max_reads + 1);
    d_temp.alloc(dev::read_trim_temp_bytes(max_reads));
    if (max_npos) {
        const uint64_t chunks = (uint64_t)dev::read_trim_npos_chunks(max_npos) + 1;
        d_ccount.alloc(chunks); d_cprefix.alloc(chunks); d_ntemp.alloc(dev::scan_temp_bytes((uint32_t)chunks));
    }
    HIPCHK(hipMemsetAsync(d_zero.data(), 0, d_zero.bytes(), stream_));
    uint32_t* const d_cerr = d_err.data() + 1;
    // mate merging: one side-1 block laid out by the new lengths in d_noff (pair_merge.hip).  A packed block is written whole by the merge
    // kernel into zeroed words -- every merged read, and every other read's kept bases -- with the unknown bases of all of them in a bitmap
    // that becomes the block's ascending list; an ASCII block has its other reads copied byte for byte and its merged reads written as text
    DeviceBuffer<uint16_t> d_mbits;
    DeviceBuffer<uint32_t> d_mcount, d_mprefix;
    DeviceBuffer<unsigned char> d_mtemp;
    DeviceBuffer<unsigned long long> d_mwords;
    if (set.merge) {
        d_mwords.alloc(dev::PM_WORDS + 1);
        HIPCHK(hipMemsetAsync(d_mwords.data(), 0, d_mwords.bytes(), stream_));
    }
    ResidentSet fresh;
    fresh.cap = resident_.cap;
    const auto merge_block = [&](size_t b, uint64_t nb) {
        const DeviceBatch& ob = old[b];
        const uint64_t nr = ob.n_reads, first = resident_.first[b];
        const uint64_t n_words = (nb + 15) / 16, payload = ob.packed ? n_words * 4 : nb;
        const std::optional<BlockRoom> room = fresh.take_block(payload, nr, 0);
        if (!room) throw Error(DRPRG_ENOMEM, "mate merging: no device memory for the merged reads beside the resident sample");
        dev::PairMergeArgs m {};
        m.loc = d_loc.data(); m.mate = d_mate.data(); m.shift = d_shift.data(); m.n = n; m.n1 = n1; m.first = first; m.n_reads = nr;
        m.noff = d_noff.data(); m.new_bases = nb; m.counts = d_mwords.data(); m.err = d_cerr;
        uint64_t* list = nullptr;
        unsigned long long n_list = 0;
        if (ob.packed) {
            const uint64_t chunks = (uint64_t)dev::base_mask_tiles(nb) + 1;
            grow(d_mbits, (n_words + 8 + 3) / 4 * 4);
            grow(d_mcount, chunks);
            grow(d_mprefix, chunks);
            grow(d_mtemp, dev::scan_temp_bytes((uint32_t)chunks));
            unsigned long long* const d_listed = d_mwords.data() + dev::PM_WORDS;
            HIPCHK(hipMemsetAsync(d_mbits.data(), 0, (n_words + 8) * sizeof(uint16_t), stream_));
            HIPCHK(hipMemsetAsync(d_listed, 0, sizeof(unsigned long long), stream_));
            HIPCHK(hipMemsetAsync(room->bases, 0, payload + 64, stream_));
            m.words = reinterpret_cast<uint32_t*>(room->bases); m.nbits = d_mbits.data(); m.all = 1;
            HIPCHK(dev::launch_pair_merge(m, stream_));
            HIPCHK(dev::launch_pair_merge_bits_count(d_mbits.data(), nb, d_mcount.data(), d_listed, stream_));
            HIPCHK(hipMemcpyAsync(&n_list, d_listed, sizeof n_list, hipMemcpyDeviceToHost, stream_));
            HIPCHK(hipStreamSynchronize(stream_));
            if (n_list) {
                if (!(list = fresh.take_list(n_list))) throw Error(DRPRG_ENOMEM, "mate merging: no device memory for the merged reads beside the resident sample");
                HIPCHK(dev::launch_base_mask_emit(d_mbits.data(), nb, d_mcount.data(), d_mprefix.data(), d_mtemp.data(), d_mtemp.size(), list, n_list, stream_));
            }
        } else {
            HIPCHK(hipMemsetAsync(room->bases + payload, 0, 64, stream_));
            HIPCHK(dev::launch_pair_merge_table(ob.d_bases, ob.d_offsets, nr, ob.n_bases, first, n1, d_shift.data(), d_keep.data(), d_noff.data(), nb, d_table.data(), d_cerr,
                stream_));
            HIPCHK(dev::launch_gather_reads(d_table.data(), (uint32_t)nr, room->bases, stream_));
            m.text = room->bases;
            HIPCHK(dev::launch_pair_merge(m, stream_));
        }
        HIPCHK(hipMemcpyAsync(room->offsets, d_noff.data(), (nr + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream_));
        fresh.add(DeviceBatch { room->bases, room->offsets, nr, nb, ob.packed, list, (uint64_t)n_list }, nr);
    };
    try {
        for (size_t b = 0; b < old.size(); ++b) {
            const DeviceBatch& ob = old[b];
            const uint64_t nr = ob.n_reads, first = resident_.first[b];
            uint64_t nb = 0;
            for (uint64_t j = 0; j < nr; ++j) nb += keep[first + j];
            if (nb == 0) continue; // (reads of no bases only: numbered below, as map_host_async counts them)
            const uint64_t payload = ob.packed ? (nb + 15) / 16 * 4 : nb;
            const uint64_t n_npos = ob.packed ? ob.n_npos : 0;
            const uint64_t* const d_end = d_keep.data() + first;
            HIPCHK(dev::launch_pair_offsets(d_end, nr, d_noff.data(), d_temp.data(), d_temp.size(), stream_));
            if (set.merge && first < n1) { // a side-1 block under mate merging: the merged reads are written, not copied
                fresh.count_empty(first - fresh.seen);
                merge_block(b, nb);
                continue;
            }
            dev::ReadTrimFill tf { ob.d_offsets, nullptr, d_zero.data(), d_end, d_noff.data(), nr, ob.n_bases, nb, ob.d_bases, nullptr,
                ob.packed ? d_start.data() : nullptr, ob.packed ? nullptr : d_table.data(), nullptr, d_cerr };
            dev::ReadTrimNpos np {};
            uint32_t n_list = 0;
            if (n_npos) {
                np = dev::ReadTrimNpos { ob.d_npos, n_npos, d_ccount.data(), d_cprefix.data(), d_ntemp.data(), d_ntemp.size() };
                HIPCHK(dev::launch_read_trim_npos_count(tf, np, stream_));
                HIPCHK(hipMemcpyAsync(&n_list, d_cprefix.data() + dev::read_trim_npos_chunks(n_npos), sizeof n_list, hipMemcpyDeviceToHost, stream_));
                HIPCHK(hipStreamSynchronize(stream_));
            }
            const std::optional<BlockRoom> room = fresh.take_block(payload, nr, n_list);
            if (!room) throw Error(DRPRG_ENOMEM, "mate overlap: no device memory for the cut reads beside the resident sample");
            fresh.count_empty(first - fresh.seen); // (reads in front of the block that lie in no block)
            HIPCHK(hipMemsetAsync(room->bases + payload, 0, 64, stream_));
            HIPCHK(dev::launch_read_trim_fill(tf, stream_));
            if (ob.packed) {
                const dev::SubsampleBlock sb { ob.d_bases, ob.d_offsets, nr, ob.n_bases, 0, nullptr, nullptr, nullptr, nr, nb };
                HIPCHK(dev::launch_subsample_pack(sb, d_noff.data(), d_start.data(), reinterpret_cast<uint32_t*>(room->bases), d_cerr, stream_));
                if (n_list) HIPCHK(dev::launch_read_trim_npos_emit(tf, np, room->npos, n_list, stream_));
            } else HIPCHK(dev::launch_gather_reads(d_table.data(), (uint32_t)nr, room->bases, stream_));
            HIPCHK(hipMemcpyAsync(room->offsets, d_noff.data(), (nr + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream_));
            fresh.add(DeviceBatch { room->bases, room->offsets, nr, nb, ob.packed, n_list ? room->npos : nullptr, n_list }, nr);
        }
        fresh.count_empty(n - fresh.seen);
        if (set.merge) {
            unsigned long long mw[dev::PM_WORDS];
            HIPCHK(hipMemcpyAsync(mw, d_mwords.data(), sizeof mw, hipMemcpyDeviceToHost, stream_)); // (compaction_clean waits for it)
            compaction_clean(d_cerr, "mate merging: the resident blocks' offsets, the shifts and the new lengths do not fit each other");
            for (int i = 0; i < dev::PM_WORDS; ++i) merged[i] = mw[i];
        } else
            compaction_clean(d_cerr, "mate overlap: the resident blocks' offsets and the kept lengths do not fit each other");
    } catch (...) {
        (void)hipStreamSynchronize(stream_); // (nothing writes the new arenas any more when their owners release them)
        throw;
    }
    adopt_kept(fresh, n);
    hand_over();
}

namespace {
// what one call of the pair kernels on the caller's batches owns, up to and including launch_pair_overlap
struct PairDeviceRun {
    DeviceBuffer<uint16_t> d_bits[2];
    DeviceBuffer<uint32_t> d_err, d_src, d_res2, d_mate;
    DeviceBuffer<uint64_t> d_keep;
    DeviceBuffer<dev::DedupLoc> d_loc;
    DeviceBuffer<unsigned long long> d_counts;
};

void pair_device_launch(PairDeviceRun& r, const Mapper::PairSetting& set, const Mapper::PairSide& a, const Mapper::PairSide& b, uint64_t n_pairs, int32_t* d_shift,
    hipStream_t stream)
{
    if (!set.on()) throw Error(DRPRG_EINVAL, "mate overlap: no setting (drprg_hip_set_pair_overlap)");
    if (!a.d_offsets || !b.d_offsets || !d_shift || (a.n_bases && !a.d_words) || (b.n_bases && !b.d_words) || (a.n_npos && !a.d_npos) || (b.n_npos && !b.d_npos))
        throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_pairs >= (1ull << 31)) throw Error(DRPRG_EOVERFLOW, "mate overlap: 2^32 reads or more in one call");
    const uint64_t n = 2 * n_pairs;
    const Mapper::PairSide* side[2] = { &a, &b };
    r.d_err.alloc(2); r.d_src.alloc(n_pairs); r.d_res2.alloc(n_pairs); r.d_mate.alloc(n); r.d_keep.alloc(n + 1); r.d_loc.alloc(n); r.d_counts.alloc(dev::PO_WORDS + dev::PM_WORDS + 1);
    HIPCHK(hipMemsetAsync(r.d_err.data(), 0, r.d_err.bytes(), stream));
    HIPCHK(hipMemsetAsync(r.d_loc.data(), 0, r.d_loc.bytes(), stream));
    HIPCHK(hipMemsetAsync(r.d_mate.data(), 0xFF, r.d_mate.bytes(), stream));
    HIPCHK(hipMemsetAsync(r.d_keep.data(), 0, r.d_keep.bytes(), stream));
    HIPCHK(hipMemsetAsync(r.d_counts.data(), 0, r.d_counts.bytes(), stream));
    for (int s = 0; s < 2; ++s) {
        const Mapper::PairSide& p = *side[s];
        const uint64_t n_words = (p.n_bases + 15) / 16;
        if (p.n_npos) {
            r.d_bits[s].alloc(n_words + 8);
            HIPCHK(hipMemsetAsync(r.d_bits[s].data(), 0, r.d_bits[s].bytes(), stream));
            HIPCHK(dev::launch_mark_npos(p.d_npos, p.n_npos, p.n_bases, r.d_bits[s].data(), stream));
        }
        const dev::DedupBatch batch { p.d_words, p.n_npos ? r.d_bits[s].data() : nullptr, p.d_offsets, n_pairs, p.n_bases };
        HIPCHK(dev::launch_dedup_loc(batch, s * n_pairs, n, r.d_loc.data(), r.d_err.data(), stream));
    }
    // every read has the source number of its place, and side 2's resident numbers follow side 1's
    HIPCHK(dev::launch_pair_numbers(nullptr, nullptr, n_pairs, ~0ull, 0, n_pairs, r.d_src.data(), r.d_err.data(), stream));
    HIPCHK(dev::launch_pair_numbers(nullptr, nullptr, n_pairs, ~0ull, (uint32_t)n_pairs, n_pairs, r.d_res2.data(), r.d_err.data(), stream));
    HIPCHK(dev::launch_pair_mates(r.d_src.data(), r.d_src.data(), (uint32_t)n_pairs, r.d_src.data(), r.d_res2.data(), (uint32_t)n_pairs, n, r.d_mate.data(), r.d_err.data(),
        stream));
    dev::PairOverlapArgs args {};
    args.loc = r.d_loc.data(); args.mate = r.d_mate.data(); args.n = n; args.n1 = n_pairs;
    args.min_overlap = set.min_overlap; args.error_milli = set.error_milli; args.clip = set.clip ? 1 : 0; args.merge = set.merge ? 1 : 0;
    args.shift = d_shift; args.keep = r.d_keep.data(); args.counts = r.d_counts.data(); args.err = r.d_err.data();
    HIPCHK(dev::launch_pair_overlap(args, stream));
}
} // namespace

void Mapper::pair_overlap_device(const PairSetting& set, const PairSide& a, const PairSide& b, uint64_t n_pairs, int32_t* d_shift, uint64_t* d_keep_a, uint64_t* d_keep_b,
    uint64_t counts[dev::PO_WORDS], hipStream_t stream)
{
    for (int i = 0; i < dev::PO_WORDS; ++i) counts[i] = 0;
    if (n_pairs == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!d_keep_a || !d_keep_b) throw Error(DRPRG_EINVAL, "null device pointer");
    PairDeviceRun r;
    PairSetting plain = set;
    plain.merge = false; // (this entry states the cut: the kept lengths are those of the reads as they lie)
    pair_device_launch(r, plain, a, b, n_pairs, d_shift, stream);
    const uint64_t n = 2 * n_pairs;
    HIPCHK(hipMemcpyAsync(d_keep_a, r.d_keep.data(), n_pairs * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_keep_b, r.d_keep.data() + n_pairs, n_pairs * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    uint32_t err = 0;
    unsigned long long got[dev::PO_WORDS];
    HIPCHK(hipMemcpyAsync(&err, r.d_err.data(), sizeof err, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(got, r.d_counts.data(), sizeof got, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (err) throw Error(DRPRG_EINVAL, "mate overlap: the offsets of a side do not ascend inside its n_bases");
    for (int i = 0; i < dev::PO_WORDS; ++i) counts[i] = got[i];
    counts[dev::PO_PAIRS] = n_pairs;
    counts[dev::PO_READS] = n;
}

void Mapper::pair_merge_device(const PairSetting& set, const PairSide& a, const PairSide& b, uint64_t n_pairs, int32_t* d_shift, uint64_t* d_out_offsets, uint32_t* d_out_words,
    uint64_t cap_words, uint64_t* d_out_npos, uint64_t cap_npos, uint64_t* n_out_npos, uint64_t counts[dev::PO_WORDS], uint64_t merged[dev::PM_WORDS], hipStream_t stream)
{
    for (int i = 0; i < dev::PO_WORDS; ++i) counts[i] = 0;
    for (int i = 0; i < dev::PM_WORDS; ++i) merged[i] = 0;
    *n_out_npos = 0;
    if (n_pairs == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!set.merge) throw Error(DRPRG_EINVAL, "mate merging: the stage is not switched on (drprg_hip_set_pair_merge)");
    if (!d_out_offsets || (cap_words && !d_out_words) || (cap_npos && !d_out_npos)) throw Error(DRPRG_EINVAL, "null device pointer");
    PairDeviceRun r;
    pair_device_launch(r, set, a, b, n_pairs, d_shift, stream);
    const uint64_t n = 2 * n_pairs;
    // the merged batch's offsets: the new length of every merged a, nothing for any other pair
    DeviceBuffer<uint64_t> d_len;
    DeviceBuffer<unsigned char> d_temp;
    d_len.alloc(n_pairs + 1);
    d_temp.alloc(dev::read_trim_temp_bytes(n_pairs));
    HIPCHK(dev::launch_pair_merge_lengths(d_shift, r.d_keep.data(), n_pairs, d_len.data(), stream));
    HIPCHK(dev::launch_pair_offsets(d_len.data(), n_pairs, d_out_offsets, d_temp.data(), d_temp.size(), stream));
    uint32_t err = 0;
    uint64_t nb = 0;
    unsigned long long got[dev::PO_WORDS + dev::PM_WORDS + 1];
    HIPCHK(hipMemcpyAsync(&err, r.d_err.data(), sizeof err, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&nb, d_out_offsets + n_pairs, sizeof nb, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (err) throw Error(DRPRG_EINVAL, "mate overlap: the offsets of a side do not ascend inside its n_bases");
    const uint64_t n_words = (nb + 15) / 16;
    if (n_words > cap_words) throw Error(DRPRG_EOVERFLOW, "mate merging: the merged reads take " + std::to_string(n_words) + " words, the caller gave room for " +
                                                          std::to_string(cap_words));
    DeviceBuffer<uint16_t> d_obits;
    DeviceBuffer<uint32_t> d_ccount, d_cprefix;
    DeviceBuffer<unsigned char> d_ntemp;
    unsigned long long* const d_listed = r.d_counts.data() + dev::PO_WORDS + dev::PM_WORDS;
    if (nb) {
        const uint64_t chunks = (uint64_t)dev::base_mask_tiles(nb) + 1;
        d_obits.alloc((n_words + 8 + 3) / 4 * 4);
        d_ccount.alloc(chunks); d_cprefix.alloc(chunks); d_ntemp.alloc(dev::scan_temp_bytes((uint32_t)chunks));
        HIPCHK(hipMemsetAsync(d_obits.data(), 0, d_obits.bytes(), stream));
        HIPCHK(hipMemsetAsync(d_out_words, 0, n_words * sizeof(uint32_t), stream));
        dev::PairMergeArgs m {};
        m.loc = r.d_loc.data(); m.mate = r.d_mate.data(); m.shift = d_shift; m.n = n; m.n1 = n_pairs; m.first = 0; m.n_reads = n_pairs;
        m.noff = d_out_offsets; m.new_bases = nb; m.words = d_out_words; m.nbits = d_obits.data(); m.text = nullptr; m.all = 0;
        m.counts = r.d_counts.data() + dev::PO_WORDS; m.err = r.d_err.data() + 1;
        HIPCHK(dev::launch_pair_merge(m, stream));
        HIPCHK(dev::launch_pair_merge_bits_count(d_obits.data(), nb, d_ccount.data(), d_listed, stream));
    }
    HIPCHK(hipMemcpyAsync(&err, r.d_err.data() + 1, sizeof err, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(got, r.d_counts.data(), sizeof got, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (err) throw Error(DRPRG_EIO, "mate merging: the shifts, the mates and the merged batch's offsets do not fit each other");
    const uint64_t listed = got[dev::PO_WORDS + dev::PM_WORDS];
    if (listed > cap_npos) throw Error(DRPRG_EOVERFLOW, "mate merging: the merged reads hold " + std::to_string(listed) + " unknown bases, the caller gave room for " +
                                                        std::to_string(cap_npos));
    if (listed) {
        HIPCHK(dev::launch_base_mask_emit(d_obits.data(), nb, d_ccount.data(), d_cprefix.data(), d_ntemp.data(), d_ntemp.size(), d_out_npos, listed, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    *n_out_npos = listed;
    for (int i = 0; i < dev::PO_WORDS; ++i) counts[i] = got[i];
    counts[dev::PO_PAIRS] = n_pairs;
    counts[dev::PO_READS] = n;
    for (int i = 0; i < dev::PM_WORDS; ++i) merged[i] = got[dev::PO_WORDS + i];
}

// ---- duplicate pairs on the resident sample (the rule: include/drprg_hip.h "duplicate pairs") -------------------------------------------
namespace {
// the scratch of one launch_pair_dedup call over n reads and `pairs` units; what the caller owns itself stays null in `a`
struct PairDedupScratch {
    DeviceBuffer<uint64_t> skey, skey_sorted, klen, boff;
    DeviceBuffer<uint32_t> unit, idx, idx_sorted, root, flag32, rank, changed;
    DeviceBuffer<uint8_t> ubases, flag;
    DeviceBuffer<unsigned long long> out;
    DeviceBuffer<unsigned char> temp;
    void alloc(uint64_t n, uint64_t pairs, dev::PairDedupArgs& a)
    {
        skey.alloc(pairs); skey_sorted.alloc(pairs); klen.alloc(n + 1); boff.alloc(n + 1);
        unit.alloc(2 * pairs); idx.alloc(pairs); idx_sorted.alloc(pairs); root.alloc(pairs); flag32.alloc(n + 1); rank.alloc(n + 1);
        changed.alloc(dev::PD_ROUNDS + 1); ubases.alloc(pairs); flag.alloc(n); out.alloc(dev::PD_WORDS);
        temp.alloc(dev::subsample_scan_temp_bytes(std::max(n, pairs)));
        a.unit = unit.data(); a.skey = skey.data(); a.skey_sorted = skey_sorted.data(); a.idx = idx.data(); a.idx_sorted = idx_sorted.data();
        a.root = root.data(); a.ubases = ubases.data(); a.flag = flag.data(); a.flag32 = flag32.data(); a.rank = rank.data(); a.klen = klen.data();
        a.boff = boff.data(); a.out = out.data(); a.changed = changed.data(); a.temp = temp.data(); a.temp_bytes = temp.size();
    }
};
} // namespace

Mapper::SubsampleResult Mapper::dedup_pairs_kept(uint32_t key_bits, std::vector<uint8_t>& flags, uint64_t counts[8], uint64_t levels[32])
{
    if (key_bits < 1 || key_bits > 64) throw Error(DRPRG_EINVAL, "duplicate pairs: key_bits must be 1..64");
    SubsampleResult res = resident_sample("duplicate pairs", flags);
    if (!pair_.dedup) throw Error(DRPRG_EINVAL, "duplicate pairs: the stage is not switched on (drprg_hip_set_dedup_pairs, before drprg_hip_pair_overlap)");
    const uint64_t n = res.reads_before, n1 = pair_.n1;
    if (!pair_.ready || pair_.d_mate.size() != n || pair_.d_srcno.size() != n)
        throw Error(DRPRG_EINVAL, "duplicate pairs: the resident reads are not paired (no drprg_hip_pair_overlap call on this sample, or it has been compacted "
                                  "since by drprg_hip_dedup, drprg_hip_subsample or an earlier drprg_hip_dedup_pairs)");
    const uint64_t pairs = pair_.pairs;
    if (n >= (1ull << 32) || pairs >= (1ull << 32)) throw Error(DRPRG_EOVERFLOW, "duplicate pairs: 2^32 reads or pairs or more in one sample");
    for (int i = 0; i < 8; ++i) counts[i] = 0;
    for (int i = 0; i < 32; ++i) levels[i] = 0;
    counts[dev::PD_UNITS] = pairs;
    counts[dev::PD_READS_BEFORE] = counts[dev::PD_READS_KEPT] = n;
    counts[dev::PD_BASES_BEFORE] = counts[dev::PD_BASES_KEPT] = res.bases_before;
    if (n == 0 || pairs == 0) {
        pair_.release_record();
        return res;
    }
    // ---- selection (device scratch of this call) ----
    DeviceBuffer<uint64_t> d_rkey, d_ukey;
    DeviceBuffer<uint32_t> d_copies, d_err;
    DeviceBuffer<uint8_t> d_keep;
    DeviceBuffer<dev::DedupLoc> d_loc;
    DeviceBuffer<unsigned long long> d_count;
    PairDedupScratch scratch;
    dev::PairDedupArgs args {};
    d_rkey.alloc(n); d_ukey.alloc(pairs); d_copies.alloc(pairs); d_err.alloc(4); d_keep.alloc(pairs); d_loc.alloc(n); d_count.alloc(1);
    scratch.alloc(n, pairs, args);
    HIPCHK(hipMemsetAsync(d_rkey.data(), 0, d_rkey.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_loc.data(), 0, d_loc.bytes(), stream_));
    HIPCHK(hipMemsetAsync(d_err.data(), 0, d_err.bytes(), stream_));
    std::vector<DedupBlock> blocks(resident_.kept.size()); // (the exact check reads every block: the scratch of all of them lives until it is done)
    for (size_t b = 0; b < resident_.kept.size(); ++b) {
        if (!resident_.kept[b].n_reads || !resident_.kept[b].n_bases) continue;
        if (resident_.first[b] + resident_.kept[b].n_reads > n) throw Error(DRPRG_EIO, "duplicate pairs: the resident blocks hold more reads than the sample");
        dedup_block(resident_.kept[b], blocks[b], d_count.data());
        HIPCHK(dev::launch_dedup_keys(blocks[b].batch, reinterpret_cast<unsigned long long*>(d_rkey.data()) + resident_.first[b], d_err.data(), stream_));
        HIPCHK(dev::launch_dedup_loc(blocks[b].batch, resident_.first[b], n, d_loc.data(), d_err.data(), stream_));
    }
    args.n = n; args.n1 = n1; args.pairs = pairs; args.key_bits = key_bits; args.loc = d_loc.data();
    args.rkey = reinterpret_cast<const unsigned long long*>(d_rkey.data()); args.srcno = pair_.d_srcno.data(); args.mate = pair_.d_mate.data();
    args.ukey = d_ukey.data(); args.copies = d_copies.data(); args.keep = d_keep.data(); args.err = d_err.data();
    HIPCHK(dev::launch_pair_dedup(args, stream_));
    uint32_t err = 0, kept = 0;
    unsigned long long got[dev::PD_WORDS];
    HIPCHK(hipMemcpyAsync(&err, d_err.data(), sizeof err, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(&kept, args.rank + n, sizeof kept, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(got, args.out, sizeof got, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    if (err) throw Error(DRPRG_EIO, "duplicate pairs: a resident block's offsets do not fit its bases, or the pairing does not fit the sample");
    counts[dev::PD_WITH_BASES] = got[dev::PD_WITH_BASES];
    counts[dev::PD_BOTH] = got[dev::PD_BOTH];
    counts[dev::PD_DROPPED] = got[dev::PD_DROPPED];
    for (int i = 0; i < 32; ++i) levels[i] = got[dev::PD_LEVELS + i];
    if (kept != n) keep_flagged(args.flag, args.rank, args.boff, d_err.data() + 1, "duplicate pairs", res, flags); // (else no read dropped: nothing else happens)
    counts[dev::PD_READS_KEPT] = res.reads_kept;
    counts[dev::PD_BASES_KEPT] = res.bases_kept;
    pair_.release_record();
    return res;
}

void Mapper::dedup_pairs_device(const PairSide& a, const PairSide& b, uint64_t n_pairs, uint32_t key_bits, uint64_t* d_keys, uint8_t* d_keep, uint32_t* d_copies,
    uint64_t out[dev::PD_WORDS], hipStream_t stream)
{
    for (int i = 0; i < dev::PD_WORDS; ++i) out[i] = 0;
    if (key_bits < 1 || key_bits > 64) throw Error(DRPRG_EINVAL, "duplicate pairs: key_bits must be 1..64");
    if (n_pairs == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (!stream) stream = stream_;
    if (!a.d_offsets || !b.d_offsets || !d_keys || !d_keep || !d_copies || (a.n_bases && !a.d_words) || (b.n_bases && !b.d_words) || (a.n_npos && !a.d_npos) ||
        (b.n_npos && !b.d_npos))
        throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_pairs >= (1ull << 31)) throw Error(DRPRG_EOVERFLOW, "duplicate pairs: 2^32 reads or more in one call");
    const uint64_t n = 2 * n_pairs;
    const PairSide* side[2] = { &a, &b };
    DeviceBuffer<uint16_t> d_bits[2];
    DeviceBuffer<uint32_t> d_err, d_srcno, d_mate;
    DeviceBuffer<uint64_t> d_rkey;
    DeviceBuffer<dev::DedupLoc> d_loc;
    PairDedupScratch scratch;
    dev::PairDedupArgs args {};
    d_err.alloc(1); d_srcno.alloc(n); d_mate.alloc(n); d_rkey.alloc(n); d_loc.alloc(n);
    scratch.alloc(n, n_pairs, args);
    HIPCHK(hipMemsetAsync(d_err.data(), 0, d_err.bytes(), stream));
    HIPCHK(hipMemsetAsync(d_loc.data(), 0, d_loc.bytes(), stream));
    HIPCHK(hipMemsetAsync(d_rkey.data(), 0, d_rkey.bytes(), stream));
    for (int s = 0; s < 2; ++s) {
        const PairSide& p = *side[s];
        const uint64_t n_words = (p.n_bases + 15) / 16;
        if (p.n_npos) {
            d_bits[s].alloc(n_words + 8);
            HIPCHK(hipMemsetAsync(d_bits[s].data(), 0, d_bits[s].bytes(), stream));
            HIPCHK(dev::launch_mark_npos(p.d_npos, p.n_npos, p.n_bases, d_bits[s].data(), stream));
        }
        const dev::DedupBatch batch { p.d_words, p.n_npos ? d_bits[s].data() : nullptr, p.d_offsets, n_pairs, p.n_bases };
        HIPCHK(dev::launch_dedup_keys(batch, reinterpret_cast<unsigned long long*>(d_rkey.data()) + s * n_pairs, d_err.data(), stream));
        HIPCHK(dev::launch_dedup_loc(batch, s * n_pairs, n, d_loc.data(), d_err.data(), stream));
        // every read has the source number of its place, and its mate is the read at that place of the other side
        HIPCHK(dev::launch_pair_numbers(nullptr, nullptr, n_pairs, ~0ull, 0, n_pairs, d_srcno.data() + s * n_pairs, d_err.data(), stream));
        HIPCHK(dev::launch_pair_numbers(nullptr, nullptr, n_pairs, ~0ull, (uint32_t)((1 - s) * n_pairs), n_pairs, d_mate.data() + s * n_pairs, d_err.data(), stream));
    }
    args.n = n; args.n1 = n_pairs; args.pairs = n_pairs; args.key_bits = key_bits; args.loc = d_loc.data();
    args.rkey = reinterpret_cast<const unsigned long long*>(d_rkey.data()); args.srcno = d_srcno.data(); args.mate = d_mate.data();
    args.ukey = d_keys; args.copies = d_copies; args.keep = d_keep; args.err = d_err.data();
    HIPCHK(dev::launch_pair_dedup(args, stream));
    uint32_t err = 0, kept = 0;
    uint64_t bases[2] = { 0, 0 };
    unsigned long long got[dev::PD_WORDS];
    HIPCHK(hipMemcpyAsync(&err, d_err.data(), sizeof err, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&kept, args.rank + n, sizeof kept, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&bases[1], args.boff + n, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(got, args.out, sizeof got, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (err) throw Error(DRPRG_EINVAL, "duplicate pairs: the offsets of a side do not ascend from 0 to its n_bases");
    bases[0] = a.n_bases + b.n_bases;
    for (int i = 0; i < dev::PD_WORDS; ++i) out[i] = got[i];
    out[dev::PD_UNITS] = n_pairs;
    out[dev::PD_READS_BEFORE] = n;
    out[dev::PD_BASES_BEFORE] = bases[0];
    out[dev::PD_READS_KEPT] = kept;
    out[dev::PD_BASES_KEPT] = bases[1];
}

void Mapper::select_reads_with_anchors(std::vector<uint64_t> anchors, uint32_t A, std::vector<uint8_t>& bases, std::vector<uint64_t>& offsets,
    std::vector<uint64_t>* ids, uint64_t window_bytes)
{
    if (!kept_complete()) throw Error(DRPRG_ENODATA, "not every read of the sample is resident");
    if (A == 0 || A > 31) throw Error(DRPRG_EINVAL, "anchor length must be 1..31");
    if (offsets.empty()) offsets.push_back(0);
    std::sort(anchors.begin(), anchors.end());
    anchors.erase(std::unique(anchors.begin(), anchors.end()), anchors.end());
    if (anchors.empty() || resident_.kept.empty()) return;
    sync();
    HIPCHK(hipSetDevice(device_));
    std::vector<uint32_t> pf(2048, 0);
    for (uint64_t a : anchors) pf[(a & 0xFFFF) >> 5] |= 1u << (a & 31);
    uint64_t total_reads = 0, max_reads = 0;
    for (const DeviceBatch& b : resident_.kept) {
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
    for (size_t b = 0; b < resident_.kept.size();) {
        size_t e = b;
        uint64_t need = 0;
        do need += expanded(resident_.kept[e++]);
        while (e < resident_.kept.size() && need + expanded(resident_.kept[e]) <= WINDOW_BYTES);
        windows.emplace_back(b, e);
        scratch_need = std::max(scratch_need, need);
        b = e;
    }
    if (scratch_need) d_ascii.alloc(scratch_need);
    std::vector<const uint8_t*> ascii(resident_.kept.size(), nullptr);
    unsigned long long done = 0; // entries of d_list the windows before this one left
    for (const auto& win : windows) {
        uint64_t at = 0;
        for (size_t b = win.first; b < win.second; ++b) {
            const DeviceBatch& kb = resident_.kept[b];
            if (!kb.packed) {
                ascii[b] = kb.d_bases;
                continue;
            }
            HIPCHK(dev::launch_unpack(reinterpret_cast<const uint32_t*>(kb.d_bases), kb.n_bases, kb.d_npos, kb.n_npos, d_ascii.data() + at, stream_));
            ascii[b] = d_ascii.data() + at;
            at += expanded(kb);
        }
        for (size_t b = win.first; b < win.second; ++b) {
            const DeviceBatch& kb = resident_.kept[b];
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

} // namespace drprg
