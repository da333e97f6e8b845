// read_prep.cpp -- what happens to a host block before it is mapped: staging sets and the copies into them, the read filter, read
// trimming, adapter trimming, poly tails, base masking, the low-complexity filter and the decoy screen with their drivers, and the packers of the harness path.  See mapper.h.
#include "mapper.h"
#include <algorithm>
#include <hip/hip_runtime.h>

namespace drprg {

void Mapper::ensure_stage(Stage& st, uint64_t payload_bytes, uint64_t n_reads, uint64_t n_npos)
{
    grow(st.d_bases, payload_bytes + 64, payload_bytes + payload_bytes / 4 + 64);
    grow(st.d_offsets, n_reads + 1, n_reads + n_reads / 4 + 1);
    grow(st.d_npos, n_npos, n_npos + n_npos / 4 + 16);
}

Mapper::DeviceBatch Mapper::copy_in(const HostBatch& hb, uint8_t* d_bases, uint64_t* d_offsets, uint64_t* d_npos, hipStream_t stream)
{
    const uint64_t n_npos = hb.packed ? hb.n_npos : 0;
    const DeviceBatch b { d_bases, d_offsets, hb.n_reads, hb.n_bases(), hb.packed, n_npos ? d_npos : nullptr, n_npos };
    HIPCHK(hipMemcpyAsync(d_bases, hb.bases, hb.payload_bytes(), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_offsets, hb.offsets, (hb.n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    if (b.n_npos) HIPCHK(hipMemcpyAsync(d_npos, hb.npos, b.n_npos * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    return b;
}

void Mapper::ensure_bam_scratch(BamScratch& s, uint64_t n_bases)
{
    const uint64_t n = (uint64_t)dev::bam_pack_chunks(n_bases) + 1;
    const size_t temp = dev::scan_temp_bytes((uint32_t)n);
    grow(s.d_count, n);
    grow(s.d_prefix, n);
    grow(s.d_temp, temp);
}

Mapper::DeviceBatch Mapper::copy_in_bam(const HostBatch& hb, Stage& st, uint8_t* d_words, uint64_t* d_offsets, uint64_t* d_npos, hipStream_t copy_stream,
    hipStream_t stream)
{
    if (!hb.seq_start || (hb.seq_bytes && !hb.bases)) throw Error(DRPRG_EINVAL, "null buffer");
    grow(st.d_seq, hb.seq_bytes + 16, hb.seq_bytes + hb.seq_bytes / 4 + 16);
    grow(st.d_seq_start, hb.n_reads);
    grow(st.d_reverse, hb.n_reads);
    ensure_bam_scratch(st.bam, hb.n_bases());
    // (n_npos: counted by the parser thread that copied the fields: no read-back, no wait)
    const DeviceBatch b { d_words, d_offsets, hb.n_reads, hb.n_bases(), true, hb.n_npos ? d_npos : nullptr, hb.n_npos };
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
    const DeviceBatch b = copy_to_stage(hb, stage_sync_, stream_, stream_);
    if (hb.stats_which) // (no prep setting: the block is counted where it lies, in front of the map)
        count_unfiltered(hb, b, hb.stats_mode == 1 ? stats_qual_in(hb, stream_) : nullptr, hb.bam && hb.reverse ? stage_sync_.d_reverse.data() : nullptr, stream_);
    map(b, nullptr, nullptr, stream_, false);
    HIPCHK(hipStreamSynchronize(stream_)); // the staging buffers are reused by the next call
}

Mapper::DeviceBatch Mapper::copy_block_in(const HostBatch& hb, Stage* st, uint8_t* d_bases, uint64_t* d_offsets, uint64_t* d_npos, hipStream_t copy_stream,
    hipStream_t stream)
{
    return hb.bam ? copy_in_bam(hb, *st, d_bases, d_offsets, d_npos, copy_stream, stream) : copy_in(hb, d_bases, d_offsets, d_npos, copy_stream);
}

Mapper::DeviceBatch Mapper::copy_to_stage(const HostBatch& hb, Stage& st, hipStream_t copy_stream, hipStream_t stream)
{
    ensure_stage(st, hb.payload_bytes(), hb.n_reads, hb.packed || hb.bam ? hb.n_npos : 0);
    return copy_block_in(hb, &st, st.d_bases.data(), st.d_offsets.data(), st.d_npos.data(), copy_stream, stream);
}

hipStream_t Mapper::copy_stream()
{
    if (!copy_stream_) copy_stream_.create();
    return copy_stream_;
}

Mapper::Stage& Mapper::next_stage()
{
    Stage& st = stage_[stage_next_];
    stage_next_ ^= 1;
    if (!st.copied) st.copied.create(false);
    return st;
}

void Mapper::count_unmapped(uint64_t n, bool keeping)
{
    tot_reads_ += n;
    if (keeping) resident_.count_empty(n);
}

void Mapper::only_empty_reads(uint64_t n_reads, const ReadFilter& f, bool keeping, FilterOutcome& o)
{
    o.dropped_short = f.min_len ? n_reads : 0;
    o.reads_kept = o.mapped_reads = n_reads - o.dropped_short;
    if (f.poly()) o.poly.reads_seen = n_reads; // (no base: no tail)
    if (f.mask_qual) o.mask.reads_seen = n_reads; // (no base: nothing to mask)
    if (f.min_complexity) o.cplx.reads_judged = o.reads_kept; // (no pair: the threshold keeps them)
    if (f.decoy()) o.decoy.reads_judged = o.reads_kept; // (no window, no hit: the screen keeps them)
    count_unmapped(o.reads_kept, keeping);
}

hipStream_t Mapper::device_entry(hipStream_t stream, bool null_pointer, uint64_t n_reads)
{
    HIPCHK(hipSetDevice(device_));
    if (null_pointer) throw Error(DRPRG_EINVAL, "null device pointer");
    if (n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
    return stream ? stream : static_cast<hipStream_t>(stream_);
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
    if (n_bases == 0) return 0;
    if (n_reads == 0) throw Error(DRPRG_EINVAL, "bases without reads");
    stream = device_entry(stream, !d_seq || !d_seq_start || !d_offsets || !d_words, n_reads);
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

void Mapper::map_host_async(const HostBatch& hb)
{
    const uint64_t n_reads = hb.n_reads;
    if (n_reads == 0) return;
    const bool keeping = resident_.active();
    if (!keeping && !use_filter_) return map_host(hb); // no deferred form of this sequence
    HIPCHK(hipSetDevice(device_));
    if (hb.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
    if (hb.n_bases() == 0) { // only empty reads: nothing to copy, nothing to keep, nothing to map (the counters still see them)
        count_unmapped(n_reads, keeping);
        for (int w = 0; w < 2; ++w)
            if (hb.stats_which >> w & 1) stats_.empty_reads[w] += n_reads;
        if (pair_.record) pair_.seen[pair_.side] += n_reads; // (mate overlap: numbered, though they lie in no block)
        return;
    }
    // under keep_reads the block goes into device memory of its own and stays there; else into a staging set
    std::optional<BlockRoom> own;
    if (keeping && !(own = resident_.take_block(hb.payload_bytes(), n_reads, hb.packed || hb.bam ? hb.n_npos : 0))) {
        stop_keeping();
        return map_host_async(hb); // (as any block of a context that keeps nothing)
    }
    const hipStream_t cs = copy_stream();
    Stage* st = own && !hb.bam ? nullptr : &next_stage(); // (a BAM block is kept in the packed form: its raw fields go through a staging set)
    if (own && !kept_copied_) kept_copied_.create(false);
    const hipEvent_t copied = own ? kept_copied_ : st->copied;
    const DeviceBatch b = own ? copy_block_in(hb, st, own->bases, own->offsets, own->npos, cs, stream_) : copy_to_stage(hb, *st, cs, stream_);
    const uint8_t* const d_stats_qual = hb.stats_which && hb.stats_mode == 1 ? stats_qual_in(hb, cs) : nullptr; // (beside the block, in front of `copied`)
    HIPCHK(hipEventRecord(copied, cs));
    HIPCHK(hipStreamWaitEvent(stream_, copied, 0));
    if (hb.stats_which) count_unfiltered(hb, b, d_stats_qual, hb.bam && hb.reverse ? st->d_reverse.data() : nullptr, stream_); // (no wait: queued in front of the map)
    if (own) {
        if (pair_.record) { // mate overlap: a whole block is numbered on from its side's running count
            if (!pair_number_block(n_reads, nullptr, nullptr, n_reads, ~0ull, pair_.seen[pair_.side], stream_))
                throw Error(DRPRG_ENOMEM, "mate overlap: no room in the resident set for a block's source numbers (DRPRG_HIP_KEEP_READS_GB raises the limit)");
            pair_.seen[pair_.side] += n_reads;
        }
        resident_.add(b, n_reads);
        map_resident_block(b);
    } else map(b, nullptr, nullptr, stream_, true);
    HIPCHK(hipEventSynchronize(copied)); // the caller's block is free again; the kernels run on
}

// ---- the read filter ---------------------------------------------------------------------------------------------------------------
void Mapper::ensure_filter_scratch(FilterScratch& fs, uint64_t n_reads, uint64_t qual_bytes, bool own_flags, bool own_sums)
{
    if (qual_bytes) grow(fs.d_qual, qual_bytes + 64);
    if (own_flags) grow(fs.d_flag, n_reads);
    if (own_sums) grow(fs.d_qsum, n_reads);
    grow(fs.d_flag32, n_reads + 1);
    grow(fs.d_rank, n_reads + 1);
    grow(fs.d_klen, n_reads + 1);
    grow(fs.d_boff, n_reads + 1);
    grow(fs.d_temp, dev::read_filter_temp_bytes(n_reads));
    if (!fs.d_work) fs.d_work.alloc(dev::RF_WORDS);
    if (!fs.h_out) fs.h_out.alloc(dev::RF_WORDS);
}

void Mapper::run_read_filter(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, uint64_t n_reads,
    uint64_t n_bases, unsigned long long* d_sums, uint8_t* d_flags, hipStream_t stream, bool decoy, bool complexity)
{
    dev::ReadFilterArgs a {};
    if (complexity) {
        a.cplx_diff = fs.x_diff.data(); a.cplx_percent = f.min_complexity;
    }
    if (decoy) {
        a.decoy_valid = fs.k_counts.data(); a.decoy_hits = fs.k_counts.data() + n_reads;
        a.decoy_frac_milli = f.decoy_frac_milli; a.decoy_min_kmers = f.decoy_min_kmers;
    }
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
    stream = device_entry(stream, !d_offsets || !d_flags || (f.use_qual() && n_bases && !d_qual), n_reads);
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
    if (use_qual) {
        grow(fs.t_first, n_reads);
        grow(fs.t_last, n_reads);
    }
    if (own_ranges) {
        grow(fs.t_begin, n_reads);
        grow(fs.t_end, n_reads);
    }
    grow(fs.t_klen, n_reads + 1);
    grow(fs.t_offsets, n_reads + 1);
    grow(fs.t_temp, dev::read_trim_temp_bytes(n_reads));
    if (n_npos) {
        const uint64_t chunks = (uint64_t)dev::read_trim_npos_chunks(n_npos) + 1;
        grow(fs.t_count, chunks);
        grow(fs.t_prefix, chunks);
        grow(fs.t_ntemp, dev::scan_temp_bytes((uint32_t)chunks));
    }
    if (adapters) {
        grow(fs.t_cut, n_reads);
        if (bitmap_bases) grow(fs.t_nbits, (bitmap_bases + 15) / 16 + 8); // (launch_mark_npos writes 32-bit words)
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
    if (pts && f.trim_points()) a.pts = *pts;
    if (pts && f.any_adapters()) {
        if (indels) edit = dev::AdapterEditSets { f.adapters, f.front_adapters, f.eq3, f.eq5 };
        else a.ad = f.adapters;
    }
    if (pts && f.poly()) { a.poly_letters = f.poly_letters; a.poly_min_len = f.poly_min_len; }
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
    stream = device_entry(stream, !d_offsets || !d_begin || !d_end || (f.trim_qual_milli && n_bases && !d_qual), n_reads);
    FilterScratch& fs = filter_api_;
    ensure_trim_scratch(fs, n_reads, 0, f.trim_qual_milli != 0, false);
    run_read_trim(fs, f, d_qual, bias, d_offsets, d_rev, n_reads, n_bases, d_begin, d_end, nullptr, 0, stream);
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < 9; ++i) res[i] = fs.t_out[i];
}

void Mapper::adapter_trim_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos,
    const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t* d_begin, uint64_t* d_end, uint64_t res[11], hipStream_t stream)
{
    for (int i = 0; i < 11; ++i) res[i] = 0;
    if (n_reads == 0) return;
    if (!f.any_adapters()) throw Error(DRPRG_EINVAL, "adapter trimming: no adapter is set (drprg_hip_set_adapters, drprg_hip_set_adapters2)");
    stream = device_entry(stream, !d_offsets || !d_begin || !d_end || (n_bases && !d_text && !d_words) || (n_npos && !d_npos), n_reads);
    FilterScratch& fs = filter_api_;
    ensure_trim_scratch(fs, n_reads, 0, false, false, true, d_words && n_npos ? n_bases : 0);
    dev::AdapterPoints p = adapter_points(fs, d_words ? reinterpret_cast<const uint8_t*>(d_words) : d_text, d_words != nullptr, d_npos, n_npos, n_bases, stream);
    p.offsets = d_offsets; p.begin = d_begin; p.end = d_end; p.n_reads = n_reads; p.n_bases = n_bases;
    HIPCHK(hipMemsetAsync(fs.t_work.data(), 0, dev::RT_WORDS * sizeof(unsigned long long), stream));
    if (f.adapter_indels)
        HIPCHK(dev::launch_adapter_edit(p, f.adapters, f.eq3, f.front_adapters, f.eq5, d_begin, d_end, nullptr, fs.t_work.data(), stream));
    else HIPCHK(dev::launch_adapter_trim(p, f.adapters, d_end, nullptr, fs.t_work.data(), stream));
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

// ---- poly tails ----------------------------------------------------------------------------------------------------------------------
void Mapper::poly_trim_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
    uint64_t n_reads, uint64_t n_bases, const uint64_t* d_begin, uint64_t* d_end, uint64_t res[6], hipStream_t stream)
{
    for (int i = 0; i < 6; ++i) res[i] = 0;
    if (!f.poly()) throw Error(DRPRG_EINVAL, "poly-tail trimming: no letter is set (drprg_hip_set_poly_trim)");
    if (n_reads == 0) return;
    stream = device_entry(stream, !d_offsets || !d_begin || !d_end || (n_bases && !d_text && !d_words) || (n_npos && !d_npos), n_reads);
    FilterScratch& fs = filter_api_;
    ensure_trim_scratch(fs, n_reads, 0, false, false, true, d_words && n_npos ? n_bases : 0);
    dev::AdapterPoints p = adapter_points(fs, d_words ? reinterpret_cast<const uint8_t*>(d_words) : d_text, d_words != nullptr, d_npos, n_npos, n_bases, stream);
    p.offsets = d_offsets; p.begin = d_begin; p.end = d_end; p.n_reads = n_reads; p.n_bases = n_bases;
    HIPCHK(hipMemsetAsync(fs.t_work.data(), 0, dev::RT_WORDS * sizeof(unsigned long long), stream));
    HIPCHK(dev::launch_poly_tail(p, f.poly_letters, f.poly_min_len, d_end, nullptr, fs.t_work.data(), stream));
    HIPCHK(hipMemcpyAsync(fs.t_out.data(), fs.t_work.data(), dev::RT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    res[0] = n_reads;
    for (int i = 0; i < 4; ++i) res[1 + i] = fs.t_out[dev::RT_PT_BASES_SEEN + i];
    res[5] = fs.t_out[dev::RT_OFFSETS];
}

// ---- the low-complexity filter -------------------------------------------------------------------------------------------------------
bool Mapper::run_read_complexity(FilterScratch& fs, const uint8_t* d_bases, bool packed, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
    uint64_t n_reads, uint64_t n_bases, hipStream_t stream, bool nbits_ready)
{
    if (n_bases >= dev::CX_MAX_READ) // (a read is no longer than its block: D is a 32-bit word)
        throw Error(DRPRG_EOVERFLOW, "read complexity: a block of 2^32 bases or more; the pairs of a read are counted in a 32-bit word");
    grow(fs.x_diff, n_reads);
    dev::ComplexityArgs a { packed ? nullptr : d_bases, packed ? reinterpret_cast<const uint32_t*>(d_bases) : nullptr, nullptr, d_offsets, n_reads, n_bases,
        fs.x_diff.data() };
    if (packed && !nbits_ready && n_npos) { // the position list as a bitmap, as adapter_points makes it
        const uint64_t n16 = (n_bases + 15) / 16 + 8;
        grow(fs.t_nbits, n16);
        HIPCHK(hipMemsetAsync(fs.t_nbits.data(), 0, n16 * sizeof(uint16_t), stream));
        HIPCHK(dev::launch_mark_npos(d_npos, n_npos, n_bases, fs.t_nbits.data(), stream));
        nbits_ready = true;
    }
    if (packed && nbits_ready) a.nbits = fs.t_nbits.data();
    HIPCHK(dev::launch_read_diff(a, stream));
    return packed && nbits_ready;
}

void Mapper::complexity_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
    uint64_t n_reads, uint64_t n_bases, uint32_t* d_diff, uint8_t* d_flags, uint64_t res[3], hipStream_t stream)
{
    for (int i = 0; i < 3; ++i) res[i] = 0;
    if (!f.min_complexity) throw Error(DRPRG_EINVAL, "read complexity: no threshold is set (drprg_hip_set_min_complexity)");
    if (n_reads == 0) return;
    stream = device_entry(stream, !d_offsets || !d_flags || (n_bases && !d_text && !d_words) || (n_npos && !d_npos), n_reads);
    FilterScratch& fs = filter_api_;
    run_read_complexity(fs, d_words ? reinterpret_cast<const uint8_t*>(d_words) : d_text, d_words != nullptr, d_npos, n_npos, d_offsets, n_reads, n_bases, stream);
    if (!fs.x_work) fs.x_work.alloc(3);
    if (!fs.x_out) fs.x_out.alloc(3);
    const dev::ComplexityArgs a { d_text, d_words, nullptr, d_offsets, n_reads, n_bases, fs.x_diff.data() };
    HIPCHK(hipMemsetAsync(fs.x_work.data(), 0, 3 * sizeof(unsigned long long), stream));
    HIPCHK(dev::launch_complexity_verdict(a, f.min_complexity, d_flags, fs.x_work.data(), reinterpret_cast<uint32_t*>(fs.x_work.data() + 2), stream));
    HIPCHK(hipMemcpyAsync(fs.x_out.data(), fs.x_work.data(), 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    if (d_diff) HIPCHK(hipMemcpyAsync(d_diff, fs.x_diff.data(), n_reads * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < 3; ++i) res[i] = fs.x_out[i];
}

// ---- the decoy screen ----------------------------------------------------------------------------------------------------------------
void Mapper::set_decoy(const std::vector<uint8_t>& text, uint64_t windows, uint32_t k, uint64_t set)
{
    HIPCHK(hipSetDevice(device_));
    sync();
    clear_decoy();
    if (text.empty() || windows == 0) throw Error(DRPRG_EINVAL, "decoy screen: the decoy files hold no k-mer");
    uint64_t n_slots = dev::DC_MIN_SLOTS;
    while (n_slots < 2 * windows) n_slots <<= 1;
    DeviceBuffer<uint8_t> d_text;
    DeviceBuffer<unsigned long long> d_distinct;
    d_text.alloc(text.size() + 64);
    d_distinct.alloc(1);
    DecoyTable t;
    t.table.alloc(n_slots);
    HIPCHK(hipMemcpyAsync(d_text.data(), text.data(), text.size(), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemsetAsync(d_text.data() + text.size(), 0, 64, stream_));
    HIPCHK(dev::launch_decoy_build(d_text.data(), text.size(), k, t.table.data(), n_slots, d_distinct.data(), stream_));
    unsigned long long distinct = 0;
    HIPCHK(hipMemcpyAsync(&distinct, d_distinct.data(), sizeof distinct, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    if (distinct == 0) throw Error(DRPRG_EINVAL, "decoy screen: the decoy files hold no k-mer (no window of " + std::to_string(k) + " letters ACGT)");
    t.distinct = distinct; t.id = set; t.k = k;
    decoy_ = std::move(t);
}

void Mapper::clear_decoy()
{
    if (!decoy_.table) return;
    sync(); // (nothing in flight reads the table: the screen runs on the copy stream and is waited for with the filter's read-back)
    decoy_ = DecoyTable {};
}

dev::DecoySet Mapper::decoy_set(const ReadFilter& f) const
{
    if (!f.decoy() || !decoy_.table || decoy_.id != f.decoy_id || decoy_.k != f.decoy_k)
        throw Error(DRPRG_EINVAL, "decoy screen: no decoy set is loaded (drprg_hip_set_decoy)");
    return dev::DecoySet { decoy_.table.data(), decoy_.table.size(), f.decoy_k, f.decoy_frac_milli, f.decoy_min_kmers };
}

void Mapper::decoy_lookup(const std::vector<uint64_t>& kmers, uint8_t* found)
{
    HIPCHK(hipSetDevice(device_));
    if (!decoy_.table) throw Error(DRPRG_EINVAL, "decoy screen: no decoy set is loaded (drprg_hip_set_decoy)");
    if (kmers.empty()) return;
    DeviceBuffer<unsigned long long> d_kmers;
    DeviceBuffer<uint8_t> d_found;
    d_kmers.alloc(kmers.size());
    d_found.alloc(kmers.size());
    const dev::DecoySet d { decoy_.table.data(), decoy_.table.size(), decoy_.k, 1, 1 };
    HIPCHK(hipMemcpyAsync(d_kmers.data(), kmers.data(), kmers.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream_));
    HIPCHK(dev::launch_decoy_lookup(d, d_kmers.data(), kmers.size(), d_found.data(), stream_));
    HIPCHK(hipMemcpyAsync(found, d_found.data(), kmers.size(), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
}

void Mapper::run_decoy_screen(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_bases, bool packed, const uint64_t* d_npos, uint64_t n_npos,
    const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, hipStream_t stream, bool nbits_ready)
{
    const dev::DecoySet d = decoy_set(f);
    grow(fs.k_counts, 2 * n_reads);
    dev::DecoyScreenArgs a { packed ? nullptr : d_bases, packed ? reinterpret_cast<const uint32_t*>(d_bases) : nullptr, nullptr, d_offsets, n_reads, n_bases,
        fs.k_counts.data(), fs.k_counts.data() + n_reads };
    if (packed && nbits_ready) a.nbits = fs.t_nbits.data();
    else if (packed && n_npos) { // the position list as a bitmap, as adapter_points makes it
        const uint64_t n16 = (n_bases + 15) / 16 + 8;
        grow(fs.t_nbits, n16);
        HIPCHK(hipMemsetAsync(fs.t_nbits.data(), 0, n16 * sizeof(uint16_t), stream));
        HIPCHK(dev::launch_mark_npos(d_npos, n_npos, n_bases, fs.t_nbits.data(), stream));
        a.nbits = fs.t_nbits.data();
    }
    HIPCHK(hipMemsetAsync(fs.k_counts.data(), 0, 2 * n_reads * sizeof(uint32_t), stream));
    HIPCHK(dev::launch_decoy_screen(a, d, stream));
}

void Mapper::decoy_screen_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
    uint64_t n_reads, uint64_t n_bases, uint32_t* d_valid, uint32_t* d_hits, uint8_t* d_flags, uint64_t res[5], hipStream_t stream)
{
    for (int i = 0; i < 5; ++i) res[i] = 0;
    const dev::DecoySet d = decoy_set(f);
    if (n_reads == 0) return;
    stream = device_entry(stream, !d_offsets || !d_flags || (n_bases && !d_text && !d_words) || (n_npos && !d_npos), n_reads);
    FilterScratch& fs = filter_api_;
    run_decoy_screen(fs, f, d_words ? reinterpret_cast<const uint8_t*>(d_words) : d_text, d_words != nullptr, d_npos, n_npos, d_offsets, n_reads, n_bases, stream);
    if (!fs.k_work) fs.k_work.alloc(5);
    if (!fs.k_out) fs.k_out.alloc(5);
    const dev::DecoyScreenArgs a { d_text, d_words, nullptr, d_offsets, n_reads, n_bases, fs.k_counts.data(), fs.k_counts.data() + n_reads };
    HIPCHK(hipMemsetAsync(fs.k_work.data(), 0, 5 * sizeof(unsigned long long), stream));
    HIPCHK(dev::launch_decoy_verdict(a, d, d_flags, fs.k_work.data(), reinterpret_cast<uint32_t*>(fs.k_work.data() + 4), stream));
    HIPCHK(hipMemcpyAsync(fs.k_out.data(), fs.k_work.data(), 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    if (d_valid) HIPCHK(hipMemcpyAsync(d_valid, fs.k_counts.data(), n_reads * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    if (d_hits) HIPCHK(hipMemcpyAsync(d_hits, fs.k_counts.data() + n_reads, n_reads * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < 5; ++i) res[i] = fs.k_out[i];
}

// ---- base masking --------------------------------------------------------------------------------------------------------------------
void Mapper::run_base_mask(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, const uint8_t* d_rev,
    uint64_t n_reads, uint64_t n_bases, uint8_t* d_bases, bool packed, const uint64_t* d_npos, uint64_t n_npos, hipStream_t stream)
{
    grow(fs.m_rflag, n_reads);
    if (!fs.m_work) fs.m_work.alloc(dev::BM_WORDS);
    if (!fs.m_out) fs.m_out.alloc(dev::BM_WORDS);
    dev::BaseMaskArgs a {};
    a.qual = d_qual; a.bias = bias; a.min_qual = f.mask_qual; a.offsets = d_offsets; a.rev = d_rev; a.n_reads = n_reads; a.n_bases = n_bases;
    a.read_flag = fs.m_rflag.data(); a.work = fs.m_work.data();
    if (packed) { // the position list as a bitmap, as adapter_points makes it: always, because the mask writes into it
        const uint64_t n16 = (n_bases + 15) / 16 + 8, chunks = (uint64_t)dev::base_mask_tiles(n_bases) + 1;
        grow(fs.t_nbits, n16);
        grow(fs.m_count, chunks);
        grow(fs.m_prefix, chunks);
        grow(fs.m_temp, dev::scan_temp_bytes((uint32_t)chunks));
        HIPCHK(hipMemsetAsync(fs.t_nbits.data(), 0, n16 * sizeof(uint16_t), stream));
        HIPCHK(dev::launch_mark_npos(d_npos, n_npos, n_bases, fs.t_nbits.data(), stream));
        a.words = reinterpret_cast<uint32_t*>(d_bases); a.nbits = fs.t_nbits.data(); a.chunk_count = fs.m_count.data();
    } else a.text = d_bases;
    HIPCHK(dev::launch_base_mask(a, stream));
    HIPCHK(hipMemcpyAsync(fs.m_out.data(), fs.m_work.data(), dev::BM_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
}

void Mapper::emit_mask_list(FilterScratch& fs, uint64_t n_bases, uint64_t n_list, hipStream_t stream)
{
    grow(fs.m_npos, n_list, n_list + n_list / 4 + 16);
    HIPCHK(dev::launch_base_mask_emit(fs.t_nbits.data(), n_bases, fs.m_count.data(), fs.m_prefix.data(), fs.m_temp.data(), fs.m_temp.size(), fs.m_npos.data(), n_list,
        stream));
}

void Mapper::base_mask_device(const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, const uint8_t* d_rev, uint64_t n_reads,
    uint64_t n_bases, uint8_t* d_text, uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, uint64_t* d_npos_out, uint64_t npos_cap, uint64_t res[8],
    hipStream_t stream)
{
    for (int i = 0; i < 8; ++i) res[i] = 0;
    if (!f.mask_qual) throw Error(DRPRG_EINVAL, "base masking: no quality is set (drprg_hip_set_base_mask)");
    if (n_reads == 0) return;
    stream = device_entry(stream, !d_offsets || (n_bases && (!d_qual || (!d_text && !d_words))) || (n_npos && !d_npos), n_reads);
    FilterScratch& fs = filter_api_;
    run_base_mask(fs, f, d_qual, bias, d_offsets, d_rev, n_reads, n_bases, d_words ? reinterpret_cast<uint8_t*>(d_words) : d_text, d_words != nullptr, d_npos, n_npos,
        stream);
    HIPCHK(hipStreamSynchronize(stream));
    const unsigned long long* h = fs.m_out.data();
    res[0] = n_reads; res[1] = n_bases; res[2] = h[dev::BM_READS_MASKED]; res[3] = h[dev::BM_BASES_MASKED]; res[4] = h[dev::BM_ALREADY];
    res[5] = d_words ? h[dev::BM_LISTED] : 0;
    res[6] = h[dev::BM_BAD_AT] == ~0ull ? 0 : h[dev::BM_BAD_AT];
    res[7] = h[dev::BM_OFFSETS];
    if (res[6] || res[7] || !res[5] || res[5] > npos_cap || !d_npos_out) return;
    HIPCHK(dev::launch_base_mask_emit(fs.t_nbits.data(), n_bases, fs.m_count.data(), fs.m_prefix.data(), fs.m_temp.data(), fs.m_temp.size(), d_npos_out, npos_cap, stream));
    HIPCHK(hipStreamSynchronize(stream));
}

// ---- read statistics -----------------------------------------------------------------------------------------------------------------
void Mapper::run_read_stats(StatsState& st, int which, const DeviceBatch& b, const uint8_t* d_qual, uint32_t bias, const uint8_t* d_rev, const uint8_t* d_flags,
    uint64_t take, hipStream_t stream)
{
    if (b.n_reads == 0) return;
    if (b.n_bases >= dev::RS_MAX_BASES) throw Error(DRPRG_EOVERFLOW, "read statistics: a block of 2^32 bases or more");
    if (st.last && st.last != stream) HIPCHK(hipStreamSynchronize(st.last)); // (the scratch below is shared: one stream at a time)
    st.last = stream;
    if (!st.acc[which]) {
        st.acc[which].alloc(dev::RS_DEV_WORDS);
        HIPCHK(dev::launch_read_stats_clear(st.acc[which].data(), stream));
    }
    grow(st.gcv, b.n_reads);
    if (d_qual) grow(st.esum, b.n_reads);
    dev::ReadStatsArgs a {};
    if (b.packed) {
        a.words = reinterpret_cast<const uint32_t*>(b.d_bases);
        if (b.n_npos) { // the position list as a bitmap, as adapter_points makes it
            const uint64_t n16 = (b.n_bases + 15) / 16 + 8;
            grow(st.nbits, n16);
            HIPCHK(hipMemsetAsync(st.nbits.data(), 0, n16 * sizeof(uint16_t), stream));
            HIPCHK(dev::launch_mark_npos(b.d_npos, b.n_npos, b.n_bases, st.nbits.data(), stream));
            a.nbits = st.nbits.data();
        }
    } else a.text = b.d_bases;
    a.qual = d_qual; a.bias = bias; a.offsets = b.d_offsets; a.rev = d_rev; a.flags = d_flags; a.n_reads = b.n_reads; a.n_bases = b.n_bases; a.take = take;
    a.gcv = st.gcv.data(); a.esum = st.esum.data(); a.acc = st.acc[which].data();
    HIPCHK(dev::launch_read_stats(a, stream));
}

const uint8_t* Mapper::stats_qual_in(const HostBatch& hb, hipStream_t stream)
{
    if (!hb.qual) throw Error(DRPRG_EINVAL, "--qc-json: the reads came without base qualities");
    DeviceBuffer<uint8_t>& q = stats_.qual[stats_.qual_next];
    stats_.qual_next ^= 1; // (two in turn: the block that used this one two calls ago is complete, as with the staging sets)
    const uint64_t n = hb.n_bases();
    grow(q, n + 64);
    HIPCHK(hipMemcpyAsync(q.data(), hb.qual, n, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(q.data() + n, 0, 64, stream));
    return q.data();
}

void Mapper::count_unfiltered(const HostBatch& hb, const DeviceBatch& b, const uint8_t* d_qual, const uint8_t* d_rev, hipStream_t stream)
{
    for (int w = 0; w < 2; ++w) {
        if (!(hb.stats_which >> w & 1)) continue;
        if (b.n_bases == 0) stats_.empty_reads[w] += b.n_reads;
        else run_read_stats(stats_, w, b, d_qual, hb.qual_bias, d_rev, nullptr, b.n_reads, stream);
    }
}

void Mapper::count_host_block(const HostBatch& hb)
{
    if (hb.n_reads == 0 || !hb.stats_which) return;
    sync();
    HIPCHK(hipSetDevice(device_));
    if (hb.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
    if (hb.n_bases() == 0) {
        for (int w = 0; w < 2; ++w)
            if (hb.stats_which >> w & 1) stats_.empty_reads[w] += hb.n_reads;
        return;
    }
    const DeviceBatch b = copy_to_stage(hb, stage_sync_, stream_, stream_);
    count_unfiltered(hb, b, hb.stats_mode == 1 ? stats_qual_in(hb, stream_) : nullptr, hb.bam && hb.reverse ? stage_sync_.d_reverse.data() : nullptr, stream_);
    HIPCHK(hipStreamSynchronize(stream_));
}

void Mapper::read_stats(int which, uint64_t out[dev::RS_WORDS])
{
    sync();
    HIPCHK(hipSetDevice(device_));
    for (uint32_t i = 0; i < dev::RS_WORDS; ++i) out[i] = 0;
    out[dev::RS_MIN_LEN] = ~0ull;
    if (stats_.acc[which]) {
        if (copy_stream_) HIPCHK(hipStreamSynchronize(copy_stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        HIPCHK(hipMemcpy(out, stats_.acc[which].data(), dev::RS_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (const uint64_t n = stats_.empty_reads[which]) { // reads of blocks that held no base
        out[dev::RS_READS] += n;
        out[dev::RS_LEN_READS] += n;
        out[dev::RS_MIN_LEN] = 0;
    }
}

void Mapper::check_read_stats()
{
    sync();
    HIPCHK(hipSetDevice(device_));
    if (copy_stream_) HIPCHK(hipStreamSynchronize(copy_stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    for (int w = 0; w < 2; ++w) {
        if (!stats_.acc[w]) continue;
        unsigned long long e[2] = { 0, 0 };
        HIPCHK(hipMemcpy(e, stats_.acc[w].data() + dev::RS_DEV_BAD_AT, sizeof e, hipMemcpyDeviceToHost));
        if (e[1]) throw Error(DRPRG_EINVAL, "read statistics: a block's offsets do not ascend to its number of bases");
        if (e[0] != ~0ull) throw Error(DRPRG_EFORMAT, "a base quality outside 0..93 (quality byte " + std::to_string(e[0] - 1) + " of an ingest block; FASTQ: bytes 33..126, BAM: bytes 0..93)");
    }
}

void Mapper::read_stats_device(const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint8_t* d_qual, uint32_t bias,
    const uint64_t* d_offsets, const uint8_t* d_rev, uint64_t n_reads, uint64_t n_bases, const uint8_t* d_flags, uint64_t take, uint64_t out[dev::RS_WORDS],
    uint64_t res[2], hipStream_t stream)
{
    for (uint32_t i = 0; i < dev::RS_WORDS; ++i) out[i] = 0;
    res[0] = res[1] = 0;
    if (n_reads == 0) return;
    stream = device_entry(stream, !d_offsets || (n_bases && !d_text && !d_words) || (n_npos && !d_npos), n_reads);
    StatsState& st = stats_api_;
    if (!st.acc[0]) st.acc[0].alloc(dev::RS_DEV_WORDS);
    if (!st.h_err) st.h_err.alloc(dev::RS_DEV_WORDS);
    HIPCHK(dev::launch_read_stats_clear(st.acc[0].data(), stream));
    const DeviceBatch b { d_words ? reinterpret_cast<const uint8_t*>(d_words) : d_text, d_offsets, n_reads, n_bases, d_words != nullptr, d_npos, n_npos };
    run_read_stats(st, 0, b, d_qual, bias, d_rev, d_flags, take, stream);
    HIPCHK(hipMemcpyAsync(st.h_err.data(), st.acc[0].data(), dev::RS_DEV_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const unsigned long long* h = st.h_err.data();
    for (uint32_t i = 0; i < dev::RS_WORDS; ++i) out[i] = h[i];
    if (out[dev::RS_MIN_LEN] == ~0ull) out[dev::RS_MIN_LEN] = 0;
    res[0] = h[dev::RS_DEV_BAD_AT] == ~0ull ? 0 : h[dev::RS_DEV_BAD_AT];
    res[1] = h[dev::RS_DEV_OFFSETS];
}

// ---- a host block behind the filter: map_host_filtered and its steps ---------------------------------------------------------------------
// what the trim stage and the filter say alike about a quality byte out of range (at: the byte's index + 1)
static Error bad_quality_error(uint64_t at, uint64_t n_bases, uint32_t bias)
{
    return Error(DRPRG_EFORMAT, "a base quality outside 0..93 (quality byte " + std::to_string(at - 1) + " of an ingest block of " + std::to_string(n_bases)
            + " bases, " + (bias ? "FASTQ: bytes 33..126" : "BAM: bytes 0..93") + ")");
}

// The trim stage: the kept range of every read, the new offsets and the counts, one read-back; a block that lost a base is compacted by
// its ranges into the set's t_* buffers (launch_subsample_pack for words, launch_gather_reads for text and for the quality bytes) and
// `src` and the quality pointer are REPLACED: the filter, the depth cut, the compaction and keep_reads see a block of trimmed reads.
// trim_err receives that compaction's error word once the stream has been waited for again (with the filter's read-back).  false: every
// base of the block is gone.
bool Mapper::trim_block(const HostBatch& hb, const ReadFilter& f, Stage& st, DeviceBatch& src, const uint8_t*& d_qual, uint32_t& trim_err, FilterOutcome& o)
{
    FilterScratch& fs = st.filt;
    const hipStream_t cs = copy_stream_;
    const uint64_t n_reads = src.n_reads, n_bases = src.n_bases;
    const uint8_t* d_rev = hb.bam && hb.reverse ? st.d_reverse.data() : nullptr; // (BAM: QUAL stays in stored order; the bases were reversed by bam_pack_kernel)
    dev::AdapterPoints pts {}; // (adapters: sought in what the crops and the quality trim leave, bases in read orientation; a packed block's bitmap first)
    if (f.trim_points()) pts = adapter_points(fs, src.d_bases, src.packed, src.d_npos, src.n_npos, n_bases, cs); // (poly tails look at the same bases)
    run_read_trim(fs, f, d_qual, hb.qual_bias, src.d_offsets, d_rev, n_reads, n_bases, fs.t_begin.data(), fs.t_end.data(), src.d_npos, src.n_npos, cs, &pts);
    HIPCHK(hipStreamSynchronize(cs)); // the trim's read-back: the trimmed sizes are known before the filter is launched
    const unsigned long long* t = fs.t_out.data();
    if (t[dev::RT_BAD_AT] == ~0ull) throw Error(DRPRG_EINVAL, "read trimming: the block's offsets do not ascend to its number of bases");
    if (t[dev::RT_BAD_AT]) throw bad_quality_error(t[dev::RT_BAD_AT], n_bases, hb.qual_bias);
    if (f.crops())
        o.trim = TrimOutcome { n_reads, n_bases, t[dev::RT_LOST_READS], t[dev::RT_CUT_FRONT], t[dev::RT_CUT_TAIL], t[dev::RT_QCUT_FRONT], t[dev::RT_QCUT_TAIL],
            t[dev::RT_EMPTIED] };
    if (f.adapters.n)
        o.adapter = AdapterOutcome { n_reads, t[dev::RT_AD_BASES_SEEN], t[dev::RT_AD_READS_CUT], t[dev::RT_AD_BASES_CUT], t[dev::RT_AD_EMPTIED] };
    if (f.front_adapters.n)
        o.front = AdapterOutcome { n_reads, t[dev::RT_FA_BASES_SEEN], t[dev::RT_FA_READS_CUT], t[dev::RT_FA_BASES_CUT], t[dev::RT_FA_EMPTIED] };
    if (f.poly()) o.poly = PolyOutcome { n_reads, t[dev::RT_PT_BASES_SEEN], t[dev::RT_PT_READS_CUT], t[dev::RT_PT_BASES_CUT], t[dev::RT_PT_EMPTIED] };
    // (a read cut by a tail has lost a base like any other)
    if (!t[dev::RT_LOST_READS] && !t[dev::RT_AD_READS_CUT] && !t[dev::RT_FA_READS_CUT] && !t[dev::RT_PT_READS_CUT]) return true; // the block lost no base to any cause
    const uint64_t nb = t[dev::RT_KEPT_BASES], n_list = src.n_npos ? t[dev::RT_KEPT_NPOS] : 0;
    o.bases_seen = nb;
    if (nb == 0) return false;
    const uint64_t payload = src.packed ? (nb + 15) / 16 * 4 : nb;
    grow(fs.t_bases, payload + 64);
    if (n_list) grow(fs.t_npos, n_list);
    if (f.qual_behind_trim()) grow(fs.t_qual, nb + 64);
    if (src.packed) grow(fs.t_src, n_reads);
    if (!src.packed) grow(fs.t_btable, n_reads);
    if (f.qual_behind_trim()) grow(fs.t_qtable, n_reads);
    uint32_t* const d_err = reinterpret_cast<uint32_t*>(fs.t_work.data() + dev::RT_KEPT_NPOS); // (zeroed with the trim's words, unused on the device)
    dev::ReadTrimFill tf { src.d_offsets, d_rev, fs.t_begin.data(), fs.t_end.data(), fs.t_offsets.data(), n_reads, n_bases, nb, src.d_bases, d_qual,
        src.packed ? fs.t_src.data() : nullptr, src.packed ? nullptr : fs.t_btable.data(), f.qual_behind_trim() ? fs.t_qtable.data() : nullptr, d_err };
    HIPCHK(dev::launch_read_trim_fill(tf, cs));
    HIPCHK(hipMemsetAsync(fs.t_bases.data() + payload, 0, 64, cs));
    if (src.packed) { // (by ranges, not by flags: the one pack launch outside compact_block)
        const dev::SubsampleBlock sb { src.d_bases, src.d_offsets, n_reads, n_bases, 0, nullptr, nullptr, nullptr, n_reads, nb };
        HIPCHK(dev::launch_subsample_pack(sb, fs.t_offsets.data(), fs.t_src.data(), reinterpret_cast<uint32_t*>(fs.t_bases.data()), d_err, cs));
        if (n_list) {
            const dev::ReadTrimNpos np { src.d_npos, src.n_npos, fs.t_count.data(), fs.t_prefix.data(), fs.t_ntemp.data(), fs.t_ntemp.size() };
            HIPCHK(dev::launch_read_trim_npos_emit(tf, np, fs.t_npos.data(), n_list, cs));
        }
    } else HIPCHK(dev::launch_gather_reads(fs.t_btable.data(), (uint32_t)n_reads, fs.t_bases.data(), cs));
    if (f.qual_behind_trim()) { // (the filter's threshold, or the mask: either sees the trimmed reads' bytes, in stored order beside d_rev)
        HIPCHK(dev::launch_gather_reads(fs.t_qtable.data(), (uint32_t)n_reads, fs.t_qual.data(), cs));
        HIPCHK(hipMemsetAsync(fs.t_qual.data() + nb, 0, 64, cs));
        d_qual = fs.t_qual.data();
    }
    HIPCHK(hipMemcpyAsync(&trim_err, d_err, sizeof trim_err, hipMemcpyDeviceToHost, cs)); // (queued behind the compaction; waited for with the filter's read-back)
    src.d_bases = fs.t_bases.data();
    src.d_offsets = fs.t_offsets.data();
    src.n_bases = nb;
    src.d_npos = n_list ? fs.t_npos.data() : nullptr;
    src.n_npos = n_list;
    return true;
}

// The mask, queued in place on the block the trim stage left -- the staging copy or the trim stage's compacted copy, never the caller's
// memory.  No wait of its own: its eight words arrive with the filter's read-back.
void Mapper::mask_block(const HostBatch& hb, const ReadFilter& f, Stage& st, const DeviceBatch& src, const uint8_t* d_qual)
{
    const uint8_t* d_rev = hb.bam && hb.reverse ? st.d_reverse.data() : nullptr; // (as the trim stage: QUAL stays in stored order)
    run_base_mask(st.filt, f, d_qual, hb.qual_bias, src.d_offsets, d_rev, src.n_reads, src.n_bases, const_cast<uint8_t*>(src.d_bases), src.packed, src.d_npos, src.n_npos,
        copy_stream_);
}

void Mapper::mask_done(const HostBatch& hb, Stage& st, DeviceBatch& src, FilterOutcome& o)
{
    FilterScratch& fs = st.filt;
    const unsigned long long* h = fs.m_out.data();
    if (h[dev::BM_OFFSETS]) throw Error(DRPRG_EINVAL, "base masking: the block's offsets do not ascend to its number of bases");
    if (h[dev::BM_BAD_AT] != ~0ull) throw bad_quality_error(h[dev::BM_BAD_AT], src.n_bases, hb.qual_bias);
    o.mask = MaskOutcome { src.n_reads, src.n_bases, h[dev::BM_READS_MASKED], h[dev::BM_BASES_MASKED], h[dev::BM_ALREADY] };
    if (!src.packed || !h[dev::BM_BASES_MASKED]) return; // (text, or no position joined the list: a base that was unknown already is listed)
    emit_mask_list(fs, src.n_bases, h[dev::BM_LISTED], copy_stream_);
    // (queued behind the filter's wait: a block that is mapped where it lies meets no other wait, so the mapping stream is told)
    HIPCHK(hipEventRecord(st.copied, copy_stream_));
    HIPCHK(hipStreamWaitEvent(stream_, st.copied, 0));
    src.d_npos = fs.m_npos.data();
    src.n_npos = h[dev::BM_LISTED];
}

// The filter on the block as the trim stage left it, with its read-back: the caller's block is free again when this returns.
void Mapper::filter_block(const HostBatch& hb, const ReadFilter& f, FilterScratch& fs, const DeviceBatch& src, const uint8_t* d_qual, const uint32_t& trim_err,
    FilterOutcome& o)
{
    const hipStream_t cs = copy_stream_;
    // (the screen in front of the filter's scans, which then see one verdict: the block as the trim stage left it, whatever its form)
    // (behind the mask a packed block's bitmap is there already, and holds the masked positions, which the list does not yet)
    // (the pair count in front of both: the threshold judges the block as the mask left it, and its bitmap serves the screen too)
    bool nbits_ready = f.mask_qual != 0 && src.packed;
    if (f.min_complexity)
        nbits_ready = run_read_complexity(fs, src.d_bases, src.packed, src.d_npos, src.n_npos, src.d_offsets, src.n_reads, src.n_bases, cs, nbits_ready) || nbits_ready;
    if (f.decoy()) run_decoy_screen(fs, f, src.d_bases, src.packed, src.d_npos, src.n_npos, src.d_offsets, src.n_reads, src.n_bases, cs, nbits_ready);
    run_read_filter(fs, f, d_qual, hb.qual_bias, src.d_offsets, src.n_reads, src.n_bases, fs.d_qsum.data(), fs.d_flag.data(), cs, f.decoy(), f.min_complexity != 0);
    HIPCHK(hipStreamSynchronize(cs));
    if (trim_err) throw Error(DRPRG_EIO, "read trimming: the block's offsets and the trimmed ranges do not fit each other");
    const unsigned long long* h = fs.h_out.data();
    if (h[dev::RF_OFFSETS]) throw Error(DRPRG_EINVAL, "read filter: the block's offsets do not ascend to its number of bases");
    if (h[dev::RF_BAD_AT]) throw bad_quality_error(h[dev::RF_BAD_AT], src.n_bases, hb.qual_bias);
    o.dropped_short = h[dev::RF_SHORT];
    o.dropped_long = h[dev::RF_LONG];
    o.dropped_lowq = h[dev::RF_LOWQ];
    o.reads_kept = h[dev::RF_KEPT_READS];
    o.bases_kept = h[dev::RF_KEPT_BASES];
    if (f.min_complexity)
        o.cplx = ComplexityOutcome { h[dev::RF_CPLX_READS], h[dev::RF_CPLX_BASES], h[dev::RF_CPLX_DROPPED], h[dev::RF_CPLX_DROPPED_BASES] };
    if (f.decoy())
        o.decoy = DecoyOutcome { h[dev::RF_DECOY_READS], h[dev::RF_DECOY_BASES], h[dev::RF_DECOY_DROPPED], h[dev::RF_DECOY_DROPPED_BASES], h[dev::RF_DECOY_VALID],
            h[dev::RF_DECOY_HITS] };
}

// Which of the kept reads go on: all of them, or -- cap_need != 0 and reached in this block -- those up to the one that holds the
// cap_need-th kept base.
Mapper::KeptPart Mapper::cut_at_cap(FilterScratch& fs, uint64_t n_reads, uint64_t cap_need, FilterOutcome& o)
{
    KeptPart k { n_reads, o.reads_kept, o.bases_kept };
    if (!cap_need || k.n_bases < cap_need) return k;
    // the cut, in the block's own numbering: boff is the running total of the kept bases (covg_cut.hip on the scan instead of the offsets)
    const hipStream_t cs = copy_stream_;
    if (!h_cut_) h_cut_.alloc(4);
    HIPCHK(dev::launch_covg_cut(fs.d_boff.data(), n_reads, cap_need, nullptr, 0, h_cut_.device_ptr(), cs));
    HIPCHK(hipStreamSynchronize(cs));
    k.take = h_cut_[0];
    k.n_bases = h_cut_[1];
    uint32_t rk = 0;
    HIPCHK(hipMemcpyAsync(&rk, fs.d_rank.data() + k.take, sizeof rk, hipMemcpyDeviceToHost, cs));
    HIPCHK(hipStreamSynchronize(cs));
    o.cut = true;
    o.cut_dropped = k.n_reads - rk;
    k.n_reads = rk;
    return k;
}

// Where the block that goes on lies when it is mapped.  A block that lost reads is compacted by the filter's flags (compact_block): into
// the resident set under keep_reads, else into the stage's c_* buffers.  A block that lost none stays in the staging set, and under
// keep_reads is copied on the device to where it stays.  keeping: cleared when the resident set cannot take the block (stop_keeping).
Mapper::DeviceBatch Mapper::place_block(FilterScratch& fs, const DeviceBatch& src, const KeptPart& k, bool& keeping)
{
    const hipStream_t cs = copy_stream_;
    const uint64_t payload = src.packed ? (k.n_bases + 15) / 16 * 4 : k.n_bases;
    if (k.n_reads == src.n_reads) { // the whole block
        if (!keeping) return src;
        const std::optional<BlockRoom> dst = resident_.take_block(payload, k.n_reads, src.n_npos);
        if (!dst) {
            stop_keeping();
            keeping = false;
            return src;
        }
        HIPCHK(hipMemsetAsync(dst->bases + payload, 0, 64, cs));
        HIPCHK(hipMemcpyAsync(dst->bases, src.d_bases, payload, hipMemcpyDeviceToDevice, cs));
        HIPCHK(hipMemcpyAsync(dst->offsets, src.d_offsets, (k.n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, cs));
        if (src.n_npos) HIPCHK(hipMemcpyAsync(dst->npos, src.d_npos, src.n_npos * sizeof(uint64_t), hipMemcpyDeviceToDevice, cs));
        HIPCHK(hipStreamSynchronize(cs)); // (the block is whole before anything on the mapping stream reads it)
        return DeviceBatch { dst->bases, dst->offsets, k.n_reads, k.n_bases, src.packed, src.n_npos ? dst->npos : nullptr, src.n_npos };
    }
    const dev::SubsampleBlock sb { src.d_bases, src.d_offsets, k.take, src.n_bases, 0, fs.d_flag.data(), fs.d_rank.data(), fs.d_boff.data(), k.n_reads, k.n_bases };
    uint32_t* const d_err = reinterpret_cast<uint32_t*>(fs.d_work.data() + dev::RF_ERR); // (zeroed with the filter's words)
    const DeviceBatch cur = compact_block(sb, src, fs.comp, d_err, cs, [&](uint64_t n_list) {
        if (keeping) {
            if (const std::optional<BlockRoom> dst = resident_.take_block(payload, k.n_reads, n_list)) return *dst;
            stop_keeping();
            keeping = false;
        }
        grow(fs.c_bases, payload + 64, payload + payload / 4 + 64); // (the staging sets' padding rule: ensure_stage)
        grow(fs.c_offsets, k.n_reads + 1, k.n_reads + k.n_reads / 4 + 1);
        grow(fs.c_npos, n_list, n_list + n_list / 4 + 16);
        return BlockRoom { fs.c_bases.data(), fs.c_offsets.data(), fs.c_npos.data() };
    });
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, cs));
    HIPCHK(hipStreamSynchronize(cs));
    if (err) throw Error(DRPRG_EIO, "read filter: the block's offsets and the filter's scans do not fit each other");
    return cur;
}

void Mapper::map_host_filtered(const HostBatch& hb, const ReadFilter& f, uint64_t cap_need, FilterOutcome& o)
{
    o = FilterOutcome {};
    const uint64_t n_reads = hb.n_reads;
    if (n_reads == 0) return;
    HIPCHK(hipSetDevice(device_));
    if (hb.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
    const uint64_t n_bases = hb.n_bases();
    o.reads_seen = n_reads;
    o.bases_seen = n_bases;
    bool keeping = resident_.active();
    const uint64_t pair_base = pair_.seen[pair_.side]; // mate overlap: source numbers count the reads the file held, whatever the stages drop
    if (pair_.record) pair_.seen[pair_.side] += n_reads;
    if (n_bases == 0) { // (the counters still see them)
        only_empty_reads(n_reads, f, keeping, o);
        if (f.read_stats) {
            stats_.empty_reads[STATS_RAW] += n_reads;
            stats_.empty_reads[STATS_PREPARED] += o.reads_kept;
        }
        return;
    }
    if (f.trim_qual_milli && !hb.qual) throw Error(DRPRG_EINVAL, "--trim-qual: the reads came without base qualities");
    if (f.mask_qual && !hb.qual) throw Error(DRPRG_EINVAL, "--mask-qual: the reads came without base qualities");
    if (f.use_qual() && !hb.qual) throw Error(DRPRG_EINVAL, "--min-read-qual: the reads came without base qualities");
    if (f.read_stats == 1 && !hb.qual) throw Error(DRPRG_EINVAL, "--qc-json: the reads came without base qualities (--qc-no-qual reports without them)");
    if (n_reads > dev::MAX_BATCH_READS) throw Error(DRPRG_EOVERFLOW, "at most " + std::to_string(dev::MAX_BATCH_READS) + " reads per batch");
    // 1. copy in: the block into a staging set, its quality bytes beside it
    const hipStream_t cs = copy_stream();
    Stage& st = next_stage();
    FilterScratch& fs = st.filt;
    const uint64_t n_npos = hb.packed || hb.bam ? hb.n_npos : 0;
    ensure_filter_scratch(fs, n_reads, f.wants_qual() ? n_bases : 0, true, f.use_qual());
    if (f.trims()) ensure_trim_scratch(fs, n_reads, n_npos, f.trim_qual_milli != 0, true, f.trim_points(), n_npos ? n_bases : 0);
    DeviceBatch src = copy_to_stage(hb, st, cs, cs);
    if (f.wants_qual()) {
        HIPCHK(hipMemcpyAsync(fs.d_qual.data(), hb.qual, n_bases, hipMemcpyHostToDevice, cs));
        HIPCHK(hipMemsetAsync(fs.d_qual.data() + n_bases, 0, 64, cs));
    }
    const uint8_t* d_qual = fs.d_qual.data();
    uint32_t trim_err = 0;
    // the raw snapshot: the block as the file held it, queued in front of the trim stage; what it refuses arrives with the next read-back
    const uint8_t* const d_stats_rev = hb.bam && hb.reverse ? st.d_reverse.data() : nullptr;
    if (f.read_stats) {
        run_read_stats(stats_, STATS_RAW, src, f.read_stats == 1 ? d_qual : nullptr, hb.qual_bias, d_stats_rev, nullptr, n_reads, cs);
        if (!stats_.h_err) stats_.h_err.alloc(2);
        HIPCHK(hipMemcpyAsync(stats_.h_err.data(), stats_.acc[STATS_RAW].data() + dev::RS_DEV_BAD_AT, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, cs));
    }
    const auto raw_refusals = [&]() { // (behind a wait for the copy stream)
        if (!f.read_stats) return;
        if (stats_.h_err[1]) throw Error(DRPRG_EINVAL, "read statistics: the block's offsets do not ascend to its number of bases");
        if (stats_.h_err[0] != ~0ull) throw bad_quality_error(stats_.h_err[0], n_bases, hb.qual_bias);
    };
    // 2. trim, 3. mask, 4. filter, 5. the depth cap
    if (f.trims() && !trim_block(hb, f, st, src, d_qual, trim_err, o)) { // reads of no bases are left: nothing to map
        hand_back_stage();
        raw_refusals();
        only_empty_reads(n_reads, f, keeping, o);
        if (f.read_stats) stats_.empty_reads[STATS_PREPARED] += o.reads_kept;
        return;
    }
    if (f.mask_qual) mask_block(hb, f, st, src, d_qual);
    filter_block(hb, f, fs, src, d_qual, trim_err, o);
    raw_refusals();
    if (f.mask_qual) mask_done(hb, st, src, o); // (the block's list is the one behind the mask before the block is placed)
    const KeptPart k = cut_at_cap(fs, n_reads, cap_need, o);
    // the prepared snapshot: exactly what the block hands on -- the filter's flags below the cap's cut, on the block before it is compacted
    if (f.read_stats)
        run_read_stats(stats_, STATS_PREPARED, src, f.read_stats == 1 ? d_qual : nullptr, hb.qual_bias, d_stats_rev, fs.d_flag.data(), k.take, cs);
    o.mapped_reads = k.n_reads;
    o.mapped_bases = k.n_bases;
    if (k.n_bases == 0) { // nothing of the block is left, or empty reads only
        hand_back_stage();
        count_unmapped(k.n_reads, keeping);
        return;
    }
    // 6. place, 7. map
    const DeviceBatch cur = place_block(fs, src, k, keeping);
    if (keeping) {
        if (pair_.record) { // the kept reads' numbers: the filter's flags and their scan below the cap's cut, or all of a whole block
            const bool whole = k.n_reads == n_reads;
            if (!pair_number_block(k.n_reads, whole ? nullptr : fs.d_flag.data(), fs.d_rank.data(), n_reads, k.take, pair_base, copy_stream_))
                throw Error(DRPRG_ENOMEM, "mate overlap: no room in the resident set for a block's source numbers (DRPRG_HIP_KEEP_READS_GB raises the limit)");
        }
        resident_.add(cur, k.n_reads);
        map_resident_block(cur);
    } else map(cur, nullptr, nullptr, stream_, true);
}

Mapper::TrimOutcome& Mapper::TrimOutcome::operator+=(const TrimOutcome& o)
{
    reads_seen += o.reads_seen; bases_seen += o.bases_seen; reads_lost_base += o.reads_lost_base; cut_front += o.cut_front;
    cut_tail += o.cut_tail; qcut_front += o.qcut_front; qcut_tail += o.qcut_tail; emptied += o.emptied;
    return *this;
}

Mapper::AdapterOutcome& Mapper::AdapterOutcome::operator+=(const AdapterOutcome& o)
{
    reads_seen += o.reads_seen; bases_seen += o.bases_seen; reads_cut += o.reads_cut; bases_cut += o.bases_cut; reads_emptied += o.reads_emptied;
    return *this;
}

Mapper::PolyOutcome& Mapper::PolyOutcome::operator+=(const PolyOutcome& o)
{
    reads_seen += o.reads_seen; bases_seen += o.bases_seen; reads_cut += o.reads_cut; bases_cut += o.bases_cut; reads_emptied += o.reads_emptied;
    return *this;
}

Mapper::ComplexityOutcome& Mapper::ComplexityOutcome::operator+=(const ComplexityOutcome& o)
{
    reads_judged += o.reads_judged; bases_judged += o.bases_judged; reads_dropped += o.reads_dropped; bases_dropped += o.bases_dropped;
    return *this;
}

Mapper::MaskOutcome& Mapper::MaskOutcome::operator+=(const MaskOutcome& o)
{
    reads_seen += o.reads_seen; bases_seen += o.bases_seen; reads_masked += o.reads_masked; bases_masked += o.bases_masked;
    bases_already_unknown += o.bases_already_unknown;
    return *this;
}

Mapper::DecoyOutcome& Mapper::DecoyOutcome::operator+=(const DecoyOutcome& o)
{
    reads_judged += o.reads_judged; bases_judged += o.bases_judged; reads_dropped += o.reads_dropped; bases_dropped += o.bases_dropped;
    valid += o.valid; hits += o.hits;
    return *this;
}

Mapper::FilterOutcome& Mapper::FilterOutcome::operator+=(const FilterOutcome& o)
{
    poly += o.poly; cplx += o.cplx;
    mask += o.mask;
    decoy += o.decoy;
    trim += o.trim; adapter += o.adapter; front += o.front;
    reads_seen += o.reads_seen; bases_seen += o.bases_seen; dropped_short += o.dropped_short; dropped_long += o.dropped_long;
    dropped_lowq += o.dropped_lowq; reads_kept += o.reads_kept; bases_kept += o.bases_kept;
    mapped_reads += o.mapped_reads; mapped_bases += o.mapped_bases; cut_dropped += o.cut_dropped;
    return *this;
}

} // namespace drprg
