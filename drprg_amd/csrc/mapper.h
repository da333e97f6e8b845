// mapper.h -- device context of the predict hot path: index tables resident in HBM, per-batch
// workspace, and the launch sequence sketch+probe -> sort -> cluster -> accumulate.
//
// This is the MI355X replacement for the read loop of `pandora map` (pangraph_from_read_file),
// spawned by the reference at /root/reference/src/lib.rs:580-642.
#pragma once
#include "device_mem.h"
#include "index.h"
#include "kernels.h"
#include <functional>
#include <optional>
#include <vector>

namespace drprg {

struct MapCounters {
    uint64_t reads = 0, bases = 0, minimizers = 0, hits = 0, clusters_kept = 0, hits_kept = 0;
    uint64_t kernel = 0; // sketch kernel in use: 1 direct (sketch_probe_kernel), 2 Bloom-prefiltered (sketch_filter_kernel)
    uint64_t leftover_reads = 0; // filtered sequence: reads that read_cluster_kernel left to the generic pipeline
    // another device's counts added in (`kernel` names a kernel form and is no count: it stays this device's)
    MapCounters& operator+=(const MapCounters& o)
    {
        reads += o.reads; bases += o.bases; minimizers += o.minimizers; hits += o.hits;
        clusters_kept += o.clusters_kept; hits_kept += o.hits_kept; leftover_reads += o.leftover_reads;
        return *this;
    }
};

// the eight words of drprg_hip_counters and of the coverage cache, in their order
inline void to_words(const MapCounters& c, uint64_t out[8])
{
    const uint64_t v[8] = { c.reads, c.bases, c.minimizers, c.hits, c.clusters_kept, c.hits_kept, c.kernel, c.leftover_reads };
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}

class Mapper {
public:
    Mapper(const FlatIndex& idx, const MapParams& p, int device);
    ~Mapper();
    Mapper(const Mapper&) = delete;
    Mapper& operator=(const Mapper&) = delete;

    int device() const { return device_; }
    uint32_t n_knodes() const { return n_knodes_; }
    uint32_t n_prgs() const { return n_prgs_; }
    hipStream_t stream() const { return stream_; }
    void set_params(const MapParams& p);

    // One batch that is resident in HBM, in either form.  packed: d_bases points at the 2-bit words (kernels.h SketchArgs::packed), u32[ceil(n_bases / 16)],
    // and d_npos at the n_npos ascending positions of the bases that are not ACGTacgt (may be null when n_npos == 0).  What a host batch becomes
    // once it is copied, what keep_reads keeps, and what every launch function is told about its input.
    struct DeviceBatch {
        const uint8_t* d_bases = nullptr;
        const uint64_t* d_offsets = nullptr;
        uint64_t n_reads = 0, n_bases = 0;
        bool packed = false;
        const uint64_t* d_npos = nullptr;
        uint64_t n_npos = 0;
    };
    // Map such a batch.  d_bases must be 16-byte aligned.  Coverage is accumulated into d_covg (u32[2*n_knodes]) and d_prg_reads (u32[n_prgs]);
    // nullptr selects the context's own accumulators, a null stream its own stream.  The filtered sequence reads packed words directly; the
    // direct sequences get an ASCII expansion made on the device (packed.hip).
    // deferred == false: the candidate sequences return once the batch is complete; the generic one is asynchronous on `stream` except for
    // one 16-byte read-back of the hit count between the sketch and the sort.
    // deferred == true: the launch sequence is queued on `stream` and the call returns; the read-back the sequence ends with (buffer overflow
    // flags, reads left to the generic pipeline, counters) is looked at while the NEXT batch runs -- by the next deferred map, or by sync() and
    // everything that reads results -- so that back-to-back batches leave no gap on the device (measured on 10 M x 150 bp: ~50 us of host
    // round trip per 0.7 ms batch).  The caller keeps the batch's buffers and the accumulators valid and unchanged until the call after the
    // next one returns, or sync() does (a batch whose candidate buffers overflowed is run again from them).  The filtered sequence and the
    // direct sequence in its candidate form (two lanes in turn) have this form; everything else, and a batch of empty reads, runs as if
    // deferred were false and then waits for the stream.
    void map(const DeviceBatch& b, uint32_t* d_covg, uint32_t* d_prg_reads, hipStream_t stream, bool deferred);
    void sync(); // completes the batch a deferred map left in flight and waits for its stream
    // what map refuses a batch for, checked without touching anything: the only place that throws these errors
    static void check(const DeviceBatch& b);

    // Depth cap (drprg_hip_set_max_covg; the running total is kept by the context, capi_map.cpp): where a device batch reaches `target` bases.
    // n_reads = the smallest i in [1, n_reads] with d_offsets[i] >= target (n_reads if there is none), n_bases = d_offsets[i], n_npos = how
    // many of the batch's listed positions lie below that.  Completes the batch a deferred map left in flight, runs covg_cut_kernel on
    // `stream` and waits for it: called for the one batch that crosses the cap, never for a batch that cannot reach it.  Refuses what
    // check() refuses; a batch without reads has no cut (all zero).
    struct CutPoint {
        uint64_t n_reads, n_bases, n_npos;
    };
    CutPoint find_cut(const DeviceBatch& b, uint64_t target, hipStream_t stream);

    // ASCII -> packed on the device (harnesses: bench.py packs its synthetic batch; tests).  Returns the number of non-ACGT bases; their
    // positions are in d_npos, ascending, if there are at most npos_cap of them.  Synchronises `stream`.
    uint64_t pack_on_device(const uint8_t* d_bases, uint64_t n_bases, uint32_t* d_words, uint64_t* d_npos, uint64_t npos_cap, hipStream_t stream);
    // BAM's 4-bit form -> packed on the device (bam_pack.hip; kernels.h launch_bam_pack says what the arrays hold).  Returns the number of
    // non-ACGT positions; they are in d_npos, ascending, if there are at most npos_cap of them.  Synchronises `stream`.
    uint64_t pack_bam_on_device(const uint8_t* d_seq, const uint64_t* d_seq_start, const uint64_t* d_offsets, const uint8_t* d_reverse, uint64_t n_reads,
        uint64_t n_bases, uint32_t* d_words, uint64_t* d_npos, uint64_t npos_cap, hipStream_t stream);
    // a host batch in one of three forms (packed: `bases` points at the words, npos / n_npos as above, in host memory; bam: `bases`
    // points at seq_bytes bytes of 4-bit sequence fields, read i starting at byte seq_start[i] and reverse-complemented when reverse[i]
    // != 0, n_npos counts the codes that are not A, C, G or T and npos is null -- ingest.h PinnedBatch)
    struct HostBatch {
        const uint8_t* bases = nullptr;
        const uint64_t* offsets = nullptr;
        uint64_t n_reads = 0;
        bool packed = false;
        const uint64_t* npos = nullptr;
        uint64_t n_npos = 0;
        bool bam = false;
        const uint64_t* seq_start = nullptr;
        const uint8_t* reverse = nullptr;
        uint64_t seq_bytes = 0;
        // the reads' quality bytes (ingest.h PinnedBatch::qual: n_bases() of them, indexed in bases in every form) and what to take off a
        // byte to get the Phred quality; looked at by map_host_filtered only, and only under a quality threshold
        const uint8_t* qual = nullptr;
        uint32_t qual_bias = 0;
        // Read statistics on a block that goes through map_host / map_host_async (no prep setting: capi_map.cpp sets these on the blocks of
        // drprg_hip_map_fastx; map_host_filtered reads ReadFilter::read_stats instead).  stats_mode: 0 off, 1 with qualities (qual is set
        // then), 2 without; stats_which: bit STATS_RAW / STATS_PREPARED set for the snapshots the block is counted into.
        uint8_t stats_mode = 0, stats_which = 0;
        uint64_t n_bases() const { return offsets[n_reads]; }
        // what the batch takes on the device once it is there (a BAM batch: converted to the packed form)
        uint64_t payload_bytes() const { return packed || bam ? ((n_bases() + 15) / 16) * 4 : n_bases(); }
    };
    uint64_t bam_blocks() const { return bam_blocks_; } // BAM batches converted on this device since the last reset_coverage
    // Map a host batch (copied into a staging set, then map on the own accumulators).
    void map_host(const HostBatch& b);
    // The same without waiting for the kernels: the copy to the device runs on a copy stream into one of two staging sets, the
    // launch sequence is queued behind it (a deferred map) and the call returns as soon as the COPY is done -- the host block
    // may be reused then -- so that the next block's copy overlaps this block's kernels.  sync() (or anything that reads
    // results) completes what is in flight.  Sequences without a deferred form fall back to map_host.
    void map_host_async(const HostBatch& b);
    // The read filter (the rule: include/drprg_hip.h "read filter"; read_qual.hip).  T: the rule's threshold for min_qual_milli
    // (dev::rq_threshold), 0 when there is no quality test.
    // Read trimming (the rule: include/drprg_hip.h "read trimming"; read_trim.hip) rides in the same settings: it runs in front of the
    // filter, on the same block.  trim_window is 1..32 whenever trim_qual_milli != 0.  Adapter trimming (the rule: include/drprg_hip.h
    // "adapter trimming"; adapter_trim.hip) runs behind the crops and the quality trim, inside the same stage; it needs no quality byte.
    struct ReadFilter {
        uint64_t min_len = 0, max_len = 0, T = 0;
        uint32_t min_qual_milli = 0;
        uint64_t trim_front = 0, trim_tail = 0;
        uint32_t trim_qual_milli = 0, trim_window = 0;
        dev::AdapterSet adapters {}; // n == 0: none (3' adapters under the indel rule)
        // the indel rule (drprg_hip_set_adapters2, adapter_edit.hip): 5' adapters, held letter-reversed, and both sides' match masks
        bool adapter_indels = false;
        dev::AdapterSet front_adapters {};
        dev::AdapterEq eq3 {}, eq5 {};
        // The decoy screen (the rule: include/drprg_hip.h "decoy screen"; decoy_screen.hip): K (0: no decoy set), f and M.  The table
        // itself lives on every device of the context (set_decoy); decoy_id names the set these settings were made for, and a Mapper
        // refuses to screen against any other.
        uint32_t decoy_k = 0, decoy_frac_milli = 0, decoy_min_kmers = 0;
        uint64_t decoy_id = 0;
        // Base masking (the rule: include/drprg_hip.h "base masking"; base_mask.hip): Q, 1..93 (0: off).  Behind the trim stage, in
        // front of the decoy screen and the filter; it needs the quality bytes.
        uint32_t mask_qual = 0;
        // Poly tails (the rule: include/drprg_hip.h "poly tails"; poly_tail.hip): the set S (bit 0 A, 1 C, 2 G, 3 T; 0: off) and M,
        // 2..255 whenever S is set.  Inside the trim stage, behind both adapter sides; it needs no quality byte.
        uint32_t poly_letters = 0, poly_min_len = 0;
        // The low-complexity filter (the rule: include/drprg_hip.h "read complexity"; read_complexity.hip): P, 1..100 (0: off).  Behind
        // the mask, on the reads the length and quality tests kept, in front of the decoy screen's verdict.
        uint32_t min_complexity = 0;
        // Read statistics (the rule: include/drprg_hip.h "read statistics"; read_stats.hip): 0 off, 1 with qualities, 2 without.  No prep
        // setting -- any() does not see it: a block of a context without one goes through map_host_async and is counted there.
        uint32_t read_stats = 0;
        bool decoy() const { return decoy_k != 0; }
        bool poly() const { return poly_letters != 0; }
        bool any_adapters() const { return adapters.n != 0 || front_adapters.n != 0; }
        bool crops() const { return trim_front || trim_tail || trim_qual_milli; } // what drprg_hip_read_trim_info counts
        bool filters() const { return min_len || max_len || min_qual_milli; }
        bool trims() const { return crops() || any_adapters() || poly(); }
        bool trim_points() const { return any_adapters() || poly(); } // the trim stage looks at the bases (a packed block's bitmap first)
        bool any() const { return filters() || trims() || decoy() || mask_qual || min_complexity; }
        bool use_qual() const { return min_qual_milli != 0; }
        bool wants_qual() const { return min_qual_milli != 0 || trim_qual_milli != 0 || mask_qual != 0 || read_stats == 1; } // the ingest carries quality bytes
        bool qual_behind_trim() const { return use_qual() || mask_qual != 0 || read_stats == 1; } // the trim stage gathers the trimmed reads' quality bytes
    };
    // (operator+=: a block's outcome added to a running total, count by count)
    struct TrimOutcome { // drprg_hip_read_trim_info
        uint64_t reads_seen = 0, bases_seen = 0, reads_lost_base = 0, cut_front = 0, cut_tail = 0, qcut_front = 0, qcut_tail = 0, emptied = 0;
        TrimOutcome& operator+=(const TrimOutcome& o);
    };
    struct AdapterOutcome { // drprg_hip_adapter_trim_info
        uint64_t reads_seen = 0, bases_seen = 0, reads_cut = 0, bases_cut = 0, reads_emptied = 0;
        AdapterOutcome& operator+=(const AdapterOutcome& o);
    };
    struct DecoyOutcome { // drprg_hip_decoy_info: the reads the other tests kept, and what the screen made of them
        uint64_t reads_judged = 0, bases_judged = 0, reads_dropped = 0, bases_dropped = 0, valid = 0, hits = 0;
        DecoyOutcome& operator+=(const DecoyOutcome& o);
    };
    struct MaskOutcome { // drprg_hip_base_mask_info: the reads and bases behind the cuts, and what the mask made of them
        uint64_t reads_seen = 0, bases_seen = 0, reads_masked = 0, bases_masked = 0, bases_already_unknown = 0;
        MaskOutcome& operator+=(const MaskOutcome& o);
    };
    struct PolyOutcome { // drprg_hip_poly_trim_info: the reads and bases behind both adapter cuts, and what the tail cut took
        uint64_t reads_seen = 0, bases_seen = 0, reads_cut = 0, bases_cut = 0, reads_emptied = 0;
        PolyOutcome& operator+=(const PolyOutcome& o);
    };
    struct ComplexityOutcome { // drprg_hip_complexity_info: the reads the length and quality tests kept, and what the threshold dropped
        uint64_t reads_judged = 0, bases_judged = 0, reads_dropped = 0, bases_dropped = 0;
        ComplexityOutcome& operator+=(const ComplexityOutcome& o);
    };
    struct FilterOutcome {
        PolyOutcome poly;       // (all zero without poly-tail trimming)
        ComplexityOutcome cplx; // (all zero without a complexity threshold)
        MaskOutcome mask;       // (all zero without a base mask)
        DecoyOutcome decoy;     // (all zero without a decoy set)
        TrimOutcome trim;       // (all zero without a crop or a quality trim)
        AdapterOutcome adapter; // (all zero without adapters)
        AdapterOutcome front;   // drprg_hip_front_adapter_info (all zero without 5' adapters; bases_seen: behind the 3' cut)
        uint64_t reads_seen = 0, bases_seen = 0, dropped_short = 0, dropped_long = 0, dropped_lowq = 0, reads_kept = 0, bases_kept = 0;
        uint64_t mapped_reads = 0, mapped_bases = 0; // what was mapped: the kept reads, or those of them in front of the depth cap
        uint64_t cut_dropped = 0;                    // kept reads behind the depth cap
        bool cut = false;                            // (of one block: not summed)
        FilterOutcome& operator+=(const FilterOutcome& o);
    };
    // map_host_async behind the filter: the block is copied into a staging set -- its quality bytes too, under a quality threshold --, the
    // filter runs on the copy stream, the call waits for its 64-byte read-back (the caller's block is free then) and what is left of the
    // block is mapped as map_host_async maps a block: a block that lost no read as it lies in the staging set, any other compacted by the
    // kernels of subsample.hip; under keep_reads the block that stays is the compacted one, carved from the arena at its own size (a block
    // that lost nothing is copied there on the device).  Quality bytes never stay.  cap_need != 0: the depth cap is reached at the
    // cap_need-th kept base of this block (counted from 1): the kept reads up to the one that holds it are mapped, as cap_host_cut cuts a block.
    void map_host_filtered(const HostBatch& b, const ReadFilter& f, uint64_t cap_need, FilterOutcome& out);
    // The filter alone on the caller's device buffers (drprg_hip_read_filter_device): d_sums (may be null) receives the sums of E, d_flags
    // one byte per read; res[0..7]: dev::RF_*.  d_qual must be readable for 64 bytes behind n_bases when it is 16-byte aligned (any other
    // address is read byte by byte).  Synchronises `stream`.
    void read_filter_device(const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases,
        unsigned long long* d_sums, uint8_t* d_flags, uint64_t res[8], hipStream_t stream);
    // The trim kernels alone on the caller's device buffers (drprg_hip_read_trim_device): d_begin / d_end receive every read's kept range in
    // read orientation; d_rev: one byte per read (non-zero: the quality bytes are stored mirrored) or null; d_qual may be null without a
    // quality threshold, and must be readable for 64 bytes behind n_bases when it is 16-byte aligned.  res[0..8]: dev::RT_*.  Synchronises `stream`.
    void read_trim_device(const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, const uint8_t* d_rev, uint64_t n_reads,
        uint64_t n_bases, uint64_t* d_begin, uint64_t* d_end, uint64_t res[9], hipStream_t stream);
    // The adapter kernels alone on the caller's device buffers, under whatever adapter rule is set (drprg_hip_adapter_trim_device and
    // drprg_hip_adapter_trim_device2): the bases as text (d_words == null) or as packed words with their ascending position list; d_begin /
    // d_end hold every read's range, d_end receives the cut ranges' ends and, under 5' adapters, d_begin their begins.  res[0..4]: the 3'
    // side's reads seen, bases seen, reads cut, bases cut, reads emptied; res[5..9]: the 5' side's (bases seen: behind the 3' cut); res[10]:
    // the ranges do not lie inside the reads.  Synchronises `stream`.
    void adapter_trim_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
        uint64_t n_reads, uint64_t n_bases, uint64_t* d_begin, uint64_t* d_end, uint64_t res[11], hipStream_t stream);
    // The tail cut alone on the caller's device buffers (drprg_hip_poly_trim_device): buffers as for adapter_trim_device; d_end receives the
    // cut ranges' ends.  res[0..4]: reads seen, bases seen, reads cut, bases cut, reads emptied; res[5]: the ranges do not lie inside the
    // reads.  Synchronises `stream`.
    void poly_trim_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
        uint64_t n_reads, uint64_t n_bases, const uint64_t* d_begin, uint64_t* d_end, uint64_t res[6], hipStream_t stream);
    // The complexity kernels alone on the caller's device buffers (drprg_hip_complexity_device): the bases as for adapter_trim_device; d_diff
    // (may be null) receives D, d_flags 1 for a kept read; res[0..1]: reads dropped, bases dropped; res[2]: the offsets do not ascend from
    // 0 to n_bases.  Synchronises `stream`.
    void complexity_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
        uint64_t n_reads, uint64_t n_bases, uint32_t* d_diff, uint8_t* d_flags, uint64_t res[3], hipStream_t stream);
    // The decoy set of this device (drprg_hip_set_decoy).  text: the records' letters, one 'N' between two records; windows: the windows
    // of the records (what the table is sized by); set: the name ReadFilter::decoy_id carries.  The table is built on the device
    // (decoy_screen.hip) and stays until clear_decoy or the Mapper goes; -EINVAL, and no set, when the text holds no k-mer.
    void set_decoy(const std::vector<uint8_t>& text, uint64_t windows, uint32_t k, uint64_t set);
    void clear_decoy();
    uint64_t decoy_distinct() const { return decoy_.distinct; }
    uint64_t decoy_slots() const { return decoy_.table.size(); }
    // found[i] = 1 iff canonical k-mer kmers[i] is in the table.  Synchronises.
    void decoy_lookup(const std::vector<uint64_t>& kmers, uint8_t* found);
    // The screen kernels alone on the caller's device buffers (drprg_hip_decoy_screen_device): the bases as for adapter_trim_device;
    // d_valid / d_hits (either may be null) receive V and H, d_flags 1 for a kept read; res[0..3]: reads dropped, bases dropped, sum of V,
    // sum of H; res[4]: the offsets do not ascend from 0 to n_bases.  Synchronises `stream`.
    void decoy_screen_device(const ReadFilter& f, const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
        uint64_t n_reads, uint64_t n_bases, uint32_t* d_valid, uint32_t* d_hits, uint8_t* d_flags, uint64_t res[5], hipStream_t stream);
    // The mask kernels alone on the caller's device buffers (drprg_hip_base_mask_device): the quality bytes as for read_trim_device, the
    // bases -- changed in place -- as text (d_words == null) or as packed words with their ascending position list, which is left as it is:
    // the list behind the mask goes to d_npos_out (may be d_npos's own buffer only if it is no longer needed: it is read first), when it
    // holds at most npos_cap positions.  res[0..4]: reads seen, bases seen, reads masked, bases masked, bases already unknown; res[5]: the
    // new list's length; res[6]: first bad quality byte + 1, or 0; res[7]: the offsets do not run from 0 to n_bases.  Synchronises `stream`.
    void base_mask_device(const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, const uint8_t* d_rev, uint64_t n_reads,
        uint64_t n_bases, uint8_t* d_text, uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, uint64_t* d_npos_out, uint64_t npos_cap, uint64_t res[8],
        hipStream_t stream);
    // Read statistics (drprg_hip_set_read_stats): two snapshots of dev::RS_WORDS words, kept in device memory per Mapper, zeroed by
    // reset_coverage(true), added to by every block that is counted: STATS_RAW the block as it arrived, STATS_PREPARED what it hands on to
    // mapping.  read_stats: the snapshot, read back (synchronises; RS_MIN_LEN is ~0 without a read: the caller folds the devices first).
    // check_read_stats: what the kernels refused since the reset, thrown (synchronises; map_host_filtered looks per block, the other
    // paths leave it to the end of the pass).  count_host_block: a host block copied in and counted into the snapshots of hb.stats_which,
    // nothing else (the block the depth cap cuts, as the file held it); waits.
    enum { STATS_RAW = 0, STATS_PREPARED = 1 };
    void read_stats(int which, uint64_t out[dev::RS_WORDS]);
    void check_read_stats();
    void count_host_block(const HostBatch& hb);
    // The kernels alone on the caller's device buffers (drprg_hip_read_stats_device): the bases as for adapter_trim_device, the quality
    // bytes as for base_mask_device or null (no quality section is filled), d_flags one byte per read (0: not counted) or null, take: only
    // reads below it count.  out: one snapshot; res[0]: first bad quality byte + 1, or 0; res[1]: the offsets do not ascend from 0 to
    // n_bases.  Synchronises `stream`.
    void read_stats_device(const uint8_t* d_text, const uint32_t* d_words, const uint64_t* d_npos, uint64_t n_npos, const uint8_t* d_qual, uint32_t bias,
        const uint64_t* d_offsets, const uint8_t* d_rev, uint64_t n_reads, uint64_t n_bases, const uint8_t* d_flags, uint64_t take, uint64_t out[dev::RS_WORDS],
        uint64_t res[2], hipStream_t stream);
    // Reads that stay in HBM (off by default).  keep_reads(max_bytes > 0): from now on map_host_async copies every block into
    // device memory of its own instead of a staging set and leaves it there -- at most max_bytes of it; one byte more and
    // everything kept is dropped and the staging sets are back.  kept_complete(): every read mapped since keep_reads() /
    // reset_coverage() is among kept().  What they are for: select_reads_with_anchors below (the pile-up of `discover` without a
    // second pass over the file) and mapping the same reads again against another index (map_kept_from).
    void keep_reads(uint64_t max_bytes);
    bool kept_complete() const { return resident_.active(); }
    const std::vector<DeviceBatch>& kept() const { return resident_.kept; }
    uint64_t kept_bytes() const { return resident_.bytes; }
    void drop_kept();
    // Every kept read that holds one of `anchors` (k-mers of length A <= 31 packed 2 bits per base, A=0 .. T=3, first base in the
    // high bits) -- and possibly a few that do not -- appended to bases / offsets (offsets[0] = 0 is written when offsets is
    // empty), in batch and read order.  anchor_scan.hip.  ids (may be null): kept batch << 32 | read in the batch of every read appended.
    // window_bytes: how much ASCII expansion of packed batches one window holds (0: SELECT_WINDOW_BYTES).
    static constexpr uint64_t SELECT_WINDOW_BYTES = 1ull << 30;
    void select_reads_with_anchors(std::vector<uint64_t> anchors, uint32_t A, std::vector<uint8_t>& bases, std::vector<uint64_t>& offsets,
        std::vector<uint64_t>* ids = nullptr, uint64_t window_bytes = 0);
    // maps the batches another Mapper of the same device keeps (it must outlive the call); returns the reads mapped
    uint64_t map_kept_from(const Mapper& other);
    // Random subsample of the resident sample to target_bases (the rule: include/drprg_hip.h "random subsample"; subsample.hip).  Needs
    // kept_complete().  The sum of the lengths is at most target_bases: nothing happens.  Otherwise the kept reads are selected on the device,
    // every resident block is compacted into a block of its kept reads (arenas of their own: the peak is the old set plus the new one), the
    // old arenas go back through their owners, coverage, reads per PRG and the counters are cleared and the new set is mapped; kept(),
    // kept_bytes() and everything that reads them see the kept reads from then on.  flags: one byte per read of the sample as it was,
    // 1 = kept (left empty when nothing was dropped).
    struct SubsampleResult {
        uint64_t reads_before, bases_before, reads_kept, bases_kept;
    };
    SubsampleResult subsample_kept(uint64_t target_bases, uint64_t seed, std::vector<uint8_t>& flags);
    // Exact duplicate reads dropped from the resident sample (the rule: include/drprg_hip.h "duplicate reads"; dedup.hip).  Needs
    // kept_complete().  Fewer than two reads with bases, or no read dropped: nothing else happens (no compaction, coverage and counters
    // untouched, flags left empty).  Otherwise what subsample_kept does with its selection.  key_bits (1..64): how many low bits of the
    // content key the sort sees; the result does not depend on it.  A call that fails leaves the sample as it was.
    SubsampleResult dedup_kept(uint32_t key_bits, std::vector<uint8_t>& flags);
    // The key kernel alone on the caller's packed batch (drprg_hip_dedup_keys_device): d_keys[i] = the content key of read i, 0 for a read
    // of no bases.  Synchronises `stream`.
    void dedup_keys_device(const uint32_t* d_words, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, const uint64_t* d_npos, uint64_t n_npos,
        unsigned long long* d_keys, hipStream_t stream);
    // Mate overlap (the rule: include/drprg_hip.h "mate overlap"; pair_overlap.hip).  min_overlap 8 .. PO_MAX_LEN, error_milli 0 .. 250.
    struct PairSetting {
        uint32_t min_overlap = 0, error_milli = 0;
        bool clip = false;
        bool merge = false; // mate merging (drprg_hip_set_pair_merge; never beside clip)
        bool on() const { return min_overlap != 0; }
    };
    // one side of the caller's pairs: a packed batch of n_pairs reads
    struct PairSide {
        const uint32_t* d_words;
        const uint64_t* d_offsets;
        uint64_t n_bases;
        const uint64_t* d_npos;
        uint64_t n_npos;
    };
    // The stage on the resident sample.  pair_record(true): from now on every block the resident set takes gets the source numbers of its
    // reads (their numbers among the reads of their side as the files held them, counted before any stage dropped one); begin_mates(): the
    // reads mapped from here on are side 2.  pair_overlap_kept: needs kept_complete(), one begin_mates() call and sides of the same size;
    // mates are found by source number and judged by the rule; no read lost a base: nothing else happens (no compaction, coverage and
    // counters untouched).  Otherwise every block is compacted by the ranges [0, keep) into a new set and the cut reads are mapped afresh, as
    // dedup_kept does with its flags.  shifts: per source pair the chosen shift (PO_NO_SHIFT, PO_NOT_JUDGED).  The source numbers are
    // dropped either way.  A call that fails leaves the sample as it was.
    void pair_record(bool on) { pair_.record = on; }
    void begin_mates();
    // set.merge (the rule: include/drprg_hip.h "mate merging"; pair_merge.hip): every pair with a chosen shift becomes its merged read in a's
    // place and a read of no bases in b's; no pair has a chosen shift: nothing else happens.  merged: the PM_WORDS counts (null without merge).
    void pair_overlap_kept(const PairSetting& set, std::vector<int32_t>& shifts, uint64_t counts[dev::PO_WORDS], uint64_t* merged = nullptr);
    // The two pair kernels alone on the caller's packed batches (drprg_hip_pair_overlap_device): pair s is (read s of a, read s of b).
    // d_shift[s] the chosen shift (PO_NO_SHIFT, PO_NOT_JUDGED), d_keep_a[s] / d_keep_b[s] the bases either mate keeps, counts the PO_WORDS
    // counters.  Synchronises `stream`.
    void pair_overlap_device(const PairSetting& set, const PairSide& a, const PairSide& b, uint64_t n_pairs, int32_t* d_shift, uint64_t* d_keep_a, uint64_t* d_keep_b,
        uint64_t counts[dev::PO_WORDS], hipStream_t stream);
    // The overlap kernel and the merge kernel alone on the caller's packed batches (drprg_hip_pair_merge_device): a packed batch of n_pairs
    // reads, the merged read of a pair with a chosen shift and a read of no bases for every other.  d_out_offsets: u64[n_pairs + 1];
    // d_out_words / d_out_npos: room for cap_words words and cap_npos positions (too little: DRPRG_EOVERFLOW, nothing is written beyond
    // them); *n_out_npos: the length of the ascending list.  Synchronises `stream`.
    void pair_merge_device(const PairSetting& set, const PairSide& a, const PairSide& b, uint64_t n_pairs, int32_t* d_shift, uint64_t* d_out_offsets, uint32_t* d_out_words,
        uint64_t cap_words, uint64_t* d_out_npos, uint64_t cap_npos, uint64_t* n_out_npos, uint64_t counts[dev::PO_WORDS], uint64_t merged[dev::PM_WORDS], hipStream_t stream);

    // Duplicate pairs dropped from the resident sample (the rule: include/drprg_hip.h "duplicate pairs"; pair_dedup.hip).
    // pair_dedup_record(true): from now on pair_overlap_kept keeps, as device buffers of pair_, the mate and the source number of every
    // resident read (the overlap stage drops no read, so the numbers hold through its compaction); off, nothing is kept.  dedup_pairs_kept
    // needs that record of this very sample -- any other compaction releases it -- and begins as dedup_kept does; no unit dropped: nothing
    // else happens.  counts: the eight PD_* counts, levels: the 32 duplication levels.  The record is released when the call is done;
    // a call that fails leaves it, and the sample, as they were.
    void pair_dedup_record(bool on)
    {
        pair_.dedup = on;
        if (!on) pair_.release_record();
    }
    SubsampleResult dedup_pairs_kept(uint32_t key_bits, std::vector<uint8_t>& flags, uint64_t counts[8], uint64_t levels[32]);
    // The stage's kernels alone on the caller's packed batches (drprg_hip_dedup_pairs_device): unit s is (read s of a, read s of b).
    // d_keys[s] = U, d_keep[s] = 0 for a duplicate unit, d_copies[s] = the copies of a kept unit with bases, else 0; out: the PD_WORDS
    // words.  Synchronises `stream`.
    void dedup_pairs_device(const PairSide& a, const PairSide& b, uint64_t n_pairs, uint32_t key_bits, uint64_t* d_keys, uint8_t* d_keep, uint32_t* d_copies,
        uint64_t out[dev::PD_WORDS], hipStream_t stream);

    // this += other, on the device (the other Mapper's vectors are left as they are): peer copy into a scratch buffer + one
    // add kernel, or the add kernel alone when both live on the same device.  Both are synchronised first.
    void add_vectors_from(Mapper& other);

    // page-locked host memory for ingest blocks (H2D copies from it run at DMA speed)
    static void* pinned_alloc(size_t bytes);
    static void pinned_free(void* p);
    static void warm_device(int device);

    // new_sample: the reads kept in HBM (keep_reads) go as well.  The switches are read again: a context maps with those it was opened or last
    // reset with (DRPRG_HIP_MIN_CAPACITY, DRPRG_FORCE_MID_TIER and DRPRG_MID_MAX_RECORDS shape construction: they take effect at open only)
    void reset_coverage(bool new_sample = true);
    // own accumulators
    uint32_t* d_covg() const { return d_covg_.data(); }
    uint32_t* d_prg_reads() const { return d_covg_.data() + 2 * (size_t)n_knodes_; }
    void download(std::vector<uint32_t>& covg, std::vector<uint32_t>& prg_reads);
    void upload(const std::vector<uint32_t>& covg, const std::vector<uint32_t>& prg_reads);
    MapCounters counters(); // synchronises
    // out[0] = words of the L2-resident Bloom tier in front of the probe table (0: none), out[1] = bytes of the probe table
    // (keys + slot records), out[2] = bytes of the LDS-resident filter arrays (0: none), out[3] = sequence in use (1/2/3)
    void device_tables(uint64_t out[6]) const;

    // timing of the dominant kernel (HIP events on the launch stream), for bench.py
    // is the batch queued by a deferred map (not yet completed) accumulating into these buffers?
    bool pending_writes_to(const uint32_t* covg, const uint32_t* prg_reads) const
    {
        return pending_.active && ((covg && pending_.covg == covg) || (prg_reads && pending_.prg_reads == prg_reads));
    }
    // sketch_filter_kernel's schedule and how it went in the batch completed last (bench.py; drprg_hip_filter_schedule): out[0] rounds (1: static),
    // [1] slices = tickets, [2] tiles per wave of round 0 (even share), [3..6] shares of the four wave classes in 1/256 of an even one,
    // [7..10] when the classes were through in 10 ns from the kernel's first wave (0: not clocked), [11] slices per workgroup, [12..19] chunk size per round
    void filter_schedule(uint64_t out[20]);
    // the buffers that grow when a batch does not fit them (drprg_hip_buffer_info; counts since the Mapper was made, reset() keeps them):
    // out[0] batches of the filtered sequence run again after a candidate slice overflowed, [1] the same for the direct sequence's
    // candidate form, [2] regrows of the generic hit buffer, [3] largest capacity of any lane (entries), [4] hit_capacity(), [5] sketch_form().  Synchronises.
    void buffer_info(uint64_t out[6]);
    void enable_kernel_timing(bool on) { timing_ = on; }
    double sketch_ms_total() const { return sketch_ms_; }
    uint64_t sketch_launches() const { return sketch_launches_; }
    void reset_kernel_timing() { sketch_ms_ = 0; sketch_launches_ = 0; }

private:
    // Every device allocation, pinned block, event and stream below is held by an owner of device_mem.h: nothing is freed by hand.  The
    // streams come first, so that they are destroyed last -- after the buffers that work queued on them used.
    Stream stream_, copy_stream_; // (copy_stream_: the copies of map_host_async, created with the first of them)
    void zero_now(void* p, size_t bytes);
    void ensure_workspace(uint64_t hit_capacity);
    // What one batch of a candidate sequence (filtered: sketch_filter -> verify -> read_cluster; direct: sketch -> read_cluster from the
    // tile slices) keeps to itself: candidate buffers (all of capacity() entries; grow_lane), per-sequence counters with their pinned
    // mirror, and events on the batch's stream (done: behind the batch's read-back; t0 / t1 around the dominant kernel) -- the last three
    // made by ensure_lanes.  Two lanes: deferred maps take them in turn, the synchronous calls use lane 0.
    struct Lane {
        Event done, t0, t1;
        DeviceBuffer<uint64_t> raw_pos, cand_info;
        DeviceBuffer<uint4> cand_rec;
        DeviceBuffer<uint32_t> cand_pos1, small;
        DeviceBuffer<unsigned long long> d_scratch; // L_N x u64 per-sequence counters (below)
        PinnedBuffer<unsigned long long> h_scratch; // pinned mirror
        bool scratch_zero = false;                  // d_scratch is known to be zero on the device
        dev::FilterWork fw {};
        uint64_t capacity() const { return raw_pos.size(); }
    };
    enum { L_HITS = 0, L_OVERFLOW = 1, L_MAXLEN = 2, L_UNSORTED = 3, L_COMPLEX = 4, L_CHUNK = 5, L_MINIMIZERS = 6, L_FT_CLOCK = 7 /* five words: FilterBuffers::class_clock */, L_N = 12 };
    // A batch of one of the two candidate sequences, as its launch and finish functions see it.  The description travels with the batch (a
    // re-run or its leftover reads see the format it came in) -- until round 5 the batch's ADDRESS was looked up in a map, which every free
    // and every recycled address had to keep honest.
    struct Batch {
        DeviceBatch batch;
        bool active = false;
        bool direct = false; // the direct sequence's candidate form (else the filtered sequence)
        int lane = 0;        // lanes_[lane] (direct: and tsets_[lane])
        uint32_t *covg = nullptr, *prg_reads = nullptr;
        hipStream_t stream = nullptr;
    };
    Batch make_batch(int lane, const DeviceBatch& batch, uint32_t* covg, uint32_t* prg_reads, hipStream_t stream) const;
    void ensure_lanes();
    void grow_lane(Lane& lane, uint64_t capacity);
    // One attempt of a batch, queued on its stream with the lane's `done` recorded behind it; finish: the attempt's read-back has arrived
    // -- false: a candidate buffer was too small, nothing was counted, the buffers have grown and the batch must run again.
    void launch(const Batch& b);
    void filter_launch(const Batch& b);
    bool filter_finish(const Batch& b, int attempt);
    void direct_launch(const Batch& b);
    bool direct_finish(const Batch& b, int attempt);
    void leftovers(const Batch& b);
    void run_batch(const DeviceBatch& batch, uint32_t* d_covg, uint32_t* d_prg_reads, hipStream_t stream);
    void cluster_hits(const uint64_t* d_offsets, uint32_t n_hits, bool ordered, unsigned long long* d_unsorted, uint32_t* d_covg,
        uint32_t* d_prg_reads, hipStream_t stream);
    // what the launch functions of a batch on a lane say alike: the lane's counters as the sketch's n_hits / n_minimizers / overflow, its
    // candidate buffers, read_cluster_kernel's arguments, and the events around the dominant kernel (when kernels are timed)
    void count_on_lane(dev::SketchArgs& a, const Lane& lane) const;
    dev::FilterBuffers filter_buffers(const Lane& lane) const;
    dev::ReadClusterArgs read_cluster_args(const Batch& b) const;
    dev::KernelTimer kernel_timer(hipEvent_t t0, hipEvent_t t1) const;
    // the batch itself, or -- for a packed batch -- its ASCII expansion in scratch buffer `slot` (0 / 1: the two tile sets of the direct
    // sequence's candidate form, 2: the generic sequence), made on `stream`
    DeviceBatch ascii_view(int slot, const DeviceBatch& batch, hipStream_t stream);
    DeviceBuffer<uint8_t> d_unpacked_[3];
    DeviceBuffer<unsigned long long> d_pack_count_; // pack_on_device's counter word
    PinnedBuffer<unsigned long long> h_cut_;        // find_cut's three result words
    void read_counters(hipStream_t stream);
    void note_kernel_time(hipEvent_t t0, hipEvent_t t1);
    // deferred completion: the batches take the two lanes in turn; `pending_` is the batch whose read-back nobody has looked at yet
    void complete_pending();
    void complete_batch(const Batch& b);
    Batch pending_;
    int pipe_next_ = 0;

    int device_ = 0;
    Switches sw_ = read_switches(); // the hot path's switches (switches.h): read at construction and again by reset_coverage
    MapParams params_;
    bool wide_hash_ = false;
    int halo_ = 16;
    uint32_t n_knodes_ = 0, n_prgs_ = 0;
    // The index on the device.  fill() refuses an index the kernels cannot address before it allocates anything, then uploads table by table.
    struct IndexTables {
        uint32_t table_bits = 0;
        DeviceBuffer<unsigned char> slot_key; // u32 keys, u64 when wide_hash
        DeviceBuffer<uint2> slot_rec;
        DeviceBuffer<uint4> slot_first;
        DeviceBuffer<uint32_t> rec_knode;
        DeviceBuffer<uint16_t> rec_prg;
        DeviceBuffer<uint32_t> min_path_len;
        DeviceBuffer<uint32_t> prg_thr; // per PRG: floor(shortest k-mer path * cluster fraction), follows set_params
        std::vector<uint32_t> h_min_path_len;
        DeviceBuffer<uint32_t> bloom;
        uint32_t bloom_wbits = 0;
        DeviceBuffer<uint32_t> pbloom; // Bloom tier of the direct kernel (large indexes)
        uint32_t pbloom_wbits = 0;
        DeviceBuffer<uint32_t> bloom0;  // level 0 of the filter (k = 15, small indexes)
        DeviceBuffer<uint32_t> bloom0f; // level 0 + second-stage bits in one array
        uint32_t bloom0_wbits = 0;
        DeviceBuffer<uint32_t> bloomr; // second stage of the level-0 form
        // middle tier of the filter (FlatIndex::mid0 / mid_bitmap / midc): level 0 in LDS, the other two in global memory (L2-resident)
        DeviceBuffer<uint32_t> mid0, mid_bitmap, midc;
        uint32_t midc_wbits = 0, mid0_bits = 0;
        DeviceBuffer<uint32_t> blkc; // small tier: the second stage as a split-block filter in global memory (FlatIndex::blkc)
        uint32_t blkc_wbits = 0;
        void fill(const FlatIndex& idx, bool wide_hash, uint64_t mid_max_records);
        dev::BloomTables bloom_tables(bool mid) const; // what sketch_filter_kernel tests against (mid: in its middle-tier form)
    };
    IndexTables tables_;
    bool use_mid_ = false;                   // the filtered sequence runs in its middle-tier form
    int n_cus_ = 256;
    bool use_filter_ = false;
    bool use_direct_cands_ = false; // direct sketch kernel in its candidate form (read_cluster_kernel instead of sort + cluster kernels)
    int sketch_form() const;
    // accumulators: ONE allocation [coverage | reads per PRG]
    DeviceBuffer<uint32_t> d_covg_;
    DeviceBuffer<unsigned long long> d_counters_; // 8 x u64: hits(batch), minimizers, clusters_kept, hits_kept, overflow, ...
    PinnedBuffer<unsigned long long> h_counters_; // pinned mirror
    // per-batch device counters are read back once per batch and summed here (an aborted attempt -- a buffer that has to
    // grow -- is simply not added, whatever sequence ran before it)
    uint64_t tot_reads_ = 0, tot_bases_ = 0, tot_hits_ = 0, tot_leftover_ = 0, tot_minimizers_ = 0;
    // workspace of the generic pipeline: hit_capacity() entries each (d_cstart_ one more), d_temp_ what the sort and the scan ask for
    DeviceBuffer<uint64_t> d_key_a_, d_key_b_;
    DeviceBuffer<uint32_t> d_val_a_, d_val_b_;
    DeviceBuffer<uint32_t> d_head_, d_scan_, d_cstart_, d_order_;
    DeviceBuffer<dev::ClusterRec> d_clusters_;
    DeviceBuffer<unsigned char> d_temp_;
    uint64_t hit_capacity() const { return d_key_a_.size(); }
    Lane lanes_[2];
    // smallest capacity of the candidate / hit buffers, in entries (DRPRG_HIP_MIN_CAPACITY, taken at construction; tests lower it so that
    // small batches run at the production ratio -- n_bases / 48 for the filtered sequence --, or below it to make the buffers regrow)
    static constexpr uint64_t MIN_CAPACITY_CLAMP = 4096;
    uint64_t min_capacity_ = 1u << 20;
    uint64_t reruns_filter_ = 0, reruns_direct_ = 0, regrows_hits_ = 0; // buffer_info
    // candidate form of the direct sequence: ws_tiles slices of ws_cap records, one slice per tile, with the per-tile counts and the scan's
    // scratch (ensure_tile_workspace).  One set of the workspace per lane (a batch's slices must survive until its read-back has been
    // looked at: reads left to the generic pipeline are gathered from them).  d_tile_first also serves the generic sequence (set 0).
    struct TileSet {
        uint32_t slice_cap = 256, ws_tiles = 0, ws_cap = 0;
        DeviceBuffer<uint64_t> d_tile_info;
        DeviceBuffer<uint32_t> d_tile_pos1, d_tile_count, d_tile_hits, d_tile_nmin, d_tile_prefix;
        DeviceBuffer<uint4> d_tile_rec;
        DeviceBuffer<unsigned char> d_tile_temp;
        DeviceBuffer<uint32_t> d_tile_first; // first read of every tile (reserve_tile_first)
        // packed batches through sketch_wave_kernel: one bit per base in u16 words, set for the positions in the batch's npos (allocated
        // with the first batch that has any; all zero except between a launch and the next launch on this set)
        DeviceBuffer<uint16_t> d_nbits;
        bool nbits_dirty = false;
        uint32_t mark = 0, n_tiles = 0;   // of the batch in flight
        dev::SketchArgs a_done {};
    };
    TileSet tsets_[2];
    // the sketch's arguments for a batch; `tiles`: the tile set whose first-read table it fills -- tsets_[lane] for a direct batch,
    // tsets_[0] for the generic sequence, null for the filtered sequence, whose kernels have no such table
    dev::SketchArgs sketch_args(const DeviceBatch& batch, const TileSet* tiles) const;
    uint32_t slices_epoch_ = 0x80000000u; // mark of the last batch whose candidates read_cluster_kernel took from the slices
    void ensure_tile_workspace(TileSet& t, uint32_t n_tiles, uint32_t tile_cap);
    void reserve_tile_first(TileSet& t, uint32_t n_tiles);
    // host staging: device buffers a host batch is copied into, each replaced by one a quarter larger when a batch does not fit it
    // (ensure_stage).  map_host has one set; map_host_async takes two in turn, their copies on copy_stream_ with `copied` behind them
    struct BamScratch { // launch_bam_pack's per-workgroup counts, their scan and the scan's scratch
        DeviceBuffer<uint32_t> d_count, d_prefix;
        DeviceBuffer<unsigned char> d_temp;
    };
    // a buffer too small for `need` elements is replaced by one of `grown` -- a quarter more, unless the caller has a padding rule of its
    // own --, behind sync(): freeing device memory waits for the device, and this is explicit about the batch in flight
    template <typename Buf> void grow(Buf& buf, uint64_t need, uint64_t grown)
    {
        if (need <= buf.size()) return;
        sync();
        buf.alloc(grown);
    }
    template <typename Buf> void grow(Buf& buf, uint64_t need) { grow(buf, need, need + need / 4); }
    // what the kernels of subsample.hip make a compacted block from: per kept read its first base in the old block (d_src: packed blocks,
    // d_table: text), and the listed positions' per-chunk counts with their scan
    struct CompactScratch {
        DeviceBuffer<uint64_t> d_src;
        DeviceBuffer<dev::GatherEntry> d_table;
        DeviceBuffer<uint32_t> d_count, d_prefix;
        DeviceBuffer<unsigned char> d_ntemp;
    };
    void compact_room(CompactScratch& cs, bool packed, uint64_t n_kept, uint64_t n_npos); // room for such a block
    struct BlockRoom { // where a block goes
        uint8_t* bases;
        uint64_t *offsets, *npos;
    };
    // The one compaction by flag / rank / boff (resident.cpp): block `sb` of `src`, in either form, to where `room` says once it is told how
    // many listed positions the kept reads hold (counted first: one 4-byte read-back on `stream`, none for a source without any).  Then
    // tables, pack or gather, emit on `stream`; *d_err (zeroed by the caller) is the caller's to read back.  Returns the new block.
    DeviceBatch compact_block(const dev::SubsampleBlock& sb, const DeviceBatch& src, CompactScratch& cs, uint32_t* d_err, hipStream_t stream,
        const std::function<BlockRoom(uint64_t n_list)>& room);
    // what the read filter of one block needs beside the block: the quality bytes, the per-read words of read_qual.hip, and -- for a block
    // that loses reads and is not kept -- the compacted block with the tables the kernels of subsample.hip make it from
    struct FilterScratch {
        DeviceBuffer<uint8_t> d_qual, d_flag;
        DeviceBuffer<unsigned long long> d_qsum, d_work;
        DeviceBuffer<uint32_t> d_flag32, d_rank;
        DeviceBuffer<uint64_t> d_klen, d_boff;
        DeviceBuffer<unsigned char> d_temp;
        PinnedBuffer<unsigned long long> h_out;
        CompactScratch comp;
        DeviceBuffer<uint8_t> c_bases;
        DeviceBuffer<uint64_t> c_offsets, c_npos;
        // read trimming: the per-read words of read_trim.hip, and the trimmed block (bases or words, offsets, positions, qualities) that a
        // block which lost a base is replaced by before the filter sees it
        DeviceBuffer<uint32_t> t_first, t_last, t_count, t_prefix;
        DeviceBuffer<uint64_t> t_begin, t_end, t_klen, t_src;
        DeviceBuffer<unsigned long long> t_work;
        DeviceBuffer<unsigned char> t_temp, t_ntemp;
        DeviceBuffer<dev::GatherEntry> t_btable, t_qtable;
        PinnedBuffer<unsigned long long> t_out;
        DeviceBuffer<uint8_t> t_bases, t_qual;
        DeviceBuffer<uint64_t> t_offsets, t_npos;
        // adapter trimming: every read's smallest matching start, and a packed block's bitmap of non-ACGT bases
        DeviceBuffer<uint32_t> t_cut;
        DeviceBuffer<uint16_t> t_nbits;
        // the decoy screen: V and H of every read ([0, n_reads) and [n_reads, 2 n_reads)), and -- the device entry -- its four counts and
        // error word with their pinned mirror
        DeviceBuffer<uint32_t> k_counts;
        DeviceBuffer<unsigned long long> k_work;
        PinnedBuffer<unsigned long long> k_out;
        // the low-complexity filter: D of every read; complexity_device's three words with their pinned mirror
        DeviceBuffer<uint32_t> x_diff;
        DeviceBuffer<unsigned long long> x_work;
        PinnedBuffer<unsigned long long> x_out;
        // base masking: one claim word per read, the counts with their pinned mirror, and -- packed blocks, whose bitmap is t_nbits -- the
        // per-chunk counts of listed positions, their scan and the list behind the mask
        DeviceBuffer<uint32_t> m_rflag, m_count, m_prefix;
        DeviceBuffer<unsigned char> m_temp;
        DeviceBuffer<unsigned long long> m_work;
        PinnedBuffer<unsigned long long> m_out;
        DeviceBuffer<uint64_t> m_npos;
    };
    struct Stage {
        FilterScratch filt;
        DeviceBuffer<uint8_t> d_bases;
        DeviceBuffer<uint64_t> d_offsets, d_npos;
        Event copied;
        // a BAM batch as it arrives: converted into d_bases -- or into the block that stays resident -- by launch_bam_pack
        DeviceBuffer<uint8_t> d_seq, d_reverse;
        DeviceBuffer<uint64_t> d_seq_start;
        BamScratch bam;
    };
    void ensure_bam_scratch(BamScratch& s, uint64_t n_bases);
    // The copies of a BAM batch into st's raw buffers on copy_stream and, behind them on `stream`, its conversion into the packed batch
    // at these addresses, which is returned.  st.copied is recorded behind the copies when the two streams differ.
    DeviceBatch copy_in_bam(const HostBatch& hb, Stage& st, uint8_t* d_words, uint64_t* d_offsets, uint64_t* d_npos, hipStream_t copy_stream, hipStream_t stream);
    // room for the filter of n_reads reads (qual_bytes: 0 without a quality threshold); own_flags / own_sums: the caller has none
    void ensure_filter_scratch(FilterScratch& fs, uint64_t n_reads, uint64_t qual_bytes, bool own_flags, bool own_sums);
    // queues the filter on `stream`; fs.h_out holds dev::RF_* once the stream has been waited for
    // decoy: fs.k_counts holds the screen's V and H of these reads (run_decoy_screen, on the same stream), and the flags see its verdict
    void run_read_filter(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, uint64_t n_reads,
        uint64_t n_bases, unsigned long long* d_sums, uint8_t* d_flags, hipStream_t stream, bool decoy = false, bool complexity = false);
    // D of every read of the batch into fs.x_diff, queued on `stream`, which the flags then hold against f.min_complexity: a packed batch's
    // bitmap (fs.t_nbits) first, unless nbits_ready.  true: fs.t_nbits holds the batch's bitmap afterwards
    bool run_read_complexity(FilterScratch& fs, const uint8_t* d_bases, bool packed, const uint64_t* d_npos, uint64_t n_npos, const uint64_t* d_offsets,
        uint64_t n_reads, uint64_t n_bases, hipStream_t stream, bool nbits_ready = false);
    // room for the trim kernels over n_reads reads (own_ranges: the caller brings no begin / end arrays)
    // adapters: room for the cut words too, and for a bitmap over bitmap_bases packed bases (0: text, or no listed position)
    void ensure_trim_scratch(FilterScratch& fs, uint64_t n_reads, uint64_t n_npos, bool use_qual, bool own_ranges, bool adapters = false, uint64_t bitmap_bases = 0);
    // the bases of a block for adapter_points_kernel; a packed block's bitmap is made on `stream` first (ensure_trim_scratch gave it room)
    dev::AdapterPoints adapter_points(FilterScratch& fs, const uint8_t* d_bases, bool packed, const uint64_t* d_npos, uint64_t n_npos, uint64_t n_bases, hipStream_t stream);
    // queues the trim kernels on `stream`; fs.t_out holds dev::RT_* once the stream has been waited for, fs.t_offsets the new offsets
    void run_read_trim(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, const uint8_t* d_rev,
        uint64_t n_reads, uint64_t n_bases, uint64_t* d_begin, uint64_t* d_end, const uint64_t* d_npos, uint64_t n_npos, hipStream_t stream,
        const dev::AdapterPoints* pts = nullptr);
    // this device's decoy set: the table, its distinct k-mers and the name of the set (0: none)
    struct DecoyTable {
        DeviceBuffer<unsigned long long> table;
        uint64_t distinct = 0, id = 0;
        uint32_t k = 0;
    };
    DecoyTable decoy_;
    dev::DecoySet decoy_set(const ReadFilter& f) const; // what the kernels are told; refuses settings made for another set
    // V and H of every read of the batch into fs.k_counts, queued on `stream`: a packed batch's bitmap (fs.t_nbits) first
    // nbits_ready: fs.t_nbits already holds the batch's bitmap (the mask stage left it): it is not made again
    void run_decoy_screen(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_bases, bool packed, const uint64_t* d_npos, uint64_t n_npos,
        const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, hipStream_t stream, bool nbits_ready = false);
    // Queues the mask on `stream`, in place on these bases: a packed batch's bitmap (fs.t_nbits) is made first and holds the masked
    // positions too afterwards.  fs.m_out holds dev::BM_* once the stream has been waited for.
    void run_base_mask(FilterScratch& fs, const ReadFilter& f, const uint8_t* d_qual, uint32_t bias, const uint64_t* d_offsets, const uint8_t* d_rev,
        uint64_t n_reads, uint64_t n_bases, uint8_t* d_bases, bool packed, const uint64_t* d_npos, uint64_t n_npos, hipStream_t stream);
    // the list of a packed batch behind the mask, n_list positions, into fs.m_npos from the bitmap (queued on `stream`)
    void emit_mask_list(FilterScratch& fs, uint64_t n_bases, uint64_t n_list, hipStream_t stream);
    // read statistics: the two snapshots' accumulators (allocated with the first block that is counted), the per-read words of
    // read_stats.hip, a packed block's bitmap, the quality bytes of a block that goes through map_host_async (two buffers in turn, as the
    // staging sets), the reads of blocks without a base (counted here: such a block is never copied) and the error words' pinned mirror
    struct StatsState {
        DeviceBuffer<unsigned long long> acc[2], gcv, esum;
        DeviceBuffer<uint16_t> nbits;
        DeviceBuffer<uint8_t> qual[2];
        int qual_next = 0;
        uint64_t empty_reads[2] = { 0, 0 };
        PinnedBuffer<unsigned long long> h_err;
        hipStream_t last = nullptr; // the stream the scratch was last used on: another one waits for it first
    };
    StatsState stats_;
    StatsState stats_api_; // read_stats_device's own
    // queues the count of `b` into st.acc[which] on `stream` (d_qual null: without the quality sections)
    void run_read_stats(StatsState& st, int which, const DeviceBatch& b, const uint8_t* d_qual, uint32_t bias, const uint8_t* d_rev, const uint8_t* d_flags,
        uint64_t take, hipStream_t stream);
    // the block's quality bytes into one of stats_.qual, queued on `stream`
    const uint8_t* stats_qual_in(const HostBatch& hb, hipStream_t stream);
    // map_host's and map_host_async's hook: block `b` of `hb`, which is on the device once `stream` gets there, counted as hb.stats_which says
    void count_unfiltered(const HostBatch& hb, const DeviceBatch& b, const uint8_t* d_qual, const uint8_t* d_rev, hipStream_t stream);
    FilterScratch filter_api_; // read_filter_device's and read_trim_device's own (as bam_api_)
    BamScratch bam_api_; // pack_bam_on_device's own (the caller's stream is not ordered with the context's)
    uint64_t bam_blocks_ = 0;
    // room in `st` for a batch of these sizes (n_npos: 0 for an ASCII batch)
    void ensure_stage(Stage& st, uint64_t payload_bytes, uint64_t n_reads, uint64_t n_npos);
    Stage stage_[2], stage_sync_;
    // queues the copies of a host batch to these device addresses (d_npos: used when the batch lists positions) on `stream`; returns the
    // batch they will hold
    DeviceBatch copy_in(const HostBatch& hb, uint8_t* d_bases, uint64_t* d_offsets, uint64_t* d_npos, hipStream_t stream);
    // either of the two: a BAM block through st's raw buffers (copy_in_bam), any other straight to the addresses (st may be null then)
    DeviceBatch copy_block_in(const HostBatch& hb, Stage* st, uint8_t* d_bases, uint64_t* d_offsets, uint64_t* d_npos, hipStream_t copy_stream, hipStream_t stream);
    DeviceBatch copy_to_stage(const HostBatch& hb, Stage& st, hipStream_t copy_stream, hipStream_t stream); // into st's own buffers, given room first
    hipStream_t copy_stream(); // (created with the first call)
    // The two sets of the asynchronous paths, taken in turn: the batch that used a set two calls ago was completed by the previous call (a
    // deferred map completes the batch before the one it queues), so the set is free.  A block that took a set and ends without a map call
    // hands it back: nothing has completed the batch in flight, whose kernels read the OTHER set, so the next block must take this one
    // again -- were the turn kept, its copies would overwrite what the batch in flight is still reading.
    Stage& next_stage();
    void hand_back_stage() { stage_next_ ^= 1; }
    int stage_next_ = 0;
    // reads that are counted and go nowhere (empty reads only): the counters see them, and under keep_reads they are numbered
    void count_unmapped(uint64_t n, bool keeping);
    // a block of such reads in front of the filter: the lower bound decides, there is nothing to copy and nothing to map
    void only_empty_reads(uint64_t n_reads, const ReadFilter& f, bool keeping, FilterOutcome& o);
    // what the *_device entries begin with alike: the device made current, the refusals, the stream to use (null: the context's own)
    hipStream_t device_entry(hipStream_t stream, bool null_pointer, uint64_t n_reads);
    // the steps of map_host_filtered behind the copy (read_prep.cpp), in their order
    struct KeptPart { // the block's first `take` reads hold the n_reads reads and n_bases bases that go on
        uint64_t take, n_reads, n_bases;
    };
    bool trim_block(const HostBatch& hb, const ReadFilter& f, Stage& st, DeviceBatch& src, const uint8_t*& d_qual, uint32_t& trim_err, FilterOutcome& o);
    // mask_block queues the mask in place on the block the trim stage left; its counts come with filter_block's read-back, which hands
    // them to mask_done: the outcome, the refusals, and -- a packed block whose list changed -- `src`'s list REPLACED by the one behind the mask
    void mask_block(const HostBatch& hb, const ReadFilter& f, Stage& st, const DeviceBatch& src, const uint8_t* d_qual);
    void mask_done(const HostBatch& hb, Stage& st, DeviceBatch& src, FilterOutcome& o);
    void filter_block(const HostBatch& hb, const ReadFilter& f, FilterScratch& fs, const DeviceBatch& src, const uint8_t* d_qual, const uint32_t& trim_err,
        FilterOutcome& o);
    KeptPart cut_at_cap(FilterScratch& fs, uint64_t n_reads, uint64_t cap_need, FilterOutcome& o);
    DeviceBatch place_block(FilterScratch& fs, const DeviceBatch& src, const KeptPart& k, bool& keeping);
    // sketch_filter_kernel's tile shares, followed from batch to batch ([0] ASCII, [1] packed input; {0}: the launcher's built-in ones so far)
    uint32_t ft_share_[2][4] = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 } };
    uint64_t ft_last_[20] = {};
    void tune_filter_shares(const Lane& lane, bool packed, uint64_t n_bases);
    // keep_reads: the resident sample.  Device memory in large pieces (arenas), handed out front to back, at most `cap` bytes of it.
    struct ResidentSet {
        std::vector<DeviceBuffer<uint8_t>> arenas;
        uint8_t* at = nullptr; // the bump pointer into the last arena
        size_t left = 0;       // what is left behind it
        uint64_t cap = 0, bytes = 0; // (cap == 0: nothing is kept)
        std::vector<DeviceBatch> kept;
        // the reads of the sample are numbered in the order they were kept: first[b] = number of kept[b]'s first read, seen = reads numbered
        // so far (a block of empty reads only is not kept, but its reads are numbered)
        std::vector<uint64_t> first;
        uint64_t seen = 0;
        bool broken = false; // reads were mapped that are not among kept
        bool active() const { return cap > 0 && !broken; }
        // room for a block: payload_bytes (and 64 more, which the caller clears) of bases, n_reads + 1 offsets, n_npos listed positions
        // (npos null without any) -- or nothing, when the cap or the device says no
        std::optional<BlockRoom> take_block(uint64_t payload_bytes, uint64_t n_reads, uint64_t n_npos);
        void add(const DeviceBatch& b, uint64_t n_reads) { kept.push_back(b); first.push_back(seen); seen += n_reads; }
        uint64_t* take_list(uint64_t n_npos) { return static_cast<uint64_t*>(arena_take(n_npos * sizeof(uint64_t))); } // (mate merging: a block's list, sized behind its words)
        uint32_t* take_numbers(uint64_t n_reads) { return static_cast<uint32_t*>(arena_take(n_reads * sizeof(uint32_t))); } // (mate overlap: a block's source numbers)
        void count_empty(uint64_t n) { seen += n; }
        // everything but the cap goes; the caller has made sure that nothing on the device reads the blocks any more
        void clear() { *this = ResidentSet { {}, nullptr, 0, cap }; }

    private:
        void* arena_take(size_t bytes);
    };
    ResidentSet resident_;
    // a map call on a block of the resident set: the only kind that does not break the set
    bool in_keep_call_ = false;
    void map_resident_block(const DeviceBatch& b);
    Event kept_copied_;
    // what subsample_kept and dedup_kept begin with (the sample is resident, nothing is in flight), and their second half: compaction by the
    // flags into a new set, the kept reads mapped afresh
    SubsampleResult resident_sample(const char* what, std::vector<uint8_t>& flags);
    void keep_flagged(const uint8_t* d_flag, const uint32_t* d_rank, const uint64_t* d_boff, uint32_t* d_err, const char* what, SubsampleResult& res,
        std::vector<uint8_t>& flags);
    // the second half's own tail, which pair_overlap_kept shares: the compaction's error word read back (a set one: the new set is given
    // up), then the new set in the old one's place, coverage and counters cleared, its blocks mapped
    void compaction_clean(uint32_t* d_err, const std::string& what);
    void adopt_kept(ResidentSet& fresh, uint64_t reads_kept);
    // mate overlap: what the blocks of the resident set were numbered with (src[b]: kept[b]'s source numbers, in the set's arenas)
    struct PairState {
        bool record = false;
        std::vector<const uint32_t*> src;
        uint64_t seen[2] = { 0, 0 }; // the reads either side's files held
        int side = 0, begun = 0;     // begin_mates calls
        size_t block2 = 0;           // side 2's first block
        uint64_t n1 = 0;             // and first resident number
        bool spent = false;          // the sample was compacted, or the stage has run: the numbers no longer stand for it
        // duplicate pairs: switched on; what pair_overlap_kept left for it (ready): mate[i] and srcno[i] of resident read i, the source pairs
        bool dedup = false, ready = false;
        uint64_t pairs = 0;
        DeviceBuffer<uint32_t> d_mate, d_srcno;
        void release_record()
        {
            ready = false;
            pairs = 0;
            d_mate.reset();
            d_srcno.reset();
        }
    };
    PairState pair_;
    // the source numbers of a block the resident set has just taken (flag / rank / take: launch_pair_numbers); base: the side's reads in front
    // of the block.  false: the set had no room for them.  The callers fail the block then (-ENOMEM, naming DRPRG_HIP_KEEP_READS_GB) rather
    // than stop keeping: the block's own room is taken from the arenas already, and a paired run needs the resident sample anyway
    bool pair_number_block(uint64_t n_reads, const uint8_t* d_flag, const uint32_t* d_rank, uint64_t src_reads, uint64_t take, uint64_t base, hipStream_t stream);
    struct DedupBlock;
    void dedup_block(const DeviceBatch& kb, DedupBlock& out, unsigned long long* d_count);
    void stop_keeping(); // the resident set given up (over its limit, or the device is full): what map_host_async and map_host_filtered do alike
    DeviceBuffer<uint32_t> d_peer_tmp_; // add_vectors_from: the other device's vectors on this device
    // timing
    bool timing_ = false;
    double sketch_ms_ = 0;
    uint64_t sketch_launches_ = 0;
    Event ev0_, ev1_;
};

} // namespace drprg
