// ingest.h -- multi-threaded FASTA/FASTQ/BAM ingest for the CLI path (NEXT-4).
//
// The kernels map 10 M reads in under 2 ms; end to end the path is bound by text parsing and the host->device copy.
// A plain file is memory-mapped and cut at record boundaries into slices that worker threads parse straight into
// pinned buffers (so the H2D copy runs at DMA speed); gzip input is inflated window by window -- BGZF members in
// parallel with libdeflate, a plain gzip stream by all threads at once (pgunzip.h), a small one in one libdeflate call, anything else by zlib -- and cut the same way.  Read order is irrelevant to the result (coverage is a sum), so workers submit batches independently.
#pragma once
#include "common.h"
#include <functional>

namespace drprg {

struct PinnedBatch {
    uint8_t* bases = nullptr;    // ASCII; packed: the 2-bit words (pack.h), 16 bases per u32
    uint64_t* offsets = nullptr; // offsets[0] == 0 (in bases, whatever the format)
    uint64_t n_reads = 0, n_bases = 0;
    bool packed = false;
    const uint64_t* npos = nullptr; // packed: ascending positions of the bases that are not ACGTacgt (pageable memory)
    uint64_t n_npos = 0;
    // BAM's own form (IngestHooks::bam_native; bam.h): `bases` holds the concatenated 4-bit sequence fields (seq_bytes of them, high
    // nibble first), read i starts at byte seq_start[i], is offsets[i + 1] - offsets[i] bases long and is the reverse complement of its
    // field when reverse[i] != 0.  n_npos counts the codes that are not A, C, G or T; npos is null (the device makes the list).
    bool bam = false;
    const uint64_t* seq_start = nullptr;
    const uint8_t* reverse = nullptr;
    uint64_t seq_bytes = 0;
    // IngestHooks::want_qual: the reads' quality bytes as the file holds them, n_bases of them, those of read i from byte offsets[i] on --
    // indexed in bases in all three forms -- and what to take off a byte to get the Phred quality: 33 (FASTQ text) or 0 (BAM's QUAL field,
    // in the record's order whatever its flag says)
    const uint8_t* qual = nullptr;
    uint32_t qual_bias = 0;
};

struct IngestHooks {
    std::function<void*(size_t)> alloc;            // pinned allocation (falls back to malloc when null)
    std::function<void(void*)> release;
    std::function<void(const PinnedBatch&)> submit; // called by one thread at a time ...
    bool concurrent_submit = false;                 // ... unless set: then by any parser thread, and submit does its own locking
    bool packed = false;                            // the parser threads pack the bases to 2 bits as they copy them (pack.h): a block is a
                                                    // quarter of the bytes to page-lock and to move over PCIe
    // When set, it replaces submit: the blocks are handed over one at a time IN FILE ORDER (a block then never spans two slices of the
    // text, and a parser thread waits with a full block until the slices before its own are through).  false: stop -- nothing more is
    // handed over, the parser threads take no new slices and the rest of the file is not read.  For callers whose result depends on
    // which reads come first (the depth cap, drprg_hip_set_max_covg); everything else keeps the unordered hand-over.
    std::function<bool(const PinnedBatch&)> submit_in_order;
    // A BAM file's reads are handed over in BAM's 4-bit form (PinnedBatch::bam; `packed` does not apply to them).  false: the parser
    // threads convert them to upper-case text, and the hooks see the ASCII (or packed) blocks the FASTQ of the same reads would give.
    bool bam_native = false;
    // The blocks carry the reads' quality bytes (PinnedBatch::qual): the parser threads copy the quality line or the QUAL field beside the
    // bases without looking at the bytes.  A read of one base or more that has none -- a FASTA record, a BAM record whose QUAL field starts
    // with 0xFF -- ends the call with DRPRG_EINVAL.  false: nothing about the ingest changes, no quality byte is parsed, copied or moved.
    bool want_qual = false;
    const char* qual_flag = "--min-read-qual"; // the setting that asked for the qualities: named in that error (the read filter's, or --trim-qual)
};

struct IngestStats {
    uint64_t reads = 0, bases = 0, batches = 0;
    uint64_t discarded_reads = 0; // submit_in_order said stop: reads the parser threads had in blocks that were never handed over
    bool parallel = false;
    int gz_mode = 0; // 0 plain text, 1 BGZF (members inflated in parallel), 2 one gzip member in one libdeflate call, 3 zlib streaming,
                     // 4 one plain gzip stream inflated by all threads (pgunzip.h)
    // BAM input (bam.h): records seen, records skipped (secondary / supplementary), reads that were reverse-complemented
    bool bam = false;
    uint64_t bam_records = 0, bam_skipped = 0, bam_reversed = 0;
};

// Parses `path` (fasta/fastq, plain or .gz; or BAM) with `threads` parser threads and feeds every batch to hooks.submit.
// Throws Error on malformed input.
IngestStats ingest_fastx(const std::string& path, int threads, const IngestHooks& hooks);

} // namespace drprg
