/*
 * drprg_hip.h -- C ABI of the MI355X-native drprg predict hot path (libdrprg_hip.so).
 *
 * The reference has no FFI for this path: drprg drives the external `pandora` executable through
 * struct Pandora (/root/reference/src/lib.rs:459-698).  Each entry point below names the reference
 * interface it replaces; a Rust host binds them with `extern "C"` (stub in INTEGRATION.md), or keeps
 * using the process boundary through the drop-in executable drprg_amd/bin/pandora (`drprg predict -p`,
 * /root/reference/src/predict.rs:136-144).
 *
 * Conventions: every function returns 0 on success or a negative errno-style code; no exception
 * crosses the ABI; `drprg_hip_last_error` gives the message of the last failure on that context
 * (or, with ctx == NULL, of the last failed open/index call on the calling thread).  A context is
 * not thread-safe.  Buffers passed in stay owned by the caller; nothing returned needs freeing
 * except the context itself (`drprg_hip_close`).  Plain pointers and sizes only.
 */
#ifndef DRPRG_HIP_H
#define DRPRG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct drprg_hip_ctx drprg_hip_ctx;

/* Mapping options = the argv drprg builds for `pandora map/discover`
 * (/root/reference/src/predict.rs:236-245, src/lib.rs:594-618).
 * ZERO-INITIALISE the struct (memset / `= {0}` / Rust `Default`) before setting fields: every field has a default at 0 and new
 * fields are only ever added where 0 keeps the previous behaviour (`binomial` took what was tail padding in round 3:
 * sizeof stayed 48, and a host that filled the struct field by field without zeroing it would pass an indeterminate value).
 * DRPRG_HIP_MAP_OPTS_SIZE is checked by drprg_hip_set_opts_sized, the entry a host built against another header revision
 * should call: a size other than this library's is refused with -EINVAL instead of being read past or short. */
#define DRPRG_HIP_MAP_OPTS_SIZE 48
typedef struct drprg_hip_map_opts {
    int32_t max_diff;          /* --max-diff; <=0: default (250, or 2k+1 with illumina) */
    double error_rate;         /* -e; <=0: default (0.11, or 0.001 with illumina) */
    uint32_t min_cluster_size; /* -c (drprg passes 10) */
    int32_t illumina;          /* -I */
    uint64_t genome_size;      /* -g (drprg passes 4411532) */
    double genotyping_error_rate; /* <=0: 0.01 */
    int32_t kernel;            /* 0 auto (2 when it applies, else 3); 1 direct sketch kernel + generic cluster pipeline (radix sort);
                                * 2 Bloom-prefiltered kernel (k<=15, w<=16, small index); 3 direct sketch kernel, candidate form */
    int32_t binomial;          /* --bin: binomial model of the k-mer coverages (pandora's default, and what drprg runs, is the negative
                                * binomial: the argv of /root/reference/src/lib.rs:594-618 has no --bin) */
} drprg_hip_map_opts;

/* Replaces Pandora::index_with (`pandora index -t T -w W -k K <prg>`, /root/reference/src/lib.rs:479-510):
 * writes <prg>.k<K>.w<W>.idx and <dir>/kmer_prgs/ beside the PRG (/root/reference/src/builder.rs:263-269).
 * Host-only work; needs no GPU. */
int drprg_hip_index(const char* prg_file, int w, int k, int threads);

/* Opens the index that drprg_hip_index wrote (the files `validate_index` requires,
 * /root/reference/src/predict.rs:400-418) and uploads its probe tables to HIP device `device`.
 * device < 0 opens a host-only context: index export and genotyping work, every map call fails with
 * -ENODEV (there is no CPU fallback for the hot path).  Returns NULL on failure. */
drprg_hip_ctx* drprg_hip_open(const char* prg_file, int w, int k, int device);
/* Why the last drprg_hip_open / _open_prg / _open_multi of the calling thread returned NULL (a negative errno-style code; 0 if it did
 * not): -EINVAL for a (w, k) outside 1 <= k <= 31, 1 <= w <= 1024 -- the range every part of the library serves, drprg_hip_index and a
 * host-only context included.  drprg_hip_last_error(NULL) has the message. */
int drprg_hip_open_error(void);

/* Same, but sketches the PRG in memory instead of reading .idx / kmer_prgs (no files needed or written). */
drprg_hip_ctx* drprg_hip_open_prg(const char* prg_file, int w, int k, int device, int threads);

/* One context over several HIP devices of a node (the reference is single-process): the index tables
 * are replicated on every device, drprg_hip_map_fastx shards the reads by ingest block over the devices and sums their coverage
 * vectors into devices[0] before it returns (unsigned integer sums: the result is the same whatever device mapped what), so
 * coverage / counters / genotype then see the whole sample.  Every other call (map_host, map_device, device_coverage) uses
 * devices[0].  from_files != 0: like drprg_hip_open, else like drprg_hip_open_prg.  A device may be listed more than once
 * (two concurrent launch sequences on one GPU: what the single-GPU test uses). */
drprg_hip_ctx* drprg_hip_open_multi(const char* prg_file, int w, int k, const int* devices, int ndev, int from_files);

/* ---- the one collective of the path: the sum of the per-GPU coverage vectors (BASELINE north_star "a single
 * RCCL reduce over xGMI").  The reference is single-process and has no counterpart; what these calls feed is the genotyping
 * that follows `pandora map`'s read loop (/root/reference/src/lib.rs:580-642).  RCCL is bound at run time (librccl.so.1):
 * a host that never reduces across GPUs does not need the library.
 *
 * Layout A, one process over several GPUs (drprg_hip_open_multi): drprg_hip_reduce sums the devices' vectors into devices[0]
 * on the devices -- one ncclReduce(sum, u32) over a communicator of the context's devices, or, when a device is listed twice
 * / RCCL is absent / DRPRG_HIP_NO_RCCL=1, a peer copy + add kernel per device -- clears the other devices and folds their
 * counters.  drprg_hip_map_fastx calls it before it returns.  drprg_hip_reduce_info: which of the two ran last. */
int drprg_hip_reduce(drprg_hip_ctx* ctx);
int drprg_hip_reduce_info(const drprg_hip_ctx* ctx, char* out, size_t cap);
/* Layout B, one process per GPU (what `north_star` describes and bench.py --gpus N runs): rank 0 makes an id
 * (drprg_hip_comm_unique_id, 128 bytes) and hands it to the other ranks by whatever channel the host has; every rank calls
 * drprg_hip_comm_init_rank(&comm, nranks, id, rank, device) and, after its last batch, drprg_hip_allreduce(ctx, comm, ...):
 * ONE in-place ncclAllReduce(sum, u32) over the vector [coverage | reads per PRG] (n_covg + n_prgs words of
 * drprg_hip_coverage_size) on `hip_stream` (NULL: the context's stream), asynchronous on that stream -- every rank then holds the
 * sample's vectors and rank 0 genotypes.  d_covg NULL: the context's own accumulators (which are laid out that way; a batch
 * still queued by drprg_hip_map_device_async is completed first).  d_covg given: d_prg_reads == d_covg + n_covg takes the same
 * single call, anything else two calls in one group; the CALLER orders the reduce behind the batch that filled the buffers -- except the batch
 * still queued by drprg_hip_map_device_async INTO these buffers, which the reduce completes first (it may still need the host).  `comm` is an ncclComm_t: a host that already has one (its own RCCL binding) may pass it. */
int drprg_hip_comm_unique_id(uint8_t id[128]);
int drprg_hip_comm_init_rank(void** comm, int nranks, const uint8_t id[128], int rank, int device);
int drprg_hip_comm_destroy(void* comm);
int drprg_hip_allreduce(drprg_hip_ctx* ctx, void* comm, void* d_covg, void* d_prg_reads, void* hip_stream);

void drprg_hip_close(drprg_hip_ctx* ctx);
const char* drprg_hip_last_error(const drprg_hip_ctx* ctx);
/* Always 0: there is one build of the library.  (It returned 1 for a measurement build that also held the kernel forms which lost their
 * measurement; those forms were deleted.)  Nothing of the reference corresponds to it (test infrastructure). */
int drprg_hip_experimental(void);

int drprg_hip_set_opts(drprg_hip_ctx* ctx, const drprg_hip_map_opts* opts);
/* The same with the caller's sizeof(drprg_hip_map_opts): -EINVAL when it differs from this library's (header / library mismatch). */
int drprg_hip_set_opts_sized(drprg_hip_ctx* ctx, const drprg_hip_map_opts* opts, size_t opts_size);

/* Read mapping: the loop inside `pandora map` / `pandora discover` that
 * Pandora::genotype_with / discover_with wait on (/root/reference/src/lib.rs:580-642, :513-578).
 * Coverage accumulates in the context until drprg_hip_reset. */
int drprg_hip_map_fastx(drprg_hip_ctx* ctx, const char* reads_path); /* fasta/fastq, plain or .gz; or BAM ("BAM input" below) */
/* Parser threads used by drprg_hip_map_fastx (the -t that drprg forwards to pandora, /root/reference/src/predict.rs:236-245);
 * default 4.  The file is cut at record boundaries and parsed in parallel into pinned blocks. */
int drprg_hip_set_threads(drprg_hip_ctx* ctx, int threads);

/* Depth cap: `pandora map --max-covg`.  pandora takes the reads in file order, adds each read's length to a running total and stops
 * after the first read for which total / genome_size > max_covg (integer division) [UPSTREAM-MEMORY: pandora's source is not under
 * /root/reference and drprg always passes 4294967295, so nothing there pins this rule].  Restated: with T = (max_covg + 1) * genome_size
 * and B(i) the bases of the first i reads mapped on this context since the last drprg_hip_reset -- over all calls and all entry points,
 * host, device, packed and map_fastx --, the accepted reads are the first n, n the smallest i with B(i) >= T (all reads if there is no
 * such i).  What follows read n is neither mapped nor counted: not in the counters' reads and bases, not in the total the genotyper's
 * expected depth is taken from.  Zero-length reads follow the same rule (they can never be the cut themselves).  Once the cap has been
 * reached every further map call returns 0 and maps nothing, until drprg_hip_reset: that clears the running total and keeps the cap.
 *   drprg_hip_set_max_covg: the default is off, and so is any max_covg >= 4294967295 (what drprg passes).  genome_size is the one of
 *     the map options in force.  Set after reads were mapped, it applies from the current running total.
 *   A device batch that cannot reach the cap (running total + n_bases < T) costs nothing extra: no launch, no synchronisation.  The one
 *     batch that crosses it is cut on the device (covg_cut.hip): the call completes a batch still in flight from the async form, waits
 *     for that one small kernel and maps the prefix.  drprg_hip_map_fastx hands its blocks over in file order while a cap is set; at the
 *     cut it copies nothing further to a device and its parser and inflate threads take no new piece of the file -- a plain file, a BGZF
 *     file and a gzip stream are not read to their end (up to one 8 MB / 32 MB piece per parser thread is already under way and is
 *     dropped); only a small single-member .gz, which is inflated by one library call before the first read is parsed, is still inflated
 *     whole.  Only the accepted reads stay resident (drprg_hip_keep_reads); drprg_hip_discover_reads then sees exactly the reads that
 *     were mapped, from HBM or from the file.  A call that is refused (bad pointers, ...) changes nothing of the cap's state.  A context over several devices counts where the blocks are handed
 *     to the devices: the summed vector does not depend on which device mapped what.
 *   drprg_hip_max_covg_info: out[0] = 1 if the cap was reached, out[1] = reads accepted, out[2] = bases accepted, out[3] = reads that
 *     were offered and dropped (map_fastx: the reads parsed before the ingest stopped, not the rest of the file).  Synchronises.
 *   The cap is per context.  Nothing coordinates it across the one-process-per-GPU layout: a caller who shards the reads of a sample
 *     over ranks shards the cap, and each rank stops at its own T. */
int drprg_hip_set_max_covg(drprg_hip_ctx* ctx, uint64_t max_covg);
int drprg_hip_max_covg_info(drprg_hip_ctx* ctx, uint64_t out[4]);
/* Host-only self-check of that ingest: parses the file with `threads` parser threads and returns
 * out[0..4] = reads, bases, order-independent digest (sum of the FNV-1a hashes of the reads), batches, and how gzip input
 * was inflated (0 plain text, 1 BGZF members in parallel, 2 one member in one libdeflate call, 3 zlib streaming, 4 one plain
 * gzip stream inflated by all threads: chunks entered at block boundaries found in the compressed data, csrc/pgunzip.h).
 * A BAM file ("BAM input" below; its BGZF members are inflated as way 1, or by zlib where libdeflate is missing) is turned into the
 * upper-case text of its reads on the parser threads: reads, bases and digest are those of the FASTQ of the same reads. */
int drprg_hip_parse_fastx(const char* reads_path, int threads, uint64_t out[5], char* err, size_t err_len);
/* The same for the hand-over in file order that the depth cap uses: the blocks are taken one at a time, in file order, until max_reads
 * reads have been seen (the last block is cut there), then the ingest is told to stop.  out[0..5] = reads seen, their bases, an
 * order-DEPENDENT digest (sum over the reads of (index + 1) x FNV-1a of the read, index counted from 0 in file order), blocks handed
 * over, how gzip input was inflated (as above), reads the parser threads had in blocks that were never handed over. */
int drprg_hip_parse_fastx_ordered(const char* reads_path, int threads, uint64_t max_reads, uint64_t out[6], char* err, size_t err_len);
/* Host-only self-check of way 4 on any gzip file (not only FASTQ): inflates gz_path with `threads` threads and chunks of
 * chunk_bytes compressed bytes (0 = automatic) into out_path; out[0..2] = bytes written, chunks accepted as their threads
 * inflated them, chunks inflated again from the known position.  Member CRC-32s and lengths are checked as gzip does. */
int drprg_hip_gunzip_file(const char* gz_path, int threads, uint64_t chunk_bytes, const char* out_path, uint64_t out[3], char* err, size_t err_len);
int drprg_hip_map_host(drprg_hip_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads);
/* Batch already resident in HBM.  d_bases: ASCII bases of all reads back to back, 16-byte aligned;
 * d_offsets: u64[n_reads+1], d_offsets[0] == 0, d_offsets[n_reads] == n_bases.  d_covg (u32[2*n_knodes]) and
 * d_prg_reads (u32[n_prgs]) may be NULL to use the context's accumulators; hip_stream may be NULL.
 * Stream rule of every call that takes device buffers (map_device*, map_device_packed*, pack_device, allreduce): the work is queued on
 * hip_stream, or -- NULL -- on the context's own stream, which does NOT wait for the legacy default stream or anybody else's.  Whatever
 * produced the buffers must be complete on that stream: a producer on another stream (a framework's, say) is synchronised by the caller first. */
int drprg_hip_map_device(drprg_hip_ctx* ctx, const void* d_bases, const void* d_offsets, uint64_t n_reads,
    uint64_t n_bases, void* d_covg, void* d_prg_reads, void* hip_stream);
/* The same without the host waiting for the batch: the launch sequence is queued and the call returns; the read-back the
 * sequence ends with (overflow flags, reads left to the generic pipeline, counters) is looked at while the NEXT batch runs
 * -- by the next call, by drprg_hip_sync, or by anything that reads results -- so back-to-back batches leave no gap on the
 * device.  The buffers of a batch (bases, offsets, accumulators) stay valid and unchanged until the call after the next
 * one returns or drprg_hip_sync does; from then on the batch is done on the device as well (its accumulators may be read or
 * reused from any stream).  An error of a batch is reported by the call that completes it. */
int drprg_hip_map_device_async(drprg_hip_ctx* ctx, const void* d_bases, const void* d_offsets, uint64_t n_reads,
    uint64_t n_bases, void* d_covg, void* d_prg_reads, void* hip_stream);
int drprg_hip_sync(drprg_hip_ctx* ctx); /* completes the batch in flight and waits for its stream */

/* ---- 2-bit packed reads: a second input format (SURVEY.md section 8f NEXT-4 "optional 2-bit packing"; the reference takes any fasta /
 * fastq, /root/reference/src/predict.rs:166-170 -- this is about what crosses PCIe and what the streaming kernel reads, a quarter of the
 * bytes).  Base i of a batch is bits [2 (i & 15) + 1 : 2 (i & 15)] of u32 word i >> 4; the letter is bits 2:1 of the base's ASCII
 * code (A 0, C 1, T 2, G 3, either case -- and of any other byte too); npos lists, ascending, the positions of the bases that are
 * not one of ACGTacgt (they invalidate every k-mer that holds them, as in the ASCII form).  Offsets stay u64[n_reads + 1] in BASES.
 * Results are identical to the ASCII form's, bit for bit (the parity suite runs every case through both).
 *   drprg_hip_set_input_format(ctx, 1): drprg_hip_map_fastx packs on its parser threads (0: ASCII blocks, the default).
 *   drprg_hip_pack_reads: host helper, bases[n_bases] -> words[ceil(n_bases / 16)] + npos (-EOVERFLOW, *n_npos set, when npos_cap is
 *     too small).
 *   drprg_hip_map_host_packed / drprg_hip_map_device_packed(_async): the packed counterparts of map_host / map_device(_async); d_words
 *     16-byte aligned like d_bases (the kernels read them with 16-byte loads; -EINVAL otherwise), d_npos may be NULL when n_npos == 0.
 *   drprg_hip_pack_device: the same conversion for a batch that is already on the device (harnesses); d_npos: room for npos_cap
 *     positions, *n_npos receives their number (positions ascending); d_npos NULL: -EINVAL if the batch holds a base that is not ACGT. */
int drprg_hip_set_input_format(drprg_hip_ctx* ctx, int packed);
int drprg_hip_pack_reads(const uint8_t* bases, uint64_t n_bases, uint32_t* words, uint64_t* npos, uint64_t npos_cap, uint64_t* n_npos);
int drprg_hip_map_host_packed(drprg_hip_ctx* ctx, const uint32_t* words, const uint64_t* offsets, uint64_t n_reads, const uint64_t* npos, uint64_t n_npos);
int drprg_hip_map_device_packed(drprg_hip_ctx* ctx, const void* d_words, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void* d_npos,
    uint64_t n_npos, void* d_covg, void* d_prg_reads, void* hip_stream);
int drprg_hip_map_device_packed_async(drprg_hip_ctx* ctx, const void* d_words, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void* d_npos,
    uint64_t n_npos, void* d_covg, void* d_prg_reads, void* hip_stream);
int drprg_hip_pack_device(drprg_hip_ctx* ctx, const void* d_bases, uint64_t n_bases, void* d_words, void* d_npos, uint64_t npos_cap, uint64_t* n_npos,
    void* hip_stream);

/* ---- BAM input.  THIS BUILD'S OWN RULE: the reference's reader (needletail) refuses BAM, so nothing under /root/reference pins what a
 * BAM file means as reads.  The rule below restates FROM MEMORY what `samtools fastq` does by default; samtools was not at hand to
 * check it against.  drprg_hip_map_fastx, drprg_hip_parse_fastx, drprg_hip_parse_fastx_ordered and drprg_hip_discover_reads take a BAM
 * path wherever they take a FASTA / FASTQ path; no other input changes its meaning.
 *   1. A file is BAM if it is BGZF (gzip members that carry the BC extra subfield) and the inflated stream starts with "BAM\1".  A
 *      bgzip'd FASTQ stays what it was.  The header text and the reference list are skipped; a missing 28-byte EOF block is accepted.
 *   2. Records are read in file order.  A record with flag 0x100 (secondary) or 0x800 (supplementary) is skipped and counted as
 *      skipped; every other record is one read, whatever its paired, QC-fail and duplicate flags say.  l_seq == 0: a read of length 0.
 *   3. The read's bases are its SEQ field -- code i of "=ACMGRSVTWYHKDBN" per base, high nibble first --, reverse-complemented when
 *      flag 0x10 is set.  The complement of a code is the code with its four bits reversed (A=1 <-> T=8, C=2 <-> G=4, M <-> K, R <-> Y,
 *      ...; '=', S, W and N map to themselves).
 *   4. Codes A, C, G, T are bases.  Every other code is a non-ACGT position: it invalidates every k-mer that holds it, as an N byte of
 *      a FASTQ does, and its 2-bit letter in the packed form is bits 2:1 of the ASCII code of its upper-case letter.  So the words and
 *      the position list of a BAM batch are bit-identical to drprg_hip_pack_reads of the upper-case text of the same reads.
 *   5. Qualities, names, CIGAR, tags and alignment coordinates are ignored.
 *   6. A read longer than 2^23 bases is refused (-EOVERFLOW), as everywhere else.
 *   7. Malformed input is an error, never a crash or a silently shorter sample.  -84 (EFORMAT): a block_size smaller than the fixed part
 *      + name + cigar + seq + qual, a record that runs past the end of the stream, a wrong magic behind BGZF.
 * A BAM file's reads always travel to the device in their 4-bit form (half the bytes of the text) and are converted there to the packed
 * form above (csrc/bam_pack.hip): drprg_hip_set_input_format does not apply to them.  Blocks that stay resident (drprg_hip_keep_reads)
 * are kept packed, so everything behind -- drprg_hip_select_reads, drprg_hip_map_resident, the discover pass from HBM, the depth cap --
 * sees an ordinary packed batch; drprg_hip_resident_info counts packed bytes.  Multi-line FASTQ's serial reader never sees a BAM file.
 *   drprg_hip_pack_device_bam: the device counterpart of drprg_hip_pack_device for a batch whose sequences are in that 4-bit form.
 *     d_seq: the sequence fields; d_seq_start: u64[n_reads], the byte of d_seq at which read i's field starts (the fields need not be
 *     adjacent or in order); d_offsets: u64[n_reads + 1] in bases, as for every batch; d_reverse: u8[n_reads], != 0: the read is the
 *     reverse complement of its field (NULL: no read is).  d_words: u32[ceil(n_bases / 16)], written with 16-byte stores when it is
 *     16-byte aligned (what the map entries ask for anyway); d_npos: room for npos_cap positions.  *n_npos receives the number of non-ACGT
 *     positions (below 2^32), the positions come out ascending; more than npos_cap: -EOVERFLOW with *n_npos set and the first npos_cap
 *     positions written; d_npos NULL: -EINVAL if there is any.  Stream rule as above; the call waits for its stream.  The result goes
 *     to drprg_hip_map_device_packed(_async) as it is.
 *   drprg_hip_bam_info: out[0] = BAM records seen by drprg_hip_map_fastx, out[1] = of those skipped as secondary / supplementary,
 *     out[2] = reads that were reverse-complemented, out[3] = blocks converted on the device(s); since the last drprg_hip_reset, all 0
 *     for a context that never saw a BAM file.  Under a depth cap the first three count what was parsed before the ingest stopped. */
int drprg_hip_pack_device_bam(drprg_hip_ctx* ctx, const void* d_seq, const void* d_seq_start, const void* d_offsets, const void* d_reverse /* may be NULL */,
    uint64_t n_reads, uint64_t n_bases, void* d_words, void* d_npos, uint64_t npos_cap, uint64_t* n_npos, void* hip_stream);
int drprg_hip_bam_info(drprg_hip_ctx* ctx, uint64_t out[4]);

/* The per-k-mer-node coverage vector (what gets sum-reduced across GPUs):
 * covg[2g] forward, covg[2g+1] reverse coverage of global k-mer node g; prg_reads[p] clusters on PRG p. */
int drprg_hip_coverage_size(const drprg_hip_ctx* ctx, uint64_t* n_covg, uint64_t* n_prgs);
int drprg_hip_coverage(drprg_hip_ctx* ctx, uint32_t* covg, uint64_t n_covg, uint32_t* prg_reads, uint64_t n_prgs);
int drprg_hip_set_coverage(drprg_hip_ctx* ctx, const uint32_t* covg, uint64_t n_covg, const uint32_t* prg_reads,
    uint64_t n_prgs, uint64_t total_bases);
int drprg_hip_device_coverage(drprg_hip_ctx* ctx, void** d_covg, void** d_prg_reads);
int drprg_hip_reset(drprg_hip_ctx* ctx);
/* out[0..7] = reads, bases, minimizers examined (direct kernel: every read minimizer; filtered kernel: those that are
 * index keys), hits, clusters kept, hits kept, sequence in use (1 direct + generic cluster pipeline, 2 Bloom-prefiltered,
 * 3 direct in its candidate form), reads of sequences 2 / 3 that went through the generic cluster pipeline instead of the
 * per-read kernel */
int drprg_hip_counters(drprg_hip_ctx* ctx, uint64_t out[8]);

/* Coverage -> VCF: the tail of `pandora map --genotype --local --vcf-refs <genes.fa>`; writes the file
 * Pandora::vcf_filename names (/root/reference/src/lib.rs:644-646), format of
 * /root/reference/tests/cases/predict/ERR4796933.pandora.vcf. */
int drprg_hip_genotype(drprg_hip_ctx* ctx, const char* vcf_refs, const char* out_vcf, const char* sample);
/* exp_depth_covg / min_kmer_covg / #present / #records of the last drprg_hip_genotype */
int drprg_hip_genotype_info(const drprg_hip_ctx* ctx, uint32_t out[4]);

/* The tail of `pandora discover` (Pandora::discover_with, /root/reference/src/lib.rs:513-578) on the coverage accumulated so
 * far: calls every site, walks the called consensus of every present locus and writes <out_dir>/candidate_regions.tsv (the
 * low-coverage regions pandora would hand to its local assembler), <out_dir>/denovo_paths.txt and denovo_sequences.fa.
 * This entry does not look at the reads again: denovo_paths.txt reports "0 loci with denovo variants" (the format
 * /root/reference/src/lib.rs:648-697 parses); drprg_hip_discover_reads below also finds the novel variants.
 * *n_candidates (may be NULL) receives the number of candidate regions. */
int drprg_hip_discover(drprg_hip_ctx* ctx, const char* vcf_refs, const char* out_dir, const char* sample, uint32_t* n_candidates);
/* drprg_hip_discover + the second half of `pandora discover`: a host-side pass over the reads file piles up, per candidate
 * region, what the reads spell between the exact 15-base anchors either side of it; the most frequent allele that differs
 * from the called consensus (>= 3 reads, >= half of the spanning reads) is a novel variant (with illumina = 0 in
 * the map options the strings are aligned to the consensus and counted column by column: >= 4 reads, >= 60 %).  Writes candidate_regions.tsv, denovo_variants.tsv,
 * denovo_sequences.fa and denovo_paths.txt; list_loci != 0 lists the loci and their variants in denovo_paths.txt in pandora's
 * layout (/root/reference/src/lib.rs:3010-3038) so that the caller's make_prg update runs, 0 keeps "0 loci with denovo
 * variants".  out[0..2] = candidate regions, novel variants, loci with novel variants. */
int drprg_hip_discover_reads(drprg_hip_ctx* ctx, const char* reads_path, const char* vcf_refs, const char* out_dir, const char* sample,
    int list_loci, uint32_t out[3]);
/* Reads that stay in HBM.  The reference reads the sample once per pandora process it spawns -- `pandora discover`
 * (/root/reference/src/predict.rs:248-256), then `pandora map` on the updated PRG (:296-302) -- and pandora discover itself walks
 * the reads twice (mapping, then local assembly).  A sample is 1-5 GB of bases and the device has 288 GB:
 *   drprg_hip_keep_reads(ctx, max_bytes): from now on drprg_hip_map_fastx leaves every block it copies to the device there, up to
 *     max_bytes per device (0 = off, the default; past the limit everything kept is dropped and later calls read files again).
 *   drprg_hip_discover_reads then finds the reads that hold an anchor k-mer with one kernel over the resident base stream
 *     (anchor_scan.hip) and runs its pile-up on those alone, when every read mapped since the last reset came from ONE
 *     drprg_hip_map_fastx call on the same path; otherwise it reads the file, as before.  Same output either way.
 *   drprg_hip_map_resident(ctx, from): maps the reads `from` keeps against the index of `ctx` (same devices, in the same order;
 *     `from` stays open during the call).  -ENODATA (-61) when `from` does not hold all of its reads: map the file instead.
 *   drprg_hip_resident_info: out[0] = 1 if every read mapped since the last reset is resident, out[1] = bytes kept (all devices),
 *     out[2] = blocks kept, out[3] = 1 if the last drprg_hip_discover_reads took its reads from HBM. */
int drprg_hip_keep_reads(drprg_hip_ctx* ctx, uint64_t max_bytes);
int drprg_hip_map_resident(drprg_hip_ctx* ctx, drprg_hip_ctx* from);
int drprg_hip_resident_info(drprg_hip_ctx* ctx, uint64_t out[4]);
/* ---- Random subsample of the resident sample to a target depth.  THIS BUILD'S OWN RULE, not pandora's: pandora knows only the depth cap
 * above, a prefix of the file, which is a fair sample only of a file in random order (under a cap a coordinate-sorted BAM gives reads
 * from the start of the genome alone).  Workflows subsample at random before they call drprg; this does it on the reads that are
 * already in HBM, instead of one more pass over the file on the host.
 *   The reads of the sample are numbered i = 0 .. n-1 in the order they were mapped since the last drprg_hip_reset: file order, through the
 *   resident blocks and through several drprg_hip_map_fastx calls.  L_i is the length of read i.  Given T = target_bases and a 64-bit seed:
 *     1. sum(L_i) <= T: every read is kept and nothing else happens (coverage, counters and the resident set are untouched).
 *     2. Otherwise key(i) = splitmix64(seed + 0x9E3779B97F4A7C15 * (i + 1)) in 64-bit unsigned arithmetic, where splitmix64(z) is the
 *        usual finaliser: z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31).
 *     3. The reads are ordered by (key, i) ascending and kept in that order up to AND INCLUDING the first read at which the running sum
 *        of lengths reaches T -- the same "up to and including" as the depth cap.  (T = 0: exactly the first read in key order.)
 *     4. The kept reads stay in file order.  Zero-length reads take part like any other read.
 *   The result depends on the reads' order and lengths, T and the seed alone: not on how the ingest cut the file into blocks, not on the
 *   input form (ASCII, packed, BAM), not on the number of parser threads.
 *   drprg_hip_subsample(ctx, target_bases, seed, out): out[0..3] = reads before, bases before, reads kept, bases kept.  When reads are
 *     dropped, every resident block is compacted on the device into a block of its kept reads (csrc/subsample.hip; the peak device memory
 *     of the call is the old set plus the new one), coverage, reads per PRG and the counters are cleared and the kept reads are mapped
 *     afresh: from then on the context -- drprg_hip_coverage, drprg_hip_counters, drprg_hip_genotype, drprg_hip_discover_reads from HBM,
 *     drprg_hip_select_reads, drprg_hip_map_resident, drprg_hip_resident_info -- is that of a context that was given the kept reads
 *     alone, and a second call numbers the kept reads from 0.  Needs every read mapped since the last reset to be resident
 *     (drprg_hip_keep_reads before the first drprg_hip_map_fastx): -ENODATA (-61) otherwise, and the text names DRPRG_HIP_KEEP_READS_GB, the
 *     executables' limit.  -EINVAL for a context over several devices (drprg_hip_open_multi) and for a context with a depth cap set
 *     (drprg_hip_set_max_covg below 4294967295): the two rules are alternatives.  -EOVERFLOW for 2^32 reads or more.  A refused or failed
 *     call leaves the context as it was.
 *   drprg_hip_subsample_flags(ctx, flags, n): flags[i] = 1 if read i (numbering before the call) was kept by the last drprg_hip_subsample
 *     since the last reset, else 0; all ones when nothing was dropped.  -EINVAL unless n is that call's out[0]. */
int drprg_hip_subsample(drprg_hip_ctx* ctx, uint64_t target_bases, uint64_t seed, uint64_t out[4]);
/* drprg_hip_map_fastx normally hands its blocks to the device as its parser threads fill them, in no particular order (coverage is a sum).
 * The numbering above needs them in FILE order: drprg_hip_set_ordered_ingest(ctx, 1) makes drprg_hip_map_fastx hand them over one at a
 * time in file order, the hand-over the depth cap uses, without a cap (0, the default: as before).  A sample of which some file arrived
 * as more than one block without it is refused by drprg_hip_subsample (-EINVAL) rather than numbered by chance; a file that fits one
 * block, and every block under a depth cap, is in order anyway.  The executables switch it on when --subsample-covg is given. */
int drprg_hip_set_ordered_ingest(drprg_hip_ctx* ctx, int on);
int drprg_hip_subsample_flags(drprg_hip_ctx* ctx, uint8_t* flags, uint64_t n);
/* ---- Duplicate reads: exact duplicates dropped from the resident sample, on the device.  THIS BUILD'S OWN RULE (what fastp --dedup,
 * clumpify dedupe and seqkit rmdup -s do in front of drprg, made exact); neither pandora nor drprg has one.  Every copy of a PCR or optical
 * duplicate counts as depth: in the k-mer coverage, in the total bases the expected depth comes from, under --max-covg and in the target
 * of --subsample-covg.
 *   Numbering.  Reads are numbered i = 0 .. n-1 as drprg_hip_subsample numbers them: the order mapped since the last reset, which is file
 *   order, through the resident blocks and through several drprg_hip_map_fastx calls.  This is after the read filter and after a depth cap,
 *   which both act at ingest.
 *   Letters and words.  A base's letter is the packed form's: A/a = 0, C/c = 1, T/t = 2, G/g = 3.  Any other byte, and any BAM code other
 *   than A, C, G, T, is MASKED: letter 0 and a mask bit.  The packed form cannot tell N from R, so neither does the rule.  For a read of
 *   L >= 1 bases and j = 0 .. ceil(L/16) - 1:
 *       v_j = sum over t < 16, 16j+t < L of letter(16j+t) << 2t
 *       m_j = sum over t < 16, 16j+t < L of masked(16j+t) << t
 *       x_j = v_j | (uint64)m_j << 32
 *   Identity.  Two reads are identical iff they have the same L and the same sequence x_0, x_1, ...: the same length, masked bases at the
 *   same places, and the same letters elsewhere, case-insensitively.  It is forward strand only: a read and its reverse complement are
 *   different reads, as for fastp and seqkit rmdup -s -P.  A BAM record with flag 0x10 is compared as the read it becomes, which is
 *   already reverse-complemented.  BAM flag 0x400 stays ignored, as now.
 *   Selection.  Read i is dropped iff some read h < i is identical to it.  The first copy in file order is kept.  Kept reads stay in file
 *   order.  A read of no bases is never a duplicate and never makes one: it is always kept.
 *   The key (not part of the decision, but part of the statement).  fin is the splitmix64 finaliser stated under "random subsample",
 *   G = 0x9E3779B97F4A7C15, and key = fin(G * L) + sum over j of fin(x_j + G * (j + 1)) in 64-bit unsigned arithmetic.  It is a sum, so
 *   pieces of a read computed by different lanes, waves and workgroups add up in any order to the same bits.  L is in the key because
 *   letter 0 is A: without it a read and the same read with a poly-A tail would share a key systematically.  Equal keys never decide
 *   anything.  Identity does.
 *   Invariance.  The result depends on the reads and their order alone.  It does not depend on how ingest cut the file into blocks, on the
 *   input form (ASCII, packed, BAM), on -t, or on key_bits below.
 *   drprg_hip_dedup(ctx, key_bits, out): out[0..3] = reads before, bases before, reads kept, bases kept.  key_bits is in 1..64: how many
 *     low bits of the key the sort sees; 64 is what the executables pass.  The result does not depend on it, as drprg_hip_select_reads'
 *     window_bytes does not change its result; it exists so that the collision path is reachable.  Fewer than two reads with bases, or no
 *     read dropped: nothing else happens (no compaction, no fresh mapping; coverage and counters are untouched).  Otherwise every resident
 *     block is compacted into a block of its kept reads and the kept reads are mapped afresh, as drprg_hip_subsample does it (csrc/dedup.hip,
 *     csrc/subsample.hip): after the call the context is that of one given the kept reads alone, and a following drprg_hip_subsample
 *     numbers the kept reads from 0 -- the pipeline dedupe | rasusa | drprg.  -EINVAL for key_bits outside 1..64, for a context over
 *     several devices and for a sample whose drprg_hip_map_fastx blocks arrived unordered (drprg_hip_set_ordered_ingest); -ENODATA (-61)
 *     unless the sample is resident (the text names DRPRG_HIP_KEEP_READS_GB); -EOVERFLOW for 2^32 reads or more.  A depth cap is NOT
 *     refused: the cap decides at ingest which reads arrive, dedup sees those.  A refused or failed call leaves the context as it was.
 *   drprg_hip_dedup_flags(ctx, flags, n): flags[i] = 1 if read i (numbering before the call) was kept by the last drprg_hip_dedup since
 *     the last reset, else 0; all ones when nothing was dropped.  -EINVAL unless n is that call's out[0].
 *   drprg_hip_dedup_keys_device: the key kernel alone on a caller-owned packed batch, under the stream rule of the other device entries
 *     (NULL: the context's own stream; the call returns when the work is done).  d_words: u32[ceil(n_bases / 16)], read with 16-byte loads
 *     when 16-byte aligned; d_offsets: u64[n_reads + 1] from 0 to n_bases (-EINVAL otherwise); d_npos: the n_npos positions of the masked
 *     bases, in any order (may be NULL when n_npos is 0); d_keys: u64[n_reads], 0 for a read of no bases.  -EOVERFLOW for 2^32 reads or more. */
int drprg_hip_dedup(drprg_hip_ctx* ctx, uint32_t key_bits, uint64_t out[4]);
int drprg_hip_dedup_flags(drprg_hip_ctx* ctx, uint8_t* flags, uint64_t n);
int drprg_hip_dedup_keys_device(drprg_hip_ctx* ctx, const void* d_words, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void* d_npos,
    uint64_t n_npos, void* d_keys, void* hip_stream);
/* ---- Mate overlap: read-through adapters cut off paired reads by the overlap of the two mates, on the resident sample.  THIS BUILD'S OWN
 * RULE, stated from memory of fastp's overlap analysis (its default for paired reads); nothing in pandora or drprg pins it.  It is the one
 * adapter removal that needs no adapter sequence: an insert shorter than the read shows itself in the mates.
 *   Sides and numbers.  Reads mapped before drprg_hip_begin_mates are side 1, reads mapped after it side 2.  A read's SOURCE NUMBER is its
 *   number among the reads of its side as the files held them, counted before any ingest-time stage dropped anything (reads seen, not reads
 *   kept).  Pair s is (read s of side 1, read s of side 2).  Sides that hold different numbers of reads are an error (-84; the text gives
 *   both counts).
 *   Who is judged.  A mate is PRESENT if it is in the resident sample with at least one base after the ingest-time stages.  A pair is judged
 *   iff both mates are present and neither is longer than PO_MAX_LEN = 1024 bases.  Otherwise every present mate passes unchanged, counted as
 *   an orphan (the partner was dropped or has no bases) or under pairs_too_long.  Nothing is ever dropped because its mate was: pandora maps
 *   reads singly, and a good orphan is still coverage.
 *   Comparison.  Letters are those of the packed form, case-insensitive; any other byte, any BAM code other than A, C, G, T and any base
 *   --mask-qual masked is the unknown base.  For mates a (side 1, La bases) and b (side 2, Lb bases) let B[j] = complement(b[Lb-1-j]);
 *   unknown stays unknown.  For every shift d in -(Lb-1) .. La-1 the columns are i = max(0,d) .. min(La, Lb+d)-1, and column i pairs a[i]
 *   with B[i-d].  c(d) is the number of columns where both bases are known, x(d) the number of those where the letters differ; a column with
 *   an unknown base on either side is neither a match nor a difference.
 *   Qualifying and choosing.  d qualifies iff c(d) >= O and 1000 x(d) <= e c(d), in integers; O (min_overlap) is a whole number in 8 .. 1024
 *   (the executables' default: 30), e (error_milli) 1000 times a decimal in [0, 0.25] with at most three places (default 0.05: e = 50).  The
 *   chosen shift has the largest c; among equals the smallest x; among equals the largest d.  No shift qualifies: the pair is unchanged.
 *   Cuts.  Both are prefixes; no base is rewritten and qualities are not needed.  With I = Lb + d (the insert from a's first base to B's
 *   last): a keeps its first min(La, I) bases and b its first min(Lb, I) -- the read-through cut.  With clip set, a keeps min(La, I) and b
 *   keeps max(0, I - La): every column of the molecule then counts once, and a's base stands where the mates differ.  A read cut to nothing
 *   stays a read of no bases, as everywhere else.
 *   Order.  The stage runs on the resident sample, behind the mapping pass and so behind every ingest-time stage, which judge and cut each
 *   mate alone as before; it runs in front of drprg_hip_dedup and drprg_hip_subsample.  The kept reads are compacted and mapped afresh: the
 *   context is then that of a file holding side 1's reads and then side 2's, cut by the rule (fastp -i -I | cat | dedupe | rasusa | drprg),
 *   whatever -t, the block boundaries and the input form.
 *   Limits.  A pair from a tandem repeat can qualify at a shift that is not its true one; largest-c keeps the cut smallest then.  Behind
 *   --trim-front or a 5' adapter cut, b loses the columns a no longer has.  Interleaved files, BAM mate flags, quality-weighted
 *   correction and contexts over several devices are not served (merging mates into one read: "mate merging" below; pair-aware dedup:
 *   "duplicate pairs" below).  No claim
 *   about real samples is made.
 *   drprg_hip_set_pair_overlap(ctx, min_overlap, error_milli, clip): the setting; all zero: off.  -EINVAL outside the ranges above, and with clip
 *     set while mate merging is on ("mate merging" below).  While
 *     it is on, every block the resident set takes from drprg_hip_map_fastx is numbered by side (u32 per read, in the resident arenas), and
 *     drprg_hip_map_host* / drprg_hip_map_device* return -EINVAL.  Off, nothing of this exists: no numbers, no launch, no wait.
 *   drprg_hip_begin_mates(ctx): the files mapped from here on are side 2.  -EINVAL without the setting, over several devices, or when
 *     called twice for one sample.  From here on drprg_hip_discover_reads takes its reads from device memory and returns -ENODATA (-61)
 *     when they are not there (a pass over `reads_path` would see side 1 alone, uncut).
 *   drprg_hip_pair_overlap(ctx, out): the stage.  out[0..11] = pairs, pairs_judged, orphans (present reads without a present partner),
 *     pairs_too_long, pairs_overlapping (judged pairs with a chosen shift), pairs_read_through (of those, pairs in which the read-through
 *     cut took a base), bases_cut (by the read-through cut), bases_clipped (the further bases clip took off b), reads_emptied, reads (of the
 *     resident sample), bases_before, bases_kept.  No read lost a base: nothing else happens (no compaction, no fresh mapping; coverage and
 *     counters untouched).  -EINVAL without the setting, over several devices, while a depth cap is set (the prefix cap would take side 1
 *     alone), for a sample whose blocks arrived unordered (drprg_hip_set_ordered_ingest), without a drprg_hip_begin_mates call, and for a
 *     sample an earlier drprg_hip_pair_overlap, drprg_hip_dedup or drprg_hip_subsample has compacted; -ENODATA (-61) unless the sample is
 *     resident; -84 for sides of different sizes; -EOVERFLOW for 2^32 reads or more.  A refused or failed call leaves the context as it was.
 *     The source numbers are dropped after the stage: a following drprg_hip_dedup or drprg_hip_subsample numbers the reads from 0 as ever.
 *   drprg_hip_pair_overlap_shifts(ctx, d, n): per source pair the shift the last drprg_hip_pair_overlap chose, INT32_MIN when none
 *     qualified, INT32_MIN + 1 when the pair was not judged.  -EINVAL unless n is that call's out[0].
 *   drprg_hip_pair_overlap_info(ctx, out): the twelve counts of the last drprg_hip_pair_overlap since the last reset (all zero: none).
 *   drprg_hip_pair_overlap_device: the two pair kernels alone on two caller-owned packed batches of n_pairs reads each (pair s: read s of
 *     either), under the stream rule of the other device entries.  A side is d_words (u32[ceil(n_bases / 16)]), d_offsets (u64[n_pairs + 1],
 *     ascending inside n_bases; -EINVAL otherwise) and d_npos, the n_npos positions of its unknown bases in any order (may be NULL when
 *     n_npos is 0).  d_shift: i32[n_pairs]; d_keep_a, d_keep_b: u64[n_pairs], the bases either mate keeps; out: the twelve counts.  A mate
 *     of no bases is not present.  -EINVAL without the setting; -EOVERFLOW for 2^31 pairs or more. */
int drprg_hip_set_pair_overlap(drprg_hip_ctx* ctx, uint32_t min_overlap, uint32_t error_milli, int clip);
int drprg_hip_begin_mates(drprg_hip_ctx* ctx);
int drprg_hip_pair_overlap(drprg_hip_ctx* ctx, uint64_t out[12]);
int drprg_hip_pair_overlap_shifts(drprg_hip_ctx* ctx, int32_t* d, uint64_t n);
int drprg_hip_pair_overlap_info(drprg_hip_ctx* ctx, uint64_t out[12]);
int drprg_hip_pair_overlap_device(drprg_hip_ctx* ctx, const void* d_words_a, const void* d_offsets_a, uint64_t n_bases_a, const void* d_npos_a, uint64_t n_npos_a,
    const void* d_words_b, const void* d_offsets_b, uint64_t n_bases_b, const void* d_npos_b, uint64_t n_npos_b, uint64_t n_pairs, void* d_shift, void* d_keep_a,
    void* d_keep_b, uint64_t out[12], void* hip_stream);
/* ---- Mate merging: overlapping mates merged into one read on the resident sample, inside the "mate overlap" stage.  THIS BUILD'S OWN
 * RULE (what fastp -m, PEAR, FLASH and bbmerge are run for); nothing in pandora or drprg pins it.  Everything is in the terms of "mate
 * overlap": a, b, La, Lb, B[j] = complement(b[Lb-1-j]), the chosen shift d, I = Lb + d (1 <= I <= La + Lb - 1).
 *   Who is merged.  A judged pair with a chosen shift.  Every other pair -- no shift qualifies, an orphan, a mate longer than 1024 bases --
 *   passes exactly as under "mate overlap" alone.
 *   The merged read M has I bases, in a's orientation.  Position p (0 <= p < I) is covered by a iff p < La and by B iff p >= d; the
 *   qualifying overlap guarantees that one of them holds.  M[p] is: the base of the one mate that covers p; where both cover p -- both
 *   known and the same letter: that letter; both known and different: the unknown base; exactly one known: the known one; both unknown:
 *   unknown.  The bases of a at p >= I and the bases of B in front of a's first base are read-through adapter and fall away, as in the
 *   read-through cut.  No quality is looked at: a disagreement makes the column unknown, it is never decided.
 *   How M is written.  Upper-case ACGT and N in a block of text; letters and an entry of the unknown list in a packed block (an unknown
 *   base carries letter 3 there, as an N does).  Every merged read is rewritten whole; every other read keeps its bytes.
 *   Where M goes.  M takes a's place in side 1 and b stays in side 2 as a read of no bases: the sample's read count does not change and
 *   nothing is renumbered.  "duplicate pairs" behind the stage sees the unit (M, e), by its own definition of an empty mate.  The context
 *   afterwards is that of a file holding side 1 with every merged a replaced by M, then side 2 with every merged b empty, whatever -t,
 *   the block boundaries and the input form.
 *   Counts.  The twelve counts of "mate overlap" keep their meaning: bases_cut is unchanged; bases_clipped is the number of columns both
 *   mates covered, min(La,I) + min(Lb,I) - I, which is the clip's figure; reads_emptied counts every merged b; bases_kept is the sum of
 *   the new lengths.  The eight counts of this stage: pairs_merged, columns_both (columns both mates covered), columns_agreeing,
 *   columns_disagreeing (made unknown), columns_filled (one known base of two), columns_unknown (unknown in both), bases_merged (the
 *   bases of the merged reads), longest_merged.  The four column kinds add up to columns_both.
 *   Limits.  A column with a disagreement costs every k-mer that holds it (up to k of them; 15 at k = 15), and with e = 50 a merged read
 *   can carry up to 5 % such columns.  A tandem repeat can merge at a wrong shift, as it can be cut at one.  Qualities in the resident
 *   sample, quality-weighted choice of a base, interleaved input, BAM mate flags and several devices are not served.  No claim about real
 *   samples is made.
 *   drprg_hip_set_pair_merge(ctx, on): the switch.  -EINVAL without a mate-overlap setting or while that setting clips (merging subsumes
 *     the clip); while the switch is on, drprg_hip_set_pair_overlap with clip set is -EINVAL too, and switching the setting off switches
 *     this off.  A refused call leaves the context as it was.  On, drprg_hip_pair_overlap merges (csrc/pair_merge.hip): no pair has a
 *     chosen shift: nothing else happens.  Off, nothing of this exists: no launch, no allocation, no wait.
 *   drprg_hip_pair_merge_info(ctx, out): the eight counts of the last drprg_hip_pair_overlap that merged, since the last reset (all
 *     zero: none).
 *   drprg_hip_pair_merge_device: the overlap kernel, then the merge kernel, alone on two caller-owned packed sides given as in
 *     drprg_hip_pair_overlap_device, under the same stream rule.  d_shift: i32[n_pairs].  The merged reads come back as one packed batch
 *     of n_pairs reads in which an unmerged pair is a read of no bases: d_out_offsets (u64[n_pairs + 1]), d_out_words (room for cap_words
 *     words; the bits behind the last base of the last word are clear), d_out_npos (room for cap_npos positions) with *n_out_npos, the
 *     length of the list, ASCENDING.  out12: the twelve counts, out8: the eight.  -EINVAL without the switch; -EOVERFLOW when the words
 *     or the list need more room than given (nothing is written beyond it) and for 2^31 pairs or more. */
int drprg_hip_set_pair_merge(drprg_hip_ctx* ctx, int on);
int drprg_hip_pair_merge_info(drprg_hip_ctx* ctx, uint64_t out[8]);
int drprg_hip_pair_merge_device(drprg_hip_ctx* ctx, const void* d_words_a, const void* d_offsets_a, uint64_t n_bases_a, const void* d_npos_a, uint64_t n_npos_a,
    const void* d_words_b, const void* d_offsets_b, uint64_t n_bases_b, const void* d_npos_b, uint64_t n_npos_b, uint64_t n_pairs, void* d_shift, void* d_out_offsets,
    void* d_out_words, uint64_t cap_words, void* d_out_npos, uint64_t cap_npos, uint64_t* n_out_npos, uint64_t out12[12], uint64_t out8[8], void* hip_stream);
/* ---- Duplicate pairs: exact duplicate read PAIRS dropped from the resident sample, behind "mate overlap".  THIS BUILD'S OWN RULE (what
 * fastp -i -I --dedup, clumpify dedupe on pairs and Picard do in front of drprg: they judge the pair); nothing in pandora or drprg pins it.
 * "duplicate reads" judges every read alone, and two different fragments that start at the same base of the same strand have identical
 * first mates: only their second mates tell them apart.
 *   Units.  Source pair s is the pair of "mate overlap": read s of side 1 and read s of side 2, counted as the files held them.  A_s is the
 *   side-1 read of pair s as it lies in the resident sample when drprg_hip_pair_overlap is done, B_s the side-2 read: both behind every
 *   ingest-time stage, the read-through cut and the clip.  A read that is not in the resident sample (an ingest-time stage dropped it) and
 *   a read of no bases are the same thing: the empty read e.  An orphan is therefore the unit (a, e) or (e, b), and a pair whose second
 *   mate the clip emptied is (a, e) too: it carries the same bases as that orphan and is treated as it.
 *   Identity.  Two units are identical iff A_h is identical to A_s and B_h to B_s by the identity of "duplicate reads": the same length,
 *   masked bases at the same places, the same letters elsewhere, case-insensitively, forward strand only.  e is identical to e and to
 *   nothing else.  (a, b) and (b, a) are different units.
 *   Selection.  Unit s is a duplicate iff at least one of A_s, B_s has bases and some h < s is identical to it.  Every read with bases of
 *   a duplicate unit is dropped: both mates go, or neither.  A read of no bases is always kept, as under "duplicate reads".  Kept reads
 *   stay where they were: side 1 in file order, then side 2.
 *   Copies and levels.  Identity is an equivalence relation; a kept unit with bases is the first of its class, and its copies are the
 *   size of that class.  levels[c-1], c = 1 .. 31, is the number of kept units with exactly c copies, levels[31] the number with 32 or more.
 *   The key (part of the statement, never of the decision).  With ka, kb the content keys of "duplicate reads" (0 for e), fin and G as
 *   there: U = fin(ka + G) + fin(kb + 2G) in 64-bit unsigned arithmetic.  The two constants keep (a, b) and (b, a) apart.  Equal keys
 *   decide nothing.  Identity does.
 *   Invariance.  The result depends on the two files' reads and the settings alone: not on -t, on the block boundaries of either side, on
 *   the input form (ASCII, packed, BAM), or on key_bits.
 *   Limits.  Forward orientation only: the same fragment sequenced from the other strand arrives as (b, a) and is not found.  Exact
 *   identity only: one sequencing error in either mate keeps a copy.  There is no optical-distance rule.  Interleaved files, BAM mate
 *   flags and contexts over several devices are not served, as for "mate overlap".
 *   drprg_hip_set_dedup_pairs(ctx, on): the switch; set it before drprg_hip_pair_overlap.  While it is on, that call keeps the mate and
 *     the source number of every resident read in device memory (8 bytes per read) until this stage, a reset or another compaction
 *     releases them.  Off, nothing is kept and nothing is launched.  -EINVAL without a mate-overlap setting; switching that off switches
 *     this off too.
 *   drprg_hip_dedup_pairs(ctx, key_bits, out): the stage (csrc/pair_dedup.hip).  out[0..7] = units (source pairs), units with bases, units
 *     with both mates (both have bases), units dropped, reads before, bases before, reads kept, bases kept.  key_bits as for
 *     drprg_hip_dedup.  No unit dropped: nothing else happens.  Otherwise the kept reads are compacted and mapped afresh as
 *     drprg_hip_dedup does it, and a following drprg_hip_subsample numbers the kept reads from 0.  -EINVAL for key_bits outside 1..64,
 *     for a context over several devices, without the switch, without a drprg_hip_pair_overlap call on this sample, and for a sample
 *     that drprg_hip_dedup, drprg_hip_subsample or an earlier drprg_hip_dedup_pairs has compacted since (the stage releases its record
 *     when it is done, so a second call on one sample is refused); -ENODATA (-61) unless the sample is resident; -EOVERFLOW for 2^32
 *     reads or pairs or more.  A refused or failed call leaves the context as it was.
 *   drprg_hip_dedup_pairs_flags(ctx, flags, n): one byte per resident read, numbered before the call: 1 kept, 0 dropped; all ones when
 *     nothing was dropped.  -EINVAL unless n is that call's out[4].
 *   drprg_hip_dedup_pairs_info(ctx, out): the eight counts, then the 32 levels, of the last call since the last reset (all zero: none).
 *   drprg_hip_dedup_pairs_device: the stage's kernels alone on two caller-owned packed batches of n_pairs reads each (unit s: read s of
 *     either), the sides given as in drprg_hip_pair_overlap_device, under the stream rule of the other device entries.  d_keys:
 *     u64[n_pairs], U; d_keep: u8[n_pairs], 0 for a duplicate unit; d_copies: u32[n_pairs], the copies of a kept unit with bases, else 0;
 *     out: the eight counts (reads: 2 n_pairs), then the 32 levels.  Needs no setting.  -EOVERFLOW for 2^31 pairs or more. */
int drprg_hip_set_dedup_pairs(drprg_hip_ctx* ctx, int on);
int drprg_hip_dedup_pairs(drprg_hip_ctx* ctx, uint32_t key_bits, uint64_t out[8]);
int drprg_hip_dedup_pairs_flags(drprg_hip_ctx* ctx, uint8_t* flags, uint64_t n);
int drprg_hip_dedup_pairs_info(drprg_hip_ctx* ctx, uint64_t out[40]);
int drprg_hip_dedup_pairs_device(drprg_hip_ctx* ctx, const void* d_words_a, const void* d_offsets_a, uint64_t n_bases_a, const void* d_npos_a, uint64_t n_npos_a,
    const void* d_words_b, const void* d_offsets_b, uint64_t n_bases_b, const void* d_npos_b, uint64_t n_npos_b, uint64_t n_pairs, uint32_t key_bits, void* d_keys,
    void* d_keep, void* d_copies, uint64_t out[40], void* hip_stream);
/* ---- Read filter: reads dropped by length and mean quality on the device, as they arrive.  THIS BUILD'S OWN RULE, stated from memory of
 * what the filters nanopore workflows run in front of drprg compute (nanoq, chopper -q Q -l L, filtlong); neither pandora nor drprg has one.
 *   Settings, per context: min_len (0: no lower bound), max_len (0: no upper bound), min_qual_milli = Q * 1000 (0: no quality test).
 *   A read of L bases with Phred qualities q_0 .. q_{L-1}:
 *     1. Length.  Dropped as SHORT if L < min_len; otherwise dropped as LONG if max_len != 0 and L > max_len.
 *     2. Quality, only if min_qual_milli != 0 and only for a read that passed 1.  E[q] = round(2^31 * 10^(-q / 10)) for q = 0 .. 93, a
 *        literal table of 94 32-bit values (csrc/read_qual_piece.h; E[0] = 2^31, E[93] = 1).  S = sum of E[q_j] in 64 bits (L <= 2^23 keeps
 *        it at or below 2^54).  The read is kept iff S <= L * T, where T = E[Q] when min_qual_milli is a multiple of 1000 and otherwise
 *        T = floor(2^31 * 10^(-min_qual_milli / 10000) + 0.5) computed in double.  That is "mean error probability <= 10^(-Q / 10)", the
 *        mean quality those tools mean, in integer arithmetic: the result does not depend on the order of the sum.  A read of no bases
 *        passes (0 <= 0); the length test decides its fate.
 *     3. Kept reads stay in file order.
 *   Where a base's quality comes from: a FASTQ byte minus 33 (a byte below 33 or above 126 fails the call with -84); a BAM record's QUAL
 *   byte as it is (bytes 94 .. 254 fail the call with -84), not reversed for flag 0x10 -- the sum does not care.  Under a quality
 *   threshold a read of one base or more WITHOUT qualities -- a FASTA record, a BAM QUAL field whose first byte is 0xFF -- fails the call
 *   with -EINVAL (the text names --min-read-qual): such a read is never silently kept or dropped.  Without a threshold no quality byte is
 *   parsed, copied or moved, whatever the input.
 *   The filter runs in drprg_hip_map_fastx, per ingest block, on the device that takes the block, before anything else sees the block:
 *   mapping, drprg_hip_counters' reads / bases and the genotyper's total, the depth cap's running total, the resident set and
 *   drprg_hip_resident_info, drprg_hip_select_reads and discover from HBM, drprg_hip_map_resident, and the numbering of
 *   drprg_hip_subsample / drprg_hip_subsample_flags all see the kept reads alone, exactly as if the file had held only them (the pipeline
 *   chopper | rasusa | drprg).  drprg_hip_map_host* and drprg_hip_map_device* carry no qualities: while any setting is non-zero they
 *   return -EINVAL rather than map unfiltered reads without saying so.  drprg_hip_map_resident maps what `from` keeps, which is filtered.
 *   drprg_hip_discover_reads takes its reads from HBM, where only the kept ones are; when the filter dropped reads and the sample is not
 *   resident it returns -ENODATA (-61) rather than pile up the file's unfiltered reads.
 *   drprg_hip_set_read_filter: applies from the next drprg_hip_map_fastx; a reset keeps the settings.  -EINVAL for max_len != 0 &&
 *     max_len < min_len and for min_qual_milli > 93000.
 *   drprg_hip_read_filter_info: since the last reset, out[0..6] = reads seen, bases seen, dropped short, dropped long, dropped for their
 *     quality, reads kept, bases kept; out[7] = T.
 *   drprg_hip_read_filter_device: the filter alone on caller-owned device buffers, under the stream rule of the other device entries
 *     (NULL: the context's own stream; the call returns when the work is done).  d_qual: n_bases quality bytes, read i's from byte
 *     d_offsets[i] on (u64[n_reads + 1], [0] = 0); when d_qual is 16-byte aligned the 64 bytes behind n_bases must be readable; may be NULL
 *     when no quality threshold is set.  qual_bias: 33 or 0.  d_sums (u64[n_reads], may be NULL) receives S, d_flags (u8[n_reads]) 1 for a
 *     kept read.  out[0..3] = kept reads, kept bases, position + 1 of the first quality byte out of range (0: none; the call returns -84),
 *     reserved. */
int drprg_hip_set_read_filter(drprg_hip_ctx* ctx, uint64_t min_len, uint64_t max_len, uint32_t min_qual_milli);
int drprg_hip_read_filter_info(drprg_hip_ctx* ctx, uint64_t out[8]);
int drprg_hip_read_filter_device(drprg_hip_ctx* ctx, const void* d_qual, uint32_t qual_bias, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
    void* d_sums, void* d_flags, uint64_t out[4], void* hip_stream);
/* ---- Read trimming: read ends cut by quality and by fixed crops on the device, as the reads arrive.  THIS BUILD'S OWN RULE, stated from
 * memory of what the trimmers workflows run in front of drprg compute (fastp --cut_front / --cut_tail / -f / -t, Trimmomatic LEADING /
 * TRAILING / SLIDINGWINDOW, cutadapt -q, chopper --headcrop / --tailcrop); neither pandora nor drprg has one and nothing in them pins it.
 *   Settings, per context: front, tail = bases cut off the start and the end of every read (0: none); qual_milli = Q * 1000 (0: no quality
 *   trimming; at most 93000); window = W, 1..32 (4 when qual_milli != 0 and window is given as 0).
 *   A read of L bases, in the orientation the mapper sees, with Phred qualities q_0 .. q_{L-1}:
 *     1. Fixed crop.  a0 = min(front, L), b0 = L - min(tail, L - a0).
 *     2. Quality trimming, only if qual_milli != 0.  A window is a start i with a0 <= i and i + W <= b0; it is GOOD iff
 *        1000 * (q_i + ... + q_{i+W-1}) >= qual_milli * W -- the MEAN PHRED VALUE of the window, which is what fastp and Trimmomatic
 *        compare, NOT the mean error probability the read filter holds a read against.  Exact in 32-bit integers.  With i_first the
 *        smallest and i_last the largest good start, the range is [i_first, i_last + W), then narrowed from either end while the end
 *        base has 1000 * q < qual_milli (a good window holds a base at or above Q, so the narrowing stays inside the edge windows).  No
 *        good window -- a cropped read shorter than W among them -- leaves the empty range.
 *     3. Without quality trimming the range is [a0, b0).  Every empty range is reported as [0, 0).
 *   W = 1 is Trimmomatic's LEADING:Q TRAILING:Q; W = 4 is the family of fastp --cut_front --cut_tail.
 *   The read IS its kept range for everything behind the ingest.  A read trimmed to nothing stays a read of no bases, as an empty FASTQ
 *   record would be, and is counted as a read (--min-read-len 1 drops it); trimming itself never drops or reorders reads.
 *   Qualities come from where the read filter's come from: a FASTQ byte minus 33, a BAM QUAL byte as it is; a byte out of range fails the
 *   call with -84.  With qual_milli != 0 a read of one base or more WITHOUT qualities (a FASTA record, a BAM QUAL field that starts with
 *   0xFF) fails the call with -EINVAL, and the text names --trim-qual.  With fixed crops alone no quality byte is parsed, copied or moved
 *   and every input is served.  A BAM record with flag 0x10 keeps its QUAL field in stored order; the rule is mirror-symmetric, so such a
 *   read is trimmed in stored order with front and tail swapped and the range is mirrored.
 *   Trimming runs in drprg_hip_map_fastx, per ingest block, on the device that takes the block, BEFORE the read filter: length bounds and
 *   mean quality are those of the trimmed read, and the depth cap, the resident set, drprg_hip_dedup, the numbering of drprg_hip_subsample,
 *   discover and the genotyper see trimmed reads -- the run is that of a file of the trimmed reads (fastp | chopper | dedupe | rasusa |
 *   drprg), whatever the thread count, the block boundaries and the input form.  drprg_hip_read_filter_info counts trimmed reads and bases
 *   as "seen".  drprg_hip_map_host* and drprg_hip_map_device* return -EINVAL while any trim setting is non-zero.  Once a read lost a base,
 *   drprg_hip_discover_reads takes its reads from HBM and returns -ENODATA (-61) when the sample is not resident.  With no setting nothing
 *   of this exists: no launch, no wait, no quality copy.
 *   drprg_hip_set_read_trim: applies from the next drprg_hip_map_fastx; a reset keeps the settings.  -EINVAL for qual_milli > 93000, for
 *     window > 32 and for window != 0 && qual_milli == 0.
 *   drprg_hip_read_trim_info: since the last reset, out[0..7] = reads seen, bases seen, reads that lost a base, bases cut by the fixed
 *     front crop, by the fixed tail crop, by quality at the front, by quality at the tail, reads trimmed to nothing.  Bases kept = out[1] -
 *     out[3] - out[4] - out[5] - out[6]; a read without a good window counts its cropped bases as cut by quality at the front.
 *   drprg_hip_read_trim_device: the trim kernels alone on caller-owned device buffers, under the stream rule of the other device entries
 *     (NULL: the context's own stream; the call returns when the work is done).  d_qual: n_bases quality bytes in stored order, read i's
 *     from byte d_offsets[i] on (u64[n_reads + 1], [0] = 0); when d_qual is 16-byte aligned the 64 bytes behind n_bases must be readable;
 *     may be NULL when qual_milli == 0.  qual_bias: 33 or 0.  d_rev: u8[n_reads], non-zero for a read stored mirrored, or NULL.  d_begin,
 *     d_end: u64[n_reads], the kept range of every read in read orientation.  out[0..3] = kept bases, reads that lost a base, position + 1
 *     of the first quality byte out of range (0: none; the call returns -84), reserved.  Reads of 2^31 bases or more: -EINVAL. */
int drprg_hip_set_read_trim(drprg_hip_ctx* ctx, uint64_t front, uint64_t tail, uint32_t qual_milli, uint32_t window);
int drprg_hip_read_trim_info(drprg_hip_ctx* ctx, uint64_t out[8]);
int drprg_hip_read_trim_device(drprg_hip_ctx* ctx, const void* d_qual, uint32_t qual_bias, const void* d_offsets, const void* d_rev, uint64_t n_reads,
    uint64_t n_bases, void* d_begin, void* d_end, uint64_t out[4], void* hip_stream);
/* ---- Adapter trimming: sequencing adapters cut off read ends on the device, as the reads arrive.  THIS BUILD'S OWN RULE, stated from memory
 * of what fastp and cutadapt -a do with a 3' adapter; neither pandora nor drprg has one and nothing in them pins it.
 *   Settings, per context: 1 to 4 adapter sequences A_1 .. A_n, each 1 to 64 letters of ACGTacgt and no other; an error rate E in [0, 0.5]
 *   held as an integer per-mille e (E = 0.1 is e = 100, the executables' default); a minimum overlap O, 1 .. the length of the shortest
 *   adapter (given as 0: 3, or that length if it is smaller).
 *   Order.  Adapter trimming runs BEHIND the fixed crops and the quality trim of "read trimming", where fastp and cutadapt put it: it works
 *   on the range [x, y) those left, in read orientation, n = y - x.  For a BAM record with flag 0x10 that is the read as the device has
 *   already restored it: the bases need no mirror.
 *   Match.  For an adapter A of m letters and a start p in 0 .. n - 1: c = min(m, n - p); p is a MATCH iff c >= O and the number of j < c
 *   with read[x + p + j] != A[j] is at most floor(c * e / 1000).  The comparison is case-insensitive; a read base that is not ACGT differs
 *   from every adapter letter.  A window never reaches past y, so never into the next read.
 *   Cut.  The read is cut at the smallest matching p over all adapters: end = x + p.  A read cut to nothing stays a read of no bases, as
 *   with trimming; nothing is dropped or reordered.  This plain rule compares at a fixed start with substitutions only; the indel rule below
 *   (drprg_hip_set_adapters2) adds insertions, deletions and 5' adapters.  Still missing under either: anchored adapters and indels
 *   inside an adapter that the read's end cuts short.  Pair-overlap detection (fastp's default for paired reads) is a stage of its own on the
 *   resident sample: "mate overlap" above.
 *   Invariance.  Leftmost is a minimum: the result is bit-identical whatever the launch geometry, the thread count and the input form.
 *   Adapter trimming runs inside the trim stage of drprg_hip_map_fastx, so everything "read trimming" says about what lies behind it holds:
 *   the read filter, the depth cap, the resident set, drprg_hip_dedup, drprg_hip_subsample, discover and the genotyper see cut reads.  It
 *   needs no quality byte: FASTA and BAM records without qualities are served, and no quality byte is parsed, copied or moved unless
 *   another setting needs them.  drprg_hip_read_trim_info keeps counting crops and quality alone.  drprg_hip_map_host* and
 *   drprg_hip_map_device* return -EINVAL while adapters are set.  Once an adapter cut a base, drprg_hip_discover_reads takes its reads
 *   from HBM and returns -ENODATA (-61) when the sample is not resident.  With no adapter set nothing of this exists: no launch, no wait.
 *   drprg_hip_set_adapters: applies from the next drprg_hip_map_fastx; n == 0 clears (seqs may be NULL then); a reset keeps the settings.
 *     -EINVAL for n > 4, a NULL or empty sequence, one over 64 letters or with a letter outside ACGTacgt, error_milli > 500 and
 *     min_overlap above the length of the shortest adapter.
 *   drprg_hip_adapter_trim_info: since the last reset, out[0..4] = reads seen, bases seen (behind crops and quality), reads cut, bases
 *     cut, reads emptied by the adapter (they still had a base before it).
 *   drprg_hip_adapter_trim_device: the two adapter kernels alone on caller-owned device buffers, under the stream rule of the other device
 *     entries.  The bases as text (d_text: n_bases bytes; when 16-byte aligned the 64 bytes behind them must be readable; any other address
 *     is read byte by byte and never behind n_bases; d_words NULL) or as packed words (d_words: u32[ceil(n_bases / 16)], the form of
 *     drprg_hip_pack_device, with d_npos: n_npos ascending positions of the bases that are not ACGT; d_text NULL).  d_offsets: u64[n_reads
 *     + 1].  d_begin, d_end: u64[n_reads], every read's range [x, y) counted from its first base; d_end[i] becomes x + p for a cut read.
 *     out[0..4]: the five counts of this call.  -EINVAL when no adapter is set, when the offsets do not ascend to n_bases or a range does
 *     not lie inside its read; -EINVAL under the indel rule (drprg_hip_adapter_trim_device2 runs it).
 *
 *   THE INDEL RULE (drprg_hip_set_adapters2 with flag bit 0; this build's own as well, what cutadapt -a / -g -e do in spirit).  Settings per
 *   context: 0 to 4 3' adapters and 0 to 4 5' adapters, each 1 to 64 letters ACGTacgt; e and O as above, shared by both sides, O at most
 *   the shortest adapter of either side; the flag INDELS, without which there are no 5' adapters.  L(c) = floor(c * e / 1000).  ed(S, T) is
 *   the Levenshtein distance with unit costs, case-insensitive; a read base that is not ACGT differs from every adapter letter.
 *   3' side.  In the range [x, y) the crops and the quality trim left, r[0 .. n): for an adapter A of m letters, full(p) = min over p <= q
 *   <= n of ed(A, r[p .. q)) for p in 0 .. n - 1, and full(n) = m.  A start p is a MATCH of A iff
 *     (a) the adapter runs off the read's end: c = n - p < m, c >= O, and at most L(c) of the j < c have r[p + j] != A[j] (the plain rule's
 *         partial overlap, substitutions only), or
 *     (b) full(p) <= L(m) and full(p + 1) >= full(p).  The second clause takes the slack out of an edit distance: without it every start
 *         up to L(m) bases left of an occurrence would match by counting genome bases as insertions.  It needs the next start's score only.
 *   The read is cut at the smallest matching p over all 3' adapters: end = x + p.  Limit: an adapter cut short by the read's end that
 *   carries an indel in what is left is found only through (b).
 *   5' side: the exact mirror, behind the 3' cut, on [x, y').  Reverse r and reverse every 5' adapter letter by letter (no complement),
 *   apply the 3' rule; a cut at p' there gives begin = x + (n' - p').  Directly: g(q) = min over p <= q of ed(A, r[p .. q)), g(0) = m; an
 *   end q in 1 .. n' matches iff (a) q < m, q >= O and the last q letters of A differ from r[0 .. q) in at most L(q) places, or (b) g(q) <=
 *   L(m) and g(q - 1) >= g(q); the read is cut at the LARGEST matching q.  A read cut to nothing stays a read of no bases.
 *   At e = 0 the indel rule is the plain rule.  Scores may be computed in bounded windows: a verdict at p is the same when the scores are
 *   computed afresh from a window that ends m + L(m) + 2 bases behind p (or at y), which is what lets the kernels tile the buffer.
 *   Without the flag and without 5' adapters the plain rule runs, byte for byte, with its launches and no other.  Everything said above
 *   about what sees cut reads holds for both sides: -22 from drprg_hip_map_host* / drprg_hip_map_device* while any adapter is set, -61 from
 *   drprg_hip_discover_reads once either side cut a base of a sample that is not resident.
 *   drprg_hip_set_adapters2: flags bit 0 = INDELS.  -EINVAL for what drprg_hip_set_adapters refuses, on either list; for n5 > 0 without
 *     bit 0; for unknown flag bits.  n3 == n5 == 0 clears.  drprg_hip_set_adapters sets the plain rule: it clears 5' adapters and the flag.
 *   drprg_hip_front_adapter_info: since the last reset, out[0..4] = reads seen, bases seen (behind the 3' cut), reads cut, bases cut, reads
 *     emptied by a 5' adapter.  drprg_hip_adapter_trim_info keeps its five counts for the 3' side.
 *   drprg_hip_adapter_trim_device2: the buffers of drprg_hip_adapter_trim_device with d_begin writable; runs whatever rule is set; d_begin[i]
 *     becomes x + q for a read cut at its 5' end.  out[0..4]: the 3' side's counts of this call, out[5..9]: the 5' side's. */
int drprg_hip_set_adapters(drprg_hip_ctx* ctx, const char* const* seqs, uint32_t n, uint32_t error_milli, uint32_t min_overlap);
int drprg_hip_adapter_trim_info(drprg_hip_ctx* ctx, uint64_t out[5]);
int drprg_hip_adapter_trim_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, const void* d_begin, void* d_end, uint64_t out[5], void* hip_stream);
#define DRPRG_HIP_ADAPTER_INDELS 1u
int drprg_hip_set_adapters2(drprg_hip_ctx* ctx, const char* const* seqs3, uint32_t n3, const char* const* seqs5, uint32_t n5, uint32_t error_milli,
    uint32_t min_overlap, uint32_t flags);
int drprg_hip_front_adapter_info(drprg_hip_ctx* ctx, uint64_t out[5]);
int drprg_hip_adapter_trim_device2(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, void* d_begin, void* d_end, uint64_t out[10], void* hip_stream);
/* ---- Decoy screen: contaminant reads dropped on the device, as the reads arrive.  THIS BUILD'S OWN RULE, stated from memory of what bbduk
 * ref=... does (k-mer containment against a reference), the step clinical pipelines run as bbduk, kraken2, nohuman or clockwork
 * remove_contam in front of drprg; neither pandora nor drprg has one and nothing in them pins it.
 *   Settings, per context: a decoy set D; a k-mer length K in 9..31 (31 when given as 0); a fraction held as an integer per-mille f in
 *   1..1000 (500 when given as 0); a minimum number of hits M >= 1 (1 when given as 0).
 *   K-mers.  Bases are coded A 0, C 1, G 2, T 3, case-insensitive, first base in the high bits: the coding drprg_hip_select_reads takes its
 *   anchors in.  The canonical k-mer of a window of K bases is the smaller of the window's code and its reverse complement's code.  A window
 *   that holds any other letter yields no k-mer.
 *   The set.  D is the set of the canonical k-mers of every window of every record of 1 to 8 FASTA files, plain or .gz (the reader that
 *   reads the sample).  Windows never span two records; a record shorter than K adds nothing.  Limit: at most 2^31 - 1 windows in all
 *   (-EOVERFLOW beyond): mitochondrion, NTM genomes, phiX and the like.  A whole human genome is out of scope.
 *   Verdict.  For a read of L bases, as the trim stage left it: V = the number of starts p in 0 .. L - K whose window is all ACGT, H = the
 *   number of those whose canonical k-mer is in D.  The read is dropped as DECOY iff H >= M and 1000 * H >= f * V.  A read with V == 0 is
 *   kept (M >= 1).  The sums are integers: the verdict depends on nothing but the read and D.
 *   Order.  The screen runs in drprg_hip_map_fastx, per ingest block, on the device that takes the block, BEHIND the trim stage (crops,
 *   quality, 3' and 5' adapters) and behind the length and quality tests of the read filter: it judges only the reads those tests kept, and a
 *   read whose decoy part a crop or an adapter cut off is judged on what is left.  Everything "read filter" lists as seeing the kept reads
 *   alone sees the reads that also passed the screen: mapping, drprg_hip_counters' reads / bases and the genotyper's total, the depth cap's
 *   running total, the resident set and drprg_hip_resident_info, drprg_hip_select_reads and discover from HBM, drprg_hip_map_resident,
 *   drprg_hip_dedup and the numbering of drprg_hip_subsample -- the run is that of a file of the kept reads, whatever the thread count, the
 *   block boundaries and the input form (FASTQ, FASTA, .gz, BAM; ASCII or packed transport).  The screen needs no quality byte, and none is
 *   parsed, copied or moved on its account.  drprg_hip_map_host* and drprg_hip_map_device* return -EINVAL while a decoy set is loaded.  Once
 *   the screen dropped a read of a sample that is not resident, drprg_hip_discover_reads returns -ENODATA (-61).  With no decoy set nothing of
 *   this exists: no launch, no wait, no allocation.
 *   Under a decoy set drprg_hip_read_filter_info's reads kept and bases kept (out[5], out[6]) count what passed every test, the screen
 *   included: seen = short + long + low quality + decoy + kept, decoy being drprg_hip_decoy_info's out[4].
 *   The table (csrc/decoy_screen.hip): 64-bit slots in device memory, the smallest power of two >= 2 x the windows and
 *   at least 8, ~0 for an empty slot, linear probing that wraps.  Its layout depends on the order of insertion; membership does not.
 *   drprg_hip_set_decoy: builds the table on every device of the context; applies from the next drprg_hip_map_fastx; n == 0 clears the set
 *     and frees the table (fasta_paths may be NULL then).  A reset keeps the settings and the table; drprg_hip_close frees the table.
 *     -EINVAL for n > 8, k outside 9..31, min_frac_milli > 1000, a NULL path, and files that yield no k-mer at all; an unreadable file:
 *     what drprg_hip_map_fastx returns for an unreadable reads file (-ENOENT).  On any failure the context is left with no decoy set.
 *   drprg_hip_decoy_info: out[0] = distinct canonical k-mers in the set, out[1] = table slots; since the last reset, out[2..7] = reads
 *     judged, bases judged, reads dropped, bases dropped, sum of V, sum of H (over the judged reads).
 *   drprg_hip_decoy_lookup: found[i] = 1 iff k-mer kmers[i] (the coding above, either orientation: the entry canonicalises) is in the set;
 *     probed in the table on the device -- the table's own test hook.  -EINVAL without a decoy set.
 *   drprg_hip_decoy_screen_device: the screen kernels alone on caller-owned device buffers; the two input forms, the address, padding and
 *     stream rules of drprg_hip_adapter_trim_device.  d_valid, d_hits: u32[n_reads], receive V and H (either may be NULL); d_flags:
 *     u8[n_reads], 1 for a kept read.  out[0..3] = reads dropped, bases dropped, sum of V, sum of H.  -EINVAL without a decoy set, or when
 *     the offsets do not ascend from 0 to n_bases. */
int drprg_hip_set_decoy(drprg_hip_ctx* ctx, const char* const* fasta_paths, uint32_t n, uint32_t k, uint32_t min_frac_milli, uint32_t min_kmers);
int drprg_hip_decoy_info(drprg_hip_ctx* ctx, uint64_t out[8]);
int drprg_hip_decoy_lookup(drprg_hip_ctx* ctx, const uint64_t* kmers, uint64_t n, uint8_t* found);
int drprg_hip_decoy_screen_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, void* d_valid, void* d_hits, void* d_flags, uint64_t out[4], void* hip_stream);
/* ---- Base masking: low-quality bases made unknown on the device, as the reads arrive.  THIS BUILD'S OWN RULE: the switch every pile-up
 * caller has (samtools mpileup -Q, GATK's minimum base quality) and the k-mer tools have as a quality cut-off (Cortex, mccortex, Jellyfish);
 * neither pandora nor drprg has one and nothing in them pins it.
 *   Setting, per context: Q, an integer in 1..93 (0: off, the default).
 *   The rule.  A base whose Phred quality is below Q becomes an unknown base; a base of quality Q or more is untouched, whatever it is.  The
 *   run is exactly that of a file in which those bases are the letter N and everything else -- the quality bytes included -- is unchanged.
 *   The read keeps its length: its bases keep counting towards the expected depth, the depth cap and the random subsample's target, and
 *   its mean error probability under the read filter is what it was.  Only the k-mers that hold a masked base stop existing.
 *   Qualities.  The FASTQ line's byte - 33, or BAM's QUAL byte.  A reverse-strand BAM record's QUAL stays in stored order while its bases
 *   are reversed on the device: base p of a read of L bases is judged by quality byte L - 1 - p.  A byte outside 0..93 fails the run
 *   (-EFORMAT, -84), as under the other quality settings.
 *   Order.  Masking runs in drprg_hip_map_fastx, per ingest block, on the device that takes the block, BEHIND the trim stage (crops, quality
 *   trim, 3' and 5' adapters: adapters are compared as letters, and a masked base would differ from every letter) and IN FRONT OF the decoy
 *   screen (its V and H are those of the masked read), the read filter and everything behind it: mapping, the resident set,
 *   drprg_hip_dedup (where any non-ACGT base is one masked base), drprg_hip_select_reads and discover from HBM, drprg_hip_map_resident and
 *   the genotyper see the masked reads, whatever the thread count, the block boundaries and the input form (FASTQ, .gz, BAM; ASCII or packed
 *   transport).  The block is changed in its staging copy, or in the trim stage's compacted copy; the caller's memory never is.  A packed
 *   block's 2-bit letter becomes 3 (bits 2:1 of 'N') and the position joins the block's ascending list of non-ACGT positions, without a
 *   duplicate where the base was unknown already: word for word and position for position the block the file with N would have given.
 *   Masking needs qualities: a FASTA record, or a BAM record whose QUAL starts with 0xFF, fails drprg_hip_map_fastx with -EINVAL and a text
 *   that names --mask-qual (when --trim-qual is set too it is named instead: the first setting to miss them).  drprg_hip_map_host* and
 *   drprg_hip_map_device* carry no qualities and return -EINVAL while Q != 0.  Once a base of a sample that is not resident was masked,
 *   drprg_hip_discover_reads returns -ENODATA (-61).  With Q == 0 nothing of this exists: no quality byte is parsed, copied or moved on its
 *   account, no launch, no wait, no allocation.
 *   Limits.  Masking is a threshold on what the basecaller claims, no more.  At Nanopore qualities a Q of 10 or more masks so many bases that
 *   few 15-mers survive.  No claim about real samples is made: none were run.
 *   drprg_hip_set_base_mask: applies from the next drprg_hip_map_fastx, on every device of the context; a reset keeps it.  -EINVAL above 93.
 *   drprg_hip_base_mask_info: since the last reset, out[0..4] = reads seen and bases seen by the stage (behind the cuts), reads with at least
 *     one masked base, bases below Q that were one of ACGTacgt (masked), bases below Q that were not (already unknown).
 *   drprg_hip_base_mask_device: the mask kernels alone on caller-owned device buffers, under the context's Q (-EINVAL when it is 0).  d_qual,
 *     qual_bias, d_offsets, d_rev: as drprg_hip_read_trim_device takes them (d_qual readable for 64 bytes behind n_bases when it is 16-byte
 *     aligned; any other address is read byte by byte).  The bases are changed IN PLACE: d_text (n_bases bytes; nothing behind them is
 *     written) or d_words (u32[ceil(n_bases / 16)]) with d_npos / n_npos, the ascending list of its non-ACGT positions, which is only
 *     read.  d_npos_out: u64[npos_cap], receives the list behind the mask, ascending.  out[0..4]: the five counts above; out[5]: the new
 *     list's length (0 for text).  -EOVERFLOW when npos_cap is smaller than that -- out[5] still says what is needed, the words are masked,
 *     nothing is written to d_npos_out.  -EFORMAT for a quality byte outside 0..93, the text naming its position; -EINVAL when the offsets do not run from 0 to n_bases.
 *     Synchronises the stream. */
int drprg_hip_set_base_mask(drprg_hip_ctx* ctx, uint32_t min_qual);
int drprg_hip_base_mask_info(drprg_hip_ctx* ctx, uint64_t out[5]);
int drprg_hip_base_mask_device(drprg_hip_ctx* ctx, const void* d_qual, uint32_t qual_bias, const void* d_offsets, const void* d_rev, uint64_t n_reads,
    uint64_t n_bases, void* d_text, void* d_words, const void* d_npos, uint64_t n_npos, void* d_npos_out, uint64_t npos_cap, uint64_t out[6], void* hip_stream);
/* ---- Poly tails: runs of one letter cut off read ends on the device, as the reads arrive.  THIS BUILD'S OWN RULE, stated from memory of
 * fastp's poly-G / poly-X tail trimming (which fastp turns on by itself for NextSeq and NovaSeq data: on two-colour chemistry "no signal" is
 * called as G, with HIGH qualities, so neither quality setting touches such a tail); neither pandora nor drprg has one and nothing in them
 * pins it.
 *   The comparison, shared with "read complexity" below: case-insensitive; every byte that is not one of ACGTacgt is the one unknown base
 *   U -- a listed position of a packed block and a base drprg_hip_set_base_mask masked included --; U equals U and differs from every letter.
 *   Settings, per context: a non-empty set S of letters from ACGT, and M, a whole number in 2..255 (the executables' default: 10).
 *   The rule.  A read of L bases in read orientation, as the stages in front left it.  For a letter X and n in M..L the suffix of n bases
 *   QUALIFIES when its first (leftmost) base is X and the number mm of its bases that are not X is at most min(floor(n / 8), 5).  The read
 *   loses its LONGEST qualifying suffix over all X in S; nothing when none qualifies.  "Longest" is a maximum over independent tests: the
 *   result is bit-identical whatever the launch geometry, the thread count, the block boundaries and the input form.  mm only grows with n,
 *   so a scan from the read's end may stop at the sixth base that is not X: the work per read is its tail's length plus a few bases.
 *   Differences from fastp, on purpose: fastp stops at the first prefix-from-the-end that breaks its allowance; this rule has no running
 *   condition.  And the rule can take along up to five bases that were not X (e.g. TTTT GACGT G x 40 under S = {G}, M = 10 loses 45 bases).
 *   Order.  The cut runs in drprg_hip_map_fastx, per ingest block, inside the trim stage BEHIND the crops, the quality trim, the 3' and the
 *   5' adapters, on what they left, and IN FRONT OF base masking, the decoy screen, the read filter and everything behind them: the run is
 *   that of a file of the cut reads.  A reverse-strand BAM record is cut in read orientation.  It needs no quality byte and serves FASTA
 *   and BAM without QUAL.  A read cut to nothing stays, as a read of no bases.  drprg_hip_map_host* and drprg_hip_map_device* return -EINVAL
 *   while S is set.  Once a tail was cut off a read of a sample that is not resident, drprg_hip_discover_reads returns -ENODATA (-61).  With
 *   no S nothing of this exists: no launch, no wait, no allocation, no copy.
 *   drprg_hip_set_poly_trim: letters: a string of distinct letters of ACGTacgt; NULL or "" clears the setting.  Applies from the next
 *     drprg_hip_map_fastx, on every device of the context; a reset keeps it.  -EINVAL for any other letter, a repeated letter, or min_len
 *     outside 2..255.
 *   drprg_hip_poly_trim_info: since the last reset, out[0..4] = reads seen and bases seen by the cut (behind both adapter sides), reads cut,
 *     bases cut, reads emptied.
 *   drprg_hip_poly_trim_device: the tail cut alone on caller-owned device buffers, under the context's settings (-EINVAL without): the
 *     buffers, the two input forms and the stream, alignment and readable-64-bytes rules of drprg_hip_adapter_trim_device.  d_begin / d_end
 *     hold every read's range; d_end receives the cut ranges' ends.  out[0..4]: this call's five counts.  Synchronises the stream. */
int drprg_hip_set_poly_trim(drprg_hip_ctx* ctx, const char* letters, uint32_t min_len);
int drprg_hip_poly_trim_info(drprg_hip_ctx* ctx, uint64_t out[5]);
int drprg_hip_poly_trim_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, const void* d_begin, void* d_end, uint64_t out[5], void* hip_stream);
/* ---- Read complexity: low-complexity reads dropped on the device, as the reads arrive.  THIS BUILD'S OWN RULE, stated from memory of
 * fastp's low-complexity filter (whose default threshold is 30 %; here the default is off).
 *   Setting, per context: P, a whole number in 1..100 (0: off).
 *   The rule, under the comparison of "poly tails".  For a read of L bases, D = the number of i in 0..L - 2 whose bases i and i + 1 differ.
 *   The read is dropped as LOW COMPLEXITY iff L >= 2 and 100 * D < P * (L - 1), in 64-bit integers.  A read of 0 or 1 bases is kept by this
 *   test (lengths are the read filter's business).  D is a sum over independent positions: the verdict depends on nothing but the read.
 *   So a read that is dark from its first cycle (all G), homopolymer and dinucleotide-poor reads, and reads that base masking turned almost
 *   wholly unknown are dropped.
 *   Order.  The test runs in drprg_hip_map_fastx, per ingest block, on the read as the trim stage (both adapter sides and the tail cut
 *   included) and base masking left it.  Only the reads the length and quality tests of the read filter kept are judged, and the decoy
 *   screen's verdict then applies only to the reads this test kept as well.  Everything "read filter" lists as seeing the kept reads alone
 *   sees one verdict.  It needs no quality byte.  A read is shorter than 2^32 bases (a block that is not is refused, -EOVERFLOW).
 *   drprg_hip_map_host* and drprg_hip_map_device* return -EINVAL while P != 0.  Once the test dropped a read of a sample that is not
 *   resident, drprg_hip_discover_reads returns -ENODATA (-61).  With P == 0 nothing of this exists: no launch, no wait, no allocation.
 *   drprg_hip_read_filter_info's reads kept and bases kept (out[5], out[6]) count what passed every test: seen = short + long + low quality
 *   + low complexity + decoy + kept, low complexity being drprg_hip_complexity_info's out[2] and decoy drprg_hip_decoy_info's out[4].
 *   drprg_hip_set_min_complexity: applies from the next drprg_hip_map_fastx, on every device of the context; a reset keeps it; 0 clears it.
 *     -EINVAL above 100.
 *   drprg_hip_complexity_info: since the last reset, out[0..3] = reads judged, their bases, reads dropped, bases dropped.
 *   drprg_hip_complexity_device: the kernels alone on caller-owned device buffers, under the context's P (-EINVAL when it is 0); the two
 *     input forms and the address, padding and stream rules of drprg_hip_adapter_trim_device.  d_diff: u32[n_reads], receives D (may be
 *     NULL); d_flags: u8[n_reads], 1 for a kept read.  out[0..1] = reads dropped, bases dropped.  -EINVAL when the offsets do not ascend
 *     from 0 to n_bases.  Synchronises the stream. */
int drprg_hip_set_min_complexity(drprg_hip_ctx* ctx, uint32_t percent);
int drprg_hip_complexity_info(drprg_hip_ctx* ctx, uint64_t out[4]);
int drprg_hip_complexity_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, void* d_diff, void* d_flags, uint64_t out[2], void* hip_stream);
/* ---- Read statistics: the QC record of a sample (--qc-json), counted on the device as the reads arrive.  THIS BUILD'S OWN RULE: the sums
 * fastp, NanoStat and nanoq report, before and after preparation.  Statistics only: no pass or fail verdict, no adapter guess (the
 * duplication levels of a paired sample: "duplicate pairs" above, the report's "pair_dedup" entry).
 *   Setting, per context: mode 0 (off, the default), 1 (with qualities), 2 (without the three quality sections: --qc-no-qual).
 *   Two snapshots.  RAW: every read of every ingest block of drprg_hip_map_fastx as the file holds it, in front of the trim stage (BAM: read
 *   orientation, secondary and supplementary records skipped, as the ingest does).  PREPARED: exactly the reads and bases the block hands on
 *   to mapping: behind the crops, the quality trim, both adapter sides, the tail cut, the mask (a masked base is an unknown base), the read
 *   filter, the complexity test, the decoy verdict and the depth cap's cut; a read trimmed to nothing that is kept is a read of 0 bases.  It
 *   lies IN FRONT OF drprg_hip_dedup and drprg_hip_subsample, which work on the resident sample without qualities and keep counts of their
 *   own.  When no prep setting and no depth cap is active the prepared snapshot is the raw one by definition and is not counted a second
 *   time (drprg_hip_read_stats_prepared_is_raw).  Under a depth cap the ingest stops at the block that reaches it: the raw snapshot
 *   holds that block whole and nothing behind it.
 *   The rule, under the comparison of "poly tails": case-insensitive; every byte not in ACGTacgt, a listed position of a packed block and
 *   a masked base are the one unknown base U.  A snapshot is drprg_hip_read_stats_words() u64 words; drprg_hip_read_stats_layout gives
 *   out[0..12] = words, the offsets of len_reads, len_bases, cyc_base, cyc_qsum, qual_hist, readq_hist, gc_hist, then B, C, 5, 94, 101:
 *     [0] reads, [1] bases, [2] shortest read (0 without a read), [3] longest read.
 *     len_reads[B], len_bases[B], B = 2432: reads per length bin, and the exact sum of their lengths.  The bin of L is L for L < 1024;
 *       otherwise, with e = floor(log2 L) in 10..31, 1024 + (e - 10) * 64 + ((L >> (e - 6)) & 63): exact below 1024, within 1/64 above.
 *       N50 (N90) is taken on the host: the bins walked downwards over len_bases until ceil(bases / 2) (ceil(9 bases / 10)) are reached;
 *       the bin's lowest length is reported.
 *     cyc_base[C + 1][5], cyc_qsum[C + 1], C = 512: for position p of a read, in read orientation, the bases A, C, G, T, U and the sum of
 *       the Phred values; entry C takes every p >= 512.  The sample's base totals are the column sums.
 *     qual_hist[94]: bases per Phred value.
 *     readq_hist[94]: a read of L >= 1 bases falls into the largest q with sum(E[qual_i]) <= E[q] * L in 64-bit integers, E the read
 *       filter's table round(2^31 * 10^(-q / 10)): the quality of the read's MEAN ERROR PROBABILITY, what --min-read-qual judges, not the
 *       mean of its Phred values.  q = 0 always holds.  Reads of no bases are not counted.
 *     gc_hist[101]: a read with V >= 1 bases of ACGT falls into floor(100 * (G + C) / V); reads without one are not counted.
 *   Every word is an integer sum over independent reads and positions: bit-exact whatever the thread count, the block boundaries, the
 *   devices and the input form (FASTQ, .gz, BAM; ASCII or packed transport).
 *   Qualities: the FASTQ byte - 33, or BAM's QUAL byte; base p of a reverse-strand BAM record of L bases has quality byte L - 1 - p; a byte
 *   outside 0..93 fails the run (-EFORMAT, -84).  Mode 1 needs them: a FASTA record, or a BAM record whose QUAL starts with 0xFF, fails
 *   drprg_hip_map_fastx with -EINVAL and a text that names --qc-json (another quality setting, when one is set, is named first).  Under
 *   mode 2 no quality byte is parsed, copied or moved on the statistics' account, qual_hist, readq_hist and cyc_qsum stay zero, and every
 *   input is served.  drprg_hip_map_host* and drprg_hip_map_device* carry no qualities: they return -EINVAL while mode 1 is set, and under
 *   mode 2 their reads are simply not counted.  A block is shorter than 2^32 bases (-EOVERFLOW otherwise).
 *   With only this setting on, coverage, every counter and the resident sample are those of a run without it; the kernels are queued beside
 *   the block's other work and add no wait per block.  With mode 0 nothing of this exists: no launch, no allocation, no quality byte.
 *   drprg_hip_set_read_stats: applies from the next drprg_hip_map_fastx, on every device of the context; a reset keeps the setting and
 *     zeroes both snapshots.  -EINVAL for another mode.
 *   drprg_hip_read_stats_info: which = 0 raw, 1 prepared; the devices' snapshots folded, read back once.  -EINVAL when n_words is below
 *     drprg_hip_read_stats_words().
 *   drprg_hip_read_stats_device: the kernels alone on caller-owned device buffers; one snapshot into out.  The bases in the two forms and
 *     under the address, padding and stream rules of drprg_hip_base_mask_device (d_npos only read); d_qual with qual_bias and d_rev as
 *     there, or d_qual NULL: the quality sections stay zero.  d_flags: u8[n_reads], 0 for a read that is not counted, or NULL; take: only
 *     reads below it are counted (n_reads: all).  n_reads == 0: a snapshot of zeros, no pointer is looked at.  -EFORMAT for a quality byte
 *     outside 0..93, the text naming it; -EINVAL when the offsets do not ascend from 0 to n_bases or n_words is too small.
 *   drprg_hip_write_qc_json: the report both executables write for --qc-json: sample, settings, both snapshots (totals, N50, N90, base
 *     totals, non-empty length bins as [lowest length, reads, bases], per-cycle arrays cut at the longest read, the histograms) and, under
 *     "stages", the words of every stage's *_info entry in their order, with drprg_hip_dedup's and drprg_hip_subsample's four outputs. */
uint64_t drprg_hip_read_stats_words(void);
int drprg_hip_read_stats_layout(uint64_t out[13]);
int drprg_hip_set_read_stats(drprg_hip_ctx* ctx, int mode);
int drprg_hip_read_stats_info(drprg_hip_ctx* ctx, int which, uint64_t* out, uint64_t n_words);
int drprg_hip_read_stats_prepared_is_raw(drprg_hip_ctx* ctx); /* 1: yes, 0: no; negative: error */
int drprg_hip_read_stats_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_qual,
    uint32_t qual_bias, const void* d_offsets, const void* d_rev, uint64_t n_reads, uint64_t n_bases, const void* d_flags, uint64_t take, uint64_t* out,
    uint64_t n_words, void* hip_stream);
int drprg_hip_write_qc_json(drprg_hip_ctx* ctx, const char* path, const char* sample);
/* The read selection drprg_hip_discover_reads uses when the reads are resident, on its own: for every device of the context, in order,
 * every kept read in which a k-mer of `anchors` STARTS (anchors: n_anchors k-mers of A bases, 2 bits per base, A 0 C 1 G 2 T 3, first base
 * in the high bits; any order, duplicates allowed).  A block's reads are one base stream: read r of a block is returned iff for some p with
 * offsets[r] <= p < offsets[r + 1] and p + A <= the block's bases, stream[p .. p + A) is all ACGTacgt and, upper-cased, an anchor -- the
 * k-mer may run on into the reads behind r (the caller's own scan of the returned reads decides; no read that holds an anchor is lost).
 *   A read is returned once.  Reads come in block order, then read order, device after device.  A block kept in the packed form returns
 *   upper case (non-ACGT bytes as N), an ASCII block the bytes of the file.
 *   bases[bases_cap], offsets[reads_cap + 1] (offsets[0] = 0), ids[reads_cap]: ids[i] = kept block << 32 | read in that block, the blocks
 *   counted through the devices as drprg_hip_resident_info counts them.  out[0] = reads, out[1] = bases selected, always; -EOVERFLOW
 *   (-75) with nothing copied when either buffer is too small -- call with both caps 0 for the sizes.
 *   window_bytes: packed blocks are expanded to ASCII for the scan a window of consecutive blocks at a time, as many as expand into
 *   window_bytes (a larger block alone); 0 = the built-in 1 GB, what discover uses.  The result does not depend on it.
 *   -ENODATA (-61) unless every read mapped since the last reset is resident; -EINVAL for A outside 1..31. */
int drprg_hip_select_reads(drprg_hip_ctx* ctx, const uint64_t* anchors, uint64_t n_anchors, uint32_t A, uint64_t window_bytes, uint8_t* bases,
    uint64_t bases_cap, uint64_t* offsets, uint64_t* ids, uint64_t reads_cap, uint64_t out[2]);

/* What MakePrg::update does in the reference (/root/reference/src/lib.rs:279-456: mafft --add of the consensus with the novel
 * variants, then make_prg from_msa) for a host without make_prg / mafft: writes the context's PRG file again with every novel variant
 * added as a new site -- first allele: the stretch of the PRG string the variant touches, whole sites it runs into included; second
 * allele: the called path over that stretch with the variant applied; markers numbered again in pandora's parse order -- so that the
 * PRG spells everything it spelled before and the sample's sequence (index it with drprg_hip_index, open it, map again).
 *   drprg_hip_update_prg: the variants of the last drprg_hip_discover_reads.
 *   drprg_hip_update_prg_from_paths: the loci, called paths and variants of a denovo_paths.txt -- this library's or pandora discover's own
 *     (layout: /root/reference/src/lib.rs:3010-3038; the file MakePrg::update is handed, src/predict.rs:260-279).  -EINVAL if the file
 *     does not parse, names a locus the PRG file does not hold, or its node intervals are not intervals of this context's PRG.  Host only.
 * *n_applied: variants placed. */
int drprg_hip_update_prg(drprg_hip_ctx* ctx, const char* out_prg, uint32_t* n_applied);
int drprg_hip_update_prg_from_paths(drprg_hip_ctx* ctx, const char* denovo_paths, const char* out_prg, uint32_t* n_applied);

/* Coverage hand-over between `discover` and the `map` that follows it on the same reads and PRG
 * (/root/reference/src/predict.rs:248-255, :296-302): save writes vector + counters under `tag`; load returns 0 and installs
 * them only if the file exists, is intact and carries the same tag and index shape (-ENOENT otherwise: map the reads). */
int drprg_hip_save_coverage(drprg_hip_ctx* ctx, const char* path, const char* tag);
int drprg_hip_load_coverage(drprg_hip_ctx* ctx, const char* path, const char* tag, uint64_t counters[8]);

/* a-9 on raw inputs, for parity harnesses (host only, no context): the same functions drprg_hip_genotype applies per allele
 * and per site (pandora SampleInfo; pinned by the reference's fixture VCFs, tests/golden/likelihood_kat.tsv).
 * out[0..5] = MEAN_FWD, MEAN_REV, MED_FWD, MED_REV, SUM_FWD, SUM_REV; *gaps = GAPS. */
int drprg_hip_allele_stats(const uint32_t* fwd, const uint32_t* rev, uint32_t n, uint32_t min_kmer_covg, uint32_t out[6], double* gaps);
int drprg_hip_genotype_site(const uint32_t* mean_fwd, const uint32_t* mean_rev, const double* gaps, uint32_t n_alleles, double e,
    double eps, double* likelihood, int32_t* gt, double* gt_conf);
/* Which k-mer nodes every allele of the last drprg_hip_genotype took its statistics over: one TSV line per allele
 * (chrom, pos, allele, n, comma-separated global k-mer node numbers = indexes/2 into the coverage vector). */
int drprg_hip_genotype_alleles(drprg_hip_ctx* ctx, const char* out_tsv);

/* Host-side check of the Bloom filters of the prefiltered kernel (no device needed): out[0] = index k-mer codes tested
 * (both orientations), out[1..3] = codes that level 0 / levels 1+2 / the second stage would wrongly reject (false
 * negatives: must be 0), out[4..6] = bits set per thousand in those three arrays, out[7] = codes that the array holding level 0
 * and the second-stage bits together (second stage inside the streaming kernel) would wrongly reject.  All zero: no filter. */
int drprg_hip_filter_selfcheck(const drprg_hip_ctx* ctx, uint64_t out[8]);
/* ---- between the read loop and the VCF: the coverage model of the sample, the best path of a locus, the presence rule ----
 * (csrc/params.h; what `pandora map` computes in estimate_parameters / find_max_path / add_consensus_path_to_fastaq behind
 * /root/reference/src/lib.rs:580-642.  The reference consumes e = exp_depth_covg through every LIKELIHOOD / GT_CONF --
 * /root/reference/src/filter.rs:12-16, :149 -- and the presence of a locus through the ##contig lines,
 * /root/reference/src/predict.rs:757-765.)  drprg_hip_genotype runs all of it; these entries expose the pieces so that the test
 * suite can hold each against the oracle's separate statement (oracle/oracle_params.c).
 * estimate_parameters: kmer_covg = fwd + rev coverage of every k-mer of every locus with a cluster; out[0] exp_depth_covg,
 * [1] binomial model in force, [2] e_rate, [3] nb_p, [4] nb_r, [5] branch (1 binomial, 2 negative binomial, 3 insufficient
 * coverage, 0 no locus), [6] mean, [7] variance, [8] clusters per locus, [9] binomial p.  coverage_model: the same of the last
 * drprg_hip_genotype, then [10] thresh, [11] loci dropped because their best path was almost bare. */
int drprg_hip_estimate_parameters(const uint32_t* kmer_covg, uint64_t n, uint64_t clusters, uint64_t loci, uint32_t global_covg, int k,
    double e_rate, int bin, double out[10]);
int drprg_hip_kmer_log_prob(int use_bin, double nb_p, double nb_r, double bin_p, uint32_t fwd, uint32_t rev, uint32_t locus_reads, float* out);
int drprg_hip_prob_threshold(const float* logp, uint64_t n, int* out);
/* best path of locus `prg` for per-node log probabilities logp[n_nodes of that locus]: node ids, source and sink excluded */
int drprg_hip_max_path(const drprg_hip_ctx* ctx, uint32_t prg, const float* logp, int thresh, uint32_t max_kmers_to_average, uint32_t* path,
    uint64_t cap, uint64_t* n_path);
/* per-base coverage of the local nodes along `path`; covg2 = (fwd, rev) per k-mer node of the locus */
int drprg_hip_path_base_coverage(const drprg_hip_ctx* ctx, uint32_t prg, const uint32_t* path, uint64_t n_path, const uint32_t* covg2,
    uint32_t* out, uint64_t cap, uint64_t* n_out);
int drprg_hip_path_coverage_too_low(const uint32_t* base_covg, uint64_t n, uint32_t global_covg); /* 1: the locus is dropped */
int drprg_hip_coverage_model(const drprg_hip_ctx* ctx, double out[12]);

/* Index introspection for harnesses: sizes[0..4] = keys, records, prgs, k-mer nodes, table slots. */
int drprg_hip_index_sizes(const drprg_hip_ctx* ctx, uint64_t sizes[5]);
int drprg_hip_index_export(const drprg_hip_ctx* ctx, uint64_t* keys, uint32_t* rec_off, uint32_t* rec_prg,
    uint32_t* rec_knode, uint8_t* rec_strand, uint32_t* prg_min_path_len, uint32_t* prg_knode_base);

/* Device-side tables of an open context: out[0] = 32-bit words of the L2-resident Bloom tier in front of the probe table
 * (0: the table fits the L2, no tier), out[1] = bytes of the open-addressed probe table (keys + slot records), out[2] = bytes
 * of the LDS-resident filter arrays of the prefiltered sequence (0: index too large / k > 15), out[3] = sequence in use,
 * out[4] = bytes of the filter tiers of that sequence that live in global memory (L2-resident: the middle tier's bitmap and
 * code filter; the small tier's block filter, which is the second stage for packed batches; 0 otherwise), out[5] = the sketch
 * form that serves the context: 1 sketch_wave_kernel; sketch_probe_kernel with 2 its compile-time window, 3 its sequential scan on
 * 32-bit keys, 4 on 64-bit keys; of the prefiltered sequence 10 the small tier, 11 levels 1+2 alone (k < 15), 12 the middle tier. */
int drprg_hip_device_tables(drprg_hip_ctx* ctx, uint64_t out[6]);

/* Local-graph introspection of PRG `prg` (node intervals are offsets into the PRG string, markers and their
 * spaces included: the convention of pandora's denovo_paths.txt, /root/reference/src/lib.rs:3015-3023).
 * Writes up to cap node [start,end) pairs; *n_nodes receives the node count, *n_sites the site count. */
int drprg_hip_prg_nodes(const drprg_hip_ctx* ctx, uint32_t prg, uint32_t* starts, uint32_t* ends, uint32_t cap,
    uint32_t* n_nodes, uint32_t* n_sites);

/* ---- post-VCF stage (host only; SURVEY.md section 8f NEXT-1) ------------------------------------------------
 * Options of Filterer (/root/reference/src/filter.rs:165-197) and MinorAllele (/root/reference/src/minor.rs:19-49)
 * with the CLI defaults of `drprg predict`; a disabled filter is min_covg < 0, max_covg = INT32_MAX,
 * min_strand_bias / min_gt_conf / min_frs < 0, max_indel < 0. */
typedef struct drprg_hip_annotate_opts {
    int32_t min_covg, max_covg;
    float min_strand_bias, min_gt_conf, min_frs;
    int32_t max_indel;
    float maf, max_gaps, max_called_gaps, max_gaps_diff;
    int32_t minor_min_covg;
    float minor_min_strand_bias;
    int32_t ignore_synonymous;
    uint64_t id_seed; /* 0: random 8-hex record IDs like the reference's Uuid::new_v4()[..8] */
} drprg_hip_annotate_opts;

/* Replaces Predict::predict_from_pandora_vcf (/root/reference/src/predict.rs:420-544): pandora VCF -> filtered,
 * annotated VCF (FILTER, PDP/OGT/VARID/PREDICT INFO).  index_dir holds .config.toml, genes.fa, panel.bcf, rules.csv.
 * Deviation: the output is VCF text, not BCF.  err receives the message on failure (may be NULL). */
int drprg_hip_annotate(const char* index_dir, const char* pandora_vcf, const char* out_vcf,
    const drprg_hip_annotate_opts* opts, char* err, size_t err_len);
/* The annotated VCF as BCF2.2 in BGZF: the format and file name (<sample>.drprg.bcf) the reference writes through rust-htslib
 * (/root/reference/src/predict.rs:429-431).  `drprg predict` of this build writes both the text VCF and this. */
int drprg_hip_vcf_to_bcf(const char* vcf_path, const char* bcf_path, char* err, size_t err_len);
/* Replaces Predict::vcf_to_json (/root/reference/src/predict.rs:716-1086).  padding < 0 / index_version NULL: taken from
 * <index_dir>/.config.toml. */
int drprg_hip_report_json(const char* index_dir, const char* annotated_vcf, const char* out_json, const char* sample,
    int padding, const char* index_version, char* err, size_t err_len);

/* HIP-event timing of the dominant kernel (sketch_filter_kernel / sketch_probe_kernel) on its launch stream (bench.py roofline);
 * launches = launches of that kernel, one per batch (a batch run again with larger buffers counts its first attempt only).
 * enable != 0 starts/keeps timing; ms_total / launches may be NULL; reset != 0 clears the sums. */
int drprg_hip_kernel_timing(drprg_hip_ctx* ctx, int enable, int reset, double* ms_total, uint64_t* launches);
/* How sketch_filter_kernel handed its tiles out in the batch completed last, and when its four wave classes were through (bench.py prints
 * it next to the roofline; csrc/kernels.h FilterSched).  out[0] rounds of the schedule (1: static, one chunk per wave), [1] chunks = slices,
 * [2] tiles per wave of round 0, [3..6] the classes' shares of round 0 in 1/256 of an even one, [7..10] the classes' end times in 10 ns from
 * the kernel's first wave (0: not clocked), [11] chunks per workgroup, [12..19] chunk size of every round in tiles.  Synchronises. */
int drprg_hip_filter_schedule(drprg_hip_ctx* ctx, uint64_t out[20]);
/* The device buffers that grow when a batch does not fit them, and how often they had to (tests: the paths that run a batch again).
 * out[0] batches of the filtered sequence run again after a candidate slice overflowed, [1] the same for the direct sequence's
 * candidate form, [2] regrows of the generic pipeline's hit buffer, [3] largest candidate capacity of any lane in entries, [4] hit
 * buffer capacity in entries, [5] 0 (reserved).  Counted from drprg_hip_open like the buffers themselves: drprg_hip_reset keeps them.
 * A multi-device context sums [0..2] and takes the largest [3..4].  The smallest capacity is DRPRG_HIP_MIN_CAPACITY entries (default
 * 2^20, at least 4096; read when the context opens).  Synchronises. */
int drprg_hip_buffer_info(drprg_hip_ctx* ctx, uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif
