"""Host-side mirror of the reference's `Pandora` shim for the predict hot path.

`Pandora` below exposes the operator interface of struct Pandora in /root/reference/src/lib.rs:459-698
(`index_with`, `discover_with`, `genotype_with`, `vcf_filename`, `list_prgs_with_novel_variants`) with
the same argument meaning and error behaviour, but runs in-process on an MI355X through the C ABI of
include/drprg_hip.h instead of spawning the external `pandora` program.  `Context` is the thin object
wrapper of the C ABI that tests and bench.py drive directly.
"""
import ctypes as C
import os
import re

import numpy as np

from ._lib import MapOpts, lib

MTB_GENOME_SIZE = 4411532  # /root/reference/src/lib.rs:36


class DependencyError(RuntimeError):
    """Mirror of DependencyError (/root/reference/src/lib.rs:43-75): ProcessError / MissingExpectedOutput /
    NovelVariantParsingError are told apart by `kind`."""

    def __init__(self, kind, message, code=0):
        super().__init__(f"{kind}: {message}")
        self.kind = kind
        self.code = code


def _check(rc, ctx=None):
    if rc != 0:
        msg = lib.drprg_hip_last_error(ctx)
        raise DependencyError("ProcessError", (msg or b"").decode() or f"error {rc}", code=-rc)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One opened index (+ its HIP device).  device=-1: host-only (index export, genotyping)."""

    def __init__(self, prg_file, w, k, device=0, from_files=True, threads=1, devices=None):
        """devices: a list of HIP device ids -> one context over all of them (drprg_hip_open_multi: map_fastx shards the reads)"""
        p = os.fsencode(prg_file)
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            self._h = lib.drprg_hip_open_multi(p, w, k, arr, len(devices), 1 if from_files else 0)
            device = devices[0]
        else:
            self._h = lib.drprg_hip_open(p, w, k, device) if from_files else lib.drprg_hip_open_prg(p, w, k, device, threads)
        if not self._h:
            raise DependencyError("ProcessError", lib.drprg_hip_last_error(None).decode(), code=-lib.drprg_hip_open_error())
        self.w, self.k, self.device = w, k, device
        sizes = (C.c_uint64 * 5)()
        lib.drprg_hip_index_sizes(self._h, sizes)
        self.n_keys, self.n_records, self.n_prgs, self.n_knodes, self.n_slots = (int(x) for x in sizes)

    def close(self):
        if self._h:
            lib.drprg_hip_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    # ---- options -------------------------------------------------------------------------------
    def set_opts(self, illumina=False, min_cluster_size=10, genome_size=MTB_GENOME_SIZE, max_diff=0, error_rate=0.0,
                 genotyping_error_rate=0.0, kernel=0, binomial=False):
        """kernel: 0 auto, 1 direct sketch kernel + generic cluster pipeline, 2 Bloom-prefiltered kernel, 3 direct sketch
        kernel in its candidate form (read_cluster_kernel)"""
        o = MapOpts(max_diff, error_rate, min_cluster_size, 1 if illumina else 0, genome_size, genotyping_error_rate, kernel,
                    1 if binomial else 0)
        _check(lib.drprg_hip_set_opts_sized(self._h, C.byref(o), C.sizeof(o)), self._h)

    # ---- mapping -------------------------------------------------------------------------------
    def set_threads(self, threads):
        """parser threads of map_fastx (the -t drprg forwards to pandora)"""
        _check(lib.drprg_hip_set_threads(self._h, int(threads)), self._h)

    def map_fastx(self, path):
        _check(lib.drprg_hip_map_fastx(self._h, os.fsencode(path)), self._h)

    def map_host(self, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _check(lib.drprg_hip_map_host(self._h, _ptr(bases), _ptr(offsets), len(offsets) - 1), self._h)

    # ---- 2-bit packed reads (include/drprg_hip.h "packed reads") -----------------------------------
    def set_input_format(self, packed):
        """map_fastx packs the reads to 2 bits on its parser threads (True) or hands ASCII blocks to the device (False, the default)"""
        _check(lib.drprg_hip_set_input_format(self._h, 1 if packed else 0), self._h)

    def map_host_packed(self, words, offsets, npos=None):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        npos = np.ascontiguousarray(npos if npos is not None else [], dtype=np.uint64)
        _check(lib.drprg_hip_map_host_packed(self._h, _ptr(words), _ptr(offsets), len(offsets) - 1, _ptr(npos) if npos.size else None, npos.size), self._h)

    def map_device_packed(self, d_words, d_offsets, n_reads, n_bases, d_npos=None, n_npos=0, d_covg=None, d_prg_reads=None, stream=None, deferred=False):
        fn = lib.drprg_hip_map_device_packed_async if deferred else lib.drprg_hip_map_device_packed
        _check(fn(self._h, d_words, d_offsets, n_reads, n_bases, d_npos, n_npos, d_covg, d_prg_reads, stream), self._h)

    def pack_device(self, d_bases, n_bases, d_words, d_npos=None, npos_cap=0, stream=None):
        """ASCII -> packed on the device; returns the number of non-ACGT bases (their positions, ascending, in d_npos)"""
        n = C.c_uint64()
        _check(lib.drprg_hip_pack_device(self._h, d_bases, n_bases, d_words, d_npos, npos_cap, C.byref(n), stream), self._h)
        return int(n.value)

    # ---- BAM input (include/drprg_hip.h "BAM input") ----------------------------------------------
    def pack_device_bam(self, d_seq, d_seq_start, d_offsets, d_reverse, n_reads, n_bases, d_words, d_npos=None, npos_cap=0, stream=None):
        """BAM's 4-bit sequence fields -> packed on the device (drprg_hip_pack_device_bam); returns the number of non-ACGT positions
        (ascending in d_npos).  d_reverse may be None: no read is reverse-complemented."""
        n = C.c_uint64()
        _check(lib.drprg_hip_pack_device_bam(self._h, d_seq, d_seq_start, d_offsets, d_reverse, n_reads, n_bases, d_words, d_npos, npos_cap,
                                             C.byref(n), stream), self._h)
        return int(n.value)

    def bam_info(self):
        """what map_fastx saw of BAM files since the last reset"""
        out = (C.c_uint64 * 4)()
        _check(lib.drprg_hip_bam_info(self._h, out), self._h)
        return dict(records=int(out[0]), skipped=int(out[1]), reversed=int(out[2]), device_blocks=int(out[3]))

    def map_device(self, d_bases, d_offsets, n_reads, n_bases, d_covg=None, d_prg_reads=None, stream=None):
        """Pointers are integer device addresses (e.g. torch.Tensor.data_ptr())."""
        _check(lib.drprg_hip_map_device(self._h, d_bases, d_offsets, n_reads, n_bases, d_covg, d_prg_reads, stream), self._h)

    def map_device_async(self, d_bases, d_offsets, n_reads, n_bases, d_covg=None, d_prg_reads=None, stream=None):
        """map_device without the host waiting: the batch is queued and completed by the next call (or sync(), or anything
        that reads results); its buffers must stay valid and unchanged until then (drprg_hip_map_device_async)."""
        _check(lib.drprg_hip_map_device_async(self._h, d_bases, d_offsets, n_reads, n_bases, d_covg, d_prg_reads, stream), self._h)

    def sync(self):
        _check(lib.drprg_hip_sync(self._h), self._h)

    def reduce(self):
        """multi-device context: the devices' vectors summed into the first device, on the devices (drprg_hip_reduce)"""
        _check(lib.drprg_hip_reduce(self._h), self._h)
        buf = C.create_string_buffer(256)
        lib.drprg_hip_reduce_info(self._h, buf, len(buf))
        return buf.value.decode()

    # ---- coverage ------------------------------------------------------------------------------
    def coverage(self):
        covg = np.zeros(2 * self.n_knodes, dtype=np.uint32)
        prg_reads = np.zeros(self.n_prgs, dtype=np.uint32)
        _check(lib.drprg_hip_coverage(self._h, _ptr(covg), covg.size, _ptr(prg_reads), prg_reads.size), self._h)
        return covg, prg_reads

    def set_coverage(self, covg, prg_reads, total_bases):
        covg = np.ascontiguousarray(covg, dtype=np.uint32)
        prg_reads = np.ascontiguousarray(prg_reads, dtype=np.uint32)
        _check(lib.drprg_hip_set_coverage(self._h, _ptr(covg), covg.size, _ptr(prg_reads), prg_reads.size, total_bases), self._h)

    def device_coverage(self):
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib.drprg_hip_device_coverage(self._h, C.byref(a), C.byref(b)), self._h)
        return a.value, b.value

    def reset(self):
        _check(lib.drprg_hip_reset(self._h), self._h)

    # ---- depth cap (include/drprg_hip.h: drprg_hip_set_max_covg) -------------------------------
    def set_max_covg(self, max_covg):
        """`pandora --max-covg`: reads are accepted in order until (max_covg + 1) * genome_size bases have been mapped since the last
        reset; None, or anything from 2**32 - 1 up, switches the cap off (the default)"""
        _check(lib.drprg_hip_set_max_covg(self._h, 2 ** 64 - 1 if max_covg is None else int(max_covg)), self._h)

    def max_covg_info(self):
        out = (C.c_uint64 * 4)()
        _check(lib.drprg_hip_max_covg_info(self._h, out), self._h)
        return dict(reached=bool(out[0]), reads=int(out[1]), bases=int(out[2]), dropped=int(out[3]))

    # ---- reads that stay in HBM (include/drprg_hip.h: drprg_hip_keep_reads) --------------------
    def keep_reads(self, max_bytes):
        """map_fastx leaves the blocks it copies on the device (up to max_bytes per device; 0 switches it off)"""
        _check(lib.drprg_hip_keep_reads(self._h, int(max_bytes)), self._h)

    def map_resident(self, other):
        """maps the reads `other` keeps in HBM against this context's index (DependencyError with code -61 if it does not hold them all)"""
        _check(lib.drprg_hip_map_resident(self._h, other._h), self._h)

    def resident_info(self):
        out = (C.c_uint64 * 4)()
        _check(lib.drprg_hip_resident_info(self._h, out), self._h)
        return dict(complete=bool(out[0]), bytes=int(out[1]), blocks=int(out[2]), last_discover_from_hbm=bool(out[3]))

    # ---- random subsample of the resident sample (include/drprg_hip.h: drprg_hip_subsample) -----
    SUBSAMPLE_SEED = 1  # the executables' default --seed

    def subsample(self, target_bases, seed=SUBSAMPLE_SEED):
        """cuts the resident sample to about target_bases at random and maps the kept reads afresh (nothing happens when the sample holds
        no more than that); returns what was there and what is left"""
        out = (C.c_uint64 * 4)()
        _check(lib.drprg_hip_subsample(self._h, int(target_bases), int(seed) & (2 ** 64 - 1), out), self._h)
        return dict(reads_before=int(out[0]), bases_before=int(out[1]), reads_kept=int(out[2]), bases_kept=int(out[3]))

    def set_ordered_ingest(self, on):
        """map_fastx hands its blocks over in file order (what subsample()'s numbering needs of a file of more than one block)"""
        _check(lib.drprg_hip_set_ordered_ingest(self._h, 1 if on else 0), self._h)

    def subsample_flags(self, n_reads):
        """one byte per read of the sample as the last subsample() found it, 1 = kept (n_reads: how many it held)"""
        flags = np.zeros(int(n_reads), dtype=np.uint8)
        _check(lib.drprg_hip_subsample_flags(self._h, _ptr(flags), flags.size), self._h)
        return flags

    # ---- duplicate reads (include/drprg_hip.h: drprg_hip_dedup) -----------------------------------
    def dedup(self, key_bits=64):
        """drops every resident read that is identical to a read before it and maps the kept reads afresh (nothing happens when no read is
        dropped); returns what was there and what is left.  key_bits: how many low bits of the content key the sort sees (the result does
        not depend on it)"""
        out = (C.c_uint64 * 4)()
        _check(lib.drprg_hip_dedup(self._h, int(key_bits), out), self._h)
        return dict(reads_before=int(out[0]), bases_before=int(out[1]), reads_kept=int(out[2]), bases_kept=int(out[3]))

    def dedup_flags(self, n_reads):
        """one byte per read of the sample as the last dedup() found it, 1 = kept (n_reads: how many it held)"""
        flags = np.zeros(int(n_reads), dtype=np.uint8)
        _check(lib.drprg_hip_dedup_flags(self._h, _ptr(flags), flags.size), self._h)
        return flags

    def dedup_keys_device(self, d_words, d_offsets, n_reads, n_bases, d_npos, n_npos, d_keys, stream=None):
        """the content keys of a packed batch in device memory (addresses as integers; d_npos may be None when n_npos is 0) into
        d_keys (u64 per read)"""
        _check(lib.drprg_hip_dedup_keys_device(self._h, d_words, d_offsets, int(n_reads), int(n_bases), d_npos, int(n_npos), d_keys, stream), self._h)

    # ---- mate overlap (include/drprg_hip.h: drprg_hip_set_pair_overlap) --------------------------
    PAIR_COUNTS = ("pairs", "pairs_judged", "orphans", "pairs_too_long", "pairs_overlapping", "pairs_read_through", "bases_cut", "bases_clipped",
                   "reads_emptied", "reads", "bases_before", "bases_kept")

    def set_pair_overlap(self, min_overlap=30, error=0.05, clip=False):
        """the mate-overlap setting: the smallest overlap (8 .. 1024 columns with both bases known), the largest share of differing columns
        (0 .. 0.25, at most three places: error_milli below raises ValueError otherwise), and whether the second mate is clipped to what the first does not cover; min_overlap=0 clears it"""
        if not min_overlap:
            _check(lib.drprg_hip_set_pair_overlap(self._h, 0, 0, 0), self._h)
        else:
            _check(lib.drprg_hip_set_pair_overlap(self._h, int(min_overlap), self.error_milli(error), 1 if clip else 0), self._h)

    def begin_mates(self):
        """the files mapped from here on are side 2 of the sample's pairs"""
        _check(lib.drprg_hip_begin_mates(self._h), self._h)

    def pair_overlap(self):
        """cuts read-through adapters and (with clip) the second mate's share of the overlap off the resident pairs and maps the cut reads
        afresh (nothing happens when no read loses a base); returns the twelve counts"""
        out = (C.c_uint64 * 12)()
        _check(lib.drprg_hip_pair_overlap(self._h, out), self._h)
        return dict(zip(self.PAIR_COUNTS, (int(v) for v in out)))

    def pair_overlap_shifts(self, n_pairs):
        """per source pair the shift the last pair_overlap() chose (-2^31: none qualified, -2^31 + 1: not judged)"""
        d = np.zeros(int(n_pairs), dtype=np.int32)
        _check(lib.drprg_hip_pair_overlap_shifts(self._h, _ptr(d), d.size), self._h)
        return d

    def pair_overlap_info(self):
        out = (C.c_uint64 * 12)()
        _check(lib.drprg_hip_pair_overlap_info(self._h, out), self._h)
        return dict(zip(self.PAIR_COUNTS, (int(v) for v in out)))

    def pair_overlap_device(self, side_a, side_b, n_pairs, d_shift, d_keep_a, d_keep_b, stream=None):
        """the overlap kernel alone on two packed batches of n_pairs reads in device memory; a side is (d_words, d_offsets, n_bases,
        d_npos or None, n_npos), addresses as integers.  d_shift: i32 per pair, d_keep_a / d_keep_b: u64 per pair.  Returns the twelve counts"""
        out = (C.c_uint64 * 12)()
        (wa, oa, ba, pa, na), (wb, ob, bb, pb, nb) = side_a, side_b
        _check(lib.drprg_hip_pair_overlap_device(self._h, wa, oa, int(ba), pa, int(na), wb, ob, int(bb), pb, int(nb), int(n_pairs), d_shift, d_keep_a,
                                                 d_keep_b, out, stream), self._h)
        return dict(zip(self.PAIR_COUNTS, (int(v) for v in out)))

    # ---- mate merging (include/drprg_hip.h: drprg_hip_set_pair_merge) ----------------------------
    PAIR_MERGE_COUNTS = ("pairs_merged", "columns_both", "columns_agreeing", "columns_disagreeing", "columns_filled", "columns_unknown", "bases_merged",
                         "longest_merged")

    def set_pair_merge(self, on=True):
        """switches mate merging on (behind set_pair_overlap() without clip: pair_overlap() then merges every pair with a chosen shift into
        one read) or off"""
        _check(lib.drprg_hip_set_pair_merge(self._h, 1 if on else 0), self._h)

    def pair_merge_info(self):
        """the eight counts of the last pair_overlap() that merged"""
        out = (C.c_uint64 * 8)()
        _check(lib.drprg_hip_pair_merge_info(self._h, out), self._h)
        return dict(zip(self.PAIR_MERGE_COUNTS, (int(v) for v in out)))

    def pair_merge_device(self, side_a, side_b, n_pairs, d_shift, d_out_offsets, d_out_words, cap_words, d_out_npos, cap_npos, stream=None):
        """the overlap and the merge kernel alone on two packed batches of n_pairs reads in device memory, the sides as pair_overlap_device
        takes them.  d_shift: i32 per pair; the merged batch: d_out_offsets (u64[n_pairs + 1]), d_out_words (room for cap_words u32),
        d_out_npos (room for cap_npos u64, ascending).  Returns (the twelve counts, the eight counts, the length of the list)"""
        out12, out8, n_list = (C.c_uint64 * 12)(), (C.c_uint64 * 8)(), C.c_uint64(0)
        (wa, oa, ba, pa, na), (wb, ob, bb, pb, nb) = side_a, side_b
        _check(lib.drprg_hip_pair_merge_device(self._h, wa, oa, int(ba), pa, int(na), wb, ob, int(bb), pb, int(nb), int(n_pairs), d_shift, d_out_offsets,
                                               d_out_words, int(cap_words), d_out_npos, int(cap_npos), C.byref(n_list), out12, out8, stream), self._h)
        return (dict(zip(self.PAIR_COUNTS, (int(v) for v in out12))), dict(zip(self.PAIR_MERGE_COUNTS, (int(v) for v in out8))), int(n_list.value))

    # ---- duplicate pairs (include/drprg_hip.h: drprg_hip_set_dedup_pairs) ------------------------
    PAIR_DEDUP_COUNTS = ("units", "units_with_bases", "units_both_mates", "units_dropped", "reads_before", "bases_before", "reads_kept", "bases_kept")

    def set_dedup_pairs(self, on=True):
        """switches pair dedup on (before pair_overlap(), which then keeps the pairing of the resident reads) or off"""
        _check(lib.drprg_hip_set_dedup_pairs(self._h, 1 if on else 0), self._h)

    def dedup_pairs(self, key_bits=64):
        """drops every resident pair (or orphan) that is identical, mate by mate, to one before it and maps the kept reads afresh (nothing
        happens when no unit is dropped); returns the eight counts"""
        out = (C.c_uint64 * 8)()
        _check(lib.drprg_hip_dedup_pairs(self._h, int(key_bits), out), self._h)
        return dict(zip(self.PAIR_DEDUP_COUNTS, (int(v) for v in out)))

    def dedup_pairs_flags(self, n_reads):
        """one byte per read of the sample as the last dedup_pairs() found it, 1 = kept (n_reads: how many it held)"""
        flags = np.zeros(int(n_reads), dtype=np.uint8)
        _check(lib.drprg_hip_dedup_pairs_flags(self._h, _ptr(flags), flags.size), self._h)
        return flags

    def dedup_pairs_info(self):
        """the eight counts of the last dedup_pairs() and, under "levels", the 32 duplication levels"""
        out = (C.c_uint64 * 40)()
        _check(lib.drprg_hip_dedup_pairs_info(self._h, out), self._h)
        d = dict(zip(self.PAIR_DEDUP_COUNTS, (int(v) for v in out[:8])))
        d["levels"] = [int(v) for v in out[8:40]]
        return d

    def dedup_pairs_device(self, side_a, side_b, n_pairs, key_bits, d_keys, d_keep, d_copies, stream=None):
        """the stage's kernels alone on two packed batches of n_pairs reads in device memory; a side is (d_words, d_offsets, n_bases,
        d_npos or None, n_npos), addresses as integers.  d_keys: u64, d_keep: u8, d_copies: u32 per pair.  Returns the eight counts and "levels" """
        out = (C.c_uint64 * 40)()
        (wa, oa, ba, pa, na), (wb, ob, bb, pb, nb) = side_a, side_b
        _check(lib.drprg_hip_dedup_pairs_device(self._h, wa, oa, int(ba), pa, int(na), wb, ob, int(bb), pb, int(nb), int(n_pairs), int(key_bits), d_keys,
                                                d_keep, d_copies, out, stream), self._h)
        d = dict(zip(self.PAIR_DEDUP_COUNTS, (int(v) for v in out[:8])))
        d["levels"] = [int(v) for v in out[8:40]]
        return d

    # ---- read filter (include/drprg_hip.h: drprg_hip_set_read_filter) ---------------------------
    @staticmethod
    def qual_milli(min_qual):
        """a decimal mean quality (number or text, as --min-read-qual takes it) as thousandths"""
        from decimal import Decimal
        return int((Decimal(str(min_qual)) * 1000).to_integral_value()) if min_qual else 0

    def set_read_filter(self, min_len=0, max_len=0, min_qual=0):
        """from the next map_fastx on, reads shorter than min_len, longer than max_len (0: no bound) or of a mean quality below min_qual
        (a decimal Phred value, 0: no test) are dropped on the device before anything else sees them; all zero clears the filter"""
        _check(lib.drprg_hip_set_read_filter(self._h, int(min_len), int(max_len), self.qual_milli(min_qual)), self._h)

    def read_filter_info(self):
        out = (C.c_uint64 * 8)()
        _check(lib.drprg_hip_read_filter_info(self._h, out), self._h)
        names = ("reads_seen", "bases_seen", "dropped_short", "dropped_long", "dropped_low_qual", "reads_kept", "bases_kept", "T")
        return dict(zip(names, (int(x) for x in out)))

    def read_filter_device(self, d_qual, qual_bias, d_offsets, n_reads, n_bases, d_sums, d_flags, stream=None):
        """the filter alone on device buffers (addresses as integers; d_qual / d_sums may be None): returns (kept reads, kept bases, position
        + 1 of the first quality byte out of range or 0) -- and raises with code -84 when there is such a byte"""
        out = (C.c_uint64 * 4)()
        rc = lib.drprg_hip_read_filter_device(self._h, d_qual, int(qual_bias), d_offsets, int(n_reads), int(n_bases), d_sums, d_flags, out, stream)
        self.last_filter_out = tuple(int(x) for x in out)
        _check(rc, self._h)
        return self.last_filter_out[:3]

    # ---- read trimming (include/drprg_hip.h: drprg_hip_set_read_trim) --------------------------
    def set_read_trim(self, front=0, tail=0, qual=0, window=0):
        """from the next map_fastx on, every read loses `front` bases at its start and `tail` at its end, and -- qual != 0, a decimal Phred
        value -- what lies outside its first and last window of `window` bases (0: 4) with a mean quality of at least qual; the trimmed
        read is what everything behind the ingest sees; all zero clears the settings"""
        _check(lib.drprg_hip_set_read_trim(self._h, int(front), int(tail), self.qual_milli(qual), int(window)), self._h)

    def read_trim_info(self):
        out = (C.c_uint64 * 8)()
        _check(lib.drprg_hip_read_trim_info(self._h, out), self._h)
        names = ("reads_seen", "bases_seen", "reads_lost_base", "cut_front", "cut_tail", "qual_cut_front", "qual_cut_tail", "reads_emptied")
        return dict(zip(names, (int(x) for x in out)))

    def read_trim_device(self, d_qual, qual_bias, d_offsets, d_rev, n_reads, n_bases, d_begin, d_end, stream=None):
        """the trim kernels alone on device buffers (addresses as integers; d_qual may be None without a quality, d_rev may be None):
        d_begin / d_end (u64 per read) receive the kept ranges in read orientation; returns (kept bases, reads that lost a base, position + 1
        of the first quality byte out of range or 0) -- and raises with code -84 when there is such a byte"""
        out = (C.c_uint64 * 4)()
        rc = lib.drprg_hip_read_trim_device(self._h, d_qual, int(qual_bias), d_offsets, d_rev, int(n_reads), int(n_bases), d_begin, d_end, out, stream)
        self.last_trim_out = tuple(int(x) for x in out)
        _check(rc, self._h)
        return self.last_trim_out[:3]

    # ---- adapter trimming (include/drprg_hip.h: drprg_hip_set_adapters) -------------------------
    @staticmethod
    def error_milli(error):
        """a decimal error rate with at most three places (number or text, as --adapter-error takes it) as thousandths; ValueError otherwise"""
        from decimal import Decimal
        milli = Decimal(str(error)) * 1000
        if milli != milli.to_integral_value() or milli < 0:
            raise ValueError(f"an error rate is a decimal in [0, 0.5] with at most three places, not {error!r}")
        return int(milli)

    def set_adapters(self, seqs, error="0.1", min_overlap=0, front=(), indels=False):
        """from the next map_fastx on, every read is cut at the leftmost start at which one of `seqs` (1 to 4 sequences of 1 to 64 letters
        ACGT) matches with at most floor(c * error) substitutions over the c letters compared, c >= min_overlap (0: 3, or the shortest
        adapter's length); behind the crops and the quality trim; an empty list clears the settings.  indels=True: the indel rule
        (include/drprg_hip.h) -- an occurrence may carry insertions and deletions too, and `front` (0 to 4 sequences) names 5' adapters,
        which are cut off the reads' starts behind the 3' cut"""
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in (seqs or [])]
        arr = (C.c_char_p * max(len(seqs), 1))(*seqs)
        front = [s.encode() if isinstance(s, str) else bytes(s) for s in (front or [])]
        if not front and not indels:
            _check(lib.drprg_hip_set_adapters(self._h, arr, len(seqs), self.error_milli(error), int(min_overlap)), self._h)
            return
        arr5 = (C.c_char_p * max(len(front), 1))(*front)
        _check(lib.drprg_hip_set_adapters2(self._h, arr, len(seqs), arr5, len(front), self.error_milli(error), int(min_overlap), 1 if indels else 0), self._h)

    def adapter_trim_info(self):
        out = (C.c_uint64 * 5)()
        _check(lib.drprg_hip_adapter_trim_info(self._h, out), self._h)
        names = ("reads_seen", "bases_seen", "reads_cut", "bases_cut", "reads_emptied")
        return dict(zip(names, (int(x) for x in out)))

    def adapter_trim_device(self, d_text, d_words, d_npos, n_npos, d_offsets, n_reads, n_bases, d_begin, d_end, stream=None):
        """the adapter kernels alone on device buffers (addresses as integers): the bases as text (d_words None) or as packed words with
        their ascending position list (d_text None; d_npos may be None when n_npos is 0); d_begin / d_end (u64 per read) hold every read's
        range and d_end receives the cut ends; returns the call's (reads seen, bases seen, reads cut, bases cut, reads emptied)"""
        out = (C.c_uint64 * 5)()
        _check(lib.drprg_hip_adapter_trim_device(self._h, d_text, d_words, d_npos, int(n_npos), d_offsets, int(n_reads), int(n_bases), d_begin, d_end, out,
                                                 stream), self._h)
        return tuple(int(x) for x in out)

    def front_adapter_info(self):
        """the 5' side's counts since the last reset (bases_seen: behind the 3' cut)"""
        out = (C.c_uint64 * 5)()
        _check(lib.drprg_hip_front_adapter_info(self._h, out), self._h)
        names = ("reads_seen", "bases_seen", "reads_cut", "bases_cut", "reads_emptied")
        return dict(zip(names, (int(x) for x in out)))

    def adapter_trim_device2(self, d_text, d_words, d_npos, n_npos, d_offsets, n_reads, n_bases, d_begin, d_end, stream=None):
        """adapter_trim_device under whatever rule is set: d_begin receives the begins a 5' adapter moved; returns the call's ten counts,
        the 3' side's five and the 5' side's five"""
        out = (C.c_uint64 * 10)()
        _check(lib.drprg_hip_adapter_trim_device2(self._h, d_text, d_words, d_npos, int(n_npos), d_offsets, int(n_reads), int(n_bases), d_begin, d_end, out,
                                                  stream), self._h)
        return tuple(int(x) for x in out)

    # ---- poly tails (include/drprg_hip.h: drprg_hip_set_poly_trim) -----------------------------
    def set_poly_trim(self, letters="", min_len=10):
        """from the next map_fastx on, every read loses its longest suffix of at least min_len (2..255) bases that begins with one of
        `letters` (distinct letters of ACGT, e.g. "G") and holds at most min(n // 8, 5) other bases -- on the device, behind the crops, the
        quality trim and both adapter sides; "" or None clears it"""
        if letters and int(min_len) != min_len:
            raise ValueError(f"a tail's shortest length is a whole number from 2 to 255, not {min_len!r}")
        s = letters.encode() if isinstance(letters, str) else (bytes(letters) if letters else None)
        _check(lib.drprg_hip_set_poly_trim(self._h, s or None, int(min_len) if s else 0), self._h)

    def poly_trim_info(self):
        out = (C.c_uint64 * 5)()
        _check(lib.drprg_hip_poly_trim_info(self._h, out), self._h)
        names = ("reads_seen", "bases_seen", "reads_cut", "bases_cut", "reads_emptied")
        return dict(zip(names, (int(x) for x in out)))

    def poly_trim_device(self, d_text, d_words, d_npos, n_npos, d_offsets, n_reads, n_bases, d_begin, d_end, stream=None):
        """the tail cut alone on device buffers (addresses as integers): the buffers of adapter_trim_device; d_end receives the cut ends;
        returns the call's (reads seen, bases seen, reads cut, bases cut, reads emptied)"""
        out = (C.c_uint64 * 5)()
        _check(lib.drprg_hip_poly_trim_device(self._h, d_text, d_words, d_npos, int(n_npos), d_offsets, int(n_reads), int(n_bases), d_begin, d_end, out,
                                              stream), self._h)
        return tuple(int(x) for x in out)

    # ---- read complexity (include/drprg_hip.h: drprg_hip_set_min_complexity) -------------------
    def set_min_complexity(self, percent=0):
        """from the next map_fastx on, a read of L >= 2 bases is dropped when fewer than percent % (a whole number, 1..100) of its L - 1
        neighbouring base pairs differ -- on the device, behind the trim stage and the mask, on the reads the length and quality tests
        kept, in front of the decoy screen's verdict; 0 clears it"""
        if int(percent) != percent:
            raise ValueError(f"a complexity threshold is a whole percentage from 0 to 100, not {percent!r}")
        _check(lib.drprg_hip_set_min_complexity(self._h, int(percent)), self._h)

    def complexity_info(self):
        out = (C.c_uint64 * 4)()
        _check(lib.drprg_hip_complexity_info(self._h, out), self._h)
        names = ("reads_seen", "bases_seen", "reads_dropped", "bases_dropped")
        return dict(zip(names, (int(x) for x in out)))

    def complexity_device(self, d_text, d_words, d_npos, n_npos, d_offsets, n_reads, n_bases, d_diff, d_flags, stream=None):
        """the complexity kernels alone on device buffers (addresses as integers): the bases as for adapter_trim_device; d_diff (u32 per
        read, may be None) receives D, d_flags (u8 per read) 1 for a kept read; returns the call's (reads dropped, bases dropped)"""
        out = (C.c_uint64 * 2)()
        _check(lib.drprg_hip_complexity_device(self._h, d_text, d_words, d_npos, int(n_npos), d_offsets, int(n_reads), int(n_bases), d_diff, d_flags, out,
                                               stream), self._h)
        return tuple(int(x) for x in out)

    # ---- read statistics (include/drprg_hip.h: drprg_hip_set_read_stats) -----------------------
    @staticmethod
    def read_stats_layout():
        """the snapshot's layout as the library holds it (csrc/read_stats_words.h): words, the sections' offsets and sizes"""
        out = (C.c_uint64 * 13)()
        _check(lib.drprg_hip_read_stats_layout(out))
        names = ("words", "len_reads", "len_bases", "cyc_base", "cyc_qsum", "qual_hist", "readq_hist", "gc_hist", "len_bins", "cycles", "cols", "quals", "gc_bins")
        lay = dict(zip(names, (int(x) for x in out)))
        assert lay["words"] == int(lib.drprg_hip_read_stats_words())
        return lay

    @classmethod
    def read_stats_dict(cls, words):
        """a snapshot's words as a dict of numpy arrays (views of `words`): reads, bases, min_len, max_len, len_reads, len_bases,
        cyc_base [cycles + 1, 5] (A, C, G, T, U), cyc_qsum, qual_hist, readq_hist, gc_hist, and the flat `words`"""
        lay = cls.read_stats_layout()
        w = np.asarray(words, dtype=np.uint64)
        ncyc = lay["cycles"] + 1
        return {
            "words": w, "reads": int(w[0]), "bases": int(w[1]), "min_len": int(w[2]), "max_len": int(w[3]),
            "len_reads": w[lay["len_reads"]:lay["len_reads"] + lay["len_bins"]], "len_bases": w[lay["len_bases"]:lay["len_bases"] + lay["len_bins"]],
            "cyc_base": w[lay["cyc_base"]:lay["cyc_base"] + ncyc * lay["cols"]].reshape(ncyc, lay["cols"]),
            "cyc_qsum": w[lay["cyc_qsum"]:lay["cyc_qsum"] + ncyc], "qual_hist": w[lay["qual_hist"]:lay["qual_hist"] + lay["quals"]],
            "readq_hist": w[lay["readq_hist"]:lay["readq_hist"] + lay["quals"]], "gc_hist": w[lay["gc_hist"]:lay["gc_hist"] + lay["gc_bins"]],
        }

    def set_read_stats(self, mode=1):
        """from the next map_fastx on, every ingest block is counted on the device into the raw and the prepared snapshot: mode 1 with
        qualities (FASTA is an error then), 2 without the three quality sections, 0 off"""
        _check(lib.drprg_hip_set_read_stats(self._h, int(mode)), self._h)

    def read_stats_info(self, which=0, n_words=None):
        """the snapshot (0 raw, 1 prepared) as read_stats_dict gives it; n_words: the size of the buffer handed to the library"""
        n = int(lib.drprg_hip_read_stats_words()) if n_words is None else int(n_words)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        _check(lib.drprg_hip_read_stats_info(self._h, int(which), out.ctypes.data, n), self._h)
        return self.read_stats_dict(out)

    def read_stats_prepared_is_raw(self):
        rc = lib.drprg_hip_read_stats_prepared_is_raw(self._h)
        _check(min(rc, 0), self._h)
        return rc == 1

    def read_stats_device(self, d_text, d_words, d_npos, n_npos, d_qual, qual_bias, d_offsets, d_rev, n_reads, n_bases, d_flags=None, take=None, n_words=None,
                          stream=None):
        """the statistics kernels alone on device buffers (addresses as integers): the bases as text (d_words None) or packed words (d_text
        None) with their ascending position list; d_qual None: no quality section; d_rev, d_flags may be None; take: only reads below it
        count (None: all).  Returns the snapshot as read_stats_dict gives it; raises -84 for a quality byte out of range, -22 for offsets
        that do not ascend to n_bases or a buffer (n_words) that is too small"""
        n = int(lib.drprg_hip_read_stats_words()) if n_words is None else int(n_words)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        _check(lib.drprg_hip_read_stats_device(self._h, d_text, d_words, d_npos, int(n_npos), d_qual, int(qual_bias), d_offsets, d_rev, int(n_reads), int(n_bases),
                                               d_flags, int(n_reads if take is None else take), out.ctypes.data, n, stream), self._h)
        return self.read_stats_dict(out)

    def write_qc_json(self, path, sample=""):
        """the report --qc-json writes: both snapshots and every stage's counters, as JSON"""
        _check(lib.drprg_hip_write_qc_json(self._h, os.fsencode(path), sample.encode()), self._h)

    # ---- base masking (include/drprg_hip.h: drprg_hip_set_base_mask) ---------------------------
    def set_base_mask(self, min_qual=0):
        """from the next map_fastx on, every base whose Phred quality is below min_qual (a whole number, 1..93) becomes an unknown base on
        the device, behind the trim stage and in front of everything else: the run is that of a file with N in its place; 0 clears it"""
        if int(min_qual) != min_qual:
            raise ValueError(f"a base quality is a whole number from 0 to 93, not {min_qual!r}")
        _check(lib.drprg_hip_set_base_mask(self._h, int(min_qual)), self._h)

    def base_mask_info(self):
        out = (C.c_uint64 * 5)()
        _check(lib.drprg_hip_base_mask_info(self._h, out), self._h)
        names = ("reads_seen", "bases_seen", "reads_masked", "bases_masked", "bases_already_unknown")
        return dict(zip(names, (int(x) for x in out)))

    def base_mask_device(self, d_qual, qual_bias, d_offsets, d_rev, n_reads, n_bases, d_text, d_words, d_npos, n_npos, d_npos_out, npos_cap, stream=None):
        """the mask kernels alone on device buffers (addresses as integers), in place: the bases as text (d_words None) or as packed words
        (d_text None) with their ascending position list, which is only read; d_npos_out (u64 x npos_cap) receives the list behind the
        mask; d_rev may be None.  Returns (reads seen, bases seen, reads masked, bases masked, bases already unknown, new list length) --
        and raises with code -75 when npos_cap is too small, -84 for a quality byte out of range; last_mask_out holds the six words then"""
        out = (C.c_uint64 * 6)()
        rc = lib.drprg_hip_base_mask_device(self._h, d_qual, int(qual_bias), d_offsets, d_rev, int(n_reads), int(n_bases), d_text, d_words, d_npos, int(n_npos),
                                            d_npos_out, int(npos_cap), out, stream)
        self.last_mask_out = tuple(int(x) for x in out)
        _check(rc, self._h)
        return self.last_mask_out

    # ---- decoy screen (include/drprg_hip.h: drprg_hip_set_decoy) -------------------------------
    @staticmethod
    def frac_milli(frac):
        """a decimal fraction in (0, 1] with at most three places (number or text, as --decoy-min-frac takes it) as thousandths; 0 or None:
        the default; ValueError otherwise"""
        from decimal import Decimal
        if not frac:
            return 0
        milli = Decimal(str(frac)) * 1000
        if milli != milli.to_integral_value() or milli < 1 or milli > 1000:
            raise ValueError(f"a fraction is a decimal in (0, 1] with at most three places, not {frac!r}")
        return int(milli)

    def set_decoy(self, fasta_paths, k=0, min_frac=0, min_kmers=0):
        """from the next map_fastx on, a read is dropped when at least min_kmers (0: 1) of its k-mers (k 9..31, 0: 31) and at least the
        fraction min_frac (0: 0.5) of its valid k-mers are canonical k-mers of the 1 to 8 FASTA files; behind the trim stage and the length
        and quality tests; an empty list clears the set and frees the table"""
        paths = [os.fspath(p).encode() for p in (fasta_paths or [])]
        arr = (C.c_char_p * max(len(paths), 1))(*paths)
        _check(lib.drprg_hip_set_decoy(self._h, arr, len(paths), int(k), self.frac_milli(min_frac), int(min_kmers)), self._h)

    def decoy_info(self):
        out = (C.c_uint64 * 8)()
        _check(lib.drprg_hip_decoy_info(self._h, out), self._h)
        names = ("kmers", "slots", "reads_seen", "bases_seen", "reads_dropped", "bases_dropped", "valid", "hits")
        return dict(zip(names, (int(x) for x in out)))

    def decoy_lookup(self, kmers):
        """membership of k-mers (integers, 2 bits per base, A 0 C 1 G 2 T 3, first base high; either orientation) in the decoy set, probed
        on the device: one byte per k-mer"""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        found = np.zeros(kmers.size, dtype=np.uint8)
        _check(lib.drprg_hip_decoy_lookup(self._h, _ptr(kmers), kmers.size, _ptr(found)), self._h)
        return found

    def decoy_screen_device(self, d_text, d_words, d_npos, n_npos, d_offsets, n_reads, n_bases, d_valid, d_hits, d_flags, stream=None):
        """the screen kernels alone on device buffers (addresses as integers): the bases as for adapter_trim_device; d_valid / d_hits (u32
        per read, either may be None) receive V and H, d_flags (u8 per read) 1 for a kept read; returns the call's (reads dropped, bases
        dropped, sum of V, sum of H)"""
        out = (C.c_uint64 * 4)()
        _check(lib.drprg_hip_decoy_screen_device(self._h, d_text, d_words, d_npos, int(n_npos), d_offsets, int(n_reads), int(n_bases), d_valid, d_hits, d_flags,
                                                 out, stream), self._h)
        return tuple(int(x) for x in out)

    def select_reads(self, anchors, A, window_bytes=0):
        """the resident reads in which one of `anchors` (k-mers of A bases as integers, 2 bits per base, A 0 C 1 G 2 T 3, first base high)
        starts -- the selection discover_reads runs on the device (drprg_hip_select_reads); returns (bases u8, offsets u64, ids u64 =
        kept block << 32 | read in the block)"""
        anchors = np.ascontiguousarray(anchors, dtype=np.uint64)
        out = (C.c_uint64 * 2)()
        offsets = np.zeros(1, np.uint64)
        rc = lib.drprg_hip_select_reads(self._h, _ptr(anchors), anchors.size, int(A), int(window_bytes), None, 0, _ptr(offsets), None, 0, out)
        if rc == 0:  # nothing selected
            return np.zeros(0, np.uint8), offsets, np.zeros(0, np.uint64)
        if rc != -75:  # -EOVERFLOW: out holds the sizes needed
            _check(rc, self._h)
        n_reads, n_bases = int(out[0]), int(out[1])
        bases, offsets, ids = np.zeros(n_bases, np.uint8), np.zeros(n_reads + 1, np.uint64), np.zeros(n_reads, np.uint64)
        _check(lib.drprg_hip_select_reads(self._h, _ptr(anchors), anchors.size, int(A), int(window_bytes), _ptr(bases), n_bases, _ptr(offsets),
                                          _ptr(ids), n_reads, out), self._h)
        return bases, offsets, ids

    def counters(self):
        out = (C.c_uint64 * 8)()
        _check(lib.drprg_hip_counters(self._h, out), self._h)
        names = ("reads", "bases", "minimizers", "hits", "clusters_kept", "hits_kept", "kernel", "leftover_reads")
        return dict(zip(names, (int(x) for x in out)))

    # ---- genotyping ----------------------------------------------------------------------------
    def genotype(self, vcf_refs, out_vcf, sample="sample"):
        _check(lib.drprg_hip_genotype(self._h, os.fsencode(vcf_refs) if vcf_refs else None, os.fsencode(out_vcf),
                                      sample.encode()), self._h)
        gi = (C.c_uint32 * 4)()
        lib.drprg_hip_genotype_info(self._h, gi)
        return dict(exp_depth_covg=int(gi[0]), min_kmer_covg=int(gi[1]), loci_present=int(gi[2]), records=int(gi[3]))

    def coverage_model(self):
        """what estimate_parameters made of the coverage of the last genotype() (drprg_hip_coverage_model)"""
        out = (C.c_double * 12)()
        _check(lib.drprg_hip_coverage_model(self._h, out), self._h)
        names = ("exp_depth_covg", "binomial", "e_rate", "nb_p", "nb_r", "branch", "mean", "var", "reads_per_locus", "bin_p", "thresh",
                 "dropped_low_coverage")
        d = dict(zip(names, (float(x) for x in out)))
        for key in ("exp_depth_covg", "binomial", "branch", "reads_per_locus", "thresh", "dropped_low_coverage"):
            d[key] = int(d[key])
        return d

    def discover(self, vcf_refs, out_dir, sample="sample"):
        """candidate_regions.tsv + denovo_paths.txt ("0 loci": no local assembly) under out_dir; returns the regions"""
        n = C.c_uint32()
        _check(lib.drprg_hip_discover(self._h, os.fsencode(vcf_refs) if vcf_refs else None, os.fsencode(out_dir), sample.encode(),
                                      C.byref(n)), self._h)
        regions = []
        for line in open(os.path.join(out_dir, "candidate_regions.tsv")):
            if not line.startswith("#"):
                f = line.rstrip("\n").split("\t")
                regions.append(dict(locus=f[0], start=int(f[1]), end=int(f[2]), low_start=int(f[3]), low_end=int(f[4]),
                                    max_covg=int(f[5]), seq=f[6]))
        assert len(regions) == n.value
        return regions

    def discover_reads(self, reads, vcf_refs, out_dir, sample="sample", list_loci=True):
        """candidate regions + the pile-up of the reads over them; returns the novel variants [(locus, pos1, ref, alt, support, spanning)]"""
        out = (C.c_uint32 * 3)()
        _check(lib.drprg_hip_discover_reads(self._h, os.fsencode(reads), os.fsencode(vcf_refs) if vcf_refs else None, os.fsencode(out_dir),
                                            sample.encode(), 1 if list_loci else 0, out), self._h)
        variants = []
        for line in open(os.path.join(out_dir, "denovo_variants.tsv")):
            if not line.startswith("#"):
                f = line.rstrip("\n").split("\t")
                variants.append((f[0], int(f[1]), "" if f[2] == "." else f[2], "" if f[3] == "." else f[3], int(f[4]), int(f[5])))
        assert len(variants) == out[1]
        return variants

    def update_prg(self, out_prg):
        """the PRG file with the novel variants of the last discover_reads added as sites; returns how many were added"""
        n = C.c_uint32()
        _check(lib.drprg_hip_update_prg(self._h, os.fsencode(out_prg), C.byref(n)), self._h)
        return int(n.value)

    def update_prg_from_paths(self, denovo_paths, out_prg):
        """MakePrg::update (/root/reference/src/lib.rs:279-456) on a denovo_paths.txt -- this library's or pandora discover's own"""
        n = C.c_uint32()
        _check(lib.drprg_hip_update_prg_from_paths(self._h, os.fsencode(denovo_paths), os.fsencode(out_prg), C.byref(n)), self._h)
        return int(n.value)

    def save_coverage(self, path, tag):
        _check(lib.drprg_hip_save_coverage(self._h, os.fsencode(path), tag.encode()), self._h)

    def load_coverage(self, path, tag):
        """True if the cached vector belonged to this (PRG, reads, parameters) and is now installed"""
        rc = lib.drprg_hip_load_coverage(self._h, os.fsencode(path), tag.encode(), None)
        if rc == -2:
            return False
        _check(rc, self._h)
        return True

    def genotype_alleles(self, out_tsv):
        """per allele of the last genotype(): (chrom, pos, allele) -> global k-mer nodes its statistics were taken over"""
        _check(lib.drprg_hip_genotype_alleles(self._h, os.fsencode(out_tsv)), self._h)
        out = {}
        for line in open(out_tsv):
            if line.startswith("#"):
                continue
            chrom, pos, a, n, nodes = line.rstrip("\n").split("\t")
            out[(chrom, int(pos), int(a))] = np.array([int(x) for x in nodes.split(",") if x], dtype=np.int64)
        return out

    # ---- introspection -------------------------------------------------------------------------
    def filter_selfcheck(self):
        out = (C.c_uint64 * 8)()
        _check(lib.drprg_hip_filter_selfcheck(self._h, out), self._h)
        names = ("codes", "level0_false_negatives", "level12_false_negatives", "stage2_false_negatives", "level0_fill_permille",
                 "level12_fill_permille", "stage2_fill_permille", "shared_array_false_negatives")
        return dict(zip(names, (int(x) for x in out)))

    def table_tier(self):
        out = (C.c_uint64 * 6)()
        _check(lib.drprg_hip_device_tables(self._h, out), self._h)
        return dict(pbloom_words=int(out[0]), table_bytes=int(out[1]), lds_filter_bytes=int(out[2]), kernel=int(out[3]),
                    l2_filter_bytes=int(out[4]), sketch_form=int(out[5]))

    def export_index(self):
        """Flat index (sorted keys + CSR records) in the layout oracle/oracle.c consumes."""
        keys = np.zeros(self.n_keys, dtype=np.uint64)
        rec_off = np.zeros(self.n_keys + 1, dtype=np.uint32)
        rec_prg = np.zeros(self.n_records, dtype=np.uint32)
        rec_knode = np.zeros(self.n_records, dtype=np.uint32)
        rec_strand = np.zeros(self.n_records, dtype=np.uint8)
        min_path_len = np.zeros(self.n_prgs, dtype=np.uint32)
        knode_base = np.zeros(self.n_prgs + 1, dtype=np.uint32)
        _check(lib.drprg_hip_index_export(self._h, _ptr(keys), _ptr(rec_off), _ptr(rec_prg), _ptr(rec_knode), _ptr(rec_strand),
                                          _ptr(min_path_len), _ptr(knode_base)), self._h)
        return dict(keys=keys, rec_off=rec_off, rec_prg=rec_prg, rec_knode=rec_knode, rec_strand=rec_strand,
                    min_path_len=min_path_len, knode_base=knode_base)

    def prg_nodes(self, prg):
        """(starts, ends, n_sites) of the local graph of PRG `prg`"""
        n, ns = C.c_uint32(), C.c_uint32()
        _check(lib.drprg_hip_prg_nodes(self._h, prg, None, None, 0, C.byref(n), C.byref(ns)), self._h)
        starts = np.zeros(n.value, dtype=np.uint32)
        ends = np.zeros(n.value, dtype=np.uint32)
        _check(lib.drprg_hip_prg_nodes(self._h, prg, _ptr(starts), _ptr(ends), n.value, C.byref(n), C.byref(ns)), self._h)
        return starts, ends, int(ns.value)

    def filter_schedule(self):
        """sketch_filter_kernel's chunk schedule in the batch completed last and when its wave classes were through (include/drprg_hip.h)"""
        out = (C.c_uint64 * 20)()
        _check(lib.drprg_hip_filter_schedule(self._h, out), self._h)
        v = [int(x) for x in out]
        return {"form": "dynamic" if v[0] > 1 else "static", "rounds": v[0], "slices": v[1], "slices_per_workgroup": v[11], "round0_tiles_per_wave": v[2],
                "round0_class_shares_per_256": v[3:7], "chunk_tiles_per_round": [x for x in v[13:20] if x],
                "class_end_us": [round(x / 100.0, 1) for x in v[7:11]]}

    def buffer_info(self):
        """how often the candidate / hit buffers overflowed and the batch ran again, and their capacities in entries (include/drprg_hip.h)"""
        out = (C.c_uint64 * 6)()
        _check(lib.drprg_hip_buffer_info(self._h, out), self._h)
        return dict(filter_reruns=int(out[0]), direct_reruns=int(out[1]), hit_regrows=int(out[2]), lane_capacity=int(out[3]),
                    hit_capacity=int(out[4]))

    def kernel_timing(self, enable=True, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        _check(lib.drprg_hip_kernel_timing(self._h, 1 if enable else 0, 1 if reset else 0, C.byref(ms), C.byref(n)), self._h)
        return ms.value, int(n.value)


def allele_stats(fwd, rev, min_kmer_covg):
    """the product's per-allele statistics on raw k-mer coverages: ([MEAN_FWD, MEAN_REV, MED_FWD, MED_REV, SUM_FWD, SUM_REV], GAPS)"""
    fwd = np.ascontiguousarray(fwd, dtype=np.uint32)
    rev = np.ascontiguousarray(rev, dtype=np.uint32)
    out = np.zeros(6, np.uint32)
    gaps = C.c_double()
    _check(lib.drprg_hip_allele_stats(_ptr(fwd), _ptr(rev), len(fwd), min_kmer_covg, _ptr(out), C.byref(gaps)))
    return [int(x) for x in out], gaps.value


def genotype_site(mean_fwd, mean_rev, gaps, e, eps=0.01):
    """the product's likelihood / GT / GT_CONF of one site from its per-allele means and gaps"""
    mf = np.ascontiguousarray(mean_fwd, dtype=np.uint32)
    mr = np.ascontiguousarray(mean_rev, dtype=np.uint32)
    g = np.ascontiguousarray(gaps, dtype=np.float64)
    lik = np.zeros(len(mf), np.float64)
    gt, conf = C.c_int32(), C.c_double()
    _check(lib.drprg_hip_genotype_site(_ptr(mf), _ptr(mr), _ptr(g), len(mf), e, eps, _ptr(lik), C.byref(gt), C.byref(conf)))
    return lik, gt.value, conf.value


class Pandora:
    """In-process stand-in for struct Pandora (/root/reference/src/lib.rs:459-698)."""

    def __init__(self, device=0):
        self.device = device

    @staticmethod
    def _parse_args(args):
        """The argv drprg passes: -t T -w W -k K -c C [-I] [-K] (/root/reference/src/predict.rs:236-245), and --max-covg M (pandora's own
        default, 300, when it is not given; 4294967295 = no cap, what the reference passes in front of these)."""
        o = dict(threads=1, w=14, k=15, c=10, illumina=False, max_covg=300)
        it = iter([str(a) for a in args])
        for a in it:
            if a == "-t":
                o["threads"] = int(next(it))
            elif a == "-w":
                o["w"] = int(next(it))
            elif a == "-k":
                o["k"] = int(next(it))
            elif a == "-c":
                o["c"] = int(next(it))
            elif a == "-I":
                o["illumina"] = True
            elif a == "--max-covg":
                o["max_covg"] = int(next(it))
            elif a == "-K":
                pass
            else:
                raise DependencyError("ProcessError", f"unknown pandora option {a}", code=2)
        return o

    @staticmethod
    def _struct_args(args):
        """what struct Pandora puts in front of the caller's arguments before it spawns `pandora discover` / `pandora map`
        (/root/reference/src/lib.rs:533-534, :605-606): no depth cap.  A --max-covg among `args` comes later and wins, as on pandora's
        command line; without one discover_with / genotype_with map every read, like the struct they stand in for -- _parse_args' own
        default (300) is that of the bare `pandora` command, which these two never run bare."""
        return ["--max-covg", "4294967295"] + [str(a) for a in args]

    def index_with(self, prg_path, args=()):
        """Pandora::index_with, /root/reference/src/lib.rs:479-510."""
        o = self._parse_args(args)
        _check(lib.drprg_hip_index(os.fsencode(prg_path), o["w"], o["k"], o["threads"]))

    def _mapped_context(self, prg, reads, args):
        o = self._parse_args(args)
        ctx = Context(prg, o["w"], o["k"], device=self.device)
        ctx.set_opts(illumina=o["illumina"], min_cluster_size=o["c"], genome_size=MTB_GENOME_SIZE)
        ctx.set_max_covg(o["max_covg"])
        ctx.map_fastx(reads)
        return ctx

    @staticmethod
    def _run_tag(prg, reads, args):
        """identifies (PRG file, reads file, mapping parameters): what a cached coverage vector belongs to"""
        def stamp(p):
            st = os.stat(p)
            return f"{os.path.realpath(p)}:{st.st_size}:{st.st_mtime_ns}"
        # (the depth cap by its value, given or not: a vector mapped under one cap is not another cap's)
        rest, it = [], iter(str(a) for a in args)
        for a in it:
            if a == "--max-covg":
                next(it, None)
            elif a != "-K":
                rest.append(a)
        return "|".join([stamp(prg), stamp(reads)] + rest + [f"M{Pandora._parse_args(args)['max_covg']}"])

    COVERAGE_CACHE = ".drprg_hip_coverage"

    def discover_with(self, prg, query_idx, outdir, args=(), list_loci=False):
        """Pandora::discover_with, /root/reference/src/lib.rs:513-578.  Returns the denovo_paths.txt path.

        The mapping half runs (its coverage vector is kept under `outdir` for the genotype_with call that follows), candidate
        regions go to candidate_regions.tsv, and the reads are piled up over them: novel variants go to
        denovo_variants.tsv.  list_loci=True also lists them in denovo_paths.txt (the caller's make_prg update then runs on it;
        the layout follows the one example in the reference tree and could not be tried on make_prg here); the default keeps
        "0 loci with denovo variants"."""
        import warnings
        os.makedirs(outdir, exist_ok=True)
        args = self._struct_args(args)
        with open(query_idx) as fh:
            sample, reads = fh.readline().split()[:2]
        with self._mapped_context(prg, reads, args) as ctx:
            ctx.set_threads(self._parse_args(args)["threads"])
            self.novel_variants = ctx.discover_reads(reads, None, outdir, sample, list_loci=list_loci)
            ctx.save_coverage(os.path.join(outdir, self.COVERAGE_CACHE), self._run_tag(prg, reads, args))
        if self.novel_variants and not list_loci:
            warnings.warn(f"discover: {len(self.novel_variants)} novel variant(s) found (denovo_variants.tsv) but not listed in "
                          "denovo_paths.txt: the PRG will not be updated")
        path = os.path.join(outdir, "denovo_paths.txt")
        if not os.path.exists(path):
            raise DependencyError("MissingExpectedOutput", path)
        return path

    def genotype_with(self, prg, vcf_ref, reads, outdir, args=()):
        """Pandora::genotype_with, /root/reference/src/lib.rs:580-642.  If discover_with left this run's coverage vector
        under <outdir>/discover (where drprg puts it, /root/reference/src/predict.rs:248), the reads are not mapped again."""
        os.makedirs(outdir, exist_ok=True)
        args = self._struct_args(args)
        o = self._parse_args(args)
        cache = os.path.join(outdir, "discover", self.COVERAGE_CACHE)
        ctx = Context(prg, o["w"], o["k"], device=self.device)
        with ctx:
            ctx.set_opts(illumina=o["illumina"], min_cluster_size=o["c"], genome_size=MTB_GENOME_SIZE)
            ctx.set_max_covg(o["max_covg"])
            self.reused_discover_coverage = os.path.exists(cache) and ctx.load_coverage(cache, self._run_tag(prg, reads, args))
            if not self.reused_discover_coverage:
                ctx.map_fastx(reads)
            ctx.genotype(vcf_ref, os.path.join(outdir, self.vcf_filename()))

    @staticmethod
    def vcf_filename():
        """/root/reference/src/lib.rs:644-646"""
        return "pandora_genotyped.vcf"

    @staticmethod
    def list_prgs_with_novel_variants(denovo_file):
        """/root/reference/src/lib.rs:648-697"""
        try:
            contents = open(denovo_file).read()
        except OSError:
            raise DependencyError("NovelVariantParsingError", f"Unable to read {denovo_file!r}")
        m = re.search(r"\n(?P<num>\d+) loci with denovo variants\n", contents)
        if not m:
            raise DependencyError("NovelVariantParsingError", "Unable to find line describing the number of novel variants")
        expected = int(m.group("num"))
        genes, prev = [], ""
        for line in contents.splitlines():
            if line.endswith("nodes"):
                genes.append(prev)
            prev = line
        if len(genes) != expected:
            raise DependencyError("NovelVariantParsingError",
                                  f"Expected {expected} genes with novel variants, but found {len(genes)}")
        return genes


def pack_reads(bases):
    """host helper: uint8 ASCII bases -> (uint32 words, uint64 ascending positions of the bases that are not ACGTacgt)"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    words = np.zeros((bases.size + 15) // 16, dtype=np.uint32)
    cap = 1024
    while True:
        npos = np.zeros(cap, dtype=np.uint64)
        n = C.c_uint64()
        rc = lib.drprg_hip_pack_reads(_ptr(bases), bases.size, _ptr(words), _ptr(npos), cap, C.byref(n))
        if rc == 0:
            return words, npos[:n.value].copy()
        if rc != -75:  # -EOVERFLOW: n holds the number needed
            _check(rc)
        cap = int(n.value)
