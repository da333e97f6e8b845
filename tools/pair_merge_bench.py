"""Mate merging (DESIGN.md section 4 "Mate merging"): what the merge kernel adds to the overlap kernel, and what the whole resident call costs
beside the clip.  The input is tools/pair_overlap_bench.py's case two: N pairs of 150-base mates as two packed batches, half of them
overlapping by 50 bases, 5 % reading through (an insert of 120 bases), the rest independent.
  python tools/pair_merge_bench.py [pairs] [resident pairs]
Device entries, in one session on the same input: drprg_hip_pair_overlap_device, then drprg_hip_pair_merge_device (the same kernels, then
the lengths, the scan of the offsets, two memsets, the merge kernel, the count of the unknown bases and the read-backs) between two events.
Then the whole drprg_hip_pair_overlap call on a resident sample of `resident pairs` pairs (default 2 M; 0 skips the leg), mapped from two
FASTQ files in the page cache: wall time of the call alone, with --pair-merge and with --pair-clip-overlap.  Medians of three.  Reads
nothing outside the repository."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drprg_amd import Context, synth  # noqa: E402
from pair_overlap_bench import READ_LEN, mates, median3, packed_side, write_fastq  # noqa: E402


def kernel_leg(ctx, n_pairs):
    d_o = torch.from_numpy(np.arange(n_pairs + 1, dtype=np.int64) * READ_LEN).cuda()
    d_s = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
    d_ka, d_kb = torch.empty(n_pairs, dtype=torch.int64, device="cuda"), torch.empty(n_pairs, dtype=torch.int64, device="cuda")
    a, b = mates(2)
    (d_wa, n_bases), (d_wb, _) = packed_side(ctx, a, n_pairs), packed_side(ctx, b, n_pairs)
    sa, sb = (d_wa.data_ptr(), d_o.data_ptr(), n_bases, None, 0), (d_wb.data_ptr(), d_o.data_ptr(), n_bases, None, 0)
    cap_words, cap_npos = (2 * n_bases + 15) // 16, 1 << 20
    d_oo = torch.empty(n_pairs + 1, dtype=torch.int64, device="cuda")
    d_ow = torch.empty(cap_words, dtype=torch.int32, device="cuda")
    d_on = torch.empty(cap_npos, dtype=torch.int64, device="cuda")
    print(f"pairs={n_pairs} bases={2 * n_bases}")
    ctx.set_pair_merge(False)
    med0, lo, hi, out = median3(lambda: ctx.pair_overlap_device(sa, sb, n_pairs, d_s.data_ptr(), d_ka.data_ptr(), d_kb.data_ptr()))
    print(f"pair_overlap_device: median {med0:.3f} ms (min {lo:.3f}, max {hi:.3f}); overlapping={out['pairs_overlapping']}")
    ctx.set_pair_merge(True)
    med1, lo, hi, out = median3(lambda: ctx.pair_merge_device(sa, sb, n_pairs, d_s.data_ptr(), d_oo.data_ptr(), d_ow.data_ptr(), cap_words, d_on.data_ptr(), cap_npos))
    print(f"pair_merge_device:   median {med1:.3f} ms (min {lo:.3f}, max {hi:.3f}); the merge adds {med1 - med0:.3f} ms; merged={out[1]['pairs_merged']} "
          f"bases_merged={out[1]['bases_merged']} columns_both={out[1]['columns_both']} columns_disagreeing={out[1]['columns_disagreeing']} listed={out[2]}")
    ctx.set_pair_merge(False)


def resident_leg(ctx, n_pairs):
    a, b = mates(2)
    d = tempfile.mkdtemp(prefix="pair_merge_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    r1, r2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    write_fastq(r1, a, n_pairs)
    write_fastq(r2, b, n_pairs)
    ctx.set_threads(16)
    ctx.set_ordered_ingest(True)
    ctx.set_input_format(True)
    ctx.keep_reads(8 << 30)
    try:
        for what in ("merge", "clip"):
            ctx.set_pair_merge(False)
            ctx.set_pair_overlap(30, "0.05", what == "clip")
            ctx.set_pair_merge(what == "merge")
            times = []
            for rep in range(4):
                ctx.reset()
                ctx.map_fastx(r1)
                ctx.begin_mates()
                ctx.map_fastx(r2)
                ctx.counters()
                t0 = time.perf_counter()
                out = ctx.pair_overlap()
                ctx.counters()
                times.append(time.perf_counter() - t0)
            t = sorted(times[1:])
            print(f"pair_overlap on a resident sample, {what}: median {t[1] * 1e3:.1f} ms (min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}) of 3, {n_pairs} pairs; "
                  f"overlapping={out['pairs_overlapping']} bases_clipped={out['bases_clipped']} bases_kept={out['bases_kept']} "
                  f"(the call holds the compaction of every block and the fresh mapping of the reads)")
    finally:
        os.remove(r1)
        os.remove(r2)
        os.rmdir(d)


def main():
    n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
    n_resident = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
    tmp = tempfile.mkdtemp(prefix="pair_merge_bench_")
    prg = os.path.join(tmp, "dr.prg")
    synth.small_panel(seed=42).write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_opts(illumina=True, genome_size=20000)
    ctx.set_pair_overlap(30, "0.05", False)
    kernel_leg(ctx, n_pairs)
    if n_resident:
        resident_leg(ctx, n_resident)
    ctx.close()


if __name__ == "__main__":
    main()
