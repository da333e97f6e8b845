"""The mate-overlap kernels (DESIGN.md section 4 "Mate overlap"): N pairs of 150-base mates as two packed batches (random letters; made on
the host in a piece of 100 000 pairs that repeats), one call of drprg_hip_pair_overlap_device between two events -- the memsets, the two
small kernels that find the mates, the overlap kernel, the copies and the read-back.  Case one: no pair overlaps (independent mates).  Case
two: half the pairs overlap by 50 bases, 5 % read through (an insert of 120 bases), the rest do not overlap.  Beside case one the yardstick
of the same session for "one pass over the packed bases": the dedup key kernel over the same two batches (drprg_hip_dedup_keys_device).
  python tools/pair_overlap_bench.py [pairs] [resident pairs]
Then the whole drprg_hip_pair_overlap call on a resident sample of `resident pairs` pairs of case two (default 2 M; 0 skips the leg), mapped
from two FASTQ files in the page cache: wall time of the call alone, with and without --pair-clip-overlap.  Medians of three.  Reads nothing
outside the repository."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drprg_amd import Context, synth  # noqa: E402

READ_LEN, PIECE = 150, 100_000
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.zeros(256, np.uint8)
_COMP[list(b"ACGT")] = list(b"TGCA")


def mates(case, seed=5):
    """PIECE pairs as two (PIECE, READ_LEN) byte matrices"""
    rng = np.random.default_rng(seed)
    a, b = rng.choice(_ACGT, size=(PIECE, READ_LEN)), rng.choice(_ACGT, size=(PIECE, READ_LEN))
    if case == 2:
        mol = rng.choice(_ACGT, size=(PIECE, 2 * READ_LEN))
        what = rng.random(PIECE)
        for lo, hi, ins in ((0.0, 0.5, 2 * READ_LEN - 50), (0.5, 0.55, 120)):
            rows = np.flatnonzero((what >= lo) & (what < hi))
            n = min(ins, READ_LEN)
            a[rows, :n] = mol[rows, :n]
            b[rows, :n] = _COMP[mol[rows, ins - n:ins][:, ::-1]]
    return a, b


def median3(call, reps=3):
    times, out = [], None
    for _ in range(reps + 1):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        x.record()
        out = call()
        y.record()
        torch.cuda.synchronize()
        times.append(x.elapsed_time(y))
    t = sorted(times[1:])  # (the first call allocates)
    return t[len(t) // 2], t[0], t[-1], out


def packed_side(ctx, piece, n_pairs):
    n_bases = n_pairs * READ_LEN
    text = np.zeros(n_bases + 64, np.uint8)
    text[:n_bases] = np.resize(piece.reshape(-1), n_bases)
    d_t = torch.from_numpy(text).cuda()
    d_w = torch.empty((n_bases + 15) // 16 + 16, dtype=torch.int32, device="cuda")
    d_np = torch.empty(1024, dtype=torch.int64, device="cuda")
    assert ctx.pack_device(d_t.data_ptr(), n_bases, d_w.data_ptr(), d_np.data_ptr(), 1024) == 0
    del d_t
    return d_w, n_bases


def kernel_leg(ctx, n_pairs):
    d_o = torch.from_numpy(np.arange(n_pairs + 1, dtype=np.int64) * READ_LEN).cuda()
    d_s = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
    d_ka, d_kb = torch.empty(n_pairs, dtype=torch.int64, device="cuda"), torch.empty(n_pairs, dtype=torch.int64, device="cuda")
    d_k = torch.empty(n_pairs, dtype=torch.int64, device="cuda")
    print(f"pairs={n_pairs} bases={2 * n_pairs * READ_LEN}")
    for case in (1, 2):
        a, b = mates(case)
        (d_wa, n_bases), (d_wb, _) = packed_side(ctx, a, n_pairs), packed_side(ctx, b, n_pairs)
        sa, sb = (d_wa.data_ptr(), d_o.data_ptr(), n_bases, None, 0), (d_wb.data_ptr(), d_o.data_ptr(), n_bases, None, 0)
        if case == 1:
            def keys():
                ctx.dedup_keys_device(d_wa.data_ptr(), d_o.data_ptr(), n_pairs, n_bases, None, 0, d_k.data_ptr())
                ctx.dedup_keys_device(d_wb.data_ptr(), d_o.data_ptr(), n_pairs, n_bases, None, 0, d_k.data_ptr())
            med, lo, hi, _ = median3(keys)
            print(f"dedup_keys_device on both batches (the yardstick): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
        med, lo, hi, out = median3(lambda: ctx.pair_overlap_device(sa, sb, n_pairs, d_s.data_ptr(), d_ka.data_ptr(), d_kb.data_ptr()))
        print(f"pair_overlap_device case {case}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {n_pairs / med / 1e3:.2f} M pairs/s; "
              f"overlapping={out['pairs_overlapping']} read_through={out['pairs_read_through']} bases_cut={out['bases_cut']}")
        del d_wa, d_wb
        torch.cuda.empty_cache()


def write_fastq(path, piece, n_reads):
    rec = np.empty((n_reads, 3 + READ_LEN + 3 + READ_LEN + 1), dtype=np.uint8)
    rec[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + READ_LEN] = np.resize(piece, (n_reads, READ_LEN))
    rec[:, 3 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + READ_LEN:6 + 2 * READ_LEN] = ord("I")
    rec[:, -1] = ord("\n")
    rec.tofile(path)


def resident_leg(ctx, n_pairs):
    a, b = mates(2)
    d = tempfile.mkdtemp(prefix="pair_overlap_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    r1, r2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    write_fastq(r1, a, n_pairs)
    write_fastq(r2, b, n_pairs)
    ctx.set_threads(16)
    ctx.set_ordered_ingest(True)
    ctx.set_input_format(True)
    ctx.keep_reads(8 << 30)
    try:
        for clip in (False, True):
            ctx.set_pair_overlap(30, "0.05", clip)
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
            print(f"pair_overlap on a resident sample, clip {'on' if clip else 'off'}: median {t[1] * 1e3:.1f} ms (min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}) of 3, "
                  f"{n_pairs} pairs; overlapping={out['pairs_overlapping']} bases_cut={out['bases_cut']} bases_clipped={out['bases_clipped']} "
                  f"(the call holds the compaction of every block and the fresh mapping of the cut reads)")
    finally:
        os.remove(r1)
        os.remove(r2)
        os.rmdir(d)


def main():
    n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
    n_resident = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
    tmp = tempfile.mkdtemp(prefix="pair_overlap_bench_")
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
