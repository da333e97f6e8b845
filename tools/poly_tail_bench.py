"""poly_tail_kernel and read_diff_kernel on one block (DESIGN.md section 4 "Poly tails and read complexity"): N reads of 150 bases (random,
65 % GC; made on the host in a piece of 100 000 reads that repeats), as text and as packed words, in turn, for four cases:
  the tail cut (S = {G}, M = 10) with no G tail, and with tails of 20 to 100 G on 5 % of the reads;
  the pair count and its verdict (P = 30) with nothing dropped, and with 1 % of the reads all G.
Prints the time of each call of drprg_hip_poly_trim_device / drprg_hip_complexity_device between two events: the memsets, the kernel(s)
and the read-back.  The ends are put back before every call.
  python tools/poly_tail_bench.py [reads] [launches] [e2e reads]
Then, end to end: `e2e reads` reads (default 2 M; 0 skips the leg) of the 5 % / 1 % mixture as FASTQ text in the page cache, the wall time
of drprg_hip_map_fastx with and without the two settings, ASCII and packed transport, median of three."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drprg_amd import Context, synth  # noqa: E402

M, P, READ_LEN, PIECE = 10, 30, 150, 100_000


def piece(tail_share, dark_share, seed):
    """PIECE reads of READ_LEN random bases at 65 % GC; a share of them ends in 20 to 100 G, a share is all G"""
    rng = np.random.default_rng(seed)
    reads = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(PIECE, READ_LEN), p=[0.175, 0.325, 0.325, 0.175])
    for i in np.flatnonzero(rng.random(PIECE) < tail_share):
        reads[i, READ_LEN - int(rng.integers(20, 101)):] = ord("G")
    reads[rng.random(PIECE) < dark_share] = ord("G")
    return reads


def on_device(reads, n_reads):
    out = np.zeros(n_reads * READ_LEN + 64, dtype=np.uint8)
    out[:n_reads * READ_LEN] = np.resize(reads.reshape(-1), n_reads * READ_LEN)
    return torch.from_numpy(out).cuda()


def timed(call, launches, before=None):
    times, out = [], None
    for _ in range(launches + 1):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    t = sorted(times[1:])  # (the first call allocates)
    return t[len(t) // 2], t[0], t[-1], out


def kernel_leg(ctx, n_reads, launches):
    n_bases = n_reads * READ_LEN
    d_o = torch.from_numpy(np.arange(n_reads + 1, dtype=np.int64) * READ_LEN).cuda()
    d_begin = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    d_end0 = torch.full((n_reads,), READ_LEN, dtype=torch.int64, device="cuda")
    d_end = torch.empty_like(d_end0)
    d_flags = torch.empty(n_reads, dtype=torch.uint8, device="cuda")
    d_w = torch.empty((n_bases + 15) // 16 + 16, dtype=torch.int32, device="cuda")
    print(f"reads={n_reads} bases={n_bases} launches={launches} S=G M={M} P={P}")
    for what, tail_share, dark_share in (("no tail", 0.0, 0.0), ("tails on 5 %", 0.05, 0.0), ("nothing dropped", 0.0, 0.0), ("1 % all G", 0.0, 0.01)):
        d_t = on_device(piece(tail_share, dark_share, 7), n_reads)
        assert ctx.pack_device(d_t.data_ptr(), n_bases, d_w.data_ptr(), None, 0) == 0
        for form, text, words in (("text", d_t.data_ptr(), None), ("packed", None, d_w.data_ptr())):
            if what in ("no tail", "tails on 5 %"):
                med, lo, hi, out = timed(lambda: ctx.poly_trim_device(text, words, None, 0, d_o.data_ptr(), n_reads, n_bases, d_begin.data_ptr(), d_end.data_ptr()),
                                         launches, lambda: d_end.copy_(d_end0))
                print(f"poly_trim_device {form}, {what}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {n_bases / med / 1e9:.3f} T bases/s; "
                      f"reads_cut={out[2]} bases_cut={out[3]} reads_emptied={out[4]}")
            else:
                med, lo, hi, out = timed(lambda: ctx.complexity_device(text, words, None, 0, d_o.data_ptr(), n_reads, n_bases, None, d_flags.data_ptr()), launches)
                print(f"complexity_device {form}, {what}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {n_bases / med / 1e9:.3f} T bases/s; "
                      f"reads_dropped={out[0]} bases_dropped={out[1]}")
        del d_t


def e2e_leg(ctx, n_reads):
    gen = synth.HaplotypeGenomes(synth.small_panel(seed=42), genome_size=20000, n_hap=4)
    bases, _ = synth.sample_short_reads(gen, n_reads, seed=1)
    reads = bases.reshape(n_reads, READ_LEN).copy()
    rng = np.random.default_rng(3)
    for i in np.flatnonzero(rng.random(n_reads) < 0.05):
        reads[i, READ_LEN - int(rng.integers(20, 101)):] = ord("G")
    reads[rng.random(n_reads) < 0.01] = ord("G")
    rec = np.empty((n_reads, 3 + READ_LEN + 3 + READ_LEN + 1), dtype=np.uint8)
    rec[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + READ_LEN] = reads
    rec[:, 3 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + READ_LEN:6 + 2 * READ_LEN] = 35 + 33
    rec[:, -1] = ord("\n")
    d = tempfile.mkdtemp(prefix="poly_tail_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    fq = os.path.join(d, "reads.fq")
    rec.tofile(fq)
    ctx.set_threads(16)
    try:
        for packed in (False, True):
            for on in (False, True, False, True):
                ctx.set_input_format(packed)
                ctx.set_poly_trim("G" if on else "", M)
                ctx.set_min_complexity(P if on else 0)
                times = []
                for rep in range(4):
                    ctx.reset()
                    t0 = time.perf_counter()
                    ctx.map_fastx(fq)
                    ctx.counters()
                    times.append(time.perf_counter() - t0)
                t = sorted(times[1:])
                print(f"map_fastx {'packed' if packed else 'ascii'} {'--poly-tail G --min-complexity 30' if on else 'neither flag'}: median {t[1] * 1e3:.1f} ms "
                      f"(min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}) of 3, {n_reads} reads; reads_cut={ctx.poly_trim_info()['reads_cut']} "
                      f"reads_dropped={ctx.complexity_info()['reads_dropped']}")
    finally:
        os.remove(fq)
        os.rmdir(d)


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    n_e2e = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000_000
    tmp = tempfile.mkdtemp(prefix="poly_tail_bench_")
    prg = os.path.join(tmp, "dr.prg")
    synth.small_panel(seed=42).write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_opts(illumina=True, genome_size=20000)
    ctx.set_poly_trim("G", M)
    ctx.set_min_complexity(P)
    kernel_leg(ctx, n_reads, launches)
    torch.cuda.empty_cache()
    if n_e2e:
        e2e_leg(ctx, n_e2e)
    ctx.close()


if __name__ == "__main__":
    main()
