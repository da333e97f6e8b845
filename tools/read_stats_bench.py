"""The read-statistics kernels on one block (DESIGN.md section 4 "Read statistics"): N reads of 150 bases (random, 65 % GC, 2 % N; NovaSeq-like
qualities of four values; made on the host in a piece of 100 000 reads that repeats), as text and as packed words, with and without
qualities: the raw snapshot alone, and the raw one plus the prepared one (keep flags that drop every tenth read, `take` at 95 % of the block).
Beside them the yardstick of the same session: the mask kernel on the same bytes with nothing masked (drprg_hip_base_mask_device, Q = 2).
Prints the time of each call between two events: the memsets, the kernels and the read-back.
  python tools/read_stats_bench.py [reads] [launches] [e2e reads]
Then, end to end: `e2e reads` reads (default 2 M; 0 skips the leg) as FASTQ text in the page cache, the wall time of drprg_hip_map_fastx
without the setting, with it, and with it without qualities, ASCII and packed transport, median of three.  Reads nothing outside the repository."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drprg_amd import Context, synth  # noqa: E402

READ_LEN, PIECE = 150, 100_000
QUALS = np.array([2, 12, 23, 37], dtype=np.uint8)


def on_device(piece, n, pad=64):
    out = np.zeros(n + pad, dtype=np.uint8)
    out[:n] = np.resize(piece.reshape(-1), n)
    return torch.from_numpy(out).cuda()


def timed(call, launches):
    times, out = [], None
    for _ in range(launches + 1):
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
    rng = np.random.default_rng(7)
    reads = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=(PIECE, READ_LEN), p=[0.1715, 0.3185, 0.3185, 0.1715, 0.02])
    quals = rng.choice(QUALS, size=(PIECE, READ_LEN), p=[0.01, 0.03, 0.11, 0.85])
    d_t, d_q = on_device(reads, n_bases), on_device(quals, n_bases)
    d_o = torch.from_numpy(np.arange(n_reads + 1, dtype=np.int64) * READ_LEN).cuda()
    d_w = torch.empty((n_bases + 15) // 16 + 16, dtype=torch.int32, device="cuda")
    cap = n_bases // 40 + 1024
    d_np = torch.empty(cap, dtype=torch.int64, device="cuda")
    n_npos = ctx.pack_device(d_t.data_ptr(), n_bases, d_w.data_ptr(), d_np.data_ptr(), cap)
    d_np2 = torch.empty(cap, dtype=torch.int64, device="cuda")
    flags = np.ones(n_reads, dtype=np.uint8)
    flags[::10] = 0
    d_f = torch.from_numpy(flags).cuda()
    take = n_reads * 95 // 100
    print(f"reads={n_reads} bases={n_bases} launches={launches} listed positions={n_npos}")
    for form, text, words, npos, nn in (("text", d_t.data_ptr(), None, None, 0), ("packed", None, d_w.data_ptr(), d_np.data_ptr(), n_npos)):
        med, lo, hi, out = timed(lambda: ctx.base_mask_device(d_q.data_ptr(), 0, d_o.data_ptr(), None, n_reads, n_bases, text, words, npos, nn, d_np2.data_ptr(), cap),
                                 launches)
        print(f"base_mask_device {form}, nothing masked (the yardstick): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {n_bases / med / 1e9:.3f} T bases/s; "
              f"bases_masked={out[3]}")
        for qual in (d_q.data_ptr(), None):
            def raw():
                return ctx.read_stats_device(text, words, npos, nn, qual, 0, d_o.data_ptr(), None, n_reads, n_bases)

            def both():
                raw()
                return ctx.read_stats_device(text, words, npos, nn, qual, 0, d_o.data_ptr(), None, n_reads, n_bases, d_f.data_ptr(), take)

            for what, call in (("raw", raw), ("raw + prepared", both)):
                med, lo, hi, out = timed(call, launches)
                print(f"read_stats_device {form}, {'with' if qual else 'without'} qualities, {what}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = "
                      f"{n_bases / med / 1e9:.3f} T bases/s; reads={out['reads']} bases={out['bases']}")


def e2e_leg(ctx, n_reads):
    gen = synth.HaplotypeGenomes(synth.small_panel(seed=42), genome_size=20000, n_hap=4)
    bases, _ = synth.sample_short_reads(gen, n_reads, seed=1)
    rng = np.random.default_rng(3)
    rec = np.empty((n_reads, 3 + READ_LEN + 3 + READ_LEN + 1), dtype=np.uint8)
    rec[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + READ_LEN] = bases.reshape(n_reads, READ_LEN)
    rec[:, 3 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + READ_LEN:6 + 2 * READ_LEN] = np.resize(rng.choice(QUALS, size=(PIECE, READ_LEN), p=[0.01, 0.03, 0.11, 0.85]), (n_reads, READ_LEN)) + 33
    rec[:, -1] = ord("\n")
    d = tempfile.mkdtemp(prefix="read_stats_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    fq = os.path.join(d, "reads.fq")
    rec.tofile(fq)
    ctx.set_threads(16)
    try:
        for packed in (False, True):
            for mode in (0, 1, 2, 0, 1):
                ctx.set_input_format(packed)
                ctx.set_read_stats(mode)
                times = []
                for rep in range(4):
                    ctx.reset()
                    t0 = time.perf_counter()
                    ctx.map_fastx(fq)
                    ctx.counters()
                    times.append(time.perf_counter() - t0)
                t = sorted(times[1:])
                print(f"map_fastx {'packed' if packed else 'ascii'} read statistics {('off', 'with qualities', 'without qualities')[mode]}: median {t[1] * 1e3:.1f} ms "
                      f"(min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}) of 3, {n_reads} reads; counted reads={ctx.read_stats_info(0)['reads']}")
    finally:
        os.remove(fq)
        os.rmdir(d)


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    n_e2e = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000_000
    tmp = tempfile.mkdtemp(prefix="read_stats_bench_")
    prg = os.path.join(tmp, "dr.prg")
    synth.small_panel(seed=42).write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_opts(illumina=True, genome_size=20000)
    ctx.set_base_mask(2)
    kernel_leg(ctx, n_reads, launches)
    ctx.set_base_mask(0)
    torch.cuda.empty_cache()
    if n_e2e:
        e2e_leg(ctx, n_e2e)
    ctx.close()


if __name__ == "__main__":
    main()
