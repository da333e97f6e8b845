"""base_mask_kernel on one block (DESIGN.md section 4 "Base masking"): N reads of 150 bases (random ACGT, every quality at 35 except a share
P of them at 5; made on the host in a piece of 16 M bases that repeats), through drprg_hip_base_mask_device under Q = 10 as text and as
packed words, in turn, for P = 0, 0.03 and 0.2.  Prints the time of each call between two events: the memsets, a packed block's bitmap,
the mask kernel and the read-back -- and, for a packed block with a masked base, the scan and the emit of the position list.  The bases
are put back before every call.
  python tools/base_mask_bench.py [reads] [launches] [e2e reads]
Then, end to end: `e2e reads` reads (default 2 M; 0 skips the leg) with qualities at P = 0.03 as FASTQ text in the page cache, the wall time
of drprg_hip_map_fastx with and without the mask, ASCII and packed transport, median of three, and the launches of the dominant mapping
kernel in each run (drprg_hip_kernel_timing): the mask adds none to a run without it."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drprg_amd import Context, synth  # noqa: E402

Q, READ_LEN = 10, 150


def tiled(block, n, pad):
    """n bytes made of copies of `block`, `pad` zero bytes behind them, on the device (a plain copy: the data are made on the host)"""
    out = np.zeros(n + pad, dtype=np.uint8)
    out[:n] = np.resize(block, n)
    return torch.from_numpy(out).cuda()


def device_quals(n_bases, share, seed):
    """every quality at 35 except a share of them at 5 (FASTQ bytes); the pattern repeats every 2^24 + 13 bases"""
    q = np.full((1 << 24) + 13, 35 + 33, dtype=np.uint8)
    q[np.random.default_rng(seed).random(q.size) < share] = 5 + 33
    return tiled(q, n_bases, 64)


def kernel_leg(ctx, n_reads, launches):
    n_bases = n_reads * READ_LEN
    n_words = (n_bases + 15) // 16
    d_o = torch.from_numpy(np.arange(n_reads + 1, dtype=np.int64) * READ_LEN).cuda()
    d_t0 = tiled(np.random.default_rng(1).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(1 << 24) + 7), n_bases, 64)
    d_w0 = torch.empty(n_words + 16, dtype=torch.int32, device="cuda")
    assert ctx.pack_device(d_t0.data_ptr(), n_bases, d_w0.data_ptr(), None, 0) == 0
    d_t, d_w = torch.empty_like(d_t0), torch.empty_like(d_w0)
    print(f"reads={n_reads} bases={n_bases} launches={launches} Q={Q}")
    for share in (0.0, 0.03, 0.2):
        d_q = device_quals(n_bases, share, 7)
        d_list = torch.empty(int(n_bases * share * 1.05) + 1024, dtype=torch.int64, device="cuda")
        calls = [("text", lambda: ctx.base_mask_device(d_q.data_ptr(), 33, d_o.data_ptr(), None, n_reads, n_bases, d_t.data_ptr(), None, None, 0, None, 0)),
                 ("packed", lambda: ctx.base_mask_device(d_q.data_ptr(), 33, d_o.data_ptr(), None, n_reads, n_bases, None, d_w.data_ptr(), None, 0, d_list.data_ptr(),
                                                         d_list.numel()))]
        for name, call in calls:
            times, out = [], None
            for _ in range(launches + 1):
                d_t.copy_(d_t0)
                d_w.copy_(d_w0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                out = call()
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b))
            t = sorted(times[1:])  # (the first call allocates)
            med = t[len(t) // 2]
            print(f"base_mask_device {name} masked_share={share}: median {med:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}) = {n_bases / med / 1e9:.3f} T bases/s; "
                  f"reads_masked={out[2]} bases_masked={out[3]} list={out[5]}")
        del d_q, d_list


def e2e_leg(ctx, n_reads):
    rng = np.random.default_rng(3)
    gen = synth.HaplotypeGenomes(synth.small_panel(seed=42), genome_size=20000, n_hap=4)
    bases, _ = synth.sample_short_reads(gen, n_reads, seed=1)
    quals = np.full(bases.size, 35 + 33, dtype=np.uint8)
    quals[rng.random(bases.size) < 0.03] = 5 + 33
    head = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec = np.empty((n_reads, 3 + READ_LEN + 3 + READ_LEN + 1), dtype=np.uint8)
    rec[:, :3] = head
    rec[:, 3:3 + READ_LEN] = bases.reshape(n_reads, READ_LEN)
    rec[:, 3 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + READ_LEN:6 + 2 * READ_LEN] = quals.reshape(n_reads, READ_LEN)
    rec[:, -1] = ord("\n")
    d = tempfile.mkdtemp(prefix="base_mask_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    fq = os.path.join(d, "reads.fq")
    rec.tofile(fq)
    ctx.set_threads(16)
    try:
        for packed in (False, True):
            for q in (0, Q, 0, Q):
                ctx.set_input_format(packed)
                ctx.set_base_mask(q)
                times = []
                for rep in range(4):
                    ctx.reset()
                    ctx.kernel_timing(enable=True, reset=True)
                    t0 = time.perf_counter()
                    ctx.map_fastx(fq)
                    ctx.counters()
                    times.append(time.perf_counter() - t0)
                    k_ms, k_n = ctx.kernel_timing(enable=False)
                t = sorted(times[1:])
                info = ctx.base_mask_info()
                print(f"map_fastx {'packed' if packed else 'ascii'} mask_qual={q}: median {t[1] * 1e3:.1f} ms (min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}) of 3, {n_reads} reads; "
                      f"mapping kernel launches={k_n} ({k_ms:.2f} ms); bases_masked={info['bases_masked']}")
    finally:
        os.remove(fq)
        os.rmdir(d)


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    n_e2e = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000_000
    tmp = tempfile.mkdtemp(prefix="base_mask_bench_")
    prg = os.path.join(tmp, "dr.prg")
    synth.small_panel(seed=42).write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_opts(illumina=True, genome_size=20000)
    ctx.set_base_mask(Q)
    kernel_leg(ctx, n_reads, launches)
    torch.cuda.empty_cache()
    if n_e2e:
        e2e_leg(ctx, n_e2e)
    ctx.close()


if __name__ == "__main__":
    main()
