"""The trim kernels beside read_qual_kernel on one Nanopore-like block (DESIGN.md section 6 "Read trimming"): N reads of lognormal length
around 4 kb, their quality bytes made on the device, through drprg_hip_read_filter_device (min_len 500, max_len 50 000, Q 10) and
drprg_hip_read_trim_device (Q 20, W 4, no crops) in turn.  Prints the time of each call between two events; run it under
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/read_trim_bench.py [reads] [launches]
for the kernels' own durations (tools/profile_summary.py reads the stats file)."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drprg_amd import Context, synth  # noqa: E402


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    rng = np.random.default_rng(1)
    lengths = np.clip(rng.lognormal(np.log(3500.0), 0.5, size=n_reads), 200, 60_000).astype(np.int64)
    offs = np.zeros(n_reads + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lengths)
    n_bases = int(offs[-1])
    d_o = torch.from_numpy(offs).cuda()
    # qualities 3..40 in runs of 64 bytes around one of four levels, so that reads have bad stretches at their ends and inside; bias 33
    d_q = torch.empty(n_bases + 64, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for at in range(0, n_bases, step):
        m = min(step, n_bases - at)
        level = torch.randint(0, 4, ((m + 63) // 64,), device="cuda", dtype=torch.uint8).repeat_interleave(64)[:m]
        d_q[at:at + m] = 33 + 3 + level * 8 + torch.randint(0, 14, (m,), device="cuda", dtype=torch.uint8)
    d_q[n_bases:] = 0
    d_sums = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    d_flags = torch.zeros(n_reads, dtype=torch.uint8, device="cuda")
    d_begin = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    d_end = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    tmp = tempfile.mkdtemp(prefix="read_trim_bench_")
    prg = os.path.join(tmp, "dr.prg")
    synth.small_panel(seed=42).write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_read_filter(min_len=500, max_len=50_000, min_qual=10)
    ctx.set_read_trim(qual=20, window=4)
    t_filter, t_trim = [], []
    for _ in range(launches):
        for times, call in ((t_filter, lambda: ctx.read_filter_device(d_q.data_ptr(), 33, d_o.data_ptr(), n_reads, n_bases, d_sums.data_ptr(), d_flags.data_ptr())),
                            (t_trim, lambda: ctx.read_trim_device(d_q.data_ptr(), 33, d_o.data_ptr(), None, n_reads, n_bases, d_begin.data_ptr(), d_end.data_ptr()))):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            out = call()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
    kept = int((d_end - d_begin).sum().item())
    print(f"reads={n_reads} quality_bytes={n_bases} launches={launches} trim: kept_bases={out[0]} (sum of ranges {kept}) reads_lost_base={out[1]}")
    for name, t in (("read_filter_device", t_filter), ("read_trim_device", t_trim)):
        t = sorted(t)
        print(f"{name}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}) = {n_bases / t[len(t) // 2] / 1e9:.3f} TB/s on the quality bytes")
    ctx.close()


if __name__ == "__main__":
    main()
