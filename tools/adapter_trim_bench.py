"""adapter_points_kernel beside trim_points_kernel on one block (DESIGN.md section 6 "Adapter trimming"): N reads, their bases made on the
device (random ACGT: a 33-letter adapter at E 0.1 then matches next to nowhere in full and as a 3-letter partial at one read end in 64),
through drprg_hip_adapter_trim_device as text and as packed words, and -- on quality bytes of the same sizes -- through
drprg_hip_read_trim_device (Q 20, W 4, no crops), in turn; then the same adapter and E under the indel rule (--adapter-indels:
adapter_edit_points_kernel, drprg_hip_adapter_trim_device2), alone and with a 28-letter 5' adapter.  Prints the time of each call between two events; run it under
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/adapter_trim_bench.py SHAPE [reads] [launches]
for the kernels' own durations.  SHAPE: "long" (lognormal around 4 kb, the block tools/read_trim_bench.py makes; default 2 M reads) or
"short" (150 bases; default 10 M reads) or "nanopore" (lognormal around 9 kb, up to 200 kb; default 500 k reads).  A fourth argument
"plain" leaves the indel rule out (a build that has none runs that way by itself)."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drprg_amd import Context, synth  # noqa: E402

ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"  # 33 letters
FRONT = "AATGTACTTCGTTCAGTTACGTATTGCT"         # 28 letters: a ligation adapter's top strand


def main():
    shape = sys.argv[1] if len(sys.argv) > 1 else "long"
    n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else dict(long=2_000_000, nanopore=500_000).get(shape, 10_000_000)
    launches = int(sys.argv[3]) if len(sys.argv) > 3 else 12
    rng = np.random.default_rng(1)
    if shape == "long":
        lengths = np.clip(rng.lognormal(np.log(3500.0), 0.5, size=n_reads), 200, 60_000).astype(np.int64)
    elif shape == "nanopore":
        lengths = np.clip(rng.lognormal(np.log(9000.0), 0.8, size=n_reads), 200, 200_000).astype(np.int64)
    else:
        lengths = np.full(n_reads, 150, dtype=np.int64)
    offs = np.zeros(n_reads + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lengths)
    n_bases = int(offs[-1])
    n_words = (n_bases + 15) // 16
    d_o = torch.from_numpy(offs).cuda()
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    d_t = torch.empty(n_bases + 64, dtype=torch.uint8, device="cuda")
    d_q = torch.empty(n_bases + 64, dtype=torch.uint8, device="cuda")
    d_w = torch.empty(n_words + 16, dtype=torch.int32, device="cuda")
    step = 1 << 28
    for at in range(0, n_bases, step):
        m = min(step, n_bases - at)
        d_t[at:at + m] = letters[torch.randint(0, 4, (m,), device="cuda")]
        level = torch.randint(0, 4, ((m + 63) // 64,), device="cuda", dtype=torch.uint8).repeat_interleave(64)[:m]
        d_q[at:at + m] = 33 + 3 + level * 8 + torch.randint(0, 14, (m,), device="cuda", dtype=torch.uint8)
    for at in range(0, n_words, step):
        m = min(step, n_words - at)
        d_w[at:at + m] = torch.randint(-2 ** 31, 2 ** 31, (m,), device="cuda", dtype=torch.int64).to(torch.int32)
    d_t[n_bases:] = 0
    d_q[n_bases:] = 0
    d_begin = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    d_end = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    d_len = torch.from_numpy(lengths).cuda()
    tmp = tempfile.mkdtemp(prefix="adapter_trim_bench_")
    prg = os.path.join(tmp, "dr.prg")
    synth.small_panel(seed=42).write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_adapters([ADAPTER], error="0.1")
    ctx.set_read_trim(qual=20, window=4)

    def adapter(text):
        if text:
            return ctx.adapter_trim_device(d_t.data_ptr(), None, None, 0, d_o.data_ptr(), n_reads, n_bases, d_begin.data_ptr(), d_end.data_ptr())
        return ctx.adapter_trim_device(None, d_w.data_ptr(), None, 0, d_o.data_ptr(), n_reads, n_bases, d_begin.data_ptr(), d_end.data_ptr())

    def adapter2(text):
        if text:
            return ctx.adapter_trim_device2(d_t.data_ptr(), None, None, 0, d_o.data_ptr(), n_reads, n_bases, d_begin.data_ptr(), d_end.data_ptr())
        return ctx.adapter_trim_device2(None, d_w.data_ptr(), None, 0, d_o.data_ptr(), n_reads, n_bases, d_begin.data_ptr(), d_end.data_ptr())

    plain = lambda: ctx.set_adapters([ADAPTER], error="0.1")
    calls = [("adapter_trim_device text", plain, lambda: adapter(True)), ("adapter_trim_device packed", plain, lambda: adapter(False)),
             ("read_trim_device", plain, lambda: ctx.read_trim_device(d_q.data_ptr(), 33, d_o.data_ptr(), None, n_reads, n_bases, d_begin.data_ptr(), d_end.data_ptr()))]
    if hasattr(ctx, "adapter_trim_device2") and (len(sys.argv) < 5 or sys.argv[4] != "plain"):
        indels = lambda: ctx.set_adapters([ADAPTER], error="0.1", indels=True)
        both = lambda: ctx.set_adapters([ADAPTER], front=[FRONT], error="0.1", indels=True)
        calls += [("adapter_trim_device2 plain rule text", plain, lambda: adapter2(True)), ("adapter_trim_device2 indels 3' text", indels, lambda: adapter2(True)),
                  ("adapter_trim_device2 indels 3' packed", indels, lambda: adapter2(False)), ("adapter_trim_device2 indels 3' + 5' text", both, lambda: adapter2(True)),
                  ("adapter_trim_device2 indels 3' + 5' packed", both, lambda: adapter2(False))]
    times, outs = {name: [] for name, _, _ in calls}, {}
    for _ in range(launches):
        for name, setup, call in calls:
            setup()
            d_begin.zero_()
            d_end.copy_(d_len)  # (every adapter launch on whole reads)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            outs[name] = call()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    print(f"shape={shape} reads={n_reads} bases={n_bases} launches={launches}")
    for name, _, _ in calls:
        t = sorted(times[name])
        print(f"{name}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}) = {n_bases / t[len(t) // 2] / 1e9:.3f} T bases/s; out={outs[name]}")
    ctx.close()


if __name__ == "__main__":
    main()
