"""decoy_screen_kernel on one block (DESIGN.md section 4 "Decoy screen"): N reads, their bases made on the device (random ACGT, every
sixteenth read a stretch of the decoy so that there are hits to find), through drprg_hip_decoy_screen_device as text and as packed words,
in turn, against a decoy of DECOY random bases at K = 31.  Prints the time of each call between two events (the screen kernel, the verdict
kernel, two memsets and the read-back), the probes (valid windows: one table lookup each) and the bytes moved: the bases once, the offsets
once, eight bytes per probed slot at the least.  Run it under
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/decoy_screen_bench.py SHAPE [reads] [launches] [decoy bases]
for the kernels' own durations.  SHAPE: "short" (150 bases; default 10 M reads) or "long" (lognormal around 4 kb; default 2 M reads).
The decoy's default size is 1 M bases: a table of 2^21 slots, 16 MB -- beyond one XCD's L2, inside the Infinity Cache."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drprg_amd import Context, synth  # noqa: E402

K = 31


def main():
    shape = sys.argv[1] if len(sys.argv) > 1 else "short"
    n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else dict(long=2_000_000).get(shape, 10_000_000)
    launches = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    n_decoy = int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000
    rng = np.random.default_rng(1)
    if shape == "long":
        lengths = np.clip(rng.lognormal(np.log(3500.0), 0.5, size=n_reads), 200, 60_000).astype(np.int64)
    else:
        lengths = np.full(n_reads, 150, dtype=np.int64)
    offs = np.zeros(n_reads + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lengths)
    n_bases = int(offs[-1])
    n_words = (n_bases + 15) // 16
    decoy = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n_decoy)
    tmp = tempfile.mkdtemp(prefix="decoy_screen_bench_")
    fa = os.path.join(tmp, "decoy.fa")
    with open(fa, "wb") as fh:
        fh.write(b">decoy\n" + decoy.tobytes() + b"\n")
    d_o = torch.from_numpy(offs).cuda()
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    d_t = torch.empty(n_bases + 64, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for at in range(0, n_bases, step):
        m = min(step, n_bases - at)
        d_t[at:at + m] = letters[torch.randint(0, 4, (m,), device="cuda")]
    d_t[n_bases:] = 0
    d_decoy = torch.from_numpy(decoy).cuda()
    for i in range(0, n_reads, 16):  # every sixteenth read: decoy bases, as many as fit
        m = min(int(lengths[i]), n_decoy)
        s = int(rng.integers(0, n_decoy - m + 1))
        d_t[int(offs[i]):int(offs[i]) + m] = d_decoy[s:s + m]
        if i > 16 * 20_000:  # (enough of them: the copies are one launch each)
            break
    prg = os.path.join(tmp, "dr.prg")
    synth.small_panel(seed=42).write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_decoy([fa], k=K)
    info = ctx.decoy_info()
    # the packed form of the same bases (all ACGT: no position list)
    d_w = torch.empty(n_words + 16, dtype=torch.int32, device="cuda")
    assert ctx.pack_device(d_t.data_ptr(), n_bases, d_w.data_ptr(), None, 0) == 0
    d_v = torch.zeros(n_reads, dtype=torch.int32, device="cuda")
    d_h = torch.zeros(n_reads, dtype=torch.int32, device="cuda")
    d_f = torch.zeros(n_reads, dtype=torch.uint8, device="cuda")
    calls = [("decoy_screen_device text", lambda: ctx.decoy_screen_device(d_t.data_ptr(), None, None, 0, d_o.data_ptr(), n_reads, n_bases, d_v.data_ptr(), d_h.data_ptr(),
                                                                          d_f.data_ptr()), n_bases),
             ("decoy_screen_device packed", lambda: ctx.decoy_screen_device(None, d_w.data_ptr(), None, 0, d_o.data_ptr(), n_reads, n_bases, d_v.data_ptr(), d_h.data_ptr(),
                                                                            d_f.data_ptr()), n_words * 4)]
    times, outs = {name: [] for name, _, _ in calls}, {}
    for _ in range(launches):
        for name, call, _ in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            outs[name] = call()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    print(f"shape={shape} reads={n_reads} bases={n_bases} launches={launches} decoy_bases={n_decoy} k={K} decoy_kmers={info['kmers']} table_slots={info['slots']} "
          f"table_bytes={8 * info['slots']}")
    for name, _, base_bytes in calls:
        t = sorted(times[name])
        dropped, dropped_bases, probes, hits = outs[name]
        moved = base_bytes + 8 * (n_reads + 1) + 8 * probes
        print(f"{name}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}) = {n_bases / t[len(t) // 2] / 1e9:.3f} T bases/s; probes={probes} hits={hits} "
              f"reads_dropped={dropped} bytes_moved>={moved} ({moved / t[len(t) // 2] / 1e9:.3f} TB/s)")
    ctx.close()


if __name__ == "__main__":
    main()
