"""The duplicate-pair stage (DESIGN.md section 4 "Duplicate pairs"): N pairs of 150-base mates as two packed batches made on the device
(uniformly random letters: no two mates coincide by chance), one call of drprg_hip_dedup_pairs_device between two events -- the memsets, the
key kernel on both batches, the unit table, the sort, the exact check, the pointer doubling, copies, levels, flags and the two scans, and
the read-back.  Three cases: no duplicates; one pair in ten is a copy of an earlier pair; one stack of `stack` copies of one pair (default
N / 5).  The tool stops with an error unless every case reports exactly the copies that were planted.  Beside them the yardstick of the same
session for "one pass over the same packed bases": the dedup key kernel over both batches (drprg_hip_dedup_keys_device).
  python tools/pair_dedup_bench.py [pairs, default 5e6] [resident pairs, default 2e6]
Then the whole drprg_hip_dedup_pairs call on a resident sample of `resident pairs` pairs of which one in ten is a copy (0 skips the leg),
mapped from two FASTQ files in the page cache: wall time of the call alone, and beside it plain drprg_hip_dedup on the same resident sample
(the selection --dedup makes of the same bytes; both calls hold the compaction of every block and the fresh mapping of the kept reads).
Medians of three.  Reads nothing outside the repository."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drprg_amd import Context, synth  # noqa: E402

READ_LEN = 150


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


def planted(n_pairs, case, stack, seed=11):
    """(dst, src): pair dst[i] becomes a copy of pair src[i]; every src is an original in front of its dst"""
    rng = np.random.default_rng(seed)
    if case == "none":
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if case == "tenth":
        dst = np.sort(rng.choice(np.arange(1, n_pairs), size=n_pairs // 10, replace=False))
        originals = np.setdiff1d(np.arange(n_pairs), dst, assume_unique=True)
        before = dst - np.arange(dst.size)  # originals in front of dst[i]: at least pair 0
        return dst, originals[(rng.random(dst.size) * before).astype(np.int64)]
    dst = np.sort(rng.choice(np.arange(1, n_pairs), size=stack - 1, replace=False))
    return dst, np.zeros(dst.size, np.int64)


def text_sides(n_pairs, dst, src, seed=3):
    """two (n_pairs, READ_LEN) byte matrices of random letters on the device, the copies planted in both"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    sides = []
    for _ in range(2):
        t = torch.empty((n_pairs, READ_LEN), dtype=torch.uint8, device="cuda")
        for lo in range(0, n_pairs, 1 << 20):
            m = min(1 << 20, n_pairs - lo)
            t[lo:lo + m] = lut[torch.randint(0, 4, (m, READ_LEN), dtype=torch.int32, device="cuda", generator=g)]
        if dst.size:
            t[torch.from_numpy(dst).cuda()] = t[torch.from_numpy(src).cuda()]
        sides.append(t)
    return sides


def packed_side(ctx, text, n_pairs):
    n_bases = n_pairs * READ_LEN
    d_t = torch.zeros(n_bases + 64, dtype=torch.uint8, device="cuda")
    d_t[:n_bases] = text.reshape(-1)
    d_w = torch.empty((n_bases + 15) // 16 + 16, dtype=torch.int32, device="cuda")
    d_np = torch.empty(1024, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (the text was made on torch's stream, the context packs on its own)
    assert ctx.pack_device(d_t.data_ptr(), n_bases, d_w.data_ptr(), d_np.data_ptr(), 1024) == 0
    return d_w, n_bases


def kernel_leg(ctx, n_pairs, stack):
    d_o = torch.from_numpy(np.arange(n_pairs + 1, dtype=np.int64) * READ_LEN).cuda()
    d_keys, d_k = torch.empty(n_pairs, dtype=torch.int64, device="cuda"), torch.empty(n_pairs, dtype=torch.int64, device="cuda")
    d_keep, d_copies = torch.empty(n_pairs, dtype=torch.uint8, device="cuda"), torch.empty(n_pairs, dtype=torch.int32, device="cuda")
    print(f"pairs={n_pairs} bases={2 * n_pairs * READ_LEN}")
    for case in ("none", "tenth", "stack"):
        dst, src = planted(n_pairs, case, stack)
        a, b = text_sides(n_pairs, dst, src)
        (d_wa, n_bases), (d_wb, _) = packed_side(ctx, a, n_pairs), packed_side(ctx, b, n_pairs)
        del a, b
        torch.cuda.empty_cache()
        sa, sb = (d_wa.data_ptr(), d_o.data_ptr(), n_bases, None, 0), (d_wb.data_ptr(), d_o.data_ptr(), n_bases, None, 0)
        if case == "none":
            def keys():
                ctx.dedup_keys_device(d_wa.data_ptr(), d_o.data_ptr(), n_pairs, n_bases, None, 0, d_k.data_ptr())
                ctx.dedup_keys_device(d_wb.data_ptr(), d_o.data_ptr(), n_pairs, n_bases, None, 0, d_k.data_ptr())
            med, lo, hi, _ = median3(keys)
            print(f"dedup_keys_device on both batches (the yardstick): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
        med, lo, hi, out = median3(lambda: ctx.dedup_pairs_device(sa, sb, n_pairs, 64, d_keys.data_ptr(), d_keep.data_ptr(), d_copies.data_ptr()))
        if out["units_dropped"] != dst.size or out["reads_kept"] != 2 * (n_pairs - dst.size):
            sys.exit(f"pair_dedup_bench: {dst.size} copies were planted among {n_pairs} pairs, the call says {out}")
        levels = {c + 1: v for c, v in enumerate(out["levels"]) if v}
        print(f"dedup_pairs_device case {case}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {n_pairs / med / 1e3:.2f} M pairs/s; "
              f"units_dropped={out['units_dropped']} levels={levels}")
        del d_wa, d_wb
        torch.cuda.empty_cache()


def write_fastq(path, rows):
    n_reads = rows.shape[0]
    rec = np.empty((n_reads, 3 + READ_LEN + 3 + READ_LEN + 1), dtype=np.uint8)
    rec[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + READ_LEN] = rows
    rec[:, 3 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + READ_LEN:6 + 2 * READ_LEN] = ord("I")
    rec[:, -1] = ord("\n")
    rec.tofile(path)


def resident_leg(ctx, n_pairs):
    dst, src = planted(n_pairs, "tenth", 0)
    a, b = text_sides(n_pairs, dst, src)
    d = tempfile.mkdtemp(prefix="pair_dedup_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    r1, r2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    write_fastq(r1, a.cpu().numpy())
    write_fastq(r2, b.cpu().numpy())
    del a, b
    torch.cuda.empty_cache()
    ctx.set_threads(16)
    ctx.set_ordered_ingest(True)
    ctx.set_input_format(True)
    ctx.keep_reads(8 << 30)
    ctx.set_pair_overlap(30, "0.05", False)
    try:
        for what in ("dedup_pairs", "dedup"):
            ctx.set_dedup_pairs(what == "dedup_pairs")
            times = []
            for rep in range(4):
                ctx.reset()
                ctx.map_fastx(r1)
                ctx.begin_mates()
                ctx.map_fastx(r2)
                ctx.pair_overlap()
                ctx.counters()
                t0 = time.perf_counter()
                out = ctx.dedup_pairs() if what == "dedup_pairs" else ctx.dedup()
                ctx.counters()
                times.append(time.perf_counter() - t0)
            if out["reads_kept"] != 2 * (n_pairs - dst.size):
                sys.exit(f"pair_dedup_bench: {dst.size} copies were planted among {n_pairs} pairs, {what} says {out}")
            t = sorted(times[1:])
            print(f"{what} on a resident sample: median {t[1] * 1e3:.1f} ms (min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}) of 3, {n_pairs} pairs; "
                  f"reads_kept={out['reads_kept']} of {out['reads_before']} (the call holds the compaction of every block and the fresh mapping of the kept reads)")
    finally:
        os.remove(r1)
        os.remove(r2)
        os.rmdir(d)


def main():
    n_pairs = int(float(sys.argv[1])) if len(sys.argv) > 1 else 5_000_000
    n_resident = int(float(sys.argv[2])) if len(sys.argv) > 2 else 2_000_000
    tmp = tempfile.mkdtemp(prefix="pair_dedup_bench_")
    prg = os.path.join(tmp, "dr.prg")
    synth.small_panel(seed=42).write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_opts(illumina=True, genome_size=20000)
    kernel_leg(ctx, n_pairs, max(2, n_pairs // 5))
    if n_resident:
        resident_leg(ctx, n_resident)
    ctx.close()


if __name__ == "__main__":
    main()
