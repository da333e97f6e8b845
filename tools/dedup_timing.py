#!/usr/bin/env python3
"""The timings of duplicate removal (nothing here is a gate; DESIGN.md section 6 keeps the numbers).

  keys: dedup_keys_kernel through drprg_hip_dedup_keys_device on a packed batch of N reads of L bases made on the device, HIP events around
        each call after a warm-up.  The call zeroes the keys and ends in a 4-byte read-back and a stream wait, so the figure is a call time,
        an upper bound of the kernel's; bytes read = n_bases / 4 + 8 per read, as a share of 8 TB/s.  The kernel alone, and the sort and
        the exact check of a whole call, come from a profiler run of their own:
            rocprofv3 --kernel-trace --stats -- python tools/dedup_timing.py call ...
  call: a FASTQ of N reads of L uniformly random bases (no two coincide by chance) of which the given fraction are copies of original reads in
        front of them; drprg_hip_map_fastx (ordered ingest, reads resident) is one mapping pass -- the same code on the parent commit, so this
        figure is the yardstick for what --dedup costs a run; random reads find no locus, so both it and the fresh mapping inside the call
        are those of a sample that maps nowhere --, then drprg_hip_dedup on the resident sample, wall clock around the synchronous call.
        The tool stops with an error unless the call kept exactly the reads that are no copies.

  python tools/dedup_timing.py keys [reads, default 10e6] [read length, default 150] [reps, default 7]
  python tools/dedup_timing.py call [reads, default 10e6] [read length, default 150] [duplicate fraction, default 0.3] [threads, default 16]
One JSON line per measurement on stdout."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12  # bytes per second


def _context(tmp):
    from drprg_amd import Context, synth
    panel = synth.small_panel(seed=42)
    prg = os.path.join(tmp, "dr.prg")
    panel.write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_opts(illumina=True, genome_size=4411532)
    return ctx, panel


def keys(n_reads, L, reps):
    import torch
    ctx, _ = _context(tempfile.mkdtemp(prefix="dedup_timing_"))
    n_bases = n_reads * L
    n_words = (n_bases + 15) // 16
    g = torch.Generator(device="cuda").manual_seed(1)
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_words + 4,), dtype=torch.int32, device="cuda", generator=g)
    offs = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    out = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for _ in range(reps + 1):  # (the first call warms up)
        torch.cuda.synchronize()
        ev[0].record()
        ctx.dedup_keys_device(words.data_ptr(), offs.data_ptr(), n_reads, n_bases, None, 0, out.data_ptr(), stream=stream)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ms = float(np.median(times[1:]))
    nbytes = n_words * 4 + 8 * n_reads
    print(json.dumps(dict(measurement="dedup_keys_call", n_reads=n_reads, read_len=L, n_bases=n_bases, reps=reps, call_ms=round(ms, 4),
                          bytes_read=nbytes, tb_per_s=round(nbytes / ms / 1e9, 3), share_of_hbm_peak=round(nbytes / (ms * 1e-3) / HBM_PEAK, 3),
                          runs_ms=[round(x, 4) for x in times[1:]])))
    ctx.close()


def call(n_reads, L, dup, threads):
    from drprg_amd import synth
    tmp = tempfile.mkdtemp(prefix="dedup_timing_")
    ctx, _ = _context(tmp)
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    block = np.empty((n_reads, L), np.uint8)
    step = max(1, (1 << 28) // L)
    for lo in range(0, n_reads, step):  # uniform random bases: no two reads of 150 bases or more coincide by chance
        m = min(step, n_reads - lo)
        block[lo:lo + m] = acgt[rng.integers(0, 4, size=(m, L), dtype=np.uint8)]
    n_dup = int(round(n_reads * dup))
    if n_dup:
        # n_dup places behind the first read; each takes a copy of an ORIGINAL read in front of it, so exactly n_dup reads are duplicates
        at = np.sort(rng.choice(np.arange(1, n_reads), size=n_dup, replace=False))
        originals = np.setdiff1d(np.arange(n_reads), at, assume_unique=True)
        before = at - np.arange(n_dup)  # originals in front of at[i]: at least read 0
        block[at] = block[originals[(rng.random(n_dup) * before).astype(np.int64)]]
    fq = os.path.join(tmp, "reads.fq")
    synth.write_fastq_fixed(fq, block.reshape(-1), L)
    del block
    ctx.set_threads(threads)
    ctx.set_input_format(True)
    ctx.keep_reads(64 << 30)
    ctx.set_ordered_ingest(True)
    res = {}
    for rep in range(2):  # (the first pass warms up: page cache, device buffers)
        ctx.reset()
        t0 = time.perf_counter()
        ctx.map_fastx(fq)
        ctx.counters()
        t1 = time.perf_counter()
        out = ctx.dedup()
        ctx.counters()
        t2 = time.perf_counter()
        if out["reads_before"] != n_reads or out["reads_kept"] != n_reads - n_dup:
            sys.exit(f"dedup_timing: {n_dup} copies were put among {n_reads} reads, the call says {out}")
        res = dict(map_pass_s=round(t1 - t0, 4), dedup_call_s=round(t2 - t1, 4), **out)
    print(json.dumps(dict(measurement="dedup_call", n_reads=n_reads, read_len=L, duplicate_fraction=dup, threads=threads,
                          resident=ctx.resident_info(), **res)))
    ctx.close()
    os.remove(fq)


if __name__ == "__main__":
    a = sys.argv[1:]
    if not a or a[0] not in ("keys", "call"):
        sys.exit(__doc__)
    n = int(float(a[1])) if len(a) > 1 else 10_000_000
    length = int(a[2]) if len(a) > 2 else 150
    if a[0] == "keys":
        keys(n, length, int(a[3]) if len(a) > 3 else 7)
    else:
        call(n, length, float(a[3]) if len(a) > 3 else 0.3, int(a[4]) if len(a) > 4 else 16)
