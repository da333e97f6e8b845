#!/usr/bin/env python3
"""The two timings of the BAM path (nothing here is a gate; DESIGN.md section 6 keeps the numbers).

  kernel: bam_pack_kernel (drprg_hip_pack_device_bam) against pack_kernel (drprg_hip_pack_device) on the same reads -- as 4-bit fields and
          as ASCII -- on one device in one process, runs alternating, HIP events around each call; once all forward, once half reversed.
          The calls end in a small read-back and a stream wait, the same for both, so the figures are call times, not pure kernel times.
  e2e:    drprg_hip_map_fastx on N x 150 bp as BAM and as the bgzip'd FASTQ of the same reads, both written here with zlib level 1 and
          the same member size.

  python tools/bam_ingest_timing.py kernel [bases, default 1.5e9] [reps, default 7]
  python tools/bam_ingest_timing.py e2e [reads, default 10e6] [threads, default 16] [reps, default 3]
One JSON line per measurement on stdout."""
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODE = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    CODE[_c] = _i


def _context(tmp):
    from drprg_amd import Context, synth
    panel = synth.small_panel(seed=42)
    prg = os.path.join(tmp, "dr.prg")
    panel.write(prg, os.path.join(tmp, "genes.fa"))
    ctx = Context(prg, 11, 15, device=0, from_files=False)
    ctx.set_opts(illumina=True, genome_size=4411532)
    return ctx, panel


def kernel(n_bases, reps):
    import tempfile
    import torch
    ctx, _ = _context(tempfile.mkdtemp(prefix="bam_timing_"))
    L = 150
    n_reads = n_bases // L
    n_bases = n_reads * L
    g = torch.Generator(device="cuda").manual_seed(1)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    ascii_ = letters[torch.randint(0, 4, (n_bases,), device="cuda", generator=g)]
    code = torch.from_numpy(CODE).cuda()[ascii_.long()].view(n_reads, L)
    seq = (code[:, 0::2] << 4 | code[:, 1::2]).contiguous().view(-1)  # 75 bytes per read, forward fields
    start = torch.arange(n_reads, dtype=torch.int64, device="cuda") * (L // 2)
    offs = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    words = torch.zeros((n_bases + 15) // 16, dtype=torch.int32, device="cuda")
    npos = torch.zeros(1024, dtype=torch.int64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])
    stream = torch.cuda.current_stream().cuda_stream
    for name, frac in (("all_forward", 0.0), ("half_reversed", 0.5)):
        rev = (torch.rand(n_reads, device="cuda", generator=g) < frac).to(torch.uint8)
        t_bam, t_pack = [], []
        for _ in range(reps + 1):  # (the first pair warms up)
            t_bam.append(timed(lambda: ctx.pack_device_bam(seq.data_ptr(), start.data_ptr(), offs.data_ptr(), rev.data_ptr(), n_reads, n_bases,
                                                           words.data_ptr(), npos.data_ptr(), 1024, stream=stream)))
            t_pack.append(timed(lambda: ctx.pack_device(ascii_.data_ptr(), n_bases, words.data_ptr(), npos.data_ptr(), 1024, stream=stream)))
        b, p = float(np.median(t_bam[1:])), float(np.median(t_pack[1:]))
        print(json.dumps(dict(measurement="bam_pack_vs_pack", reads=name, n_bases=n_bases, reps=reps, bam_pack_ms=round(b, 4), pack_ms=round(p, 4),
                              ratio=round(b / p, 3), bam_pack_runs_ms=[round(x, 4) for x in t_bam[1:]], pack_runs_ms=[round(x, 4) for x in t_pack[1:]])))
    ctx.close()


def _bgzf_members(chunks, fh, payload=65280, level=1):
    """the byte stream `chunks` yields, as BGZF members of `payload` bytes + the EOF block"""
    pend = bytearray()

    def member(data):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = co.compress(data) + co.flush()
        fh.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(data), len(data)))
    for c in chunks:
        pend += c
        while len(pend) >= payload:
            member(bytes(pend[:payload]))
            del pend[:payload]
    if pend:
        member(bytes(pend))
    fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def e2e(n_reads, threads, reps):
    import tempfile
    from drprg_amd import synth
    tmp = tempfile.mkdtemp(prefix="bam_timing_")
    ctx, panel = _context(tmp)
    L = 150
    gen = synth.HaplotypeGenomes(panel, genome_size=4411532 // 100, n_hap=4, seed=3)
    step = 200_000

    def batches():
        for i in range(0, n_reads, step):
            bases, _ = synth.sample_short_reads(gen, min(step, n_reads - i), seed=100 + i)
            yield bases.reshape(-1, L)

    def fastq_chunks():
        for b in batches():
            rec = np.empty((b.shape[0], 2 * L + 8), np.uint8)
            rec[:, :4] = np.frombuffer(b"@r0\n", np.uint8)
            rec[:, 4:4 + L] = b
            rec[:, 4 + L:7 + L] = np.frombuffer(b"\n+\n", np.uint8)
            rec[:, 7 + L:7 + 2 * L] = ord("I")
            rec[:, 7 + 2 * L] = ord("\n")
            yield rec.tobytes()

    def bam_chunks():
        yield b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 0)
        body = 32 + 3 + L // 2 + L
        fixed = struct.pack("<IiiBBHHHIiii", body, -1, -1, 3, 0, 4680, 0, 4, L, -1, -1, 0) + b"r0\0"
        for b in batches():
            c = CODE[b]
            rec = np.empty((b.shape[0], 4 + body), np.uint8)
            rec[:, :len(fixed)] = np.frombuffer(fixed, np.uint8)
            rec[:, len(fixed):len(fixed) + L // 2] = c[:, 0::2] << 4 | c[:, 1::2]
            rec[:, len(fixed) + L // 2:] = 40
            yield rec.tobytes()
    files = {}
    for name, chunks in (("bam", bam_chunks), ("fastq_bgzf", fastq_chunks)):
        files[name] = os.path.join(tmp, "reads." + ("bam" if name == "bam" else "fq.gz"))
        with open(files[name], "wb") as fh:
            _bgzf_members(chunks(), fh)
    ctx.set_threads(threads)
    ctx.set_input_format(True)  # what the executables use for text
    out = {}
    for rep in range(reps + 1):
        for name in files:  # alternating
            ctx.reset()
            t0 = time.perf_counter()
            ctx.map_fastx(files[name])
            ctx.sync()
            out.setdefault(name, []).append(time.perf_counter() - t0)
            assert ctx.counters()["reads"] == n_reads
    for name, ts in out.items():
        med = float(np.median(ts[1:]))
        print(json.dumps(dict(measurement="map_fastx_e2e", input=name, n_reads=n_reads, threads=threads, file_bytes=os.path.getsize(files[name]),
                              seconds=round(med, 4), reads_per_s=round(n_reads / med), runs_s=[round(x, 4) for x in ts[1:]])))
    ctx.close()
    for f in files.values():
        os.unlink(f)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    a = [float(x) for x in sys.argv[2:]]
    if what == "kernel":
        kernel(int(a[0]) if a else 1_500_000_000, int(a[1]) if len(a) > 1 else 7)
    else:
        e2e(int(a[0]) if a else 10_000_000, int(a[1]) if len(a) > 1 else 16, int(a[2]) if len(a) > 2 else 3)
