"""The depth cap (`pandora --max-covg`, drprg_hip_set_max_covg) on the device: whatever entry point the reads come through, the context
maps exactly the first n reads and counts nothing else.  n comes from np.cumsum of the read lengths (tests/max_covg_rule.py), the expected
vectors and counters from the oracle on those n reads -- never from the code under test."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from max_covg_rule import OFF, accepted_reads
from test_gpu_parity import _ctx, _oracle_index, _oracle_map

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, K = 11, 15
G, CAP = 10_000, 3  # T = 40 000 bases: about 267 reads of 150


def _panel():
    from drprg_amd import synth
    panel = synth.small_panel(seed=23, n_loci=4, length=900)
    return panel, synth.HaplotypeGenomes(panel, genome_size=20000, n_hap=4, seed=9)


def _reads_of(genomes, lengths, seed):
    """reads of the given lengths cut from the haplotype genomes, either strand"""
    from drprg_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        h = genomes.haps[int(rng.integers(0, len(genomes.haps)))]
        s = int(rng.integers(0, len(h) - L + 1))
        r = h[s:s + L]
        out.append(synth._COMP[r[::-1]] if rng.random() < 0.5 else r.copy())
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths, dtype=np.uint64)
    return (np.concatenate(out) if offs[-1] else np.zeros(0, np.uint8)), offs


def _want(oracle, ctx, bases, offs, n):
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    return _oracle_map(oracle, idx, bases[:int(offs[n])], offs[:n + 1], W, K, True)


def _check(ctx, want, n, n_bases, reached, dropped, what=""):
    ocov, oprg, ocnt = want
    info = ctx.max_covg_info()
    print(f"{what}: info {info}; expected reached={reached} reads={n} bases={n_bases} dropped={dropped}")
    assert info == dict(reached=reached, reads=n, bases=n_bases, dropped=dropped), what
    cov, prg = ctx.coverage()
    cnt = ctx.counters()
    assert cnt["reads"] == n and cnt["bases"] == n_bases, what
    for key in ("hits", "clusters_kept", "hits_kept"):
        assert cnt[key] == ocnt[key], (what, key)
    assert np.array_equal(prg, oprg) and np.array_equal(cov, ocov), what


class _Device:
    """one batch in device memory, ASCII and packed"""

    def __init__(self, bases, offs):
        import torch
        from drprg_amd.pandora import pack_reads
        self.n_reads, self.n_bases = len(offs) - 1, int(offs[-1])
        pad = np.concatenate([bases, np.zeros(64, np.uint8)])
        self.bases = torch.from_numpy(pad).cuda()
        self.offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        words, npos = pack_reads(bases)
        self.words = torch.from_numpy(np.concatenate([words, np.zeros(16, np.uint32)]).view(np.int32)).cuda()
        self.n_npos = int(npos.size)
        self.npos = torch.from_numpy(np.concatenate([npos, np.zeros(1, np.uint64)]).astype(np.int64)).cuda()
        torch.cuda.synchronize()


def _map(ctx, entry, bases, offs, dev=None):
    from drprg_amd.pandora import pack_reads
    if entry == "host":
        ctx.map_host(bases, offs)
    elif entry == "host_packed":
        words, npos = pack_reads(bases)
        ctx.map_host_packed(words, offs, npos)
    elif entry in ("device", "device_async"):
        fn = ctx.map_device if entry == "device" else ctx.map_device_async
        fn(dev.bases.data_ptr(), dev.offs.data_ptr(), dev.n_reads, dev.n_bases)
    else:
        ctx.map_device_packed(dev.words.data_ptr(), dev.offs.data_ptr(), dev.n_reads, dev.n_bases, dev.npos.data_ptr() if dev.n_npos else None, dev.n_npos,
                              deferred=entry == "device_packed_async")


ENTRIES = ("host", "host_packed", "device", "device_async", "device_packed", "device_packed_async")


@pytest.mark.parametrize("kernel", [1, 2, 3])
def test_every_entry_point_maps_the_accepted_prefix(tmp_path, oracle, kernel):
    """host and device entry points, ASCII and packed, the three kernel sequences: vector, prg_reads and counters of the capped context
    equal the oracle's on the first n reads, and max_covg_info says (1, n, B(n), offered - n)"""
    from drprg_amd import synth
    panel, genomes = _panel()
    bases, offs = synth.sample_short_reads(genomes, 3000, seed=2)
    bases[np.random.default_rng(3).integers(0, bases.size, 200)] = ord("N")
    n, n_bases, reached = accepted_reads(np.diff(offs), G, CAP)
    assert reached and n == 267 and n_bases == 40050
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G, kernel=kernel)
    assert ctx.counters()["kernel"] == kernel
    want = _want(oracle, ctx, bases, offs, n)
    assert want[2]["clusters_kept"] > 5
    dev = _Device(bases, offs)
    ctx.set_max_covg(CAP)
    for entry in ENTRIES:
        ctx.reset()
        _map(ctx, entry, bases, offs, dev)
        _check(ctx, want, n, n_bases, True, 3000 - n, f"kernel {kernel} {entry}")
    # ... and with the cap off again the same context maps the whole batch
    ctx.set_max_covg(OFF)
    ctx.reset()
    _map(ctx, "device", bases, offs, dev)
    _check(ctx, _want(oracle, ctx, bases, offs, 3000), 3000, int(offs[-1]), False, 0, "cap off")
    ctx.close()


CUTS = {
    # name: (read lengths, genome size)
    "exactly_T": ([150] * 266 + [100] + [150] * 40, G),                       # B(267) == 40 000 == T
    "one_short_then_a_long_read": ([150] * 266 + [99] + [4000] + [150] * 40, G),  # B(267) == T - 1, the 4 kb read crosses
    "first_read": ([4000] + [150] * 60, 1000),                                # T = 4000: the first read is the cut
    "last_read_of_the_batch": ([150] * 266 + [100], G),                       # the cut is the batch's last read: nothing is dropped
    "never": ([150] * 200, G),                                                # 30 000 < T
    "one_base_short": ([150] * 266 + [99], G),                                # B == T - 1 at the end of the batch
    "empty_reads_around_the_cut": ([150] * 266 + [0, 0, 100, 0, 0] + [150] * 40, G),
    "empty_reads_at_both_ends": ([0, 0] + [150] * 270 + [0, 0], G),
}


@pytest.mark.parametrize("name", list(CUTS))
def test_cut_positions(tmp_path, oracle, name):
    """where the cut may fall -- on T exactly, one base short of it with a long read next, at read 1, at the last read, nowhere, beside
    empty reads --, through the host path and the device path (covg_cut_kernel), ASCII and packed"""
    lengths, g = CUTS[name]
    panel, genomes = _panel()
    bases, offs = _reads_of(genomes, lengths, seed=len(lengths))
    n, n_bases, reached = accepted_reads(lengths, g, CAP)
    assert reached == (name not in ("never", "one_base_short"))
    if name == "exactly_T":
        assert n_bases == (CAP + 1) * g and n == 267
    if name == "one_short_then_a_long_read":
        assert int(offs[267]) == (CAP + 1) * g - 1 and n == 268
    if name == "first_read":
        assert n == 1
    if name == "last_read_of_the_batch":
        assert n == len(lengths)
    if name == "empty_reads_around_the_cut":
        assert n == 269 and lengths[n - 1] == 100
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=g)
    want = _want(oracle, ctx, bases, offs, n)
    if not reached:  # the capped context equals the uncapped one
        ctx.map_host(bases, offs)
        ucov, uprg = ctx.coverage()
        assert np.array_equal(ucov, want[0]) and np.array_equal(uprg, want[1])
    dev = _Device(bases, offs)
    ctx.set_max_covg(CAP)
    for entry in ("host", "host_packed", "device", "device_packed", "device_async"):
        ctx.reset()
        _map(ctx, entry, bases, offs, dev)
        _check(ctx, want, n, n_bases, reached, len(lengths) - n, f"{name} {entry}")
    ctx.close()


@pytest.mark.parametrize("entry", ["host", "device", "device_async", "device_packed_async"])
def test_the_count_runs_across_calls_and_reset_starts_it_again(tmp_path, oracle, entry):
    """three batches with the cut inside the second: the third maps nothing and returns 0; the async form back to back, then sync; reset()
    starts the count again and keeps the cap"""
    from drprg_amd import synth
    panel, genomes = _panel()
    bases, offs = synth.sample_short_reads(genomes, 450, seed=6)
    parts = [(bases[i * 22500:(i + 1) * 22500], offs[i * 150:i * 150 + 151] - offs[i * 150]) for i in range(3)]
    n, n_bases, reached = accepted_reads(np.diff(offs), G, CAP)
    assert reached and 150 < n < 300
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    want = _want(oracle, ctx, bases, offs, n)
    devs = [_Device(b, o) for b, o in parts]
    ctx.set_max_covg(CAP)
    for round_ in range(2):
        for (b, o), d in zip(parts, devs):
            _map(ctx, entry, b, o, d)  # (a refused call would raise: the third returns 0)
        ctx.sync()
        _check(ctx, want, n, n_bases, True, 450 - n, f"{entry} round {round_}")
        ctx.reset()
        assert ctx.max_covg_info() == dict(reached=False, reads=0, bases=0, dropped=0)
    # a cap set after reads were mapped applies from the running total: the first batch uncapped, then the cap
    ctx.set_max_covg(None)
    _map(ctx, entry, *parts[0], devs[0])
    ctx.set_max_covg(CAP)
    _map(ctx, entry, *parts[1], devs[1])
    _map(ctx, entry, *parts[2], devs[2])
    _check(ctx, want, n, n_bases, True, 450 - n, f"{entry} cap set late")
    ctx.close()


@pytest.mark.parametrize("kernel", [1, 2, 3])
def test_packed_batches_with_odd_bytes_at_the_cut(tmp_path, oracle, kernel):
    """non-ACGT bytes at the last accepted base, at the first dropped base and well past the cut: the packed forms give what the ASCII
    form and the oracle give (the position list is cut with the batch)"""
    from drprg_amd import synth
    panel, genomes = _panel()
    bases, offs = synth.sample_short_reads(genomes, 1200, seed=8)
    n, n_bases, _ = accepted_reads(np.diff(offs), G, CAP)
    for at in (n_bases - 1, n_bases, n_bases + 1, n_bases + 15, n_bases + 16, n_bases + 5000, int(offs[-1]) - 1, 7):
        bases[at] = ord("N")
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G, kernel=kernel)
    want = _want(oracle, ctx, bases, offs, n)
    dev = _Device(bases, offs)
    assert dev.n_npos == 8
    ctx.set_max_covg(CAP)
    for entry in ENTRIES:
        ctx.reset()
        _map(ctx, entry, bases, offs, dev)
        _check(ctx, want, n, n_bases, True, 1200 - n, f"kernel {kernel} {entry}")
    ctx.close()


def _ingest_block_bases():
    """the ingest's block and slice sizes in force, read from csrc/ingest.cpp (defaults; the environment may override them)"""
    src = open(os.path.join(ROOT, "drprg_amd", "csrc", "ingest.cpp")).read()
    m = re.search(r'getenv\("DRPRG_INGEST_BLOCK_MB"\);.*?\? mb : (\d+)\) << 20', src, re.S)
    s = re.search(r'getenv\("DRPRG_INGEST_SLICE_MB"\);.*?\? mb : (\d+)\) << 20', src, re.S)
    block = int(os.environ.get("DRPRG_INGEST_BLOCK_MB", 0) or 0) or int(m.group(1))
    slice_ = int(os.environ.get("DRPRG_INGEST_SLICE_MB", 0) or 0) or int(s.group(1))
    return block << 20, slice_ << 20


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_device", "device_listed_twice"])
def test_map_fastx_stops_at_the_cap(tmp_path, oracle, gz, devices):
    """map_fastx on a multi-block FASTQ: 400 000 reads of 150 bases = 60 M bases, 126.4 MB of text (63 MB of bases would already be five
    blocks of the ingest's 12 MB; under a cap a block also ends with its 8 MB slice of the text, so the file is 16 slices).  The cut (read
    267) lies in the first block; the result equals the oracle on the first n reads, ASCII and packed ingest, the reads kept resident are
    those n and another context maps exactly them, and the ingest stopped long before the end of the file."""
    from drprg_amd import Context, synth
    panel, genomes = _panel()
    n_reads = 400_000
    bases, offs = synth.sample_short_reads(genomes, n_reads, seed=12)
    block, slice_ = _ingest_block_bases()
    fq = str(tmp_path / "reads.fq")
    synth.write_fastq_fixed(fq, bases, 150)
    text = os.path.getsize(fq)
    assert text == n_reads * 316 and text >= 8 * slice_ and int(offs[-1]) >= 4 * block  # several whole blocks lie behind the cut
    if gz:
        with open(fq, "rb") as src, gzip.open(fq + ".gz", "wb", compresslevel=1) as dst:
            while True:
                chunk = src.read(8 << 20)
                if not chunk:
                    break
                dst.write(chunk)
        fq += ".gz"
    n, n_bases, reached = accepted_reads(np.diff(offs), G, CAP)
    assert reached and n == 267
    prg = str(tmp_path / "dr.prg")
    panel.write(prg, str(tmp_path / "genes.fa"))

    def open_ctx():
        c = Context(prg, W, K, device=0, from_files=False) if devices is None else Context(prg, W, K, from_files=False, devices=devices)
        c.set_opts(illumina=True, genome_size=G)
        c.prg_strings = panel.prgs
        return c
    ctx = open_ctx()
    ctx.set_threads(8)
    want = _want(oracle, ctx, bases, offs, n)
    ctx.set_max_covg(CAP)
    for packed in (False, True):
        ctx.reset()
        ctx.set_input_format(packed)
        ctx.keep_reads(1 << 28)
        ctx.map_fastx(fq)
        info = ctx.max_covg_info()
        print(f"gz={gz} devices={devices} packed={packed}: {info}, reads behind the cut {n_reads - n}")
        assert (info["reached"], info["reads"], info["bases"]) == (True, n, n_bases)
        assert 0 <= info["dropped"] < n_reads - n  # the reads parsed before the ingest stopped, not the rest of the file
        cov, prgr = ctx.coverage()
        cnt = ctx.counters()
        assert cnt["reads"] == n and cnt["bases"] == n_bases
        for key in ("hits", "clusters_kept", "hits_kept"):
            assert cnt[key] == want[2][key], key
        assert np.array_equal(cov, want[0]) and np.array_equal(prgr, want[1])
        # the kept set is the accepted prefix: another context maps exactly those reads from HBM
        assert ctx.resident_info()["complete"]
        other = open_ctx()
        other.map_resident(ctx)
        ocov, oprg = other.coverage()
        assert other.counters()["reads"] == n and np.array_equal(ocov, want[0]) and np.array_equal(oprg, want[1])
        other.close()
        # a second file after the cap: nothing is mapped, the call returns 0
        ctx.map_fastx(fq)
        assert ctx.counters()["reads"] == n and ctx.max_covg_info()["reads"] == n
    ctx.close()


def _truncated_fastq(src, dst, n):
    with open(src) as fh, open(dst, "w") as out:
        for i, line in enumerate(fh):
            if i >= 4 * n:
                break
            out.write(line)


def _fastq_lengths(fq):
    return [len(line.rstrip("\n")) for i, line in enumerate(open(fq)) if i % 4 == 1]


def test_pandora_map_with_a_cap_equals_the_truncated_file(tmp_path):
    """`pandora map --max-covg M` on F writes the pandora_genotyped.vcf that `--max-covg 4294967295` writes on F cut to its first n reads,
    byte for byte -- and not the one of the whole file (today's behaviour: the option was parsed and ignored)"""
    from drprg_amd import synth
    from drprg_amd._lib import PANDORA_EXE
    panel, genomes = _panel()
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    panel.write(prg, genes)
    bases, offs = synth.sample_short_reads(genomes, 12000, seed=14)
    fq, cut = str(tmp_path / "reads.fq"), str(tmp_path / "cut.fq")
    synth.write_fastq_fixed(fq, bases, 150)
    g, cap = 20000, 30
    n, n_bases, reached = accepted_reads(_fastq_lengths(fq), g, cap)
    assert reached and n == 4134
    _truncated_fastq(fq, cut, n)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    vcfs = {}
    for name, reads, m in (("capped", fq, cap), ("truncated", cut, OFF), ("whole", fq, OFF)):
        out = tmp_path / name
        r = subprocess.run([PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(g), "--max-covg", str(m),
                            "--vcf-refs", genes, "-t", "4", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert (f"stopped reading at {n} reads: max coverage reached" in r.stdout) == (name == "capped"), r.stdout
        assert f"reads={n if name != 'whole' else 12000} " in r.stdout, r.stdout
        vcfs[name] = open(out / "pandora_genotyped.vcf", "rb").read()
    assert vcfs["capped"] == vcfs["truncated"]
    assert vcfs["capped"] != vcfs["whole"]


def test_pandora_discover_with_a_cap_equals_the_truncated_file_and_tags_its_coverage(tmp_path):
    """the four files of `pandora discover` under a cap equal those of an uncapped run on the truncated file, with the second pass from
    HBM and (DRPRG_HIP_KEEP_READS_GB=0) from the file; the coverage it leaves is taken by a `map` under the same cap only"""
    from drprg_amd._lib import PANDORA_EXE
    from test_resident import K as RK, W as RW, _files, _sample
    panel, prg, genes, fq = _sample(tmp_path, n_background=20000)
    g, cap = 4000, 300  # (the executable's default cap: T = 1 204 000 bases of the file's 3 405 000)
    n, n_bases, reached = accepted_reads(_fastq_lengths(fq), g, cap)
    assert reached and n == 8027
    cut = str(tmp_path / "cut.fq")
    _truncated_fastq(fq, cut, n)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "4", "-w", str(RW), "-k", str(RK), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    outs = {}
    for name, reads, m, gb in (("capped_hbm", fq, cap, None), ("capped_file", fq, cap, "0"), ("cut_hbm", cut, OFF, None), ("cut_file", cut, OFF, "0")):
        q = tmp_path / f"{name}.tsv"
        q.write_text(f"s\t{reads}\n")
        env = dict(os.environ)
        if gb is not None:
            env["DRPRG_HIP_KEEP_READS_GB"] = gb
        r = subprocess.run([PANDORA_EXE, "discover", "-g", str(g), "--max-covg", str(m), "-v", "-o", str(tmp_path / name / "discover"), "-t", "4", "-w", str(RW),
                            "-k", str(RK), "-c", "10", "-I", prg, str(q)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert ("resident in device memory" in r.stdout) == (gb is None), r.stdout
        assert ("max coverage reached" in r.stdout) == name.startswith("capped"), r.stdout
        outs[name] = _files(tmp_path / name / "discover")
    assert outs["capped_hbm"] == outs["cut_hbm"] == outs["capped_file"] == outs["cut_file"]
    assert b"1 denovo variants" in outs["capped_hbm"]["denovo_paths.txt"]  # (a third of the reads still shows the sample's off-panel change)
    # the coverage discover left under cap 300: a map under the same cap takes it, a map under another cap maps the reads itself
    for m, reused in ((cap, True), (200, False), (OFF, False)):
        r = subprocess.run([PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(tmp_path / "capped_hbm"), "-g", str(g), "--max-covg", str(m),
                            "--vcf-refs", genes, "-t", "4", "-w", str(RW), "-k", str(RK), "-c", "10", "-I", prg, fq], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert ("no second mapping pass" in r.stdout) == reused, r.stdout


def test_pandora_map_uncapped_over_two_devices(tmp_path):
    """the drop-in executable over "two devices" (device 0 listed twice) with the cap switched off, as drprg runs it: every block goes
    through the concurrent hand-over -- any parser thread, the first idle device -- and the VCF is that of the one-device run; under the
    executable's default cap the same file stops at n reads on one device and on two"""
    from drprg_amd import synth
    from drprg_amd._lib import PANDORA_EXE
    panel = synth.small_panel(seed=17, n_loci=5, length=900)
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    panel.write(prg, genes)
    gen = synth.HaplotypeGenomes(panel, genome_size=60000, n_hap=4, seed=3)
    n_reads = 1_000_000  # 150 M bases: about ten ingest blocks
    bases, offs = synth.sample_short_reads(gen, n_reads, seed=4)
    fq = str(tmp_path / "reads.fq")
    synth.write_fastq_fixed(fq, bases, 150)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n_default, _, reached = accepted_reads(np.diff(offs), 60000, 300)
    assert reached and n_default == 120_400
    for cap, n in ((OFF, n_reads), (None, n_default)):
        vcfs = []
        for devs in ("0", "0,0"):
            out = tmp_path / f"out_{cap}_{devs.replace(',', '_')}"
            argv = [PANDORA_EXE, "map", "--genotype", "--local", "-v", "-o", str(out), "-g", "60000"] + (["--max-covg", str(cap)] if cap is not None else [])
            r = subprocess.run(argv + ["--vcf-refs", genes, "-t", "8", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, fq], capture_output=True, text=True,
                               env=dict(os.environ, DRPRG_HIP_DEVICES=devs))
            assert r.returncode == 0, r.stderr
            assert f"reads={n} bases={n * 150} " in r.stdout, r.stdout
            assert ("max coverage reached" in r.stdout) == (cap is None), r.stdout
            vcfs.append(open(out / "pandora_genotyped.vcf", "rb").read())
        assert vcfs[0] == vcfs[1] and vcfs[0].count(b"\n") > 30
