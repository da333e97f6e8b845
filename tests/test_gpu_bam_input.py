"""BAM input on the device (pytest -m gpu): bam_pack.hip alone against the host packer on the rule's text, and BAM files through
map_fastx -- every kernel sequence, the depth cap, resident reads, two lanes, the executable -- against the oracle on the rule's reads
(tests/bam_rule.py) and against the FASTQ of the same reads.  The files come from tests/bam_writer.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bam_rule
import bam_writer
from bam_writer import Rec
from max_covg_rule import accepted_reads
from test_gpu_parity import _oracle_index, _oracle_map

pytestmark = pytest.mark.gpu

W, K = 11, 15
ALL16 = bam_writer.CODES
CHUNK = 16384  # bases one workgroup of bam_pack_kernel converts (csrc/bam_pack.hip: BP_CHUNK_WORDS * 16)
_REV = {c: bam_rule.COMPLEMENT[c] for c in ALL16}


def _stored(read_text, reverse):
    """the SEQ field that stands for this read under this flag"""
    return "".join(_REV[c] for c in reversed(read_text)) if reverse else read_text


# ---- the kernel alone -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kctx(tmp_path_factory):
    from drprg_amd import Context, synth
    d = tmp_path_factory.mktemp("bam_kernel")
    synth.small_panel(seed=42).write(str(d / "dr.prg"), str(d / "genes.fa"))
    ctx = Context(str(d / "dr.prg"), W, K, device=0, from_files=False)
    yield ctx
    ctx.close()


def _device_batch(torch, recs, scatter, rng):
    """the records' fields in one device buffer -- back to back in order, or scattered with gaps of 0xFF in a random order"""
    fields = [r.seq_bytes() for r in recs]
    order = list(rng.permutation(len(recs))) if scatter else list(range(len(recs)))
    buf, start = bytearray(), [0] * len(recs)
    for i in order:
        if scatter:
            buf += b"\xff" * int(rng.integers(0, 7))
        start[i] = len(buf)
        buf += fields[i]
    buf += b"\xff" * 3
    lens = [len(r.seq) for r in recs]
    offs = np.zeros(len(recs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    rev = np.array([1 if r.flag & 0x10 else 0 for r in recs], dtype=np.uint8)
    t = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).cuda()
    return t(np.frombuffer(bytes(buf), np.uint8), np.uint8), t(start or [0], np.int64), t(offs, np.int64), t(rev if len(rev) else [0], np.uint8), int(offs[-1])


def _check_kernel(ctx, recs, scatter=False, null_reverse=False, seed=0):
    import torch
    from drprg_amd.pandora import pack_reads
    rng = np.random.default_rng(seed)
    text = b"".join(bam_rule.read_of(r) for r in recs)
    want_words, want_npos = pack_reads(np.frombuffer(text, np.uint8))
    d_seq, d_start, d_offs, d_rev, n_bases = _device_batch(torch, recs, scatter, rng)
    assert n_bases == len(text)
    n_words = (n_bases + 15) // 16
    d_words = torch.full((n_words + 8,), -1, dtype=torch.int32, device="cuda")  # (the sentinel behind the last word must survive)
    cap = int(want_npos.size) + 3
    d_npos = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
    n = ctx.pack_device_bam(d_seq.data_ptr(), d_start.data_ptr(), d_offs.data_ptr(), None if null_reverse else d_rev.data_ptr(), len(recs), n_bases,
                            d_words.data_ptr(), d_npos.data_ptr(), cap)
    got = d_words.cpu().numpy().view(np.uint32)
    assert n == want_npos.size
    assert np.array_equal(got[:n_words], want_words), np.flatnonzero(got[:n_words] != want_words)[:8]
    assert np.all(got[n_words:] == 0xFFFFFFFF)
    npos = d_npos.cpu().numpy()
    assert np.array_equal(npos[:n].astype(np.uint64), want_npos) and np.all(npos[n:] == -1)
    return dict(d_seq=d_seq, d_start=d_start, d_offs=d_offs, d_rev=d_rev, n_bases=n_bases, want_npos=want_npos, n_words=n_words)


def _edge_records(seed=5):
    """lengths 0 .. 33 so that a forward and a reversed read that holds a whole word start at every base offset mod 16 (both parities of the
    word's first nibble in the field), every read once forward and once reversed, all 16 codes, a read of non-ACGT codes only, zero-length
    reads first, in the middle and last"""
    rng = np.random.default_rng(seed)
    recs = [Rec("", flag=4), Rec("", flag=0x10)]
    seen = set()
    at = 0
    while len(seen) < 32 or len(recs) < 200:
        L = int(rng.choice([0, 1, 2, 15, 16, 17, 31, 32, 33]))
        p = [0.235, 0.235, 0.235, 0.235] + [0.06 / 12] * 12
        s = "".join(rng.choice(list("ACGT" + "=MRSVWYHKDBN"), size=L, p=p))
        for flag in (0, 0x10):
            if L >= 32:
                seen.add((at % 16, flag))
            recs.append(Rec(_stored(s, flag), flag=flag, low_nibble_pad=int(rng.integers(0, 16))))
            at += L
        if rng.random() < 0.3:  # (the pair moves the start by 2 L: a single base now and then, or no forward read starts at an odd offset)
            recs.append(Rec("T", flag=0))
            at += 1
        if len(recs) >= 100 and not any(r.seq == ALL16 for r in recs):
            recs += [Rec("", flag=0), Rec(ALL16, flag=0), Rec(ALL16, flag=0x10), Rec("NRY=MKSWBDHV" * 3, flag=0x10), Rec("", flag=0x10)]
            at += 16 + 16 + 36
    assert len(seen) == 32
    recs += [Rec(ALL16 + "A", flag=0x10)]
    if sum(len(r.seq) for r in recs) % 16 == 0:
        recs.append(Rec("C", flag=0))
    return recs + [Rec("", flag=0), Rec("", flag=0x10)]


def test_kernel_edge_lengths_offsets_and_codes(kctx):
    recs = _edge_records()
    assert sum(len(r.seq) for r in recs) % 16 != 0  # the last word is partial: its tail bits must be clear
    _check_kernel(kctx, recs)
    _check_kernel(kctx, recs, scatter=True, seed=1)  # the fields scattered and out of order in d_seq
    fwd = [Rec(bam_rule.read_of(r).decode(), flag=0) for r in recs]
    _check_kernel(kctx, fwd, null_reverse=True)


def test_kernel_smallest_batches_and_a_long_odd_read(kctx):
    _check_kernel(kctx, [])
    _check_kernel(kctx, [Rec("G", flag=0)])
    _check_kernel(kctx, [Rec("N", flag=0x10)])
    _check_kernel(kctx, [Rec("", flag=0), Rec("", flag=0x10)])
    rng = np.random.default_rng(2)
    s = "".join(rng.choice(list("ACGTN"), size=1001, p=[0.24, 0.25, 0.25, 0.24, 0.02]))
    _check_kernel(kctx, [Rec(s, flag=0)])
    _check_kernel(kctx, [Rec(s, flag=0x10)])  # (odd length: the nibble parity of every base flips under the reversal)
    _check_kernel(kctx, [Rec(s, flag=0x10), Rec(s[:1000], flag=0x10), Rec(s, flag=0)])


def _workgroup_records():
    """four workgroups' worth of words and a partial last word; read boundaries on a word boundary and on each workgroup boundary but the
    second, which lies inside a long read; non-ACGT positions on either side of every workgroup boundary and nowhere near some others"""
    rng = np.random.default_rng(8)
    total = 4 * CHUNK + 16 * 5 + 7
    text = bytearray(rng.choice(list(b"ACGT"), size=total).tolist())
    for b in (CHUNK, 2 * CHUNK, 3 * CHUNK, 4 * CHUNK):
        for at, c in ((b - 17, b"R"), (b - 1, b"N"), (b, b"Y"), (b + 1, b"="), (b + 16, b"K")):
            text[at:at + 1] = c
    for at in (0, 15, 16, 5000, 5001, 5002, total - 1):
        text[at:at + 1] = b"N"
    cuts = [0]
    while cuts[-1] + 150 < CHUNK - 160:
        cuts.append(cuts[-1] + 150)
    cuts += [CHUNK - 160, CHUNK]                      # a read that ends on the first workgroup boundary (a word boundary as well)
    cuts += [CHUNK + 16 * 9, CHUNK + 16 * 9 + 33]     # a boundary on a word boundary inside a workgroup, then an odd one
    cuts += [2 * CHUNK + 4001]                        # one read across the second workgroup boundary
    while cuts[-1] + 151 < 3 * CHUNK - 200:
        cuts.append(cuts[-1] + 151)
    cuts += [3 * CHUNK, 3 * CHUNK, 3 * CHUNK + 1, 4 * CHUNK, total]  # (an empty read on a workgroup boundary)
    recs = []
    for i in range(len(cuts) - 1):
        flag = 0x10 if i % 2 else 0
        recs.append(Rec(_stored(bytes(text[cuts[i]:cuts[i + 1]]).decode(), flag), flag=flag))
    return recs, bytes(text)


def test_kernel_positions_ascend_across_workgroups(kctx):
    from drprg_amd._lib import lib
    recs, text = _workgroup_records()
    assert b"".join(bam_rule.read_of(r) for r in recs) == text and len(text) > 3 * CHUNK and len(text) % 16 != 0
    d = _check_kernel(kctx, recs)
    assert np.all(np.diff(d["want_npos"].astype(np.int64)) > 0) and d["want_npos"].size >= 20
    _check_kernel(kctx, recs, scatter=True, seed=3)
    # npos_cap one too small: -EOVERFLOW (75) with *n_npos set
    import torch
    n_want = int(d["want_npos"].size)
    d_words = torch.zeros(d["n_words"], dtype=torch.int32, device="cuda")
    d_npos = torch.full((n_want + 4,), -1, dtype=torch.int64, device="cuda")
    n = C.c_uint64(0)
    rc = lib.drprg_hip_pack_device_bam(kctx._h, d["d_seq"].data_ptr(), d["d_start"].data_ptr(), d["d_offs"].data_ptr(), d["d_rev"].data_ptr(), len(recs),
                                       d["n_bases"], d_words.data_ptr(), d_npos.data_ptr(), n_want - 1, C.byref(n), None)
    assert rc == -75 and n.value == n_want
    assert np.all(d_npos.cpu().numpy()[n_want - 1:] == -1)  # nothing written beyond the capacity given


# ---- through the file -------------------------------------------------------------------------------------------------------------------
def _records_of_reads(reads, seed, junk=True):
    """records whose reads (by the rule) are exactly `reads`, about half of them stored reversed, with secondary / supplementary records
    in between"""
    rng = np.random.default_rng(seed)
    recs = []
    for i, r in enumerate(reads):
        flag = int(rng.choice([0, 4, 0x10, 0x10 | 0x1 | 0x80, 0x400]))
        recs.append(Rec(_stored(r.decode(), flag & 0x10), flag=flag, name=b"r%d" % i, n_cigar=int(i % 3), tags=b"NMi\0\0\0\0" if i % 2 else b"",
                        low_nibble_pad=int(rng.integers(0, 16))))
        if junk and i % 11 == 0:
            recs.append(Rec("ACGTTGCATTGACCA" * 4, flag=int(rng.choice([0x100, 0x800, 0x910])), name=b"junk%d" % i))
    return recs


def _sample(n_reads=3000, seed=7):
    """a small panel and short reads of its haplotypes, some with non-ACGT codes, + the edge reads (empty, all 16 codes, N only)"""
    from drprg_amd import synth
    panel = synth.small_panel(seed=42)
    gen = synth.HaplotypeGenomes(panel, genome_size=20000, n_hap=4, seed=3)
    bases, offs = synth.sample_short_reads(gen, n_reads, seed=seed)
    bases = bases.copy()
    rng = np.random.default_rng(seed)
    for at in rng.integers(0, bases.size, 60):
        bases[at] = ord(rng.choice(list("NRY=K")))
    b = bases.tobytes()
    reads = [b[int(offs[i]):int(offs[i + 1])] for i in range(n_reads)]
    reads[5:5] = [b"", ALL16.encode(), b"NNNNNNNNNNNNNNNNNNNN"]
    reads.append(b"")
    return panel, reads


def _open(tmp_path, panel, kernel=0, devices=None, genome_size=20000):
    from drprg_amd import Context
    prg = str(tmp_path / "dr.prg")
    if not os.path.exists(prg):
        panel.write(prg, str(tmp_path / "genes.fa"))
    ctx = Context(prg, W, K, device=0, from_files=False) if devices is None else Context(prg, W, K, from_files=False, devices=devices)
    ctx.set_opts(illumina=True, genome_size=genome_size, kernel=kernel)
    ctx.prg_strings = panel.prgs
    return ctx


_KEYS = ("reads", "bases", "minimizers", "hits", "clusters_kept", "hits_kept")


def _assert_oracle(ctx, want, kernel_counts_all_minimizers, what):
    ocov, oprg, ocnt = want
    cov, prg = ctx.coverage()
    cnt = ctx.counters()
    print(what, cnt)
    for key in ("hits", "clusters_kept", "hits_kept") + (("minimizers",) if kernel_counts_all_minimizers else ()):
        assert cnt[key] == ocnt[key], (what, key)
    assert np.array_equal(prg, oprg) and np.array_equal(cov, ocov), what
    return cov, prg, cnt


@pytest.fixture(scope="module")
def sample(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("bam_sample")
    panel, reads = _sample()
    recs = _records_of_reads(reads, seed=1)
    assert bam_rule.reads_of(recs) == reads
    bam = str(bam_writer.write(d / "reads.bam", recs))
    bam_small = str(bam_writer.write(d / "reads_997.bam", recs, payload=997, eof=False))
    fq = d / "reads.fq"
    fq.write_bytes(bam_rule.fastq_of(reads))
    bases, offs = bam_rule.batch_of(reads)
    idx = _oracle_index(oracle, panel.prgs, W, K)
    want = _oracle_map(oracle, idx, bases, offs, W, K, True)
    return dict(panel=panel, reads=reads, recs=recs, bam=bam, bam_small=bam_small, fq=str(fq), bases=bases, offs=offs, want=want, idx=idx)


@pytest.mark.parametrize("kernel", [0, 3, 1], ids=["filtered", "wave", "generic"])
def test_map_fastx_of_a_bam_equals_the_oracle_and_the_fastq(tmp_path, sample, kernel):
    ctx = _open(tmp_path, sample["panel"], kernel)
    ctx.set_threads(4)
    ctx.map_fastx(sample["bam"])
    cov, prg, cnt = _assert_oracle(ctx, sample["want"], kernel != 0, f"bam kernel={kernel}")
    if kernel == 0:
        assert cnt["kernel"] == 2  # the small filtered tier reads the packed words itself
    assert cnt["reads"] == len(sample["reads"]) and cnt["bases"] == int(sample["offs"][-1])
    info = ctx.bam_info()
    assert {k: info[k] for k in ("records", "skipped", "reversed")} == bam_writer.counts(sample["recs"]) and info["device_blocks"] >= 1
    ctx.reset()
    assert ctx.bam_info() == dict(records=0, skipped=0, reversed=0, device_blocks=0)
    ctx.map_fastx(sample["fq"])
    fcov, fprg = ctx.coverage()
    fcnt = ctx.counters()
    assert np.array_equal(fcov, cov) and np.array_equal(fprg, prg)
    for key in _KEYS + ("kernel",):
        assert fcnt[key] == cnt[key], key
    assert ctx.bam_info() == dict(records=0, skipped=0, reversed=0, device_blocks=0)
    if kernel == 0:  # once more with 997-byte BGZF members, no EOF block and 8 threads
        ctx.reset()
        ctx.set_threads(8)
        ctx.map_fastx(sample["bam_small"])
        _assert_oracle(ctx, sample["want"], False, "997-byte members")
    ctx.close()


def test_depth_cap_cuts_inside_a_bam_block(tmp_path, sample, oracle):
    G, CAP = 10_000, 3  # T = 40 000 bases: the cut falls a few hundred reads into the one block
    reads = sample["reads"]
    n, n_bases, reached = accepted_reads([len(r) for r in reads], G, CAP)
    assert reached and 100 < n < len(reads) - 100
    bases, offs = bam_rule.batch_of(reads[:n])
    assert any(set(r) - set(b"ACGT") for r in reads[:n]) and any(set(r) - set(b"ACGT") for r in reads[n:])
    for kernel in (0, 3):
        ctx = _open(tmp_path, sample["panel"], kernel, genome_size=G)
        want = _oracle_map(oracle, sample["idx"], bases, offs, W, K, True)
        ctx.set_threads(2)
        ctx.set_max_covg(CAP)
        ctx.keep_reads(1 << 28)
        ctx.map_fastx(sample["bam"])
        info = ctx.max_covg_info()
        print(kernel, info)
        assert (info["reached"], info["reads"], info["bases"]) == (True, n, n_bases) and 0 <= info["dropped"] <= len(reads) - n
        _, _, cnt = _assert_oracle(ctx, want, kernel != 0, f"cap kernel={kernel}")
        assert cnt["reads"] == n and cnt["bases"] == n_bases
        assert ctx.resident_info()["complete"]
        other = _open(tmp_path, sample["panel"], kernel, genome_size=G)
        other.map_resident(ctx)
        assert other.counters()["reads"] == n
        _assert_oracle(other, want, kernel != 0, "resident prefix")
        other.close()
        ctx.close()


def test_resident_bam_blocks_serve_selection_and_a_second_mapping(tmp_path, sample):
    from test_gpu_read_selection import _fold, _split, code, ref_select
    reads = sample["reads"]
    ctx = _open(tmp_path, sample["panel"])
    ctx.set_threads(1)
    ctx.keep_reads(1 << 28)
    ctx.map_fastx(sample["bam"])
    info = ctx.resident_info()
    packed_bytes = (int(sample["offs"][-1]) + 15) // 16 * 4
    assert info["complete"] and info["blocks"] == 1 and packed_bytes <= info["bytes"] < int(sample["offs"][-1])  # kept packed: a quarter of the bases + offsets
    # a few anchors: 15-mers out of the middle of some reads, and one that no read holds
    A = 15
    anchors = sorted({r[40:40 + A] for r in reads[100:2000:317] if len(r) >= 60 and set(r[40:40 + A]) <= set(b"ACGT")} | {b"ACGTACGTACGTACG"})
    assert len(anchors) >= 4
    stream, offs = b"".join(reads), [int(x) for x in sample["offs"]]
    ref = ref_select(stream, offs, anchors, A)
    assert len(ref) >= len(anchors) - 1
    bases, offsets, ids = ctx.select_reads([code(a) for a in anchors], A)
    assert [int(i) for i in ids] == ref
    assert _split(bases, offsets) == [_fold(reads[r]) for r in ref]
    # the kept reads mapped into a second context == the file mapped there
    other = _open(tmp_path, sample["panel"])
    other.map_resident(ctx)
    _assert_oracle(other, sample["want"], False, "map_resident")
    rcov, rcnt = other.coverage()[0], other.counters()
    other.reset()
    other.map_fastx(sample["bam"])
    assert np.array_equal(other.coverage()[0], rcov)
    for key in _KEYS:
        assert other.counters()[key] == rcnt[key], key
    other.close()
    ctx.close()


def test_discover_reads_from_hbm_and_from_the_bam_file(tmp_path):
    from test_gpu_read_selection import _fastq_reads
    from test_resident import _discover, _files, _sample as _variant_sample
    panel, prg, genes, fq = _variant_sample(tmp_path, kind="snp")
    reads = [r.upper() for r in _fastq_reads(fq)]
    bam = str(bam_writer.write(tmp_path / "reads.bam", _records_of_reads(reads, seed=2)))
    a, va = _discover(prg, genes, bam, tmp_path / "file", 0)
    b, vb = _discover(prg, genes, bam, tmp_path / "hbm", 1 << 30)
    c, vc = _discover(prg, genes, fq, tmp_path / "fastq", 0)
    assert not a.resident_info()["last_discover_from_hbm"] and b.resident_info()["last_discover_from_hbm"] and b.resident_info()["complete"]
    assert len(va) == 1 and va == vb == vc
    assert _files(tmp_path / "file") == _files(tmp_path / "hbm") == _files(tmp_path / "fastq")
    for x in (a, b, c):
        x.close()


def test_two_lanes_of_one_device(tmp_path, sample):
    ctx = _open(tmp_path, sample["panel"], devices=[0, 0])
    ctx.set_threads(4)
    ctx.map_fastx(sample["bam_small"])
    _, _, cnt = _assert_oracle(ctx, sample["want"], False, "devices=[0, 0]")
    assert cnt["reads"] == len(sample["reads"]) and cnt["bases"] == int(sample["offs"][-1])
    info = ctx.bam_info()
    assert {k: info[k] for k in ("records", "skipped", "reversed")} == bam_writer.counts(sample["recs"])
    ctx.close()


def test_pandora_map_writes_the_same_vcf_from_bam_and_fastq(tmp_path, sample):
    """the drop-in executable with the reference's argv, a fresh child process per run"""
    from drprg_amd._lib import PANDORA_EXE
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    sample["panel"].write(prg, genes)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    vcfs = []
    for name, reads in (("bam", sample["bam"]), ("fq", sample["fq"])):
        out = tmp_path / name
        argv = [PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", "20000", "--max-covg", "4294967295",
                "--vcf-refs", genes, "-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert f"reads={len(sample['reads'])}" in r.stdout
        assert ("bam: records=%d" % len(sample["recs"]) in r.stdout) == (name == "bam"), r.stdout
        vcfs.append((out / "pandora_genotyped.vcf").read_bytes())
    assert vcfs[0] == vcfs[1] and b"\n" in vcfs[0]
