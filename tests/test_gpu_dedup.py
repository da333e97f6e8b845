"""Exact duplicate reads dropped from the resident sample (drprg_hip_dedup, csrc/dedup.hip; pytest -m gpu).  The keys, the flags and the
four numbers come from the rule in plain Python (tests/dedup_rule.py), the vectors and counters from the oracle on the reads the rule
keeps, the files from runs that were given those reads alone -- never from the code under test.

How the reads get resident: as in tests/test_gpu_subsample.py -- one small file = one block, several files = several blocks, in ASCII,
packed and BAM form."""
import os
import subprocess

import numpy as np
import pytest

import bam_writer
from bam_writer import Rec
from dedup_rule import keep_flags, keep_flags_fast, key
from max_covg_rule import accepted_reads
from subsample_rule import keep_flags as subsample_keep_flags
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from test_gpu_subsample import _assert_oracle, _map_files, _pandora_map
from util import vcf_without_date

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
EINVAL, ENODATA = 22, 61
TILE = 65536  # bases per workgroup of dedup_keys_kernel
_COMP = bytes.maketrans(b"ACGTNR", b"TGCANY")


# ---- 1. keys equal the rule -------------------------------------------------------------------------------------------------------------
def _pack(reads):
    """the packed form of a batch: words (letter = bits 2:1 of the byte, whatever it is), the positions of the bytes that are not
    ACGTacgt, offsets"""
    flat = np.frombuffer(b"".join(reads), np.uint8)
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    n = flat.size
    pad = np.zeros((n + 15) // 16 * 16, np.uint32)
    pad[:n] = (flat >> 1) & 3
    words = (pad.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    npos = np.flatnonzero(~np.isin(flat, np.frombuffer(b"ACGTacgt", np.uint8))).astype(np.uint64)
    return words, npos, offs


def _device_keys(ctx, torch, reads, shift_words=0):
    words, npos, offs = _pack(reads)
    n_reads, n_bases = len(reads), int(offs[-1])
    buf = np.zeros(words.size + 4 + shift_words, np.uint32)
    buf[shift_words:shift_words + words.size] = words
    d_w = torch.from_numpy(buf.view(np.int32)).cuda()
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_n = torch.from_numpy(npos.astype(np.int64)).cuda() if npos.size else None
    d_k = torch.full((max(n_reads, 1),), -1, dtype=torch.int64, device="cuda")  # (stale on purpose)
    ctx.dedup_keys_device(d_w.data_ptr() + 4 * shift_words, d_o.data_ptr(), n_reads, n_bases, d_n.data_ptr() if npos.size else None, npos.size, d_k.data_ptr())
    torch.cuda.synchronize()
    return d_k.cpu().numpy().view(np.uint64)[:n_reads].tolist()


def _ragged_reads():
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def read(L):
        return bytearray(rng.choice(acgt, size=L).tobytes())

    reads = [b"", b"", b""]
    for L in range(0, 71):  # every phase and every L mod 16, 1, 15, 16, 17, 31, 32, 33 among them
        reads.append(bytes(read(L)))
    reads += [b""] * 4
    for L in (1, 2, 15, 16, 17, 31, 32, 33, 48, 70):  # masked bases at the first base, the last, both sides of a word boundary, everywhere
        for places in ([0], [L - 1], [15, 16], [0, L - 1], range(L)):
            r = read(L)
            for p in places:
                if p < L:
                    r[p] = ord("N") if p % 2 else ord("R")
            reads.append(bytes(r))
        reads.append(b"")
    long_read = read(2 * TILE + 9001)  # tile edges fall inside it
    for p in (0, 15, 16, TILE - 1, TILE, 2 * TILE + 9000):
        long_read[p] = ord("N")
    reads.append(bytes(long_read))
    for _ in range(900):  # short reads over more than one further tile: many reads per workgroup
        reads.append(bytes(read(int(rng.integers(0, 200)))))
    for _ in range(3000):  # reads of 1 .. 30 bases: more of them under one tile than the workgroup has sums in LDS (1024)
        reads.append(bytes(read(int(rng.integers(1, 31)))))
    reads.append(bytes(read(13)))
    reads += [b"", b""]
    return reads


def test_keys_of_the_kernel_equal_the_rule(tmp_path):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    reads = _ragged_reads()
    n_bases = sum(len(r) for r in reads)
    assert n_bases % 16 != 0 and n_bases > 3 * TILE and reads[:3] == [b""] * 3 and reads[-2:] == [b""] * 2
    starts = np.cumsum([0] + [len(r) for r in reads[:-1]])
    assert np.bincount(starts // TILE).max() > 1024 + 200  # (reads that start in one tile: some go past the workgroup's array of sums)
    want = [key(r) for r in reads]
    assert len({w for w, r in zip(want, reads) if r}) == len({r for r in reads if r})  # (no two different reads of the fixture share a key)
    got = _device_keys(ctx, torch, reads)
    assert got == want, [i for i in range(len(reads)) if got[i] != want[i]][:8]
    # the same reads behind a read of 5 bases: every phase moves, the keys of the common reads stay
    shifted = _device_keys(ctx, torch, [b"ACGTA"] + reads)
    assert shifted[1:] == want and shifted[0] == key(b"ACGTA")
    # a word buffer that is not 16-byte aligned is read word by word: the same keys
    assert _device_keys(ctx, torch, reads, shift_words=1) == want
    # a batch without listed positions takes no bitmap at all
    plain = [r for r in reads if set(r) <= set(b"ACGT")]
    assert _device_keys(ctx, torch, plain) == [key(r) for r in plain]
    # offsets that do not end at n_bases are refused, and nothing is written out of bounds
    words, npos, offs = _pack(reads[:200])
    bad = offs.copy()
    bad[-1] += 40
    d_w, d_o = torch.from_numpy(words.view(np.int32)).cuda(), torch.from_numpy(bad.astype(np.int64)).cuda()
    d_k = torch.zeros(200, dtype=torch.int64, device="cuda")
    with pytest.raises(DependencyError) as e:
        ctx.dedup_keys_device(d_w.data_ptr(), d_o.data_ptr(), 200, int(offs[-1]), None, 0, d_k.data_ptr())
    assert e.value.code == EINVAL
    ctx.close()


# ---- 2. flags and the four numbers equal the rule ---------------------------------------------------------------------------------------
_FIXTURE = {}


def _dup_fixture():
    """about 5 000 reads of 0 .. 400 bases: originals cut from the haplotype genomes in upper case (some with an N), about 30 % copies at
    random later places, and the near-misses of the rule.  Every lower-case or R-bearing read is a copy of an upper-case / N-bearing read
    in front of it, so the reads the rule keeps are upper-case ACGTN: what the oracle maps."""
    if _FIXTURE:
        return _FIXTURE["v"]
    panel, genomes = _panel()
    rng = np.random.default_rng(31)
    n0 = 3300
    L = np.where(rng.random(n0) < 0.3, rng.integers(0, 401, size=n0), rng.integers(0, 151, size=n0))
    for at in rng.integers(0, n0 - 40, size=8):
        L[at:at + int(rng.integers(2, 20))] = 0
    L[:3] = 0
    L[-2:] = 0
    L = [int(x) for x in L]
    bases, offs = _reads_of(genomes, L, seed=5)
    orig = [bytearray(bases[int(offs[i]):int(offs[i + 1])].tobytes()) for i in range(n0)]
    for i in range(0, n0, 9):  # an N somewhere in every ninth read
        if L[i]:
            orig[i][int(rng.integers(0, L[i]))] = ord("N")
    orig = [bytes(r) for r in orig]
    placed = [(float(i), r) for i, r in enumerate(orig)]
    rot = bytes.maketrans(b"ACGTN", b"CGTAA")
    for _ in range(1700):
        i = int(rng.integers(0, n0))
        r = orig[i]
        what = rng.random()
        if what < 0.60 or not r:
            v = r  # a copy
        elif what < 0.68:
            v = r.lower()  # case: a duplicate
        elif what < 0.76:
            v = r.replace(b"N", b"R")  # N against R: a duplicate
        elif what < 0.82:
            v = r[:-1] + r[-1:].translate(rot)  # differs in the last base only
        elif what < 0.88:
            v = r + b"A"  # one trailing base more (letter 0)
        elif what < 0.92:
            v = r[:-1]  # one trailing base less
        else:
            p = r.find(b"A")  # N against A at one place
            v = r[:p] + b"N" + r[p + 1:] if p >= 0 else r
        placed.append((float(rng.uniform(i, n0)), v))
    placed.sort(key=lambda t: t[0])  # (stable: an original stands in front of everything made from it)
    reads = [r for _, r in placed]
    flags = keep_flags(reads)
    assert 0.2 < 1 - sum(flags) / len(flags) < 0.4 and sum(len(r) for r in reads) < 700_000 and max(len(r) for r in reads) == 400
    kept = [r for r, f in zip(reads, flags) if f]
    assert all(set(r) <= set(b"ACGTN") for r in kept)
    _FIXTURE["v"] = (panel, reads, flags)
    return _FIXTURE["v"]


def _batch(reads):
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return (np.frombuffer(b"".join(reads), np.uint8) if offs[-1] else np.zeros(0, np.uint8)), offs


def _write_fastq(path, reads):
    with open(path, "wb") as fh:
        for i, r in enumerate(reads):
            fh.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    return str(path)


def _write_bam(path, reads):
    """every third record stored on the reverse strand: the read it becomes is the one given"""
    recs = []
    for i, r in enumerate(reads):
        u = r.upper()
        recs.append(Rec(u.translate(_COMP)[::-1].decode(), flag=0x10, name=b"b%d" % i) if i % 3 == 0 else Rec(u.decode(), flag=0, name=b"b%d" % i))
    return str(bam_writer.write(path, recs))


def _write_layout(d, reads, cuts, forms, tag):
    files, formats = [], []
    for i, form in enumerate(forms):
        part = reads[cuts[i]:cuts[i + 1]]
        files.append(_write_bam(d / f"{tag}_{i}.bam", part) if form == "bam" else _write_fastq(d / f"{tag}_{i}.fq", part))
        formats.append(form != "ascii")
    return files, formats


def test_flags_and_counts_equal_the_rule(tmp_path):
    panel, reads, want = _dup_fixture()
    n, S = len(reads), sum(len(r) for r in reads)
    kept_bases = sum(len(r) for r, f in zip(reads, want) if f)
    layouts = {
        "one block": ([0, n], ["packed"]),
        "four blocks in mixed forms": ([0, 1300, 2500, 3800, n], ["packed", "ascii", "bam", "ascii"]),
    }
    # (the BAM block holds upper-case text: the rule does not tell the cases apart, so the expected flags are the same)
    assert sum(1 for i in range(2500, 3800) if not want[i]) > 100 and sum(1 for i in range(1300, 2500) if not want[i]) > 100  # duplicates across blocks
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    for name, (cuts, forms) in layouts.items():
        files, formats = _write_layout(tmp_path, reads, cuts, forms, name.split()[0])
        for key_bits in (64, 8, 1):
            _map_files(ctx, files, formats)
            assert ctx.resident_info()["complete"] and ctx.resident_info()["blocks"] == len(forms)
            out = ctx.dedup(key_bits)
            got = ctx.dedup_flags(n)
            assert out == dict(reads_before=n, bases_before=S, reads_kept=sum(want), bases_kept=kept_bases), (name, key_bits, out)
            assert got.tolist() == want, (name, key_bits, np.flatnonzero(got != np.array(want))[:8])
            cnt = ctx.counters()
            assert cnt["reads"] == sum(want) and cnt["bases"] == kept_bases and ctx.resident_info()["complete"], (name, key_bits, cnt)
    # one block of empty reads only: nothing is a duplicate
    _map_files(ctx, [_write_fastq(tmp_path / "empty.fq", [b""] * 7)], [True])
    assert ctx.dedup() == dict(reads_before=7, bases_before=0, reads_kept=7, bases_kept=0) and ctx.dedup_flags(7).tolist() == [1] * 7
    assert ctx.counters()["reads"] == 7
    ctx.close()


# ---- 3. the context afterwards equals the oracle on the kept reads ----------------------------------------------------------------------
def test_the_context_afterwards_is_that_of_the_kept_reads(tmp_path, oracle):
    panel, reads, flags = _dup_fixture()
    n = len(reads)
    kept = [r for r, f in zip(reads, flags) if f]
    kb, ko = _batch(kept)
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    cuts, forms = [0, 1700, 3400, n], ["packed", "ascii", "packed"]
    files, formats = _write_layout(tmp_path, reads, cuts, forms, "ctx")
    _map_files(ctx, files, formats)
    out = ctx.dedup()
    assert out["reads_kept"] == len(kept) and ctx.dedup_flags(n).tolist() == flags
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    want = _oracle_map(oracle, idx, kb, ko, W, K, True)
    assert want[2]["clusters_kept"] > 5
    _assert_oracle(ctx, want, len(kept), int(ko[-1]), "after dedup")
    info = ctx.resident_info()
    assert info["complete"] and info["blocks"] == 3
    (tmp_path / "second").mkdir()
    second = _ctx(tmp_path / "second", panel, W, K, True, genome_size=G)
    second.map_resident(ctx)
    _assert_oracle(second, want, len(kept), int(ko[-1]), "map_resident of the kept reads")
    second.close()
    # the selection kernel sees kept reads only: every read that comes back is one of them, each at most once per copy the rule kept
    from test_gpu_read_selection import code
    anchors = sorted({r[100:115] for r in kept if len(r) >= 200 and set(r[100:115]) <= set(b"ACGT")})[:6]
    assert len(anchors) >= 3
    sb, so, _ = ctx.select_reads([code(a) for a in anchors], 15)
    selected = [bytes(sb[int(so[i]):int(so[i + 1])]).upper() for i in range(len(so) - 1)]
    assert len(selected) >= 3 and len(set(selected)) == len(selected) and set(selected) <= {r.upper() for r in kept}
    # a second call drops nothing and touches nothing
    before = (ctx.coverage(), ctx.counters(), ctx.resident_info())
    assert ctx.dedup() == dict(reads_before=len(kept), bases_before=int(ko[-1]), reads_kept=len(kept), bases_kept=int(ko[-1]))
    assert ctx.dedup_flags(len(kept)).tolist() == [1] * len(kept)
    after = (ctx.coverage(), ctx.counters(), ctx.resident_info())
    assert after[1:] == before[1:] and all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
    # a subsample behind it numbers the kept reads from 0
    KL = [len(r) for r in kept]
    T, seed = int(ko[-1]) // 3, 5
    sflags = subsample_keep_flags(KL, T, seed)
    sout = ctx.subsample(T, seed)
    assert sout["reads_before"] == len(kept) and sout["reads_kept"] == sum(sflags) and ctx.subsample_flags(len(kept)).tolist() == sflags
    sel = [r for r, f in zip(kept, sflags) if f]
    b2, o2 = _batch(sel)
    _assert_oracle(ctx, _oracle_map(oracle, idx, b2, o2, W, K, True), len(sel), int(o2[-1]), "subsample behind dedup")
    # under a depth cap the reads that arrive are the cap's prefix, and the flags are the rule's on that prefix
    L = [len(r) for r in reads]
    cap = 20
    n_acc, _, reached = accepted_reads(L, G, cap)
    assert reached and 1000 < n_acc < n
    ctx.set_max_covg(cap)
    _map_files(ctx, files, formats)
    pflags = keep_flags(reads[:n_acc])
    assert 0 < sum(pflags) < n_acc
    out = ctx.dedup()
    assert out["reads_before"] == n_acc and out["reads_kept"] == sum(pflags) and ctx.dedup_flags(n_acc).tolist() == pflags
    pk = [r for r, f in zip(reads[:n_acc], pflags) if f]
    b3, o3 = _batch(pk)
    ocov, oprg, ocnt = _oracle_map(oracle, idx, b3, o3, W, K, True)
    cov, prg = ctx.coverage()
    assert np.array_equal(cov, ocov) and np.array_equal(prg, oprg) and ctx.counters()["reads"] == len(pk)
    ctx.set_max_covg(None)
    ctx.close()


# ---- 4. a sample without duplicates -----------------------------------------------------------------------------------------------------
def test_a_sample_without_duplicates_is_left_untouched(tmp_path, oracle):
    panel, reads, flags = _dup_fixture()
    kept = [r for r, f in zip(reads, flags) if f]
    kb, ko = _batch(kept)
    n = len(kept)
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    files, formats = _write_layout(tmp_path, kept, [0, 1500, n], ["packed", "ascii"], "nodup")
    _map_files(ctx, files, formats)
    before = (ctx.coverage(), ctx.counters(), ctx.resident_info())
    for key_bits in (64, 3):
        out = ctx.dedup(key_bits)
        assert out == dict(reads_before=n, bases_before=int(ko[-1]), reads_kept=n, bases_kept=int(ko[-1]))
        assert ctx.dedup_flags(n).tolist() == [1] * n
        after = (ctx.coverage(), ctx.counters(), ctx.resident_info())
        assert after[1:] == before[1:] and all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True)
    _assert_oracle(ctx, want, n, int(ko[-1]), "untouched")
    ctx.close()


# ---- 5. a file of several blocks ----------------------------------------------------------------------------------------------------------
def test_a_file_of_several_blocks_is_numbered_in_file_order(tmp_path):
    from drprg_amd import synth
    from drprg_amd.pandora import DependencyError
    panel, genomes = _panel()
    n = 240_000
    bases, offs = synth.sample_short_reads(genomes, n, seed=12)
    block = bases.reshape(n, 150).copy()
    rng = np.random.default_rng(2)
    for i in range(19, n, 20):  # one read in 20 repeats a read somewhere in front of it, mostly in another ingest block
        block[i] = block[int(rng.integers(0, i))]
    fq = str(tmp_path / "big.fq")
    synth.write_fastq_fixed(fq, block.reshape(-1), 150)
    want = np.array(keep_flags_fast([row.tobytes() for row in block]), np.uint8)
    # every repeat goes; so do the many reads that are equal by chance (240 000 error-poor reads of four 20 kb haplotypes, either strand)
    assert not want[19::20].any() and n // 5 < int(want.sum()) < n - n // 20
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 30)
    ctx.set_threads(4)
    for packed in (True, False):
        ctx.reset()
        ctx.set_input_format(packed)
        ctx.set_ordered_ingest(True)
        ctx.map_fastx(fq)
        assert ctx.resident_info()["complete"] and ctx.resident_info()["blocks"] >= 2
        out = ctx.dedup()
        assert out == dict(reads_before=n, bases_before=150 * n, reads_kept=int(want.sum()), bases_kept=150 * int(want.sum())), out
        assert np.array_equal(ctx.dedup_flags(n), want)
        assert ctx.counters()["reads"] == int(want.sum())
    ctx.reset()
    ctx.set_ordered_ingest(False)
    ctx.map_fastx(fq)
    assert ctx.resident_info()["blocks"] >= 2
    with pytest.raises(DependencyError) as e:
        ctx.dedup()
    assert e.value.code == EINVAL and "drprg_hip_set_ordered_ingest" in str(e.value)
    ctx.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(tmp_path, oracle):
    from drprg_amd import Context
    from drprg_amd.pandora import DependencyError
    panel, reads, flags = _dup_fixture()
    reads = reads[:2000]
    flags = keep_flags(reads)
    bases, offs = _batch(reads)
    S = int(offs[-1])
    fq = _write_fastq(tmp_path / "r.fq", reads)
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), *_batch([r.upper() for r in reads]), W, K, True)

    def refused(c, code, text, call=lambda c: c.dedup()):
        state = (c.coverage(), c.counters(), c.resident_info())
        with pytest.raises(DependencyError) as e:
            call(c)
        assert e.value.code == code and text in str(e.value), e.value
        after = (c.coverage(), c.counters(), c.resident_info())
        assert after[1:] == state[1:] and all(np.array_equal(x, y) for x, y in zip(state[0], after[0]))

    # no dedup call yet: there are no flags
    with pytest.raises(DependencyError) as e:
        ctx.dedup_flags(2000)
    assert e.value.code == EINVAL
    # the reads are not resident: keep_reads off, then over its limit
    ctx.map_fastx(fq)
    refused(ctx, ENODATA, "DRPRG_HIP_KEEP_READS_GB")
    _assert_oracle(ctx, want, 2000, S, "not resident")
    ctx.reset()
    ctx.keep_reads(1000)
    ctx.map_fastx(fq)
    assert not ctx.resident_info()["complete"]
    refused(ctx, ENODATA, "DRPRG_HIP_KEEP_READS_GB")
    _assert_oracle(ctx, want, 2000, S, "over the limit")
    # key_bits outside 1..64
    ctx.keep_reads(1 << 28)
    ctx.reset()
    ctx.map_fastx(fq)
    assert ctx.resident_info()["complete"]
    for bits in (0, 65):
        refused(ctx, EINVAL, "key_bits", lambda c: c.dedup(bits))
    _assert_oracle(ctx, want, 2000, S, "key_bits")
    # the flags of a call, asked for with the wrong number of reads
    out = ctx.dedup()
    assert out["reads_kept"] == sum(flags) < 2000
    for n in (1999, 2001, sum(flags), 0):
        with pytest.raises(DependencyError) as e:
            ctx.dedup_flags(n)
        assert e.value.code == EINVAL, n
    assert ctx.dedup_flags(2000).tolist() == flags
    # a reset clears them; and the context maps on: the whole sample again, the oracle's vectors
    ctx.reset()
    with pytest.raises(DependencyError):
        ctx.dedup_flags(2000)
    ctx.map_fastx(fq)
    _assert_oracle(ctx, want, 2000, S, "after everything")
    ctx.close()
    # a context over several devices
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=[0, 0])
    multi.set_opts(illumina=True, genome_size=G)
    multi.keep_reads(1 << 28)
    multi.map_fastx(fq)
    refused(multi, EINVAL, "several devices")
    _assert_oracle(multi, want, 2000, S, "several devices")
    multi.close()


# ---- 7. the executables -------------------------------------------------------------------------------------------------------------------
def test_pandora_map_dedup_equals_the_run_on_the_kept_reads(tmp_path):
    from drprg_amd._lib import PANDORA_EXE
    panel, reads, flags = _dup_fixture()
    kept = [r for r, f in zip(reads, flags) if f]
    size = G
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    panel.write(prg, genes)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dup_fq, kept_fq = _write_fastq(tmp_path / "dup.fq", reads), _write_fastq(tmp_path / "kept.fq", kept)
    nocap = ["--max-covg", "4294967295"]
    stdout, got = _pandora_map(PANDORA_EXE, tmp_path / "dd", prg, genes, size, dup_fq, ["--dedup"] + nocap)
    _, want = _pandora_map(PANDORA_EXE, tmp_path / "kk", prg, genes, size, kept_fq, nocap)
    _, with_dups = _pandora_map(PANDORA_EXE, tmp_path / "all", prg, genes, size, dup_fq, nocap)
    assert got == want
    S, KS = sum(len(r) for r in reads), sum(len(r) for r in kept)
    assert f"dedup: reads_before={len(reads)} bases_before={S} reads_kept={len(kept)} bases_kept={KS}" in stdout and f"reads={len(kept)} " in stdout, stdout
    assert with_dups != want  # (the duplicates do change what the file reports)
    # in front of the subsample: the subsample of the kept reads
    _, got = _pandora_map(PANDORA_EXE, tmp_path / "dds", prg, genes, size, dup_fq, ["--dedup", "--subsample-covg", "8", "--seed", "3"])
    _, want = _pandora_map(PANDORA_EXE, tmp_path / "kks", prg, genes, size, kept_fq, ["--subsample-covg", "8", "--seed", "3"])
    assert got == want and KS > 8 * size
    # the sample must be resident: with that switched off the run fails, it never maps the duplicates silently
    r = subprocess.run([PANDORA_EXE, "map", "-o", str(tmp_path / "off"), "-g", str(size), "--dedup", "-w", str(W), "-k", str(K), "-I", prg, dup_fq],
                       capture_output=True, text=True, env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "pandora_genotyped.vcf").exists()


def test_drprg_predict_dedup_equals_the_run_on_the_kept_reads(tmp_path):
    from drprg_amd import synth
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 9000, seed=1)
    block = bases.reshape(9000, 150)
    rng = np.random.default_rng(4)
    src = np.concatenate([np.arange(9000), rng.integers(0, 9000, size=5000)])
    order = np.argsort(np.concatenate([np.arange(9000, dtype=np.float64), rng.uniform(src[9000:], 9000)]), kind="stable")
    dup = block[src[order]]
    flags = np.array(keep_flags_fast([row.tobytes() for row in dup]), bool)
    kept = dup[flags]
    assert 5000 < kept.shape[0] <= 9000 and dup.shape[0] == 14000  # (every inserted copy goes, and the reads that are equal by chance)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    fq_dup, fq_kept = str(tmp_path / "a" / "wt.fq"), str(tmp_path / "b" / "wt.fq")
    synth.write_fastq_fixed(fq_dup, dup.reshape(-1), 150)
    synth.write_fastq_fixed(fq_kept, kept.reshape(-1), 150)

    def run(fq, out, extra, env=None):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "-o", str(tmp_path / out), "-s", "wt", "-I", "-v"] + extra
        return subprocess.run(argv, capture_output=True, text=True, env=env)

    a, b = run(fq_dup, "dd", ["--dedup"]), run(fq_kept, "kk", [])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert (tmp_path / "dd" / "wt.drprg.json").read_bytes() == (tmp_path / "kk" / "wt.drprg.json").read_bytes()
    n_kept = kept.shape[0]
    assert f"dedup: reads_before=14000 bases_before={14000 * 150} reads_kept={n_kept} bases_kept={n_kept * 150}" in a.stderr, a.stderr
    assert f"] reads={n_kept} " in a.stderr
    r = run(fq_dup, "off", ["--dedup"], env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "wt.drprg.json").exists()
