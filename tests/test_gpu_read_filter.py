"""The read filter (drprg_hip_set_read_filter, csrc/read_qual.hip; pytest -m gpu).  Sums, flags and counts come from the rule in plain Python
(tests/read_filter_rule.py), the vectors and counters from the oracle on the reads the rule keeps and from contexts that were given a file
of those reads alone -- never from the code under test.

How the blocks come about: the ingest hands a worker's first block over at 750 000 bases, so the small sample (under that) is one block
and the big one several, whatever the number of parser threads."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import bam_writer
import read_filter_rule as rule
from bam_writer import Rec
from max_covg_rule import accepted_reads
from read_filter_rule import KEEP, census, fates, qual_milli, qual_sum
from subsample_rule import keep_flags
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from util import vcf_without_date

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
EINVAL, EFORMAT = 22, 84
TILE = 16384  # bytes of the quality buffer per workgroup of read_qual_kernel
SETTINGS = dict(min_len=rule.MIN_LEN, max_len=rule.MAX_LEN, min_qual=rule.MIN_QUAL)
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _write_fastq(path, bases, offs, quals, gz=False):
    op = gzip.open if gz else open
    with op(path, "wb") as fh:
        for i in range(len(offs) - 1):
            s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
            fh.write(b"@r%d\n" % i + s + b"\n+\n" + (quals[i] + 33).astype(np.uint8).tobytes() + b"\n")
    return str(path)


def _write_bam(path, bases, offs, quals):
    """every third record stored on the reverse strand: SEQ is the reverse complement of the read, QUAL runs the other way"""
    recs = []
    for i in range(len(offs) - 1):
        s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
        q = quals[i].astype(np.uint8).tobytes()
        if i % 3 == 0:
            recs.append(Rec(s.translate(COMP)[::-1].decode(), flag=0x10, name=b"r%d" % i, qual=q[::-1]))
        else:
            recs.append(Rec(s.decode(), flag=4, name=b"r%d" % i, qual=q))
    return str(bam_writer.write(path, recs))


def _select(bases, offs, keep, quals=None):
    idx = [i for i, k in enumerate(keep) if k]
    parts = [bases[int(offs[i]):int(offs[i + 1])] for i in idx]
    o = np.zeros(len(idx) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([p.size for p in parts])
    b = np.concatenate(parts) if len(parts) and o[-1] else np.zeros(0, np.uint8)
    return (b, o) if quals is None else (b, o, [quals[i] for i in idx])


def _assert_oracle(ctx, want, n_reads, n_bases, what):
    ocov, oprg, ocnt = want
    cov, prg = ctx.coverage()
    cnt = ctx.counters()
    assert cnt["reads"] == n_reads and cnt["bases"] == n_bases, (what, cnt, n_reads, n_bases)
    for key in ("hits", "clusters_kept", "hits_kept"):
        assert cnt[key] == ocnt[key], (what, key)
    assert np.array_equal(prg, oprg) and np.array_equal(cov, ocov), what


_SAMPLES = {}


def _sample(which, oracle, ctx):
    """the sample's reads, the rule's verdict on them, and the oracle's vectors of the kept reads: made once, shared, left unchanged"""
    if which not in _SAMPLES:
        _, genomes = _panel()
        lengths, quals = rule.small_sample() if which == "small" else rule.big_sample()
        bases, offs = _reads_of(genomes, lengths, seed=41)
        bases = bases.copy()
        for i in range(0, len(lengths), 10):  # a base that is not ACGT in every tenth read, kept or dropped: packed blocks list positions
            bases[int(offs[i]) + 5] = ord("N")
        s = dict(lengths=lengths, quals=quals, bases=bases, offs=offs)
        for name, kw in (("all", SETTINGS), ("len", dict(min_len=rule.MIN_LEN, max_len=rule.MAX_LEN, min_qual=0))):
            T = rule.threshold(qual_milli(kw["min_qual"])) if kw["min_qual"] else 0
            what = fates(lengths, quals, kw["min_len"], kw["max_len"], T)
            keep = [w == KEEP for w in what]
            kb, ko, kq = _select(bases, offs, keep, quals)
            idx = _oracle_index(oracle, ctx.prg_strings, W, K)
            s[name] = dict(keep=keep, census=census((what, lengths)), bases=kb, offs=ko, quals=kq, want=_oracle_map(oracle, idx, kb, ko, W, K, True, threads=4))
        assert s["all"]["want"][2]["clusters_kept"] > 5
        _SAMPLES[which] = s
    return _SAMPLES[which]


def _info_counts(ctx):
    info = ctx.read_filter_info()
    info.pop("T")
    return info


# ---- 1. sums and flags of the kernel equal the rule -----------------------------------------------------------------------------------------
def _ragged():
    """about 100 kb: runs of empty reads at the start, at the end and on a tile edge; lengths 0, 1, 15, 16, 17 and 16383 .. 16385; a read over
    three tiles (one byte of the first, all of the second, fifteen of the third); reads that end on a lane edge and on a tile edge"""
    L = [0, 0, 0, 1, 15, 16, 17, 16334, 16400, 1, 16368, 0, 0, 0, 16383, 1, 16384, 16385, 16, 0, 0]
    o = np.zeros(len(L) + 1, dtype=np.uint64)
    o[1:] = np.cumsum(L)
    assert o[8] == TILE - 1 and o[9] == 2 * TILE + 15 and o[10] == 2 * TILE + 16 and o[11] == o[14] == 3 * TILE  # three tiles; lane edge; tile edge
    assert o[16] == 4 * TILE and o[17] == 5 * TILE and (o[18] - o[17]) == 16385 and o[19] % 16 == 1
    return L, o


def _device_filter(ctx, torch, quals_flat, offs, bias, pad=64, shift=0):
    """shift: the quality buffer starts that many bytes behind a 16-byte aligned address (it is read byte by byte then)"""
    n_reads, n_bases = len(offs) - 1, int(offs[-1])
    buf = np.zeros(shift + n_bases + pad, dtype=np.uint8)
    buf[shift:shift + n_bases] = quals_flat + bias
    d_q = torch.from_numpy(buf).cuda()
    assert d_q.data_ptr() % 16 == 0
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_s = torch.full((max(n_reads, 1),), -1, dtype=torch.int64, device="cuda")  # (stale on purpose)
    d_f = torch.full((max(n_reads, 1),), 7, dtype=torch.uint8, device="cuda")
    out = ctx.read_filter_device(d_q.data_ptr() + shift, bias, d_o.data_ptr(), n_reads, n_bases, d_s.data_ptr(), d_f.data_ptr())
    torch.cuda.synchronize()
    return out, d_s.cpu().numpy().astype(np.uint64)[:n_reads], d_f.cpu().numpy()[:n_reads]


@pytest.mark.parametrize("bias", [33, 0])
def test_sums_and_flags_of_the_kernel_equal_the_rule(tmp_path, bias):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    L, offs = _ragged()
    rng = np.random.default_rng(5 + bias)
    q = rng.integers(0, 94, size=int(offs[-1])).astype(np.uint8)
    q[0], q[1], q[int(offs[8])], q[int(offs[9]) - 1] = 0, 93, 93, 0
    # uniform qualities have a mean error near Q 12.9: a fractional threshold there splits the reads; T comes from the info call
    ctx.set_read_filter(min_len=1, max_len=16400, min_qual="12.9")
    T = ctx.read_filter_info()["T"]
    assert abs(T - rule.threshold(12900)) <= 1

    def check(L, offs, q, what, shift=0):
        per_read = [q[int(offs[i]):int(offs[i + 1])] for i in range(len(L))]
        sums = [qual_sum(x) for x in per_read]
        keep = [w == KEEP for w in fates(L, per_read, 1, 16400, T)]
        out, got_s, got_f = _device_filter(ctx, torch, q, offs, bias, shift=shift)
        assert got_s.tolist() == sums, (what, [i for i in range(len(L)) if int(got_s[i]) != sums[i]][:8])
        assert got_f.tolist() == [int(k) for k in keep], what
        assert out == (sum(keep), sum(l for l, k in zip(L, keep) if k), 0), (what, out)
        return keep

    keep = check(L, offs, q, "ragged")
    assert 0 < sum(keep) < len(L) - 8  # (the eight empty reads are short; the threshold keeps some of the rest and drops some)
    # the overflow route: more than 1 024 reads under one tile (tests/read_filter_rule.py: overflow_batch), 16-byte aligned and one byte off
    L3, behind, straddler = rule.overflow_batch()
    o3 = np.zeros(len(L3) + 1, dtype=np.uint64)
    o3[1:] = np.cumsum(L3)
    q3 = rng.integers(0, 94, size=int(o3[-1])).astype(np.uint8)
    for shift in (0, 1):
        keep3 = check(L3, o3, q3, ("overflow", shift), shift)
        assert 0 < sum(keep3) < len(L3) - 1100 and not any(keep3[behind - 1100:behind])
    # a second launch on the same context with a smaller batch: no sum of the first one is left behind
    L2 = [0, 2, 0, 3, 0]
    o2 = np.array([0, 0, 2, 2, 5, 5], dtype=np.uint64)
    check(L2, o2, np.array([0, 93, 40, 1, 12], dtype=np.uint8), "five bases")
    # a batch of empty reads only: nothing to sum, and the sums are still written
    check([0, 0, 0], np.zeros(4, dtype=np.uint64), np.zeros(0, dtype=np.uint8), "empty reads only")
    # a buffer that is not 16-byte aligned is read byte by byte: the same sums
    n_bases = int(offs[-1])
    buf = np.zeros(n_bases + 80, dtype=np.uint8)
    buf[3:3 + n_bases] = q + bias
    d_q, d_o = torch.from_numpy(buf).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
    d_s, d_f = torch.zeros(len(L), dtype=torch.int64, device="cuda"), torch.zeros(len(L), dtype=torch.uint8, device="cuda")
    ctx.read_filter_device(d_q.data_ptr() + 3, bias, d_o.data_ptr(), len(L), n_bases, d_s.data_ptr(), d_f.data_ptr())
    assert d_s.cpu().numpy().astype(np.uint64).tolist() == [qual_sum(q[int(offs[i]):int(offs[i + 1])]) for i in range(len(L))]
    # one byte out of range: -84, and the position is named
    for at, value in ((int(offs[8]) + TILE + 5, bias + 94), (77, 255 if bias == 0 else 32)):
        bad = q.astype(np.int64) + bias
        bad[at] = value
        buf = np.zeros(n_bases + 64, dtype=np.uint8)
        buf[:n_bases] = bad.astype(np.uint8)
        d_q = torch.from_numpy(buf).cuda()
        with pytest.raises(DependencyError) as e:
            ctx.read_filter_device(d_q.data_ptr(), bias, d_o.data_ptr(), len(L), n_bases, d_s.data_ptr(), d_f.data_ptr())
        assert e.value.code == EFORMAT and str(at) in str(e.value) and ctx.last_filter_out[2] == at + 1, (at, e.value)
    # without a threshold the qualities are not looked at (no buffer is needed) and the lengths alone decide
    ctx.set_read_filter(min_len=16, max_len=16384)
    out = ctx.read_filter_device(None, bias, d_o.data_ptr(), len(L), n_bases, None, d_f.data_ptr())
    want = [int(16 <= l <= 16384) for l in L]
    assert d_f.cpu().numpy().tolist() == want and out == (sum(want), sum(l for l, k in zip(L, want) if k), 0)
    ctx.close()


# ---- 2. a filtered sample equals the sample of its kept reads --------------------------------------------------------------------------------
FORMS = ["fastq ascii", "fastq packed", "bam", "fastq.gz"]


def _file_of(tmp_path, form, bases, offs, quals, tag):
    if form == "bam":
        return _write_bam(tmp_path / f"{tag}.bam", bases, offs, quals)
    if form == "fastq.gz":
        return _write_fastq(tmp_path / f"{tag}.fq.gz", bases, offs, quals, gz=True)
    return _write_fastq(tmp_path / f"{tag}.fq", bases, offs, quals)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["small", "big"])
def test_a_filtered_sample_equals_the_sample_of_its_kept_reads(tmp_path, oracle, which, form):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample(which, oracle, ctx)
    k = s["all"]
    ctx.set_threads(1 if which == "small" else 4)
    ctx.set_input_format(form == "fastq packed")
    ctx.keep_reads(1 << 28)
    ctx.set_read_filter(**SETTINGS)
    ctx.map_fastx(_file_of(tmp_path, form, s["bases"], s["offs"], s["quals"], "all"))
    n_kept, b_kept = k["census"]["reads_kept"], k["census"]["bases_kept"]
    _assert_oracle(ctx, k["want"], n_kept, b_kept, (which, form))
    assert _info_counts(ctx) == k["census"]
    info = ctx.resident_info()
    assert info["complete"] and (info["blocks"] == 1 if which == "small" else info["blocks"] >= 2), info
    # a second context that was given a file of only those reads, and no filter
    (tmp_path / "other").mkdir()
    other = _ctx(tmp_path / "other", panel, W, K, True, genome_size=G)
    other.set_threads(1)
    other.set_input_format(form == "fastq packed")
    other.keep_reads(1 << 28)
    other.map_fastx(_file_of(tmp_path, form, k["bases"], k["offs"], k["quals"], "kept"))
    assert ctx.counters() == other.counters()
    assert all(np.array_equal(x, y) for x, y in zip(ctx.coverage(), other.coverage()))
    if which == "small":  # one block either way: what stays resident is what the kept reads alone leave
        assert info == other.resident_info()
        if form in ("fastq packed", "bam"):
            assert (b_kept + 15) // 16 * 4 <= info["bytes"] < b_kept
    ctx.close()
    other.close()


# ---- 3. everything behind it sees the kept reads -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_everything_behind_the_filter_sees_the_kept_reads(tmp_path, oracle, packed):
    from test_gpu_read_selection import code
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    k = s["all"]
    kL = np.diff(k["offs"].astype(np.int64)).tolist()
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    kept_fq = _write_fastq(tmp_path / "kept.fq", k["bases"], k["offs"], k["quals"])
    ctx.set_threads(1)
    ctx.set_input_format(packed)
    ctx.keep_reads(1 << 28)
    ctx.set_ordered_ingest(True)
    ctx.set_read_filter(**SETTINGS)
    ctx.map_fastx(fq)
    (tmp_path / "other").mkdir()
    other = _ctx(tmp_path / "other", panel, W, K, True, genome_size=G)
    other.set_threads(1)
    other.set_input_format(packed)
    other.keep_reads(1 << 28)
    other.set_ordered_ingest(True)
    other.map_fastx(kept_fq)
    full_info = other.resident_info()
    assert ctx.resident_info() == full_info and full_info["blocks"] == 1 and full_info["complete"]
    # the selection kernel returns kept reads only: the same reads, under the same numbers, as from the context that never saw the others
    anchors = sorted({bytes(k["bases"][int(k["offs"][i]) + 100:int(k["offs"][i]) + 115]) for i in range(0, len(kL), 7) if kL[i] >= 300})[:8]
    dropped = [i for i, keep in enumerate(k["keep"]) if not keep and s["lengths"][i] >= 150][:40]
    anchors += [bytes(s["bases"][int(s["offs"][i]) + 60:int(s["offs"][i]) + 75]) for i in dropped]  # (anchors from dropped reads as well)
    a, b = ctx.select_reads([code(x) for x in anchors], 15), other.select_reads([code(x) for x in anchors], 15)
    assert a[2].size >= 8 and all(np.array_equal(x, y) for x, y in zip(a, b))
    # another context maps them from HBM
    (tmp_path / "third").mkdir()
    third = _ctx(tmp_path / "third", panel, W, K, True, genome_size=G)
    third.map_resident(ctx)
    _assert_oracle(third, k["want"], len(kL), int(k["offs"][-1]), "map_resident")
    third.close()
    # the subsample numbers the kept reads
    T = int(k["offs"][-1]) // 2
    flags = keep_flags(kL, T, 9)
    out = ctx.subsample(T, 9)
    assert out["reads_before"] == len(kL) and out["bases_before"] == int(k["offs"][-1]) and out["reads_kept"] == sum(flags)
    assert ctx.subsample_flags(len(kL)).tolist() == flags
    # the depth cap cuts on the kept reads' running total
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    for max_covg in (3, 8):
        n, n_bases, reached = accepted_reads(kL, G, max_covg)
        assert reached and 0 < n < len(kL)
        want = _oracle_map(oracle, idx, k["bases"][:n_bases], k["offs"][:n + 1], W, K, True)
        for c, path in ((ctx, fq), (other, kept_fq)):
            c.reset()
            c.set_max_covg(max_covg)
            c.map_fastx(path)
            info = c.max_covg_info()
            assert info["reached"] and info["reads"] == n and info["bases"] == n_bases, (max_covg, info)
            _assert_oracle(c, want, n, n_bases, ("cap", max_covg))
        assert ctx.resident_info() == other.resident_info()
    ctx.set_max_covg(None)
    # a block that loses every read: nothing is mapped, nothing is kept
    ctx.reset()
    ctx.set_read_filter(min_len=20_000)
    ctx.map_fastx(fq)
    assert ctx.counters()["reads"] == 0 and ctx.counters()["bases"] == 0 and not ctx.coverage()[0].any()
    assert ctx.resident_info()["blocks"] == 0 and ctx.resident_info()["bytes"] == 0
    assert _info_counts(ctx) == dict(reads_seen=len(s["lengths"]), bases_seen=sum(s["lengths"]), dropped_short=len(s["lengths"]), dropped_long=0, dropped_low_qual=0,
                                     reads_kept=0, bases_kept=0)
    # a block that loses none
    ctx.reset()
    ctx.set_read_filter(min_len=100, max_len=100_000, min_qual=1)
    ctx.map_fastx(kept_fq)
    _assert_oracle(ctx, k["want"], len(kL), int(k["offs"][-1]), "loses none")
    assert ctx.resident_info() == full_info
    assert _info_counts(ctx)["reads_kept"] == len(kL) == _info_counts(ctx)["reads_seen"]
    ctx.close()
    other.close()


def test_a_middle_block_that_loses_every_read(tmp_path, oracle):
    """three blocks of one file, the middle one of over-long reads only, reads not resident: the block that maps nothing must not hand the
    staging set of the block before it -- whose kernels may still be running -- to the block after it.  The ingest hands the first block
    over at 786 432 bases and the next at 12 582 912: the reads are sized to fill them exactly."""
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    lengths = [384] * 2048 + [8192] * 1536 + [384] * 512
    assert sum(lengths[:2048]) == 786_432 and sum(lengths[2048:2048 + 1536]) == 12_582_912
    bases, offs = _reads_of(genomes, lengths, seed=43)
    fq = str(tmp_path / "three.fq")
    with open(fq, "wb") as fh:
        for i, L in enumerate(lengths):
            fh.write(b"@r%d\n" % i + bases[int(offs[i]):int(offs[i + 1])].tobytes() + b"\n+\n" + b"I" * L + b"\n")
    keep = [L == 384 for L in lengths]
    kb, ko = _select(bases, offs, keep)
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    counts = dict(reads_seen=len(lengths), bases_seen=sum(lengths), dropped_short=0, dropped_long=1536, dropped_low_qual=0, reads_kept=2560, bases_kept=2560 * 384)
    ctx.set_threads(4)
    ctx.set_read_filter(min_len=100, max_len=5000, min_qual=20)
    for packed in (True, False):
        for keep_bytes in (0, 1 << 28):
            ctx.reset()
            ctx.set_input_format(packed)
            ctx.keep_reads(keep_bytes)
            ctx.map_fastx(fq)
            _assert_oracle(ctx, want, 2560, 2560 * 384, (packed, keep_bytes))
            assert _info_counts(ctx) == counts
            if keep_bytes:  # the three blocks were there: two of them left something to keep
                assert ctx.resident_info()["complete"] and ctx.resident_info()["blocks"] == 2
    ctx.close()


def test_later_blocks_outgrow_the_buffers_while_a_batch_is_in_flight(tmp_path):
    """The filtered path without keep_reads, blocks that grow: one parser thread hands over a first block at a sixteenth of the ingest's
    block size, then a full block, then what is left -- here three times the first.  The two staging sets take the blocks in turn, so the
    second block allocates its set while the first block's deferred batch is in flight, and the third block, larger than the first by more
    than the quarter a buffer is given on top, regrows every buffer of the first set -- staging, filter scratch, compaction tables, the
    compacted block -- while the second block's batch is in flight.  (Blocks of a few hundred reads cannot come about: the ingest hands
    nothing over below that sixteenth, 786 432 bases.)  Reads of 60 .. 150 bases, packed input, a base that is not ACGT in every tenth
    read, kept or dropped; the lower bound of 90 drops a third of every block.  Vectors, counters and the filter's counts equal those of a
    context that was given the kept reads alone and no filter; with the reads resident the same blocks give the same vectors again."""
    from test_gpu_max_covg import _ingest_block_bases
    panel, genomes = _panel()
    block, _ = _ingest_block_bases()
    first, min_len = block // 16, 90
    rng = np.random.default_rng(47)
    lengths = rng.integers(60, 151, size=(first + block + 3 * first) // 105)
    offs = np.zeros(lengths.size + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lengths)
    cut = np.searchsorted(offs, [first, first + block])  # the reads that complete the first and the second block
    sizes = np.diff(np.concatenate(([0], offs[cut], offs[-1:])))
    assert sizes[0] >= first and sizes[1] >= block and sizes[2] > sizes[0] * 5 // 4 + 4096, sizes
    genome = np.concatenate(genomes.haps)
    starts = rng.integers(0, genome.size - 150, size=lengths.size)  # (a read may run from one haplotype into the next: any text will do)
    bases = genome[np.repeat(starts - offs[:-1], lengths) + np.arange(offs[-1])]
    bases[offs[:-1:10] + 5] = ord("N")
    keep = lengths >= min_len
    for lo, hi in zip(np.concatenate(([0], cut)), np.concatenate((cut, [lengths.size]))):
        with_n = keep[lo:hi][np.arange(lo, hi) % 10 == 0]
        assert 0.25 < 1 - keep[lo:hi].mean() < 0.40 and with_n.any() and not with_n.all()  # a third of the block dropped; N in both kinds
    files = {}
    for name, sel in (("all", np.ones_like(keep)), ("kept", keep)):
        files[name] = str(tmp_path / f"{name}.fq")
        with open(files[name], "wb") as fh:
            fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bases[offs[i]:offs[i + 1]].tobytes(), b"I" * int(lengths[i])) for i in np.flatnonzero(sel)))
    n_kept, b_kept = int(keep.sum()), int(lengths[keep].sum())
    counts = dict(reads_seen=int(lengths.size), bases_seen=int(offs[-1]), dropped_short=int(lengths.size) - n_kept, dropped_long=0, dropped_low_qual=0,
                  reads_kept=n_kept, bases_kept=b_kept)
    (tmp_path / "plain").mkdir()
    plain = _ctx(tmp_path / "plain", panel, W, K, True, genome_size=G)
    plain.set_threads(1)
    plain.set_input_format(True)
    plain.map_fastx(files["kept"])
    want_cnt, want_cov = plain.counters(), plain.coverage()
    assert want_cnt["reads"] == n_kept and want_cnt["bases"] == b_kept and want_cnt["clusters_kept"] > 5
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.set_threads(1)
    ctx.set_input_format(True)
    ctx.set_read_filter(min_len=min_len)
    for keep_bytes in (0, 1 << 28):
        ctx.reset()
        ctx.keep_reads(keep_bytes)
        ctx.map_fastx(files["all"])
        assert ctx.counters() == want_cnt, keep_bytes
        assert all(np.array_equal(x, y) for x, y in zip(ctx.coverage(), want_cov)), keep_bytes
        assert _info_counts(ctx) == counts
        if keep_bytes:  # the three blocks were there
            assert ctx.resident_info()["complete"] and ctx.resident_info()["blocks"] == 3, ctx.resident_info()
    ctx.close()
    plain.close()


# ---- 4. two devices ------------------------------------------------------------------------------------------------------------------------------
def test_two_devices_give_the_vectors_of_one(tmp_path, oracle):
    from drprg_amd import Context
    panel, _ = _panel()
    one = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, one)
    k = s["all"]
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=[0, 0])
    multi.set_opts(illumina=True, genome_size=G)
    for c in (one, multi):
        c.set_threads(4)
        c.set_read_filter(**SETTINGS)
        c.map_fastx(fq)
        _assert_oracle(c, k["want"], k["census"]["reads_kept"], k["census"]["bases_kept"], "devices")
        assert _info_counts(c) == k["census"]
    one.close()
    multi.close()


# ---- 5. refusals and state -------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(tmp_path, oracle):
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    k, kl = s["all"], s["len"]
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    fa = str(tmp_path / "all.fa")
    with open(fa, "wb") as fh:
        for i in range(len(s["lengths"])):
            fh.write(b">r%d\n" % i + s["bases"][int(s["offs"][i]):int(s["offs"][i + 1])].tobytes() + b"\n")
    noq = str(bam_writer.write(tmp_path / "noq.bam", [Rec(s["bases"][int(s["offs"][i]):int(s["offs"][i + 1])].tobytes().decode(), flag=4, name=b"r%d" % i)
                                                      for i in range(len(s["lengths"]))]))
    ctx.set_threads(2)
    # no qualities under a quality threshold: refused, never silently kept or dropped
    ctx.set_read_filter(**SETTINGS)
    for path in (fa, noq):
        ctx.reset()
        with pytest.raises(DependencyError) as e:
            ctx.map_fastx(path)
        assert e.value.code == EINVAL and "--min-read-qual" in str(e.value), (path, e.value)
    # the same inputs under a length bound alone map without error, on the lengths
    ctx.set_read_filter(min_len=rule.MIN_LEN, max_len=rule.MAX_LEN)
    for path in (fa, noq):
        ctx.reset()
        ctx.map_fastx(path)
        _assert_oracle(ctx, kl["want"], kl["census"]["reads_kept"], kl["census"]["bases_kept"], path)
        assert _info_counts(ctx) == kl["census"]
    # a quality byte out of range: -84
    bad = [q.copy() for q in s["quals"]]
    bad[len(bad) // 2][3] = 94
    ctx.set_read_filter(**SETTINGS)
    ctx.reset()
    with pytest.raises(DependencyError) as e:
        ctx.map_fastx(_write_fastq(tmp_path / "bad.fq", s["bases"], s["offs"], bad))
    assert e.value.code == EFORMAT
    # map_host carries no qualities: refused while a filter is set, and the context maps on afterwards
    ctx.reset()
    for call in (lambda: ctx.map_host(k["bases"], k["offs"]),):
        with pytest.raises(DependencyError) as e:
            call()
        assert e.value.code == EINVAL and "drprg_hip_set_read_filter" in str(e.value)
    assert ctx.counters()["reads"] == 0
    ctx.map_fastx(fq)
    _assert_oracle(ctx, k["want"], k["census"]["reads_kept"], k["census"]["bases_kept"], "after the refusals")
    # a reset clears the counts and keeps the settings
    assert _info_counts(ctx) == k["census"]
    ctx.reset()
    assert _info_counts(ctx) == {key: 0 for key in k["census"]} and ctx.read_filter_info()["T"] == rule.E[10]
    ctx.map_fastx(fq)
    assert _info_counts(ctx) == k["census"]
    # cleared: the old behaviour, every read, and map_host is served again
    ctx.set_read_filter()
    ctx.reset()
    ctx.map_host(k["bases"], k["offs"])
    _assert_oracle(ctx, k["want"], k["census"]["reads_kept"], k["census"]["bases_kept"], "map_host, no filter")
    ctx.reset()
    ctx.map_fastx(fq)
    cnt = ctx.counters()
    assert cnt["reads"] == len(s["lengths"]) and cnt["bases"] == sum(s["lengths"]) and _info_counts(ctx)["reads_seen"] == 0
    ctx.close()


# ---- 6. the executables ---------------------------------------------------------------------------------------------------------------------------
def test_pandora_map_writes_the_vcf_of_the_prefiltered_file(tmp_path, oracle):
    from drprg_amd._lib import PANDORA_EXE
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    ctx.close()
    k = s["all"]
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bam = _write_bam(tmp_path / "all.bam", s["bases"], s["offs"], s["quals"])
    kept_fq = _write_fastq(tmp_path / "kept.fq", k["bases"], k["offs"], k["quals"])

    def run(out, reads, extra):
        argv = [PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(G), "--max-covg", "4294967295"] + extra + [
            "--vcf-refs", genes, "-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout, open(out / "pandora_genotyped.vcf", "rb").read()

    flags = ["--min-read-len", str(rule.MIN_LEN), "--max-read-len", str(rule.MAX_LEN), "--min-read-qual", str(rule.MIN_QUAL)]
    stdout, got = run(tmp_path / "filtered", bam, flags)
    _, want = run(tmp_path / "kept", kept_fq, [])
    assert vcf_without_date(str(tmp_path / "filtered" / "pandora_genotyped.vcf")) == vcf_without_date(str(tmp_path / "kept" / "pandora_genotyped.vcf"))
    assert [l for l in got.splitlines() if not l.startswith(b"##fileDate")] == [l for l in want.splitlines() if not l.startswith(b"##fileDate")]
    c = k["census"]
    line = (f"read filter: reads_seen={c['reads_seen']} bases_seen={c['bases_seen']} dropped_short={c['dropped_short']} dropped_long={c['dropped_long']} "
            f"dropped_low_qual={c['dropped_low_qual']} reads_kept={c['reads_kept']} bases_kept={c['bases_kept']} (T={rule.E[10]})")
    assert line in stdout and f"reads={c['reads_kept']} " in stdout, stdout
    # a usage error exits with status 2 before anything is opened
    r = subprocess.run([PANDORA_EXE, "map", "--min-read-len", "9", "--max-read-len", "8", prg, bam], capture_output=True, text=True)
    assert r.returncode == 2 and "--max-read-len" in r.stderr


def test_drprg_predict_takes_the_same_flags(tmp_path):
    from drprg_amd import synth
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 6000, seed=1)
    n = len(offs) - 1
    quals = [np.full(150, 30 if i % 4 else 5, dtype=np.uint8) for i in range(n)]  # every fourth read is bad
    keep = [bool(i % 4) for i in range(n)]
    fq = _write_fastq(tmp_path / "wt.fq", bases, offs, quals)
    kb, ko, kq = _select(bases, offs, keep, quals)
    kept_fq = _write_fastq(tmp_path / "kept.fq", kb, ko, kq)

    def run(out, reads, extra):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", reads, "-o", str(out), "-s", "wt", "-I", "-v"] + extra
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        calls = json.load(open(out / "wt.drprg.json"))["susceptibility"]
        for drug in calls.values():
            for ev in drug["evidence"]:
                ev.pop("vcfid")  # (a fresh identifier per run)
        return r.stderr, (open(out / "pandora_genotyped.vcf").read(), calls)

    err, got = run(tmp_path / "filtered", fq, ["--min-read-len", "100", "--min-read-qual", "12.5"])
    _, want = run(tmp_path / "kept", kept_fq, [])
    assert got == want
    n_kept = sum(keep)
    assert f"read filter: reads_seen={n} bases_seen={150 * n} dropped_short=0 dropped_long=0 dropped_low_qual={n - n_kept} reads_kept={n_kept} bases_kept={150 * n_kept} (T=" in err, err
    assert f"] reads={n_kept} " in err
    r = subprocess.run([os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "--min-read-len", "5", "--max-read-len", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--max-read-len" in r.stderr
