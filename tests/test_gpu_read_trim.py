"""Read trimming (drprg_hip_set_read_trim, csrc/read_trim.hip; pytest -m gpu).  Kept ranges and counts come from the rule in plain Python
(tests/read_trim_rule.py), the vectors and counters from the oracle on the reads the rule leaves -- never from the code under test.

How the blocks come about: the ingest hands a worker's first block over at 750 000 bases, so the small sample (under that) is one block
and the big one several, whatever the number of parser threads."""
import json
import os
import subprocess

import numpy as np
import pytest

import bam_writer
import read_filter_rule as frule
import read_trim_rule as rule
from bam_writer import Rec
from max_covg_rule import accepted_reads
from read_trim_rule import kept_range, kept_range_stored, qual_milli
from subsample_rule import keep_flags
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from test_gpu_read_filter import _assert_oracle, _file_of, _write_bam, _write_fastq
from util import vcf_without_date

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
EINVAL, ENODATA, EFORMAT = 22, 61, 84
TILE = 16384  # bytes of the quality buffer per workgroup of trim_points_kernel
SETTINGS = dict(front=rule.FRONT_N, tail=rule.TAIL_N, qual=rule.QUAL)  # (window 0: the default of 4)
FLAGS = ["--trim-front", str(rule.FRONT_N), "--trim-tail", str(rule.TAIL_N), "--trim-qual", str(rule.QUAL)]
NO_TRIM = dict(reads_seen=0, bases_seen=0, reads_lost_base=0, cut_front=0, cut_tail=0, qual_cut_front=0, qual_cut_tail=0, reads_emptied=0)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _cut(bases, offs, ranges, quals=None):
    """the reads cut to their ranges: (bases, offsets[, qualities]); a read trimmed to nothing stays, as a read of no bases"""
    parts = [bases[int(offs[i]) + a:int(offs[i]) + b] for i, (a, b) in enumerate(ranges)]
    o = np.zeros(len(parts) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([p.size for p in parts])
    b = np.concatenate(parts) if o[-1] else np.zeros(0, np.uint8)
    return (b, o) if quals is None else (b, o, [quals[i][a:b] for i, (a, b) in enumerate(ranges)])


def _filter_counts(ctx):
    info = ctx.read_filter_info()
    info.pop("T")
    return info


_SAMPLES = {}


def _sample(which, oracle, ctx):
    """the sample's reads, the rule's ranges, and the oracle's vectors of the trimmed reads: made once, shared, left unchanged"""
    if which not in _SAMPLES:
        _, genomes = _panel()
        lengths, quals = rule.small_sample() if which == "small" else rule.big_sample()
        bases, offs = _reads_of(genomes, lengths, seed=41)
        bases = bases.copy()
        for i in range(0, len(lengths), 10):  # a base that is not ACGT in every tenth read, now in the cut part, now in the kept: packed blocks list positions
            if lengths[i] > 40:
                bases[int(offs[i]) + (2 if i % 20 else 40)] = ord("N")
        s = dict(lengths=lengths, quals=quals, bases=bases, offs=offs)
        idx = _oracle_index(oracle, ctx.prg_strings, W, K)
        for name, kw in (("all", SETTINGS), ("crop", dict(front=rule.FRONT_N, tail=rule.TAIL_N, qual=0))):
            ranges = rule.sample_ranges(lengths, quals, kw["front"], kw["tail"], kw["qual"], 0)
            tb, to, tq = _cut(bases, offs, ranges, quals)
            s[name] = dict(ranges=ranges, info=rule.info(lengths, ranges, kw["front"], kw["tail"]), bases=tb, offs=to, quals=tq, lengths=np.diff(to.astype(np.int64)).tolist(),
                           want=_oracle_map(oracle, idx, tb, to, W, K, True, threads=4))
        assert s["all"]["want"][2]["clusters_kept"] > 5
        _SAMPLES[which] = s
    return _SAMPLES[which]


def _assert_trimmed(ctx, s, k, what):
    n, nb = len(s["lengths"]), int(k["offs"][-1])
    _assert_oracle(ctx, k["want"], n, nb, what)
    assert ctx.read_trim_info() == k["info"], what
    assert _filter_counts(ctx) == dict(reads_seen=n, bases_seen=nb, dropped_short=0, dropped_long=0, dropped_low_qual=0, reads_kept=n, bases_kept=nb), what


# ---- 1. the kernels against the rule ----------------------------------------------------------------------------------------------------
def _device_trim(ctx, torch, Q, L, rev, bias, shift=0, flat=None):
    offs = np.zeros(len(L) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(L)
    n_reads, n_bases = len(L), int(offs[-1])
    buf = np.zeros(n_bases + 64 + 16, dtype=np.uint8)
    buf[shift:shift + n_bases] = (np.concatenate(Q).astype(np.int64) + bias).astype(np.uint8) if flat is None else flat
    d_q, d_o = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    d_r = torch.from_numpy(np.array(rev, dtype=np.uint8)).cuda()
    d_b = torch.full((n_reads,), -1, dtype=torch.int64, device="cuda")  # (stale on purpose)
    d_e = torch.full((n_reads,), -1, dtype=torch.int64, device="cuda")
    assert d_q.data_ptr() % 16 == 0
    out = ctx.read_trim_device(d_q.data_ptr() + shift, bias, d_o.data_ptr(), d_r.data_ptr(), n_reads, n_bases, d_b.data_ptr(), d_e.data_ptr())
    torch.cuda.synchronize()
    return out, list(zip(d_b.cpu().numpy().tolist(), d_e.cpu().numpy().tolist()))


@pytest.mark.parametrize("crops", [(0, 0), (5, 3)])
@pytest.mark.parametrize("window", [1, 4, 32])
@pytest.mark.parametrize("bias", [33, 0])
def test_the_kernels_equal_the_rule(tmp_path, bias, window, crops):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    L, Q, rev, milli = rule.kernel_batch(window)
    assert milli == 20500
    want = [kept_range_stored(q, l, v, crops[0], crops[1], milli, window) for q, l, v in zip(Q, L, rev)]
    kept, lost = sum(b - a for a, b in want), sum((b - a) != l for (a, b), l in zip(want, L))
    ctx.set_read_trim(front=crops[0], tail=crops[1], qual="20.5", window=window)
    for shift in (0, 1):  # 16-byte aligned, and one byte off (read byte by byte)
        out, got = _device_trim(ctx, torch, Q, L, rev, bias, shift)
        diff = [i for i in range(len(L)) if got[i] != want[i]]
        assert not diff, (shift, [(i, L[i], rev[i], got[i], want[i]) for i in diff[:8]])
        assert out == (kept, lost, 0), (shift, out)
    if window == 4:  # a window given as 0 is 4
        ctx.set_read_trim(front=crops[0], tail=crops[1], qual="20.5")
        assert _device_trim(ctx, torch, Q, L, rev, bias)[1] == want
        ctx.set_read_trim(front=crops[0], tail=crops[1], qual="20.5", window=window)
    # a second launch on the same context with a smaller batch: nothing of the first one is left behind
    Q2 = [np.array(x, dtype=np.uint8) for x in ([], [30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30], [], [5] * 9, [])]
    L2, rev2 = [q.size for q in Q2], [0, 1, 0, 0, 1]
    out, got = _device_trim(ctx, torch, Q2, L2, rev2, bias)
    assert got == [kept_range_stored(q, l, v, crops[0], crops[1], milli, window) for q, l, v in zip(Q2, L2, rev2)]
    # the fixed crops alone: no quality buffer is needed
    ctx.set_read_trim(front=7, tail=2)
    offs = np.zeros(len(L) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(L)
    d_o = torch.from_numpy(offs).cuda()
    d_b, d_e = torch.zeros(len(L), dtype=torch.int64, device="cuda"), torch.zeros(len(L), dtype=torch.int64, device="cuda")
    out = ctx.read_trim_device(None, bias, d_o.data_ptr(), None, len(L), int(offs[-1]), d_b.data_ptr(), d_e.data_ptr())
    crop = [kept_range(None, l, 7, 2) for l in L]
    assert list(zip(d_b.cpu().numpy().tolist(), d_e.cpu().numpy().tolist())) == crop and out[0] == sum(b - a for a, b in crop)
    # one byte out of range: -84, and the position is named
    ctx.set_read_trim(qual="20.5", window=window)
    flat = (np.concatenate(Q).astype(np.int64) + bias)
    for at, value in ((TILE + 5, bias + 94), (77, 255 if bias == 0 else 32)):
        bad = flat.copy()
        bad[at] = value
        with pytest.raises(DependencyError) as e:
            _device_trim(ctx, torch, Q, L, rev, bias, 0, bad.astype(np.uint8))
        assert e.value.code == EFORMAT and str(at) in str(e.value) and ctx.last_trim_out[2] == at + 1, (at, e.value)
    ctx.close()


# ---- 2. a trimmed sample equals the sample of its trimmed reads ---------------------------------------------------------------------------
FORMS = ["fastq ascii", "fastq packed", "bam", "fastq.gz"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["small", "big"])
def test_a_trimmed_sample_equals_the_sample_of_its_trimmed_reads(tmp_path, oracle, which, form):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample(which, oracle, ctx)
    k = s["all"]
    path = _file_of(tmp_path, form, s["bases"], s["offs"], s["quals"], "all")
    for packed in ((True,) if form == "fastq packed" else (False,) if form == "fastq ascii" else (False, True)):
        ctx.reset()
        ctx.set_threads(1 if which == "small" else 4)
        ctx.set_input_format(packed)
        ctx.keep_reads(1 << 28)
        ctx.set_read_trim(**SETTINGS)
        ctx.map_fastx(path)
        _assert_trimmed(ctx, s, k, (which, form, packed))
        info = ctx.resident_info()
        assert info["complete"] and (info["blocks"] == 1 if which == "small" else info["blocks"] >= 2), info
        if which == "small" and (packed or form == "bam"):  # what stays resident is the trimmed block
            nb = int(k["offs"][-1])
            assert (nb + 15) // 16 * 4 <= info["bytes"] < nb
    ctx.close()


# ---- 3. packed blocks with N positions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fastq packed", "bam"])
def test_listed_positions_move_with_the_kept_range(tmp_path, oracle, form):
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    n, L = 600, 120
    bases, offs = _reads_of(genomes, [L] * n, seed=47)
    bases = bases.copy()
    q = np.full(L, 35, dtype=np.uint8)
    q[:10], q[-12:] = 4, 6  # kept: [10, 108)
    quals = [q.copy() for _ in range(n)]
    assert kept_range(q, L, 0, 0, 20000, 4) == (10, 108)
    for i in range(n):  # Ns in the cut front, on both edges of the kept range, inside it and in the cut tail -- and reads without any
        for p in ((2,), (9, 10), (10, 60), (107, 108), (107,), (115,), (), (0, 10, 11, 59, 107, 119))[i % 8]:
            bases[int(offs[i]) + p] = ord("N")
    ranges = [(10, 108)] * n
    tb, to = _cut(bases, offs, ranges)
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), tb, to, W, K, True, threads=4)
    assert want[2]["clusters_kept"] > 5
    ctx.set_threads(2)
    ctx.set_input_format(True)
    ctx.set_read_trim(qual=20)
    for keep in (0, 1 << 28):
        ctx.reset()
        ctx.keep_reads(keep)
        ctx.map_fastx(_file_of(tmp_path, form, bases, offs, quals, "n"))
        _assert_oracle(ctx, want, n, 98 * n, (form, keep))
        assert ctx.read_trim_info() == rule.info([L] * n, ranges)
    ctx.close()


# ---- 4. everything behind it sees trimmed reads -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_the_read_filter_sees_trimmed_reads(tmp_path, oracle, packed):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, ctx)
    k = s["all"]
    MIN_LEN, MIN_QUAL = 160, 20
    T = frule.threshold(qual_milli(MIN_QUAL))
    before = frule.fates(s["lengths"], s["quals"], MIN_LEN, 0, T)
    after = frule.fates(k["lengths"], k["quals"], MIN_LEN, 0, T)
    # a read that passes the mean quality only once its tail is gone is kept; one that falls under the length bound only after trimming is dropped
    assert sum(b == frule.LOWQ and a == frule.KEEP for b, a in zip(before, after)) >= 3
    assert sum(b == frule.KEEP and a == frule.SHORT for b, a in zip(before, after)) >= 3
    keep = [a == frule.KEEP for a in after]
    idx = [i for i, x in enumerate(keep) if x]
    parts = [k["bases"][int(k["offs"][i]):int(k["offs"][i + 1])] for i in idx]
    ko = np.zeros(len(idx) + 1, dtype=np.uint64)
    ko[1:] = np.cumsum([p.size for p in parts])
    kb = np.concatenate(parts)
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    ctx.set_threads(4)
    ctx.set_input_format(packed)
    ctx.keep_reads(1 << 28)
    ctx.set_read_trim(**SETTINGS)
    ctx.set_read_filter(min_len=MIN_LEN, min_qual=MIN_QUAL)
    ctx.map_fastx(_write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"]))
    _assert_oracle(ctx, want, len(idx), int(ko[-1]), "trim + filter")
    assert ctx.read_trim_info() == k["info"]
    assert _filter_counts(ctx) == frule.census((after, k["lengths"]))  # trimmed reads and bases are what the filter has "seen"
    assert ctx.resident_info()["complete"]
    ctx.close()


def test_the_depth_cap_and_the_subsample_count_trimmed_bases(tmp_path, oracle):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, ctx)
    k = s["all"]
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    ctx.set_threads(4)
    ctx.keep_reads(1 << 28)
    ctx.set_read_trim(**SETTINGS)
    # the cap cuts on the trimmed reads' running total: in the first block, and in a later one (the first holds 786 432 untrimmed bases)
    for max_covg, packed in ((3, True), (99, False), (99, True)):
        n, n_bases, reached = accepted_reads(k["lengths"], G, max_covg)
        assert reached and 0 < n < len(k["lengths"]) and (max_covg == 3 or n_bases > 800_000)
        want = _oracle_map(oracle, idx, k["bases"][:n_bases], k["offs"][:n + 1], W, K, True, threads=4)
        ctx.reset()
        ctx.set_input_format(packed)
        ctx.set_max_covg(max_covg)
        ctx.map_fastx(fq)
        info = ctx.max_covg_info()
        assert info["reached"] and info["reads"] == n and info["bases"] == n_bases, (max_covg, info)
        _assert_oracle(ctx, want, n, n_bases, ("cap", max_covg, packed))
        assert ctx.resident_info()["complete"]
    ctx.set_max_covg(None)
    # the subsample numbers the trimmed reads and aims at their bases
    ctx.reset()
    ctx.set_ordered_ingest(True)
    ctx.map_fastx(fq)
    total = int(k["offs"][-1])
    T = total // 2
    flags = keep_flags(k["lengths"], T, 9)
    out = ctx.subsample(T, 9)
    assert out["reads_before"] == len(k["lengths"]) and out["bases_before"] == total and out["reads_kept"] == sum(flags)
    assert ctx.subsample_flags(len(flags)).tolist() == flags
    ctx.close()


def test_dedup_sees_trimmed_reads(tmp_path, oracle):
    """two reads that are identical once their junk tails are gone, and different before: one is dropped"""
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    n, L = 150, 200
    half, offs1 = _reads_of(genomes, [L] * n, seed=53)
    bases = np.concatenate([half, half]).copy()
    offs = np.arange(2 * n + 1, dtype=np.uint64) * L
    for i in range(n):  # the copy's last 20 bases are other letters
        tail = bases[int(offs[n + i]) + L - 20:int(offs[n + i + 1])]
        tail[:] = np.frombuffer(bytes(tail).translate(bytes.maketrans(b"ACGT", b"CATG")), dtype=np.uint8)
    q = np.full(L, 30, dtype=np.uint8)
    q[-20:] = 5
    assert kept_range(q, L, 0, 0, 20000, 4) == (0, 180)
    fq = _write_fastq(tmp_path / "dup.fq", bases, offs, [q] * (2 * n))
    from dedup_rule import keep_flags_fast
    reads = [bases[int(offs[i]):int(offs[i + 1])] for i in range(2 * n)]
    n_before = sum(keep_flags_fast(reads))  # untrimmed: a read and its copy differ
    flags = keep_flags_fast([r[:180] for r in reads])
    n_after = sum(flags)
    assert n_before >= 2 * n - 30 and n_after == n_before - n and not any(flags[n:])
    kept = [i for i, f in enumerate(flags) if f]
    tb, to = np.concatenate([reads[i][:180] for i in kept]), np.arange(len(kept) + 1, dtype=np.uint64) * 180
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), tb, to, W, K, True)
    ctx.set_threads(1)
    ctx.set_ordered_ingest(True)
    ctx.keep_reads(1 << 28)
    for packed in (True, False):
        ctx.set_input_format(packed)
        ctx.reset()
        ctx.set_read_trim()
        ctx.map_fastx(fq)
        assert ctx.dedup()["reads_kept"] == n_before
        ctx.reset()
        ctx.set_read_trim(qual=20)
        ctx.map_fastx(fq)
        assert ctx.resident_info()["complete"]
        out = ctx.dedup()
        assert out == dict(reads_before=2 * n, bases_before=360 * n, reads_kept=n_after, bases_kept=180 * n_after), out
        _assert_oracle(ctx, want, n_after, 180 * n_after, ("dedup", packed))
    ctx.close()


# ---- 5. a middle block whose every read is trimmed to nothing ----------------------------------------------------------------------------------
def test_a_middle_block_that_is_trimmed_to_nothing(tmp_path, oracle):
    """three blocks of one file, the middle one of reads without a good window: the block that maps nothing must not hand the staging set of
    the block before it -- whose kernels may still be running -- to the block after it.  The ingest hands the first block over at 786 432
    bases and the next at 12 582 912: the reads are sized to fill them exactly."""
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    lengths = [384] * 2048 + [8192] * 1536 + [384] * 512
    bases, offs = _reads_of(genomes, lengths, seed=43)
    fq = str(tmp_path / "three.fq")
    with open(fq, "wb") as fh:
        for i, L in enumerate(lengths):
            fh.write(b"@r%d\n" % i + bases[int(offs[i]):int(offs[i + 1])].tobytes() + b"\n+\n" + (b"I" if L == 384 else b"&") * L + b"\n")
    ranges = [(0, L) if L == 384 else (0, 0) for L in lengths]
    kb, ko = _cut(bases, offs, ranges)
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    ctx.set_threads(4)
    ctx.set_read_trim(qual=20)
    for packed in (True, False):
        for keep_bytes in (0, 1 << 28):
            ctx.reset()
            ctx.set_input_format(packed)
            ctx.keep_reads(keep_bytes)
            ctx.map_fastx(fq)
            _assert_oracle(ctx, want, len(lengths), 2560 * 384, (packed, keep_bytes))  # (the emptied reads stay reads)
            assert ctx.read_trim_info() == rule.info(lengths, ranges)
            if keep_bytes:  # the three blocks were there: two of them left something to keep
                assert ctx.resident_info()["complete"] and ctx.resident_info()["blocks"] == 2
    ctx.close()


# ---- 6. fixed crops alone -----------------------------------------------------------------------------------------------------------------------
def test_fixed_crops_alone_serve_inputs_without_qualities(tmp_path, oracle):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    k = s["crop"]
    n = len(s["lengths"])
    fa = str(tmp_path / "all.fa")
    with open(fa, "wb") as fh:
        for i in range(n):
            fh.write(b">r%d\n" % i + s["bases"][int(s["offs"][i]):int(s["offs"][i + 1])].tobytes() + b"\n")
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    recs = []
    for i in range(n):  # every third record on the reverse strand, none with qualities
        t = s["bases"][int(s["offs"][i]):int(s["offs"][i + 1])].tobytes()
        recs.append(Rec(t.translate(comp)[::-1].decode(), flag=0x10, name=b"r%d" % i) if rule.reverse_flag(i) else Rec(t.decode(), flag=4, name=b"r%d" % i))
    noq = str(bam_writer.write(tmp_path / "noq.bam", recs))
    ctx.set_threads(2)
    ctx.set_read_trim(front=rule.FRONT_N, tail=rule.TAIL_N)
    for path in (fa, noq):
        for packed in (False, True):
            ctx.reset()
            ctx.set_input_format(packed)
            ctx.map_fastx(path)
            _assert_trimmed(ctx, s, k, (path, packed))
    ctx.close()


# ---- 7. refusals and state ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(tmp_path, oracle):
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    k = s["all"]
    n = len(s["lengths"])
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    fa = str(tmp_path / "all.fa")
    with open(fa, "wb") as fh:
        for i in range(n):
            fh.write(b">r%d\n" % i + s["bases"][int(s["offs"][i]):int(s["offs"][i + 1])].tobytes() + b"\n")
    noq = str(bam_writer.write(tmp_path / "noq.bam", [Rec(s["bases"][int(s["offs"][i]):int(s["offs"][i + 1])].tobytes().decode(), flag=4, name=b"r%d" % i)
                                                      for i in range(n)]))
    ctx.set_threads(2)
    # nothing set: the vectors of the untrimmed sample, and no count
    full = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), s["bases"], s["offs"], W, K, True, threads=4)
    ctx.map_fastx(fq)
    _assert_oracle(ctx, full, n, sum(s["lengths"]), "nothing set")
    assert ctx.read_trim_info() == NO_TRIM and _filter_counts(ctx)["reads_seen"] == 0
    # bad settings
    for bad in (dict(qual="93.001"), dict(qual=20, window=33), dict(window=4), dict(front=3, window=1)):
        with pytest.raises(DependencyError) as e:
            ctx.set_read_trim(**bad)
        assert e.value.code == EINVAL, bad
    # no qualities under --trim-qual: refused, and the text names the flag
    ctx.set_read_trim(**SETTINGS)
    for path in (fa, noq):
        ctx.reset()
        with pytest.raises(DependencyError) as e:
            ctx.map_fastx(path)
        assert e.value.code == EINVAL and "--trim-qual" in str(e.value), (path, e.value)
    # a quality byte out of range: -84
    bad = [q.copy() for q in s["quals"]]
    bad[n // 2][3] = 94
    ctx.reset()
    with pytest.raises(DependencyError) as e:
        ctx.map_fastx(_write_fastq(tmp_path / "bad.fq", s["bases"], s["offs"], bad))
    assert e.value.code == EFORMAT
    # map_host and map_device carry no qualities: refused while a trim setting is non-zero, and the context maps on afterwards
    ctx.reset()
    import torch
    d_b, d_o = torch.from_numpy(k["bases"]).cuda(), torch.from_numpy(k["offs"].astype(np.int64)).cuda()
    for call in (lambda: ctx.map_host(k["bases"], k["offs"]), lambda: ctx.map_device(d_b.data_ptr(), d_o.data_ptr(), n, int(k["offs"][-1]))):
        with pytest.raises(DependencyError) as e:
            call()
        assert e.value.code == EINVAL and "drprg_hip_set_read_trim" in str(e.value)
    assert ctx.counters()["reads"] == 0
    ctx.map_fastx(fq)
    _assert_trimmed(ctx, s, k, "after the refusals")
    # discover without resident reads after a trimmed block: -61
    (tmp_path / "disc").mkdir()
    with pytest.raises(DependencyError) as e:
        ctx.discover_reads(fq, str(tmp_path / "genes.fa"), str(tmp_path / "disc"))
    assert e.value.code == ENODATA
    # a reset clears the counts and keeps the settings
    ctx.reset()
    assert ctx.read_trim_info() == NO_TRIM
    ctx.map_fastx(fq)
    _assert_trimmed(ctx, s, k, "after a reset")
    # cleared: today's path, every base, and map_host is served again
    ctx.set_read_trim()
    ctx.reset()
    ctx.map_host(k["bases"], k["offs"])
    _assert_oracle(ctx, k["want"], n, int(k["offs"][-1]), "map_host, nothing set")
    ctx.reset()
    ctx.map_fastx(fq)
    _assert_oracle(ctx, full, n, sum(s["lengths"]), "cleared")
    assert ctx.read_trim_info() == NO_TRIM and _filter_counts(ctx)["reads_seen"] == 0
    ctx.close()


# ---- 8. / 9. the executables ---------------------------------------------------------------------------------------------------------------------
def test_pandora_map_writes_the_vcf_of_the_pretrimmed_file(tmp_path, oracle):
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
    cut_fq = _write_fastq(tmp_path / "cut.fq", k["bases"], k["offs"], k["quals"])

    def run(out, reads, extra):
        argv = [PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(G), "--max-covg", "4294967295"] + extra + [
            "--vcf-refs", genes, "-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout, open(out / "pandora_genotyped.vcf", "rb").read()

    stdout, got = run(tmp_path / "trimmed", bam, FLAGS)
    _, want = run(tmp_path / "cut", cut_fq, [])
    assert vcf_without_date(str(tmp_path / "trimmed" / "pandora_genotyped.vcf")) == vcf_without_date(str(tmp_path / "cut" / "pandora_genotyped.vcf"))
    assert [l for l in got.splitlines() if not l.startswith(b"##fileDate")] == [l for l in want.splitlines() if not l.startswith(b"##fileDate")]
    c = k["info"]
    line = "read trimming: " + " ".join(f"{key}={c[key]}" for key in ("reads_seen", "bases_seen", "reads_lost_base", "cut_front", "cut_tail", "qual_cut_front",
                                                                       "qual_cut_tail", "reads_emptied"))
    assert line in stdout and f"reads={c['reads_seen']} bases={int(k['offs'][-1])} " in stdout, stdout
    r = subprocess.run([PANDORA_EXE, "map", "--trim-window", "4", prg, bam], capture_output=True, text=True)
    assert r.returncode == 2 and "--trim-window" in r.stderr


def test_drprg_predict_takes_the_same_flags(tmp_path):
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 6000, seed=1)
    n = len(offs) - 1
    quals = []
    for i in range(n):  # every fourth read has a junk tail, every eighth a junk start as well
        q = np.full(150, 30, dtype=np.uint8)
        if i % 4 == 0:
            q[-25:] = 4
        if i % 8 == 0:
            q[:12] = 7
        quals.append(q)
    ranges = [kept_range(q, 150, 2, 0, 12500, 4) for q in quals]
    assert {(2, 150), (2, 125), (12, 125)} == set(ranges)
    fq = _write_fastq(tmp_path / "wt.fq", bases, offs, quals)
    cb, co, cq = _cut(bases, offs, ranges, quals)
    cut_fq = _write_fastq(tmp_path / "cut.fq", cb, co, cq)

    def run(out, reads, extra):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", reads, "-o", str(out), "-s", "wt", "-I", "-v"] + extra
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        calls = json.load(open(out / "wt.drprg.json"))["susceptibility"]
        for drug in calls.values():
            for ev in drug["evidence"]:
                ev.pop("vcfid")  # (a fresh identifier per run)
        return r.stderr, (open(out / "pandora_genotyped.vcf").read(), calls)

    err, got = run(tmp_path / "trimmed", fq, ["--trim-front", "2", "--trim-qual", "12.5", "--trim-window", "4"])
    _, want = run(tmp_path / "cut", cut_fq, [])
    assert got == want
    c = rule.info([150] * n, ranges, 2, 0)
    assert "read trimming: " + " ".join(f"{key}={c[key]}" for key in c) in err, err
    assert f"] reads={n} " in err
    r = subprocess.run([os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "--trim-window", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--trim-window" in r.stderr
    r = subprocess.run([os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "--trim-qual", "94"], capture_output=True, text=True)
    assert r.returncode == 2 and "--trim-qual" in r.stderr


# ---- 10. two devices --------------------------------------------------------------------------------------------------------------------------------
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
        c.set_read_trim(**SETTINGS)
        c.map_fastx(fq)
        _assert_trimmed(c, s, k, "devices")
    one.close()
    multi.close()
