"""Read statistics (drprg_hip_set_read_stats, csrc/read_stats.hip; pytest -m gpu).  Every expected word comes from the rule in plain Python
(tests/read_stats_rule.py), for the prepared snapshot applied to the reads the other plain-Python rules leave, composed in the documented
order -- never from the code under test.  Every count is compared for equality.

How the blocks come about: the ingest hands a worker's first block over at 750 000 bases, so the sample (under that) is one block whatever
the number of parser threads, and a depth cap below its kept bases is reached in the middle of that block."""
import json
import subprocess

import numpy as np
import pytest

import adapter_rule
import decoy_rule
import mask_qual_rule
import max_covg_rule
import polyx_rule
import read_filter_rule
import read_stats_rule as rule
import read_trim_rule
from bam_writer import Rec, write as write_bam
from test_gpu_decoy import _fasta, _fasta_reads, _flat
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx
from test_gpu_polyx import ADAPTER, _Bases
from test_gpu_read_filter import _write_fastq

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
EINVAL, EFORMAT = 22, 84
TILE = 16384
COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
NOVASEQ = np.array([2, 12, 23, 37])
INFOS = ("read_filter_info", "read_trim_info", "adapter_trim_info", "front_adapter_info", "poly_trim_info", "base_mask_info", "complexity_info", "decoy_info",
         "max_covg_info", "bam_info", "resident_info")
SECTIONS = ("len_reads", "len_bases", "cyc_base", "cyc_qsum", "qual_hist", "readq_hist", "gc_hist")


def _same(got, want, what):
    """a snapshot of the library (Context.read_stats_dict) against the rule's words, with the first words that differ named"""
    w = got["words"][:want.size]
    if np.array_equal(w, want):
        return
    lay = rule.layout()
    bad = np.flatnonzero(w != want)
    where = [(max((k for k in SECTIONS if lay[k] <= i), key=lambda k: lay[k], default="totals"), int(i), int(w[i]), int(want[i])) for i in bad[:8]]
    raise AssertionError((what, len(bad), [(s, i - (lay[s] if s != "totals" else 0), g, x) for s, i, g, x in where]))


# ---- 1. the kernels against the rule, on device buffers ---------------------------------------------------------------------------------
_BATCH = {}


def _kernel_batch():
    """reads, their qualities in read orientation, and which of them are stored mirrored: every length class and letter class of the issue"""
    if _BATCH:
        return _BATCH
    rng = np.random.default_rng(91)

    def dna(n, letters=b"ACGT"):
        return bytes(rng.choice(np.frombuffer(letters, np.uint8), size=n).tolist())

    lengths = [0, 1, 0, 150, 1, 15, 16, 17]
    lengths += [TILE - sum(lengths) - 1, 1, 1, 31, 32, 33]  # a read that ends one base in front of the first tile's end, one on it, one behind
    lengths += [511, 512, 513, 1023, 1024, 1025]
    lengths += [150] * 40 + [70_000] + [151] * 40  # one long read among short ones: it spans four tiles
    lengths += [65535, 65536, 65537, 0, 0, 7]
    lengths += [int(x) for x in rng.integers(0, 300, size=300)]
    lengths += [int(x) for x in rng.integers(0, 4, size=1500)]  # thousands of reads under one tile: a lane walks dozens of them
    at = sum(lengths)
    lengths += [(-at) % TILE, TILE, 16, 1]  # a read that ends on a tile boundary, a read that is one tile, two short ones behind them
    reads = [dna(n) for n in lengths]
    reads[3] = reads[3].lower()
    reads[15] = dna(512, b"ACGTNacgtnRYKMSWBDHV")
    reads[16] = b"N" * 513
    reads[21] = dna(150, b"NRYKM")  # a read of U only
    reads[22] = dna(150, b"GCgc")
    reads[23] = dna(150, b"ATat")
    reads[60] = dna(70_000, b"ACGTN")
    quals = []
    for i, r in enumerate(reads):
        if i % 7 == 0:
            q = rng.integers(0, 94, size=len(r))
        elif i % 7 == 1:
            q = np.full(len(r), 93 if i % 2 else 0)
        else:
            q = rng.choice(NOVASEQ, size=len(r), p=[0.02, 0.05, 0.13, 0.8])  # the contended case: four values
        if len(r) > 40:  # asymmetric: a mirrored read of the wrong orientation gives other per-cycle sums
            q[:20] = 2
            q[-20:] = 40
        quals.append(q.astype(np.uint8))
    rev = np.array([i % 3 == 0 for i in range(len(reads))])
    _BATCH.update(reads=reads, quals=quals, rev=rev)
    return _BATCH


def _stored(quals, rev=None):
    """the quality bytes as the device buffer holds them: every read's in stored order (mirrored where rev), with 64 bytes of padding"""
    parts = [q[::-1] if rev is not None and rev[i] else q for i, q in enumerate(quals)]
    flat = np.concatenate(parts).astype(np.uint8) if parts and sum(p.size for p in parts) else np.zeros(0, np.uint8)
    return np.concatenate([flat, np.full(64, 0x5A, np.uint8)])


_WANT = {}


def _want(key, make):
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


@pytest.mark.parametrize("form", ["text", "packed"])
def test_the_kernels_equal_the_rule(tmp_path, form):
    import torch
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    lay = rule.layout()
    kb = _kernel_batch()
    reads, quals, rev = kb["reads"], kb["quals"], kb["rev"]
    n = len(reads)

    def run(rs, qs, bias=0, mirrored=None, flags=None, take=None, shifted=False):
        b = _Bases(torch, rs, form, shifted)
        d_q = torch.from_numpy(_stored(qs, mirrored) + np.uint8(bias)).cuda() if qs is not None else None
        d_r = torch.from_numpy(mirrored.astype(np.uint8)).cuda() if mirrored is not None else None
        d_f = torch.from_numpy(np.asarray(flags, dtype=np.uint8)).cuda() if flags is not None else None
        try:
            got = ctx.read_stats_device(b.d_text, b.d_words, b.d_npos, b.n_npos, d_q.data_ptr() if qs is not None else None, bias, b.d_o.data_ptr(),
                                        d_r.data_ptr() if d_r is not None else None, len(rs), b.n_bases, d_f.data_ptr() if d_f is not None else None, take)
        finally:
            torch.cuda.synchronize()
        assert b.untouched(), "the bases were written"
        return got

    # no reads: a snapshot of zeros, no pointer looked at
    got = ctx.read_stats_device(None, None, None, 0, None, 0, None, None, 0, 0)
    assert not got["words"].any()
    # every length and letter class, qualities 0, 93 and the four-value set; FASTQ bias and BAM bias give the same words
    want = _want("all", lambda: rule.snapshot(reads, quals, lay))
    _same(run(reads, quals), want, "ragged")
    _same(run(reads, quals, bias=33), want, "ragged, bias 33")
    assert want[0] == n and want[3] == 70_000 and want[2] == 0
    # reverse-strand records: the quality bytes are stored mirrored, the words are those of the read orientation
    _same(run(reads, quals, mirrored=rev), want, "mirrored")
    assert not np.array_equal(rule.snapshot(reads, [q[::-1] if rev[i] else q for i, q in enumerate(quals)], lay), want), "the qualities are symmetric: nothing is tested"
    # every second read dropped and a bound inside the block
    flags = [i % 2 for i in range(n)]
    take = n - 37
    picked = [i for i in range(take) if flags[i]]
    want_f = _want("flags", lambda: rule.snapshot([reads[i] for i in picked], [quals[i] for i in picked], lay))
    _same(run(reads, quals, mirrored=rev, flags=flags, take=take), want_f, "flags and take")
    want_t = _want("take", lambda: rule.snapshot(reads[:61], quals[:61], lay))
    _same(run(reads, quals, take=61), want_t, "take alone: the long read is the last one counted")
    # without qualities: a null pointer, the three quality sections stay zero
    want_n = _want("noqual", lambda: rule.snapshot(reads, None, lay))
    got = run(reads, None)
    _same(got, want_n, "no qualities")
    assert not got["qual_hist"].any() and not got["readq_hist"].any() and not got["cyc_qsum"].any() and got["gc_hist"].sum() > 0
    # a second, small launch on the same context: nothing of the first one is left; reads of 0 and 1 base only; an unaligned text buffer
    small = [b"", b"A", b"", b"n", b"", b""]
    sq = [np.zeros(0, np.uint8), np.array([93], np.uint8), np.zeros(0, np.uint8), np.array([0], np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint8)]
    _same(run(small, sq), rule.snapshot(small, sq, lay), "reads of 0 and 1 base")
    _same(run([b"", b""], None), rule.snapshot([b"", b""], None, lay), "empty reads only")
    some = reads[:14] + reads[14:40]
    _same(run(some, quals[:40], shifted=True), _want("some", lambda: rule.snapshot(some, quals[:40], lay)), "one byte off the alignment")
    ctx.close()


def test_refusals(tmp_path):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    n_words = rule.layout()["words"]
    d_t = torch.from_numpy(np.full(264, 71, np.uint8)).cuda()
    d_o = torch.from_numpy(np.asarray([0, 50, 200], dtype=np.int64)).cuda()
    # a quality byte out of range: BAM byte 94, FASTQ byte 32 -- the byte is named
    for bias, byte, at in ((0, 94, 123), (33, 32, 7), (33, 127, 199), (0, 255, 0)):
        q = np.full(264, 30 + bias, np.uint8)
        q[at] = byte
        d_q = torch.from_numpy(q).cuda()
        with pytest.raises(DependencyError) as e:
            ctx.read_stats_device(d_t.data_ptr(), None, None, 0, d_q.data_ptr(), bias, d_o.data_ptr(), None, 2, 200)
        torch.cuda.synchronize()
        assert e.value.code == EFORMAT and f"quality byte {at}" in str(e.value), (bias, byte, str(e.value))
    d_q = torch.from_numpy(np.full(264, 30, np.uint8)).cuda()
    assert ctx.read_stats_device(d_t.data_ptr(), None, None, 0, d_q.data_ptr(), 0, d_o.data_ptr(), None, 2, 200)["bases"] == 200
    # offsets that do not ascend to n_bases
    for offs in ([0, 50, 199], [0, 50, 201], [1, 50, 200], [0, 201, 200], [0, 250, 200]):
        d_bad = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
        with pytest.raises(DependencyError) as e:
            ctx.read_stats_device(d_t.data_ptr(), None, None, 0, d_q.data_ptr(), 0, d_bad.data_ptr(), None, 2, 200)
        torch.cuda.synchronize()
        assert e.value.code == EINVAL, offs
    # a buffer that is too small, on both entries; a mode that does not exist; a quality bias that does not exist
    for call in (lambda: ctx.read_stats_device(d_t.data_ptr(), None, None, 0, None, 0, d_o.data_ptr(), None, 2, 200, n_words=n_words - 1),
                 lambda: ctx.read_stats_info(0, n_words=n_words - 1), lambda: ctx.read_stats_info(1, n_words=0), lambda: ctx.read_stats_info(2),
                 lambda: ctx.set_read_stats(3), lambda: ctx.set_read_stats(-1),
                 lambda: ctx.read_stats_device(d_t.data_ptr(), None, None, 0, d_q.data_ptr(), 64, d_o.data_ptr(), None, 2, 200)):
        with pytest.raises(DependencyError) as e:
            call()
        assert e.value.code == EINVAL
    # mode 1 needs qualities: FASTA names --qc-json, or the other quality setting first; mode 2 serves it
    bases, offs = _reads_of(genomes, [150] * 200, seed=3)
    reads = [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(200)]
    fa = _fasta_reads(tmp_path / "reads.fa", reads)
    ctx.set_read_stats(1)
    with pytest.raises(DependencyError) as e:
        ctx.map_fastx(fa)
    assert e.value.code == EINVAL and "--qc-json" in str(e.value), str(e.value)
    ctx.set_base_mask(10)
    ctx.reset()
    with pytest.raises(DependencyError) as e:
        ctx.map_fastx(fa)
    assert e.value.code == EINVAL and "--mask-qual" in str(e.value) and "--qc-json" not in str(e.value), str(e.value)
    ctx.set_base_mask(0)
    ctx.set_read_stats(2)
    ctx.reset()
    ctx.map_fastx(fa)
    _same(ctx.read_stats_info(0), rule.snapshot(reads, None), "FASTA without qualities")
    # a bad quality byte in a file fails the run, with the statistics alone and behind a prep setting
    quals = [np.full(150, 30, np.uint8) for _ in reads]
    quals[77][5] = 94
    fq = _write_fastq(tmp_path / "bad.fq", bases, offs, quals)
    for prep in (False, True):
        ctx.set_read_stats(1)
        ctx.set_read_filter(min_len=10 if prep else 0)
        ctx.reset()
        with pytest.raises(DependencyError) as e:
            ctx.map_fastx(fq)
        assert e.value.code == EFORMAT and "outside 0..93" in str(e.value), (prep, str(e.value))
    ctx.set_read_filter()
    # the host and device entries carry no qualities: refused under mode 1, served and not counted under mode 2
    d_b, d_o2 = torch.from_numpy(bases.copy()).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
    calls = (lambda: ctx.map_host(bases, offs), lambda: ctx.map_device(d_b.data_ptr(), d_o2.data_ptr(), 200, int(offs[-1])))
    ctx.reset()
    for call in calls:
        with pytest.raises(DependencyError) as e:
            call()
        assert e.value.code == EINVAL and "drprg_hip_set_read_stats" in str(e.value), str(e.value)
    assert ctx.counters()["reads"] == 0
    ctx.set_read_stats(2)
    for call in calls:
        call()
        torch.cuda.synchronize()
    assert ctx.counters()["reads"] == 400 and ctx.read_stats_info(0)["reads"] == 0
    ctx.close()


# ---- 2. the whole path ----------------------------------------------------------------------------------------------------------------------
_SAMPLE = {}
FRONT, TAIL, TRIM_Q, WINDOW, MASK_Q, MIN_LEN, MAX_LEN, MIN_Q, DK = 2, 3, 15, 4, 10, 40, 1000, 15, 31
M, P = polyx_rule.M, polyx_rule.P


def _sample():
    """the sample (reads and qualities in read orientation), a decoy, and the reads every prep stage together leaves: made once, left unchanged"""
    if _SAMPLE:
        return _SAMPLE
    _, genomes = _panel()
    rng = np.random.default_rng(92)
    n = 2400
    lengths = [150] * n
    for i in range(3, n, 50):
        lengths[i] = int(rng.integers(0, 9))
    for i in range(17, n, 120):
        lengths[i] = 300
    lengths[1000], lengths[1500] = 1500, 2000
    bases, offs = _reads_of(genomes, lengths, seed=93)
    data = bases.tobytes()
    reads, kinds = polyx_rule.tailed_sample([data[int(offs[i]):int(offs[i + 1])] for i in range(n)], seed=94)
    decoy = decoy_rule.random_dna(np.random.default_rng(95), 6000)
    for j in range(30):
        reads[40 * j + 9] = decoy[150 * j:150 * j + 150]
    for i in range(0, n, 10):
        if len(reads[i]) > 40:
            r = bytearray(reads[i])
            r[5] = ord("N")
            reads[i] = bytes(r) if i % 20 else bytes(r).lower()
    for i in range(7, n, 22):  # read-through: the adapter, then G to the read's end
        if kinds[i] == "plain" and len(reads[i]) == 150:
            at = int(rng.integers(60, 110))
            reads[i] = (reads[i][:at] + ADAPTER.encode() + b"G" * 150)[:150]
    quals = []
    for i, r in enumerate(reads):
        q = rng.choice(NOVASEQ, size=len(r), p=[0.01, 0.03, 0.11, 0.85]).astype(np.uint8)
        if len(r) == 150 and i % 13 == 5:
            q[-25:] = 4  # a tail the quality trim cuts
        if len(r) == 150 and i % 17 == 6:
            q[10:130 if i % 2 else 30] = 3  # a stretch the mask turns unknown: most of the read, or a few bases
        if len(r) == 150 and i % 29 == 8:
            q[:] = rng.choice([8, 12, 16], size=150)  # a read the mean-quality bound drops
        quals.append(q)
    # the prep stages, in the documented order: crops and quality trim, 3' adapter, tail cut, mask, length and quality bounds, complexity, decoy, cap
    ranges = [read_trim_rule.kept_range(q, len(r), FRONT, TAIL, read_trim_rule.qual_milli(TRIM_Q), WINDOW) for r, q in zip(reads, quals)]
    ranges, ainfo = adapter_rule.cut_ranges(reads, ranges, [ADAPTER], 100, 3)
    ranges, pinfo = polyx_rule.cut_ranges(reads, ranges, "G", M)
    left = [r[a:b] for r, (a, b) in zip(reads, ranges)]
    lq = [q[a:b] for q, (a, b) in zip(quals, ranges)]
    masked = [mask_qual_rule.masked(r, q, MASK_Q) if len(r) else r for r, q in zip(left, lq)]
    T = read_filter_rule.threshold(read_filter_rule.qual_milli(MIN_Q))
    fates = [read_filter_rule.fate(len(r), q, MIN_LEN, MAX_LEN, T) for r, q in zip(masked, lq)]
    passed = [f == read_filter_rule.KEEP for f in fates]
    cinfo, keep = polyx_rule.census(masked, passed, P)
    dinfo, keep = decoy_rule.census(masked, keep, decoy_rule.decoy_set([decoy], DK), DK)
    kept = [i for i, k in enumerate(keep) if k]
    kept_bases = sum(len(masked[i]) for i in kept)
    max_covg = kept_bases // (2 * G) - 1  # the cap is reached about half way through the kept reads
    taken, taken_bases, reached = max_covg_rule.accepted_reads([len(masked[i]) for i in kept], G, max_covg)
    assert reached and 0 < taken < len(kept) - 100
    # every stage matters: no run that leaves one out gives the prepared snapshot
    assert ainfo["reads_cut"] > 20 and pinfo["reads_cut"] > 100 and cinfo["reads_dropped"] > 50 and 15 < dinfo["reads_dropped"] <= 30
    assert fates.count(read_filter_rule.SHORT) > 100 and fates.count(read_filter_rule.LONG) == 2 and fates.count(read_filter_rule.LOWQ) > 30
    assert sum(m != l for m, l in zip(masked, left)) > 50 and int(offs[-1]) < 750_000
    b, o = _flat(reads)
    _SAMPLE.update(reads=reads, quals=quals, bases=b, offs=o, decoy=decoy, masked=masked, lq=lq, kept=kept, taken=taken, max_covg=max_covg,
                   pinfo=pinfo, cinfo=cinfo)
    return _SAMPLE


def _bam(path, reads, quals, without_qual=()):
    """every third record on the reverse strand (SEQ reverse-complemented, QUAL mirrored); the records of without_qual carry no QUAL"""
    recs = []
    for i, (r, q) in enumerate(zip(reads, quals)):
        qb = None if i in without_qual else q.astype(np.uint8).tobytes()
        if i % 3 == 0:
            recs.append(Rec(r.upper().translate(COMP)[::-1].decode(), flag=0x10, name=b"r%d" % i, qual=None if qb is None else qb[::-1]))
        else:
            recs.append(Rec(r.upper().decode(), flag=4, name=b"r%d" % i, qual=qb))
    return str(write_bam(path, recs))


def _files(tmp_path, s):
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    gz = _write_fastq(tmp_path / "all.fq.gz", s["bases"], s["offs"], s["quals"], gz=True)
    return dict(fastq=fq, gz=gz, bam=_bam(tmp_path / "all.bam", s["reads"], s["quals"]))


def _upper(reads):
    return [r.upper() for r in reads]  # (BAM holds no case; the statistics do not see it either)


def test_the_raw_snapshot_of_a_file_is_the_rules(tmp_path):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample()
    lay = rule.layout()
    want = _want("sample raw", lambda: rule.snapshot(s["reads"], s["quals"], lay))
    want_n = _want("sample raw, no qualities", lambda: rule.snapshot(s["reads"], None, lay))
    files = _files(tmp_path, s)
    files["bam, one record without QUAL"] = _bam(tmp_path / "noqual.bam", s["reads"], s["quals"], without_qual={1203})
    ctx.set_read_stats(1)
    for form, path in files.items():
        for packed in (False, True):
            for threads in (1, 4):
                mode = 2 if "without" in form else 1
                ctx.set_read_stats(mode)
                ctx.reset()
                ctx.set_threads(threads)
                ctx.set_input_format(packed)
                ctx.map_fastx(path)
                what = (form, packed, threads)
                _same(ctx.read_stats_info(0), want if mode == 1 else want_n, what)
                assert ctx.read_stats_prepared_is_raw(), what
                _same(ctx.read_stats_info(1), want if mode == 1 else want_n, what + ("prepared is raw",))
    assert rule.n50(want, lay) == 150 and int(want[3]) == 2000
    # mode 1 on the BAM whose record lacks QUAL: refused, naming the flag
    from drprg_amd.pandora import DependencyError
    ctx.set_read_stats(1)
    ctx.reset()
    with pytest.raises(DependencyError) as e:
        ctx.map_fastx(files["bam, one record without QUAL"])
    assert e.value.code == EINVAL and "--qc-json" in str(e.value), str(e.value)
    ctx.close()


def _everything(ctx):
    cov, prg = ctx.coverage()
    return cov, prg, ctx.counters(), {k: getattr(ctx, k)() for k in INFOS}


def test_the_setting_alone_changes_nothing_else(tmp_path):
    import resident_readback as rb
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample()
    files = _files(tmp_path, s)
    for form, packed, keep in (("fastq", False, False), ("fastq", True, True), ("bam", False, True), ("gz", True, False)):
        runs = []
        for mode in (0, 1, 2):
            ctx.set_read_stats(mode)
            ctx.reset()
            ctx.set_threads(2)
            ctx.set_input_format(packed)
            if keep:
                ctx.keep_reads(1 << 28)
            ctx.map_fastx(files[form])
            runs.append(_everything(ctx))
            if keep and mode:  # the resident sample is the file's reads, byte for byte
                rb.assert_resident(ctx, s["reads"] if form != "bam" else _upper(s["reads"]), packed or form == "bam", (form, mode))
            if mode == 0:
                assert ctx.read_stats_info(0)["reads"] == 0 and not ctx.read_stats_info(0)["words"].any()
        for other in runs[1:]:
            assert np.array_equal(other[0], runs[0][0]) and np.array_equal(other[1], runs[0][1]) and other[2] == runs[0][2] and other[3] == runs[0][3], form
    ctx.close()


def _prepare(ctx, tmp_path, s, cap=True):
    ctx.set_read_trim(front=FRONT, tail=TAIL, qual=TRIM_Q, window=WINDOW)
    ctx.set_adapters([ADAPTER])
    ctx.set_poly_trim("G", M)
    ctx.set_base_mask(MASK_Q)
    ctx.set_read_filter(min_len=MIN_LEN, max_len=MAX_LEN, min_qual=MIN_Q)
    ctx.set_min_complexity(P)
    ctx.set_decoy([_fasta(tmp_path / "decoy.fa", [s["decoy"]])], k=DK)
    ctx.set_max_covg(s["max_covg"] if cap else None)


def test_the_prepared_snapshot_is_the_rule_on_what_every_stage_leaves(tmp_path):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample()
    lay = rule.layout()
    raw = _want("sample raw", lambda: rule.snapshot(s["reads"], s["quals"], lay))
    went_on = s["kept"][:s["taken"]]
    prepared = _want("sample prepared", lambda: rule.snapshot(_upper(s["masked"][i] for i in went_on), [s["lq"][i] for i in went_on], lay))
    uncapped = _want("sample prepared, no cap", lambda: rule.snapshot(_upper(s["masked"][i] for i in s["kept"]), [s["lq"][i] for i in s["kept"]], lay))
    assert prepared[0] == s["taken"] and 0 < prepared[1] < uncapped[1] < raw[1]
    files = _files(tmp_path, s)
    _prepare(ctx, tmp_path, s)
    ctx.set_read_stats(1)
    for form in ("fastq", "gz", "bam"):
        for packed in (False, True):
            ctx.reset()
            ctx.set_threads(4 if packed else 1)
            ctx.set_input_format(packed)
            ctx.keep_reads(1 << 28)
            ctx.map_fastx(files[form])
            what = (form, packed)
            assert not ctx.read_stats_prepared_is_raw()
            _same(ctx.read_stats_info(1), prepared, what + ("prepared",))
            _same(ctx.read_stats_info(0), raw, what + ("raw stays what it was",))
            assert ctx.max_covg_info()["reads"] == s["taken"] and ctx.poly_trim_info() == s["pinfo"] and ctx.complexity_info() == s["cinfo"], what
    # without the cap; and without the qualities' sections
    ctx.set_max_covg(None)
    ctx.reset()
    ctx.map_fastx(files["fastq"])
    _same(ctx.read_stats_info(1), uncapped, "no cap")
    ctx.set_read_stats(2)
    ctx.set_max_covg(s["max_covg"])
    ctx.reset()
    ctx.map_fastx(files["bam"])
    got = ctx.read_stats_info(1)
    _same(got, _want("sample prepared, no qualities", lambda: rule.snapshot(_upper(s["masked"][i] for i in went_on), None, lay)), "mode 2")
    ctx.close()


def test_a_depth_cap_alone_separates_the_two_snapshots(tmp_path):
    """no prep setting: the blocks go through the unfiltered path, the block that crosses the cap is cut on the host"""
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample()
    lay = rule.layout()
    raw = _want("sample raw", lambda: rule.snapshot(s["reads"], s["quals"], lay))
    lengths = [len(r) for r in s["reads"]]
    taken, _, reached = max_covg_rule.accepted_reads(lengths, G, 9)
    assert reached and 100 < taken < len(lengths) - 100
    want = rule.snapshot(_upper(s["reads"][:taken]), s["quals"][:taken], lay)
    files = _files(tmp_path, s)
    ctx.set_read_stats(1)
    ctx.set_max_covg(9)
    for form, packed in (("fastq", False), ("fastq", True), ("bam", False)):
        ctx.reset()
        ctx.set_threads(2)
        ctx.set_input_format(packed)
        ctx.map_fastx(files[form])
        assert not ctx.read_stats_prepared_is_raw() and ctx.max_covg_info()["reads"] == taken
        _same(ctx.read_stats_info(1), want, (form, packed, "prepared"))
        _same(ctx.read_stats_info(0), raw, (form, packed, "raw"))
    ctx.close()


def test_a_reset_zeroes_both_snapshots_and_samples_do_not_leak(tmp_path):
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample()
    lay = rule.layout()
    raw = _want("sample raw", lambda: rule.snapshot(s["reads"], s["quals"], lay))
    files = _files(tmp_path, s)
    bases, offs = _reads_of(genomes, [100] * 300 + [0, 0], seed=4)
    other = [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(302)]
    oq = [np.full(len(r), 25, np.uint8) for r in other]
    other_fq = _write_fastq(tmp_path / "other.fq", bases, offs, oq)
    ctx.set_read_stats(1)
    ctx.set_read_filter(min_len=120)
    ctx.map_fastx(files["fastq"])
    assert ctx.read_stats_info(0)["reads"] == len(s["reads"]) and 0 < ctx.read_stats_info(1)["reads"] < len(s["reads"])
    ctx.reset()
    for which in (0, 1):
        got = ctx.read_stats_info(which)
        assert not got["words"].any(), which
    assert ctx.read_stats_prepared_is_raw()
    # the next sample on the same context: its own words, nothing of the first
    ctx.map_fastx(other_fq)
    _same(ctx.read_stats_info(0), rule.snapshot(other, oq, lay), "the second sample, raw")
    _same(ctx.read_stats_info(1), rule.snapshot([], [], lay), "the second sample, prepared: nothing is 120 bases long")
    # a read trimmed to nothing that is kept is a read of 0 bases in the prepared snapshot
    dark = [b"G" * 150] * 5 + other[:20]
    db, do = _flat(dark)
    dq = [np.full(len(r), 30, np.uint8) for r in dark]
    ctx.set_read_filter()
    ctx.set_poly_trim("G", M)
    ctx.reset()
    ctx.map_fastx(_write_fastq(tmp_path / "dark.fq", db, do, dq))
    cut, _ = polyx_rule.cut(dark, "G", M)
    got = ctx.read_stats_info(1)
    _same(got, rule.snapshot(cut, [q[:len(c)] for q, c in zip(dq, cut)], lay), "reads emptied by the tail cut")
    assert got["len_reads"][0] == 5 and got["reads"] == 25 and got["min_len"] == 0
    _same(ctx.read_stats_info(0), rule.snapshot(dark, dq, lay), "raw of the same")
    ctx.set_poly_trim("")
    # a second file without a reset adds to the first: sums add, the shortest and longest read are those of both
    ctx.set_read_filter()
    ctx.reset()
    ctx.map_fastx(other_fq)
    ctx.map_fastx(files["gz"])
    _same(ctx.read_stats_info(0), rule.snapshot(other + s["reads"], oq + s["quals"], lay), "two files")
    assert raw[0] + 302 == ctx.read_stats_info(0)["reads"]
    ctx.close()


# ---- 3. the executables ---------------------------------------------------------------------------------------------------------------------
def _json_equals(snap, words, lay, what, with_qual=True):
    """a snapshot of the JSON report against a snapshot's words"""
    d = {k: words[lay[k]:lay[k] + n] for k, n in (("len_reads", 2432), ("len_bases", 2432), ("qual_hist", 94), ("readq_hist", 94), ("gc_hist", 101), ("cyc_qsum", 513))}
    cyc = words[lay["cyc_base"]:lay["cyc_base"] + 513 * 5].reshape(513, 5)
    assert [snap["reads"], snap["bases"], snap["min_length"], snap["max_length"]] == [int(x) for x in words[:4]], what
    assert snap["n50"] == rule.n50(words, lay) and snap["n90"] == rule.n90(words, lay), what
    assert snap["base_totals"] == dict(zip("ACGTU", (int(x) for x in cyc.sum(axis=0)))), what
    assert snap["length_hist"] == [[rule.bin_low(b), int(d["len_reads"][b]), int(d["len_bases"][b])] for b in np.flatnonzero(d["len_reads"])], what
    n = min(int(words[3]), 513)
    assert snap["cycles"]["n"] == n and all(snap["cycles"][c] == [int(x) for x in cyc[:n, j]] for j, c in enumerate("ACGTU")), what
    assert snap["gc_hist"] == [int(x) for x in d["gc_hist"]], what
    if with_qual:
        assert snap["qual_hist"] == [int(x) for x in d["qual_hist"]] and snap["readq_hist"] == [int(x) for x in d["readq_hist"]], what
        assert snap["cycles"]["qual_sum"] == [int(x) for x in d["cyc_qsum"][:n]] and len(snap["cycles"]["mean_qual"]) == n, what
        tot = cyc[:n].sum(axis=1)
        assert all(abs(m - (int(q) / int(t) if t else 0)) < 6e-4 for m, q, t in zip(snap["cycles"]["mean_qual"], d["cyc_qsum"][:n], tot)), what
    else:
        assert "qual_hist" not in snap and "readq_hist" not in snap and "qual_sum" not in snap["cycles"], what


STAGES = dict(read_trim="read_trim_info", adapter_trim="adapter_trim_info", front_adapter="front_adapter_info", poly_trim="poly_trim_info", base_mask="base_mask_info",
              read_filter="read_filter_info", complexity="complexity_info", decoy="decoy_info", max_covg="max_covg_info")


def test_pandora_map_writes_the_report(tmp_path):
    from drprg_amd._lib import PANDORA_EXE
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample()
    lay = rule.layout()
    files = _files(tmp_path, s)
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    flags = ["--trim-front", str(FRONT), "--trim-tail", str(TAIL), "--trim-qual", str(TRIM_Q), "--trim-window", str(WINDOW), "--adapter", ADAPTER, "--poly-tail", "G",
             "--mask-qual", str(MASK_Q), "--min-read-len", str(MIN_LEN), "--max-read-len", str(MAX_LEN), "--min-read-qual", str(MIN_Q), "--min-complexity", str(P),
             "--decoy", _fasta(tmp_path / "decoy.fa", [s["decoy"]]), "--max-covg", str(s["max_covg"])]

    def run(out, reads, extra):
        argv = [PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(G)] + extra + [
            "--vcf-refs", genes, "-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout

    # every stage on: the report's numbers are those of drprg_hip_read_stats_info and of every *_info entry under the same settings
    qc = tmp_path / "qc.json"
    stdout = run(tmp_path / "prepared", files["fastq"], flags + ["--qc-json", str(qc)])
    rep = json.load(open(qc))
    _prepare(ctx, tmp_path, s)
    ctx.set_read_stats(1)
    ctx.set_threads(2)
    ctx.map_fastx(files["fastq"])
    raw, prepared = ctx.read_stats_info(0)["words"], ctx.read_stats_info(1)["words"]
    _same(dict(words=raw), _want("sample raw", lambda: rule.snapshot(s["reads"], s["quals"], lay)), "the context the report is compared with")
    assert rep["prepared_is_raw"] is False and rep["qualities"] is True and rep["length_resolution"] == "exact below 1024, 1/64 above" and rep["sample"] == "sample"
    _json_equals(rep["raw"], raw, lay, "raw")
    _json_equals(rep["prepared"], prepared, lay, "prepared")
    for name, info in STAGES.items():
        assert rep["stages"][name] == list(getattr(ctx, info)().values()), (name, rep["stages"][name], getattr(ctx, info)())
    assert rep["stages"]["dedup"] == [] and rep["stages"]["subsample"] == []
    assert rep["settings"]["mask_qual"] == MASK_Q and rep["settings"]["min_read_len"] == MIN_LEN and rep["settings"]["max_covg"] == s["max_covg"]
    assert list(rep)[:3] == ["sample", "format", "length_resolution"] and list(rep)[-4:] == ["settings", "raw", "prepared", "stages"]
    for which, w in (("raw", raw), ("prepared", prepared)):
        line = f"read statistics: {which} reads={int(w[0])} bases={int(w[1])} n50={rule.n50(w, lay)} mean_length={int(w[1]) / int(w[0]):.1f} mean_base_qual="
        assert line in stdout, (line, stdout)
    # nothing set, without qualities, a BAM: prepared is raw; --dedup's counts are in the report
    qc2 = tmp_path / "qc2.json"
    stdout = run(tmp_path / "plain", files["bam"], ["--max-covg", "4294967295", "--dedup", "--qc-json", str(qc2), "--qc-no-qual"])
    rep = json.load(open(qc2))
    want = _want("sample raw, no qualities", lambda: rule.snapshot(s["reads"], None, lay))
    assert rep["prepared_is_raw"] is True and rep["qualities"] is False and rep["prepared"] == rep["raw"]
    _json_equals(rep["raw"], want, lay, "raw, no qualities", with_qual=False)
    dd = rep["stages"]["dedup"]
    assert len(dd) == 4 and 0 < dd[2] <= dd[0] <= len(s["reads"]) and 0 < dd[3] <= dd[1] <= rep["raw"]["bases"], dd
    assert "mean_base_qual" not in stdout and "(prepared_is_raw)" in stdout
    # without the flag: no line, no file
    assert "read statistics:" not in run(tmp_path / "off", files["fastq"], [])
    ctx.close()


def test_drprg_predict_writes_the_report_of_its_first_pass(tmp_path):
    import os
    from drprg_amd import synth
    from test_gpu_predict_e2e import BIN, _make_index
    idx, panel, _ = _make_index(tmp_path)
    lay = rule.layout()
    rng = np.random.default_rng(7)
    spacer = synth.random_seq(rng, 300)
    genome = spacer + spacer.join(panel.refs) + spacer
    gn = np.frombuffer(genome.encode(), np.uint8)
    starts = rng.integers(0, len(gn) - 150, size=16000)
    block = gn[starts[:, None] + np.arange(150)]
    reads, _ = polyx_rule.tailed_sample([block[i].tobytes() for i in range(len(starts))], seed=8)
    quals = [rng.choice(NOVASEQ, size=150, p=[0.01, 0.03, 0.11, 0.85]).astype(np.uint8) for _ in reads]
    cut, pinfo = polyx_rule.cut(reads, "G", M)
    cq = [q[:len(c)] for q, c in zip(quals, cut)]
    b, o = _flat(reads)
    fq = _write_fastq(tmp_path / "reads.fq", b, o, quals)
    qc = tmp_path / "out" / "qc.json"
    argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "-o", str(tmp_path / "out"), "-s", "s1", "-I", "-v", "--poly-tail", "G", "--qc-json", str(qc)]
    r = subprocess.run(argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rep = json.load(open(qc))
    assert rep["sample"] == "s1" and rep["prepared_is_raw"] is False
    _json_equals(rep["raw"], rule.snapshot(reads, quals, lay), lay, "raw")
    _json_equals(rep["prepared"], rule.snapshot(cut, cq, lay), lay, "prepared")
    assert rep["stages"]["poly_trim"] == [pinfo[k] for k in ("reads_seen", "bases_seen", "reads_cut", "bases_cut", "reads_emptied")]
    assert r.stderr.count("read statistics: raw reads=16000 ") == 1 and r.stderr.count("read statistics: prepared reads=16000 ") == 1, r.stderr
