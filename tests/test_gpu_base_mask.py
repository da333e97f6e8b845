"""Base masking (drprg_hip_set_base_mask, csrc/base_mask.hip; pytest -m gpu).  Expected bytes, words, lists and counts come from the rule in
plain Python (tests/mask_qual_rule.py), vectors, counters and VCFs from the oracle on the rule's reads -- never from the code under test.

How the blocks come about: the ingest hands a worker's first block over at 750 000 bases, so the small sample (under that) is one block
and the big one several, whatever the number of parser threads."""
import json
import os
import subprocess

import numpy as np
import pytest

import adapter_rule
import decoy_rule
import mask_qual_rule as rule
import read_trim_rule as rtrim
import resident_readback as rb
from dedup_rule import keep_flags_fast
from test_gpu_decoy import _fasta, _flat
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from test_gpu_read_filter import _assert_oracle, _file_of, _write_bam, _write_fastq
from util import vcf_without_date

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
Q = rule.Q
EINVAL, ENODATA, EOVERFLOW, EFORMAT = 22, 61, 75, 84
NO_MASK = dict(reads_seen=0, bases_seen=0, reads_masked=0, bases_masked=0, bases_already_unknown=0)
OTHER = bytes.maketrans(b"ACGT", b"CATG")


def _masked(reads, quals, rev=None):
    return [rule.masked(r, q, Q, bool(rev[i]) if rev is not None else False) for i, (r, q) in enumerate(zip(reads, quals))]


# ---- 1. the kernel against the rule, on device buffers ----------------------------------------------------------------------------------------
def _device_mask(ctx, torch, reads, quals, rev, form, bias, shifted, cap=None, want_list=True):
    """one call of the device entry; returns (the six words, the bases behind it -- bytes or words --, the list, the pad behind the bases)"""
    text, offs = _flat(reads)
    n_reads, n_bases = len(reads), int(offs[-1])
    qflat = (np.concatenate([np.asarray(q, dtype=np.uint8) for q in quals]) if n_bases else np.zeros(0, np.uint8)) + np.uint8(bias)
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_r = torch.from_numpy(np.asarray(rev, dtype=np.uint8)).cuda() if any(rev) else None
    qs = 1 if shifted else 0  # (one byte off: read byte by byte, and the buffer ends with its last byte)
    qbuf = np.full(n_bases + (qs if shifted else 64), 0 if not shifted else 200, dtype=np.uint8)
    qbuf[qs:qs + n_bases] = qflat
    d_q = torch.from_numpy(qbuf).cuda()
    assert d_q.data_ptr() % 16 == 0
    STALE = 0x5A
    if form == "text":
        ts = 3 if shifted else 0
        buf = np.full(ts + n_bases + 64, STALE, dtype=np.uint8)
        buf[ts:ts + n_bases] = text
        d_t = torch.from_numpy(buf).cuda()
        try:
            out = ctx.base_mask_device(d_q.data_ptr() + qs, bias, d_o.data_ptr(), d_r.data_ptr() if d_r is not None else None, n_reads, n_bases,
                                       d_t.data_ptr() + ts, None, None, 0, None, 0)
        finally:
            torch.cuda.synchronize()
        got = d_t.cpu().numpy()
        return out, got[ts:ts + n_bases].tobytes(), [], got[ts + n_bases:].tolist() + got[:ts].tolist()
    words, npos = adapter_rule.packed_form(text.tobytes())
    ws = 1 if shifted else 0  # (one word off: no 16-byte alignment)
    wbuf = np.full(ws + words.size + 16, 0x5A5A5A5A, dtype=np.uint32)
    wbuf[ws:ws + words.size] = words
    d_w = torch.from_numpy(wbuf.view(np.int32)).cuda()
    d_n = torch.from_numpy(npos.astype(np.int64)).cuda() if npos.size else None
    cap = n_bases if cap is None else cap
    d_out = torch.full((max(cap, 1) + 4,), -7, dtype=torch.int64, device="cuda")  # (stale on purpose)
    try:
        out = ctx.base_mask_device(d_q.data_ptr() + qs, bias, d_o.data_ptr(), d_r.data_ptr() if d_r is not None else None, n_reads, n_bases, None,
                                   d_w.data_ptr() + 4 * ws, d_n.data_ptr() if d_n is not None else None, int(npos.size), d_out.data_ptr() if want_list else None, cap)
    finally:
        torch.cuda.synchronize()
        _device_mask.last = (d_w.cpu().numpy().view(np.uint32)[ws:ws + words.size].copy(), d_out.cpu().numpy().copy())
    got = d_w.cpu().numpy().view(np.uint32)
    lst = d_out.cpu().numpy()
    assert lst[int(out[5]):].tolist() == [-7] * (lst.size - int(out[5]))  # nothing behind the list was written
    return out, got[ws:ws + words.size], lst[:int(out[5])].tolist(), got[ws + words.size:].tolist() + got[:ws].tolist()


def _expect(reads, quals, rev, form):
    m = b"".join(_masked(reads, quals, rev))
    info = rule.info(reads, quals, Q, rev)
    counts = tuple(info[k] for k in ("reads_seen", "bases_seen", "reads_masked", "bases_masked", "bases_already_unknown"))
    if form == "text":
        return m, [], counts + (0,)
    words, npos = adapter_rule.packed_form(m)
    return words, npos.tolist(), counts + (int(npos.size),)


@pytest.mark.parametrize("bias", [33, 0])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("form", ["text", "packed"])
def test_the_kernels_equal_the_rule(tmp_path, form, shifted, bias):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.set_base_mask(Q)

    def check(batch, what):
        reads, quals, rev = batch
        want, want_list, want_out = _expect(reads, quals, rev, form)
        out, got, lst, pad = _device_mask(ctx, torch, reads, quals, rev, form, bias, shifted)
        print(what, "out", out, "expected", want_out)
        assert out == want_out, (what, out, want_out)
        if form == "text":
            diff = [p for p in range(len(want)) if got[p] != want[p]]
            assert not diff, (what, len(diff), diff[:8], got[diff[0] - 4:diff[0] + 4], want[diff[0] - 4:diff[0] + 4])
            assert set(pad) == {0x5A}, (what, "bytes outside the block were written")
        else:
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, (what, diff.size, diff[:8].tolist(), [hex(int(x)) for x in got[diff[:4]]], [hex(int(x)) for x in want[diff[:4]]])
            assert lst == want_list, (what, len(lst), len(want_list), [(a, b) for a, b in zip(lst, want_list) if a != b][:8])
            assert set(pad) == {0x5A5A5A5A}, (what, "words outside the block were written")
        return want_out

    full = rule.kernel_batch()
    out = check(full, "ragged")
    assert out[3] > 500 and out[4] >= 2
    # a second, smaller launch on the same context: nothing of the first one is left behind
    small = ([b"", b"ACGTNACGTACGTACGTA", b"", b"acgtRYacgtacgtacg"], [np.zeros(0, np.uint8), np.array([2] + [35] * 3 + [2] + [35] * 12 + [9]), np.zeros(0, np.uint8),
                                                                      np.array([35] * 5 + [2] + [35] * 10 + [2])], [False, False, False, True])
    assert check(small, "small")[2:5] == (2, 4, 1)
    out = check(rule.kernel_batch(listed=False), "no list before")  # an empty list before, a list after
    assert out[4] == 0 and out[5] == out[3] or form == "text"
    assert check(rule.kernel_batch(listed=False, low=False), "nothing")[2:] == (0, 0, 0, 0)  # both empty
    assert check(([b"", b"", b""], [np.zeros(0, np.uint8)] * 3, [False, True, False]), "empty reads only") == (3, 0, 0, 0, 0, 0)
    reads, quals, rev = full
    if form == "packed":  # a list buffer one entry short: -EOVERFLOW, the needed length still reported
        need = _expect(reads, quals, rev, form)[2][5]
        with pytest.raises(DependencyError) as e:
            _device_mask(ctx, torch, reads, quals, rev, form, bias, shifted, cap=need - 1)
        assert e.value.code == EOVERFLOW and ctx.last_mask_out[5] == need and ctx.last_mask_out[:5] == _expect(reads, quals, rev, form)[2][:5]
        assert set(_device_mask.last[1].tolist()) == {-7}
    # a quality byte out of range: -84, the text naming its position (the first one); in a forward and in a reversed read
    starts = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    for i in (next(i for i in range(20, len(reads)) if not rev[i] and len(reads[i]) > 40), next(i for i in range(20, len(reads)) if rev[i] and len(reads[i]) > 40)):
        bad = [q.copy() for q in quals]
        for at in (7, 30):
            bad[i][at] = 94 if bias == 0 else 255  # (255 + 33 wraps to 32, one below the bias)
        with pytest.raises(DependencyError) as e:
            _device_mask(ctx, torch, reads, bad, rev, form, bias, shifted)
        assert e.value.code == EFORMAT and f"quality byte {int(starts[i]) + 7}" in str(e.value) and str(int(starts[i]) + 30) not in str(e.value), str(e.value)
    # offsets that do not run from 0 to n_bases
    d_q = torch.from_numpy(np.full(200, 35 + bias, np.uint8)).cuda()
    d_t = torch.from_numpy(np.full(200, 65, np.uint8)).cuda()
    for offs in ([1, 50, 100], [0, 50, 99]):
        d_o = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
        with pytest.raises(DependencyError) as e:
            ctx.base_mask_device(d_q.data_ptr(), bias, d_o.data_ptr(), None, 2, 100, d_t.data_ptr(), None, None, 0, None, 0)
        assert e.value.code == EINVAL, offs
    ctx.set_base_mask(0)
    with pytest.raises(DependencyError) as e:
        ctx.base_mask_device(d_q.data_ptr(), bias, d_o.data_ptr(), None, 2, 100, d_t.data_ptr(), None, None, 0, None, 0)
    assert e.value.code == EINVAL
    ctx.close()


# ---- 2. a masked sample equals the sample of its masked reads ---------------------------------------------------------------------------------
_SAMPLES = {}


def _sample(which, oracle, ctx):
    """panel reads with substitution errors at half of their low-quality bases (the other half are correct bases of low quality), a letter
    that is no base in every tenth read, some of those of low quality; the rule's reads and the oracle's vectors of them: made once, shared,
    left unchanged"""
    if which not in _SAMPLES:
        _, genomes = _panel()
        lengths, quals = rule.small_sample() if which == "small" else rule.big_sample()
        bases, offs = _reads_of(genomes, lengths, seed=63)
        bases = bases.copy()
        rng = np.random.default_rng(64)
        qflat = np.concatenate(quals)
        wrong = np.flatnonzero((qflat < Q) & (rng.random(qflat.size) < 0.5))
        bases[wrong] = np.frombuffer(bases[wrong].tobytes().translate(OTHER), dtype=np.uint8)
        for i in range(0, len(lengths), 10):
            if lengths[i] > 40:
                bases[int(offs[i]) + 5] = ord("N")
                if i % 20 == 0:
                    quals[i][5] = 3
        data = bases.tobytes()
        reads = [data[int(offs[i]):int(offs[i + 1])] for i in range(len(lengths))]
        masked = _masked(reads, quals)
        mb, mo = _flat(masked)
        idx = _oracle_index(oracle, ctx.prg_strings, W, K)
        s = dict(reads=reads, quals=quals, bases=bases, offs=offs, masked=masked, mbases=mb, info=rule.info(reads, quals, Q),
                 want=_oracle_map(oracle, idx, mb, mo, W, K, True, threads=4), plain=_oracle_map(oracle, idx, bases, offs, W, K, True, threads=4))
        # masking matters: no run that leaves the bases alone can pass
        assert not np.array_equal(s["want"][0], s["plain"][0]) and s["want"][2]["hits"] != s["plain"][2]["hits"]
        assert s["want"][2]["clusters_kept"] > 5 and s["info"]["bases_already_unknown"] > 3 and s["info"]["bases_masked"] > 0.03 * mb.size
        _SAMPLES[which] = s
    return _SAMPLES[which]


def _assert_masked(ctx, s, what, calls=1):
    if calls == 1:
        _assert_oracle(ctx, s["want"], len(s["reads"]), int(s["offs"][-1]), what)
    assert ctx.base_mask_info() == {k: calls * v for k, v in s["info"].items()}, (what, ctx.base_mask_info(), s["info"])


@pytest.mark.parametrize("form", ["fastq ascii", "fastq packed", "bam"])
@pytest.mark.parametrize("which", ["small", "big"])
def test_a_masked_sample_equals_the_sample_of_its_masked_reads(tmp_path, oracle, which, form):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample(which, oracle, ctx)
    path = _file_of(tmp_path, form, s["bases"], s["offs"], s["quals"], "all")
    ctx.set_base_mask(Q)
    for packed in ((True,) if form == "fastq packed" else (False,) if form == "fastq ascii" else (False, True)):
        for threads in (1, 4):
            ctx.reset()
            ctx.set_threads(threads)
            ctx.set_input_format(packed)
            ctx.keep_reads(1 << 28)
            ctx.map_fastx(path)
            _assert_masked(ctx, s, (which, form, packed, threads))
            info = ctx.resident_info()
            assert info["complete"] and (info["blocks"] == 1 if which == "small" else info["blocks"] >= 2), info
            if which == "small" or threads == 1:  # the resident reads are the rule's reads, byte for byte
                rb.assert_resident(ctx, s["masked"], packed or form == "bam", (form, packed, threads))
    if form == "fastq ascii":  # a context given the file with N alone, with no mask; and the setting off: the plain reads' vectors
        ctx.set_base_mask(0)
        ctx.reset()
        ctx.map_fastx(_write_fastq(tmp_path / "masked.fq", s["mbases"], s["offs"], s["quals"]))
        _assert_oracle(ctx, s["want"], len(s["reads"]), int(s["offs"][-1]), "the file with N")
        assert ctx.base_mask_info() == NO_MASK
        ctx.reset()
        ctx.map_fastx(path)
        _assert_oracle(ctx, s["plain"], len(s["reads"]), int(s["offs"][-1]), "no mask")
    ctx.close()


# ---- 3. the point of it -------------------------------------------------------------------------------------------------------------------------
def test_a_low_quality_error_puts_no_coverage_on_the_other_allele(tmp_path, oracle):
    """reads of a haplotype that carries the first allele everywhere; in half of the reads over one SNP site the base is the other allele's,
    at quality 2.  Unmasked, the oracle puts coverage on that allele's k-mer nodes; masked, none -- and the device run equals the latter."""
    from drprg_amd import synth
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    rng = np.random.default_rng(65)
    refs = [synth.haplotype_with(t, lambda i: 0) for t in panel.trees]
    assert refs == panel.refs
    n_nodes = [oracle.sketch_prg(p, W, K)["n_nodes"] for p in panel.prgs]
    base = np.concatenate([[0], np.cumsum(n_nodes)])
    # a SNP site of a locus, away from the ends, whose other allele has k-mer nodes of its own
    pick = None
    for g, prg in enumerate(panel.prgs):
        for rec in oracle.vcf_sites(prg, W, K)[0]:
            if pick is None and rec["vc"] == "SNP" and len(rec["ref"]) == 1 and 200 < rec["pos"] < len(refs[g]) - 200:
                own = sorted(set(rec["knodes"][1]) - set(rec["knodes"][0]))
                if len(own) >= 2 and len(rec["alts"][0]) == 1:
                    pick = (g, rec, own)
    assert pick is not None
    g, rec, own = pick
    at = rec["pos"] - 1
    assert refs[g][at] == rec["ref"], (refs[g][at - 3:at + 4], rec)
    nodes = np.asarray([2 * (int(base[g]) + j) + s for j in own for s in (0, 1)])
    spacer = synth.random_seq(rng, 300)
    genome = spacer + spacer.join(refs) + spacer
    site = len(spacer) + sum(len(r) + len(spacer) for r in refs[:g]) + at
    gn = np.frombuffer(genome.encode(), np.uint8)
    starts = rng.integers(0, len(gn) - 150, size=3000)
    reads, quals = [], []
    for i, s0 in enumerate(int(x) for x in starts):
        r, q = bytearray(gn[s0:s0 + 150].tobytes()), np.full(150, rule.GOOD, dtype=np.uint8)
        if s0 <= site < s0 + 150 and i % 2 == 0:
            r[site - s0:site - s0 + 1] = rec["alts"][0].encode()
            q[site - s0] = 2
        if i % 3 == 0:  # either strand
            r, q = bytearray(bytes(r).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]), q[::-1].copy()
        reads.append(bytes(r))
        quals.append(q)
    assert sum(int((q < Q).sum()) for q in quals) > 20
    masked = _masked(reads, quals)
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    b, o = _flat(reads)
    mb, mo = _flat(masked)
    plain, want = _oracle_map(oracle, idx, b, o, W, K, True, threads=4), _oracle_map(oracle, idx, mb, mo, W, K, True, threads=4)
    print("coverage on the other allele's nodes: plain", int(plain[0][nodes].sum()), "masked", int(want[0][nodes].sum()))
    assert plain[0][nodes].sum() > 0 and want[0][nodes].sum() == 0
    fq = _write_fastq(tmp_path / "errors.fq", b, o, quals)
    for packed in (False, True):
        ctx.reset()
        ctx.set_input_format(packed)
        ctx.set_base_mask(0)
        ctx.map_fastx(fq)
        _assert_oracle(ctx, plain, len(reads), int(o[-1]), ("plain", packed))
        assert ctx.coverage()[0][nodes].sum() > 0
        ctx.reset()
        ctx.set_base_mask(Q)
        ctx.map_fastx(fq)
        _assert_oracle(ctx, want, len(reads), int(o[-1]), ("masked", packed))
        assert ctx.coverage()[0][nodes].sum() == 0 and ctx.base_mask_info() == rule.info(reads, quals, Q)
    ctx.close()


# ---- 4. order and neighbours --------------------------------------------------------------------------------------------------------------------
def test_the_mask_runs_behind_trimming_and_adapters(tmp_path, oracle):
    """--trim-qual, an adapter and --mask-qual together: the run is the oracle's on trim-rule, then adapter-rule, then mask-rule reads.  The
    adapter's letters are of a quality below Q in every read that holds it: it is still found and cut"""
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    ADAPTER, TRIM_Q = adapter_rule.TRUSEQ[:33], 20
    rng = np.random.default_rng(66)
    reads, quals = [], []
    for i, (r, q) in enumerate(zip(s["reads"], s["quals"])):
        if len(r) > 1000:
            continue
        q = q.copy()
        if i % 3 == 1 and len(r) > 100:  # read-through: the adapter at a low quality, good bases behind it
            at = int(rng.integers(60, len(r) - 20))
            tail = len(r) - at
            r = r[:at] + (ADAPTER.encode() + rule._dna(rng, 20))[:tail]
            q = q[:len(r)]
            q[at:at + min(33, tail)] = 5
            q[at + min(33, tail):] = rule.GOOD
            q[at - 8:at] = rule.GOOD
        elif i % 3 == 2 and len(r) > 60:  # bad ends: the quality trim takes them
            q[:6], q[-9:] = 2, 3
        reads.append(r)
        quals.append(q)
    rev = [i % 3 == 0 for i in range(len(reads))]  # (as _write_bam stores them: trimmed in stored order, the range mirrored)
    milli = rtrim.qual_milli(TRIM_Q)

    def expected(bam):
        ranges = [rtrim.kept_range_stored(q[::-1] if bam and v else q, len(r), bam and v, 0, 0, milli, 4) for r, q, v in zip(reads, quals, rev)]
        cut, ainfo = adapter_rule.cut_ranges(reads, ranges, [ADAPTER], 100, 3)
        left = [r[a:b] for r, (a, b) in zip(reads, cut)]
        lq = [q[a:b] for q, (a, b) in zip(quals, cut)]
        return cut, ainfo, left, lq

    cut, ainfo, left, lq = expected(False)
    assert ainfo["reads_cut"] > 80 and sum(b - a != len(r) for r, (a, b) in zip(reads, cut)) > 200
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    b, o = _flat(reads)
    ctx.set_read_trim(qual=TRIM_Q, window=4)
    ctx.set_adapters([ADAPTER])
    ctx.set_base_mask(Q)
    for form in ("fastq ascii", "fastq packed", "bam"):
        cut, ainfo, left, lq = expected(form == "bam")
        mb, mo = _flat(_masked(left, lq))
        want = _oracle_map(oracle, idx, mb, mo, W, K, True, threads=4)
        ctx.reset()
        ctx.set_threads(2)
        ctx.set_input_format(form == "fastq packed")
        ctx.map_fastx(_file_of(tmp_path, form, b, o, quals, "stages"))
        _assert_oracle(ctx, want, len(reads), int(mo[-1]), form)
        assert ctx.adapter_trim_info() == ainfo, form
        assert ctx.base_mask_info() == rule.info(left, lq, Q), (form, ctx.base_mask_info(), rule.info(left, lq, Q))
    ctx.close()


def test_dedup_and_the_decoy_screen_see_the_masked_reads(tmp_path, oracle):
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    rng = np.random.default_rng(67)
    pb, po = _reads_of(genomes, [150] * 300, seed=68)
    data = pb.tobytes()
    reads = [data[int(po[i]):int(po[i + 1])] for i in range(300)]
    quals = [np.full(150, rule.GOOD, dtype=np.uint8) for _ in reads]
    # two reads that differ only in a base masked in both are duplicates; two that differ in a base masked in one are not
    reads.append(reads[10][:70] + reads[10][70:71].translate(OTHER) + reads[10][71:])
    quals.append(quals[10].copy())
    quals[10][70] = quals[-1][70] = 2
    reads.append(reads[20][:70] + reads[20][70:71].translate(OTHER) + reads[20][71:])
    quals.append(quals[20].copy())
    quals[-1][70] = 2
    # decoy reads: dropped at good quality; kept when every decoy k-mer holds a masked base (V = 0)
    decoy = decoy_rule.random_dna(np.random.default_rng(71), 5000)
    DK = 31
    for j in range(20):
        reads.append(decoy[100 * j:100 * j + 150])
        q = np.full(150, rule.GOOD, dtype=np.uint8)
        if j % 2:
            q[15::30] = 2
        quals.append(q)
    masked = _masked(reads, quals)
    D = decoy_rule.decoy_set([decoy], DK)
    census, keep = decoy_rule.census(masked, [True] * len(masked), D, DK)
    vh = decoy_rule.verdicts(masked, D, DK)
    assert [v[:2] for v in vh[-20:]] == [(120, 120), (0, 0)] * 10 and census["reads_dropped"] == 10 and keep[-1] and not keep[-2]
    kept = [r for r, k in zip(masked, keep) if k]
    flags = keep_flags_fast(kept)
    assert flags[300] == 0 and flags[301] == 1 and flags[10] == flags[20] == 1
    b, o = _flat(reads)
    for packed in (False, True):
        ctx.reset()
        ctx.set_base_mask(Q)
        ctx.set_decoy([_fasta(tmp_path / "decoy.fa", [decoy])], k=DK)
        ctx.set_input_format(packed)
        ctx.set_ordered_ingest(True)
        ctx.keep_reads(1 << 28)
        ctx.map_fastx(_write_fastq(tmp_path / "n.fq", b, o, quals))
        info = ctx.decoy_info()
        assert {k: info[k] for k in census} == census, (packed, info, census)
        rb.assert_resident(ctx, kept, packed, ("behind the screen", packed))
        out = ctx.dedup()
        assert out["reads_before"] == len(kept) and out["reads_kept"] == sum(flags), (packed, out)
        assert ctx.dedup_flags(len(kept)).tolist() == flags
    ctx.close()


# ---- 5. refusals and state ----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(tmp_path, oracle):
    import torch
    from bam_writer import Rec, write as write_bam
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    ctx.set_threads(2)
    for bad in (94, 1000):
        with pytest.raises(DependencyError) as e:
            ctx.set_base_mask(bad)
        assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        ctx.set_base_mask(12.5)
    ctx.map_fastx(fq)  # the refusals left nothing set
    _assert_oracle(ctx, s["plain"], len(s["reads"]), int(s["offs"][-1]), "nothing set")
    assert ctx.base_mask_info() == NO_MASK
    # reads without qualities
    ctx.set_base_mask(Q)
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(s["reads"][:50]) if r))
    noq = str(write_bam(tmp_path / "noqual.bam", [Rec(r.decode(), flag=4, name=b"r%d" % i, qual=None) for i, r in enumerate(s["reads"][:50]) if r]))
    for path in (str(fa), noq):
        for packed in (False, True):
            ctx.reset()
            ctx.set_input_format(packed)
            with pytest.raises(DependencyError) as e:
                ctx.map_fastx(path)
            assert e.value.code == EINVAL and "--mask-qual" in str(e.value), (path, str(e.value))
    ctx.set_read_trim(qual=20)  # (trimming is the first to miss them: it is named)
    ctx.reset()
    with pytest.raises(DependencyError) as e:
        ctx.map_fastx(str(fa))
    assert e.value.code == EINVAL and "--trim-qual" in str(e.value)
    ctx.set_read_trim()
    ctx.set_read_filter(min_qual=10)  # (the mask comes in front of the filter)
    ctx.reset()
    with pytest.raises(DependencyError) as e:
        ctx.map_fastx(str(fa))
    assert e.value.code == EINVAL and "--mask-qual" in str(e.value)
    ctx.set_read_filter()
    # a quality byte out of range fails the run
    q = [x.copy() for x in s["quals"]]
    q[40][3] = 94
    ctx.reset()
    with pytest.raises(DependencyError) as e:
        ctx.map_fastx(_write_bam(tmp_path / "bad.bam", s["bases"], s["offs"], q))
    assert e.value.code == EFORMAT
    # map_host and map_device carry no qualities: refused while the setting is on, served again once it is off
    ctx.reset()
    d_b, d_o = torch.from_numpy(s["mbases"].copy()).cuda(), torch.from_numpy(s["offs"].astype(np.int64)).cuda()
    calls = (lambda: ctx.map_host(s["mbases"], s["offs"]), lambda: ctx.map_device(d_b.data_ptr(), d_o.data_ptr(), len(s["reads"]), int(s["offs"][-1])))
    for call in calls:
        with pytest.raises(DependencyError) as e:
            call()
        assert e.value.code == EINVAL and "drprg_hip_set_base_mask" in str(e.value)
    assert ctx.counters()["reads"] == 0
    # masked bases, no resident reads, discover: -61
    ctx.map_fastx(fq)
    _assert_masked(ctx, s, "after the refusals")
    (tmp_path / "disc").mkdir()
    with pytest.raises(DependencyError) as e:
        ctx.discover_reads(fq, str(tmp_path / "genes.fa"), str(tmp_path / "disc"))
    assert e.value.code == ENODATA and "--mask-qual" in str(e.value)
    # a second call adds to the counts; a reset clears them and keeps the setting
    ctx.map_fastx(fq)
    _assert_masked(ctx, s, "two calls", calls=2)
    ctx.reset()
    assert ctx.base_mask_info() == NO_MASK
    ctx.map_fastx(fq)
    _assert_masked(ctx, s, "after a reset")
    ctx.set_base_mask(0)
    for call in calls:
        ctx.reset()
        call()
        torch.cuda.synchronize()
        _assert_oracle(ctx, s["want"], len(s["reads"]), int(s["offs"][-1]), "the setting off")
    ctx.close()


def test_two_devices_give_the_vectors_of_one(tmp_path, oracle):
    from drprg_amd import Context
    if not os.environ.get("DRPRG_HIP_DEVICES"):
        pytest.skip("DRPRG_HIP_DEVICES is not set")
    devices = [int(x) for x in os.environ["DRPRG_HIP_DEVICES"].split(",")]
    if len(devices) < 2:
        pytest.skip("one device")
    panel, _ = _panel()
    one = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, one)
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=devices)
    multi.set_opts(illumina=True, genome_size=G)
    for c in (one, multi):
        c.set_threads(4)
        c.set_base_mask(Q)
        c.map_fastx(fq)
        _assert_masked(c, s, "devices")
    one.close()
    multi.close()


def test_one_device_listed_twice_gives_the_vectors_of_one(tmp_path, oracle):
    """the setting reaches every device's blocks: the same context over device 0 twice"""
    from drprg_amd import Context
    panel, _ = _panel()
    one = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, one)
    one.close()
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=[0, 0])
    multi.set_opts(illumina=True, genome_size=G)
    multi.set_threads(4)
    multi.set_base_mask(Q)
    multi.map_fastx(_write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"]))
    _assert_masked(multi, s, "device 0 twice")
    multi.close()


# ---- 6. the executables -------------------------------------------------------------------------------------------------------------------------
def _verbose_line(info):
    return "base masking: " + " ".join(f"{k}={info[k]}" for k in ("reads_seen", "bases_seen", "reads_masked", "bases_masked", "bases_already_unknown"))


def test_pandora_map_writes_the_vcf_of_the_file_with_n(tmp_path, oracle):
    from drprg_amd._lib import PANDORA_EXE
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    ctx.close()
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bam = _write_bam(tmp_path / "all.bam", s["bases"], s["offs"], s["quals"])
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    with_n = _write_fastq(tmp_path / "with_n.fq", s["mbases"], s["offs"], s["quals"])

    def run(out, reads, extra, cmd="map"):
        if cmd == "discover":
            (tmp_path / "query.tsv").write_text(f"s\t{reads}\n")
            tail = ["-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, str(tmp_path / "query.tsv")]
            argv = [PANDORA_EXE, "discover", "-v", "-o", str(out), "-g", str(G), "--max-covg", "4294967295"] + extra + tail
        else:
            argv = [PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(G), "--max-covg", "4294967295"] + extra + [
                "--vcf-refs", genes, "-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout

    run(tmp_path / "plain", with_n, [])
    want = vcf_without_date(str(tmp_path / "plain" / "pandora_genotyped.vcf"))
    for name, reads in (("masked_fq", fq), ("masked_bam", bam)):
        stdout = run(tmp_path / name, reads, ["--mask-qual", str(Q)])
        assert vcf_without_date(str(tmp_path / name / "pandora_genotyped.vcf")) == want, name
        assert _verbose_line(s["info"]) in stdout, stdout
    run(tmp_path / "unmasked", fq, [])
    assert vcf_without_date(str(tmp_path / "unmasked" / "pandora_genotyped.vcf")) != want  # (the flag is what made them equal)
    # the coverage discover left under one Q is taken by a map under the same Q only
    out = tmp_path / "handover"
    run(out / "discover", fq, ["--mask-qual", str(Q)], cmd="discover")
    for extra, reused in ((["--mask-qual", str(Q)], True), (["--mask-qual", str(Q + 1)], False), ([], False)):
        assert ("no second mapping pass" in run(out, fq, extra)) == reused, extra


def test_drprg_predict_masks_once_through_a_prg_update(tmp_path):
    """an off-panel variant: discover finds it in the resident (masked) reads, the PRG is updated and the reads are mapped again from device
    memory -- masked already, not masked twice: the run equals that of the file with N, and the counts are those of the one pass"""
    from drprg_amd import synth
    from test_gpu_predict_e2e import BIN, _aa, _make_index
    idx, panel, sites = _make_index(tmp_path)
    g = panel.names.index("katG")
    ref = panel.refs[g]
    taken = [p for _, p, r, _ in sites["katG"] for p in range(p - 40, p + len(r) + 40)]
    pos = next(p for p in range(100 + 3 * 250, len(ref) - 400, 3) if p not in taken and p + 1 not in taken and p + 2 not in taken)
    codon = ref[pos:pos + 3]
    alt_base = next(b for b in "ACGT" if b != codon[1] and _aa(codon[0] + b + codon[2]) not in (_aa(codon), "*"))
    mutated = ref[:pos + 1] + alt_base + ref[pos + 2:]
    rng = np.random.default_rng(7)
    spacer = synth.random_seq(rng, 300)
    genome = spacer + spacer.join(mutated if gi == g else r for gi, r in enumerate(panel.refs)) + spacer
    gn = np.frombuffer(genome.encode(), np.uint8)
    starts = rng.integers(0, len(gn) - 150, size=16000)
    block = gn[starts[:, None] + np.arange(150)]
    rev = rng.random(len(starts)) < 0.5
    block[rev] = synth._COMP[block[rev][:, ::-1]]
    quals = np.full(block.shape, rule.GOOD, dtype=np.uint8)
    low = rng.random(block.shape) < 0.03
    quals[low] = rng.integers(2, Q, size=int(low.sum()))
    wrong = low & (rng.random(block.shape) < 0.5)
    block[wrong] = np.frombuffer(block[wrong].tobytes().translate(OTHER), dtype=np.uint8)
    offs = np.arange(len(starts) + 1, dtype=np.uint64) * np.uint64(150)
    reads = [block[i].tobytes() for i in range(len(starts))]
    info = rule.info(reads, list(quals), Q)
    mb, _ = _flat(_masked(reads, list(quals)))
    fq = _write_fastq(tmp_path / "novel.fq", block.reshape(-1), offs, list(quals))
    with_n = _write_fastq(tmp_path / "with_n.fq", mb, offs, list(quals))

    def run(out, path, extra):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", path, "-o", str(out), "-s", "novel", "-I", "-v"] + extra
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        calls = json.load(open(out / "novel.drprg.json"))["susceptibility"]
        for drug in calls.values():
            for ev in drug["evidence"]:
                ev.pop("vcfid")
        return r.stderr, (open(out / "pandora_genotyped.vcf").read(), calls, open(out / "discover" / "denovo_variants.tsv").read())

    err, got = run(tmp_path / "masked", fq, ["--mask-qual", str(Q)])
    _, want = run(tmp_path / "with_n", with_n, [])
    assert got == want
    assert "novel site(s) added" in err and "reads mapped again (resident in device memory)" in err, err
    assert err.count(_verbose_line(info)) == 1 and err.count("base masking:") == 1, err
    assert any(e["gene"] == "katG" for v in got[1].values() for e in v["evidence"])
