"""Poly-tail trimming and the low-complexity filter (drprg_hip_set_poly_trim, csrc/poly_tail.hip; drprg_hip_set_min_complexity,
csrc/read_complexity.hip; pytest -m gpu).  Expected ranges, flags and counts come from the rules in plain Python (tests/polyx_rule.py),
vectors, counters and VCFs from the oracle on the rules' reads -- never from the code under test.

How the blocks come about: the ingest hands a worker's first block over at 750 000 bases, so the small sample (under that) is one block
and the big one several, whatever the number of parser threads."""
import subprocess

import numpy as np
import pytest

import adapter_rule
import decoy_rule
import mask_qual_rule
import polyx_rule as rule
import resident_readback as rb
from dedup_rule import keep_flags_fast
from test_gpu_decoy import _fasta, _fasta_reads, _flat
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from test_gpu_read_filter import _assert_oracle, _file_of, _write_bam, _write_fastq
from util import vcf_without_date

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
M, P = rule.M, rule.P
EINVAL, ENODATA = 22, 61
NO_POLY = dict(reads_seen=0, bases_seen=0, reads_cut=0, bases_cut=0, reads_emptied=0)
NO_CPLX = dict(reads_seen=0, bases_seen=0, reads_dropped=0, bases_dropped=0)
POLY_KEYS = ("reads_seen", "bases_seen", "reads_cut", "bases_cut", "reads_emptied")
GOOD = 35


# ---- 1. the kernels against the rules, on device buffers ---------------------------------------------------------------------------------
class _Bases:
    """a batch's bases on the device in one form -- text, or packed words with their list --, at a 16-byte aligned address or one byte / one
    word off it (such a text buffer ends with its last byte: it is read byte by byte), with stale bytes on both sides"""

    def __init__(self, torch, reads, form, shifted):
        text, offs = _flat(reads)
        self.n_reads, self.n_bases = len(reads), int(offs[-1])
        self.d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
        self.d_text = self.d_words = self.d_npos = None
        self.n_npos = 0
        if form == "text":
            ts = 1 if shifted else 0
            buf = np.full(ts + self.n_bases + (0 if shifted else 64), 0x5A, dtype=np.uint8)
            buf[ts:ts + self.n_bases] = text
            self.keep = torch.from_numpy(buf).cuda()
            assert self.keep.data_ptr() % 16 == 0
            self.d_text = self.keep.data_ptr() + ts
        else:
            words, npos = adapter_rule.packed_form(text.tobytes())
            ws = 1 if shifted else 0
            wbuf = np.full(ws + max(words.size, 1), 0x5A5A5A5A, dtype=np.uint32)
            wbuf[ws:ws + words.size] = words
            self.keep = torch.from_numpy(wbuf.view(np.int32)).cuda()
            self.d_words = self.keep.data_ptr() + 4 * ws
            self.keep_n = torch.from_numpy(npos.astype(np.int64)).cuda() if npos.size else None
            self.d_npos = self.keep_n.data_ptr() if npos.size else None
            self.n_npos = int(npos.size)
        self.before = self.keep.cpu().numpy().copy()

    def untouched(self):
        return np.array_equal(self.keep.cpu().numpy(), self.before)


def _device_cut(ctx, torch, reads, ranges, form, shifted):
    """one call of the device entry; returns (the five words, the ends behind it, the begins, what lies around the ends)"""
    b = _Bases(torch, reads, form, shifted)
    n = len(reads)
    begin = np.asarray([x for x, _ in ranges], dtype=np.int64)
    ends = np.full(n + 8, -7, dtype=np.int64)  # (stale on both sides)
    ends[4:4 + n] = [y for _, y in ranges]
    d_b, d_e = torch.from_numpy(begin).cuda(), torch.from_numpy(ends).cuda()
    try:
        out = ctx.poly_trim_device(b.d_text, b.d_words, b.d_npos, b.n_npos, b.d_o.data_ptr(), n, b.n_bases, d_b.data_ptr(), d_e.data_ptr() + 32)
    finally:
        torch.cuda.synchronize()
    got = d_e.cpu().numpy()
    assert b.untouched() and np.array_equal(d_b.cpu().numpy(), begin), "the bases or the begins were written"
    return out, got[4:4 + n].tolist(), got[:4].tolist() + got[4 + n:].tolist()


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("form", ["text", "packed"])
def test_the_tail_kernel_equals_the_rule(tmp_path, form, shifted):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)

    def check(batch, letters, min_len, what):
        reads, ranges = batch
        want, info = rule.cut_ranges(reads, ranges, letters, min_len)
        out, ends, pad = _device_cut(ctx, torch, reads, ranges, form, shifted)
        print(what, letters, min_len, "out", out, "expected", info)
        bad = [i for i, ((_, y), e) in enumerate(zip(want, ends)) if y != e]
        assert not bad, (what, len(bad), [(i, len(reads[i]), ranges[i], want[i], ends[i]) for i in bad[:6]])
        assert set(pad) == {-7}, (what, "words around the ends were written")
        assert out == tuple(info[k] for k in POLY_KEYS), (what, out, info)
        return info

    ctx.set_poly_trim("G", M)
    full = rule.kernel_batch()
    info = check(full, "G", M, "ragged")
    assert info["reads_cut"] > 100 and info["reads_emptied"] > 5
    # a second, smaller launch on the same context: nothing of the first one is left behind
    small = ([b"", b"ACTACTACTACT" + b"G" * 11, b"", b"G" * 10, b"ACGT", b"actactgggggnggggg"], [(0, 0), (0, 23), (0, 0), (0, 10), (1, 3), (0, 17)])
    assert check(small, "G", M, "small") == dict(reads_seen=6, bases_seen=52, reads_cut=3, bases_cut=32, reads_emptied=1)
    check(rule.kernel_batch(listed=False), "G", M, "no listed position")
    check(([b"", b"", b""], [(0, 0)] * 3), "G", M, "empty reads only")
    for letters, min_len in (("ACGT", M), ("ca", 2), ("G", 255), ("TG", 16)):  # the maximum over the letters; M at its edges
        ctx.set_poly_trim(letters, min_len)
        check(rule.kernel_batch(long_reads=False), letters, min_len, "letters")
    ctx.set_poly_trim("ACGT", M)
    check(full, "ACGT", M, "ragged, every letter")
    # offsets that do not run to n_bases, and a range outside its read
    d_t = torch.from_numpy(np.full(264, 71, np.uint8)).cuda()
    for offs, begin, end in (([0, 50, 99], [0, 0], [50, 49]), ([0, 50, 100], [0, 0], [50, 51]), ([0, 50, 100], [7, 0], [6, 50]), ([0, 101, 100], [0, 0], [50, 0])):
        d_o = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
        d_b, d_e = torch.from_numpy(np.asarray(begin, dtype=np.int64)).cuda(), torch.from_numpy(np.asarray(end, dtype=np.int64)).cuda()
        with pytest.raises(DependencyError) as e:
            ctx.poly_trim_device(d_t.data_ptr(), None, None, 0, d_o.data_ptr(), 2, 100, d_b.data_ptr(), d_e.data_ptr())
        torch.cuda.synchronize()
        assert e.value.code == EINVAL, offs
    ctx.set_poly_trim("")
    with pytest.raises(DependencyError) as e:
        ctx.poly_trim_device(d_t.data_ptr(), None, None, 0, d_o.data_ptr(), 2, 100, d_b.data_ptr(), d_e.data_ptr())
    assert e.value.code == EINVAL
    ctx.close()


def _device_diff(ctx, torch, reads, form, shifted, want_diff=True):
    b = _Bases(torch, reads, form, shifted)
    n = len(reads)
    d_d = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
    d_f = torch.full((n + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    try:
        out = ctx.complexity_device(b.d_text, b.d_words, b.d_npos, b.n_npos, b.d_o.data_ptr(), n, b.n_bases, d_d.data_ptr() + 16 if want_diff else None,
                                    d_f.data_ptr() + 16)
    finally:
        torch.cuda.synchronize()
    assert b.untouched(), "the bases were written"
    diff, flags = d_d.cpu().numpy(), d_f.cpu().numpy()
    return out, diff[4:4 + n].tolist(), flags[16:16 + n].tolist(), set(diff[:4].tolist() + diff[4 + n:].tolist()), set(flags[:16].tolist() + flags[16 + n:].tolist())


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("form", ["text", "packed"])
def test_the_complexity_kernels_equal_the_rule(tmp_path, form, shifted):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)

    def check(reads, percent, what, want_diff=True):
        D = [rule.differing_pairs_fast(r) for r in reads]
        keep = [0 if rule.dropped(r, percent, d) else 1 for r, d in zip(reads, D)]
        want = (keep.count(0), sum(len(r) for r, k in zip(reads, keep) if not k))
        out, diff, flags, dpad, fpad = _device_diff(ctx, torch, reads, form, shifted, want_diff)
        print(what, percent, "out", out, "expected", want)
        if want_diff:
            bad = [i for i, (a, b) in enumerate(zip(D, diff)) if a != b]
            assert not bad, (what, len(bad), [(i, len(reads[i]), D[i], diff[i]) for i in bad[:6]])
            assert dpad == {-7}, (what, "words around D were written")
        else:
            assert set(diff) | dpad == {-7}
        assert flags == keep and fpad == {0x5A}, (what, [i for i, (a, b) in enumerate(zip(keep, flags)) if a != b][:8])
        assert out == want, (what, out, want)
        return want

    ctx.set_min_complexity(P)
    full = rule.complexity_batch()
    assert check(full, P, "ragged")[0] > 20
    # a second, smaller launch on the same context: nothing of the first one is left behind; D need not be asked for
    small = [b"", b"AA", b"AC", b"", b"NNNN", b"ANNA", b"A" * 10 + b"C" * 10, b"A" * 8 + b"CAC", b"A" * 9 + b"CA", b"g"]
    assert check(small, P, "small", want_diff=False) == (4, 2 + 4 + 20 + 11)
    check(rule.complexity_batch(listed=False), P, "no listed position")
    check([b"", b"", b""], P, "empty reads only")
    for percent in (1, 31, 100):
        ctx.set_min_complexity(percent)
        check(full, percent, "threshold")
    # offsets that do not run from 0 to n_bases
    d_t = torch.from_numpy(np.full(264, 71, np.uint8)).cuda()
    d_f = torch.zeros(8, dtype=torch.uint8, device="cuda")
    for offs in ([1, 50, 100], [0, 50, 99], [0, 101, 100]):
        d_o = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
        with pytest.raises(DependencyError) as e:
            ctx.complexity_device(d_t.data_ptr(), None, None, 0, d_o.data_ptr(), 2, 100, None, d_f.data_ptr())
        torch.cuda.synchronize()
        assert e.value.code == EINVAL, offs
    ctx.set_min_complexity(0)
    with pytest.raises(DependencyError) as e:
        ctx.complexity_device(d_t.data_ptr(), None, None, 0, d_o.data_ptr(), 2, 100, None, d_f.data_ptr())
    assert e.value.code == EINVAL
    ctx.close()


# ---- 2. a cut and judged sample equals the sample of the rules' reads ----------------------------------------------------------------------
_SAMPLES = {}
ADAPTER = adapter_rule.TRUSEQ[:33]


def _poly_counts(ctx):
    return ctx.poly_trim_info()


def _sample(which, oracle, ctx):
    """150-base panel reads (a few of 0 to 8 bases) with G tails, all-G reads, poly-A tails and repeats by turns (rule.tailed_sample), a G
    tail behind an adapter in some, a letter that is no base in every tenth read; the rules' reads (S = {G}, M = 10, then P = 30) and the
    oracle's vectors of them: made once, shared, left unchanged"""
    if which not in _SAMPLES:
        _, genomes = _panel()
        n = 2400 if which == "small" else 9000
        lengths = [150] * n
        rng = np.random.default_rng(81)
        for i in range(3, n, 50):
            lengths[i] = int(rng.integers(0, 9))
        bases, offs = _reads_of(genomes, lengths, seed=82)
        data = bases.tobytes()
        reads, kinds = rule.tailed_sample([data[int(offs[i]):int(offs[i + 1])] for i in range(n)], seed=83)
        for i in range(0, n, 10):
            if lengths[i] > 40:
                r = bytearray(reads[i])
                r[5] = ord("N")
                reads[i] = bytes(r)
        for i in range(7, n, 22):  # read-through into a dark tail: the adapter, then G to the read's end
            if kinds[i] == "plain" and lengths[i] == 150:
                at = int(rng.integers(60, 110))
                reads[i] = (reads[i][:at] + ADAPTER.encode() + b"G" * 150)[:150]
                kinds[i] = "adapter, g tail"
        quals = [np.full(len(r), GOOD, dtype=np.uint8) for r in reads]
        b, o = _flat(reads)
        cut, pinfo = rule.cut(reads, "G", M)
        cinfo, keep = rule.census(cut, [True] * n, P)
        kept = [r for r, k in zip(cut, keep) if k]
        kb, ko = _flat(kept)
        idx = _oracle_index(oracle, ctx.prg_strings, W, K)
        s = dict(reads=reads, kinds=kinds, quals=quals, bases=b, offs=o, cut=cut, pinfo=pinfo, cinfo=cinfo, keep=keep, kept=kept, kbases=kb, koffs=ko,
                 want=_oracle_map(oracle, idx, kb, ko, W, K, True, threads=4), plain=_oracle_map(oracle, idx, b, o, W, K, True, threads=4))
        cb, co = _flat(cut)
        s["want_cut"] = _oracle_map(oracle, idx, cb, co, W, K, True, threads=4)
        # both rules matter: no run that leaves the reads alone, or only cuts, can pass on the counters
        assert pinfo["reads_cut"] > n // 12 and pinfo["reads_emptied"] > n // 15 and cinfo["reads_dropped"] > n // 12
        assert all(k for k, kind, r in zip(keep, kinds, reads) if kind == "plain" and len(r) == 150) and not any(k for k, kind in zip(keep, kinds) if kind == "repeat")
        assert all(len(c) == 0 for c, kind in zip(cut, kinds) if kind == "all g")
        assert int(o[-1]) < 750_000 if which == "small" else int(o[-1]) > 1_300_000
        _SAMPLES[which] = s
    return _SAMPLES[which]


def _filter_identity(ctx):
    f, c, d = ctx.read_filter_info(), ctx.complexity_info(), ctx.decoy_info()
    return f["reads_seen"] == f["dropped_short"] + f["dropped_long"] + f["dropped_low_qual"] + c["reads_dropped"] + d["reads_dropped"] + f["reads_kept"]


def _assert_sample(ctx, s, what, calls=1):
    if calls == 1:
        _assert_oracle(ctx, s["want"], len(s["kept"]), int(s["koffs"][-1]), what)
    assert ctx.poly_trim_info() == {k: calls * v for k, v in s["pinfo"].items()}, (what, ctx.poly_trim_info(), s["pinfo"])
    assert ctx.complexity_info() == {k: calls * v for k, v in s["cinfo"].items()}, (what, ctx.complexity_info(), s["cinfo"])
    f = ctx.read_filter_info()
    assert f["reads_kept"] == calls * len(s["kept"]) and f["bases_kept"] == calls * int(s["koffs"][-1]) and _filter_identity(ctx), (what, f)


def _noqual_bam(path, reads):
    from bam_writer import Rec, write as write_bam
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    recs = [Rec(r.translate(comp)[::-1].decode(), flag=0x10, name=b"r%d" % i, qual=None) if i % 3 == 0 else Rec(r.decode(), flag=4, name=b"r%d" % i, qual=None)
            for i, r in enumerate(reads)]
    return str(write_bam(path, recs))


FORMS = ["fastq ascii", "fastq packed", "fasta", "bam", "bam without qual"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["small", "big"])
def test_a_sample_equals_the_sample_of_the_rules_reads(tmp_path, oracle, which, form):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample(which, oracle, ctx)
    if form == "fasta":
        path = _fasta_reads(tmp_path / "all.fa", s["reads"])
    elif form == "bam without qual":
        path = _noqual_bam(tmp_path / "noqual.bam", s["reads"])
    else:
        path = _file_of(tmp_path, form, s["bases"], s["offs"], s["quals"], "all")
    ctx.set_poly_trim("G", M)
    ctx.set_min_complexity(P)
    for packed in ((True,) if form == "fastq packed" else (False,) if form == "fastq ascii" else (False, True)):
        for threads in (1, 4):
            ctx.reset()
            ctx.set_threads(threads)
            ctx.set_input_format(packed)
            ctx.keep_reads(1 << 28)
            ctx.map_fastx(path)
            _assert_sample(ctx, s, (which, form, packed, threads))
            info = ctx.resident_info()
            assert info["complete"] and (info["blocks"] == 1 if which == "small" else info["blocks"] >= 2), info
            if which == "small" or threads == 1:  # the resident reads are the rules' reads, byte for byte
                rb.assert_resident(ctx, s["kept"], packed or form.startswith("bam"), (form, packed, threads))
    if form == "fastq ascii":
        # the tail cut alone: the oracle on the cut reads; the threshold alone is another run again
        ctx.set_min_complexity(0)
        ctx.reset()
        ctx.map_fastx(path)
        _assert_oracle(ctx, s["want_cut"], len(s["reads"]), sum(len(c) for c in s["cut"]), "the cut alone")
        assert ctx.poly_trim_info() == s["pinfo"] and ctx.complexity_info() == NO_CPLX
        ctx.set_poly_trim("")
        ctx.set_min_complexity(P)
        ctx.reset()
        ctx.map_fastx(path)
        cinfo, keep = rule.census(s["reads"], [True] * len(s["reads"]), P)
        assert ctx.complexity_info() == cinfo and ctx.poly_trim_info() == NO_POLY and cinfo != s["cinfo"]
        # a context given the file of the rules' reads alone, with nothing set; and both settings off on the sample: the plain reads' vectors
        ctx.set_min_complexity(0)
        ctx.reset()
        ctx.map_fastx(_write_fastq(tmp_path / "kept.fq", s["kbases"], s["koffs"], [np.full(len(r), GOOD, np.uint8) for r in s["kept"]]))
        _assert_oracle(ctx, s["want"], len(s["kept"]), int(s["koffs"][-1]), "the file of the rules' reads")
        ctx.reset()
        ctx.map_fastx(path)
        _assert_oracle(ctx, s["plain"], len(s["reads"]), int(s["offs"][-1]), "nothing set")
        assert ctx.poly_trim_info() == NO_POLY and ctx.complexity_info() == NO_CPLX
    ctx.close()


# ---- 3. order and interplay ---------------------------------------------------------------------------------------------------------------
def test_the_stages_run_in_the_stated_order(tmp_path, oracle):
    """--trim-tail, --adapter, --poly-tail, --mask-qual, --min-read-len, --min-complexity, --decoy and --dedup together: the run is the oracle's
    on crop-rule, then adapter-rule, then tail-rule, then mask-rule reads, of which the length test, then the threshold, then the screen keep
    theirs, of which dedup keeps the first copies"""
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    rng = np.random.default_rng(84)
    TAIL, MIN_LEN, Q, DK = 3, 60, mask_qual_rule.Q, 31
    decoy = decoy_rule.random_dna(np.random.default_rng(85), 6000)
    reads, quals = list(s["reads"][:1500]), [q.copy() for q in s["quals"][:1500]]
    for j in range(30):  # decoy reads; every third with a G tail in front of which a decoy part stays
        r = decoy[150 * j:150 * j + 150]
        reads.append(r[:90] + b"G" * 60 if j % 3 == 0 else r)
        quals.append(np.full(150, GOOD, dtype=np.uint8))
    for i in range(5, 1500, 17):  # a masked stretch: most of the read unknown, which the threshold then drops; or a few bases
        if len(reads[i]) == 150:
            quals[i][10:140 if i % 2 else 30] = 3
    for i in range(11, 1500, 40):  # low qualities in a G tail do not hide it: it is cut in front of the mask
        quals[i][-30:] = 2
    reads += [reads[20], reads[31], reads[44]]  # copies (of reads that stay)
    quals += [quals[20].copy(), quals[31].copy(), quals[44].copy()]
    n = len(reads)
    ranges = [(0, max(len(r) - TAIL, 0)) for r in reads]
    ranges, ainfo = adapter_rule.cut_ranges(reads, ranges, [ADAPTER], 100, 3)
    ranges, pinfo = rule.cut_ranges(reads, ranges, "G", M)
    left = [r[a:b] for r, (a, b) in zip(reads, ranges)]
    lq = [q[a:b] for q, (a, b) in zip(quals, ranges)]
    masked = [mask_qual_rule.masked(r, q, Q) for r, q in zip(left, lq)]
    long_enough = [len(r) >= MIN_LEN for r in masked]
    cinfo, keep = rule.census(masked, long_enough, P)
    D = decoy_rule.decoy_set([decoy], DK)
    dinfo, keep = decoy_rule.census(masked, keep, D, DK)
    kept = [r for r, k in zip(masked, keep) if k]
    flags = keep_flags_fast(kept)
    final = [r for r, f in zip(kept, flags) if f]
    assert ainfo["reads_cut"] > 20 and pinfo["reads_cut"] > 100 and cinfo["reads_dropped"] > 60 and 15 < dinfo["reads_dropped"] <= 30
    assert sum(flags) <= len(kept) - 3 and long_enough.count(False) > 100
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    fb, fo = _flat(final)
    want = _oracle_map(oracle, idx, fb, fo, W, K, True, threads=4)
    b, o = _flat(reads)
    ctx.set_read_trim(tail=TAIL)
    ctx.set_adapters([ADAPTER])
    ctx.set_poly_trim("G", M)
    ctx.set_base_mask(Q)
    ctx.set_read_filter(min_len=MIN_LEN)
    ctx.set_min_complexity(P)
    ctx.set_decoy([_fasta(tmp_path / "decoy.fa", [decoy])], k=DK)
    for form in ("fastq ascii", "fastq packed", "bam"):
        ctx.reset()
        ctx.set_threads(2)
        ctx.set_input_format(form == "fastq packed")
        ctx.set_ordered_ingest(True)
        ctx.keep_reads(1 << 28)
        ctx.map_fastx(_file_of(tmp_path, form, b, o, quals, "stages"))
        assert ctx.adapter_trim_info() == ainfo, form
        assert ctx.poly_trim_info() == pinfo, (form, ctx.poly_trim_info(), pinfo)
        assert ctx.base_mask_info() == mask_qual_rule.info(left, lq, Q), form
        assert ctx.complexity_info() == cinfo, (form, ctx.complexity_info(), cinfo)
        got = ctx.decoy_info()
        assert {k: got[k] for k in dinfo} == dinfo, (form, got, dinfo)
        f = ctx.read_filter_info()
        assert f["dropped_short"] == long_enough.count(False) and f["reads_kept"] == len(kept) and f["reads_seen"] == n and _filter_identity(ctx), (form, f)
        rb.assert_resident(ctx, kept, form != "fastq ascii", ("behind every stage", form))
        out = ctx.dedup()
        assert out["reads_before"] == len(kept) and out["reads_kept"] == len(final), (form, out)
        _assert_oracle(ctx, want, len(final), int(fo[-1]), form)
    ctx.close()


def test_a_subsample_counts_the_cut_reads(tmp_path, oracle):
    """--subsample-covg beside the new flags: the target is met by the bases the rules left, not by the file's"""
    from subsample_rule import keep_flags
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    ctx.set_poly_trim("G", M)
    ctx.set_min_complexity(P)
    ctx.set_ordered_ingest(True)
    ctx.keep_reads(1 << 28)
    ctx.map_fastx(_write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"]))
    target = int(s["koffs"][-1]) // 2
    out = ctx.subsample(target, seed=7)
    flags = keep_flags([len(r) for r in s["kept"]], target, 7)
    assert out["reads_before"] == len(s["kept"]) and out["bases_before"] == int(s["koffs"][-1]), out
    assert out["reads_kept"] == sum(flags) and ctx.subsample_flags(len(s["kept"])).tolist() == [int(f) for f in flags]
    ctx.close()


# ---- 4. refusals and state -----------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(tmp_path, oracle):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    ctx.set_threads(2)
    for letters, min_len in (("GX", 10), ("GG", 10), ("Gg", 10), ("N", 10), ("G ", 10), ("G", 1), ("G", 0), ("G", 256), ("ACGTA", 10)):
        with pytest.raises(DependencyError) as e:
            ctx.set_poly_trim(letters, min_len)
        assert e.value.code == EINVAL, (letters, min_len)
    for bad in (101, 1000):
        with pytest.raises(DependencyError) as e:
            ctx.set_min_complexity(bad)
        assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        ctx.set_min_complexity(12.5)
    with pytest.raises(ValueError):
        ctx.set_poly_trim("G", 10.5)
    ctx.map_fastx(fq)  # the refusals left nothing set: the plain reads' vectors, as before the settings existed
    _assert_oracle(ctx, s["plain"], len(s["reads"]), int(s["offs"][-1]), "nothing set")
    assert ctx.poly_trim_info() == NO_POLY and ctx.complexity_info() == NO_CPLX
    # map_host and map_device are refused while either is set, and served again once both are off
    kb, ko = s["kbases"], s["koffs"]
    d_b, d_o = torch.from_numpy(kb.copy()).cuda(), torch.from_numpy(ko.astype(np.int64)).cuda()
    calls = (lambda: ctx.map_host(kb, ko), lambda: ctx.map_device(d_b.data_ptr(), d_o.data_ptr(), len(s["kept"]), int(ko[-1])))
    for setting, named in ((lambda on: ctx.set_poly_trim("g" if on else "", 12), "drprg_hip_set_poly_trim"), (lambda on: ctx.set_min_complexity(P if on else 0),
                                                                                                               "drprg_hip_set_min_complexity")):
        setting(True)
        ctx.reset()
        for call in calls:
            with pytest.raises(DependencyError) as e:
                call()
            assert e.value.code == EINVAL and named in str(e.value), str(e.value)
        assert ctx.counters()["reads"] == 0
        setting(False)
    for call in calls:
        ctx.reset()
        call()
        torch.cuda.synchronize()
        _assert_oracle(ctx, s["want"], len(s["kept"]), int(ko[-1]), "both off")
    # a cut or a drop, no resident reads, discover: -61, naming the flag
    (tmp_path / "disc").mkdir()
    for setting, flag in ((lambda: ctx.set_poly_trim("G", M), "--poly-tail"), (lambda: ctx.set_min_complexity(P), "--min-complexity")):
        ctx.set_poly_trim("")
        ctx.set_min_complexity(0)
        setting()
        ctx.reset()
        ctx.map_fastx(fq)
        with pytest.raises(DependencyError) as e:
            ctx.discover_reads(fq, str(tmp_path / "genes.fa"), str(tmp_path / "disc"))
        assert e.value.code == ENODATA and flag in str(e.value), str(e.value)
    # a second call adds to the counts; a reset clears them and keeps the settings
    ctx.set_poly_trim("G", M)
    ctx.reset()
    ctx.map_fastx(fq)
    _assert_sample(ctx, s, "one call")
    ctx.map_fastx(fq)
    _assert_sample(ctx, s, "two calls", calls=2)
    ctx.reset()
    assert ctx.poly_trim_info() == NO_POLY and ctx.complexity_info() == NO_CPLX
    ctx.map_fastx(fq)
    _assert_sample(ctx, s, "after a reset")
    # reads of no bases only: seen by the cut, judged and kept by the threshold
    ctx.reset()
    ctx.map_fastx(_fasta_reads(tmp_path / "empty.fa", [b"", b"", b""]))
    assert ctx.poly_trim_info() == dict(NO_POLY, reads_seen=3) and ctx.complexity_info() == dict(NO_CPLX, reads_seen=3) and ctx.read_filter_info()["reads_kept"] == 3
    # every read emptied by the cut
    ctx.reset()
    ctx.map_fastx(_fasta_reads(tmp_path / "dark.fa", [b"G" * 150] * 5))
    assert ctx.poly_trim_info() == dict(reads_seen=5, bases_seen=750, reads_cut=5, bases_cut=750, reads_emptied=5)
    assert ctx.read_filter_info()["reads_kept"] == 5 and ctx.counters()["bases"] == 0
    ctx.close()


def test_one_device_listed_twice_gives_the_vectors_of_one(tmp_path, oracle):
    """the settings reach every device's blocks: the same context over device 0 twice"""
    from drprg_amd import Context
    panel, _ = _panel()
    one = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, one)
    one.close()
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=[0, 0])
    multi.set_opts(illumina=True, genome_size=G)
    multi.set_threads(4)
    multi.set_poly_trim("G", M)
    multi.set_min_complexity(P)
    multi.map_fastx(_write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"]))
    _assert_sample(multi, s, "device 0 twice")
    multi.close()


def test_two_devices_give_the_vectors_of_one(tmp_path, oracle):
    import os
    from drprg_amd import Context
    if not os.environ.get("DRPRG_HIP_DEVICES"):
        pytest.skip("DRPRG_HIP_DEVICES is not set")
    devices = [int(x) for x in os.environ["DRPRG_HIP_DEVICES"].split(",")]
    if len(devices) < 2:
        pytest.skip("one device")
    panel, _ = _panel()
    one = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, one)
    one.close()
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=devices)
    multi.set_opts(illumina=True, genome_size=G)
    multi.set_threads(4)
    multi.set_poly_trim("G", M)
    multi.set_min_complexity(P)
    multi.map_fastx(_write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"]))
    _assert_sample(multi, s, "devices")
    multi.close()


# ---- 5. the executables ---------------------------------------------------------------------------------------------------------------------
def _verbose_lines(s):
    p, c = s["pinfo"], s["cinfo"]
    return ("poly tail trimming: " + " ".join(f"{k}={p[k]}" for k in POLY_KEYS),
            "complexity filter: " + " ".join(f"{k}={c[k]}" for k in ("reads_seen", "bases_seen", "reads_dropped", "bases_dropped")))


def test_pandora_map_writes_the_vcf_of_the_rules_reads(tmp_path, oracle):
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
    kept = _write_fastq(tmp_path / "kept.fq", s["kbases"], s["koffs"], [np.full(len(r), GOOD, np.uint8) for r in s["kept"]])

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

    run(tmp_path / "plain", kept, [])
    want = vcf_without_date(str(tmp_path / "plain" / "pandora_genotyped.vcf"))
    flags = ["--poly-tail", "G", "--min-complexity", str(P)]
    for name, reads in (("cut_fq", fq), ("cut_bam", bam)):
        stdout = run(tmp_path / name, reads, flags)
        assert vcf_without_date(str(tmp_path / name / "pandora_genotyped.vcf")) == want, name
        for line in _verbose_lines(s):
            assert line in stdout, (line, stdout)
    stdout = run(tmp_path / "uncut", fq, [])
    assert "poly tail trimming:" not in stdout and "complexity filter:" not in stdout
    # the coverage discover left under one setting is taken by a map under the same settings only
    out = tmp_path / "handover"
    run(out / "discover", fq, flags, cmd="discover")
    for extra, reused in ((flags, True), (["--poly-tail", "G", "--poly-min-len", "10", "--min-complexity", str(P)], True), (["--poly-tail", "G"], False),
                          (["--poly-tail", "GA", "--min-complexity", str(P)], False), (["--poly-tail", "G", "--poly-min-len", "11", "--min-complexity", str(P)], False),
                          (["--poly-tail", "G", "--min-complexity", str(P + 1)], False), ([], False)):
        assert ("no second mapping pass" in run(out, fq, extra)) == reused, extra


def test_drprg_predict_cuts_and_judges_once_through_a_prg_update(tmp_path):
    """an off-panel variant: discover finds it in the resident (cut and judged) reads, the PRG is updated and the reads are mapped again from
    device memory -- cut already, not cut twice: the run equals that of the file of the rules' reads, and the counts are those of the one pass"""
    import json
    import os
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
    reads, _ = rule.tailed_sample([block[i].tobytes() for i in range(len(starts))], seed=8)
    cut, pinfo = rule.cut(reads, "G", M)
    cinfo, keep = rule.census(cut, [True] * len(cut), P)
    kept = [r for r, k in zip(cut, keep) if k]
    assert pinfo["reads_cut"] > 2000 and cinfo["reads_dropped"] > 1000
    b, o = _flat(reads)
    kb, ko = _flat(kept)
    fq = _write_fastq(tmp_path / "novel.fq", b, o, [np.full(150, GOOD, np.uint8)] * len(reads))
    rules_fq = _write_fastq(tmp_path / "rules.fq", kb, ko, [np.full(len(r), GOOD, np.uint8) for r in kept])

    def run(out, path, extra):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", path, "-o", str(out), "-s", "novel", "-I", "-v"] + extra
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        calls = json.load(open(out / "novel.drprg.json"))["susceptibility"]
        for drug in calls.values():
            for ev in drug["evidence"]:
                ev.pop("vcfid")
        return r.stderr, (open(out / "pandora_genotyped.vcf").read(), calls, open(out / "discover" / "denovo_variants.tsv").read())

    err, got = run(tmp_path / "cut", fq, ["--poly-tail", "G", "--min-complexity", str(P)])
    _, want = run(tmp_path / "rules", rules_fq, [])
    assert got == want
    assert "novel site(s) added" in err and "reads mapped again (resident in device memory)" in err, err
    for line in _verbose_lines(dict(pinfo=pinfo, cinfo=cinfo)):
        assert err.count(line) == 1, (line, err)
    assert err.count("poly tail trimming:") == 1 and err.count("complexity filter:") == 1, err
    assert any(e["gene"] == "katG" for v in got[1].values() for e in v["evidence"])


def test_the_tail_is_cut_behind_both_adapter_sides(tmp_path, oracle):
    """--trim-tail, --adapter and --front-adapter under the indel rule, then --poly-tail and --min-complexity: the run is the oracle's on
    crop-rule, then 3' and 5' adapter-rule, then tail-rule reads of which the threshold keeps its share.  A read whose 5' adapter is
    followed by nothing but G is cut at both ends to nothing"""
    from adapter_edit_rule import FRONT, cut_ranges_many
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    FRONT_ADAPTER, E, TAIL = FRONT[-28:], "0.1", 2
    reads = list(s["reads"][:900])
    for i in range(4, 900, 9):  # a 5' adapter in place of the read's start; in every fourth of them G from there to the end
        if len(reads[i]) == 150:
            reads[i] = FRONT_ADAPTER.encode() + (b"G" * 122 if i % 4 == 0 else reads[i][28:])
    n = len(reads)
    ranges = [(0, max(len(r) - TAIL, 0)) for r in reads]
    ranges, i3, i5 = cut_ranges_many(reads, ranges, [ADAPTER], [FRONT_ADAPTER], 100, 3)
    ranges, pinfo = rule.cut_ranges(reads, ranges, "G", M)
    left = [r[a:b] for r, (a, b) in zip(reads, ranges)]
    cinfo, keep = rule.census(left, [True] * n, P)
    kept = [r for r, k in zip(left, keep) if k]
    assert i3["reads_cut"] > 10 and i5["reads_cut"] > 80 and pinfo["reads_cut"] > 60 and pinfo["reads_emptied"] > 20 and cinfo["reads_dropped"] > 30
    assert pinfo["bases_seen"] == i5["bases_seen"] - i5["bases_cut"]  # the cut sees what both adapter sides left
    kb, ko = _flat(kept)
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    b, o = _flat(reads)
    ctx.set_read_trim(tail=TAIL)
    ctx.set_adapters([ADAPTER], front=[FRONT_ADAPTER], indels=True, error=E)
    ctx.set_poly_trim("G", M)
    ctx.set_min_complexity(P)
    for form in ("fastq ascii", "fastq packed", "bam"):
        ctx.reset()
        ctx.set_threads(2)
        ctx.set_input_format(form == "fastq packed")
        ctx.keep_reads(1 << 28)
        ctx.map_fastx(_file_of(tmp_path, form, b, o, [np.full(len(r), GOOD, np.uint8) for r in reads], "both_sides"))
        assert ctx.adapter_trim_info() == i3 and ctx.front_adapter_info() == i5, form
        assert ctx.poly_trim_info() == pinfo, (form, ctx.poly_trim_info(), pinfo)
        assert ctx.complexity_info() == cinfo and _filter_identity(ctx), (form, ctx.complexity_info(), cinfo)
        _assert_oracle(ctx, want, len(kept), int(ko[-1]), form)
        rb.assert_resident(ctx, kept, form != "fastq ascii", ("behind both sides", form))
    ctx.close()
