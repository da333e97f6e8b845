"""Adapter trimming (drprg_hip_set_adapters, csrc/adapter_trim.hip; pytest -m gpu).  Cut points and counts come from the rule in plain Python
(tests/adapter_rule.py), the vectors and counters from the oracle on the reads the rule leaves -- never from the code under test.

How the blocks come about: the ingest hands a worker's first block over at 750 000 bases, so the small sample (under that) is one block
and the big one several, whatever the number of parser threads."""
import json
import os
import subprocess

import numpy as np
import pytest

import adapter_rule as rule
import read_trim_rule as rtrim
import resident_readback as rb
from adapter_rule import NEXTERA, TRUSEQ, cut_ranges, kernel_batch
from max_covg_rule import accepted_reads
from subsample_rule import keep_flags
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from test_gpu_read_filter import _assert_oracle, _file_of, _write_bam, _write_fastq
from util import vcf_without_date

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
EINVAL, ENODATA = 22, 61
ADAPTER = TRUSEQ[:33]
E, O = "0.1", 3  # the defaults
NO_TRIM = dict(reads_seen=0, bases_seen=0, reads_lost_base=0, cut_front=0, cut_tail=0, qual_cut_front=0, qual_cut_tail=0, reads_emptied=0)
NO_CUT = dict(reads_seen=0, bases_seen=0, reads_cut=0, bases_cut=0, reads_emptied=0)
INFO_KEYS = ("reads_seen", "bases_seen", "reads_cut", "bases_cut", "reads_emptied")


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _flat(reads):
    o = np.zeros(len(reads) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), o


def _cut(reads, ranges):
    return [r[a:b] for r, (a, b) in zip(reads, ranges)]


def _filter_counts(ctx):
    info = ctx.read_filter_info()
    info.pop("T")
    return info


def _fasta(path, reads):
    with open(path, "wb") as fh:
        for i, r in enumerate(reads):
            fh.write(b">r%d\n" % i + r + b"\n")
    return str(path)


_SAMPLES = {}


def _sample(which, oracle, ctx):
    """the sample's reads with adapters planted, the rule's cuts, and the oracle's vectors of the cut reads: made once, shared, left unchanged"""
    if which not in _SAMPLES:
        _, genomes = _panel()
        lengths, _ = rtrim.small_sample() if which == "small" else rtrim.big_sample()
        bases, offs = _reads_of(genomes, lengths, seed=61)
        reads, kinds = rule.plant(bases, offs, ADAPTER, O, seed=62)
        for i in range(0, len(reads), 10):  # a base that is not ACGT in every tenth read: packed blocks list positions
            if len(reads[i]) > 40:
                reads[i] = reads[i][:7] + b"N" + reads[i][8:]
        ranges, info = cut_ranges(reads, [(0, len(r)) for r in reads], [ADAPTER], rule.error_milli(E), O)
        n = {k: kinds.count(k) for k in ("through", "partial", "none")}
        cut = [rg != (0, len(r)) for r, rg in zip(reads, ranges)]
        # a third of the reads each way (reads under 40 bases carry none); every planted adapter is found, and next to no other
        assert abs(n["through"] - n["partial"]) <= 12 and n["through"] > len(reads) // 4 and n["none"] > len(reads) // 4, n
        for kind in n:  # every kind among the records the BAM form stores on the reverse strand
            assert sum(k == kind and rtrim.reverse_flag(i) for i, k in enumerate(kinds)) > len(reads) // 16, kind
        assert all(c for c, k in zip(cut, kinds) if k != "none") and sum(c for c, k in zip(cut, kinds) if k == "none") < n["none"] // 5
        kept = _cut(reads, ranges)
        kb, ko = _flat(kept)
        b, o = _flat(reads)
        s = dict(reads=reads, bases=b, offs=o, quals=[np.full(len(r), 30, dtype=np.uint8) for r in reads], ranges=ranges, info=info, kept=kept, kbases=kb, koffs=ko,
                 klengths=[len(r) for r in kept])
        s["want"] = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
        assert s["want"][2]["clusters_kept"] > 5
        _SAMPLES[which] = s
    return _SAMPLES[which]


def _assert_cut(ctx, s, what):
    n, nb = len(s["reads"]), int(s["koffs"][-1])
    _assert_oracle(ctx, s["want"], n, nb, what)
    assert ctx.adapter_trim_info() == s["info"], what
    assert ctx.read_trim_info() == NO_TRIM, what
    assert _filter_counts(ctx) == dict(reads_seen=n, bases_seen=nb, dropped_short=0, dropped_long=0, dropped_low_qual=0, reads_kept=n, bases_kept=nb), what


# ---- 1. the kernels against the rule ----------------------------------------------------------------------------------------------------
_BATCHES = {}


def _batch(name, err):
    if (name, err) not in _BATCHES:
        b = kernel_batch(name, err)
        b["census"] = rule.census(b)  # (raises when a class is not what it is meant to be: no case passes empty)
        b["want"], b["info"] = cut_ranges(b["reads"], b["ranges"], b["adapters"], b["e"], b["O"])
        _BATCHES[(name, err)] = b
    return _BATCHES[(name, err)]


def _device_cut(ctx, torch, reads, ranges, form):
    text, offs = _flat(reads)
    n_reads, n_bases = len(reads), int(offs[-1])
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_b = torch.from_numpy(np.array([a for a, _ in ranges], dtype=np.int64)).cuda()
    d_e = torch.from_numpy(np.array([b for _, b in ranges], dtype=np.int64)).cuda()
    if form == "packed":
        words, npos = rule.packed_form(text.tobytes())
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_n = torch.from_numpy(npos.astype(np.int64)).cuda() if npos.size else None
        out = ctx.adapter_trim_device(None, d_w.data_ptr(), d_n.data_ptr() if npos.size else None, int(npos.size), d_o.data_ptr(), n_reads, n_bases, d_b.data_ptr(),
                                      d_e.data_ptr())
    else:
        shift = 1 if form == "text off by one" else 0
        buf = np.zeros(n_bases + (1 if shift else 64), dtype=np.uint8)  # (one byte off: read byte by byte, and the buffer ends with its last base)
        buf[shift:shift + n_bases] = text
        d_t = torch.from_numpy(buf).cuda()
        assert d_t.data_ptr() % 16 == 0
        out = ctx.adapter_trim_device(d_t.data_ptr() + shift, None, None, 0, d_o.data_ptr(), n_reads, n_bases, d_b.data_ptr(), d_e.data_ptr())
    torch.cuda.synchronize()
    return out, list(zip(d_b.cpu().numpy().tolist(), d_e.cpu().numpy().tolist()))


@pytest.mark.parametrize("form", ["text", "text off by one", "packed"])
@pytest.mark.parametrize("err", ["0", "0.1", "0.2"])
@pytest.mark.parametrize("name", ["12", "16", "17", "33", "64", "33+19"])
def test_the_kernels_equal_the_rule(tmp_path, name, err, form):
    import torch
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    b = _batch(name, err)
    ctx.set_adapters(b["adapters"], error=err)
    out, got = _device_cut(ctx, torch, b["reads"], b["ranges"], form)
    diff = [i for i in range(len(got)) if got[i] != b["want"][i]]
    where = {i: cls for cls, (idx, _) in b["classes"].items() if cls != "partial lengths" for i in idx}
    assert not diff, [(i, where.get(i), len(b["reads"][i]), b["ranges"][i], got[i], b["want"][i]) for i in diff[:8]]
    assert dict(zip(INFO_KEYS, out)) == b["info"], out
    # the census of the classes, on what came back: a cut in every read of a class meant to cut, none in a class meant not to
    for cls, (idx, kind) in b["classes"].items():
        if cls == "partial lengths":
            continue
        n_cut = sum(got[i] != b["ranges"][i] for i in idx)
        assert (n_cut, len(idx) - n_cut) == b["census"][cls] and (kind != "cut" or n_cut == len(idx) > 0) and (kind != "none" or n_cut == 0 < len(idx)), (cls, n_cut)
    (i,) = b["classes"]["the adapter itself"][0]
    assert got[i] == (0, 0) and b["info"]["reads_emptied"] >= 1
    # a second, smaller launch on the same context: nothing of the first one is left behind
    A = b["adapters"][0].encode()
    small = [b"", b"ACGTTGCAAGGCTTAACCGGATATCG" + A, b"", b"TTTTTTTTTTTTTTT", A, b"TTGACCA" + A[:5]]
    rg = [(0, len(r)) for r in small]
    want2, info2 = cut_ranges(small, rg, b["adapters"], b["e"], b["O"])
    assert want2[1] == (0, 26) and want2[4] == (0, 0) and want2[5] == (0, 7) and want2[3] == (0, 15)
    out, got = _device_cut(ctx, torch, small, rg, form)
    assert got == want2 and dict(zip(INFO_KEYS, out)) == info2
    ctx.close()


# ---- 2. a sample with adapters equals the sample of its cut reads --------------------------------------------------------------------------
FORMS = ["fastq ascii", "fastq packed", "bam", "fastq.gz", "fasta"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["small", "big"])
def test_a_sample_with_adapters_equals_the_sample_of_its_cut_reads(tmp_path, oracle, which, form):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample(which, oracle, ctx)
    path = _fasta(tmp_path / "all.fa", s["reads"]) if form == "fasta" else _file_of(tmp_path, form, s["bases"], s["offs"], s["quals"], "all")
    for packed in ((True,) if form == "fastq packed" else (False,) if form == "fastq ascii" else (False, True)):
        ctx.reset()
        ctx.set_threads(1 if which == "small" else 4)
        ctx.set_input_format(packed)
        ctx.keep_reads(1 << 28)
        ctx.set_adapters([ADAPTER], error=E)
        ctx.map_fastx(path)
        _assert_cut(ctx, s, (which, form, packed))
        info = ctx.resident_info()
        assert info["complete"] and (info["blocks"] == 1 if which == "small" else info["blocks"] >= 2), info
        if which == "small":  # the resident block is the cut block
            rb.assert_resident(ctx, s["kept"], packed or form == "bam", (form, packed))
    ctx.close()


# ---- 3. order, and what lies behind it ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fastq ascii", "fastq packed", "bam"])
def test_the_adapter_is_sought_in_what_crops_and_quality_left(tmp_path, oracle, form):
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    reads = list(s["reads"])
    body, _ = _reads_of(genomes, [100, 100], seed=63)
    body = body.tobytes()
    reads += [body[:100] + ADAPTER[:8].encode(), body[100:] + ADAPTER[:5].encode()]  # behind a tail crop of 3: five letters are a partial match, two are none
    quals = []
    for i, r in enumerate(reads):
        q = np.full(len(r), 30, dtype=np.uint8)
        if i % 4 == 0 and i < len(reads) - 2:
            q[-10:] = 5  # a junk tail: where the adapter's end lies in a third of them
        quals.append(q)
    FRONT, TAIL, QUAL = 5, 3, 20
    ranges = [rtrim.kept_range(q, len(r), FRONT, TAIL, rtrim.qual_milli(QUAL), 4) for r, q in zip(reads, quals)]
    cut, info = cut_ranges(reads, ranges, [ADAPTER], rule.error_milli(E), O)
    assert ranges[-2] == (5, 105) and cut[-2] == (5, 100) and ranges[-1] == cut[-1] == (5, 102)
    both = sum(1 for r, rg, c in zip(reads, ranges, cut) if rg != (0, len(r)) and c != rg and rg[1] < len(r) - TAIL)
    assert both > 20 and info["reads_cut"] > len(reads) // 2  # reads that lost bases to the quality trim AND to the adapter
    kb, ko = _flat(_cut(reads, cut))
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    b, o = _flat(reads)
    ctx.set_threads(2)
    ctx.set_input_format(form == "fastq packed")
    ctx.set_read_trim(front=FRONT, tail=TAIL, qual=QUAL)
    ctx.set_adapters([ADAPTER], error=E)
    ctx.map_fastx(_file_of(tmp_path, form, b, o, quals, "order"))
    _assert_oracle(ctx, want, len(reads), int(ko[-1]), form)
    assert ctx.read_trim_info() == rtrim.info([len(r) for r in reads], ranges, FRONT, TAIL)  # crops and quality alone, as without adapters
    assert ctx.adapter_trim_info() == info
    ctx.close()


def test_filter_cap_and_subsample_see_cut_reads(tmp_path, oracle):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, ctx)
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    ctx.set_threads(4)
    ctx.keep_reads(1 << 28)
    ctx.set_adapters([ADAPTER], error=E)
    # the length bound is that of the cut read
    MIN_LEN = 150
    keep = [L >= MIN_LEN for L in s["klengths"]]
    assert sum(len(r) >= MIN_LEN > L for r, L in zip(s["reads"], s["klengths"])) > 20  # long enough only with their adapter
    fb, fo = _flat([r for r, k in zip(s["kept"], keep) if k])
    want = _oracle_map(oracle, idx, fb, fo, W, K, True, threads=4)
    for packed in (False, True):
        ctx.reset()
        ctx.set_input_format(packed)
        ctx.set_read_filter(min_len=MIN_LEN)
        ctx.map_fastx(fq)
        _assert_oracle(ctx, want, sum(keep), int(fo[-1]), ("filter", packed))
        assert _filter_counts(ctx) == dict(reads_seen=len(keep), bases_seen=int(s["koffs"][-1]), dropped_short=len(keep) - sum(keep), dropped_long=0, dropped_low_qual=0,
                                           reads_kept=sum(keep), bases_kept=int(fo[-1]))
        assert ctx.adapter_trim_info() == s["info"]
    ctx.set_read_filter()
    # the cap cuts on the cut reads' running total: in the first block, and in a later one
    for max_covg, packed in ((3, True), (99, False)):
        n, n_bases, reached = accepted_reads(s["klengths"], G, max_covg)
        assert reached and 0 < n < len(s["klengths"]) and (max_covg == 3 or n_bases > 800_000)
        want = _oracle_map(oracle, idx, s["kbases"][:n_bases], s["koffs"][:n + 1], W, K, True, threads=4)
        ctx.reset()
        ctx.set_input_format(packed)
        ctx.set_max_covg(max_covg)
        ctx.map_fastx(fq)
        info = ctx.max_covg_info()
        assert info["reached"] and info["reads"] == n and info["bases"] == n_bases, (max_covg, info)
        _assert_oracle(ctx, want, n, n_bases, ("cap", max_covg, packed))
    ctx.set_max_covg(None)
    # the subsample numbers the cut reads and aims at their bases
    ctx.reset()
    ctx.set_ordered_ingest(True)
    ctx.map_fastx(fq)
    total = int(s["koffs"][-1])
    flags = keep_flags(s["klengths"], total // 2, 9)
    out = ctx.subsample(total // 2, 9)
    assert out["reads_before"] == len(flags) and out["bases_before"] == total and out["reads_kept"] == sum(flags)
    assert ctx.subsample_flags(len(flags)).tolist() == flags
    ctx.close()


def test_dedup_sees_cut_reads(tmp_path, oracle):
    """two reads that are identical once the adapter and what follows it are gone, and different before: one is dropped"""
    from dedup_rule import keep_flags_fast
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    n, L = 150, 160
    half, offs1 = _reads_of(genomes, [L] * n, seed=64)
    rng = np.random.default_rng(65)
    tails = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(1, 30)))) for _ in range(2 * n)]
    reads = [half[i % n * L:(i % n + 1) * L].tobytes() + ADAPTER.encode() + tails[i] for i in range(2 * n)]  # the copy read further into other bases
    ranges, info = cut_ranges(reads, [(0, len(r)) for r in reads], [ADAPTER], rule.error_milli(E), O)
    kept = _cut(reads, ranges)
    n_before, flags = sum(keep_flags_fast(reads)), keep_flags_fast(kept)
    assert n_before >= 2 * n - 10 and sum(flags) == n_before - n and not any(flags[n:]) and info["reads_cut"] == 2 * n
    fb, fo = _flat([r for r, f in zip(kept, flags) if f])
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), fb, fo, W, K, True)
    b, o = _flat(reads)
    fq = _write_fastq(tmp_path / "dup.fq", b, o, [np.full(len(r), 30, dtype=np.uint8) for r in reads])
    ctx.set_threads(1)
    ctx.set_ordered_ingest(True)
    ctx.keep_reads(1 << 28)
    for packed in (True, False):
        ctx.set_input_format(packed)
        ctx.reset()
        ctx.set_adapters([])
        ctx.map_fastx(fq)
        assert ctx.dedup()["reads_kept"] == n_before
        ctx.reset()
        ctx.set_adapters([ADAPTER], error=E)
        ctx.map_fastx(fq)
        out = ctx.dedup()
        assert out == dict(reads_before=2 * n, bases_before=sum(len(r) for r in kept), reads_kept=sum(flags), bases_kept=int(fo[-1])), out
        _assert_oracle(ctx, want, sum(flags), int(fo[-1]), ("dedup", packed))
    ctx.close()


def test_a_middle_block_that_the_adapter_empties(tmp_path, oracle):
    """three blocks of one file, the middle one of reads that begin with the adapter: the block that maps nothing must not disturb its
    neighbours.  The ingest hands the first block over at 786 432 bases and the next at 12 582 912: the reads are sized to fill them exactly."""
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    lengths = [384] * 2048 + [8192] * 1536 + [384] * 512
    bases, offs = _reads_of(genomes, lengths, seed=66)
    bases = bases.copy()
    a = np.frombuffer(ADAPTER.encode(), dtype=np.uint8)
    for i, L in enumerate(lengths):
        if L == 8192:
            bases[int(offs[i]):int(offs[i]) + a.size] = a
    reads = [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(lengths))]
    ranges, info = cut_ranges(reads, [(0, len(r)) for r in reads], [ADAPTER], rule.error_milli(E), O)
    assert info["reads_emptied"] == 1536 and all(rg == (0, 0) for rg, L in zip(ranges, lengths) if L == 8192)
    kb, ko = _flat(_cut(reads, ranges))
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    fq = _write_fastq(tmp_path / "three.fq", bases, offs, [np.full(L, 30, dtype=np.uint8) for L in lengths])
    ctx.set_threads(4)
    ctx.set_adapters([ADAPTER], error=E)
    for packed in (True, False):
        for keep_bytes in (0, 1 << 28):
            ctx.reset()
            ctx.set_input_format(packed)
            ctx.keep_reads(keep_bytes)
            ctx.map_fastx(fq)
            _assert_oracle(ctx, want, len(lengths), int(ko[-1]), (packed, keep_bytes))  # (the emptied reads stay reads)
            assert ctx.adapter_trim_info() == info
            if keep_bytes:
                assert ctx.resident_info()["complete"] and ctx.resident_info()["blocks"] == 2
    ctx.close()


def test_two_devices_give_the_vectors_of_one(tmp_path, oracle):
    from drprg_amd import Context
    panel, _ = _panel()
    one = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, one)
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=[0, 0])
    multi.set_opts(illumina=True, genome_size=G)
    for c in (one, multi):
        c.set_threads(4)
        c.set_adapters([ADAPTER], error=E)
        c.map_fastx(fq)
        _assert_cut(c, s, "devices")
    one.close()
    multi.close()


# ---- 4. refusals and state ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(tmp_path, oracle):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    n = len(s["reads"])
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    ctx.set_threads(2)
    # nothing set: the vectors of the sample as it is, and no count
    full = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), s["bases"], s["offs"], W, K, True, threads=4)
    ctx.map_fastx(fq)
    _assert_oracle(ctx, full, n, int(s["offs"][-1]), "nothing set")
    assert ctx.adapter_trim_info() == NO_CUT and ctx.read_trim_info() == NO_TRIM and _filter_counts(ctx)["reads_seen"] == 0
    # bad settings
    for bad in (dict(seqs=[ADAPTER] * 5), dict(seqs=[""]), dict(seqs=[TRUSEQ + "A"]), dict(seqs=["ACGN"]), dict(seqs=[ADAPTER], error="0.501"),
                dict(seqs=[ADAPTER, NEXTERA], min_overlap=20)):
        with pytest.raises(DependencyError) as e:
            ctx.set_adapters(**bad)
        assert e.value.code == EINVAL, bad
    # the kernels' own entry without adapters
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(DependencyError) as e:
        ctx.adapter_trim_device(d.data_ptr(), None, None, 0, d.data_ptr(), 1, 0, d.data_ptr(), d.data_ptr())
    assert e.value.code == EINVAL
    # map_host and map_device would map the reads with their adapters: refused while adapters are set, and the context maps on afterwards
    ctx.set_adapters([ADAPTER], error=E)
    ctx.reset()
    d_b, d_o = torch.from_numpy(s["kbases"].copy()).cuda(), torch.from_numpy(s["koffs"].astype(np.int64)).cuda()
    for call in (lambda: ctx.map_host(s["kbases"], s["koffs"]), lambda: ctx.map_device(d_b.data_ptr(), d_o.data_ptr(), n, int(s["koffs"][-1]))):
        with pytest.raises(DependencyError) as e:
            call()
        assert e.value.code == EINVAL and "drprg_hip_set_adapters" in str(e.value)
    assert ctx.counters()["reads"] == 0
    ctx.map_fastx(fq)
    _assert_cut(ctx, s, "after the refusals")
    # discover without resident reads after a cut block: -61
    (tmp_path / "disc").mkdir()
    with pytest.raises(DependencyError) as e:
        ctx.discover_reads(fq, str(tmp_path / "genes.fa"), str(tmp_path / "disc"))
    assert e.value.code == ENODATA
    # a reset clears the counts and keeps the settings
    ctx.reset()
    assert ctx.adapter_trim_info() == NO_CUT
    ctx.map_fastx(fq)
    _assert_cut(ctx, s, "after a reset")
    # cleared: today's path, every base, and map_host is served again
    ctx.set_adapters([])
    ctx.reset()
    ctx.map_host(s["kbases"], s["koffs"])
    _assert_oracle(ctx, s["want"], n, int(s["koffs"][-1]), "map_host, nothing set")
    ctx.reset()
    ctx.map_fastx(fq)
    _assert_oracle(ctx, full, n, int(s["offs"][-1]), "cleared")
    assert ctx.adapter_trim_info() == NO_CUT and _filter_counts(ctx)["reads_seen"] == 0
    ctx.close()


# ---- 5. the executables ---------------------------------------------------------------------------------------------------------------------
def test_pandora_map_writes_the_vcf_of_the_precut_file(tmp_path, oracle):
    from drprg_amd._lib import PANDORA_EXE
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    ctx.close()
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bam = _write_bam(tmp_path / "all.bam", s["bases"], s["offs"], s["quals"])
    cut_fq = _write_fastq(tmp_path / "cut.fq", s["kbases"], s["koffs"], [np.full(L, 30, dtype=np.uint8) for L in s["klengths"]])

    def run(out, reads, extra):
        argv = [PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(G), "--max-covg", "4294967295"] + extra + [
            "--vcf-refs", genes, "-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout, open(out / "pandora_genotyped.vcf", "rb").read()

    stdout, got = run(tmp_path / "adapters", bam, ["--adapter", ADAPTER])
    _, want = run(tmp_path / "cut", cut_fq, [])
    assert vcf_without_date(str(tmp_path / "adapters" / "pandora_genotyped.vcf")) == vcf_without_date(str(tmp_path / "cut" / "pandora_genotyped.vcf"))
    assert [l for l in got.splitlines() if not l.startswith(b"##fileDate")] == [l for l in want.splitlines() if not l.startswith(b"##fileDate")]
    c = s["info"]
    assert "adapter trimming: " + " ".join(f"{key}={c[key]}" for key in INFO_KEYS) in stdout and "read trimming:" not in stdout, stdout
    assert f"reads={c['reads_seen']} bases={int(s['koffs'][-1])} " in stdout, stdout


def test_drprg_predict_takes_the_same_flags(tmp_path):
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 6000, seed=1)
    reads, kinds = rule.plant(bases, offs, ADAPTER, O, seed=67)
    ranges, info = cut_ranges(reads, [(0, len(r)) for r in reads], [ADAPTER], rule.error_milli("0.1"), 3)
    assert info["reads_cut"] >= 4000
    b, o = _flat(reads)
    fq = _write_fastq(tmp_path / "wt.fq", b, o, [np.full(len(r), 30, dtype=np.uint8) for r in reads])
    kept = _cut(reads, ranges)
    kb, ko = _flat(kept)
    cut_fq = _write_fastq(tmp_path / "cut.fq", kb, ko, [np.full(len(r), 30, dtype=np.uint8) for r in kept])

    def run(out, path, extra):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", path, "-o", str(out), "-s", "wt", "-I", "-v"] + extra
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        calls = json.load(open(out / "wt.drprg.json"))["susceptibility"]
        for drug in calls.values():
            for ev in drug["evidence"]:
                ev.pop("vcfid")  # (a fresh identifier per run)
        return r.stderr, (open(out / "pandora_genotyped.vcf").read(), calls)

    err, got = run(tmp_path / "adapters", fq, ["--adapter", ADAPTER, "--adapter-error", "0.1", "--adapter-min-overlap", "3"])
    _, want = run(tmp_path / "cut", cut_fq, [])
    assert got == want
    assert "adapter trimming: " + " ".join(f"{key}={info[key]}" for key in INFO_KEYS) in err, err
    assert f"] reads={len(reads)} " in err
