"""Adapter trimming under the indel rule and at the 5' end (drprg_hip_set_adapters2, csrc/adapter_edit.hip; pytest -m gpu).  Ranges and counts
come from the rule in plain Python (tests/adapter_edit_rule.py), the vectors and counters from the oracle on the reads the rule leaves -- never
from the code under test.

How the blocks come about: the ingest hands a worker's first block over at 750 000 bases, so the small sample (under that) is one block
and the big one several, whatever the number of parser threads."""
import json
import os
import subprocess

import numpy as np
import pytest

import adapter_edit_rule as rule
import adapter_rule as plain
import read_trim_rule as rtrim
import resident_readback as rb
from adapter_edit_rule import FRONT, INFO_KEYS, cut_ranges, cut_ranges_many, kernel_batch
from adapter_rule import TRUSEQ
from subsample_rule import keep_flags
from test_gpu_adapter_trim import NO_CUT, NO_TRIM, _cut, _fasta, _filter_counts, _flat
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from test_gpu_read_filter import _assert_oracle, _file_of, _write_bam, _write_fastq
from util import vcf_without_date

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
EINVAL, ENODATA = 22, 61
ADAPTER, FRONT_ADAPTER = TRUSEQ[:33], FRONT[-28:]
E, O = "0.1", 3


def _info(out):
    return dict(zip(INFO_KEYS, out[:5])), dict(zip(INFO_KEYS, out[5:]))


# ---- 1. the kernels against the rule ----------------------------------------------------------------------------------------------------
_BATCHES = {}


def _batch(name, err):
    if (name, err) not in _BATCHES:
        b = kernel_batch(name, err)
        b["census"] = rule.census(b)  # (raises when a class is empty or not what it is meant to be: no case passes empty)
        _, b["info3"], b["info5"] = cut_ranges(b["reads"], b["ranges"], b["ad3"], b["ad5"], b["e"], b["O"], known=b["want"])
        if b["noisy"]:  # (the counts of either side alone)
            b["alone3"] = cut_ranges(b["reads"], b["ranges"], b["ad3"], [], b["e"], b["O"], known=b["want3"])[1:]
            b["alone5"] = cut_ranges(b["reads"], b["ranges"], [], b["ad5"], b["e"], b["O"], known=b["want5"])[1:]
        _BATCHES[(name, err)] = b
    return _BATCHES[(name, err)]


def _device_cut(ctx, torch, reads, ranges, form, entry=None):
    text, offs = _flat(reads)
    n_reads, n_bases = len(reads), int(offs[-1])
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_b = torch.from_numpy(np.array([a for a, _ in ranges], dtype=np.int64)).cuda()
    d_e = torch.from_numpy(np.array([b for _, b in ranges], dtype=np.int64)).cuda()
    entry = entry or ctx.adapter_trim_device2
    if form == "packed":
        words, npos = plain.packed_form(text.tobytes())
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_n = torch.from_numpy(npos.astype(np.int64)).cuda() if npos.size else None
        out = entry(None, d_w.data_ptr(), d_n.data_ptr() if npos.size else None, int(npos.size), d_o.data_ptr(), n_reads, n_bases, d_b.data_ptr(), d_e.data_ptr())
    else:
        shift = 1 if form == "text off by one" else 0
        buf = np.zeros(n_bases + (1 if shift else 64), dtype=np.uint8)  # (one byte off: read byte by byte, and the buffer ends with its last base)
        buf[shift:shift + n_bases] = text
        d_t = torch.from_numpy(buf).cuda()
        assert d_t.data_ptr() % 16 == 0
        out = entry(d_t.data_ptr() + shift, None, None, 0, d_o.data_ptr(), n_reads, n_bases, d_b.data_ptr(), d_e.data_ptr())
    torch.cuda.synchronize()
    return out, list(zip(d_b.cpu().numpy().tolist(), d_e.cpu().numpy().tolist()))


@pytest.mark.parametrize("form", ["text", "text off by one", "packed"])
@pytest.mark.parametrize("err", ["0", "0.1", "0.2", "0.5"])
@pytest.mark.parametrize("name", ["12", "16", "17", "32", "33", "64", "33+19"])
def test_the_kernels_equal_the_rule(tmp_path, name, err, form):
    import torch
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    b = _batch(name, err)
    # both sides set; and at E = 0.5, where an adapter of one side is text to the other and a side's classes are pinned with that side
    # alone, each side alone as well (adapter_edit_rule.kernel_batch)
    where = {i: cls for cls, (idx, _) in b["classes"].items() for i in idx}
    runs = [(b["ad3"], b["ad5"], b["want"], b["info3"], b["info5"], 0)]
    if b["noisy"]:
        runs += [(b["ad3"], [], b["want3"]) + b["alone3"] + (3,), ([], b["ad5"], b["want5"]) + b["alone5"] + (5,)]
    for ad3, ad5, want, info3, info5, side in runs:
        ctx.set_adapters(ad3, front=ad5, indels=True, error=err)
        out, got = _device_cut(ctx, torch, b["reads"], b["ranges"], form)
        diff = [i for i in range(len(got)) if got[i] != want[i]]
        assert not diff, (side, [(i, where.get(i), len(b["reads"][i]), b["ranges"][i], got[i], want[i]) for i in diff[:8]])
        assert _info(out) == (info3, info5), (side, out)
        # the census of the classes, on what came back: every class under the setting it is pinned with
        for cls, (idx, kind) in b["classes"].items():
            if (b["sides"][cls] if b["noisy"] else 0) != side:
                continue
            c3 = sum(got[i][1] != b["ranges"][i][1] for i in idx)
            c5 = sum(got[i][0] != b["ranges"][i][0] for i in idx)
            un = sum(got[i] == b["ranges"][i] for i in idx)
            assert idx and (c3, c5, un) == b["census"][cls], cls
        if side == 0 and not b["noisy"]:
            (i,) = b["classes"]["the two cuts take the read between them"][0]
            assert got[i][0] == got[i][1] == len(b["ad5"][0]) and b["info5"]["reads_emptied"] >= 1 and b["info3"]["reads_emptied"] >= 1
    # a second, smaller launch on the same context, either side alone: nothing of the first one is left behind
    A, F = b["ad3"][0].encode(), b["ad5"][0].encode()
    small = [b"", F + b"ACGTTGCAAGGCTTAACCGGATATCG" + A, b"", b"TTTTTTTTTTTTTTT", A, b"TTGACCA" + A[:5], F[-6:] + b"CCATCAT"]
    rg = [(0, len(r)) for r in small]
    for ad3, ad5 in ((b["ad3"], b["ad5"]), (b["ad3"], []), ([], b["ad5"])):
        want2, i3, i5 = cut_ranges(small, rg, ad3, ad5, b["e"], b["O"])
        if b["e"] <= 200:  # (at E = 0.5 the random letters of this read lie within the limit of an adapter somewhere)
            assert want2[1] == (len(F) if ad5 else 0, len(F) + 26 if ad3 else len(small[1])) and want2[3] == (0, 15)
        ctx.set_adapters(ad3, front=ad5, indels=True, error=err)
        out, got = _device_cut(ctx, torch, small, rg, form)
        assert got == want2 and _info(out) == (i3, i5), (ad3, ad5)
    ctx.close()


# ---- 2. a sample with adapters at both ends equals the sample of its cut reads ---------------------------------------------------------------
_SAMPLES = {}


def _sample(which, oracle, ctx):
    """the sample's reads with worn adapters planted at both ends, the rule's cuts, and the oracle's vectors of the cut reads: made once,
    shared, left unchanged"""
    if which not in _SAMPLES:
        _, genomes = _panel()
        lengths, _ = rtrim.small_sample() if which == "small" else rtrim.big_sample()
        bases, offs = _reads_of(genomes, lengths, seed=71)
        reads, kinds = rule.plant(bases, offs, ADAPTER, FRONT_ADAPTER, rule.error_milli(E), seed=72)
        for i in range(0, len(reads), 10):  # a base that is not ACGT in every tenth read: packed blocks list positions
            if len(reads[i]) > 120:
                reads[i] = reads[i][:60] + b"N" + reads[i][61:]
        ranges, i3, i5 = cut_ranges_many(reads, [(0, len(r)) for r in reads], [ADAPTER], [FRONT_ADAPTER], rule.error_milli(E), O)
        n = {k: kinds.count(k) for k in ("both", "front", "end", "none")}
        assert min(n.values()) > len(reads) // 6, n
        for kind in n:  # every kind among the records the BAM form stores on the reverse strand
            assert sum(k == kind and rtrim.reverse_flag(i) for i, k in enumerate(kinds)) > len(reads) // 24, kind
        # every planted adapter is found, and next to no other
        c3 = [rg[1] != len(r) for r, rg in zip(reads, ranges)]
        c5 = [rg[0] != 0 for rg in ranges]
        assert all(c for c, k in zip(c3, kinds) if k in ("both", "end")) and all(c for c, k in zip(c5, kinds) if k in ("both", "front"))
        assert sum(c for c, k in zip(c3, kinds) if k in ("front", "none")) < len(reads) // 10 and sum(c for c, k in zip(c5, kinds) if k in ("end", "none")) < len(reads) // 10
        kept = _cut(reads, ranges)
        kb, ko = _flat(kept)
        b, o = _flat(reads)
        s = dict(reads=reads, bases=b, offs=o, quals=[np.full(len(r), 30, dtype=np.uint8) for r in reads], ranges=ranges, info3=i3, info5=i5, kept=kept, kbases=kb,
                 koffs=ko, klengths=[len(r) for r in kept])
        s["want"] = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
        assert s["want"][2]["clusters_kept"] > 5
        _SAMPLES[which] = s
    return _SAMPLES[which]


def _set(ctx):
    ctx.set_adapters([ADAPTER], front=[FRONT_ADAPTER], indels=True, error=E)


def _assert_cut(ctx, s, what):
    n, nb = len(s["reads"]), int(s["koffs"][-1])
    _assert_oracle(ctx, s["want"], n, nb, what)
    assert ctx.adapter_trim_info() == s["info3"] and ctx.front_adapter_info() == s["info5"], what
    assert ctx.read_trim_info() == NO_TRIM, what
    assert _filter_counts(ctx) == dict(reads_seen=n, bases_seen=nb, dropped_short=0, dropped_long=0, dropped_low_qual=0, reads_kept=n, bases_kept=nb), what


@pytest.mark.parametrize("form", ["fastq ascii", "fastq packed", "bam", "fasta"])
@pytest.mark.parametrize("which", ["small", "big"])
def test_a_sample_with_adapters_at_both_ends_equals_the_sample_of_its_cut_reads(tmp_path, oracle, which, form):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample(which, oracle, ctx)
    path = _fasta(tmp_path / "all.fa", s["reads"]) if form == "fasta" else _file_of(tmp_path, form, s["bases"], s["offs"], s["quals"], "all")
    for packed in ((True,) if form == "fastq packed" else (False,) if form == "fastq ascii" else (False, True)):
        ctx.reset()
        ctx.set_threads(1 if which == "small" else 4)
        ctx.set_input_format(packed)
        ctx.keep_reads(1 << 28)
        _set(ctx)
        ctx.map_fastx(path)
        _assert_cut(ctx, s, (which, form, packed))
        info = ctx.resident_info()
        assert info["complete"] and (info["blocks"] == 1 if which == "small" else info["blocks"] >= 2), info
        if which == "small":  # the resident block is the block cut at both ends
            rb.assert_resident(ctx, s["kept"], packed or form == "bam", (form, packed))
    ctx.close()


# ---- 3. order, and what lies behind it ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fastq ascii", "fastq packed", "bam"])
def test_the_front_adapter_is_sought_in_what_the_crop_left(tmp_path, oracle, form):
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    reads = list(s["reads"])
    body, _ = _reads_of(genomes, [100, 100], seed=73)
    body = body.tobytes()
    F = FRONT_ADAPTER.encode()
    reads += [F[-9:] + body[:100], F[-7:] + body[100:]]  # behind a front crop of 5: four letters are a partial match, two are none
    quals = [np.full(len(r), 30, dtype=np.uint8) for r in reads]
    FRONT_CROP, TAIL = 5, 3
    ranges = [rtrim.kept_range(q, len(r), FRONT_CROP, TAIL, 0, 4) for r, q in zip(reads, quals)]
    cut, i3, i5 = cut_ranges_many(reads, ranges, [ADAPTER], [FRONT_ADAPTER], rule.error_milli(E), O)
    assert ranges[-2] == (5, 106) and cut[-2] == (9, 106) and ranges[-1] == cut[-1] == (5, 104)
    assert i5["reads_cut"] > len(reads) // 4 and i3["reads_cut"] > len(reads) // 4
    kb, ko = _flat(_cut(reads, cut))
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    b, o = _flat(reads)
    ctx.set_threads(2)
    ctx.set_input_format(form == "fastq packed")
    ctx.set_read_trim(front=FRONT_CROP, tail=TAIL)
    _set(ctx)
    ctx.map_fastx(_file_of(tmp_path, form, b, o, quals, "order"))
    _assert_oracle(ctx, want, len(reads), int(ko[-1]), form)
    assert ctx.read_trim_info() == rtrim.info([len(r) for r in reads], ranges, FRONT_CROP, TAIL)  # the crops alone, as without adapters
    assert ctx.adapter_trim_info() == i3 and ctx.front_adapter_info() == i5
    ctx.close()


def test_filter_and_subsample_see_reads_cut_at_both_ends(tmp_path, oracle):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, ctx)
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    ctx.set_threads(4)
    ctx.keep_reads(1 << 28)
    _set(ctx)
    MIN_LEN = 170  # the length bound is that of the read cut at both ends
    keep = [L >= MIN_LEN for L in s["klengths"]]
    ends_only = [rg[1] - 0 for rg in s["ranges"]]  # what the 3' cut alone would leave
    assert sum(e >= MIN_LEN > L for e, L in zip(ends_only, s["klengths"])) > 10  # long enough only with their 5' adapter
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
        assert ctx.adapter_trim_info() == s["info3"] and ctx.front_adapter_info() == s["info5"]
    ctx.set_read_filter()
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


def test_dedup_sees_reads_cut_at_both_ends(tmp_path, oracle):
    """two reads that are identical once both adapters and what lies outside them are gone, and different before: one is dropped"""
    from dedup_rule import keep_flags_fast
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    n, L = 150, 160
    half, _ = _reads_of(genomes, [L] * n, seed=74)
    rng = np.random.default_rng(75)
    tails = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(1, 30)))) for _ in range(2 * n)]
    F = FRONT_ADAPTER
    heads = [F.encode() if i < n else (F[:9] + F[10:]).encode() for i in range(2 * n)]  # the copy's 5' adapter lost a letter
    reads = [heads[i] + half[i % n * L:(i % n + 1) * L].tobytes() + ADAPTER.encode() + tails[i] for i in range(2 * n)]
    ranges, i3, i5 = cut_ranges_many(reads, [(0, len(r)) for r in reads], [ADAPTER], [F], rule.error_milli(E), O)
    kept = _cut(reads, ranges)
    n_before, flags = sum(keep_flags_fast(reads)), keep_flags_fast(kept)
    assert n_before == 2 * n and sum(flags) <= n and not any(flags[n:]) and i3["reads_cut"] == i5["reads_cut"] == 2 * n
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
        _set(ctx)
        ctx.map_fastx(fq)
        out = ctx.dedup()
        assert out == dict(reads_before=2 * n, bases_before=sum(len(r) for r in kept), reads_kept=sum(flags), bases_kept=int(fo[-1])), out
        _assert_oracle(ctx, want, sum(flags), int(fo[-1]), ("dedup", packed))
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
        _set(c)
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
    assert ctx.front_adapter_info() == NO_CUT
    # 5' adapters without the flag; the kernels' second entry without adapters
    with pytest.raises(DependencyError) as e:
        ctx.set_adapters([ADAPTER], front=[FRONT_ADAPTER])
    assert e.value.code == EINVAL
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(DependencyError) as e:
        ctx.adapter_trim_device2(d.data_ptr(), None, None, 0, d.data_ptr(), 1, 0, d.data_ptr(), d.data_ptr())
    assert e.value.code == EINVAL
    # the old device entry under the indel rule: -EINVAL; under the plain rule both entries give the plain rule's ends and counts
    small = [b"ACGTTGCAAGGCTTAACCGGATATCG" + ADAPTER.encode(), b"TTGACCA" + ADAPTER[:5].encode(), FRONT_ADAPTER.encode() + b"ACGTTGCAAGGCTTAACC"]
    rg = [(0, len(r)) for r in small]
    _set(ctx)
    with pytest.raises(DependencyError) as e:
        _device_cut(ctx, torch, small, rg, "text", entry=ctx.adapter_trim_device)
    assert e.value.code == EINVAL
    ctx.set_adapters([ADAPTER], error=E)
    want, info = plain.cut_ranges(small, rg, [ADAPTER], rule.error_milli(E), O)
    out, got = _device_cut(ctx, torch, small, rg, "text", entry=ctx.adapter_trim_device)
    assert got == want == [(0, 26), (0, 7), rg[2]] and dict(zip(INFO_KEYS, out)) == info
    out, got = _device_cut(ctx, torch, small, rg, "packed")
    assert got == want and _info(out) == (info, NO_CUT)
    # map_host and map_device would map the reads with their adapters: refused while only a 5' adapter is set, too
    ctx.set_adapters([], front=[FRONT_ADAPTER], indels=True)
    ctx.reset()
    d_b, d_o = torch.from_numpy(s["kbases"].copy()).cuda(), torch.from_numpy(s["koffs"].astype(np.int64)).cuda()
    for call in (lambda: ctx.map_host(s["kbases"], s["koffs"]), lambda: ctx.map_device(d_b.data_ptr(), d_o.data_ptr(), n, int(s["koffs"][-1]))):
        with pytest.raises(DependencyError) as e:
            call()
        assert e.value.code == EINVAL
    assert ctx.counters()["reads"] == 0
    _set(ctx)
    ctx.map_fastx(fq)
    _assert_cut(ctx, s, "after the refusals")
    # discover without resident reads after a cut block: -61
    (tmp_path / "disc").mkdir()
    with pytest.raises(DependencyError) as e:
        ctx.discover_reads(fq, str(tmp_path / "genes.fa"), str(tmp_path / "disc"))
    assert e.value.code == ENODATA
    # a reset clears the counts and keeps the settings
    ctx.reset()
    assert ctx.adapter_trim_info() == NO_CUT and ctx.front_adapter_info() == NO_CUT
    ctx.map_fastx(fq)
    _assert_cut(ctx, s, "after a reset")
    # set_adapters after set_adapters2: the plain rule, its cuts and its counts, and no 5' count
    ctx.set_adapters([ADAPTER], error=E)
    ctx.reset()
    ranges, info = plain.cut_ranges(s["reads"], [(0, len(r)) for r in s["reads"]], [ADAPTER], rule.error_milli(E), O)
    assert ranges != s["ranges"]
    kb, ko = _flat(_cut(s["reads"], ranges))
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    ctx.map_fastx(fq)
    _assert_oracle(ctx, want, n, int(ko[-1]), "the plain rule again")
    assert ctx.adapter_trim_info() == info and ctx.front_adapter_info() == NO_CUT
    # cleared through either entry: every base
    full = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), s["bases"], s["offs"], W, K, True, threads=4)
    for clear in (lambda: ctx.set_adapters([], indels=True), lambda: ctx.set_adapters([])):
        _set(ctx)
        clear()
        ctx.reset()
        ctx.map_fastx(fq)
        _assert_oracle(ctx, full, n, int(s["offs"][-1]), "cleared")
        assert ctx.adapter_trim_info() == NO_CUT and ctx.front_adapter_info() == NO_CUT and _filter_counts(ctx)["reads_seen"] == 0
    ctx.close()


# ---- 5. the executables ---------------------------------------------------------------------------------------------------------------------
def _lines(info3, info5):
    return ("] adapter trimming: " + " ".join(f"{key}={info3[key]}" for key in INFO_KEYS), "front adapter trimming: " + " ".join(f"{key}={info5[key]}" for key in INFO_KEYS))


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

    stdout, got = run(tmp_path / "adapters", bam, ["--adapter", ADAPTER, "--adapter-indels", "--front-adapter", FRONT_ADAPTER])
    _, want = run(tmp_path / "cut", cut_fq, [])
    assert vcf_without_date(str(tmp_path / "adapters" / "pandora_genotyped.vcf")) == vcf_without_date(str(tmp_path / "cut" / "pandora_genotyped.vcf"))
    assert [l for l in got.splitlines() if not l.startswith(b"##fileDate")] == [l for l in want.splitlines() if not l.startswith(b"##fileDate")]
    for line in _lines(s["info3"], s["info5"]):
        assert line in stdout, stdout
    assert "read trimming:" not in stdout and f"reads={s['info3']['reads_seen']} bases={int(s['koffs'][-1])} " in stdout, stdout


def test_drprg_predict_takes_the_same_flags(tmp_path):
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 6000, seed=1)
    reads, kinds = rule.plant(bases, offs, ADAPTER, FRONT_ADAPTER, rule.error_milli(E), seed=77)
    ranges, i3, i5 = cut_ranges_many(reads, [(0, len(r)) for r in reads], [ADAPTER], [FRONT_ADAPTER], rule.error_milli(E), O)
    assert i3["reads_cut"] >= 2500 and i5["reads_cut"] >= 2500
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

    err, got = run(tmp_path / "adapters", fq, ["--adapter", ADAPTER, "--adapter-error", E, "--adapter-min-overlap", "3", "--adapter-indels", "--front-adapter", FRONT_ADAPTER])
    _, want = run(tmp_path / "cut", cut_fq, [])
    assert got == want
    for line in _lines(i3, i5):
        assert line in err, err
    assert f"] reads={len(reads)} " in err
