"""Random subsample of the resident sample (drprg_hip_subsample, csrc/subsample.hip; pytest -m gpu).  The flags and the four numbers come
from the rule in plain Python (tests/subsample_rule.py), the vectors and counters from the oracle on the reads the rule selects, the
files from contexts that were given those reads alone -- never from the code under test.

How the reads get resident: through drprg_hip_map_fastx, one small file = one block (the ingest hands a worker's first block over at
750 000 bases: every file here but the large one stays below that), several files = several blocks.  (map_host does not keep its batch
under keep_reads -- tests/test_resident.py holds that -- so the blocks here come from files, in ASCII, packed and BAM form.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import bam_writer
from bam_writer import Rec
from max_covg_rule import accepted_reads
from subsample_rule import DEFAULT_SEED, keep_flags, keep_flags_blocks
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from util import vcf_without_date

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, K = 11, 15
G = 10_000
EINVAL, ENODATA = 22, 61


def _write_blocks(d, bases, offs, cuts, tag):
    """the reads as FASTQ files: reads [cuts[i], cuts[i + 1]) in file i"""
    from drprg_amd import synth
    files = []
    for i in range(len(cuts) - 1):
        lo, hi = cuts[i], cuts[i + 1]
        fq = str(d / f"{tag}_{i}.fq")
        synth.write_fastq(fq, bases[int(offs[lo]):int(offs[hi])], offs[lo:hi + 1] - offs[lo])
        files.append(fq)
    return files


def _map_files(ctx, files, formats):
    """a fresh sample: reset, then every file through map_fastx on one parser thread (one block each) in the input form given for it"""
    ctx.reset()
    ctx.set_threads(1)
    ctx.set_ordered_ingest(True)
    for fq, packed in zip(files, formats):
        ctx.set_input_format(packed)
        ctx.map_fastx(fq)
    ctx.set_input_format(False)


def _select(bases, offs, flags):
    """the reads with flag 1 as a batch"""
    keep = np.flatnonzero(np.asarray(flags))
    parts = [bases[int(offs[i]):int(offs[i + 1])] for i in keep]
    o = np.zeros(len(keep) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([p.size for p in parts])
    return (np.concatenate(parts) if len(parts) and o[-1] else np.zeros(0, np.uint8)), o


def _assert_oracle(ctx, want, n_reads, n_bases, what):
    ocov, oprg, ocnt = want
    cov, prg = ctx.coverage()
    cnt = ctx.counters()
    assert cnt["reads"] == n_reads and cnt["bases"] == n_bases, (what, cnt)
    for key in ("hits", "clusters_kept", "hits_kept"):
        assert cnt[key] == ocnt[key], (what, key)
    assert np.array_equal(prg, oprg) and np.array_equal(cov, ocov), what


# ---- 1. flags equal the rule ----------------------------------------------------------------------------------------------------------
def _ragged_lengths(seed=11, n=5000):
    rng = np.random.default_rng(seed)
    L = np.where(rng.random(n) < 0.3, rng.integers(0, 401, size=n), rng.integers(0, 151, size=n))  # (0 .. 400, 560 kb in all: one block)
    for at in rng.integers(0, n - 40, size=12):
        L[at:at + int(rng.integers(2, 30))] = 0  # runs of zero-length reads
    L[:3] = 0
    L[-2:] = 0
    return [int(x) for x in L]


def test_flags_and_counts_equal_the_rule(tmp_path):
    panel, genomes = _panel()
    L = _ragged_lengths()
    # a run of empty reads that will be a file -- a block that holds no base -- of its own
    L[2000:2007] = [0] * 7
    bases, offs = _reads_of(genomes, L, seed=5)
    S, n = int(offs[-1]), len(L)
    assert S < 700_000 and max(L) == 400
    layouts = {
        "one block": ([0, n], [True]),
        "four blocks, one of empty reads only": ([0, 2000, 2007, 3500, n], [False, True, True, False]),
    }
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    for name, (cuts, formats) in layouts.items():
        files = _write_blocks(tmp_path, bases, offs, cuts, name.split()[0])
        for seed in (1, 7, 2 ** 63 + 12345):
            for T in (S // 10, S // 2, S * 999 // 1000, S, S - 1, 0):
                _map_files(ctx, files, formats)
                info = ctx.resident_info()
                assert info["complete"] and info["blocks"] == len(cuts) - 1 - (1 if len(cuts) > 2 else 0), info
                want = keep_flags(L, T, seed)
                out = ctx.subsample(T, seed)
                got = ctx.subsample_flags(n)
                kept_bases = sum(l for l, f in zip(L, want) if f)
                assert out == dict(reads_before=n, bases_before=S, reads_kept=sum(want), bases_kept=kept_bases), (name, seed, T, out)
                assert got.tolist() == want, (name, seed, T, np.flatnonzero(got != np.array(want))[:8])
                cnt = ctx.counters()
                assert cnt["reads"] == sum(want) and cnt["bases"] == kept_bases, (name, seed, T, cnt)
                assert ctx.resident_info()["complete"]
    # the numpy statement of the rule, block by block, says the same
    assert [int(x) for b in keep_flags_blocks([L[:2000], L[2000:2007], L[2007:]], S // 2, 7) for x in b] == keep_flags(L, S // 2, 7)
    ctx.close()


def test_a_file_of_several_blocks_is_numbered_in_file_order(tmp_path):
    """four parser threads and a file they cut into several blocks: under the ordered hand-over the flags are the rule's on the file's
    order; without it the sample is refused, not numbered by chance"""
    from drprg_amd import synth
    from drprg_amd.pandora import DependencyError
    panel, genomes = _panel()
    n = 240_000
    bases, offs = synth.sample_short_reads(genomes, n, seed=12)
    fq = str(tmp_path / "big.fq")
    synth.write_fastq_fixed(fq, bases, 150)
    T = 150 * n // 7
    want = keep_flags_blocks([[150] * n], T, 3)[0]
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 30)
    ctx.set_threads(4)
    for packed in (True, False):
        ctx.reset()
        ctx.set_input_format(packed)
        ctx.set_ordered_ingest(True)
        ctx.map_fastx(fq)
        assert ctx.resident_info()["complete"] and ctx.resident_info()["blocks"] >= 2
        out = ctx.subsample(T, 3)
        assert out == dict(reads_before=n, bases_before=150 * n, reads_kept=int(want.sum()), bases_kept=150 * int(want.sum())), out
        assert np.array_equal(ctx.subsample_flags(n), want)
        assert ctx.counters()["reads"] == int(want.sum())
    ctx.reset()
    ctx.set_ordered_ingest(False)
    ctx.map_fastx(fq)
    assert ctx.resident_info()["blocks"] >= 2
    with pytest.raises(DependencyError) as e:
        ctx.subsample(T, 3)
    assert e.value.code == EINVAL and "drprg_hip_set_ordered_ingest" in str(e.value)
    ctx.close()


# ---- 2. compaction edges ----------------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (1, 15, 16, 17, 33, 400)


def _edge_batch(with_n):
    """6000 reads in three blocks, lengths 1, 15, 16, 17, 33, 47, 150, 400 and 0..40, some with a non-ACGT base at their first base, their
    last base or in the middle; and the first (target, seed) under which the rule's selection covers every edge the compaction has"""
    panel, genomes = _panel()
    rng = np.random.default_rng(21)
    n = 6000
    L = [int(rng.choice(EDGE_LENGTHS + (150, 150, 33, 47))) if rng.random() < 0.6 else int(rng.integers(0, 41)) for _ in range(n)]
    bases, offs = _reads_of(genomes, L, seed=6)
    bases = bases.copy()
    n_first, n_last, n_mid = set(), set(), set()
    if with_n:
        for i in range(n):
            if L[i] == 0:
                continue
            if i % 5 == 0:
                bases[int(offs[i])] = ord("N")
                n_first.add(i)
            elif i % 5 == 1:
                bases[int(offs[i + 1]) - 1] = ord("N")
                n_last.add(i)
            elif i % 5 == 2 and L[i] >= 3:
                bases[int(offs[i]) + L[i] // 2] = ord("N")
                n_mid.add(i)
    cuts = [0, 2000, 4000, n]
    S = int(offs[-1])
    for seed in range(1, 400):
        T = S // 2
        flags = keep_flags(L, T, seed)
        pairs, lengths, shared = set(), set(), False
        firsts, lasts = set(), set()
        for b in range(3):
            lo, hi = cuts[b], cuts[b + 1]
            firsts.add(flags[lo])
            lasts.add(flags[hi - 1])
            at, prev = 0, None  # new position; the last kept read with a base
            for i in range(lo, hi):
                if not flags[i] or L[i] == 0:
                    continue
                src = int(offs[i]) - int(offs[lo])
                if L[i] >= 32:  # (holds a whole output word: the funnel shift runs at this pair of phases)
                    pairs.add((src % 16, at % 16))
                lengths.add(L[i])
                if prev is not None and at % 16 != 0 and i - prev > 1 and any(L[j] > 0 for j in range(prev + 1, i)):
                    shared = True  # two kept reads in one output word, dropped reads with bases between them
                at += L[i]
                prev = i
        kept = {i for i in range(n) if flags[i]}
        ok = len(pairs) == 256 and set(EDGE_LENGTHS) <= lengths and shared and firsts == {0, 1} and lasts == {0, 1}
        if with_n:
            ok = ok and kept & n_first and kept & n_last and kept & n_mid and (n_first | n_last | n_mid) - kept
        if ok:
            return panel, L, bases, offs, cuts, T, seed, flags
    raise AssertionError("no seed covers the compaction's edges")


@pytest.mark.parametrize("form", ["packed", "ascii", "packed, no listed position"])
def test_compaction_edges_against_the_oracle(tmp_path, oracle, form):
    panel, L, bases, offs, cuts, T, seed, flags = _edge_batch(with_n=form != "packed, no listed position")
    packed = form != "ascii"
    n = len(L)
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    files = _write_blocks(tmp_path, bases, offs, cuts, "edge")
    _map_files(ctx, files, [packed] * 3)
    assert ctx.resident_info()["blocks"] == 3
    out = ctx.subsample(T, seed)
    sel_bases, sel_offs = _select(bases, offs, flags)
    assert out == dict(reads_before=n, bases_before=int(offs[-1]), reads_kept=int(sum(flags)), bases_kept=int(sel_offs[-1])), out
    assert ctx.subsample_flags(n).tolist() == flags
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    want = _oracle_map(oracle, idx, sel_bases, sel_offs, W, K, True)
    assert want[2]["clusters_kept"] > 5
    _assert_oracle(ctx, want, int(sum(flags)), int(sel_offs[-1]), form)
    # what stays resident is what a context keeps that was given the selected reads alone, block for block: for packed blocks a quarter
    # of the kept bases (+ offsets and listed positions)
    info = ctx.resident_info()
    (tmp_path / "other").mkdir()
    (tmp_path / "third").mkdir()
    other = _ctx(tmp_path / "other", panel, W, K, True, genome_size=G)
    other.keep_reads(1 << 28)
    sel_cuts = [int(sum(flags[:c])) for c in cuts]
    _map_files(other, _write_blocks(tmp_path, sel_bases, sel_offs, sel_cuts, "sel"), [packed] * 3)
    assert info == other.resident_info() and info["complete"] and info["blocks"] == 3
    if packed:
        assert (int(sel_offs[-1]) + 15) // 16 * 4 <= info["bytes"] < int(sel_offs[-1])
    _assert_oracle(other, want, int(sum(flags)), int(sel_offs[-1]), "the selected reads alone")
    # everything behind sees the kept reads and knows nothing of the subsample: the same reads come back from the selection kernel, and
    # another context maps them from HBM
    from test_gpu_read_selection import code
    anchors = sorted({bytes(sel_bases[int(sel_offs[i]) + 100:int(sel_offs[i]) + 115]) for i in range(len(sel_offs) - 1)
                      if sel_offs[i + 1] - sel_offs[i] == 400 and set(bytes(sel_bases[int(sel_offs[i]) + 100:int(sel_offs[i]) + 115])) <= set(b"ACGT")})[:6]
    assert len(anchors) >= 3
    a, b = ctx.select_reads([code(x) for x in anchors], 15), other.select_reads([code(x) for x in anchors], 15)
    assert a[2].size >= 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    third = _ctx(tmp_path / "third", panel, W, K, True, genome_size=G)
    third.map_resident(ctx)
    _assert_oracle(third, want, int(sum(flags)), int(sel_offs[-1]), "map_resident of the kept reads")
    # a second call numbers the kept reads from 0
    L2 = [L[i] for i in range(n) if flags[i]]
    T2 = int(sel_offs[-1]) // 3
    flags2 = keep_flags(L2, T2, seed + 1)
    out2 = ctx.subsample(T2, seed + 1)
    assert out2["reads_before"] == len(L2) and out2["reads_kept"] == sum(flags2) and ctx.subsample_flags(len(L2)).tolist() == flags2
    b2, o2 = _select(sel_bases, sel_offs, flags2)
    _assert_oracle(ctx, _oracle_map(oracle, idx, b2, o2, W, K, True), int(sum(flags2)), int(o2[-1]), "second subsample")
    for c in (ctx, other, third):
        c.close()


# ---- 3. nothing dropped -----------------------------------------------------------------------------------------------------------------
def test_a_target_the_sample_does_not_reach_changes_nothing(tmp_path, oracle):
    from drprg_amd import synth
    panel, genomes = _panel()
    bases, offs = synth.sample_short_reads(genomes, 2000, seed=4)
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    files = _write_blocks(tmp_path, bases, offs, [0, 900, 2000], "all")
    _map_files(ctx, files, [True, False])
    before = (ctx.coverage(), ctx.counters(), ctx.resident_info())
    S = int(offs[-1])
    for T in (S, S + 1, 2 ** 64 - 1):
        out = ctx.subsample(T, 3)
        assert out == dict(reads_before=2000, bases_before=S, reads_kept=2000, bases_kept=S)
        assert ctx.subsample_flags(2000).tolist() == [1] * 2000
        after = (ctx.coverage(), ctx.counters(), ctx.resident_info())
        assert after[1:] == before[1:] and all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), bases, offs, W, K, True)
    _assert_oracle(ctx, want, 2000, S, "untouched")
    ctx.close()


# ---- 4. discover from HBM sees the kept reads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_discover_from_hbm_after_a_subsample_equals_discover_of_the_selected_reads(tmp_path, packed):
    from drprg_amd import Context, synth
    from test_resident import _fastq_arrays, _files, _sample
    panel, prg, genes, fq = _sample(tmp_path, kind="snp")
    bases, offs = _fastq_arrays(fq)
    L = np.diff(offs.astype(np.int64)).tolist()
    T, seed = int(offs[-1]) // 2, 5
    flags = keep_flags(L, T, seed)
    sel_fq = str(tmp_path / "selected.fq")
    synth.write_fastq(sel_fq, *_select(bases, offs, flags))

    def run(reads, out, subsample):
        out.mkdir()
        ctx = Context(prg, W, K, device=0, from_files=False)
        ctx.set_opts(illumina=True, genome_size=4000)
        ctx.set_threads(2)
        ctx.set_input_format(packed)
        if subsample:
            ctx.keep_reads(1 << 30)
            ctx.set_ordered_ingest(True)
        ctx.map_fastx(reads)
        if subsample:
            res = ctx.subsample(T, seed)
            assert res["reads_kept"] == sum(flags) and res["reads_before"] == len(L)
        return ctx, ctx.discover_reads(reads, genes, str(out))

    a, va = run(fq, tmp_path / "hbm", True)
    b, vb = run(sel_fq, tmp_path / "selected", False)
    assert a.resident_info()["last_discover_from_hbm"] and not b.resident_info()["last_discover_from_hbm"]
    assert va == vb and len(va) == 1
    assert _files(tmp_path / "hbm") == _files(tmp_path / "selected")
    assert np.array_equal(a.coverage()[0], b.coverage()[0]) and a.counters() == b.counters()
    a.close()
    b.close()


# ---- 5. the executables, on a coordinate-sorted BAM ------------------------------------------------------------------------------------------
def _sorted_bam(tmp_path):
    """reads over the small panel's loci, ordered by locus and position, about 40x deep"""
    from drprg_amd import synth
    panel = synth.small_panel(seed=23, n_loci=4, length=900)
    rng = np.random.default_rng(3)
    size = sum(len(r) for r in panel.refs)
    reads, first_of_locus = [], []
    for ref in panel.refs:
        first_of_locus.append(len(reads))
        h = np.frombuffer(ref.encode(), np.uint8)
        for s in sorted(rng.integers(0, len(h) - 150, size=40 * len(h) // 150).tolist()):
            r = h[s:s + 150]
            reads.append(bytes(synth._COMP[r[::-1]]) if rng.random() < 0.5 else bytes(r))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    recs = [Rec(r.translate(comp)[::-1].decode(), flag=0x10, name=b"r%d" % i) if i % 3 == 0 else Rec(r.decode(), flag=0, name=b"r%d" % i)
            for i, r in enumerate(reads)]  # (a third of them stored on the reverse strand)
    bam = str(bam_writer.write(tmp_path / "sorted.bam", recs, text=b"@HD\tVN:1.6\tSO:coordinate\n"))
    return panel, size, reads, first_of_locus, bam


def _pandora_map(exe, out, prg, genes, size, reads, extra):
    argv = [exe, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(size)] + extra + [
        "--vcf-refs", genes, "-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
    r = subprocess.run(argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout, vcf_without_date(str(out / "pandora_genotyped.vcf"))


def test_pandora_map_subsamples_a_sorted_bam_where_the_prefix_cap_loses_loci(tmp_path):
    from drprg_amd import synth
    from drprg_amd._lib import PANDORA_EXE
    panel, size, reads, first_of_locus, bam = _sorted_bam(tmp_path)
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    panel.write(prg, genes)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = [len(r) for r in reads]
    T = 10 * size
    flags = keep_flags(L, T, 7)
    assert 0.2 < sum(flags) / len(L) < 0.3
    sel = [r for r, f in zip(reads, flags) if f]
    sel_fq = str(tmp_path / "selected.fq")
    (tmp_path / "selected.fq").write_bytes(b"".join(b"@s%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(sel)))
    stdout, got = _pandora_map(PANDORA_EXE, tmp_path / "sub", prg, genes, size, bam, ["--subsample-covg", "10", "--seed", "7"])
    _, want = _pandora_map(PANDORA_EXE, tmp_path / "sel", prg, genes, size, sel_fq, ["--max-covg", "4294967295"])
    assert got == want
    contigs = re.findall(r"(?m)^##contig=<ID=(\w+)>", got)
    assert contigs == sorted(panel.names), contigs  # every locus present
    line = f"subsample: reads_before={len(L)} bases_before={sum(L)} reads_kept={len(sel)} bases_kept={sum(len(r) for r in sel)} (target {T} bases, seed 7)"
    assert line in stdout and f"reads={len(sel)} " in stdout, stdout
    # the contrast: the prefix cap at the same depth stops inside the first loci of the sorted file.  By the cap's rule on this fixture
    # (tests/max_covg_rule.py) no read of the last locus is accepted ...
    n, _, reached = accepted_reads(L, size, 9)
    assert reached and n <= first_of_locus[-1]
    # ... so its ##contig line is gone, with exit 0
    _, capped = _pandora_map(PANDORA_EXE, tmp_path / "cap", prg, genes, size, bam, ["--max-covg", "9"])
    assert f"##contig=<ID={panel.names[-1]}>" not in capped and f"##contig=<ID={panel.names[0]}>" in capped
    # the sample must be resident: with that switched off the run fails, it never maps everything silently
    r = subprocess.run([PANDORA_EXE, "map", "-o", str(tmp_path / "off"), "-g", str(size), "--subsample-covg", "10", "-w", str(W), "-k", str(K), "-I", prg, bam],
                       capture_output=True, text=True, env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "pandora_genotyped.vcf").exists()


def test_drprg_predict_subsamples_and_says_what_it_kept(tmp_path):
    from drprg_amd import synth
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 14000, seed=1)
    fq = str(tmp_path / "wt.fq")
    synth.write_fastq_fixed(fq, bases, 150)
    T = int(0.25 * 4411532)
    argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "-o", str(tmp_path / "out"), "-s", "wt", "-I", "-v", "--subsample-covg", "0.25"]
    r = subprocess.run(argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    flags = keep_flags([150] * 14000, T, DEFAULT_SEED)
    kept = sum(flags)
    assert kept == -(-T // 150)
    assert f"subsample: reads_before=14000 bases_before={14000 * 150} reads_kept={kept} bases_kept={kept * 150} (target {T} bases, seed {DEFAULT_SEED})" in r.stderr, r.stderr
    assert f"] reads={kept} " in r.stderr and "(reads resident in device memory)" in r.stderr
    assert (tmp_path / "out" / "wt.drprg.json").exists()
    r = subprocess.run(argv[:7] + [str(tmp_path / "off")] + argv[8:], capture_output=True, text=True, env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "wt.drprg.json").exists()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(tmp_path, oracle):
    from drprg_amd import Context, synth
    from drprg_amd.pandora import DependencyError
    panel, genomes = _panel()
    bases, offs = synth.sample_short_reads(genomes, 2000, seed=8)
    S = int(offs[-1])
    fq = _write_blocks(tmp_path, bases, offs, [0, 2000], "r")[0]
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), bases, offs, W, K, True)

    def refused(c, code, text):
        state = (c.coverage(), c.counters(), c.resident_info())
        with pytest.raises(DependencyError) as e:
            c.subsample(S // 2, 1)
        assert e.value.code == code and text in str(e.value), e.value
        after = (c.coverage(), c.counters(), c.resident_info())
        assert after[1:] == state[1:] and all(np.array_equal(x, y) for x, y in zip(state[0], after[0]))

    # no subsample call yet: there are no flags
    with pytest.raises(DependencyError) as e:
        ctx.subsample_flags(2000)
    assert e.value.code == EINVAL
    # the reads are not resident: keep_reads off
    ctx.map_fastx(fq)
    refused(ctx, ENODATA, "DRPRG_HIP_KEEP_READS_GB")
    _assert_oracle(ctx, want, 2000, S, "not resident")
    # the resident set overflowed its limit
    ctx.reset()
    ctx.keep_reads(1000)
    ctx.map_fastx(fq)
    assert not ctx.resident_info()["complete"]
    refused(ctx, ENODATA, "DRPRG_HIP_KEEP_READS_GB")
    _assert_oracle(ctx, want, 2000, S, "over the limit")
    # a depth cap is set (one the sample does not reach: the reads are all resident)
    ctx.keep_reads(1 << 28)
    ctx.reset()
    ctx.set_max_covg(1000)
    ctx.map_fastx(fq)
    assert ctx.resident_info()["complete"]
    refused(ctx, EINVAL, "depth cap")
    _assert_oracle(ctx, want, 2000, S, "depth cap")
    ctx.set_max_covg(None)
    # the flags of a call, asked for with the wrong number of reads
    out = ctx.subsample(S // 2, 1)
    flags = keep_flags(np.diff(offs.astype(np.int64)).tolist(), S // 2, 1)
    assert out["reads_kept"] == sum(flags)
    for n in (1999, 2001, sum(flags), 0):
        with pytest.raises(DependencyError) as e:
            ctx.subsample_flags(n)
        assert e.value.code == EINVAL, n
    assert ctx.subsample_flags(2000).tolist() == flags
    # ... and the context maps on: the whole sample again, the oracle's vectors
    ctx.reset()
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
