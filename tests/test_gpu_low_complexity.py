"""The minimizer rule's ties on every sketch form of the device, against the oracle (pytest -m gpu).

The batches come from tests/low_complexity.py: reads over repeats, palindromes and homopolymers, where two k-mers of one window share a
canonical hash and "ties kept, each reported once" / strand = (fwd <= rc) decide the result; tests/test_low_complexity.py holds on the CPU
that every class of tie is in every batch and that a one-sided tie rule or a strict strand rule would change it.  Each case maps the whole
batch of its (w, k), ASCII and packed, and requires what test_gpu_parity._compare requires: counters, coverage vector and reads per PRG
bit-exact.  A case that fails names the first read whose mapping on its own differs from the oracle's."""
import numpy as np
import pytest

import low_complexity as L
from test_gpu_parity import _compare, _ctx

pytestmark = pytest.mark.gpu

SMALL = [(11, 15), (14, 15), (1, 15), (16, 15)]
SCAN = [(5, 9), (16, 13), (1, 15), (12, 15), (19, 21), (11, 31), (11, 14), (11, 20), (11, 30)]
# (form, kernel sequence, switches, the (w, k) it serves).  Kernel sequence 1 is sketch_probe_kernel and the generic pipeline whatever the
# switches; sequence 3 is sketch_wave_kernel where it applies (k = 15, w = 11 or 14) unless DRPRG_DIRECT_FORM=lds, sketch_probe_kernel elsewhere
FORMS = [
    ("small_tier_stage2_lds", 2, {"DRPRG_FILTER_STAGE2": "lds"}, SMALL),
    ("small_tier_stage2_l2", 2, {"DRPRG_FILTER_STAGE2": "l2"}, SMALL),
    ("levels_1_2", 2, {}, [(5, 9), (16, 13), (11, 14), (7, 12), (5, 8)]),
    ("middle_tier", 2, {"DRPRG_FORCE_MID_TIER": "1"}, [(11, 15), (14, 15)]),
    ("sketch_wave", 3, {}, [(11, 15), (14, 15)]),
    ("probe_compile_time_window", 1, {"DRPRG_DIRECT_FORM": "lds"}, [(11, 15), (14, 15)]),
    ("probe_compile_time_window", 3, {"DRPRG_DIRECT_FORM": "lds"}, [(11, 15), (14, 15)]),
    ("probe_sequential_scan", 1, {}, SCAN),
    ("probe_sequential_scan", 3, {}, SCAN),
    ("generic_pipeline_behind_the_filter", 2, {"DRPRG_FT_DEBUG": "8"}, [(11, 15), (11, 14)]),
]


def _expected_form(form, k):
    """table_tier()["sketch_form"] (include/drprg_hip.h, drprg_hip_device_tables out[5]) of the form a case is named after"""
    if form == "generic_pipeline_behind_the_filter":
        return 10 if k == 15 else 11
    if form == "probe_sequential_scan":
        return 3 if k <= 15 else 4  # 32-bit keys, 64-bit keys
    return {"small_tier_stage2_lds": 10, "small_tier_stage2_l2": 10, "levels_1_2": 11, "middle_tier": 12, "sketch_wave": 1,
            "probe_compile_time_window": 2}[form]


CASES = [pytest.param(form, kernel, env, w, k, id=f"{form}-kernel{kernel}-w{w}-k{k}") for form, kernel, env, wks in FORMS for w, k in wks]


def test_every_pair_has_its_census():
    assert {(w, k) for *_, wks in FORMS for w, k in wks} == set(L.WK)


def _first_differing_read(ctx, oracle, reads, w, k, kernel, mcs):
    """bisect the batch: the first read that fails _compare on its own (or the smallest failing range no half of which fails alone)"""
    lo, hi = 0, len(reads)

    def fails(a, b):
        try:
            _compare(ctx, oracle, *L.batch(reads[a:b]), w, k, True, kernel, min_cluster_size=mcs)
            return None
        except AssertionError as e:
            return e
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fails(lo, mid):
            hi = mid
        elif fails(mid, hi):
            lo = mid
        else:
            return f"reads {lo}..{hi - 1} differ together, neither half alone"
    return f"read {lo} differs on its own ({fails(lo, hi)!r}): {reads[lo]!r}"


def _compare_named(ctx, oracle, reads, w, k, kernel, mcs, what):
    try:
        return _compare(ctx, oracle, *L.batch(reads), w, k, True, kernel, min_cluster_size=mcs)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e!r}; {_first_differing_read(ctx, oracle, reads, w, k, kernel, mcs)}") from e


@pytest.mark.parametrize("form,kernel,env,w,k", CASES)
def test_ties_on_the_device(tmp_path, oracle, monkeypatch, form, kernel, env, w, k):
    for name, value in env.items():
        monkeypatch.setenv(name, value)  # (read once per context: set before it is opened)
    panel = L.lc_panel()[0]
    ctx = _ctx(tmp_path, panel, w, k, True, kernel=kernel, min_cluster_size=L.MCS)
    tier = ctx.table_tier()
    assert (tier["kernel"], tier["sketch_form"]) == (kernel, _expected_form(form, k)), tier  # the form the case is named after serves it
    if form == "middle_tier":
        assert tier["l2_filter_bytes"] > 0
    idx = ctx.export_index()
    want = oracle.build_index(panel.prgs, w, k)
    for key in ("knode_base", "min_path_len", "keys", "rec_off", "rec_prg", "rec_knode", "rec_strand"):
        assert np.array_equal(idx[key], want[key]), key
    cnt = _compare_named(ctx, oracle, L.reads(w, k), w, k, kernel, L.MCS, f"{form}, kernel sequence {kernel}, w={w}, k={k}")
    assert cnt["clusters_kept"] > 1000 and cnt["hits_kept"] > cnt["clusters_kept"]
    ctx.close()


# ---- the run limits alone -----------------------------------------------------------------------------------------------------------------
def _run_limit_panel(w, k):
    """one locus per period 1 .. w + 1 and length k + w - 2, k + w - 1, k + w, k + 2w - 2, k + 2w - 1: random flank, a repeat of exactly that
    length, random flank.  Returns (Panel, [(locus sequence, start of the repeat, its length)])"""
    from drprg_amd import synth
    rng = np.random.default_rng(100 * w + k)
    names, trees, loci = [], [], []
    for d in range(1, w + 2):
        unit = L._seq(rng, d)
        while d > 1 and len(set(unit)) == 1:
            unit = L._seq(rng, d)
        for n in sorted({k + w - 2, k + w - 1, k + w, k + 2 * w - 2, k + 2 * w - 1}):
            if n < k:
                continue
            rep = (unit * (n // d + 1))[:n]
            f1, f2 = L._seq(rng, 60), L._seq(rng, 60)
            # (a flank that continued the repeat would make it longer than n)
            while f1[-1] == rep[d - 1] or f2[0] == rep[n % d]:
                f1, f2 = L._seq(rng, 60), L._seq(rng, 60)
            names.append(f"p{d}_n{n}")
            trees.append([(f1 + rep + f2).decode()])
            loci.append((f1 + rep + f2, 60, n))
    return synth.Panel(names, trees), loci


@pytest.mark.parametrize("w,k", [(11, 15), (16, 13), (1, 15)])
def test_run_limits_at_both_ends_of_the_batch(tmp_path, oracle, w, k):
    """Reads that are one repeat of k + w - 2 .. k + 2w - 1 bases with 0 .. 20 bases of flank, every period 1 .. w + 1, both strands.  The
    batch is mapped in three orders, each with other bare repeats in its first and last 64 bases: there verify_one_lane reads through
    load16_guarded and walks fewer than four steps to the left, and the padding past the batch's last base meets a tie."""
    panel, loci = _run_limit_panel(w, k)
    rng = np.random.default_rng(w + k)
    reads, bare = [], {False: [], True: []}
    for i, (seq, a, n) in enumerate(loci):
        for j, (f1, f2) in enumerate([(0, 0), (0, 20), (20, 0), tuple(int(x) for x in rng.integers(1, 20, size=2))]):
            flip = bool(rng.integers(0, 2)) if j else i % 2 == 1  # (the strand is drawn apart from the flank; the bare repeats alternate)
            if j == 0:  # no flank at all: the tie touches the batch's first or last base
                bare[flip].append(len(reads))
            r = seq[a - f1:a + n + f2]
            reads.append(L.rc(r) if flip else r)
    assert bare[False] and bare[True]
    for kernel in (1, 2, 3):
        ctx = _ctx(tmp_path, panel, w, k, True, kernel=kernel, min_cluster_size=1)
        hits = 0
        for turn in range(3):  # (a forward and a reverse-complemented bare repeat at each end of the batch, in turn)
            head, tail = bare[turn % 2 == 1], bare[turn % 2 == 0]
            first, last = head[(7 * turn) % len(head)], tail[(11 * turn + 3) % len(tail)]
            order = [first] + [i for i in rng.permutation(len(reads)) if i not in (first, last)] + [last]
            cnt = _compare_named(ctx, oracle, [reads[i] for i in order], w, k, kernel, 1, f"run limits, kernel sequence {kernel}, turn {turn}")
            hits += cnt["hits_kept"]
        assert hits > 3 * len(reads)
        ctx.close()


# ---- through the executables --------------------------------------------------------------------------------------------------------------
def test_pandora_map_of_the_low_complexity_batch(tmp_path, oracle):
    """`pandora index` + `pandora map` on a FASTQ of the (11, 15) batch: the VCF of the host genotyper on the oracle's coverage of the same
    reads, byte for byte (the pattern of test_gpu_parity.test_cli_map_end_to_end)"""
    import subprocess
    from drprg_amd import Context, synth
    from drprg_amd._lib import PANDORA_EXE
    from util import cluster_fraction, map_params
    w, k = 11, 15
    panel = L.lc_panel()[0]
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    panel.write(prg, genes)
    bases, offs = L.batch(L.reads(w, k))
    fq = str(tmp_path / "reads.fq")
    synth.write_fastq(fq, bases, offs)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(w), "-k", str(k), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = tmp_path / "out"
    r = subprocess.run([PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", "20000", "--max-covg",
                        "4294967295", "--vcf-refs", genes, "-t", "1", "-w", str(w), "-k", str(k), "-c", str(L.MCS), "-I", prg, fq],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ctx = Context(prg, w, k, device=-1, from_files=True)
    ctx.set_opts(illumina=True, genome_size=20000, min_cluster_size=L.MCS)
    md, er = map_params(k, True)
    covg, prg_reads, cnt = oracle.map_reads(bases, offs, oracle.build_index(panel.prgs, w, k), w, k, md, cluster_fraction(er, k), L.MCS)
    assert cnt["clusters_kept"] > 1000
    ctx.set_coverage(covg, prg_reads, int(offs[-1]))
    ref = str(tmp_path / "ref.vcf")
    ctx.genotype(genes, ref)
    strip = lambda p: [line for line in open(p) if not line.startswith("##fileDate")]
    assert strip(out / "pandora_genotyped.vcf") == strip(ref)
    assert sum(not line.startswith("#") for line in open(ref)) >= 4  # (the panel's sites are in it)
