"""The rule of tests/read_stats_rule.py held to its own properties, and the executables' argument parsing (no device needed: the layout comes
from the library without a context, and a usage error is found before a context is opened)."""
import math
import os
import subprocess

import numpy as np
import pytest

import read_stats_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "drprg_amd", "bin")


@pytest.fixture(scope="module")
def lay():
    return rule.layout()


def test_the_layout_the_library_reports_is_the_rules(lay):
    assert (lay["len_bins"], lay["cycles"], lay["cols"], lay["quals"], lay["gc_bins"]) == (2432, 512, 5, 94, 101)
    sections = [("len_reads", 2432), ("len_bases", 2432), ("cyc_base", 513 * 5), ("cyc_qsum", 513), ("qual_hist", 94), ("readq_hist", 94), ("gc_hist", 101)]
    at = 4  # reads, bases, shortest, longest
    for name, size in sections:  # the sections follow each other without a gap or an overlap
        assert lay[name] == at, (name, lay[name], at)
        at += size
    assert lay["words"] == at


def _lengths():
    out = set(range(0, 4097))
    for e in range(1, 32):
        out.update((2 ** e - 1, 2 ** e, 2 ** e + 1))
    out.add(2 ** 32 - 1)
    return sorted(x for x in out if x < 2 ** 32)


def test_the_bin_function_is_monotone_and_brackets_every_length():
    lengths = _lengths()
    bins = [rule.len_bin(L) for L in lengths]
    assert bins == sorted(bins) and bins[0] == 0 and bins[-1] == rule.LEN_BINS - 1
    for L, b in zip(lengths, bins):
        assert 0 <= b < rule.LEN_BINS
        assert rule.bin_low(b) <= L, (L, b)
        if b + 1 < rule.LEN_BINS:
            assert L < rule.bin_low(b + 1), (L, b)
        else:
            assert L < 2 ** 32
        if L < 1024:
            assert b == L
        else:  # within 1 / 64
            assert (L - rule.bin_low(b)) * 64 < L
    lows = [rule.bin_low(b) for b in range(rule.LEN_BINS)]
    assert lows == sorted(set(lows)) and all(rule.len_bin(x) == b for b, x in enumerate(lows))


def _snap(lay, lengths):
    return rule.snapshot([b"A" * n for n in lengths], None, lay)


def test_n50_of_hand_made_sets(lay):
    assert rule.n50(_snap(lay, []), lay) == 0 and rule.n90(_snap(lay, []), lay) == 0
    assert rule.n50(_snap(lay, [0, 0]), lay) == 0
    assert rule.n50(_snap(lay, [700]), lay) == 700 and rule.n90(_snap(lay, [700]), lay) == 700
    assert rule.n50(_snap(lay, [150] * 9), lay) == 150 and rule.n90(_snap(lay, [150] * 9), lay) == 150
    s = _snap(lay, [1, 1, 2])  # 4 bases: half is 2, reached by the read of 2; nine tenths, rounded up, is 4
    assert rule.n50(s, lay) == 2 and rule.n90(s, lay) == 1
    s = _snap(lay, [10, 10, 20, 40])  # 80 bases: half falls exactly on the sum of bin 40
    assert rule.n50(s, lay) == 40 and rule.n90(s, lay) == 10
    s = _snap(lay, [10, 10, 21, 40])  # 81 bases: half, rounded up, is 41: one more than bin 40 holds
    assert rule.n50(s, lay) == 21
    s = _snap(lay, [5000, 5001, 70000])  # above 1024 the bin's lowest length is reported
    assert rule.n50(s, lay) == rule.bin_low(rule.len_bin(70000)) <= 70000 and rule.n90(s, lay) == rule.bin_low(rule.len_bin(5000)) <= 5000


def test_the_read_quality_bin_is_that_of_the_mean_error_probability():
    """not of the mean Phred value: for reads whose mean error lies at least 1e-6 (relative) away from every table value the bin is
    floor(-10 log10(mean error)) in floating point.  Qualities up to 30: there the table's rounding is below 3e-7 relative"""
    rng = np.random.default_rng(5)
    table = [10 ** (-q / 10) for q in range(rule.QUALS)]
    checked = 0
    reads = [[2] * 50 + [30] * 50, [30], [0], [0] * 7, [2, 30], [30] * 99 + [2]]
    reads += [rng.integers(2, 31, size=int(rng.integers(1, 300))).tolist() for _ in range(400)]
    reads += [rng.choice([2, 12, 23, 30], size=150, p=[0.02, 0.05, 0.13, 0.8]).tolist() for _ in range(200)]
    for q in reads:
        mean = sum(10 ** (-x / 10) for x in q) / len(q)
        if any(abs(mean - t) <= 1e-6 * t for t in table):
            continue
        checked += 1
        assert rule.readq_bin(q) == math.floor(-10 * math.log10(mean)), (q, mean)
    assert checked > 550
    assert rule.readq_bin([2] * 50 + [30] * 50) == 5  # (the mean Phred value would say 16)
    assert rule.readq_bin([93] * 10) == 93 and rule.readq_bin([0] * 10) == 0 and rule.readq_bin([40]) == 40


def test_reads_of_no_base_one_base_and_unknown_bases_only(lay):
    reads = [b"", b"G", b"NNNN", b"", b"n", b"RYKM", b"acgt"]
    quals = [[], [40], [3, 3, 3, 3], [], [0], [10, 20, 30, 40], [93, 93, 0, 93]]
    w = rule.snapshot(reads, quals, lay)
    d = {k: w[lay[k]:lay[k] + n] for k, n in (("len_reads", 2432), ("len_bases", 2432), ("qual_hist", 94), ("readq_hist", 94), ("gc_hist", 101))}
    assert w[:4].tolist() == [7, 14, 0, 4]
    assert d["len_reads"][:5].tolist() == [2, 2, 0, 0, 3] and d["len_bases"][:5].tolist() == [0, 2, 0, 0, 12]
    # reads of no bases are in the length histogram alone; reads of U only are in no GC bin, but their qualities count
    assert int(d["readq_hist"].sum()) == 5 and int(d["gc_hist"].sum()) == 2 and d["gc_hist"][100] == 1 and d["gc_hist"][50] == 1
    assert int(d["qual_hist"].sum()) == 14 and d["qual_hist"][3] == 4 and d["qual_hist"][93] == 3
    cyc = w[lay["cyc_base"]:lay["cyc_base"] + 513 * 5].reshape(513, 5)
    assert cyc[0].tolist() == [1, 0, 1, 0, 3] and cyc[3].tolist() == [0, 0, 0, 1, 2] and int(cyc.sum()) == 14
    assert w[lay["cyc_qsum"]] == 40 + 3 + 0 + 10 + 93
    # without qualities the three quality sections stay zero and everything else is what it was
    v = rule.snapshot(reads, None, lay)
    assert not v[lay["cyc_qsum"]:lay["gc_hist"]].any() and np.array_equal(v[:lay["cyc_qsum"]], w[:lay["cyc_qsum"]]) and np.array_equal(v[lay["gc_hist"]:], w[lay["gc_hist"]:])
    # every position from 512 on falls into the last cycle bin
    long = rule.snapshot([b"C" * 600], [[7] * 600], lay)
    cyc = long[lay["cyc_base"]:lay["cyc_base"] + 513 * 5].reshape(513, 5)
    assert cyc[511].tolist() == [0, 1, 0, 0, 0] and cyc[512].tolist() == [0, 88, 0, 0, 0] and long[lay["cyc_qsum"] + 512] == 88 * 7


@pytest.mark.parametrize("exe, head", [("pandora", ["map"]), ("pandora", ["discover"]), ("drprg", ["predict", "-x", "nowhere", "-i", "nothing.fq"])])
def test_the_executables_refuse_bad_arguments(exe, head):
    path = os.path.join(BIN, exe)
    tail = ["prg", "reads"] if exe == "pandora" else []
    r = subprocess.run([path] + head + ["--qc-no-qual"] + tail, capture_output=True, text=True)
    assert r.returncode == 2 and "--qc-no-qual belongs to --qc-json" in r.stderr, (exe, r.returncode, r.stderr)
    r = subprocess.run([path] + head + ["--qc-json"], capture_output=True, text=True)  # the flag without its value
    assert r.returncode == 2, (exe, r.stderr)
    r = subprocess.run([path, "--help"] if exe == "pandora" else [path, "predict", "--help"], capture_output=True, text=True)
    assert "--qc-json FILE" in r.stdout + r.stderr
