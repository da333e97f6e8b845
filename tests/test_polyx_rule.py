"""The rules of tests/polyx_rule.py on the issue's worked cases and edges, and the executables' argument parsing (no device needed: a usage
error is found before a context is opened)."""
import os
import subprocess

import numpy as np
import pytest

import polyx_rule as rule

PRE = b"TCATCATTCAACTTACAC"  # ("..." of the worked cases: no G, and no suffix of it joins a tail by the allowance)


@pytest.mark.parametrize("read, M, cut", [
    (PRE + b"AC" + b"G" * 9, 10, 0),
    (PRE + b"AC" + b"G" * 10, 10, 10),
    (PRE + b"CA" + b"GGGGAGGGGG", 10, 10),
    (PRE + b"CA" + b"GGGAGGG", 7, 0),       # floor(7 / 8) = 0
    (PRE + b"CA" + b"GGGAGGGG", 8, 8),
    (b"TTTT" + b"GACGT" + b"G" * 40, 10, 45),
    (b"C" * 30 + b"G" * 100 + b"AAAAA", 10, 105),
    (b"C" * 30 + b"G" * 100 + b"AAAAAA", 10, 0),  # six mismatches
    (b"G" * 20, 10, 20),                    # the read stays as a read of no bases
    (PRE + b"gggggNGGGGGG", 10, 12),
])
def test_the_worked_cases_of_the_tail_cut(read, M, cut):
    assert rule.tail_cut(read, "G", M) == cut
    assert rule.tail_cut_fast(read, "G", M) == cut
    assert rule.tail_cut(read, "g", M) == cut


def _tail(n, mm):
    """a suffix of n bases that begins with G and holds mm bases that are not G, right behind its first base"""
    return b"G" + b"A" * mm + b"G" * (n - 1 - mm)


@pytest.mark.parametrize("n, allowed", [(7, 0), (8, 1), (15, 1), (16, 2), (40, 5), (47, 5), (48, 5)])
def test_the_allowance_steps(n, allowed):
    assert rule.allowance(n) == allowed
    pre = b"CTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCTCT"
    assert rule.tail_cut(pre + _tail(n, allowed), "G", 2) == n
    # one more: that suffix no longer qualifies, and what qualifies is shorter (the run of G behind the other bases)
    assert rule.tail_cut(pre + _tail(n, allowed + 1), "G", 2) == n - 2 - allowed
    assert not rule.qualifies(rule.symbols(pre + _tail(n, allowed + 1)), n, "G")


def test_five_against_six_and_the_first_base():
    pre = b"CT" * 20
    five, six = b"G" + b"A" * 5 + b"G" * 60, b"G" + b"A" * 6 + b"G" * 60
    assert rule.tail_cut(pre + five, "G") == 66 and rule.tail_cut(pre + six, "G") == 60
    # the first base must be X: five other bases IN FRONT of the run never join it
    assert rule.tail_cut(pre + b"AAAAA" + b"G" * 60, "G") == 60
    assert rule.tail_cut(pre + b"A" + b"G" * 60, "G") == 60
    # M is a floor on n, not on the run
    assert rule.tail_cut(pre + b"G" * 12, "G", 13) == 0 and rule.tail_cut(pre + b"G" * 12, "G", 12) == 12


def test_unknown_bases_and_case():
    pre = b"CT" * 20
    assert rule.symbols(b"acgtNnRx-A") == "ACGTUUUUUA"
    assert rule.tail_cut(pre + b"gGgGgGgGgGgG", "G") == 12
    assert rule.tail_cut(pre + b"GGGGNGGGG", "G", 9) == 9      # U is not G: one other base in nine
    assert rule.tail_cut(pre + b"GGGGNNGGGG", "G", 4) == 4      # two in ten: floor(10 / 8) = 1
    assert rule.tail_cut(pre + b"N" * 30, "ACGT", 2) == 0       # U is no letter of any set
    assert rule.tail_cut(b"N" + b"G" * 20, "G") == 20           # U never starts a suffix


def test_the_maximum_over_the_letters():
    read = b"CT" * 20 + b"G" * 30 + b"A" * 12
    assert rule.tail_cut(read, "A") == 12 and rule.tail_cut(read, "G") == 0
    assert rule.tail_cut(read, "AG") == rule.tail_cut(read, "GA") == 12
    read = b"CT" * 20 + b"G" * 60 + b"AAA" + b"G"   # G: 64 bases with three others; A: nothing
    assert rule.tail_cut(read, "ACGT") == 64 and rule.tail_cut(read, "ACT") == 0


def test_the_one_pass_form_equals_the_quadratic_form():
    rng = np.random.default_rng(5)
    for i in range(400):
        n = int(rng.integers(0, 90))
        r = bytearray(rng.choice(list(b"ACGTNacgt"), size=n, p=[.1, .1, .5, .1, .04, .04, .04, .04, .04]).astype(np.uint8).tobytes())
        for letters in ("G", "ACGT", "CA"):
            for M in (2, 5, 10):
                assert rule.tail_cut_fast(bytes(r), letters, M) == rule.tail_cut(bytes(r), letters, M), (bytes(r), letters, M)
        assert rule.differing_pairs_fast(bytes(r)) == rule.differing_pairs(bytes(r))


def test_cut_ranges_counts():
    reads = [b"ACT" * 10 + b"G" * 20, b"G" * 15, b"ACTACT", b"", b"ACT" * 10 + b"G" * 20]
    ranges = [(0, 50), (0, 15), (0, 6), (0, 0), (3, 40)]
    out, info = rule.cut_ranges(reads, ranges, "G")
    assert out == [(0, 30), (0, 0), (0, 6), (0, 0), (3, 30)]
    assert info == dict(reads_seen=5, bases_seen=50 + 15 + 6 + 37, reads_cut=3, bases_cut=20 + 15 + 10, reads_emptied=1)


@pytest.mark.parametrize("read, D, drop", [(b"AA", 0, True), (b"AC", 1, False), (b"NNNN", 0, True), (b"ANNA", 2, False), (b"A" * 10 + b"C" * 10, 1, True)])
def test_the_worked_cases_of_the_complexity_rule(read, D, drop):
    assert rule.differing_pairs(read) == D == rule.differing_pairs_fast(read)
    assert rule.dropped(read, 30) == drop


def test_the_threshold_met_exactly_and_short_reads():
    exact, below = b"A" * 8 + b"CAC", b"A" * 9 + b"CA"  # ten pairs: 100 * 3 == 30 * 10, and 100 * 2 < 30 * 10
    assert rule.differing_pairs(exact) == 3 and not rule.dropped(exact, 30)
    assert rule.differing_pairs(below) == 2 and rule.dropped(below, 30)
    assert rule.dropped(exact, 31) and not rule.dropped(below, 20)
    for read in (b"", b"A", b"N"):  # L = 0 and 1 are kept whatever P
        assert not rule.dropped(read, 100)
    assert rule.dropped(b"AA", 1) and not rule.dropped(b"Aa" + b"C", 50) and rule.dropped(b"AaC", 51)  # L = 2; case
    assert not rule.dropped(b"ACGT" * 5, 100) and rule.dropped(b"ACGT" * 5 + b"T", 100)
    info, keep = rule.census([b"AA", b"AC", b"AA", b""], [True, True, False, True], 30)
    assert keep == [False, True, False, True] and info == dict(reads_seen=3, bases_seen=4, reads_dropped=1, bases_dropped=2)


# ---- the executables' arguments: usage errors, exit 2, before anything is opened ---------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "drprg_amd", "bin")

BAD = [
    (["--poly-tail", "GX"], "--poly-tail"),
    (["--poly-tail", "GG"], "--poly-tail"),
    (["--poly-tail", "Gg"], "--poly-tail"),
    (["--poly-tail", ""], "--poly-tail"),
    (["--poly-tail", "G", "--poly-min-len", "1"], "--poly-min-len"),
    (["--poly-tail", "G", "--poly-min-len", "256"], "--poly-min-len"),
    (["--poly-tail", "G", "--poly-min-len", "ten"], "--poly-min-len"),
    (["--poly-min-len", "12"], "--poly-min-len without --poly-tail"),
    (["--min-complexity", "0"], "--min-complexity"),
    (["--min-complexity", "101"], "--min-complexity"),
    (["--min-complexity", "30.5"], "--min-complexity"),
    (["--min-complexity", "-3"], "--min-complexity"),
]


@pytest.mark.parametrize("exe, head", [("pandora", ["map"]), ("pandora", ["discover"]), ("drprg", ["predict", "-x", "nowhere", "-i", "nothing.fq"])])
def test_the_executables_refuse_bad_arguments(exe, head):
    path = os.path.join(BIN, exe)
    for extra, named in BAD:
        r = subprocess.run([path] + head + extra + (["prg", "reads"] if exe == "pandora" else []), capture_output=True, text=True)
        assert r.returncode == 2 and named in r.stderr, (exe, extra, r.returncode, r.stderr)
    for flag in ("--poly-tail", "--poly-min-len", "--min-complexity"):  # a flag without its value
        r = subprocess.run([path] + head + [flag], capture_output=True, text=True)
        assert r.returncode == 2, (flag, r.stderr)
    r = subprocess.run([path, head[0], "--help"], capture_output=True, text=True)
    assert "--poly-tail LETTERS" in r.stderr and "--poly-min-len M" in r.stderr and "--min-complexity P" in r.stderr


def test_the_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "drprg_hip.h")).read()
    assert "int drprg_hip_set_poly_trim(drprg_hip_ctx* ctx, const char* letters, uint32_t min_len);" in text
    assert "int drprg_hip_poly_trim_info(drprg_hip_ctx* ctx, uint64_t out[5]);" in text
    assert "int drprg_hip_set_min_complexity(drprg_hip_ctx* ctx, uint32_t percent);" in text
    assert "int drprg_hip_complexity_info(drprg_hip_ctx* ctx, uint64_t out[4]);" in text
    assert "int drprg_hip_poly_trim_device(" in text and "int drprg_hip_complexity_device(" in text
    assert "poly tails" in text.lower() and "read complexity" in text.lower()
    lib_py = open(os.path.join(ROOT, "drprg_amd", "_lib.py")).read()
    for name in ("drprg_hip_set_poly_trim", "drprg_hip_poly_trim_info", "drprg_hip_poly_trim_device", "drprg_hip_set_min_complexity",
                 "drprg_hip_complexity_info", "drprg_hip_complexity_device"):
        assert f'"{name}"' in lib_py, name


def test_the_fixtures_hold_what_they_are_for():
    reads, ranges = rule.kernel_batch()
    cut, info = rule.cut_ranges(reads, ranges, "G")
    starts = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    first = [int(starts[i]) + y for i, ((x, y0), (_, y)) in enumerate(zip(ranges, cut)) if y != y0]  # every cut tail's first base, in the block
    for mod in (rule.WORD, rule.LANE):
        assert {mod - 1, 0, 1} <= {p % mod for p in first}
    assert max(y0 - y for (_, y0), (_, y) in zip(ranges, cut)) >= 70_000 and info["reads_emptied"] > 5 and info["reads_cut"] > 100
    assert cut[-1][1] < len(reads[-1]) and any(x for x, _ in ranges)
    all4, info4 = rule.cut_ranges(reads, ranges, "ACGT")
    assert info4["reads_cut"] > info["reads_cut"] and any(b"N" in r[y:y0] for r, (_, y0), (_, y) in zip(reads, ranges, cut))
    plain, _ = rule.kernel_batch(listed=False)
    assert all(b in b"ACGTacgt" for b in b"".join(plain)) and [len(r) for r in plain] == [len(r) for r in reads]
    creads = rule.complexity_batch()
    info, keep = rule.census(creads, [True] * len(creads))
    assert 20 < info["reads_dropped"] < len(creads) - 100 and max(len(r) for r in creads) >= 70_000
