"""The mate-overlap rule (include/drprg_hip.h "mate overlap") against hand-worked cases, and the usage errors of both executables.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import pair_overlap_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "drprg_amd", "bin")
_COMP = bytes.maketrans(b"ACGTacgtN", b"TGCAtgcaN")
A20 = b"ACGTTGCATGCAAGCTTAGC"  # 20 letters without a repeat of 8


def rc(s):
    return s.translate(_COMP)[::-1]


def judge(a, B, O=8, e=0, clip=False):
    """a and B as the rule lays them over each other: the second mate is B's reverse complement"""
    return rule.judge(a, rc(B), O, e, clip)


def counts(a, B, d):
    return [t for t in rule.shift_counts_plain(rule.codes(a), rule.codes(rc(B))) if t[0] == d][0]


def test_the_two_ways_to_count_agree():
    rng = np.random.default_rng(3)
    for La, Lb in ((1, 1), (1, 9), (9, 1), (17, 40), (150, 151), (64, 1024)):
        a, b = rng.integers(0, 5, size=La).astype(np.uint8), rng.integers(0, 5, size=Lb).astype(np.uint8)
        assert rule.shift_counts(a, b) == rule.shift_counts_plain(a, b)
        assert [t[0] for t in rule.shift_counts_plain(a, b)] == list(range(-(Lb - 1), La))


def test_a_positive_shift_is_a_plain_overlap():
    B = A20[8:] + b"GGATCCAA"  # B begins at a[8]: 12 columns
    assert counts(A20, B, 8) == (8, 12, 0)
    assert judge(A20, B) == (8, 20, 20)  # the insert (28) is longer than both mates: nothing is cut
    assert judge(A20, B, clip=True) == (8, 20, 8)  # b keeps the 8 bases a does not cover


def test_shift_zero():
    assert judge(A20, A20) == (0, 20, 20)
    assert judge(A20, A20, clip=True) == (0, 20, 0)  # all of b lies under a: a read of no bases


def test_a_negative_shift_is_a_read_through():
    F = A20[:12]
    a, B = F + b"TTTTTTTT", b"CCCCCCCC" + F  # the insert is F: both mates read 8 bases of adapter behind it
    assert counts(a, B, -8) == (-8, 12, 0)
    assert judge(a, B) == (-8, 12, 12)
    assert judge(a, B, clip=True) == (-8, 12, 0)


def test_a_mate_contained_in_the_other_and_unequal_lengths():
    a = A20 + b"GATTACAGAT"
    assert judge(a, a[5:15]) == (5, 15, 10)  # B ends at a[15]: a has read 15 bases past the insert's end
    assert judge(a, a[5:15], clip=True) == (5, 15, 0)
    F = A20[:12]
    assert judge(F, b"GGATCCAAGGTCA" + F) == (-13, 12, 12)  # La 12, Lb 25
    assert judge(F, b"GGATCCAAGGTCA" + F, clip=True) == (-13, 12, 0)


def test_the_overlap_bound_is_sharp():
    B = A20[12:] + b"GGATCCAAGGTC"
    assert counts(A20, B, 12) == (12, 8, 0)
    assert judge(A20, B, O=8)[0] == 12
    assert judge(A20, B, O=9) == (rule.NONE, 20, 20)


def test_the_error_bound_is_sharp():
    two, three = bytearray(A20), bytearray(A20)
    for p in (3, 11):
        two[p] = three[p] = ord("A") if A20[p] != ord("A") else ord("C")
    three[18] = ord("A")
    assert counts(A20, bytes(two), 0) == (0, 20, 2) and counts(A20, bytes(three), 0) == (0, 20, 3)
    assert judge(A20, bytes(two), e=100)[0] == 0  # 1000 * 2 == 100 * 20
    assert judge(A20, bytes(three), e=100)[0] == rule.NONE
    assert judge(A20, bytes(two), e=99)[0] == rule.NONE


def test_the_three_tie_breaks_in_order():
    P = b"ACGT" * 5
    # 1. the largest c: a period of 4 matches at d = 0, +-4, +-8, ..., and d = 0 has the most columns
    assert [counts(P, P, d)[1:] for d in (0, 4, -4)] == [(20, 0), (16, 0), (16, 0)]
    assert judge(P, P)[0] == 0
    # 3. equal c and x: the largest d.  Four unknown bases at a's front leave 16 known columns at d = 0 and at d = 4
    a = b"NNNN" + b"ACGT" * 4
    assert [counts(a, P, d)[1:] for d in (0, 4, -4, 8)] == [(16, 0), (16, 0), (12, 0), (12, 0)]
    assert judge(a, P, e=100)[0] == 4
    # 2. equal c: the smallest x.  B[1] changed: at d = 0 it lies under an unknown base, at d = 4 it is a difference
    B = b"AGGT" + b"ACGT" * 4
    assert [counts(a, B, d)[1:] for d in (0, 4)] == [(16, 0), (16, 1)]
    assert judge(a, B, e=100)[0] == 0


def test_unknown_bases_are_neither_matches_nor_differences():
    a, B = bytearray(A20), bytearray(A20)
    a[7], B[3] = ord("n"), ord("R")
    assert counts(bytes(a), bytes(B), 0) == (0, 18, 0)
    assert judge(bytes(a), bytes(B), O=18)[0] == 0 and judge(bytes(a), bytes(B), O=19)[0] == rule.NONE
    a[3] = ord("N")  # both unknown in one column: still one column less, not two
    assert counts(bytes(a), bytes(B), 0) == (0, 18, 0)
    # a base a stage in front made unknown counts like any other unknown base
    assert rule.judge(A20, rc(A20), 20, 0)[0] == 0 and rule.judge(A20, rc(A20), 20, 0, unknown_a=(5,))[0] == rule.NONE
    # letters are compared without case
    assert judge(A20.lower(), A20) == (0, 20, 20)


def test_who_is_judged():
    assert rule.judge(b"", A20) == (rule.NOT_JUDGED, 0, 20) and rule.judge(A20, b"") == (rule.NOT_JUDGED, 20, 0)
    long = (A20 * 52)[:1025]
    assert rule.judge(long, rc(long)) == (rule.NOT_JUDGED, 1025, 1025)
    assert rule.judge(long[:1024], rc(long[:1024]), 30, 50)[0] == 0
    s1 = [A20, b"", A20, None, long, A20 + b"TTTT"]
    s2 = [rc(A20), A20, None, A20, rc(long), rc(A20) + b"CCCC"]
    shifts, k1, k2, c = rule.run(s1, s2, 8, 0, False)
    assert shifts == [0, rule.NOT_JUDGED, rule.NOT_JUDGED, rule.NOT_JUDGED, rule.NOT_JUDGED, -4]
    assert k1 == [20, 0, 20, None, 1025, 20] and k2 == [20, 20, None, 20, 1025, 20]
    assert c == dict(pairs=6, pairs_judged=2, orphans=3, pairs_too_long=1, pairs_overlapping=2, pairs_read_through=1, bases_cut=8, bases_clipped=0,
                     reads_emptied=0, reads=10, bases_before=20 * 5 + 2 * 24 + 2 * 1025, bases_kept=20 * 7 + 2 * 1025)
    c = rule.run(s1, s2, 8, 0, True)[3]
    assert c["bases_clipped"] == 40 and c["reads_emptied"] == 2 and c["bases_kept"] == 20 * 5 + 2 * 1025
    assert rule.cut_reads(s1, s2, k1, k2) == [A20, b"", A20, long, A20, rc(A20), A20, A20, rc(long), rc(A20)]


def test_pair_error_is_read_as_thousandths():
    assert [rule.error_milli(t) for t in ("0", "0.05", "0.25", ".1", "0.001")] == [0, 50, 250, 100, 1]
    for bad in ("0.251", "0.0005", "-0.1", "x", "1", "nan"):
        with pytest.raises(ValueError):
            rule.error_milli(bad)


def test_unrelated_reads_do_not_overlap_at_the_defaults():
    """20 000 pairs of independent random 150-base reads: the chance that one shift of 30 columns has at most one difference is
    91 / 4^30, so none qualifies"""
    rng = np.random.default_rng(2024)
    A, B = rng.integers(0, 4, size=(20000, 150)).astype(np.uint8), rng.integers(0, 4, size=(20000, 150)).astype(np.uint8)
    assert int(rule.qualifying_batch(A, B, 30, 50).sum()) == 0


@pytest.mark.parametrize("argv, text", [
    (["--pair-min-overlap", "40"], "--pair-min-overlap belongs to --mate"),
    (["--pair-error", "0.1"], "--pair-error belongs to --mate"),
    (["--pair-clip-overlap"], "--pair-clip-overlap belongs to --mate"),
    (["--mate", "m.fq", "--pair-min-overlap", "7"], "8 .. 1024"),
    (["--mate", "m.fq", "--pair-min-overlap", "1025"], "8 .. 1024"),
    (["--mate", "m.fq", "--pair-min-overlap", "3x"], "8 .. 1024"),
    (["--mate", "m.fq", "--pair-error", "0.251"], "0 .. 0.25"),
    (["--mate", "m.fq", "--pair-error", "0.0501"], "three places"),
    (["--mate", "m.fq", "--pair-error", "-0.1"], "0 .. 0.25"),
    (["--mate"], "needs a value"),
])
def test_usage_errors_exit_2(argv, text):
    for exe in ([os.path.join(BIN, "drprg"), "predict", "-x", "idx", "-i", "r.fq"], [os.path.join(BIN, "pandora"), "map", "dr.prg", "r.fq"]):
        r = subprocess.run(exe + argv, capture_output=True, text=True)
        assert r.returncode == 2 and text in r.stderr, (exe[0], argv, r.returncode, r.stderr)


def test_an_explicit_depth_cap_beside_mate_is_a_usage_error():
    exe = [os.path.join(BIN, "pandora"), "map", "dr.prg", "r.fq", "--mate", "m.fq"]
    r = subprocess.run(exe + ["--max-covg", "300"], capture_output=True, text=True)
    assert r.returncode == 2 and "--mate and --max-covg are alternatives" in r.stderr
    r = subprocess.run(exe + ["--max-covg", "4294967295"], capture_output=True, text=True)  # (no cap: the run goes on to open the PRG)
    assert r.returncode != 2 and "alternatives" not in r.stderr
