"""The mate-merging rule (include/drprg_hip.h "mate merging") against hand-worked cases and its own algebra, and the usage errors of both
executables.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import pair_merge_rule as rule
import pair_overlap_rule as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "drprg_amd", "bin")
_COMP = bytes.maketrans(b"ACGTacgtN", b"TGCAtgcaN")
_ACGT = np.frombuffer(b"ACGT", np.uint8)
A20 = b"ACGTTGCATGCAAGCTTAGC"  # 20 letters without a repeat of 8


def rc(s):
    return s.translate(_COMP)[::-1]


def merged(a, B, O=8, e=0):
    """(d, M) of a and the second mate whose reverse complement is B"""
    d = po.judge(a, rc(B), O, e)[0]
    return d, rule.merge(a, rc(B), d)[0]


def test_the_five_kinds_of_column_by_hand():
    a = bytearray(A20[:16])           # columns 4 .. 15 are covered by both
    B = bytearray(A20[4:20])          # B begins at a[4]: d = 4, I = 20
    a[5], B[2] = ord("n"), ord("N")   # column 5: a unknown, B known (filled); column 6: B unknown, a known (filled)
    a[9], B[5] = ord("N"), ord("R")   # column 9: unknown in both
    B[8] = ord("C")                   # column 12: a holds 'A' -- a disagreement
    d = po.judge(bytes(a), rc(bytes(B)), 8, 250)[0]  # (9 columns with both bases known, one differs)
    assert d == 4
    M, kinds, kind = rule.merge(bytes(a), rc(bytes(B)), d)
    want = bytearray(A20)
    want[9], want[12] = ord("N"), ord("N")
    assert M == bytes(want)
    assert kinds == [12 - 4, 1, 2, 1] and sum(kinds) == 12
    assert kind[:4].tolist() == [-1] * 4 and kind[16:].tolist() == [-1] * 4 and kind[5] == 2 and kind[6] == 2 and kind[9] == 3 and kind[12] == 1


def test_lower_case_merges_to_upper_case_and_an_unknown_base_of_one_mate_alone_stays():
    a, B = A20[:14].lower(), bytearray(A20[4:])
    B[15] = ord("N")  # behind a's end: b alone covers it
    d, M = merged(a, bytes(B))
    want = bytearray(A20)
    want[19] = ord("N")
    assert d == 4 and M == bytes(want)


@pytest.mark.parametrize("shape", ["d < 0", "d = 0", "0 < d", "d + Lb < La"])
def test_an_error_free_fragment_merges_back_to_the_fragment(shape):
    rng = np.random.default_rng(5)
    for L in (40, 64, 150):
        frag = rng.choice(_ACGT, size=L).tobytes()
        junk = lambda n: rng.choice(_ACGT, size=n).tobytes()
        if shape == "d < 0":      # both mates read through: a = frag + adapter, B = adapter + frag
            a, B, d = frag + junk(9), junk(7) + frag, -7
        elif shape == "d = 0":    # both mates are the fragment
            a, B, d = frag, frag, 0
        elif shape == "0 < d":    # the fragment is longer than either mate
            a, B, d = frag[:L - 11], frag[13:], 13
        else:                     # B lies inside a, which reads through: the fragment ends where B ends
            a, B, d = frag + junk(10), frag[6:], 6
        got_d, M = merged(a, B, O=8)
        assert (got_d, M) == (d, frag), (shape, L)


def _random_pairs(seed, n=160):
    rng = np.random.default_rng(seed)
    side1, side2 = [], []
    for s in range(n):
        La, Lb = int(rng.integers(8, 90)), int(rng.integers(8, 90))
        if s % 4 == 3:  # unrelated, orphans, too long
            a, B = rng.choice(_ACGT, size=La).tobytes(), rng.choice(_ACGT, size=Lb).tobytes()
            if s % 16 == 3:
                a = b""
            if s % 16 == 7:
                B = rng.choice(_ACGT, size=1025).tobytes()
        else:
            d = int(rng.integers(-(Lb - 8), La - 7))
            lo, hi = min(0, d), max(La, Lb + d)
            mol = rng.choice(_ACGT, size=hi - lo)
            a, B = bytearray(mol[-lo:-lo + La].tobytes()), bytearray(mol[d - lo:d - lo + Lb].tobytes())
            for m in (a, B):
                for p in rng.integers(0, len(m), size=int(rng.integers(0, 3))):
                    m[p] = ord("N") if rng.random() < 0.5 else b"ACGT"[int(rng.integers(0, 4))]
            a, B = bytes(a), bytes(B)
        side1.append(a)
        side2.append(rc(B))
    return side1, side2


def test_the_counts_algebra():
    for seed, O, e in ((1, 8, 100), (2, 12, 50), (3, 8, 250)):
        side1, side2 = _random_pairs(seed)
        shifts, new1, new2, c12, c8 = rule.run(side1, side2, O, e)
        cut = po.run(side1, side2, O, e, False)
        clip = po.run(side1, side2, O, e, True)
        assert shifts == cut[0] == clip[0] and c8["pairs_merged"] == c12["pairs_overlapping"] > 40
        assert c12["bases_clipped"] == clip[3]["bases_clipped"] == c8["columns_both"]
        assert c12["bases_cut"] == cut[3]["bases_cut"] and c12["bases_kept"] == clip[3]["bases_kept"]
        assert sum(c8[k] for k in rule.KINDS) == c8["columns_both"] and min(c8[k] for k in rule.KINDS[:3]) > 0
        assert c12["bases_kept"] == c12["bases_before"] - c12["bases_cut"] - c8["columns_both"]
        assert c12["reads_emptied"] == c8["pairs_merged"] and c12["reads"] == cut[3]["reads"] and c12["pairs"] == len(side1)
        for k in ("pairs_judged", "orphans", "pairs_too_long", "pairs_overlapping", "pairs_read_through", "bases_before"):
            assert c12[k] == cut[3][k]
        # the file the run stands for: as many reads as before, the merged reads in a's place, bases_kept bases
        f = rule.merged_file(new1, new2)
        assert len(f) == len(side1) + len(side2) == c12["reads"] and sum(len(r) for r in f) == c12["bases_kept"]
        lens = [len(m) for d, m in zip(shifts, new1) if d > po.NOT_JUDGED]
        assert sum(lens) == c8["bases_merged"] and max(lens) == c8["longest_merged"]
        assert all(b == b"" for d, b in zip(shifts, new2) if d > po.NOT_JUDGED)
        assert all((a, b) == (x, y) for d, a, b, x, y in zip(shifts, new1, new2, side1, side2) if d <= po.NOT_JUDGED)


@pytest.mark.parametrize("argv, text", [
    (["--pair-merge"], "--pair-merge belongs to --mate"),
    (["--mate", "m.fq", "--pair-merge", "--pair-clip-overlap"], "--pair-merge and --pair-clip-overlap are alternatives"),
])
def test_usage_errors_exit_2(argv, text):
    for exe in ([os.path.join(BIN, "drprg"), "predict", "-x", "idx", "-i", "r.fq"], [os.path.join(BIN, "pandora"), "map", "dr.prg", "r.fq"]):
        r = subprocess.run(exe + argv, capture_output=True, text=True)
        assert r.returncode == 2 and text in r.stderr, (exe[0], argv, r.returncode, r.stderr)
