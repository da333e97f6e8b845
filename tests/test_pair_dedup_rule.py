"""The duplicate-pair rule (include/drprg_hip.h "duplicate pairs") against a brute-force comparison and its defining cases, and the usage
errors of both executables.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import dedup_rule as reads_rule
import pair_dedup_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "drprg_amd", "bin")
A = b"ACGTTGCATGCAAGCTTAGC"
B = b"TTGACCATGGATCCAAGTCA"
C = b"GGATCCTTAACGTGCATAGA"


def keep(units):
    return rule.run([u[0] for u in units], [u[1] for u in units])[0]


def test_the_rule_equals_the_brute_force_comparison():
    rng = np.random.default_rng(5)
    pool = [bytes(rng.choice(np.frombuffer(b"ACGTacgtNR", np.uint8), size=int(L)).tobytes()) for L in rng.integers(0, 40, size=24)] + [b"", None]
    side1 = [pool[int(i)] for i in rng.integers(0, len(pool), size=400)]
    side2 = [pool[int(i)] for i in rng.integers(0, len(pool), size=400)]
    for ident in (rule.unit_identity, rule.unit_identity_fast):
        k, copies, cnt, lv, f1, f2 = rule.run(side1, side2, identity=ident)
        assert k == rule.brute_keep(side1, side2)
        assert 50 < cnt["units_dropped"] < 350 and cnt["units_dropped"] == k.count(0)
        # copies: the size of the class of every kept unit with bases, by counting
        ids = [rule.unit_identity(a, b) for a, b in zip(side1, side2)]
        for s in range(400):
            want = ids.count(ids[s]) if k[s] and rule.has_bases(side1[s], side2[s]) else 0
            assert copies[s] == want
        assert sum(c * n for c, n in enumerate(lv[:31], 1)) + sum(c for c in copies if c >= 32) == cnt["units_with_bases"]
        assert sum(lv) == cnt["units_with_bases"] - cnt["units_dropped"]
        # flags: both mates go, or neither; a mate of no bases always stays; a mate that is not resident has none
        for a, b, kk, x, y in zip(side1, side2, k, f1, f2):
            assert (x is None) == (a is None) and (y is None) == (b is None)
            for m, f in ((a, x), (b, y)):
                if m is not None:
                    assert f == (1 if kk or len(m) == 0 else 0)
        assert cnt["reads_kept"] == sum(f for f in f1 + f2 if f) and cnt["reads_before"] == sum(m is not None for m in side1 + side2)
        assert cnt["bases_kept"] == sum(len(m) for m in rule.kept_reads(side1, side2, f1, f2))


def test_the_defining_cases():
    assert keep([(A, B), (A, C)]) == [1, 1]  # same A, different B
    assert keep([(A, B), (C, B)]) == [1, 1]  # different A, same B
    assert keep([(A, B), (B, A)]) == [1, 1]  # the other orientation is another unit
    assert keep([(A, B), (A.lower(), B)]) == [1, 0] and keep([(A, B), (A, B.lower())]) == [1, 0]  # letters without case
    n, r = A[:7] + b"N" + A[8:], A[:7] + b"R" + A[8:]
    assert keep([(n, B), (r, B)]) == [1, 0] and keep([(B, n), (B, r)]) == [1, 0]  # unknown is unknown
    other = A[:8] + b"N" + A[9:]
    assert keep([(n, B), (other, B)]) == [1, 1] and keep([(A, B), (n, B)]) == [1, 1]  # an unknown base at another place, or only in one
    assert keep([(A, B), (A + b"A", B)]) == [1, 1] and keep([(A, B), (A, B[:-1])]) == [1, 1]  # lengths
    # the empty read: dropped, emptied and never there are one thing
    assert keep([(A, b""), (A, None)]) == [1, 0] and keep([(A, None), (A, b"")]) == [1, 0]
    assert keep([(None, B), (b"", B)]) == [1, 0]
    assert keep([(A, None), (None, A)]) == [1, 1] and keep([(A, B), (A, None)]) == [1, 1]
    assert keep([(b"", b""), (None, None), (b"", None), (A, B), (b"", b"")]) == [1, 1, 1, 1, 1]  # no bases: never dropped
    # the first copy wins, and a copy of a dropped copy is a copy of the first
    k, copies = rule.run([A, C, A, A, C], [B, B, B, B, B])[:2]
    assert k == [1, 1, 0, 0, 0] and copies == [3, 2, 0, 0, 0]


def test_flags_of_a_dropped_unit():
    k, copies, cnt, lv, f1, f2 = rule.run([A, A, A, None, b""], [b"", None, b"", B, B])
    assert k == [1, 0, 0, 1, 0] and f1 == [1, 0, 0, None, 1] and f2 == [1, None, 1, 1, 0]
    assert cnt == dict(units=5, units_with_bases=5, units_both_mates=0, units_dropped=3, reads_before=8, bases_before=100, reads_kept=5, bases_kept=40)
    assert rule.kept_reads([A, A, A, None, b""], [b"", None, b"", B, B], f1, f2) == [A, b"", b"", b"", B]


def test_the_level_bins_at_31_and_32_copies():
    side1 = [A] * 31 + [B] * 32 + [C] * 33 + [A + B]
    side2 = [B] * 31 + [C] * 32 + [A] * 33 + [b""]
    k, copies, cnt, lv = rule.run(side1, side2)[:4]
    assert [copies[0], copies[31], copies[63], copies[96]] == [31, 32, 33, 1] and sum(copies) == 97
    assert lv == [1] + [0] * 29 + [1, 2] and cnt["units_dropped"] == 93


def test_the_key_keeps_the_orientations_apart():
    fin = reads_rule.fin
    assert rule.unit_key(None, None) == rule.unit_key(b"", b"") == (fin(rule.G) + fin(2 * rule.G)) & rule.MASK64
    assert rule.unit_key(A, B) != rule.unit_key(B, A) and rule.unit_key(A, b"") != rule.unit_key(b"", A)
    assert rule.unit_key(A, B) == rule.unit_key(A.lower(), B) == (fin(reads_rule.key(A) + rule.G) + fin(reads_rule.key(B) + 2 * rule.G)) & rule.MASK64


@pytest.mark.parametrize("argv, text", [
    (["--dedup-pairs"], "--dedup-pairs belongs to --mate"),
    (["--mate", "m.fq", "--dedup-pairs", "--dedup"], "--dedup-pairs and --dedup are alternatives"),
    (["--dedup", "--dedup-pairs", "--mate", "m.fq"], "--dedup-pairs and --dedup are alternatives"),
])
def test_usage_errors_exit_2(argv, text):
    for exe in ([os.path.join(BIN, "drprg"), "predict", "-x", "idx", "-i", "r.fq"], [os.path.join(BIN, "pandora"), "map", "dr.prg", "r.fq"]):
        r = subprocess.run(exe + argv, capture_output=True, text=True)
        assert r.returncode == 2 and text in r.stderr, (exe[0], argv, r.returncode, r.stderr)


def test_help_names_the_flag():
    for exe in ([os.path.join(BIN, "drprg"), "predict", "--help"], [os.path.join(BIN, "pandora"), "--help"]):
        r = subprocess.run(exe, capture_output=True, text=True)
        assert "--dedup-pairs" in r.stdout + r.stderr, exe
