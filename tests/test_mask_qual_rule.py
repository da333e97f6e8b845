"""Base masking's rule (tests/mask_qual_rule.py) on hand-written cases, the two executables' usage errors for --mask-qual, and the header's
declaration of the setting.  No GPU is needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import mask_qual_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_threshold_edges():
    assert rule.masked(b"ACGT", [9, 10, 11, 0], 10) == b"NCGN"          # q = Q - 1 is masked, q = Q is not
    assert rule.masked(b"ACGT", [0, 1, 2, 93], 1) == b"NCGT"            # Q = 1: quality 0 alone
    assert rule.masked(b"ACGT", [92, 93, 0, 93], 93) == b"NCNT"         # Q = 93: everything below the top
    assert rule.masked(b"", [], 10) == b""
    assert rule.masked(b"acgt", [2, 35, 35, 2], 10) == b"NcgN"          # the letter N, whatever the case was
    for bad_q in (0, 94):
        with pytest.raises(AssertionError):
            rule.masked(b"A", [35], bad_q)
    with pytest.raises(AssertionError):
        rule.masked(b"A", [94], 10)


def test_a_reverse_read_is_judged_by_the_mirrored_byte():
    # stored order 2, 35, 35, 35, 35: the LAST base of the read is the low one
    assert rule.masked(b"ACGTA", [2, 35, 35, 35, 35], 10, reverse=True) == b"ACGTN"
    assert rule.masked(b"ACGTA", [2, 35, 35, 35, 35], 10) == b"NCGTA"
    assert rule.masked(b"ACGTAC", [35, 3, 35, 35, 35, 9], 10, reverse=True) == b"NCGTNC"


def test_letters_that_are_no_bases():
    assert rule.masked(b"ARGNT", [35, 2, 35, 2, 35], 10) == b"ANGNT"   # a low-quality R becomes N; an N stays N
    assert rule.masked(b"ARGNT", [35, 35, 35, 35, 35], 10) == b"ARGNT"  # at quality Q or more nothing is touched, whatever it is
    reads, quals = [b"ARGNT", b"ACGT", b"", b"an"], [[35, 2, 35, 2, 2], [35] * 4, [], [2, 35]]
    assert rule.info(reads, quals, 10) == dict(reads_seen=4, bases_seen=11, reads_masked=2, bases_masked=2, bases_already_unknown=2)
    assert rule.info(reads, quals, 10, rev=[True, False, False, True]) == dict(reads_seen=4, bases_seen=11, reads_masked=2, bases_masked=1, bases_already_unknown=3)
    assert rule.info(reads, quals, 1) == dict(reads_seen=4, bases_seen=11, reads_masked=0, bases_masked=0, bases_already_unknown=0)


def test_the_fixtures_hold_what_the_gpu_tests_need():
    reads, quals, rev = rule.kernel_batch()
    L = [len(r) for r in reads]
    n = sum(L)
    assert {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65} <= set(L) and max(L) > rule.TILE and 3 * rule.TILE < n < 4 * rule.TILE
    assert all(len(q) == len(r) for q, r in zip(quals, reads)) and any(rev) and not all(rev)
    m = [rule.masked(r, q, rule.Q, v) for r, q, v in zip(reads, quals, rev)]
    flat, was = b"".join(m), b"".join(reads)
    assert flat[0:1] == b"N" and flat[-1:] == b"N" and any(x == b"N" * len(x) and len(x) > 100 for x in m) and any(x == r and len(x) > 100 for x, r in zip(m, reads))
    listed = [p for p in range(n) if was[p] not in rule.ACGT]
    after = [p for p in range(n) if flat[p] not in rule.ACGT]
    low = set(after) - set(listed)
    assert listed and set(listed) <= set(after) and len(after) > len(listed) + 500
    assert any(p + 1 in low or p - 1 in low for p in listed)  # a listed base of good quality beside a masked one ...
    info = rule.info(reads, quals, rule.Q, rev)
    assert info["bases_already_unknown"] >= 2 and info["bases_masked"] == len(low)  # ... and listed bases of low quality
    for edge in (0, rule.WORD - 1):
        assert any(p % rule.WORD == edge for p in low)
    for edge in (0, rule.LANE - 1):
        assert any(p % rule.LANE == edge for p in low)
    assert any(p % rule.TILE == rule.TILE - 1 for p in low) and any(p % rule.TILE == 0 and p for p in low)  # either side of a tile edge
    assert len({p // rule.TILE for p in after}) == 4  # the list's chunks: every workgroup of the emit writes some of it
    # a reversed read whose stored qualities are asymmetric: mirrored it is masked elsewhere
    assert any(v and rule.masked(r, q, rule.Q, True) != rule.masked(r, q, rule.Q) for r, q, v in zip(reads, quals, rev))
    r2, q2, _ = rule.kernel_batch(listed=False)
    assert all(b in rule.ACGT for b in b"".join(r2)) and [len(r) for r in r2] == L
    r3, q3, v3 = rule.kernel_batch(listed=False, low=False)
    assert rule.info(r3, q3, rule.Q, v3)["reads_masked"] == 0
    for sample in (rule.small_sample(), rule.big_sample()):
        lengths, q = sample
        low = sum(int((x < rule.Q).sum()) for x in q)
        assert 0.03 * sum(lengths) < low < 0.07 * sum(lengths) and min(int(x.min()) for x in q if x.size) >= 2
    assert sum(rule.small_sample()[0]) < 750_000 < sum(rule.big_sample()[0]) // 2


@pytest.mark.parametrize("exe,head", [("pandora", ["map"]), ("drprg", ["predict", "-x", "nowhere", "-i", "nothing.fq"])])
def test_usage_errors(exe, head):
    path = os.path.join(ROOT, "drprg_amd", "bin", exe)
    for bad in ("0", "94", "12.5", "x", "-3", ""):
        r = subprocess.run([path] + head + ["--mask-qual", bad] + (["prg", "reads"] if exe == "pandora" else []), capture_output=True, text=True)
        assert r.returncode == 2 and "--mask-qual" in r.stderr, (exe, bad, r.returncode, r.stderr)
    r = subprocess.run([path] + head + ["--mask-qual"], capture_output=True, text=True)
    assert r.returncode == 2, r.stderr
    r = subprocess.run([path, "map", "--help"] if exe == "pandora" else [path, "predict", "--help"], capture_output=True, text=True)
    assert "--mask-qual Q" in r.stderr


def test_the_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "drprg_hip.h")).read()
    assert re.search(r"int drprg_hip_set_base_mask\(drprg_hip_ctx\* ctx, uint32_t min_qual\);", text)
    assert re.search(r"int drprg_hip_base_mask_info\(drprg_hip_ctx\* ctx, uint64_t out\[5\]\);", text)
    assert "int drprg_hip_base_mask_device(" in text and "base masking" in text.lower()
    lib_py = open(os.path.join(ROOT, "drprg_amd", "_lib.py")).read()
    for name in ("drprg_hip_set_base_mask", "drprg_hip_base_mask_info", "drprg_hip_base_mask_device"):
        assert f'"{name}"' in lib_py, name
