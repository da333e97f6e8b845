"""The decoy screen's rule (tests/decoy_rule.py; include/drprg_hip.h "decoy screen") held to its own properties, and the usage errors of the
executables' --decoy flags.  No GPU."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import decoy_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seq(seed, n):
    return rule.random_dna(np.random.default_rng(seed), n)


@pytest.mark.parametrize("k", [9, 15, 16, 31])
def test_the_fast_enumeration_is_the_rule_window_by_window(k):
    s = bytearray(_seq(1, 300))
    s[0:1] = b"N"
    s[100:103] = b"acg"
    s[150:151] = b"R"
    s[-1:] = b"n"
    assert rule.kmers(s, k) == rule.kmers_plain(s, k)
    assert rule.kmers(s[:k - 1], k) == [] and len(rule.kmers(s[1:k + 1], k)) == 1
    assert rule.code_of("ACGT") == 0b00011011 and rule.revcomp_code(rule.code_of("AACG"), 4) == rule.code_of("CGTT")
    assert rule.canonical(rule.code_of("TTTT"), 4) == 0


@pytest.mark.parametrize("k", [9, 31])
def test_a_read_and_its_reverse_complement_count_alike(k):
    decoy, other = _seq(2, 400), _seq(3, 400)
    D = rule.decoy_set([decoy], k)
    for read in (decoy[50:250], other[:200], decoy[:120] + other[:90], decoy[:60] + b"N" + decoy[61:140]):
        V, H = rule.counts(read, D, k)
        assert (V, H) == rule.counts(rule.revcomp(read), D, k) and V > 0
    assert rule.counts(decoy[50:250], D, k) == (201 - k, 201 - k)
    assert rule.counts(other[:200], D, k)[1] == 0


def test_a_window_with_an_n_counts_in_neither():
    k = 15
    decoy = _seq(4, 200)
    D = rule.decoy_set([decoy], k)
    read = bytearray(decoy[20:120])
    assert rule.counts(read, D, k) == (86, 86)
    read[40:41] = b"N"  # the fifteen windows that hold it are gone from V and from H
    assert rule.counts(read, D, k) == (71, 71)
    read[0:1] = b"N"
    read[-1:] = b"N"  # the first and the last window
    assert rule.counts(read, D, k) == (69, 69)
    assert rule.counts(b"N" * 40, D, k) == (0, 0) and not rule.drops(0, 0, 1, 1)  # V == 0: kept


def test_no_kmer_spans_two_records_and_copies_change_nothing():
    k = 15
    a, b = _seq(5, 100), _seq(6, 100)
    D = rule.decoy_set([a, b], k)
    joined = rule.decoy_set([a + b], k)
    across = {c for c in rule.kmers(a[-(k - 1):] + b[:k - 1], k)}
    assert len(D) == 2 * 86 and len(joined) == len(D) + k - 1 and not (across & D) and across <= joined
    assert rule.decoy_set([a, b, a, rule.revcomp(b), a.lower()], k) == D
    assert rule.decoy_set([a[:k - 1]], k) == set() and rule.windows_of([a, b, a[:k - 1]], k) == 172
    assert [rule.slots_for(w) for w in (0, 1, 4, 5, 8, 9, 12, 2000)] == [8, 8, 8, 16, 16, 32, 32, 4096]


def test_the_files_are_read_record_by_record(tmp_path):
    a, b = _seq(7, 90), _seq(8, 70)
    plain, gz = tmp_path / "d.fa", tmp_path / "d.fa.gz"
    text = b">a first\n" + a[:60] + b"\n" + a[60:] + b"\n>b\n" + b + b"\n"
    plain.write_bytes(text)
    with gzip.open(gz, "wb") as fh:
        fh.write(text)
    assert rule.records_of(plain) == rule.records_of(gz) == [a, b]


def test_the_boundary_drops_and_one_hit_fewer_keeps():
    for f, V in ((500, 100), (1, 1000), (1000, 37), (333, 3)):
        H = -(-f * V // 1000)  # the smallest H with 1000 H >= f V
        assert rule.drops(V, H, f, 1) and not rule.drops(V, H - 1, f, 1), (f, V)
    assert 1000 * 50 == 500 * 100 and rule.drops(100, 50) and not rule.drops(100, 49)
    assert not rule.drops(100, 2, 1, 3) and rule.drops(100, 3, 1, 3)  # M decides where f does not
    # a chimera cut to the boundary, and one window short of it
    k = 15
    decoy, other = _seq(9, 300), _seq(10, 300)
    D = rule.decoy_set([decoy], k)
    on = rule.chimera(decoy, other, k, 50, 100)
    below = rule.chimera(decoy, other, k, 49, 100)
    assert rule.counts(on, D, k) == (100, 50) and rule.counts(below, D, k) == (100, 49)
    c, keep = rule.census([on, below, decoy[:80], b""], [True, True, False, True], D, k)
    assert keep == [False, True, False, True]
    assert c == dict(reads_seen=3, bases_seen=228, reads_dropped=1, bases_dropped=114, valid=200, hits=99)


@pytest.mark.parametrize("exe", ["pandora", "drprg"])
def test_usage_errors_exit_2_and_need_no_device(tmp_path, exe):
    path = os.path.join(ROOT, "drprg_amd", "bin", exe)
    head = [path, "map"] if exe == "pandora" else [path, "predict", "-x", str(tmp_path), "-i", "reads.fq"]
    tail = ["dr.prg", "reads.fq"] if exe == "pandora" else []
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a usage error comes before one is looked for)
    D = ["--decoy", "d.fa"]
    for flags, word in ((D * 9, "--decoy"), (["--decoy", ""], "--decoy"), (["--decoy-k", "21"], "--decoy-k"), (["--decoy-min-frac", "0.5"], "--decoy-min-frac"),
                        (["--decoy-min-kmers", "2"], "--decoy-min-kmers"), (D + ["--decoy-k", "8"], "--decoy-k"), (D + ["--decoy-k", "32"], "--decoy-k"),
                        (D + ["--decoy-k", "x"], "--decoy-k"), (D + ["--decoy-min-frac", "0"], "--decoy-min-frac"), (D + ["--decoy-min-frac", "1.001"], "--decoy-min-frac"),
                        (D + ["--decoy-min-frac", "0.1234"], "--decoy-min-frac"), (D + ["--decoy-min-frac", "-0.5"], "--decoy-min-frac"),
                        (D + ["--decoy-min-frac", "half"], "--decoy-min-frac"), (D + ["--decoy-min-kmers", "0"], "--decoy-min-kmers"),
                        (D + ["--decoy-min-kmers", "-1"], "--decoy-min-kmers")):
        r = subprocess.run(head + flags + tail, capture_output=True, text=True, env=env)
        assert r.returncode == 2 and word in r.stderr, (flags, r.returncode, r.stderr)
