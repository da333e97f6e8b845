"""The read filter's rule on the CPU: the literal table of the product against decimal arithmetic, the threshold T, the rule's edges, the
census of the fixtures the GPU tests filter (tests/read_filter_rule.py), and the handling of the settings that needs no device: the C
entry's refusals on a host-only context and the executables' usage errors, which come before any device is opened."""
import os
import re
import subprocess
from decimal import Decimal

import numpy as np
import pytest

import read_filter_rule as rule
from read_filter_rule import KEEP, LONG, LOWQ, SHORT, E, census, fate, fates, qual_milli, threshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 22


def _header_table():
    text = open(os.path.join(ROOT, "drprg_amd", "csrc", "read_qual_piece.h")).read()
    body = re.search(r"RQ_E\[RQ_MAX_QUAL \+ 1\] = \{(.*?)\};", text, re.S).group(1)
    return [int(x) for x in re.findall(r"(\d+)u", body)]


def _host_ctx(tmp_path):
    from drprg_amd import Context
    f = str(tmp_path / "dr.prg")
    open(f, "w").write(">g0\nACGTTGCAAGGCTTAACCGGATATCGCGATTAGGCATCAGT\n")
    return Context(f, 5, 7, device=-1, from_files=False)


def test_the_literal_table_is_the_rounded_error_probability():
    table = _header_table()
    assert len(table) == 94 and table == E
    assert table[0] == 2 ** 31 and table[93] == 1
    for q, e in enumerate(table):
        exact = Decimal(2) ** 31 * Decimal(10) ** (Decimal(-q) / 10)
        assert abs(Decimal(e) - exact) <= Decimal("0.5"), q
    assert all(a > b for a, b in zip(table[:88], table[1:89])) and all(a >= b for a, b in zip(table[88:], table[89:]))


def test_threshold(tmp_path):
    ctx = _host_ctx(tmp_path)
    for q in (7, 10, 20):
        ctx.set_read_filter(min_qual=q)
        assert ctx.read_filter_info()["T"] == E[q] == threshold(q * 1000)
    ctx.set_read_filter(min_qual="12.5")
    T = ctx.read_filter_info()["T"]
    assert abs(T - threshold(12500)) <= 1 and E[13] < T < E[12]
    assert qual_milli("12.5") == 12500 and qual_milli(10) == 10000 and qual_milli("0.001") == 1
    # all zero clears it
    ctx.set_read_filter()
    assert ctx.read_filter_info() == dict(reads_seen=0, bases_seen=0, dropped_short=0, dropped_long=0, dropped_low_qual=0, reads_kept=0, bases_kept=0, T=0)
    ctx.close()


def test_settings_that_contradict_themselves_are_refused(tmp_path):
    from drprg_amd.pandora import DependencyError
    ctx = _host_ctx(tmp_path)
    ctx.set_read_filter(min_len=300, max_len=300, min_qual=93)  # min = max and the highest quality: allowed
    before = ctx.read_filter_info()
    for kw in (dict(min_len=301, max_len=300), dict(min_qual="93.001"), dict(min_len=1, max_len=0, min_qual=94)):
        with pytest.raises(DependencyError) as e:
            ctx.set_read_filter(**kw)
        assert e.value.code == EINVAL, kw
        assert ctx.read_filter_info() == before  # a refused call leaves the settings
    ctx.close()


def test_edges_of_the_rule():
    T = threshold(10000)
    # a read of no bases passes the quality test; the length test decides its fate
    assert fate(0, [], 0, 0, T) == KEEP and fate(0, [], 1, 0, T) == SHORT and fate(0, [], 0, 5, T) == KEEP
    # Q = 0: no quality test at all, whatever the bases say
    assert fate(5, [0] * 5, 0, 0, 0) == KEEP and fate(5, None, 0, 0, 0) == KEEP
    # min = max: exactly that length
    assert [fate(L, None, 300, 300, 0) for L in (299, 300, 301)] == [SHORT, KEEP, LONG]
    # short comes before long comes before quality
    assert fate(3, [0, 0, 0], 4, 2, T) == SHORT and fate(3, [0, 0, 0], 0, 2, T) == LONG and fate(3, [0, 0, 0], 0, 3, T) == LOWQ
    # S = L * T is kept, one unit more is not
    assert fate(400, [10] * 400, 0, 0, T) == KEEP and fate(400, [10] * 399 + [9], 0, 0, T) == LOWQ
    assert fate(1, [93], 0, 0, threshold(93000)) == KEEP and fate(2, [93, 90], 0, 0, threshold(93000)) == LOWQ
    # the mean is that of the error probabilities, not of the Phred values: 40 and 0 average to Q 3, not 20
    assert fate(2, [40, 0], 0, 0, threshold(4000)) == LOWQ and fate(2, [40, 0], 0, 0, threshold(3000)) == KEEP
    # the order of the bases does not matter
    q = np.random.default_rng(1).integers(0, 94, size=500)
    assert rule.qual_sum(q) == rule.qual_sum(q[::-1]) == sum(E[int(x)] for x in q)


@pytest.mark.parametrize("which", ["small", "big"])
def test_census_of_the_gpu_fixtures(which):
    """each of the three rules drops 10-30 % of the reads of the samples the GPU tests filter, and the reads on the threshold are there"""
    lengths, quals = rule.small_sample() if which == "small" else rule.big_sample()
    T = threshold(qual_milli(rule.MIN_QUAL))
    what = fates(lengths, quals, rule.MIN_LEN, rule.MAX_LEN, T)
    c = census((what, lengths))
    n = len(lengths)
    for key in ("dropped_short", "dropped_long", "dropped_low_qual"):
        assert 0.10 <= c[key] / n <= 0.30, (key, c)
    assert c["reads_kept"] + c["dropped_short"] + c["dropped_long"] + c["dropped_low_qual"] == n and 0.3 < c["reads_kept"] / n < 0.7
    assert (sum(lengths) < 750_000) == (which == "small") and (which == "small" or sum(lengths) > 1_500_000)
    # the reads on the threshold: kept at S = L * T, dropped one unit above; 0 and 93 both present
    on = [i for i in range(n) if what[i] == KEEP and rule.qual_sum(quals[i]) == lengths[i] * T]
    above = [i for i in range(n) if what[i] == LOWQ and set(quals[i].tolist()) == {9, 10}]
    assert on and above and any(0 in q and 93 in q for q in quals)
    # length alone decides without a threshold
    only_len = fates(lengths, None, rule.MIN_LEN, rule.MAX_LEN, 0)
    assert only_len.count(LOWQ) == 0 and only_len.count(SHORT) == c["dropped_short"] and only_len.count(LONG) == c["dropped_long"]


def test_the_overflow_batch_overflows():
    """more read starts under one tile than read_qual_kernel has slots for, counted on the lengths alone"""
    L, behind, straddler = rule.overflow_batch()
    o = np.zeros(len(L) + 1, dtype=np.int64)
    o[1:] = np.cumsum(L)
    starts = np.bincount(o[:-1] // rule.TILE, minlength=3)
    assert starts[0] > rule.SLOTS + 64 and o[-1] > 2 * rule.TILE
    assert min(L[:1300]) == 1 and max(L[:1300]) == 15 and L[:16] == [1] * 16
    # the run of empty reads starts exactly on the tile edge and the read behind it holds that tile's first byte: the kernel must find that
    # read, 1 100 reads behind the first that starts there, as the tile's first (it does not count the empty ones against its slots)
    first_at_edge = int(np.searchsorted(o[:-1], rule.TILE, side="left"))
    assert o[first_at_edge] == rule.TILE and L[first_at_edge:first_at_edge + 1100] == [0] * 1100 and behind == first_at_edge + 1100
    assert L[behind] > 0 and o[behind] == rule.TILE and behind - first_at_edge == 1100
    # a read that starts in the second tile's last lane piece (16 bytes) and ends in the third
    assert 2 * rule.TILE - 16 <= o[straddler] < 2 * rule.TILE < o[straddler + 1]
    assert max(L) <= 16400 and 0 < min(x for x in L if x)


@pytest.mark.parametrize("exe, head", [("pandora", ["map"]), ("pandora", ["discover"]), ("drprg", ["predict", "-x", "nowhere", "-i", "nothing.fq"])])
def test_usage_errors_exit_with_status_2(exe, head):
    path = os.path.join(ROOT, "drprg_amd", "bin", exe)
    for extra, text in ((["--min-read-len", "500", "--max-read-len", "499"], "--max-read-len"), (["--min-read-qual", "ten"], "--min-read-qual"),
                        (["--min-read-qual", "93.5"], "--min-read-qual"), (["--min-read-len", "-3"], "--min-read-len"), (["--min-read-qual"], "needs a value")):
        r = subprocess.run([path] + head + extra, capture_output=True, text=True)
        assert r.returncode == 2 and text in r.stderr, (extra, r.returncode, r.stderr)
