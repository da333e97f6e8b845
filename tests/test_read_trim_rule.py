"""Read trimming's rule on the CPU: the two forms of the rule (read orientation; stored order with the crops swapped, mirrored) against each
other, its edges, the census of the fixtures the GPU tests trim (tests/read_trim_rule.py), the constants of csrc/read_trim_piece.h, and
the handling of the settings that needs no device: the C entry's refusals on a host-only context and the executables' usage errors, which
come before any device is opened."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import read_trim_rule as rule
from read_trim_rule import CLASSES, EMPTY_CROP, SHORTER_THAN_W, classify, kept_range, kept_range_stored, qual_milli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 22


def _host_ctx(tmp_path):
    from drprg_amd import Context
    f = str(tmp_path / "dr.prg")
    open(f, "w").write(">g0\nACGTTGCAAGGCTTAACCGGATATCGCGATTAGGCATCAGT\n")
    return Context(f, 5, 7, device=-1, from_files=False)


def test_the_two_forms_of_the_rule_agree_on_random_reads():
    rng = np.random.default_rng(1)
    seen = collections.Counter()
    for _ in range(20000):
        L = int(rng.integers(0, 80))
        W = int(rng.choice([1, 2, 4, 7, 32]))
        milli = int(rng.choice([5000, 20000, 20500, 12345]))
        front, tail = (int(rng.integers(0, 12)), int(rng.integers(0, 12))) if rng.random() < 0.5 else (0, 0)
        # runs of good and bad bases, so that every class comes about
        q = np.concatenate([rng.integers(*((milli // 1000, 41) if rng.random() < 0.5 else (0, milli // 1000 + 1)), size=int(rng.integers(1, 12))) for _ in range(L)])[:L] \
            if L else np.zeros(0, dtype=np.int64)
        a, b = kept_range(q, L, front, tail, milli, W)
        assert 0 <= a <= b <= L and (a < b or (a, b) == (0, 0))
        assert kept_range_stored(q[::-1], L, True, front, tail, milli, W) == (a, b)
        assert kept_range_stored(q, L, False, front, tail, milli, W) == (a, b)
        if a < b:  # the ends are at or above Q, inside the crop, and the range holds a good window at either end
            assert 1000 * q[a] >= milli and 1000 * q[b - 1] >= milli and a >= min(front, L) and b <= L - min(tail, L - min(front, L))
        seen[classify(L, (a, b), front, tail, milli, W)] += 1
        # the crops alone
        c = kept_range(None, L, front, tail)
        assert c == kept_range_stored(None, L, True, front, tail) and (c == (0, 0) or c == (front, L - tail))
    assert all(seen[c] > 50 for c in CLASSES), seen


def test_a_window_of_one_is_first_and_last_base_at_or_above_q():
    rng = np.random.default_rng(2)
    for _ in range(3000):
        L = int(rng.integers(0, 60))
        q = rng.integers(0, 41, size=L)
        ok = [i for i in range(L) if q[i] >= 20]
        assert kept_range(q, L, 0, 0, 20000, 1) == ((ok[0], ok[-1] + 1) if ok else (0, 0))


def test_edges_of_the_rule():
    q = [30] * 10
    assert kept_range(q, 10, 0, 0, 20000, 4) == (0, 10)
    assert kept_range(q, 10, 3, 2, 20000, 4) == (3, 8)
    assert kept_range(q, 10, 3, 2, 0, 0) == (3, 8) and kept_range(None, 10, 7, 9) == (0, 0) and kept_range(None, 10, 10, 0) == (0, 0)
    assert kept_range(q, 10, 4, 3, 20000, 4) == (0, 0)  # three bases behind the crop: shorter than W
    assert kept_range(q, 10, 4, 2, 20000, 4) == (4, 8)  # exactly W
    assert kept_range([20, 20, 20, 20], 4, 0, 0, 20000, 4) == (0, 4)  # a sum on the threshold is good
    assert kept_range([20, 20, 20, 19], 4, 0, 0, 20000, 4) == (0, 0)  # one below is not
    assert kept_range([21, 20, 20, 20], 4, 0, 0, 20500, 4) == (0, 0)   # a fractional Q: 81 < 82
    assert kept_range([21, 20, 21, 20], 4, 0, 0, 20250, 4) == (0, 3) and kept_range([21, 21, 21, 19], 4, 0, 0, 20500, 4) == (0, 3)  # narrowed: the last base is below Q
    assert kept_range([5, 40, 40, 5, 5, 5, 5, 40, 40, 5], 10, 0, 0, 20000, 4) == (1, 9)  # the inside is never looked at
    assert kept_range([], 0, 3, 3, 20000, 4) == (0, 0)
    assert qual_milli("12.5") == 12500 and qual_milli(20) == 20000 and qual_milli(0) == 0


def _census(lengths, ranges, front, tail, milli, W):
    return collections.Counter(classify(L, r, front, tail, milli, W) for L, r in zip(lengths, ranges))


@pytest.mark.parametrize("which", ["small", "big"])
def test_census_of_the_samples(which):
    lengths, quals = rule.small_sample() if which == "small" else rule.big_sample()
    assert (sum(lengths) < 750_000) == (which == "small")
    ranges = rule.sample_ranges(lengths, quals)
    c = _census(lengths, ranges, rule.FRONT_N, rule.TAIL_N, qual_milli(rule.QUAL), rule.WINDOW)
    assert all(c[k] >= 1 for k in CLASSES), c
    info = rule.info(lengths, ranges, rule.FRONT_N, rule.TAIL_N)
    assert info["bases_seen"] - info["cut_front"] - info["cut_tail"] - info["qual_cut_front"] - info["qual_cut_tail"] == sum(b - a for a, b in ranges)
    # the stored-order form on the records the BAM fixture reverses
    for i in range(0, len(lengths), 3):
        assert kept_range_stored(quals[i][::-1], lengths[i], True, rule.FRONT_N, rule.TAIL_N, qual_milli(rule.QUAL), rule.WINDOW) == ranges[i]


@pytest.mark.parametrize("crops", [(0, 0), (5, 3)])
@pytest.mark.parametrize("W", [1, 4, 32])
def test_census_of_the_kernel_batch(W, crops):
    L, Q, rev, milli = rule.kernel_batch(W)
    assert 3 * 16384 < sum(L) <= 4 * 16384 and sum(rev) >= len(L) // 4
    ranges = [kept_range_stored(q, l, v, crops[0], crops[1], milli, W) for q, l, v in zip(Q, L, rev)]
    c = _census(L, ranges, crops[0], crops[1], milli, W)
    # (a window of one base is never longer than a non-empty cropped read; without crops no read is emptied by them)
    want = [k for k in CLASSES if not (k == SHORTER_THAN_W and W == 1) and not (k == EMPTY_CROP and crops == (0, 0))]
    assert all(c[k] >= 1 for k in want), c
    # more than 1 024 reads inside one tile
    o = np.concatenate([[0], np.cumsum(L)])
    assert max(np.sum((o[:-1] >= t) & (o[:-1] < t + 16384)) for t in range(0, 4 * 16384, 16384)) > 1024 + 64


def test_the_constants_of_the_piece_header_are_the_rules():
    text = open(os.path.join(ROOT, "drprg_amd", "csrc", "read_trim_piece.h")).read()

    def const(name):
        return int(re.search(r"constexpr uint32_t %s = (\d+)" % name, text).group(1))

    assert const("RT_MAX_QUAL") == rule.MAX_QUAL and const("RT_MAX_QUAL_MILLI") == rule.MAX_QUAL_MILLI
    assert const("RT_MAX_WINDOW") == rule.MAX_WINDOW and const("RT_DEFAULT_WINDOW") == rule.DEFAULT_WINDOW and const("RT_LANE_STARTS") == 16


def test_the_settings_on_a_host_only_context(tmp_path):
    from drprg_amd.pandora import DependencyError
    ctx = _host_ctx(tmp_path)
    for bad in (dict(qual="93.001"), dict(qual=20, window=33), dict(window=4), dict(front=3, window=1)):
        with pytest.raises(DependencyError) as e:
            ctx.set_read_trim(**bad)
        assert e.value.code == EINVAL, bad
    ctx.set_read_trim(front=3, tail=2, qual="20.5", window=0)
    ctx.set_read_trim(qual=93, window=32)
    ctx.set_read_trim()
    assert ctx.read_trim_info() == dict(reads_seen=0, bases_seen=0, reads_lost_base=0, cut_front=0, cut_tail=0, qual_cut_front=0, qual_cut_tail=0, reads_emptied=0)
    ctx.close()


@pytest.mark.parametrize("exe", ["pandora", "drprg"])
def test_usage_errors_exit_2(tmp_path, exe):
    path = os.path.join(ROOT, "drprg_amd", "bin", exe)
    head = [path, "map"] if exe == "pandora" else [path, "predict", "-x", str(tmp_path), "-i", "reads.fq"]
    tail = ["dr.prg", "reads.fq"] if exe == "pandora" else []
    for flags, word in ((["--trim-window", "4"], "--trim-window"), (["--trim-qual", "20", "--trim-window", "0"], "--trim-window"),
                        (["--trim-qual", "20", "--trim-window", "33"], "--trim-window"), (["--trim-qual", "0"], "--trim-qual"),
                        (["--trim-qual", "93.5"], "--trim-qual"), (["--trim-qual", "x"], "--trim-qual"), (["--trim-front", "-1"], "--trim-front"),
                        (["--trim-tail", "3x"], "--trim-tail")):
        r = subprocess.run(head + flags + tail, capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr, (flags, r.returncode, r.stderr)
