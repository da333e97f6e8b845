"""Adapter trimming's rule on the CPU: the rule of tests/adapter_rule.py against a second, brute-force statement of itself, its edges, the
census of the fixtures the GPU tests cut, the constants of csrc/adapter_piece.h, the per-lane arithmetic of adapter_points_kernel walked
on the CPU (tools/adapter_walk.cpp), and the handling of the settings that needs no device: the C entry's refusals on a host-only
context and the executables' usage errors, which come before any device is opened."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adapter_rule as rule
from adapter_rule import NEXTERA, TRUSEQ, cut_point, cut_ranges, error_milli, kernel_batch, min_overlap
from read_trim_rule import reverse_flag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 22
NO_CUT = dict(reads_seen=0, bases_seen=0, reads_cut=0, bases_cut=0, reads_emptied=0)


def _brute(read, adapters, e, O, x, y):
    """the rule, letter by letter"""
    n = y - x
    for p in range(n):
        for A in adapters:
            c = min(len(A), n - p)
            if c < O:
                continue
            miss = 0
            for j in range(c):
                b = chr(read[x + p + j]).upper()
                if b not in "ACGT" or b != A[j].upper():
                    miss += 1
            if miss <= c * e // 1000:
                return p
    return None


def test_the_rule_equals_its_brute_force_statement_on_random_reads():
    rng = np.random.default_rng(3)
    n_cut = 0
    for trial in range(1500):
        adapters = ["".join(rng.choice(list("ACGTacgt"), size=int(rng.integers(1, 13)))) for _ in range(int(rng.integers(1, 5)))]
        e = int(rng.choice([0, 100, 200, 250, 333, 500]))
        O = int(rng.integers(1, min(len(a) for a in adapters) + 1))
        read = bytearray(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=int(rng.integers(0, 50)), p=[.12] * 8 + [.04]))
        if len(read) > 4 and trial % 2:
            A = adapters[int(rng.integers(len(adapters)))]
            at = int(rng.integers(len(read)))
            piece = A.encode()[:len(read) - at]
            read[at:at + len(piece)] = piece
        x = int(rng.integers(0, len(read) + 1))
        y = int(rng.integers(x, len(read) + 1))
        if trial % 3:
            x, y = 0, len(read)
        got, want = (cut_point(bytes(read), adapters, e, O, x, y) if y > x else None), _brute(read, adapters, e, O, x, y)
        assert got == want, (read, adapters, e, O, x, y)
        n_cut += want is not None
    assert 300 < n_cut < 1400


def test_the_edges_of_the_rule():
    A = TRUSEQ[:12]
    f = b"TTTTTTTTTTTTTTTTTTTT"  # (no letter of it starts the adapter)
    assert error_milli("0.1") == 100 and error_milli("0") == 0 and error_milli("0.5") == 500 and error_milli("0.125") == 125 and error_milli(0.2) == 200
    for bad in ("0.501", "0.1234", "-0.1", "1"):
        with pytest.raises(ValueError):
            error_milli(bad)
    assert min_overlap([A]) == 3 and min_overlap(["AC"]) == 2 and min_overlap([A, "ACGTA"], 4) == 4
    assert cut_point(b"", [A], 100, 3) is None and cut_point(A.encode(), [A], 0, 3) == 0
    # partial overlaps at the end: from O on
    assert cut_point(f + A[:2].encode(), [A], 0, 3) is None and cut_point(f + A[:3].encode(), [A], 0, 3) == 20
    assert cut_point(f + A[:2].encode(), [A], 0, 2) == 20 and cut_point(f + A[:1].encode(), [A], 0, 1) == 20
    # floor(c * e / 1000): 12 letters at 0.1 allow one mismatch, 9 letters none, 10 letters one
    one, two = b"AGATCGGTAGAG", b"AGTTCGGTAGAG"
    assert cut_point(f + one, [A], 100, 3) == 20 and cut_point(f + two, [A], 100, 3) is None and cut_point(f + two, [A], 200, 3) == 20
    assert cut_point(f + one[:9], [A], 100, 3) is None and cut_point(f + one[:10], [A], 100, 3) == 20
    # a base that is not ACGT is a mismatch, whatever the adapter holds; the comparison ignores case
    assert cut_point(f + b"AGATCGGNAGAG", [A], 100, 3) == 20 and cut_point(f + b"AGNTCGGNAGAG", [A], 100, 3) is None
    assert cut_point(f + A.lower().encode(), [A], 0, 3) == 20 and cut_point(f + A.encode(), [A.lower()], 0, 3) == 20
    # the leftmost match over all adapters, perfect or not
    assert cut_point(f + one + f + A.encode(), [A], 100, 3) == 20 and cut_point(f + NEXTERA.encode() + A.encode(), [A, NEXTERA], 0, 3) == 20
    # the range: a window never reaches past y, and a start before x is none
    r = f + A.encode() + f
    assert cut_point(r, [A], 0, 3, 0, 25) == 20 and cut_point(r, [A], 0, 3, 0, 22) is None and cut_point(r, [A], 0, 3, 21, len(r)) is None
    assert cut_point(r, [A], 0, 3, 5, len(r)) == 15
    ranges, info = cut_ranges([r, A.encode(), f, b""], [(5, len(r)), (0, 12), (0, 20), (0, 0)], [A], 0, 3)
    assert ranges == [(5, 20), (0, 0), (0, 20), (0, 0)] and info == dict(reads_seen=4, bases_seen=len(r) - 5 + 32, reads_cut=2, bases_cut=len(r) - 20 + 12, reads_emptied=1)


@pytest.mark.parametrize("E", ["0", "0.1", "0.2"])
@pytest.mark.parametrize("name", ["12", "16", "17", "33", "64", "33+19"])
def test_the_census_of_the_kernel_batch(name, E):
    b = kernel_batch(name, E)
    c = rule.census(b)  # (raises when a class is not what it is meant to be)
    for must in ("short run", "edge lengths", "the adapter itself", "partial below O", "partial from O", "at the limit", "one over the limit", "N over the limit",
                 "two occurrences", "worse to the left", "split 2", "split 5", "lower case", "straddles end", "straddles end below O", "starts before begin",
                 "across a lane boundary", "across a wave boundary", "across a tile boundary by 1", "across a tile boundary by m - 1", "long with adapter",
                 "long without adapter"):
        assert must in c, must
    m = len(b["adapters"][0])
    assert c["partial below O"] == (0, b["O"] - 1) and c["partial from O"] == (m - b["O"], 0) and c["edge lengths"] == (0, 7)
    if E == "0.1" and m >= 33:
        assert b["classes"]["partial lengths"][0] == [9, 10, 19, 20]
    if E == "0.1":
        assert b["classes"]["partial lengths"][0][:2] == [9, 10] and "N for a mismatch" in c
    if name == "33+19":
        assert c["second adapter"] == (2, 0)
    # where things lie: the short run inside the first tile and more reads than a workgroup's table, the boundaries crossed as they are meant to be
    L = [len(r) for r in b["reads"]]
    o = np.concatenate([[0], np.cumsum(L)])
    run = b["classes"]["short run"][0]
    assert len(run) >= 1100 > rule.SLOTS and o[run[-1] + 1] < rule.TILE and all(3 <= L[i] <= 8 for i in run)
    cuts, _ = cut_ranges(b["reads"], b["ranges"], b["adapters"], b["e"], b["O"])

    def start(cls):
        (i,) = b["classes"][cls][0]
        return int(o[i]) + cuts[i][1]
    assert start("across a tile boundary by 1") + m - 1 == rule.TILE and start("across a tile boundary by m - 1") == 3 * rule.TILE - 1
    assert start("across a wave boundary") % rule.WAVE == rule.WAVE - 3 and start("across a lane boundary") % rule.LANE == rule.LANE - 2
    assert start("across a lane boundary") % rule.WAVE < rule.WAVE - rule.LANE
    long_a, long_b = b["classes"]["long with adapter"][0][0], b["classes"]["long without adapter"][0][0]
    assert L[long_a] >= 20000 and cuts[long_a] == (0, 18000) and L[long_b] >= 20000 and 3 * rule.TILE < int(o[-1]) < 5 * rule.TILE
    words, npos = rule.packed_form(b"".join(b["reads"]))
    assert words.size == (int(o[-1]) + 15) // 16 and npos.size >= 1 and np.all(np.diff(npos.astype(np.int64)) > 0)


def test_planted_adapters_of_every_kind_fall_on_reversed_records():
    """the BAM fixtures store every third record on the reverse strand: read-through, partial and no adapter must all occur among them"""
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(0, 300, size=300)]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(offs[-1]))
    reads, kinds = rule.plant(bases, offs, TRUSEQ[:33], 3, seed=6)
    for kind in ("through", "partial", "none"):
        n_rev, n_fwd = sum(k == kind and reverse_flag(i) for i, k in enumerate(kinds)), sum(k == kind and not reverse_flag(i) for i, k in enumerate(kinds))
        assert n_rev >= 20 and n_fwd >= 40, (kind, n_rev, n_fwd)
    for r, k, L in zip(reads, kinds, lengths):
        assert k != "none" or len(r) == L
        assert k != "partial" or (3 <= len(r) - L <= 32 and r[L:] == TRUSEQ[:len(r) - L].encode())
        assert k != "through" or TRUSEQ[:33].encode() in r


def test_the_constants_of_the_piece_header_are_the_rules():
    text = open(os.path.join(ROOT, "drprg_amd", "csrc", "adapter_piece.h")).read()

    def const(name):
        return int(re.search(r"constexpr uint32_t %s = (\d+)" % name, text).group(1))

    assert const("AD_MAX_ADAPTERS") == rule.MAX_ADAPTERS and const("AD_MAX_LEN") == rule.MAX_LEN and const("AD_MAX_ERROR_MILLI") == rule.MAX_ERROR_MILLI
    assert const("AD_DEFAULT_ERROR_MILLI") == error_milli(rule.DEFAULT_ERROR) and const("AD_DEFAULT_MIN_OVERLAP") == rule.DEFAULT_MIN_OVERLAP
    assert const("AD_LANE_STARTS") == rule.LANE
    kernel = open(os.path.join(ROOT, "drprg_amd", "csrc", "adapter_trim.hip")).read()
    assert int(re.search(r"constexpr uint32_t AD_SLOTS = (\d+)", kernel).group(1)) == rule.SLOTS
    assert re.search(r"AD_TILE = AD_THREADS \* AD_ROUNDS \* AD_LANE_STARTS", kernel) and "AD_THREADS = 256" in kernel and "AD_ROUNDS = 4" in kernel  # 16 384


def test_the_lane_arithmetic_walked_on_the_cpu(tmp_path):
    """adapter_piece.h is host code as well: every lane's window, masks and counts against the rule letter by letter, both input forms.
    Built as plain C++ by $CXX or, without one, by the compiler the Makefile builds everything with; no compiler fails the test."""
    exe = str(tmp_path / "adapter_walk")
    cxx = os.environ.get("CXX")
    argv = [cxx] if cxx and shutil.which(cxx) else [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    r = subprocess.run(argv + ["-std=c++17", "-O1", "-I", os.path.join(ROOT, "drprg_amd", "csrc"), os.path.join(ROOT, "tools", "adapter_walk.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "reads checked" in r.stdout, (r.stdout, r.stderr)


def test_the_settings_on_a_host_only_context(tmp_path):
    from drprg_amd import Context
    from drprg_amd.pandora import DependencyError
    f = str(tmp_path / "dr.prg")
    open(f, "w").write(">g0\nACGTTGCAAGGCTTAACCGGATATCGCGATTAGGCATCAGT\n")
    ctx = Context(f, 5, 7, device=-1, from_files=False)
    A = TRUSEQ[:33]
    for bad in (dict(seqs=[A] * 5), dict(seqs=[""]), dict(seqs=[A + A]), dict(seqs=["ACGN"]), dict(seqs=["AC-T"]), dict(seqs=[A], error="0.501"),
                dict(seqs=[A, "ACGT"], min_overlap=5), dict(seqs=[A], min_overlap=34)):
        with pytest.raises(DependencyError) as e:
            ctx.set_adapters(**bad)
        assert e.value.code == EINVAL, bad
    with pytest.raises(ValueError):
        ctx.set_adapters([A], error="0.1234")
    ctx.set_adapters([A, NEXTERA, "acgt", TRUSEQ], error="0.5", min_overlap=4)
    ctx.set_adapters([A], error=0, min_overlap=33)
    ctx.set_adapters([A])
    ctx.set_adapters([])
    assert ctx.adapter_trim_info() == NO_CUT
    ctx.close()


@pytest.mark.parametrize("exe", ["pandora", "drprg"])
def test_usage_errors_exit_2_and_need_no_device(tmp_path, exe):
    path = os.path.join(ROOT, "drprg_amd", "bin", exe)
    head = [path, "map"] if exe == "pandora" else [path, "predict", "-x", str(tmp_path), "-i", "reads.fq"]
    tail = ["dr.prg", "reads.fq"] if exe == "pandora" else []
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a usage error comes before one is looked for)
    A = TRUSEQ[:12]
    for flags, word in ((["--adapter", A] * 5, "--adapter"), (["--adapter", ""], "--adapter"), (["--adapter", "A" * 65], "--adapter"),
                        (["--adapter", "ACGTN"], "--adapter"), (["--adapter", A, "--adapter-error", "0.51"], "--adapter-error"),
                        (["--adapter", A, "--adapter-error", "-0.1"], "--adapter-error"), (["--adapter", A, "--adapter-error", "0.1234"], "--adapter-error"),
                        (["--adapter", A, "--adapter-error", "x"], "--adapter-error"), (["--adapter", A, "--adapter-min-overlap", "0"], "--adapter-min-overlap"),
                        (["--adapter", A, "--adapter", "ACGT", "--adapter-min-overlap", "5"], "--adapter-min-overlap"),
                        (["--adapter", A, "--adapter-min-overlap", "13"], "--adapter-min-overlap"), (["--adapter-error", "0.1"], "--adapter-error"),
                        (["--adapter-min-overlap", "3"], "--adapter-min-overlap"), (["--adapter"], "--adapter")):
        r = subprocess.run(head + flags + tail, capture_output=True, text=True, env=env)
        assert r.returncode == 2 and word in r.stderr, (flags, r.returncode, r.stderr)
