"""The depth cap (`pandora --max-covg`, drprg_hip_set_max_covg) as far as it shows without a GPU: the entry points exist in every
layer, a host-only context takes the setter, the Python mirror and the executable default to pandora's 300, and the rule the GPU tests
compute their expectations with (tests/max_covg_rule.py) is the rule as pandora states it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from max_covg_rule import OFF, accepted_reads, pandora_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDORA = os.path.join(ROOT, "drprg_amd", "bin", "pandora")


def test_entry_points_in_header_library_and_ctypes_table():
    header = open(os.path.join(ROOT, "include", "drprg_hip.h")).read()
    assert re.search(r"int drprg_hip_set_max_covg\(drprg_hip_ctx\* ctx, uint64_t max_covg\);", header)
    assert re.search(r"int drprg_hip_max_covg_info\(drprg_hip_ctx\* ctx, uint64_t out\[4\]\);", header)
    assert "#define DRPRG_HIP_MAP_OPTS_SIZE 48" in header  # a new entry point, not a new field of the options
    assert "UPSTREAM-MEMORY" in header[header.index("Depth cap"):header.index("int drprg_hip_set_max_covg")]  # the rule is said to be unpinned
    from drprg_amd import _lib
    assert C.sizeof(_lib.MapOpts) == 48
    for name in ("drprg_hip_set_max_covg", "drprg_hip_max_covg_info"):
        assert getattr(_lib.lib, name).restype is C.c_int
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "drprg_hip_set_max_covg" in integration and "drprg_hip_max_covg_info" in integration


def test_host_only_context_takes_the_cap(tmp_path):
    from drprg_amd import Context, synth
    panel = synth.small_panel(seed=3)
    prg = str(tmp_path / "dr.prg")
    panel.write(prg, str(tmp_path / "genes.fa"))
    ctx = Context(prg, 11, 15, device=-1, from_files=False)
    ctx.set_opts(illumina=True, genome_size=10000)
    ctx.set_max_covg(3)
    assert ctx.max_covg_info() == dict(reached=False, reads=0, bases=0, dropped=0)
    # coverage that arrives with more bases than the cap allows: the cap counts from the running total
    covg, prg_reads = ctx.coverage()
    ctx.set_coverage(covg, prg_reads, 40000)
    assert ctx.max_covg_info()["reached"]
    ctx.reset()  # clears the total, keeps the cap
    assert not ctx.max_covg_info()["reached"]
    ctx.set_coverage(covg, prg_reads, 39999)
    assert not ctx.max_covg_info()["reached"]
    ctx.set_max_covg(None)
    ctx.set_coverage(covg, prg_reads, 10 ** 12)
    assert not ctx.max_covg_info()["reached"]
    ctx.close()


def test_python_mirror_defaults_to_300_and_tags_the_cap(tmp_path):
    from drprg_amd import Pandora
    assert Pandora._parse_args([])["max_covg"] == 300
    assert Pandora._parse_args(["-t", "2", "--max-covg", "4294967295", "-I"]) == dict(threads=2, w=14, k=15, c=10, illumina=True, max_covg=OFF)
    prg, reads = tmp_path / "dr.prg", tmp_path / "r.fq"
    prg.write_text("x")
    reads.write_text("y")
    tag = lambda args: Pandora._run_tag(str(prg), str(reads), args)
    assert tag(["-w", "11"]) == tag(["-w", "11", "--max-covg", "300"]) == tag(["--max-covg", "300", "-w", "11", "-K"])
    assert tag(["-w", "11"]) != tag(["-w", "11", "--max-covg", "299"])
    assert tag(["-w", "11", "--max-covg", "5"]) != tag(["-w", "11", "--max-covg", str(OFF)])


def test_usage_text_names_the_default():
    r = subprocess.run([PANDORA, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--max-covg N" in r.stderr and "default 300" in r.stderr and "4294967295" in r.stderr


RULE_TABLE = [
    # lengths, genome size, cap -> reads taken
    ([150] * 10, 100, 3, 3),            # 450 // 100 = 4 > 3 at the third read (T = 400)
    ([100] * 10, 100, 3, 4),            # B = 400 == T exactly: 400 // 100 = 4 > 3
    ([100, 100, 100, 99, 1, 5], 100, 3, 5),   # 399 // 100 = 3 is not over the cap; the one base that follows is
    ([100, 100, 100, 99, 4000, 5], 100, 3, 5),
    ([4000, 1, 1], 1000, 3, 1),         # the first read is the cut
    ([10, 10, 10], 1000, 3, 3),         # never reached
    ([0, 0, 400, 0, 0], 100, 3, 3),     # empty reads in front of the cut are taken, those behind it are not
    ([399, 0, 0, 1, 0], 100, 3, 4),     # ... and an empty read can never be the cut
    ([1] * 10, 1, 0, 1),                # cap 0: T = g
    ([5] * 10, 7, 0, 2),
    ([10 ** 6] * 5, 1, OFF, 5),         # 2^32 - 1: off
    ([10 ** 6] * 5, 1, 2 ** 40, 5),
    ([2 ** 33, 1], 2, OFF - 1, 1),      # the largest cap that is one: T = (2^32 - 1) * 2
    ([], 100, 3, 0),
]


@pytest.mark.parametrize("lengths,g,cap,n", RULE_TABLE)
def test_rule_table(lengths, g, cap, n):
    """the loop as pandora states it, and its restatement with T = (cap + 1) * g on the cumulative sum, agree with the table"""
    assert pandora_loop(lengths, g, cap) == n
    got, bases, reached = accepted_reads(lengths, g, cap)
    assert got == n and bases == sum(lengths[:n])
    assert reached == (cap < OFF and sum(lengths[:n]) >= (cap + 1) * g)


def test_rule_restatement_on_random_inputs():
    rng = np.random.default_rng(5)
    for _ in range(300):
        lengths = rng.integers(0, 400, size=int(rng.integers(1, 60))).tolist()
        g, cap, total = int(rng.integers(1, 900)), int(rng.integers(0, 6)), int(rng.integers(0, 500))
        T = (cap + 1) * g
        n, bases, reached = accepted_reads(lengths, g, cap, total)
        if total >= T:  # the cap was passed before these reads: none is taken
            assert (n, reached) == (0, True)
            continue
        assert n == pandora_loop(lengths, g, cap, total) and bases == sum(lengths[:n])


# ---- the hand-over in file order the cap's ingest uses (IngestHooks::submit_in_order), through its host-only self-check ----
def _ordered(path, threads, max_reads=2 ** 64 - 1):
    from drprg_amd._lib import lib
    out = (C.c_uint64 * 6)()
    err = C.create_string_buffer(512)
    rc = lib.drprg_hip_parse_fastx_ordered(os.fsencode(path), threads, max_reads, out, err, len(err))
    return rc, [int(x) for x in out], err.value.decode()


def _ordered_digest(bases, read_len, n):
    """sum over the first n reads of (index + 1) x FNV-1a(read), in 64-bit arithmetic: what drprg_hip_parse_fastx_ordered reports"""
    b = bases[:n * read_len].reshape(n, read_len).astype(np.uint64)
    h = np.full(n, 1469598103934665603, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for col in range(read_len):
            h = (h ^ b[:, col]) * np.uint64(1099511628211)
        return int((h * np.arange(1, n + 1, dtype=np.uint64)).sum(dtype=np.uint64))


@pytest.fixture(scope="module")
def big_fastq(tmp_path_factory):
    """200 000 reads of 150 bases: 63.2 MB of text = 8 slices of a plain file, 2 windows of inflated gzip text, 2.5 ingest blocks of bases"""
    import gzip
    from drprg_amd import synth
    d = tmp_path_factory.mktemp("ordered")
    n = 200_000
    bases = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(11).integers(0, 4, n * 150)]
    fq = str(d / "r.fq")
    synth.write_fastq_fixed(fq, bases, 150)
    text = open(fq, "rb").read()
    assert len(text) == n * 316
    with gzip.open(fq + ".gz", "wb", compresslevel=1) as fh:
        fh.write(text)
    return d, fq, bases, n, text


@pytest.mark.parametrize("threads", [1, 4, 8])
@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
def test_ordered_hand_over_is_in_file_order_and_stops(big_fastq, threads, gz):
    d, fq, bases, n, _ = big_fastq
    path = fq + ".gz" if gz else fq
    for max_reads in (1, 267, 70_001, n, 2 ** 64 - 1):
        rc, out, err = _ordered(path, threads, max_reads)
        want = min(n, max_reads)
        assert rc == 0, err
        assert out[0] == want and out[1] == want * 150 and out[2] == _ordered_digest(bases, 150, want), (threads, max_reads)
        assert out[5] <= n - want
        if max_reads >= n:
            assert out[5] == 0 and out[3] >= 3


@pytest.mark.parametrize("threads", [1, 4, 8])
def test_ordered_hand_over_fails_cleanly(big_fastq, threads):
    """a failure while parser threads stand with full blocks waiting for their turn -- a truncated multi-window .gz, a corrupt .gz, a broken
    record far into a plain file --: a clean error, every time (the threads drop what they hold; nothing is appended behind a full block)"""
    d, fq, bases, n, text = big_fastq
    gz = open(fq + ".gz", "rb").read()
    cases = {"truncated.fq.gz": gz[:len(gz) * 7 // 10], "corrupt.fq.gz": gz[:len(gz) // 2] + bytes(4096) + gz[len(gz) // 2 + 4096:],
             "broken.fq": text[:316 * 120_000] + b"this is not a record\n" + text[316 * 120_000:]}
    for name, data in cases.items():
        p = str(d / f"t{threads}_{name}")
        with open(p, "wb") as fh:
            fh.write(data)
        for _ in range(3):
            rc, out, err = _ordered(p, threads)
            assert rc != 0 and err, (name, rc, out)
        os.remove(p)
    # ... and the intact files still parse afterwards (the pinned-block pool and the text buffers are shared by the calls of a process)
    rc, out, err = _ordered(fq, threads)
    assert rc == 0 and out[0] == n and out[2] == _ordered_digest(bases, 150, n), err
