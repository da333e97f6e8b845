"""BAM input on the host (csrc/bam.cpp behind csrc/ingest.cpp): a BAM file parses to the reads the rule gives (tests/bam_rule.py), i.e.
to what the FASTQ of those reads parses to -- whatever the thread count and wherever the BGZF members cut the stream --, and malformed
files end in an error code and a message.  The files are written by tests/bam_writer.py; no BAM library is involved."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import bam_rule
import bam_writer
from bam_writer import Rec

EFORMAT = -84
ALL16 = bam_writer.CODES


def _call(path, threads, max_reads=None):
    """(rc, message, (reads, bases, digest)) of parse_fastx, or of parse_fastx_ordered when max_reads is given"""
    from drprg_amd._lib import lib
    out = (C.c_uint64 * 6)()
    err = C.create_string_buffer(512)
    if max_reads is None:
        rc = lib.drprg_hip_parse_fastx(os.fsencode(str(path)), threads, C.cast(out, C.POINTER(C.c_uint64)), err, len(err))
    else:
        rc = lib.drprg_hip_parse_fastx_ordered(os.fsencode(str(path)), threads, max_reads, C.cast(out, C.POINTER(C.c_uint64)), err, len(err))
    return rc, err.value.decode(), (int(out[0]), int(out[1]), int(out[2]))


def _ok(path, threads, max_reads=None):
    rc, msg, got = _call(path, threads, max_reads)
    assert rc == 0, (rc, msg)
    return got


def _want(reads):
    return len(reads), sum(len(r) for r in reads), bam_rule.digest(reads)


def _special_records(tags_len, n_cigar):
    """every one of the 16 codes, reverse-flagged reads of odd and even length, secondary and supplementary records in between,
    l_seq == 0, a record with many CIGAR ops and long tags, flags that must not matter"""
    tags = b"".join(b"X%cZ" % (65 + i % 26) + b"t" * 37 + b"\0" for i in range(tags_len // 41))
    return [
        Rec(ALL16, flag=4, name=b"all16_fwd"),
        Rec("ACGTTGCAAC", flag=0x100, name=b"secondary"),
        Rec(ALL16, flag=0x10, name=b"all16_rev_even"),
        Rec(ALL16 + "A", flag=0x10, name=b"all16_rev_odd", low_nibble_pad=15),
        Rec("GATTACA", flag=0x800 | 0x10, name=b"supplementary_rev"),
        Rec("", flag=4, name=b"empty"),
        Rec("", flag=0x10, name=b"empty_rev"),
        Rec("ACGTNACGTRYACGT" * 9, flag=0x10, name=b"x" * 200, n_cigar=n_cigar, tags=tags),
        Rec("TTTTGGGGC", flag=0x900, name=b"both"),
        Rec("ACGTACGTACGTACGTA", flag=0x1 | 0x40 | 0x200 | 0x400, name=b"paired_qcfail_dup", low_nibble_pad=7),
        Rec("NNNNN", flag=0, name=b"n_only"),
        Rec("C", flag=0x10, name=b"one_rev"),
    ]


def _random_records(rng, n, lengths):
    recs = []
    for i in range(n):
        L = int(rng.choice(lengths))
        codes = rng.choice(list(ALL16), size=L, p=[0.004] + [0.235, 0.235, 0.004, 0.235, 0.004, 0.004, 0.004, 0.235] + [0.004] * 6 + [0.016])
        flag = int(rng.choice([0, 4, 0x10, 0x10, 0x100, 0x800, 0x110, 0x1 | 0x80 | 0x10, 0x400]))
        recs.append(Rec("".join(codes), flag=flag, name=b"q%d" % i, n_cigar=int(rng.integers(0, 4)), tags=b"NMi" + struct.pack("<i", i) if i % 3 else b"",
                        low_nibble_pad=int(rng.integers(0, 16))))
    return recs


@pytest.fixture(scope="module")
def recs():
    rng = np.random.default_rng(11)
    return _special_records(5000, 300) + _random_records(rng, 600, [0, 1, 2, 15, 16, 17, 31, 32, 33, 150, 151, 1000, 4001])


@pytest.fixture(scope="module")
def small_recs():
    rng = np.random.default_rng(12)
    return _special_records(700, 300) + _random_records(rng, 30, [0, 1, 2, 15, 16, 17, 33, 150])


def test_rule_mentions_every_case(recs):
    """the file holds what the issue lists (a guard on the fixture, not on the library)"""
    kept = [r for r in recs if not r.flag & 0x900]
    assert set("".join(r.seq for r in kept)) == set(ALL16)
    assert any(r.flag & 0x10 and len(r.seq) % 2 == 1 for r in kept) and any(r.flag & 0x10 and len(r.seq) % 2 == 0 and r.seq for r in kept)
    assert any(r.flag & 0x100 for r in recs) and any(r.flag & 0x800 for r in recs) and any(not r.seq for r in kept)
    assert any(r.n_cigar == 300 and len(r.tags) > 4000 for r in recs)


@pytest.mark.parametrize("threads", [1, 2, 5, 8])
def test_bam_equals_fastq_of_the_rules_reads(tmp_path, recs, threads):
    reads = bam_rule.reads_of(recs)
    bam = bam_writer.write(tmp_path / "r.bam", recs)
    fq = tmp_path / "r.fq"
    fq.write_bytes(bam_rule.fastq_of(reads))
    assert _ok(bam, threads) == _ok(fq, threads) == _want(reads)


@pytest.mark.parametrize("threads", [1, 5])
def test_ordered_hand_over_cut_inside_a_block(tmp_path, recs, threads):
    reads = bam_rule.reads_of(recs)
    bam = bam_writer.write(tmp_path / "r.bam", recs, payload=997)
    fq = tmp_path / "r.fq"
    fq.write_bytes(bam_rule.fastq_of(reads))
    for max_reads in (1, 7, len(reads) // 2, len(reads) - 1, len(reads), len(reads) + 5):
        head = reads[:max_reads]
        want = (len(head), sum(len(r) for r in head), bam_rule.digest_ordered(head))
        assert _ok(bam, threads, max_reads) == _ok(fq, threads, max_reads) == want, max_reads


@pytest.mark.parametrize("payload", [1, 3, 33, 997, 65280])
def test_members_cut_the_stream_anywhere(tmp_path, small_recs, payload):
    """payload 1 and 3: every field of every record -- the block_size word too -- and the header are split across BGZF members"""
    reads = bam_rule.reads_of(small_recs)
    bam = bam_writer.write(tmp_path / "m.bam", small_recs, payload=payload, refs=[(b"chr1", 1000), (b"a_longer_reference_name", 5)])
    for threads in (1, 5):
        assert _ok(bam, threads) == _want(reads), threads
        head = reads[:9]
        assert _ok(bam, threads, 9) == (9, sum(len(r) for r in head), bam_rule.digest_ordered(head))


def test_records_straddle_inflate_windows(tmp_path):
    """more than one 32 MB window of inflated stream: records and their block_size words are carried from window to window"""
    rng = np.random.default_rng(3)
    one = "".join(rng.choice(list("ACGT"), size=100))
    recs = [Rec(one[i % 7:] + "N" * (i % 3), flag=0x10 if i % 2 else 0, name=b"w%d" % i, tags=b"XXZ" + b"u" * (4001 + i % 5) + b"\0") for i in range(8600)]
    reads = bam_rule.reads_of(recs)
    bam = bam_writer.write(tmp_path / "w.bam", recs)
    assert len(bam_writer.stream(recs)) > (32 << 20) + (1 << 20)
    assert _ok(bam, 4) == _want(reads)


def test_header_only_and_missing_eof_block(tmp_path, small_recs):
    for eof in (True, False):
        p = tmp_path / f"h{int(eof)}.bam"
        p.write_bytes(bam_writer.bgzf(bam_writer.header(text=b"@HD\tVN:1.6\n@CO\t" + b"c" * 3000 + b"\n", refs=[(b"r1", 10)] * 50), payload=100, eof=eof))
        assert _ok(p, 3) == (0, 0, 0)
    reads = bam_rule.reads_of(small_recs)
    assert _ok(bam_writer.write(tmp_path / "noeof.bam", small_recs, eof=False), 2) == _want(reads)


def test_zlib_path_reads_bam_too(tmp_path, small_recs):
    """a host without libdeflate inflates the members with zlib: the same reads (a fresh process: the library binds libdeflate once)"""
    import subprocess
    import sys
    bam = bam_writer.write(tmp_path / "z.bam", small_recs, payload=997)
    code = ("import ctypes as C, os, sys; sys.path.insert(0, %r); from drprg_amd._lib import lib; out = (C.c_uint64 * 5)(); err = C.create_string_buffer(512); "
            "rc = lib.drprg_hip_parse_fastx(os.fsencode(%r), 3, out, err, 512); print(rc, out[0], out[1], out[2], out[4])"
            % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), str(bam)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DRPRG_HIP_NO_LIBDEFLATE="1"), capture_output=True, text=True, check=True)
    rc, n, b, d, mode = (int(x) for x in r.stdout.split())
    assert (rc, n, b, d) == (0,) + _want(bam_rule.reads_of(small_recs)) and mode != 1


def _malformed_cases():
    good = Rec("ACGTACGTAC", name=b"good")
    hdr = bam_writer.header()
    # block_size below the 32 fixed bytes (the chain cannot even be hopped)
    yield "block_size_below_fixed_part", hdr + good.encode() + struct.pack("<I", 16) + b"\0" * 16
    # block_size that covers the fixed part but not the name + cigar + seq + qual it announces; the chain itself is consistent
    bad = Rec("ACGT" * 30, name=b"liar", n_cigar=2).encode()
    short = 32 + 20
    yield "block_size_below_its_fields", hdr + good.encode() + struct.pack("<I", short) + bad[4:4 + short] + good.encode()
    # the last record announces more bytes than the stream holds
    yield "record_past_the_end", hdr + good.encode() + good.encode()[:-3]
    yield "block_size_word_cut", hdr + good.encode() + good.encode()[:2]
    yield "wrong_magic_version", b"BAM\2" + hdr[4:] + good.encode()
    yield "wrong_magic_text", b"BAI\1" + hdr[4:] + good.encode()
    yield "header_cut", hdr[:-2]


@pytest.mark.parametrize("name,data", list(_malformed_cases()))
def test_malformed_files_are_errors_with_a_message(tmp_path, name, data):
    p = tmp_path / (name + ".bam")
    p.write_bytes(bam_writer.bgzf(data))
    for threads in (1, 4):
        for max_reads in (None, 100):
            rc, msg, _ = _call(p, threads, max_reads)
            assert rc == EFORMAT and msg, (name, threads, rc, msg)


def test_truncation_at_every_byte(tmp_path):
    """A three-record file cut at every byte of its stream: the reads before the cut when the cut is a record boundary (or the end of
    the header, or nothing at all), an error everywhere else -- never other bytes."""
    recs = [Rec("ACGTNACGTAC", flag=0, name=b"a", n_cigar=1, tags=b"NMi\1\0\0\0"), Rec(ALL16 + "G", flag=0x10, name=b"bb"), Rec("TTGCA", flag=0x4, name=b"ccc")]
    hdr = bam_writer.header(refs=[(b"chr", 99)])
    stream = hdr + b"".join(r.encode() for r in recs)
    ends = {len(hdr): 0}
    at = len(hdr)
    for i, r in enumerate(recs):
        at += len(r.encode())
        ends[at] = i + 1
    ends[0] = 0  # nothing at all: an empty file holds no reads
    reads = bam_rule.reads_of(recs)
    for cut in range(len(stream) + 1):
        p = tmp_path / "t.bam"
        p.write_bytes(bam_writer.bgzf(stream[:cut], payload=(65280, 5)[cut % 2], eof=bool(cut % 3)))
        rc, msg, got = _call(p, 1 + cut % 3)
        if cut in ends:
            assert rc == 0 and got == _want(reads[:ends[cut]]), (cut, rc, msg, got)
        else:
            assert rc == EFORMAT and msg, (cut, rc, msg, got)


def test_bgzipped_fastq_stays_fastq(tmp_path, small_recs):
    reads = bam_rule.reads_of(small_recs)
    p = tmp_path / "r.fq.gz"
    p.write_bytes(bam_writer.bgzf(bam_rule.fastq_of(reads), payload=997))
    assert _ok(p, 3) == _want(reads)


def test_read_longer_than_2_23_is_refused(tmp_path):
    p = bam_writer.write(tmp_path / "long.bam", [Rec("ACGT", name=b"ok"), Rec("A" * ((1 << 23) + 1), name=b"long")])
    rc, msg, _ = _call(p, 2)
    assert rc == -75 and msg, (rc, msg)
