"""The resident-read selection behind discover (include/drprg_hip.h: drprg_hip_select_reads -- Mapper::select_reads_with_anchors,
anchor_scan.hip, the windowed expansion of packed blocks) against a plain statement of its rule.

The rule (anchor_scan.hip's header): a kept block is ONE base stream; read r of it is selected iff some position p with
off[r] <= p < off[r + 1] and p + A <= n_bases has stream[p:p + A] all ACGTacgt and, upper-cased, equal to an anchor.  `ref_select` below says
that with bytes slicing and a set of anchor strings -- no packed k-mers, no prefilter, no binary search, nothing shared with denovo.cpp or
synth.  Where the layout of the blocks is not known to the test (several parser threads, several devices) two layout-free bounds hold:
  must: an anchor lies wholly inside the read                               (selected whatever stands behind the read)
  may:  must, or a proper all-ACGT suffix of the read is a prefix of an anchor   (selected only if the next reads complete it)

Exact cases are one FASTQ file far below one ingest block (the first hand-over comes at 1/16 of a block = 768 kB) read by ONE parser thread:
the block's stream is the file's reads in order, asserted through resident_info()["blocks"] == 1.  The anchors of these cases are 'A' followed
by letters of CGT and the filler is CGT only, so the occurrences are the planted ones and no others (an anchor shifted against itself never
matches: its only 'A' would have to stand at another place) -- the recipe checks, which run without a GPU, hold the builders to that.

Zero-length records: map_fastx KEEPS them (a record with an empty sequence line is a read of no bases: it counts in counters()["reads"], has
two equal offsets in its block and is never selected, since no position lies in it); `test_read_boundaries` places three.

What these tests cannot see, by construction of the code: a prefilter that passes every k-mer (the exact search behind it decides, so the
output is the same and only the time differs), and `end > n_bases` in place of `end >= n_bases` (the byte at n_bases is 'N' in an expansion and
never-written padding in an ASCII block: no base in any state a test can set up).  Dropping `run < A`, bases in the look-behind of the first
span and a `done` that stays 0 in the window loop do fail them.

Reads of the exact cases are told apart by the id the entry returns (kept block << 32 | read in the block); the returned bytes are compared
with the read of that id (reads of 1 or 14 bases cannot all be unique, the others are)."""
import bisect
import collections
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from util import ROOT

W, K = 11, 15
EINVAL, ENODATA, EOVERFLOW = 22, 61, 75  # DependencyError.code of DRPRG_EINVAL / DRPRG_ENODATA / DRPRG_EOVERFLOW (csrc/common.h)
AS = (1, 8, 9, 15, 16, 17, 31)
ALIAS = {ord("A"): b"H", ord("C"): b"B", ord("G"): b"N", ord("T"): b"U"}  # bytes whose 2-bit letter in anchor_scan.hip is that base's


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def ref_select(stream, offs, anchors, A):
    """the reads of one block's stream the rule selects, ascending.  (w.upper() is an anchor <=> w is all ACGTacgt and spells one: bytes.upper
    changes a-z only and every anchor is upper-case ACGT, which is asserted.)"""
    S = set(anchors)
    assert all(len(a) == A and set(a) <= set(b"ACGT") for a in S)
    n, out = len(stream), []
    for r in range(len(offs) - 1):
        for p in range(offs[r], offs[r + 1]):
            if p + A <= n and stream[p:p + A].upper() in S:
                out.append(r)
                break
    return out


def ref_must(read, anchors, A):
    S = set(anchors)
    return any(read[p:p + A].upper() in S for p in range(len(read) - A + 1))


def anchor_prefixes(anchors, A):
    return {a[:j] for a in anchors for j in range(1, A)}


def ref_suffix(read, prefixes, A):
    """a proper suffix of the read is a prefix of an anchor (all ACGT then, as the anchors are)"""
    return any(read[len(read) - j:].upper() in prefixes for j in range(1, min(A - 1, len(read)) + 1))


def ref_may(read, anchors, A):
    return ref_must(read, anchors, A) or ref_suffix(read, anchor_prefixes(anchors, A), A)


def fast_must(reads, anchors):
    """{i: ref_must(reads[i])} for upper-case reads, for the 300 k-read sample: bytes.find over the reads joined by newlines instead of a slice
    per position (an anchor holds no newline, so an occurrence lies inside one read); test_the_two_statements_of_must_agree"""
    text, starts, out = b"\n".join(reads), [0], set()
    for r in reads:
        starts.append(starts[-1] + len(r) + 1)
    for a in anchors:
        at = text.find(a)
        while at >= 0:
            out.add(bisect.bisect_right(starts, at) - 1)
            at = text.find(a, at + 1)
    return out


def code(kmer):
    """the u64 the C entry takes: 2 bits per base, A 0 C 1 G 2 T 3, first base in the high bits"""
    v = 0
    for c in kmer:
        v = v << 2 | b"ACGT".index(c)
    return v


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def make_anchors(rng, A, n):
    """n different anchors: 'A' + A - 1 letters of CGT (A = 1: the one anchor 'A')"""
    out = set()
    while len(out) < min(n, 3 ** (A - 1)):
        out.add(b"A" + bytes(rng.choice(np.frombuffer(b"CGT", np.uint8), size=A - 1)))
    return sorted(out)


def filler(rng, n):
    return bytearray(bytes(rng.choice(np.frombuffer(b"CGT", np.uint8), size=n)))


def cut(stream, lens):
    assert sum(lens) == len(stream)
    offs = [0]
    for l in lens:
        offs.append(offs[-1] + l)
    return [bytes(stream[offs[i]:offs[i + 1]]) for i in range(len(lens))], offs


def plant(stream, plants):
    """stream[p:p + len(s)] = s for every (p, s); the plants must not touch"""
    last = -1
    for p, s in sorted(plants):
        assert p > last and p + len(s) <= len(stream), (p, last)
        stream[p:p + len(s)] = s
        last = p + len(s)
    return stream


def occurrences(stream, anchors, A):
    S = set(anchors)
    return [p for p in range(len(stream) - A + 1) if bytes(stream[p:p + A]).upper() in S]


def boundary_case(A, seed=1):
    """~30 kB (three and a half 8 KB workgroups, fourteen 2 KB waves) in reads of 97 bases; every 2048 j is straddled by an occurrence (A = 1:
    one ends at 2048 j - 1 and one starts at 2048 j), and every other read that is free holds one occurrence whose END position runs through
    the residues mod 32.  Returns reads, offs, anchors, planted start positions."""
    rng = np.random.default_rng(seed + A)
    n_reads, L = 300, 97
    N = n_reads * L
    anchors = make_anchors(rng, A, 3)
    stream, plants, busy = filler(rng, N), [], set()
    for i in range(1, N // 2048 + 1):
        B = 2048 * i
        p = (B - 1 if i % 2 else B) if A == 1 else B - 1 - (i * 7) % (A - 1)  # A > 1: p < B <= p + A - 1
        plants.append((p, anchors[i % len(anchors)]))
        busy.update(range((p - A) // L, (p + 2 * A) // L + 1))
    k = 0
    for r in range(0, n_reads, 2):
        if r in busy:
            continue
        lo = r * L
        # end position lo + x + A - 1 == k (mod 32), the occurrence wholly inside the read
        x = (k - (lo + A - 1)) % 32
        x += 32 * ((r // 2) % ((L - A - x) // 32 + 1))
        assert x + A <= L
        plants.append((lo + x, anchors[k % len(anchors)]))
        k += 1
    plant(stream, plants)
    reads, offs = cut(stream, [L] * n_reads)
    return reads, offs, anchors, sorted(p for p, _ in plants)


def head_case(A, p, seed=2):
    rng = np.random.default_rng(seed)
    anchors = make_anchors(rng, A, 2)
    # p = -1: the stream opens with the last A - 1 bases of an anchor (what stands in front of the stream is no base)
    stream = plant(filler(rng, 7 * 23), [(p, anchors[0])] if p >= 0 else [(0, anchors[0][1:])])
    reads, offs = cut(stream, [23] * 7)
    return reads, offs, anchors


def tail_case(A, residue, whole, seed=3):
    """n_bases == residue (mod 32); the stream ends with a whole anchor, or with its first A - 1 bases only"""
    rng = np.random.default_rng(seed)
    anchors = make_anchors(rng, A, 2)
    lens = [41] * 4
    last = A + 3
    while (sum(lens) + last) % 32 != residue:
        last += 1
    lens.append(last)
    N = sum(lens)
    stream = filler(rng, N)
    tail = anchors[-1] if whole else anchors[-1][:A - 1]
    plant(stream, [(N - len(tail), tail)])
    reads, offs = cut(stream, lens)
    return reads, offs, anchors


def run_logic_case(A, seed=4):
    """reads of 64: per position of the anchor one read in which that base is replaced by the byte with the same 2-bit letter (not
    selected); then N in front of an intact occurrence, a lower-case and a mixed-case occurrence (selected); filler reads in between"""
    rng = np.random.default_rng(seed)
    anchors = make_anchors(rng, A, 2)
    a = anchors[0]
    texts = [a[:i] + ALIAS[a[i]] + a[i + 1:] for i in range(A)]
    texts += [b"N" + a, a.lower(), bytes(c | 0x20 if i % 2 else c for i, c in enumerate(a))]
    reads = []
    for i, t in enumerate(texts):
        r = filler(rng, 64)
        at = 1 + (i * 5) % (64 - len(t) - 1)
        r[at:at + len(t)] = t
        reads += [bytes(r), bytes(filler(rng, 33))]
    offs = [0]
    for r in reads:
        offs.append(offs[-1] + len(r))
    want = [2 * i for i in range(A, A + 3)]
    return reads, offs, anchors, want


def search_case(n, A=15, seed=5):
    """n anchors; reads that hold the first, a middle and the last entry of the sorted anchor array, one that shares only the low 16 bits (the last
    8 bases) with an anchor, one that shares everything but them, one with two different anchors and one with the same anchor five times"""
    rng = np.random.default_rng(seed + n)
    anchors = make_anchors(rng, A, n)
    assert len(anchors) == n and anchors == sorted(anchors, key=code)
    S = set(anchors)
    picks = sorted({0, n // 2, n - 1})
    other = lambda k: bytes(rng.choice(np.frombuffer(b"CGT", np.uint8), size=k))
    while True:
        low_only = b"A" + other(A - 9) + anchors[n // 2][A - 8:]
        high_only = anchors[n // 2][:A - 8] + other(8)
        if low_only not in S and high_only not in S:
            break
    texts = [anchors[i] for i in picks] + [low_only, high_only, anchors[0] + b"C" + anchors[n - 1], (anchors[n // 2] + b"G") * 5]
    reads = []
    for i, t in enumerate(texts):
        r = filler(rng, 120)
        at = 3 + 2 * i
        r[at:at + len(t)] = t
        reads += [bytes(r), bytes(filler(rng, 50))]
    offs = [0]
    for r in reads:
        offs.append(offs[-1] + len(r))
    want = [2 * i for i in range(len(picks))] + [2 * (len(picks) + 2), 2 * (len(picks) + 3)]
    passed = anchors + [anchors[i] for i in picks] + anchors[: n // 3]  # duplicates, and not sorted any more
    return reads, offs, anchors, passed, want


def boundary_reads_case(A=15, seed=6):
    """occurrences over read boundaries at every split, the listed read lengths, zero-length records.  Returns reads, offs, anchors, want"""
    rng = np.random.default_rng(seed)
    anchors = make_anchors(rng, A, 3)
    a = anchors[1]
    reads, want = [b""], []  # (a zero-length record opens the file)

    def add(text, selected):
        if selected:
            want.append(len(reads))
        reads.append(bytes(text))

    for s in range(0, A):  # s bases of the occurrence in the first read of the pair, the rest opens the second; s = 0: all in the second
        add(filler(rng, 40 - s) + a[:s], s > 0)
        add(a[s:] + filler(rng, 40 - (A - s)), s == 0)
    add(filler(rng, 30) + a[:6], True)  # ... and through a zero-length record, which is never selected itself
    add(b"", False)
    add(a[6:] + filler(rng, 30), False)
    add(a[:1], True)  # length 1: the first base of an occurrence that runs on through the next reads
    add(a[1:A - 1], False)  # length A - 2
    add(a[A - 1:] + filler(rng, 20), False)
    add(a[:A - 1], True)  # length A - 1, completed by the next read
    add(a[A - 1:] + filler(rng, 9), False)
    add(a, True)  # length A
    add(filler(rng, 1), False)  # length 1, no base of an anchor ('A' never is filler)
    for L in (63, 64, 65, 150):  # the anchor ends the read (gather tails of 63, 0, 1 and 22 bytes over whole 64-byte trips)
        add(filler(rng, L - A) + anchors[2], True)
        add(filler(rng, L), False)
    long_read = filler(rng, 70000)
    long_read[69000:69000 + A] = anchors[0]
    add(long_read, True)
    add(filler(rng, 70000), False)
    add(filler(rng, 20) + a[:A - 1], False)  # the stream ends inside an occurrence
    add(b"", False)  # (a zero-length record ends the file)
    offs = [0]
    for r in reads:
        offs.append(offs[-1] + len(r))
    return reads, offs, anchors, want


def extremes_case(all_selected, A=15, seed=7):
    rng = np.random.default_rng(seed)
    anchors = make_anchors(rng, A, 4)
    reads = []
    for i in range(130):
        r = filler(rng, 50 + i % 7)
        if all_selected:
            r[i % 30:i % 30 + A] = anchors[i % 4]
        reads.append(bytes(r))
    offs = [0]
    for r in reads:
        offs.append(offs[-1] + len(r))
    return reads, offs, anchors


# ---- recipe checks (no GPU): the builders place what they say, and the reference says what the rule says ---------------------------------
def test_the_reference_on_examples_worked_by_hand():
    #          0         1
    #          0123456789012345
    stream = b"CCACGTTTacgGNACG"
    offs = [0, 4, 4, 9, 16]  # reads CCAC | (empty) | GTTTa | cgGNACG
    assert ref_select(stream, offs, [b"ACG"], 3) == [0, 2, 3]  # 2..4 starts in read 0 and runs into read 2; 8..10 "acg" starts in read 2; 13..15 ends the stream
    assert ref_select(stream, offs, [b"CGG", b"GAA", b"GGA"], 3) == [3]  # "cgG" at 9; the N in "GNA" stands for no base
    assert ref_select(stream, offs, [b"ACGT"], 4) == [0]  # 13..16 would need a base behind the stream
    assert ref_select(stream, offs, [b"T"], 1) == [2] and ref_select(stream, offs, [b"A"], 1) == [0, 2, 3]
    assert ref_select(stream, offs, [b"GGG"], 3) == [] and ref_select(b"", [0], [b"A"], 1) == []
    reads = [stream[offs[i]:offs[i + 1]] for i in range(4)]
    assert [ref_must(r, [b"ACG"], 3) for r in reads] == [False, False, False, True]
    assert [ref_may(r, [b"ACG"], 3) for r in reads] == [True, False, True, True]  # "AC" ends read 0, "a" ends read 2
    assert not ref_may(b"CCAN", [b"ACG"], 3) and ref_may(b"CCNA", [b"ACG"], 3)
    assert code(b"A") == 0 and code(b"ACGT") == 0b00011011 and code(b"T" * 31) == 2 ** 62 - 1


def test_the_two_statements_of_must_agree():
    rng = np.random.default_rng(11)
    anchors = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=4)) for _ in range(6)]
    reads = [_fold(bytes(rng.choice(np.frombuffer(b"ACGTacgtNn", np.uint8), size=int(rng.integers(0, 24))))) for i in range(3000)]
    want = {i for i, r in enumerate(reads) if ref_must(r, anchors, 4)}
    assert fast_must(reads, anchors) == want and 100 < len(want) < 2900
    assert _fold(b"acgtNnxACGT-") == b"ACGTNNNACGTN"


@pytest.mark.parametrize("A", AS)
def test_recipe_boundaries(A):
    reads, offs, anchors, planted = boundary_case(A)
    stream = b"".join(reads)
    assert len(stream) >= 3 * 8192 + 2048 and occurrences(stream, anchors, A) == planted  # the planted occurrences and no others
    assert {(p + A - 1) % 32 for p in planted if offs[bisect.bisect_right(offs, p) - 1] + 97 >= p + A} == set(range(32))
    for i in range(1, len(stream) // 2048 + 1):
        B = 2048 * i
        if A > 1:
            assert any(p < B <= p + A - 1 for p in planted), B
        else:
            assert B - 1 in planted or B in planted
    want = ref_select(stream, offs, anchors, A)
    assert want == sorted({bisect.bisect_right(offs, p) - 1 for p in planted}) and 100 < len(want) < 200


def test_recipe_head_tail_run_search_and_read_boundaries():
    for A in (1, 15, 31):
        for p in sorted({0, 1, A - 1, A, 31, 32, 33}):
            reads, offs, anchors = head_case(A, p)
            assert occurrences(b"".join(reads), anchors, A) == [p]
            assert ref_select(b"".join(reads), offs, anchors, A) == [p // 23]
        if A > 1:
            reads, offs, anchors = head_case(A, -1)
            assert b"".join(reads).startswith(anchors[0][1:]) and ref_select(b"".join(reads), offs, anchors, A) == []
        for residue in (0, 1, 15, 16, 17, 31):
            for whole in (True, False):
                reads, offs, anchors = tail_case(A, residue, whole)
                stream = b"".join(reads)
                assert len(stream) % 32 == residue
                assert occurrences(stream, anchors, A) == ([len(stream) - A] if whole else [])
                assert ref_select(stream, offs, anchors, A) == ([4] if whole else [])
    for A in (8, 15, 31):
        reads, offs, anchors, want = run_logic_case(A)
        assert ref_select(b"".join(reads), offs, anchors, A) == want and len(reads) == 2 * (A + 3)
        # every rejected read spells the anchor in 2-bit letters: only the run of true bases tells it apart
        letter = lambda c: ((c >> 1) & 3) ^ ((c >> 2) & 1)
        for i in range(A):
            r = reads[2 * i]
            assert any([letter(c) for c in r[p:p + A]] == [letter(c) for c in anchors[0]] for p in range(len(r) - A + 1))
    for n in (1, 2, 1000):
        reads, offs, anchors, passed, want = search_case(n)
        assert ref_select(b"".join(reads), offs, passed, 15) == want and len(passed) > len(set(passed)) == n
        lows, highs = {code(a) & 0xFFFF for a in anchors}, {code(a) >> 16 for a in anchors}
        k = len(want) - 2
        assert any(code(reads[2 * k][p:p + 15]) & 0xFFFF in lows for p in range(100) if b"A" == reads[2 * k][p:p + 1])
        assert any(code(reads[2 * k + 2][p:p + 15]) >> 16 in highs for p in range(100) if b"A" == reads[2 * k + 2][p:p + 1])
    reads, offs, anchors, want = boundary_reads_case()
    assert ref_select(b"".join(reads), offs, anchors, 15) == want
    assert {len(r) for r in reads} >= {0, 1, 14, 15, 63, 64, 65, 150, 70000} and len(b"".join(reads)) < 700000
    for all_selected in (False, True):
        reads, offs, anchors = extremes_case(all_selected)
        assert ref_select(b"".join(reads), offs, anchors, 15) == (list(range(130)) if all_selected else [])


# ---- the device side ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prg(tmp_path_factory):
    from drprg_amd import synth
    d = tmp_path_factory.mktemp("selection_prg")
    synth.small_panel(seed=31, n_loci=3, length=900, site_every=60).write(str(d / "dr.prg"), str(d / "genes.fa"))
    return str(d / "dr.prg")


def _context(prg, **kw):
    from drprg_amd import Context
    ctx = Context(prg, W, K, from_files=False, **({"device": 0} if "devices" not in kw else kw))
    ctx.set_opts(illumina=True, genome_size=4000)
    return ctx


def _write_fastq(path, reads):
    with open(path, "wb") as fh:
        for i, s in enumerate(reads):
            fh.write(b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n")
    return str(path)


def _keep_one_block(ctx, fq, reads, packed):
    """the file, read by one parser thread, kept as the one block whose stream is the file's reads in order"""
    ctx.reset()
    ctx.set_threads(1)
    ctx.set_input_format(packed)
    ctx.keep_reads(1 << 28)
    ctx.map_fastx(fq)
    info = ctx.resident_info()
    assert info["complete"] and info["blocks"] == 1, info
    assert ctx.counters()["reads"] == len(reads)  # zero-length records included


def _split(bases, offsets):
    b = bases.tobytes()
    assert offsets[0] == 0 and offsets[-1] == len(b) and np.all(np.diff(offsets.astype(np.int64)) >= 0)
    return [b[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def check_exact(ctx, tmp_path, name, reads, offs, anchors, A, want=None, passed=None, window_bytes=0):
    """both kept forms of one exact case: ids == the reference's list, in order, each read once, its bytes, consistent offsets"""
    stream = b"".join(reads)
    ref = ref_select(stream, offs, anchors, A)
    if want is not None:
        assert ref == want
    fq = _write_fastq(tmp_path / (name + ".fq"), reads)
    codes = [code(a) for a in (passed if passed is not None else anchors)]
    for packed in (False, True):
        _keep_one_block(ctx, fq, reads, packed)
        bases, offsets, ids = ctx.select_reads(codes, A, window_bytes)
        got = [int(i) for i in ids]
        assert got == ref, (name, A, packed, got, ref)  # (block 0: the id is the read; ascending and without repeats as the reference's list is)
        seqs = _split(bases, offsets)
        assert len(seqs) == len(ref)
        for r, s in zip(ref, seqs):
            # a packed block returns upper case, and N for every byte that is no base
            assert s == (_fold(reads[r]) if packed else reads[r]), (name, A, packed, r)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("A", AS)
def test_span_wave_and_workgroup_boundaries(tmp_path, prg, A):
    reads, offs, anchors, planted = boundary_case(A)
    check_exact(_context(prg), tmp_path, "boundaries", reads, offs, anchors, A)


@pytest.mark.gpu
@pytest.mark.parametrize("A", (1, 15, 31))
def test_stream_head_and_tail(tmp_path, prg, A):
    ctx = _context(prg)
    for p in sorted({0, 1, A - 1, A, 31, 32, 33}):
        reads, offs, anchors = head_case(A, p)
        check_exact(ctx, tmp_path, "head%d" % p, reads, offs, anchors, A, want=[p // 23])
    if A > 1:
        reads, offs, anchors = head_case(A, -1)
        check_exact(ctx, tmp_path, "head_cut", reads, offs, anchors, A, want=[])
    for residue in (0, 1, 15, 16, 17, 31):
        for whole in (True, False):
            reads, offs, anchors = tail_case(A, residue, whole)
            check_exact(ctx, tmp_path, "tail%d_%d" % (residue, whole), reads, offs, anchors, A, want=[4] if whole else [])


@pytest.mark.gpu
@pytest.mark.parametrize("A", (8, 15, 31))
def test_run_logic(tmp_path, prg, A):
    reads, offs, anchors, want = run_logic_case(A)
    check_exact(_context(prg), tmp_path, "run", reads, offs, anchors, A, want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 2, 1000))
def test_anchor_search(tmp_path, prg, n):
    reads, offs, anchors, passed, want = search_case(n)
    check_exact(_context(prg), tmp_path, "search", reads, offs, anchors, 15, want=want, passed=passed)


@pytest.mark.gpu
def test_read_boundaries(tmp_path, prg):
    reads, offs, anchors, want = boundary_reads_case()
    ctx = _context(prg)
    check_exact(ctx, tmp_path, "reads", reads, offs, anchors, 15, want=want)
    check_exact(ctx, tmp_path, "reads_w1", reads, offs, anchors, 15, want=want, window_bytes=1)


@pytest.mark.gpu
def test_no_read_and_every_read(tmp_path, prg):
    ctx = _context(prg)
    reads, offs, anchors = extremes_case(False)
    check_exact(ctx, tmp_path, "none", reads, offs, anchors, 15, want=[])
    bases, offsets, ids = ctx.select_reads([code(a) for a in anchors], 15)
    assert bases.size == 0 and ids.size == 0 and offsets.tolist() == [0]
    bases, offsets, ids = ctx.select_reads([], 15)  # no anchors: no reads
    assert bases.size == 0 and ids.size == 0 and offsets.tolist() == [0]
    reads, offs, anchors = extremes_case(True)
    assert check_exact(ctx, tmp_path, "all", reads, offs, anchors, 15) == list(range(len(reads)))  # the list's capacity is the block's reads


# ---- bound cases: the layout of the blocks is the parser threads' -------------------------------------------------------------------------
def _fastq_reads(fq):
    return [line.rstrip(b"\n") for i, line in enumerate(open(fq, "rb")) if i % 4 == 1]


def _revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def _bound_anchors(panel, reads, A=15):
    """anchors as discover has them -- A-mers of the loci, either strand -- and A-mers that open and close reads of the background"""
    out = set()
    for ref in panel.refs:
        for at in (200, 415, 700):
            out.add(ref[at:at + A].encode())
    for r in (reads[1000], reads[77777 % len(reads)]):
        if set(r) <= set(b"ACGT"):
            out.update((r[:A], r[-A:]))
    return sorted(out | {_revcomp(a) for a in out})


_FOLD = bytes(c if c in b"ACGT" else ord("N") for c in range(256))
_bounds_cache = {}


def _fold(s):
    """what a packed block returns for a read: upper case, N for every byte that is no base"""
    return s.upper().translate(_FOLD)


def check_bounds(ctx, reads, anchors, A, window_bytes=0, few=True):
    """must <= got <= may as multisets of case-folded reads (the samples of test_resident repeat reads), nothing returned twice, ids ascending"""
    key = (id(reads), tuple(anchors))
    if key not in _bounds_cache:  # (the reference side once per sample and anchor set)
        have = collections.Counter(_fold(r) for r in reads)
        distinct = sorted(have)
        _bounds_cache[key] = have, {distinct[i] for i in fast_must(distinct, anchors)}, anchor_prefixes(anchors, A), set()
    have, must, prefixes, may = _bounds_cache[key]  # (may: the reads found to satisfy it so far)
    assert len(must) > 50
    bases, offsets, ids = ctx.select_reads([code(a) for a in anchors], A, window_bytes)
    ids = [int(i) for i in ids]
    assert all(x < y for x, y in zip(ids, ids[1:]))  # blocks are numbered through the mappers: ascending per mapper, and no id twice
    got = collections.Counter(_fold(s) for s in _split(bases, offsets))
    for x in must:
        assert got[x] == have[x], x  # every copy of a read that holds an anchor, once
    for x, n in got.items():
        assert n <= have[x], x  # bytes of a read of the file, no more often than the file has it
        if x not in must and x not in may:
            assert ref_suffix(x, prefixes, A), x  # (not in must: may is the suffix rule alone)
            may.add(x)
    if few:  # 15-mers and longer do not occur by chance in these samples: the 2700 reads of the loci at most, and a handful
        assert sum(got.values()) < 3000
    return ids, bases.tobytes()


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """the sample of test_resident's test_many_blocks_and_reads_without_anchors"""
    from test_resident import _sample
    d = tmp_path_factory.mktemp("selection_many")
    panel, prg, genes, fq = _sample(d, n_background=300000, odd_bases=True)
    reads = _fastq_reads(fq)
    return panel, prg, fq, reads, _bound_anchors(panel, reads)


def _keep(prg, fq, packed, threads=8, **kw):
    ctx = _context(prg, **kw)
    ctx.set_threads(threads)
    ctx.set_input_format(packed)
    ctx.keep_reads(1 << 30)
    ctx.map_fastx(fq)
    assert ctx.resident_info()["complete"]
    return ctx


@pytest.mark.gpu
def test_many_blocks_kept_ascii(many):
    panel, prg, fq, reads, anchors = many
    ctx = _keep(prg, fq, False)
    assert ctx.resident_info()["blocks"] >= 2
    check_bounds(ctx, reads, anchors, 15)


@pytest.mark.gpu
def test_many_blocks_kept_packed_and_the_windows(many):
    """the expansion a window at a time: at least three windows, a block larger than the window, every block alone -- what one window returns"""
    panel, prg, fq, reads, anchors = many
    ctx = _keep(prg, fq, True)
    blocks, n_bases = ctx.resident_info()["blocks"], sum(len(r) for r in reads)
    assert blocks >= 3
    want = check_bounds(ctx, reads, anchors, 15)
    # a block holds at most 12 M bases (expanded: + 80 bytes at most), so a 14 MB window takes whole blocks and never more than 14 MB:
    # 45 M bases need four of them
    assert n_bases // (14 << 20) + 1 >= 3
    assert check_bounds(ctx, reads, anchors, 15, window_bytes=14 << 20) == want
    # the largest block holds at least the mean: above 1 MB it stands alone in a window that it exceeds, and the others form more windows
    assert n_bases / blocks > 1 << 20
    assert check_bounds(ctx, reads, anchors, 15, window_bytes=1 << 20) == want
    assert check_bounds(ctx, reads, anchors, 15, window_bytes=1) == want  # as many windows as blocks (>= 3)
    # ... and anchors of another length: every A-mer of a slice of a locus, as the local assembly sends them
    for A in (9,):
        slice_ = panel.refs[1][300:300 + 2 * A + 20].encode()
        kmers = sorted({slice_[i:i + A] for i in range(len(slice_) - A + 1)} | {_revcomp(slice_)[i:i + A] for i in range(len(slice_) - A + 1)})
        # (9-mers do occur by chance: ~100 k-mers x 45 M bases / 4^9 = some 17 k occurrences in the background; the bounds hold them all the same)
        assert check_bounds(ctx, reads, kmers, A, window_bytes=1, few=A > 9) == check_bounds(ctx, reads, kmers, A, few=A > 9)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from test_resident import _sample
    out = []
    for seed in (4, 5):
        d = tmp_path_factory.mktemp("selection_small%d" % seed)
        panel, prg, genes, fq = _sample(d, n_background=20000, odd_bases=True, seed=seed)
        out.append((panel, prg, fq, _fastq_reads(fq)))
    return out


@pytest.mark.gpu
def test_two_mappers_on_one_device(small):
    panel, prg, fq, reads = small[0]
    for packed in (False, True):
        ctx = _keep(prg, fq, packed, threads=4, devices=[0, 0])
        assert ctx.resident_info()["blocks"] >= 2
        anchors = _bound_anchors(panel, reads)
        assert check_bounds(ctx, reads, anchors, 15) == check_bounds(ctx, reads, anchors, 15, window_bytes=1)


@pytest.mark.gpu
def test_ascii_and_packed_blocks_in_one_context(small):
    (panel, prg, fq, reads), (_, _, fq2, reads2) = small  # (the same panel: small_panel's seed is fixed; other reads)
    ctx = _context(prg)
    ctx.set_threads(4)
    ctx.keep_reads(1 << 30)
    ctx.map_fastx(fq)
    ctx.set_input_format(True)
    ctx.map_fastx(fq2)
    info = ctx.resident_info()
    assert info["complete"] and info["blocks"] >= 2
    both = reads + reads2
    anchors = _bound_anchors(panel, both)
    assert check_bounds(ctx, both, anchors, 15) == check_bounds(ctx, both, anchors, 15, window_bytes=1)


# ---- agreement with discover ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_read_the_oracle_pile_up_counts_is_selected(tmp_path):
    """a test_resident sample: the reads the oracle's pile-up (oracle/oracle_denovo.py pile_up) counts as spanning hold an anchor of that run
    wholly (must), and select_reads returns every one of them for the run's anchors"""
    from test_resident import _discover, _sample
    spec = importlib.util.spec_from_file_location("oracle_denovo", os.path.join(ROOT, "oracle", "oracle_denovo.py"))
    od = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(od)
    panel, prg, genes, fq = _sample(tmp_path, kind="snp")
    ctx, variants = _discover(prg, genes, fq, tmp_path / "hbm", 1 << 30)
    assert ctx.resident_info()["last_discover_from_hbm"] and len(variants) == 1
    cons, A = dict(zip(panel.names, panel.refs)), 15
    regions = [(f[0], int(f[1]), int(f[2])) for f in (l.split("\t") for l in open(tmp_path / "hbm" / "candidate_regions.tsv") if not l.startswith("#"))]
    regions = [(l, s, e) for l, s, e in regions if s >= A and e + A <= len(cons[l])]
    anchors = set()
    for l, s, e in regions:
        for a in (cons[l][s - A:s], cons[l][e:e + A]):
            anchors.update((a.encode(), od.revcomp(a).encode()))
    reads = _fastq_reads(fq)
    # pile_up's spanning rule, read by read: both anchors of a region, in this order, as far apart as the region +- 30, bases only in between
    spanning, votes = [], 0
    for read in reads:
        text = read.decode().upper()
        n = 0
        for l, s, e in regions:
            left, right = cons[l][s - A:s], cons[l][e:e + A]
            for first, second in ((left, right), (od.revcomp(right), od.revcomp(left))):
                ok = [(x, y) for x in od._occurrences(text, first) for y in od._occurrences(text, second)
                      if y >= x + A and abs((y - x - A) - (e - s)) <= 30]
                if len(text) >= 2 * A and ok and set(text[ok[0][0] + A:ok[0][1]]) <= set("ACGT"):
                    n += 1
        if n:
            spanning.append(read)
            votes += n
    assert votes == sum(v[5] for v in variants) and len(spanning) >= 3  # the oracle's own count of spanning reads
    bases, offsets, ids = ctx.select_reads([code(a) for a in sorted(anchors)], A)
    got, have = collections.Counter(_split(bases, offsets)), collections.Counter(reads)
    for read in spanning:
        assert ref_must(read, anchors, A) and got[read] == have[read], read


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(tmp_path, prg):
    from drprg_amd._lib import lib
    from drprg_amd.pandora import DependencyError
    reads, offs, anchors = extremes_case(True)
    fq = _write_fastq(tmp_path / "all.fq", reads)
    codes = [code(a) for a in anchors]
    ctx = _context(prg)
    with pytest.raises(DependencyError) as err:  # nothing kept
        ctx.select_reads(codes, 15)
    assert err.value.code == ENODATA
    ctx.map_fastx(fq)
    ctx.keep_reads(1 << 28)  # reads were mapped before: what is kept from now on is not the sample
    ctx.map_fastx(fq)
    assert not ctx.resident_info()["complete"]
    with pytest.raises(DependencyError) as err:
        ctx.select_reads(codes, 15)
    assert err.value.code == ENODATA
    _keep_one_block(ctx, fq, reads, False)
    for A in (0, 32):
        with pytest.raises(DependencyError) as err:
            ctx.select_reads(codes, A)
        assert err.value.code == EINVAL, A
    want = ctx.select_reads(codes, 15)
    n_reads, n_bases = len(reads), len(b"".join(reads))
    assert want[2].tolist() == list(range(n_reads)) and want[0].size == n_bases
    arr = np.asarray(codes, np.uint64)
    for short_reads, short_bases in ((1, 0), (0, 1), (n_reads, n_bases)):
        bases, offsets, ids = np.full(n_bases, 7, np.uint8), np.full(n_reads + 1, 7, np.uint64), np.full(n_reads, 7, np.uint64)
        out = (C.c_uint64 * 2)()
        rc = lib.drprg_hip_select_reads(ctx._h, arr.ctypes.data, arr.size, 15, 0, bases.ctypes.data, n_bases - short_bases, offsets.ctypes.data,
                                        ids.ctypes.data, n_reads - short_reads, out)
        assert rc == -EOVERFLOW and (out[0], out[1]) == (n_reads, n_bases)  # the sizes needed
        assert np.all(bases == 7) and np.all(offsets == 7) and np.all(ids == 7)  # nothing was copied
        again = ctx.select_reads(codes, 15)  # the context is as usable as before
        assert all(np.array_equal(x, y) for x, y in zip(again, want))
