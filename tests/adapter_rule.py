"""Adapter trimming (include/drprg_hip.h "adapter trimming") in plain Python, written from the rule's text and not from the kernel, and the
fixtures of tests/test_adapter_rule.py and tests/test_gpu_adapter_trim.py.

The rule.  Settings: 1 to 4 adapters of 1 to 64 letters ACGTacgt, an error rate E in [0, 0.5] with at most three places held as per-mille e,
a minimum overlap O (default 3, or the shortest adapter's length if that is smaller).  In the range [x, y) the crops and the quality trim
left, n = y - x: a start p in 0..n-1 matches an adapter A of m letters iff c = min(m, n - p) >= O and at most floor(c * e / 1000) of the
j < c have read[x + p + j] != A[j] (case-insensitive; a base that is not ACGT differs from every letter).  The read is cut at the smallest
matching p over all adapters: end = x + p."""
from decimal import Decimal

import numpy as np

MAX_ADAPTERS, MAX_LEN, MAX_ERROR_MILLI, DEFAULT_ERROR, DEFAULT_MIN_OVERLAP = 4, 64, 500, "0.1", 3
TILE, WAVE, LANE, SLOTS = 16384, 1024, 16, 1024  # bases per workgroup, wave and lane of adapter_points_kernel; reads per workgroup table

# the start of Illumina's TruSeq adapter with one index filled in (64 letters; its prefixes are the shorter adapters), and Nextera's (19)
TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCACGATCTCGTATGCCGTCTTCTGCTTG"
NEXTERA = "CTGTCTCTTATACACATCT"
assert len(TRUSEQ) == 64 and len(NEXTERA) == 19


def error_milli(E):
    m = Decimal(str(E)) * 1000
    if m != m.to_integral_value() or not 0 <= m <= MAX_ERROR_MILLI:
        raise ValueError(E)
    return int(m)


def min_overlap(adapters, O=0):
    return O if O else min(DEFAULT_MIN_OVERLAP, min(len(a) for a in adapters))


def _upper(b):
    """bytes / array -> upper-cased uint8 array in which everything that is not ACGT is 0"""
    r = np.frombuffer(bytes(b), dtype=np.uint8) & 0xDF
    return np.where((r == 65) | (r == 67) | (r == 71) | (r == 84), r, 0).astype(np.uint8)


def cut_point(read, adapters, e, O, x=0, y=None):
    """the smallest matching start counted from x, or None"""
    r = _upper(read)[x:len(read) if y is None else y]
    n = r.size
    if n == 0:
        return None
    best = None
    left = n - np.arange(n)  # bases from p to the end of the range
    for A in adapters:
        a = _upper(A.encode() if isinstance(A, str) else A)
        m = a.size
        miss = np.zeros(n, dtype=np.int64)
        for j in range(min(m, n)):  # letter j of the adapter against base p + j, for every p that has one
            miss[:n - j] += (r[j:] != a[j]) | (r[j:] == 0)
        c = np.minimum(m, left)
        ok = (c >= O) & (miss <= c * e // 1000)
        hit = np.flatnonzero(ok)
        if hit.size and (best is None or hit[0] < best):
            best = int(hit[0])
    return best


def cut_ranges(reads, ranges, adapters, e, O):
    """[(begin, end)] behind the adapter cut, and the five counts of drprg_hip_adapter_trim_info"""
    out = []
    info = dict(reads_seen=len(reads), bases_seen=0, reads_cut=0, bases_cut=0, reads_emptied=0)
    for r, (x, y) in zip(reads, ranges):
        p = cut_point(r, adapters, e, O, x, y) if y > x else None
        info["bases_seen"] += y - x
        if p is not None:
            info["reads_cut"] += 1
            info["bases_cut"] += y - x - p
            info["reads_emptied"] += p == 0
            y = x + p
        out.append((x, y))
    return out, info


def adapters_of(name):
    """the adapter sets of the kernel test by name: a length of the TruSeq prefix, or the pair"""
    return [TRUSEQ[:33], NEXTERA] if name == "33+19" else [TRUSEQ[:int(name)]]


def mutate(rng, seq, k, forbid=()):
    """seq with k substitutions at distinct places outside `forbid`; returns (bytes, places)"""
    s = bytearray(seq.encode() if isinstance(seq, str) else seq)
    places = [int(i) for i in rng.permutation([i for i in range(len(s)) if i not in forbid])[:k]]
    assert len(places) == k
    for i in places:
        s[i] = ord(rng.choice([c for c in "ACGT" if c != chr(s[i]).upper()]))
    return bytes(s), places


def kernel_batch(name, E):
    """The ragged batch of the kernel test for one adapter set and error rate: dict(reads, ranges, classes, adapters, e, O).  classes: name ->
    (read indices, "cut" | "none" | "mixed" | "any"): what the rule must say of them -- a cut in every read, in none, in some and not in others.
    Every read with an intended outcome is redrawn until the rule says exactly that, so that filler cannot match by accident."""
    adapters = adapters_of(name)
    A = adapters[0]
    m, e, O = len(A), error_milli(E), min_overlap(adapters)
    rng = np.random.default_rng(1000 * len(name) + m + e)
    reads, ranges, classes = [], [], {}

    def lim(c):
        return c * e // 1000

    def filler(n):
        return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))

    def pos():
        return sum(len(r) for r in reads)

    def add(cls, kind, make, want="?"):
        """make() -> bytes or (bytes, (begin, end)); want: the intended cut (int), None for no cut, "?" for whatever the rule says"""
        for _ in range(400):
            made = make()
            r, rg = made if isinstance(made, tuple) else (made, (0, len(made)))
            if want == "?" or cut_point(r, adapters, e, O, rg[0], rg[1]) == want:
                break
        else:
            raise AssertionError((cls, want))
        reads.append(r)
        ranges.append(rg)
        classes.setdefault(cls, ([], kind))[0].append(len(reads) - 1)

    def pad_to(at, cls="filler"):
        """filler reads up to absolute position at - 1 (at least one base is left for the next read's own filler)"""
        while at - pos() > 700:
            add(cls, "any", lambda: filler(int(rng.integers(100, 600))))

    def occurrence_at(cls, at, before=40):
        """a read whose occurrence of A starts at absolute position `at`, read-through followed by random bases"""
        pad_to(at - before)
        lead = at - pos()
        assert lead >= 1
        add(cls, "cut", lambda: filler(lead) + A.encode() + filler(int(rng.integers(0, 20))), lead)
        assert pos() - len(reads[-1]) + lead == at

    # more reads of 3 to 8 bases inside the first tile than a workgroup's table holds, some ending in an adapter prefix
    for i in range(SLOTS + 176):
        n = int(rng.integers(3, 9))
        add("short run", "mixed", (lambda n=n: filler(n - O) + A[:O].encode()) if i % 4 == 0 else (lambda n=n: filler(n)))
    assert len(reads) >= 1100 and pos() < TILE - 1000
    # reads of 0, 1, O - 1, O, m - 1, m and m + 1 bases without an adapter, and the adapter itself
    for n in (0, 1, O - 1, O, m - 1, m, m + 1):
        add("edge lengths", "none", lambda n=n: filler(n), None)
    add("the adapter itself", "cut", lambda: A.encode(), 0)
    # a partial overlap of every length at a read's end
    for k in range(1, m):
        add("partial below O" if k < O else "partial from O", "none" if k < O else "cut", lambda k=k: filler(30) + A[:k].encode(), None if k < O else 30)
    # exactly the allowed number of mismatches, and one more: the whole adapter, and partial overlaps on both sides of a step of the floor
    steps = [c for c in range(max(O, 2), m) if lim(c) != lim(c - 1)][:2]
    partial = sorted({c for s in steps for c in (s - 1, s) if c >= O}) or [m - 1]
    classes["partial lengths"] = (partial, "any")
    for c in [m] + partial:
        tail = (lambda: filler(10)) if c == m else (lambda: b"")
        add("at the limit", "cut", lambda c=c, tail=tail: filler(40) + mutate(rng, A[:c], lim(c))[0] + tail(), 40)
        add("one over the limit", "none", lambda c=c, tail=tail: filler(40) + mutate(rng, A[:c], lim(c) + 1)[0] + tail(), None)

    # a base that is not ACGT inside an occurrence: in place of a mismatch it changes nothing, beside the allowed mismatches it tips it over
    def with_n(extra):
        s, places = mutate(rng, A, lim(m))
        s = bytearray(s)
        at = int(rng.choice([i for i in range(m) if i not in places])) if extra or not places else places[0]
        s[at] = ord("N")
        return filler(40) + bytes(s) + filler(10)
    if lim(m):
        add("N for a mismatch", "cut", lambda: with_n(False), 40)
    add("N over the limit", "none", lambda: with_n(True), None)
    # two occurrences, and a worse but acceptable match to the left of a perfect one: the leftmost wins
    add("two occurrences", "cut", lambda: filler(30) + A.encode() + filler(20) + A.encode() + filler(5), 30)
    add("worse to the left", "cut", lambda: filler(30) + mutate(rng, A, lim(m))[0] + filler(20) + A.encode(), 30)
    # neighbours: A[0:2] | A[2:] cuts nothing at the boundary, A[0:5] | A[5:] takes five bases off the first read
    add("split 2", "none", lambda: filler(30) + A[:2].encode(), None)
    add("split rest", "any", lambda: A[2:].encode() + filler(20))
    add("split 5", "cut", lambda: filler(30) + A[:5].encode(), 30)
    add("split rest", "any", lambda: A[5:].encode() + filler(20))
    add("lower case", "cut", lambda: (filler(30) + A.encode() + filler(7)).lower(), 30)
    if len(adapters) > 1:
        add("second adapter", "cut", lambda: filler(30) + adapters[1].encode() + filler(10), 30)
        add("second adapter", "cut", lambda: filler(30) + adapters[1][:7].encode(), 30)
    # ranges narrower than the read: an occurrence that straddles `end` counts as partial, one that starts before `begin` is not found
    half = max(O, m // 2)
    add("straddles end", "cut", lambda: (filler(30) + A.encode() + filler(20), (0, 30 + half)), 30)
    add("straddles end below O", "none", lambda: (filler(30) + A.encode() + filler(20), (3, 30 + O - 1)), None)
    add("starts before begin", "none", lambda: (filler(30) + A.encode() + filler(20), (32, 50 + m)), None)
    add("inside the range", "cut", lambda: (filler(30) + A.encode() + filler(20), (10, 45 + m)), 20)
    # occurrences across a lane's 16-start boundary and across a wave boundary
    at = (pos() + 100) // LANE * LANE + LANE
    occurrence_at("across a lane boundary", (at if at % WAVE else at + LANE) - 2)
    occurrence_at("across a wave boundary", (pos() + 100) // WAVE * WAVE + WAVE - 3)
    # across tile boundaries: by one base, and by m - 1
    assert pos() < TILE - m - 40, pos()
    occurrence_at("across a tile boundary by 1", TILE - (m - 1))
    # a read of more than 20 000 bases with the adapter at 18 000, so that whole waves lie under one read; the occurrence crosses the third
    # tile boundary by m - 1 bases; and a second such read without the adapter
    pad_to(3 * TILE - 1 - 18000)
    add("filler", "any", lambda: filler(3 * TILE - 1 - 18000 - pos()))
    add("long with adapter", "cut", lambda: filler(18000) + A.encode() + filler(2500), 18000)
    assert pos() - len(reads[-1]) + 18000 == 3 * TILE - 1
    classes["across a tile boundary by m - 1"] = ([len(reads) - 1], "cut")
    add("long without adapter", "none", lambda: filler(20500), None)
    return dict(reads=reads, ranges=ranges, classes=classes, adapters=adapters, e=e, O=O)


def census(batch):
    """the rule's verdict per class: name -> (reads with a cut, reads without); raises if a class is not what it is meant to be"""
    cuts, _ = cut_ranges(batch["reads"], batch["ranges"], batch["adapters"], batch["e"], batch["O"])
    out = {}
    for name, (idx, kind) in batch["classes"].items():
        if name == "partial lengths":
            continue
        n_cut = sum(cuts[i] != batch["ranges"][i] for i in idx)
        out[name] = (n_cut, len(idx) - n_cut)
        assert idx and (kind != "cut" or n_cut == len(idx)) and (kind != "none" or n_cut == 0) and (kind != "mixed" or 0 < n_cut < len(idx)), (name, kind, out[name])
    return out


def packed_form(text):
    """the 2-bit words (A0 C1 T2 G3, first base lowest) and the ascending list of the bases that are not ACGT, as the ingest packs a block"""
    b = np.frombuffer(bytes(text), dtype=np.uint8)
    n = b.size
    code = np.zeros((n + 15) // 16 * 16, dtype=np.uint32)
    code[:n] = (b >> 1) & 3
    words = (code.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
    return words, np.flatnonzero(_upper(b) == 0).astype(np.uint64)


def plant(bases, offs, adapter, O, seed):
    """A sample's reads with adapters inserted, by turns: read-through (the read's end replaced by the adapter and up to 20 random bases), a
    partial adapter of O .. m - 1 letters appended, and nothing -- the turn shifted by one every three reads, so that the records the BAM
    fixtures store on the reverse strand (every third) are of every kind.  Returns (reads as bytes, kinds)."""
    rng = np.random.default_rng(seed)
    reads, kinds = [], []
    for i in range(len(offs) - 1):
        r = bytes(bases[int(offs[i]):int(offs[i + 1])])
        kind = ("through", "partial", "none")[(i + i // 3) % 3] if len(r) >= 40 else "none"
        if kind == "through":
            p = int(rng.integers(len(r) // 2, len(r)))
            r = r[:p] + adapter.encode() + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(0, 21))))
        elif kind == "partial":
            r = r + adapter[:int(rng.integers(O, len(adapter)))].encode()
        reads.append(r)
        kinds.append(kind)
    return reads, kinds
