"""The resident sample read back byte for byte (a helper of tests/test_resident_readback.py and tests/test_gpu_resident_readback.py, not a test).

The observer: drprg_hip_select_reads with A = 1 and the four one-base anchors returns every resident read that holds at least one of ACGTacgt,
in block order then read order -- packed blocks upper-cased with N at the listed positions, ASCII blocks as the bytes of the file.  That is a
verbatim read-back of what the compaction kernels wrote (ss_pack_kernel, gather_reads_kernel, ss_npos_kernel / trim_npos_kernel, bam_pack_kernel,
the cut behind covg_cut_kernel); it needs no oracle.  What it cannot see: a read without an ACGT byte (its length is still held through the
counters) and the bits behind the last base in a block's last packed word.

The expected side is the rule modules composed (`pipeline`): read_trim_rule, read_filter_rule, max_covg_rule, dedup_rule, subsample_rule, in
the order the headers state.  Nothing here imports the product at module level; the batches are plain lists of bytes and numpy qualities, so
that their census can be taken without a device."""
import collections

import numpy as np

import bam_rule
import bam_writer
import dedup_rule
import max_covg_rule
import read_filter_rule
import read_trim_rule
import subsample_rule

ANCHORS, A = [0, 1, 2, 3], 1
NORMAL = bytes(c if c in b"ACGT" else (c - 32 if c in b"acgt" else ord("N")) for c in range(256))  # what a packed block can say of a byte
HAS_BASE = set(b"ACGTacgt")
FORMS = ("fastq ascii", "fastq packed", "bam", "fastq.gz")
EDGE_LENGTHS = (1, 15, 16, 17, 33)
IUPAC = b"RYKMSWBDHVN"  # (all of them letters of BAM's 4-bit code)
BLOCK_BASES = 750_000  # the ingest hands a worker's first block over there: a file below it is one block


def is_packed(form):
    """does the block that stays resident hold 2-bit letters (True) or the bytes of the file (False)?"""
    return form in ("fastq packed", "bam")


# ---- the observer ---------------------------------------------------------------------------------------------------------------------------
def read_back(ctx):
    """every resident read with an ACGT base, as bytes, and the ids the entry gives them"""
    bases, offs, ids = ctx.select_reads(ANCHORS, A)
    data = bases.tobytes()
    return [data[int(offs[i]):int(offs[i + 1])] for i in range(len(ids))], [int(x) for x in ids]


def expected(reads, packed):
    """what read_back must return for a sample of these reads (file bytes, in order): (the reads it returns, the indices of those it cannot)"""
    out, omitted = [], []
    for i, r in enumerate(reads):
        r = bytes(r)
        if HAS_BASE.isdisjoint(r):
            omitted.append(i)  # (an empty read among them)
        else:
            out.append(r.translate(NORMAL) if packed else r)
    return out, omitted


def kept_blocks(reads, blocks):
    """per read of the sample (kept block, read in that block) as the headers of drprg_hip_select_reads and drprg_hip_resident_info count: a
    block that kept no base is not a kept block.  blocks: the read counts of the blocks, in order"""
    assert sum(blocks) == len(reads), (sum(blocks), len(reads))
    where, at, kept = [], 0, 0
    for n in blocks:
        if sum(len(r) for r in reads[at:at + n]) == 0:
            where += [None] * n
        else:
            where += [(kept, j) for j in range(n)]
            kept += 1
        at += n
    return where, kept


def _starts(reads, blocks):
    """where each read starts in its block's base stream"""
    out, at = [], 0
    for n in blocks if blocks else [len(reads)]:
        pos = 0
        for r in reads[at:at + n]:
            out.append(pos)
            pos += len(r)
        at += n
    return out


def assert_resident(ctx, reads, packed, what, blocks=None, src=None):
    """the resident set of ctx is exactly `reads` (file bytes, in order; packed: normalised as a packed block stores them).  src (optional): per
    read, where its first base stood in the block the compaction read from -- named in the failure message"""
    reads = [bytes(r) for r in reads]
    want, omitted = expected(reads, packed)
    blind = set(omitted)
    returned = [i for i in range(len(reads)) if i not in blind]
    got, ids = read_back(ctx)
    dst = _starts(reads, blocks)
    for k in range(min(len(got), len(want))):
        if got[k] != want[k]:
            i = returned[k]
            p = next((p for p in range(min(len(got[k]), len(want[k]))) if got[k][p] != want[k][p]), min(len(got[k]), len(want[k])))
            raise AssertionError(f"{what}: read {i} (returned as number {k}) of {len(want[k])} bases, source phase {'?' if src is None else src[i] % 16}, "
                                 f"destination phase {dst[i] % 16}: {len(got[k])} bases came back, first difference at position {p}: "
                                 f"{got[k][max(p - 8, 0):p + 8]!r} for {want[k][max(p - 8, 0):p + 8]!r}")
    assert len(got) == len(want), f"{what}: {len(got)} reads came back, {len(want)} are expected"
    assert all(a < b for a, b in zip(ids, ids[1:])), f"{what}: the ids are not strictly ascending"
    cnt = ctx.counters()
    assert cnt["reads"] == len(reads) and cnt["bases"] == sum(len(r) for r in reads), (what, cnt["reads"], cnt["bases"], len(reads), sum(len(r) for r in reads))
    info = ctx.resident_info()
    assert info["complete"], (what, info)
    if blocks is not None:
        where, n_kept = kept_blocks(reads, blocks)
        assert info["blocks"] == n_kept, (what, info, n_kept)
        want_ids = [where[i][0] << 32 | where[i][1] for i in returned]
        bad = [k for k in range(len(ids)) if ids[k] != want_ids[k]]
        assert not bad, f"{what}: read {returned[bad[0]]} came back as block {ids[bad[0]] >> 32} read {ids[bad[0]] & 0xFFFFFFFF}, expected {where[returned[bad[0]]]}"


# ---- the pipeline as the rule modules state it ---------------------------------------------------------------------------------------------
Alive = collections.namedtuple("Alive", "index block seq qual src")  # src: where the first base stood in the block the stage's compaction reads
Stage = collections.namedtuple("Stage", "name alive flags")           # flags: the keep flags of a resident step over the reads it found, else None


def block_counts(alive, n_blocks):
    out = [0] * n_blocks
    for a in alive:
        out[a.block] += 1
    return out


def _block_of(cuts, n):
    out = []
    for b in range(len(cuts) - 1):
        out += [b] * (cuts[b + 1] - cuts[b])
    assert len(out) == n
    return out


def _resident_step(alive, flags, n_blocks):
    """what a compaction of the resident blocks leaves: the source of a kept read is its place in the block as it was"""
    starts = _starts([a.seq for a in alive], block_counts(alive, n_blocks))
    return [a._replace(src=starts[j]) for j, a in enumerate(alive) if flags[j]]


def pipeline(reads, quals, rev, settings):
    """the ingest and resident pipeline on reads given in read orientation (file bytes, Phred values or None, reverse-strand flags of the
    BAM form): trim, then filter, then the depth cap -- all at ingest, per block in file order --, then the resident steps in the order given.
    settings: cuts (block boundaries; default one block), front, tail, trim_qual, window, min_len, max_len, min_qual (whole Phred values),
    max_covg + genome_size, steps = [("dedup", key_bits) | ("subsample", target, seed), ...].  Returns a list of Stage: "trim", "filter",
    "cap", then one per step; `alive` are the reads alive after the stage."""
    s = dict(cuts=[0, len(reads)], front=0, tail=0, trim_qual=0, window=0, min_len=0, max_len=0, min_qual=0, max_covg=None, genome_size=0, steps=[])
    assert set(settings) <= set(s), set(settings) - set(s)
    s.update(settings)
    n_blocks = len(s["cuts"]) - 1
    block = _block_of(s["cuts"], len(reads))
    reads = [bytes(r) for r in reads]
    starts = _starts(reads, [s["cuts"][b + 1] - s["cuts"][b] for b in range(n_blocks)])
    milli = read_trim_rule.qual_milli(s["trim_qual"])
    stages, alive = [], []
    for i, r in enumerate(reads):  # trim: a BAM record of the reverse strand is trimmed in stored order and the range mirrored
        q = None if quals is None else np.asarray(quals[i])
        stored = None if q is None or not milli else (q[::-1] if rev[i] else q)
        a, b = read_trim_rule.kept_range_stored(stored, len(r), bool(rev[i]), s["front"], s["tail"], milli, s["window"])
        alive.append(Alive(i, block[i], r[a:b], None if q is None else q[a:b], starts[i] + a))
    stages.append(Stage("trim", alive, None))
    T = read_filter_rule.threshold(read_filter_rule.qual_milli(s["min_qual"])) if s["min_qual"] else 0
    alive = [a for a in alive if read_filter_rule.fate(len(a.seq), a.qual, s["min_len"], s["max_len"], T) == read_filter_rule.KEEP]
    stages.append(Stage("filter", alive, None))
    if s["max_covg"] is not None:
        n, _, _ = max_covg_rule.accepted_reads([len(a.seq) for a in alive], s["genome_size"], s["max_covg"])
        alive = alive[:n]
    stages.append(Stage("cap", alive, None))
    for step in s["steps"]:
        if step[0] == "dedup":
            flags = dedup_rule.keep_flags_fast([a.seq for a in alive])
        else:
            assert step[0] == "subsample", step
            flags = subsample_rule.keep_flags([len(a.seq) for a in alive], step[1], step[2])
        alive = _resident_step(alive, flags, n_blocks)
        stages.append(Stage(step[0], alive, flags))
    return stages


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
def bam_text(read):
    """a read as the BAM form can store it: upper case, N for what is no letter of the 4-bit code"""
    return "".join(ch if ch in bam_writer.CODES else "N" for ch in bytes(read).decode().upper())


def write_file(path, form, reads, quals, rev):
    """reads in read orientation -> one file in the given form.  The text forms go through tests/test_gpu_read_filter.py::_write_fastq (reads
    without qualities get 40 throughout).  The BAM form has a writer here: a reverse-strand record stores the reverse complement and QUAL
    mirrored, and the complement must know every letter of the 4-bit code, which _write_bam (ACGTN only) does not."""
    if form == "bam":
        recs = []
        for i, r in enumerate(reads):
            t = bam_text(r)
            q = None if quals is None else np.asarray(quals[i], dtype=np.uint8).tobytes()
            if rev[i]:
                recs.append(bam_writer.Rec("".join(bam_rule.COMPLEMENT[ch] for ch in reversed(t)), flag=0x10, name=b"r%d" % i, qual=None if q is None else q[::-1]))
            else:
                recs.append(bam_writer.Rec(t, flag=4, name=b"r%d" % i, qual=q))
        return str(bam_writer.write(path, recs))
    from test_gpu_read_filter import _write_fastq
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    q = [np.full(len(r), 40, dtype=np.uint8) for r in reads] if quals is None else [np.asarray(x, dtype=np.uint8) for x in quals]
    return _write_fastq(path, np.frombuffer(b"".join(bytes(r) for r in reads), dtype=np.uint8), offs, q, gz=form == "fastq.gz")


def write_blocks(d, tag, form, reads, quals, rev, cuts):
    """one file per block: reads [cuts[i], cuts[i + 1]) in file i"""
    ext = {"bam": "bam", "fastq.gz": "fq.gz"}.get(form, "fq")
    return [write_file(d / f"{tag}_{i}.{ext}", form, reads[cuts[i]:cuts[i + 1]], None if quals is None else quals[cuts[i]:cuts[i + 1]], rev[cuts[i]:cuts[i + 1]])
            for i in range(len(cuts) - 1)]


def as_form(reads, form):
    """the reads as the file of that form holds them (the BAM form cannot hold lower case or a byte outside its code)"""
    return [bam_text(r).encode() for r in reads] if form == "bam" else [bytes(r) for r in reads]


# ---- census: what a compaction has to get right, taken from the reference alone ---------------------------------------------------------------
def census(alive, n_blocks):
    """of the reads a compaction keeps: the (source start mod 16, destination start mod 16) pairs among those of 32 bases or more -- which hold
    a whole output word, so that the funnel shift runs at that pair of phases --, and the lengths that occur"""
    dst = _starts([a.seq for a in alive], block_counts(alive, n_blocks))
    pairs = {(a.src % 16, d % 16) for a, d in zip(alive, dst) if len(a.seq) >= 32}
    return pairs, {len(a.seq) for a in alive}


def unreturnable(alive):
    """(reads with bases the read-back cannot return, reads with bases)"""
    with_bases = [a for a in alive if len(a.seq)]
    return sum(1 for a in with_bases if HAS_BASE.isdisjoint(a.seq)), len(with_bases)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------------
Batch = collections.namedtuple("Batch", "reads quals rev cuts notes")


def _random_read(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)) if n else b""


def sprinkle(rng, read, rate=0.02):
    """lower case, IUPAC letters and N here and there; a read keeps at least one ACGT byte"""
    r = bytearray(read)
    for p in np.flatnonzero(rng.random(len(r)) < rate):
        r[p] = r[p] | 0x20 if rng.random() < 0.5 else IUPAC[int(rng.integers(0, len(IUPAC)))]
    return bytes(r) if not HAS_BASE.isdisjoint(r) else bytes(read)


def reverse_flags(n):
    return [i % 3 == 0 for i in range(n)]


_EDGE = {}  # the batches, made once
SOFT = 31  # bases at quality 19 behind the middle of a "soft" read of the trim batch
TRIM_SETTINGS = {
    "window 1": dict(trim_qual=20, window=1),
    "window 4": dict(trim_qual=20, window=4),
    "window 32": dict(trim_qual=20, window=32),
    "crops": dict(front=5, tail=3),
}


def trim_batch():
    """_trim_batch at the first seed under which the kept ranges cover all 256 phase pairs under every setting of TRIM_SETTINGS"""
    if "trim" not in _EDGE:
        for seed in range(1, 40):
            b = _trim_batch(seed)
            if all(len(census([a for a in pipeline(b.reads, b.quals, b.rev, dict(kw, cuts=b.cuts))[0].alive if a.seq], 3)[0]) == 256 for kw in TRIM_SETTINGS.values()):
                _EDGE["trim"] = b
                break
        else:
            raise AssertionError("no seed covers the compaction's edges")
    return _EDGE["trim"]


def _trim_batch(seed):
    """4 500 reads in three blocks.  Read i is a bad front of a bases (quality 2), a good middle of K bases (quality 40) and a bad tail of t
    bases: under a threshold of 20 the rule keeps the middle at window 1; with these two quality levels it keeps it at window 4 too unless
    K = 1, and at window 32 if K >= 16 and the read holds 32 bases (else the read is emptied).  notes["soft"]: five reads whose good middle of
    K = 1, 15, 16, 17, 33 bases stands at quality 93 and is followed by 31 bases at 19, one below the threshold: a window of up to 32 bases
    that starts on the middle is good by its mean, and the narrowing takes the 19s off again -- the word-edge lengths occur under every
    window.  notes["edges"]: reads with a = 5 and t = 3 -- the fixed crops of TRIM_SETTINGS, so that they
    sit on the same edges under every setting -- that hold a non-ACGT base on the last cut base of the front, the first kept base, the last
    kept base or the first cut base of the tail; forward and reverse-strand records of each."""
    rng = np.random.default_rng(seed)
    n = 4500
    spec = []
    for i in range(n):
        u = rng.random()
        K = int(rng.integers(32, 121)) if u < 0.7 else int(rng.choice(EDGE_LENGTHS)) if u < 0.8 else int(rng.integers(0, 41))
        a, t = (0, 0) if i % 11 == 0 else (int(rng.integers(0, 21)), int(rng.integers(0, 21)))
        spec.append([a, K, t])
    rev = reverse_flags(n)
    edges = {}
    at = 40
    for where in ("front cut", "first kept", "last kept", "tail cut"):
        for strand in (False, True):
            while rev[at] != strand:
                at += 1
            spec[at] = [5, 40 + at % 7, 3]
            edges[(where, strand)] = at
            at += 1501  # (one in every block)
            at %= n
    for j, K in enumerate(EDGE_LENGTHS):  # the edge lengths behind the fixed crops too
        spec[200 + j] = [5, K, 3]
    soft = {}
    for j, K in enumerate(EDGE_LENGTHS):  # ... and behind every window
        spec[210 + j] = [5, K, SOFT + 3]
        soft[210 + j] = K
    spec[10] = [4, 0, 4]     # no good base, and no base behind the crops: trimmed to nothing
    spec[11] = [0, 90, 0]    # untouched
    spec[12] = [5, 1, 3]     # its one kept base is N: the read-back cannot return it
    spec[13] = [5, 6, 3]     # its kept bases are all N
    spec[14] = [5, 40, 3]    # the same with a range that every window keeps
    reads, quals = [], []
    for i, (a, K, t) in enumerate(spec):
        r = sprinkle(rng, _random_read(rng, a + K + t))
        q = np.full(a + K + t, 2, dtype=np.uint8)
        q[a:a + K] = 40
        if i in soft:
            r = _random_read(rng, a + K + t)
            q[a:a + K], q[a + K:a + K + SOFT] = 93, 19
        reads.append(r)
        quals.append(q)
    for (where, _), i in edges.items():
        a, K, t = spec[i]
        p = {"front cut": a - 1, "first kept": a, "last kept": a + K - 1, "tail cut": a + K}[where]
        r = bytearray(_random_read(rng, a + K + t))
        r[p] = ord("N")
        reads[i] = bytes(r)
    reads[12] = reads[12][:5] + b"N" + reads[12][6:]
    reads[13] = reads[13][:5] + b"NNRNYN" + reads[13][11:]
    reads[14] = reads[14][:5] + b"NnRY" * 10 + reads[14][45:]
    return Batch(reads, quals, rev, [0, 1500, 3000, n], dict(spec=spec, edges=edges, soft=soft, emptied=10, untouched=11, unreturnable=(12, 13, 14)))


def edge_batch():
    """tests/test_gpu_subsample.py::_edge_batch (6 000 reads in three blocks, and the (target, seed) under which the subsample's selection
    covers all 256 phase pairs and the edge lengths) as a Batch; of its reads of N alone all but three get their base back, so that the
    read-back returns 98 % of the reads.  notes: T, seed, flags (the subsample's), panel"""
    if "batch" not in _EDGE:
        from test_gpu_subsample import _edge_batch
        panel, L, bases, offs, cuts, T, seed, flags = _edge_batch(with_n=True)
        data = bases.tobytes()
        reads = [data[int(offs[i]):int(offs[i + 1])] for i in range(len(L))]
        rng = np.random.default_rng(8)
        blind = [i for i, r in enumerate(reads) if r and HAS_BASE.isdisjoint(r)]
        for i in blind[3:]:
            reads[i] = _random_read(rng, len(reads[i]))
        _EDGE["batch"] = Batch(reads, None, reverse_flags(len(L)), list(cuts), dict(T=T, seed=seed, flags=list(flags), panel=panel))
    return _EDGE["batch"]


FILTER_SETTINGS = dict(min_len=1, min_qual=20)


def filter_batch():
    """edge_batch with qualities under which the read filter (FILTER_SETTINGS) drops exactly the reads the subsample drops there -- every base
    at 40 in a kept read, at 2 in a dropped one --, and the empty reads: the same phase pairs and lengths"""
    b = edge_batch()
    quals = [np.full(len(r), 40 if f else 2, dtype=np.uint8) for r, f in zip(b.reads, b.notes["flags"])]
    return b._replace(quals=quals)


def dedup_batch():
    """6 000 reads in four blocks: a small first block, then three in which about two reads in five are copies of a read in an EARLIER block.
    Every other read differs from all reads before it (reads too short for that become copies).  The first seed under which the rule's
    selection covers all 256 phase pairs and the edge lengths"""
    if "dedup" in _EDGE:
        return _EDGE["dedup"]
    cuts = [0, 600, 2400, 4200, 6000]
    for seed in range(1, 40):
        rng = np.random.default_rng(100 + seed)
        reads, seen, by_block = [], set(), [[] for _ in range(4)]
        for b in range(4):
            earlier = [r for blk in by_block[:b] for r in blk if r]
            for _ in range(cuts[b + 1] - cuts[b]):
                u = rng.random()
                L = int(rng.integers(32, 90)) if u < 0.72 else int(rng.choice(EDGE_LENGTHS)) if u < 0.9 else int(rng.integers(0, 41))
                r = None
                if len(reads) in (5, 5000):
                    r = b"NNNN" if len(reads) == 5 else b"nnRn"  # a read the read-back cannot return, and its copy in the last block
                elif L == 0:
                    r = b""
                elif not (earlier and rng.random() < 0.4):
                    for _ in range(8):
                        c = sprinkle(rng, _random_read(rng, L)) if L > 3 else _random_read(rng, L)
                        if c.translate(NORMAL) not in seen:
                            r = c
                            break
                if r is None:
                    same = [e for e in earlier if len(e) == L] if earlier else []
                    r = same[int(rng.integers(0, len(same)))] if same and rng.random() < 0.5 else (earlier[int(rng.integers(0, len(earlier)))] if earlier else None)
                    if r is None:
                        r = _random_read(rng, 41 + len(reads))  # (first block only: a length no other read has)
                seen.add(r.translate(NORMAL))
                reads.append(r)
                by_block[b].append(r)
        batch = Batch(reads, None, reverse_flags(len(reads)), cuts, dict(seed=seed))
        st = pipeline(reads, None, batch.rev, dict(cuts=cuts, steps=[("dedup", 64)]))[-1]
        pairs, lengths = census(st.alive, 4)
        if len(pairs) == 256 and set(EDGE_LENGTHS) <= lengths:
            _EDGE["dedup"] = batch
            return batch
    raise AssertionError("no seed covers the compaction's edges")


CAP_G, CAP_COVG = 10_000, 3  # the cap is reached at the 40 000-th base


def cap_batch(seed=5):
    """900 reads of 60 to 140 bases in three blocks; the cap of CAP_COVG at a genome of CAP_G bases cuts inside the second block.  The cut read
    and the reads either side of it hold a listed position; notes["cut"]: the last read accepted"""
    rng = np.random.default_rng(seed)
    n = 900
    reads = [sprinkle(rng, _random_read(rng, int(rng.integers(60, 141))), 0.01) for _ in range(n)]
    reads[7], reads[450] = b"", b""
    reads[20] = b"NNNNNNNNNNNNNNNNNNNN"  # the read-back cannot return it
    cut, _, reached = max_covg_rule.accepted_reads([len(r) for r in reads], CAP_G, CAP_COVG)
    assert reached
    cut -= 1
    for i, p in ((cut - 1, -1), (cut, 0), (cut, -1), (cut + 1, 0)):  # (no length changes: the cut stays where it is)
        r = bytearray(reads[i])
        r[p] = ord("N")
        reads[i] = bytes(r)
    return Batch(reads, None, reverse_flags(n), [0, 300, 600, n], dict(cut=cut))


TRIPWIRE_TRIM, TRIPWIRE_FILTER = dict(trim_qual=20, window=4), dict(min_qual=30)


def tripwire_batch(seed=6):
    """600 reads of 20 to 150 bases: a kept range at quality 40, every cut byte at 2.  Trimmed at 20 (window 4) and filtered at 30: one cut byte
    that leaks into the qualities the filter sums pulls the read's mean error above the bound -- tests/test_resident_readback.py holds the
    longest read to that"""
    rng = np.random.default_rng(seed)
    reads, quals = [], []
    for i in range(600):
        K = int(rng.integers(4, 131)) if i else 130
        a, t = (int(rng.integers(0, 11)), int(rng.integers(0, 11))) if i else (10, 10)
        if i % 7 == 3:
            a = 0
        if i % 7 == 5:
            t = 0
        q = np.full(a + K + t, 2, dtype=np.uint8)
        q[a:a + K] = 40
        reads.append(_random_read(rng, a + K + t))
        quals.append(q)
    reads[9], quals[9] = b"", np.zeros(0, np.uint8)
    reads[30] = b"NRYN" * 40  # a read the read-back cannot return (as long as no read here is: it still holds its kept range and cut bytes)
    reads[30] = reads[30][:len(quals[30])]
    return Batch(reads, quals, reverse_flags(600), [0, 600], dict(unreturnable=30))


VANISH_KINDS = ("trimmed to nothing", "filtered away", "empty reads only")


def vanish_batch(kind, seed=9):
    """three blocks of 300 reads of which the middle one leaves no base: its reads have no good window, or fail the filter, or are empty.  A
    third of the last block's reads are copies of reads of the first.  Returns the batch and the settings that make the block vanish"""
    rng = np.random.default_rng(seed)
    reads, quals = [], []
    for i in range(900):
        L = int(rng.integers(1, 120))
        if 300 <= i < 600 and kind == "empty reads only":
            L = 0
        if i >= 600 and i % 3 == 0:
            j = int(rng.integers(0, 300))
            reads.append(reads[j])
            quals.append(quals[j])
            continue
        reads.append(sprinkle(rng, _random_read(rng, L)))
        quals.append(np.full(L, 2 if 300 <= i < 600 else 40, dtype=np.uint8))
    reads[3], quals[3] = b"NNNNRNNN", np.full(8, 40, dtype=np.uint8)
    settings = {"trimmed to nothing": dict(trim_qual=20, window=4), "filtered away": dict(min_qual=20), "empty reads only": {}}[kind]
    return Batch(reads, quals, reverse_flags(900), [0, 300, 600, 900], {}), settings


def composed_batch(seed=12):
    """about 4 000 reads of 0 to 600 bases cut from the test panel's genomes, in three blocks, with bad ends, bad reads and planted duplicates
    (bases and qualities alike), and the settings of the composed run: trim, filter, a depth cap that cuts in the third block, two dedups, two
    subsamples.  notes: settings, panel"""
    if "composed" in _EDGE:
        return _EDGE["composed"]
    from test_gpu_max_covg import _panel, _reads_of
    panel, genomes = _panel()
    rng = np.random.default_rng(seed)
    n = 4000
    u = rng.random(n)
    L = np.where(u < 0.5, rng.integers(0, 151, size=n), np.where(u < 0.85, rng.integers(150, 401, size=n), rng.integers(400, 601, size=n)))
    L[5], L[1700], L[-1] = 0, 0, 600
    L = [int(x) for x in L]
    bases, offs = _reads_of(genomes, L, seed=seed)
    data = bases.tobytes()
    reads, quals = [], []
    for i in range(n):
        if i >= 200 and i % 6 == 0:  # a duplicate of an earlier read, often of an earlier block
            j = int(rng.integers(0, i))
            reads.append(reads[j])
            quals.append(quals[j])
            continue
        q = rng.integers(25, 41, size=L[i])
        kind = i % 8
        if kind in (1, 3):
            q[:int(rng.integers(3, 40))] = rng.integers(2, 15)
        if kind in (2, 3):
            q[max(L[i] - int(rng.integers(3, 60)), 0):] = rng.integers(2, 15)
        if kind == 5 and i % 16 == 5:
            q[:] = rng.integers(2, 14, size=L[i])  # bad all over
        if kind == 7 and i % 16 == 7:
            q[:] = 21  # survives the trim, fails the filter
        reads.append(sprinkle(rng, data[int(offs[i]):int(offs[i + 1])], 0.004))
        quals.append(q.astype(np.uint8))
    # reads the read-back cannot return, good enough to pass the trim and the filter: N and IUPAC letters alone, all of different lengths (two
    # of one length are duplicates under the rule: every base masked), in the first two blocks; and a copy of the first in each later block
    blind = [20 + 130 * j for j in range(20)]
    for j, i in enumerate(blind):
        reads[i], quals[i] = (b"NRYKMN" * 20)[:45 + j], np.full(45 + j, 35, dtype=np.uint8)
    for i in (1400, 2800):
        reads[i], quals[i] = reads[blind[0]], quals[blind[0]]
    cuts = [0, 1300, 2700, n]
    settings = dict(cuts=cuts, front=3, tail=2, trim_qual=20, window=4, min_len=30, max_len=500, min_qual=25)
    alive = pipeline(reads, quals, reverse_flags(n), settings)[1].alive
    per_block = [sum(len(a.seq) for a in alive if a.block == b) for b in range(3)]
    G = 10_000
    settings.update(genome_size=G, max_covg=(per_block[0] + per_block[1] + per_block[2] // 2) // G - 1)
    after = pipeline(reads, quals, reverse_flags(n), dict(settings, steps=[("dedup", 64)]))[-1].alive
    total = sum(len(a.seq) for a in after)
    settings["steps"] = [("dedup", 64), ("dedup", 3), ("subsample", total * 3 // 5, 11), ("subsample", total // 4, 12)]
    _EDGE["composed"] = Batch(reads, quals, reverse_flags(n), cuts, dict(settings=settings, panel=panel, blind=blind, blind_copies=(1400, 2800)))
    return _EDGE["composed"]
