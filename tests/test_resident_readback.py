"""The exact read-back's reference side on the CPU (tests/resident_readback.py): `expected` and `pipeline` on hand-written cases, and the
census of the batches tests/test_gpu_resident_readback.py compacts -- taken from the reference alone, so that the GPU tests cannot pass
vacuously: every (source phase, destination phase) pair of the funnel shift, the word-edge lengths, listed positions on every edge of a
kept range, and few enough reads the observer cannot return."""
import numpy as np
import pytest

import read_filter_rule
import resident_readback as rb
from resident_readback import Alive, census, expected, pipeline


def _seqs(stage):
    return [a.seq for a in stage.alive]


# ---- expected ---------------------------------------------------------------------------------------------------------------------------------
def test_expected_on_hand_written_reads():
    reads = [b"ACGT", b"acgt", b"AcGn", b"ARYKMSWBDHVC", b"NNNN", b"", b"nnrn", b"N", b"A", b"=.-*t"]
    got, omitted = expected(reads, packed=False)
    assert got == [b"ACGT", b"acgt", b"AcGn", b"ARYKMSWBDHVC", b"A", b"=.-*t"] and omitted == [4, 5, 6, 7]
    got, omitted = expected(reads, packed=True)
    assert got == [b"ACGT", b"ACGT", b"ACGN", b"ANNNNNNNNNNC", b"A", b"NNNNT"] and omitted == [4, 5, 6, 7]
    assert expected([], True) == ([], []) and expected([b"", b""], False) == ([], [0, 1])
    # the numbering the headers state: a block that kept no base is not a kept block
    where, kept = rb.kept_blocks([b"AC", b"", b"", b"", b"N", b"G"], [2, 2, 2])
    assert kept == 2 and where == [(0, 0), (0, 1), None, None, (1, 0), (1, 1)]
    assert rb.kept_blocks([b"", b"A"], [1, 0, 1]) == ([None, (0, 0)], 1)
    # what the BAM form can store of a read
    assert rb.as_form([b"acgRn.x"], "bam") == [b"ACGRNNN"] and rb.as_form([b"acgRn.x"], "fastq.gz") == [b"acgRn.x"]


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------------------
Q = lambda *v: np.array(v, dtype=np.uint8)  # noqa: E731


def test_pipeline_trims_before_it_filters_before_it_caps():
    reads = [b"AACCGGTT", b"ACGTACGT", b"TTTT", b"", b"GGGGGGGGGG", b"CCCCCC"]
    quals = [Q(2, 2, 40, 40, 40, 40, 2, 2), Q(*[40] * 8), Q(2, 2, 2, 2), Q(), Q(*[40] * 10), Q(*[40] * 6)]
    rev = [False, True, False, False, True, False]
    st = pipeline(reads, quals, rev, dict(trim_qual=20, window=1))
    assert [s.name for s in st] == ["trim", "filter", "cap"]
    assert _seqs(st[0]) == [b"CCGG", b"ACGTACGT", b"", b"", b"GGGGGGGGGG", b"CCCCCC"] == _seqs(st[1]) == _seqs(st[2])
    assert [a.src for a in st[0].alive] == [2, 8, 16, 20, 20, 30]  # the first kept base in the file's stream (an emptied read: its start)
    assert st[0].alive[0].qual.tolist() == [40] * 4
    # the length bound sees the trimmed read: 8 bases in the file, 4 behind the trim
    st = pipeline(reads, quals, rev, dict(trim_qual=20, window=1, min_len=5))
    assert _seqs(st[0])[0] == b"CCGG" and _seqs(st[1]) == [b"ACGTACGT", b"GGGGGGGGGG", b"CCCCCC"]
    # ... and so does the mean quality: untrimmed the first read fails Q 30 (four bases at 2), trimmed it passes
    assert read_filter_rule.fate(8, quals[0], 0, 0, read_filter_rule.threshold(30000)) == read_filter_rule.LOWQ
    st = pipeline(reads, quals, rev, dict(trim_qual=20, window=1, min_qual=30, min_len=1))
    assert _seqs(st[1]) == [b"CCGG", b"ACGTACGT", b"GGGGGGGGGG", b"CCCCCC"]
    # the cap counts what the filter kept: T = (0 + 1) * 12 is reached by the second kept read, 4 + 8 bases
    st = pipeline(reads, quals, rev, dict(trim_qual=20, window=1, min_len=1, max_covg=0, genome_size=12))
    assert _seqs(st[2]) == [b"CCGG", b"ACGTACGT"]
    # untrimmed it would have been reached by the second read of the file as well, but at 16 bases; one base more in the genome and it is the third
    assert _seqs(pipeline(reads, quals, rev, dict(min_len=1, max_covg=0, genome_size=17))[2]) == [b"AACCGGTT", b"ACGTACGT", b"TTTT"]
    # fixed crops on a reverse-strand record cut the READ's front and tail, whatever the stored order
    st = pipeline([b"AACCGGTT"], [Q(*[40] * 8)], [True], dict(front=3, tail=1))
    assert _seqs(st[0]) == [b"CGGT"]
    # window 4: a lone good base is no good window
    assert _seqs(pipeline([b"ACGTA"], [Q(2, 2, 40, 2, 2)], [False], dict(trim_qual=20, window=4))[0]) == [b""]
    assert _seqs(pipeline([b"ACGTA"], [Q(2, 2, 40, 2, 2)], [False], dict(trim_qual=20, window=1))[0]) == [b"G"]


def test_pipeline_dedups_before_it_subsamples_and_numbers_through_the_blocks():
    from subsample_rule import keep_flags
    reads = [b"ACGT", b"", b"acgt", b"ACGN", b"ACGR", b"TTTTTTTT", b"", b"ACGT", b"TTTTTTTT", b"GG"]
    cuts = [0, 4, 7, 10]
    st = pipeline(reads, None, [False] * 10, dict(cuts=cuts, steps=[("dedup", 64), ("dedup", 3)]))
    assert [s.name for s in st] == ["trim", "filter", "cap", "dedup", "dedup"]
    assert st[3].flags == [1, 1, 0, 1, 0, 1, 1, 0, 0, 1]  # case and the kind of masked byte do not tell reads apart; empty reads always stay
    assert [a.index for a in st[3].alive] == [0, 1, 3, 5, 6, 9] and [a.block for a in st[3].alive] == [0, 0, 0, 1, 1, 2]
    assert [a.src for a in st[3].alive] == [0, 4, 8, 4, 12, 12]  # where the read stood in its block before the step
    assert st[4].flags == [1] * 6 and _seqs(st[4]) == _seqs(st[3])
    assert rb.block_counts(st[3].alive, 3) == [3, 2, 1]
    # the subsample numbers what the dedup left: 6 reads, not 10
    L = [len(s) for s in _seqs(st[3])]
    for seed in (1, 2, 3):
        two = pipeline(reads, None, [False] * 10, dict(cuts=cuts, steps=[("dedup", 64), ("subsample", 9, seed)]))
        assert two[4].flags == keep_flags(L, 9, seed) and len(two[4].flags) == 6
        other = pipeline(reads, None, [False] * 10, dict(cuts=cuts, steps=[("subsample", 9, seed), ("dedup", 64)]))
        assert other[3].flags == keep_flags([len(r) for r in reads], 9, seed)
    # ingest stages come first whatever the resident steps are: the filter drops the empty reads before the dedup numbers them
    st = pipeline(reads, None, [False] * 10, dict(cuts=cuts, min_len=1, steps=[("dedup", 64)]))
    assert len(st[3].flags) == 8 and [a.index for a in st[3].alive] == [0, 3, 5, 9]


def test_census_counts_phases_of_whole_word_reads_only():
    alive = [Alive(0, 0, b"A" * 32, None, 5), Alive(1, 0, b"C" * 31, None, 40), Alive(2, 0, b"G" * 40, None, 80), Alive(3, 1, b"T" * 33, None, 7)]
    pairs, lengths = census(alive, 2)
    assert pairs == {(5, 0), (0, 15), (7, 0)} and lengths == {32, 31, 40, 33}


# ---- the batches of the GPU tests ------------------------------------------------------------------------------------------------------------
def _few_blind(alive, on_purpose=1):
    blind, with_bases = rb.unreturnable(alive)
    assert on_purpose <= blind <= 0.02 * with_bases, (blind, with_bases)


@pytest.mark.parametrize("name", list(rb.TRIM_SETTINGS))
def test_census_of_the_trim_batch(name):
    b = rb.trim_batch()
    kw = rb.TRIM_SETTINGS[name]
    st = pipeline(b.reads, b.quals, b.rev, dict(kw, cuts=b.cuts))[0]
    pairs, lengths = census([a for a in st.alive if a.seq], 3)
    assert len(pairs) == 256, sorted(set((s, d) for s in range(16) for d in range(16)) - pairs)[:8]
    # the word-edge lengths, under every setting: behind the crops from the reads of 8 bases more, behind every window from the "soft" reads,
    # whose neighbours one below the threshold make the window good and are narrowed away again
    assert set(rb.EDGE_LENGTHS) <= lengths
    if "trim_qual" in kw:
        assert sorted(len(st.alive[i].seq) for i in b.notes["soft"]) == sorted(rb.EDGE_LENGTHS)
        assert all(st.alive[i].seq == b.reads[i][5:5 + k] for i, k in b.notes["soft"].items())
    # a listed position on every edge of the kept range, for a forward and for a reverse-strand record -- the reads of notes["edges"] sit on
    # the same edges under every setting
    for (where, strand), i in b.notes["edges"].items():
        a = st.alive[i]
        r = b.reads[i]
        at = a.src - rb._starts(b.reads, [1500] * 3)[i]
        assert b.rev[i] == strand and len(a.seq) >= 40 and at == 5 and at + len(a.seq) == len(r) - 3
        p = {"front cut": at - 1, "first kept": at, "last kept": at + len(a.seq) - 1, "tail cut": at + len(a.seq)}[where]
        assert r[p] == ord("N") and set(r[:p] + r[p + 1:]) <= set(b"ACGT")
    assert len({i // 1500 for i in b.notes["edges"].values()}) == 3
    assert b.reads[b.notes["emptied"]] and not st.alive[b.notes["emptied"]].seq
    if "front" not in kw:  # (a fixed crop touches every read that has a base)
        assert st.alive[b.notes["untouched"]].seq == b.reads[b.notes["untouched"]] != b""
    assert sum(1 for a, r in zip(st.alive, b.reads) if r and not a.seq) >= 10
    for i in b.notes["unreturnable"]:  # (a window longer than their range empties the first two)
        assert rb.HAS_BASE.isdisjoint(st.alive[i].seq) and (st.alive[i].seq or i != b.notes["unreturnable"][-1])
    _few_blind(st.alive, 1)
    assert sum(len(r) for r in b.reads) < 3 * rb.BLOCK_BASES / 4 and len(b.reads) <= 6000


def test_census_of_the_subsample_and_the_filter_batch():
    b = rb.edge_batch()
    T, seed = b.notes["T"], b.notes["seed"]
    sub = pipeline(b.reads, None, b.rev, dict(cuts=b.cuts, steps=[("subsample", T, seed)]))[-1]
    assert sub.flags == b.notes["flags"]
    f = rb.filter_batch()
    fil = pipeline(f.reads, f.quals, f.rev, dict(rb.FILTER_SETTINGS, cuts=f.cuts))[1]
    # the filter keeps the reads with bases the subsample keeps, at the places it keeps them
    assert [a.index for a in fil.alive] == [a.index for a in sub.alive if a.seq]
    for st in (sub, fil):
        pairs, lengths = census([a for a in st.alive if a.seq], 3)
        assert len(pairs) == 256 and set(rb.EDGE_LENGTHS) <= lengths
        _few_blind(st.alive)
    _few_blind([Alive(i, 0, r, None, 0) for i, r in enumerate(b.reads)], 3)
    assert max(sum(len(r) for r in b.reads[lo:hi]) for lo, hi in zip(b.cuts, b.cuts[1:])) < rb.BLOCK_BASES and len(b.reads) <= 6000


def test_census_of_the_dedup_batch():
    b = rb.dedup_batch()
    st = pipeline(b.reads, None, b.rev, dict(cuts=b.cuts, steps=[("dedup", 64)]))[-1]
    pairs, lengths = census([a for a in st.alive if a.seq], 4)
    assert len(pairs) == 256 and set(rb.EDGE_LENGTHS) <= lengths
    # every dropped read's first copy lies in an earlier block
    first, block = {}, rb._block_of(b.cuts, len(b.reads))
    dropped = 0
    for i, (r, keep) in enumerate(zip(b.reads, st.flags)):
        t = r.translate(rb.NORMAL)
        if keep:
            first.setdefault(t, i)
        else:
            dropped += 1
            assert block[first[t]] < block[i], (i, first[t])
    assert 0.25 < dropped / len(b.reads) < 0.5 and all(0 in st.flags[lo:hi] for lo, hi in zip(b.cuts[1:], b.cuts[2:]))
    _few_blind(st.alive)
    assert not st.flags[5000] and st.flags[5] and len(b.reads) <= 6000


def test_census_of_the_cap_batch():
    b = rb.cap_batch()
    st = pipeline(b.reads, None, b.rev, dict(cuts=b.cuts, max_covg=rb.CAP_COVG, genome_size=rb.CAP_G))[2]
    cut = b.notes["cut"]
    assert [a.index for a in st.alive] == list(range(cut + 1))
    assert b.cuts[1] + 1 < cut < b.cuts[2] - 2  # neither first nor last of the second block
    listed = lambda r: any(c not in rb.HAS_BASE for c in r)  # noqa: E731
    assert listed(b.reads[cut]) and listed(b.reads[cut - 1]) and listed(b.reads[cut + 1])
    assert b.reads[cut][-1:] == b"N" and b.reads[cut + 1][:1] == b"N"  # the last base kept and the first base dropped are listed
    _few_blind(st.alive)


def test_the_tripwire_batch_trips():
    """inside every kept range all qualities are 40 and every cut byte is 2: one cut byte among the qualities the filter sums fails the read"""
    b = rb.tripwire_batch()
    T = read_filter_rule.threshold(30000)
    st = pipeline(b.reads, b.quals, b.rev, dict(rb.TRIPWIRE_TRIM, **rb.TRIPWIRE_FILTER))
    assert len(st[1].alive) == len(b.reads) and max(len(r) for r in b.reads) == 150  # nothing is dropped when the filter sees the kept ranges
    _few_blind(st[1].alive)
    assert st[1].alive[b.notes["unreturnable"]].seq and rb.HAS_BASE.isdisjoint(st[1].alive[b.notes["unreturnable"]].seq)
    assert sum(1 for a, r in zip(st[0].alive, b.reads) if len(a.seq) < len(r)) > 500 and any(len(a.seq) == len(r) > 0 for a, r in zip(st[0].alive, b.reads))
    longest = max(st[0].alive, key=lambda a: len(a.seq))
    assert len(longest.seq) == 130 and set(longest.qual.tolist()) == {40}
    for at in (0, 64, 129):  # one leaked byte in place of a kept one, and one byte more than the range
        q = longest.qual.copy()
        q[at] = 2
        assert read_filter_rule.fate(130, q, 0, 0, T) == read_filter_rule.LOWQ
    assert read_filter_rule.fate(131, np.append(longest.qual, 2), 0, 0, T) == read_filter_rule.LOWQ
    # every read, not the longest alone: a shorter read has fewer good bases to hide the bad one behind
    assert all(read_filter_rule.qual_sum(a.qual) + read_filter_rule.E[2] - read_filter_rule.E[40] > len(a.seq) * T for a in st[0].alive if a.seq)


@pytest.mark.parametrize("kind", rb.VANISH_KINDS)
def test_the_vanishing_block_vanishes(kind):
    b, settings = rb.vanish_batch(kind)
    st = pipeline(b.reads, b.quals, b.rev, dict(settings, cuts=b.cuts, steps=[("dedup", 64)]))
    counts = rb.block_counts(st[2].alive, 3)
    assert counts == ([300, 0, 300] if kind == "filtered away" else [300, 300, 300])
    assert sum(len(a.seq) for a in st[2].alive if a.block == 1) == 0
    where, kept = rb.kept_blocks([a.seq for a in st[2].alive], counts)
    assert kept == 2 and where[0] == (0, 0) and where[-1] == (1, 299)
    assert sum(1 for f, a in zip(st[3].flags, st[2].alive) if not f and a.block == 2) >= 100  # the planted copies, numbered through the gap
    _few_blind(st[2].alive)


def test_census_of_the_composed_batch():
    b = rb.composed_batch()
    s = b.notes["settings"]
    st = pipeline(b.reads, b.quals, b.rev, s)
    n = [len(x.alive) for x in st]
    assert 3900 <= len(b.reads) <= 4100 and max(len(r) for r in b.reads) == 600 and min(len(r) for r in b.reads) == 0
    assert [x.name for x in st] == ["trim", "filter", "cap", "dedup", "dedup", "subsample", "subsample"]
    assert n[0] == len(b.reads) and n[1] < 0.9 * n[0] and n[2] < n[1] and n[3] < 0.95 * n[2] and n[4] == n[3] and n[5] < 0.8 * n[4] and n[6] < 0.6 * n[5]
    assert st[2].alive[-1].block == 2 and b.cuts[2] + 1 < st[2].alive[-1].index < b.cuts[3] - 2  # the cap cuts inside the third block
    assert sum(1 for a, r in zip(st[0].alive, b.reads) if len(a.seq) < len(r)) > 0.9 * n[0]
    # duplicates across blocks and within one
    blocks_of_dropped = {(a.block) for a, f in zip(st[2].alive, st[3].flags) if not f}
    assert blocks_of_dropped == {0, 1, 2}
    # reads the read-back cannot return go through every stage: the counters and the ids have to count past them, to the last step
    for x in st[2:]:
        _few_blind(x.alive)
    assert all(b.reads[i] and rb.HAS_BASE.isdisjoint(b.reads[i]) for i in b.notes["blind"])
    index_of = {a.index: j for j, a in enumerate(st[2].alive)}
    assert st[3].flags[index_of[b.notes["blind"][0]]] == 1 and [st[3].flags[index_of[i]] for i in b.notes["blind_copies"]] == [0, 0]
    assert any(rb.HAS_BASE.isdisjoint(a.seq) and a.seq for a in st[-1].alive[1:-1])
    assert max(sum(len(r) for r in b.reads[lo:hi]) for lo, hi in zip(b.cuts, b.cuts[1:])) < rb.BLOCK_BASES and sum(len(r) for r in b.reads) <= 1_000_000
