"""The census of tests/batch_sequences.py on the CPU: the schedule covers what it promises and, by the oracle's own counters, each kind
of batch is what its name says.  Conditions, not measurements: a change to a recipe that loses a pair of states, an entry point behind a
kind, or the property a kind is there for fails here, before a GPU is asked (tests/test_gpu_batch_sequences.py maps the schedule)."""
import numpy as np
import pytest

import batch_sequences as B

# every (w, k, illumina) the device tests map the schedule with
WKI = [(11, 15, True), (11, 15, False), (11, 14, True), (12, 15, True), (19, 21, True)]


def test_schedule_covers_every_ordered_pair_of_states():
    steps = B.schedule()
    cov = B.coverage_of(steps)
    n = len(B.STATES)
    print(f"schedule: {len(steps)} batches, {cov['resets']} resets; pairs adjacent {len(cov['pairs1'])}/{n * n}, two apart {len(cov['pairs2'])}/{n * n}; "
          f"(kind, next entry point) {len(cov['entry_after'])}/{len(B.KINDS) * 6}; kinds with a reset behind them {len(cov['reset_after'])}/{len(B.KINDS)}")
    assert n == 20 and n * n + 1 <= len(steps) <= B.MAX_STEPS  # (a batch closes at most one pair of each distance)
    every = {(a, b) for a in B.STATES for b in B.STATES}
    assert cov["pairs1"] == every, sorted(every - cov["pairs1"])[:5]
    assert cov["pairs2"] == every, sorted(every - cov["pairs2"])[:5]
    assert steps == B._build(B.SEED + min(range(8), key=lambda i: len(B._build(B.SEED + i))))  # seeded: the same on every machine
    # the pairs again, the plain way: no reset between the two batches
    for d, name in ((1, "pairs1"), (2, "pairs2")):
        seen = {((steps[i - d].kind, steps[i - d].packed), (steps[i].kind, steps[i].packed)) for i in range(d, len(steps))
                if not any(steps[j].reset_before for j in range(i - d + 1, i + 1))}
        assert seen == cov[name]


def test_every_entry_point_and_a_reset_follow_every_kind():
    steps = B.schedule()
    cov = B.coverage_of(steps)
    entries = [e for es in B.ENTRIES.values() for e in es]
    assert len(entries) == 6
    for kind in B.KINDS:
        for e in entries:
            assert (kind, e) in cov["entry_after"], (kind, e)
        assert kind in cov["reset_after"], kind
    assert len(B.KINDS) <= cov["resets"] <= 3 * len(B.KINDS) and not steps[0].reset_before
    for st in steps:
        assert st.entry in B.ENTRIES[st.packed]


def test_kinds_are_small_and_seeded():
    for kind in B.KINDS:
        bases, offs = B.kind_batch(kind)
        lens = np.diff(offs.astype(np.int64))
        assert bases.size == int(offs[-1]) < 1 << 20 and offs[0] == 0
        assert len(lens) <= 3000 and (lens.max(initial=0) <= 2000 or len(lens) <= 200), kind
        B._CACHE.pop(("kind", kind))
        again = B.kind_batch(kind)
        assert np.array_equal(again[0], bases) and np.array_equal(again[1], offs), kind
    assert len(B.kind_batch("none")[1]) == 1
    assert len(B.kind_batch("empties")[1]) == 6 and int(B.kind_batch("empties")[1][-1]) == 0
    assert len(B.kind_batch("tiny")[1]) == 11
    lens = np.diff(B.kind_batch("ragged")[1].astype(np.int64))
    assert (lens == 0).sum() >= 50 and ((lens > 0) & (lens < 14)).sum() >= 30  # empty reads, reads shorter than every k mapped
    rb = B.kind_batch("ragged")[0]
    assert (rb >= ord("a")).sum() > 10000  # lower case
    assert np.array_equal(B.kind_batch("ragged")[1], B.kind_batch("ragged_clean")[1])


def test_packed_forms_hold_their_n_positions():
    """kind 8 lists N positions in its packed form, kind 9 -- the same reads with a base in each of those places -- lists none: mapped
    behind kind 8 it is right only if nothing of kind 8's positions survives"""
    words, npos = B.kind_packed("ragged")
    bases = B.kind_batch("ragged")[0]
    print(f"ragged: {npos.size} N positions in {bases.size} bases")
    assert npos.size >= 100 and np.array_equal(npos, np.nonzero(~B._IS_BASE[bases])[0].astype(np.uint64))
    runs = np.split(npos, np.nonzero(np.diff(npos.astype(np.int64)) != 1)[0] + 1)
    assert max(len(r) for r in runs) >= 17 and sum(len(r) == 1 for r in runs) >= 50  # runs longer than a k-mer or a packed word, single Ns
    cwords, cnpos = B.kind_packed("ragged_clean")
    assert cnpos.size == 0 and cwords.size == words.size
    # one more kind lists positions -- fewer, elsewhere, in a shorter batch: a mark of the ragged kind that outlives its batch falls on a base
    # of this one (and the other way round); a batch behind ITSELF would set the same bits again and show nothing
    mnpos = B.kind_packed("medium")[1]
    print(f"medium: {mnpos.size} N positions in {B.kind_batch('medium')[0].size} bases")
    assert 100 <= mnpos.size < npos.size and B.kind_batch("medium")[0].size < bases.size
    stale = np.setdiff1d(npos[npos < B.kind_batch("medium")[0].size], mnpos)
    assert stale.size >= 1000 and np.setdiff1d(mnpos, npos).size >= 100
    for kind in B.KINDS:
        if kind not in ("ragged", "medium"):
            assert B.kind_packed(kind)[1].size == 0, kind


def test_mean_lengths_fall_in_three_look_ahead_classes():
    mean = {}
    for kind in B.KINDS:
        offs = B.kind_batch(kind)[1]
        n = len(offs) - 1
        mean[kind] = int(offs[-1]) // n if n else 0  # (launch_read_cluster's own division)
    print("mean read lengths:", mean, "-> look-ahead", {k: B.look_ahead(v) for k, v in mean.items()})
    assert (B.look_ahead(mean["dense"]), B.look_ahead(mean["medium"]), B.look_ahead(mean["long"])) == (128, 256, 512)
    assert 300 < mean["medium"] <= 600
    lens = np.diff(B.kind_batch("long")[1].astype(np.int64))
    assert lens.min() >= 3000 and lens.max() <= 9000 and lens.max() > 512  # (READ_SORT_MAX_LEN: the leftovers take the radix sort)
    assert np.diff(B.kind_batch("dense")[1].astype(np.int64)).max() <= 512  # (... and those of the short kinds the per-read sort)


@pytest.mark.parametrize("w,k,illumina", WKI)
def test_kinds_are_what_their_names_say(oracle, w, k, illumina):
    per = B.oracle_of_kinds(oracle, w, k, illumina)
    for kind in B.KINDS:
        offs = B.kind_batch(kind)[1]
        cnt = per[kind][2]
        print(f"w={w} k={k} illumina={illumina} {kind}: reads {len(offs) - 1} bases {int(offs[-1])} " + " ".join(f"{key} {cnt[key]}" for key in B.COUNTERS[2:]))
        assert cnt["reads"] == len(offs) - 1 and cnt["bases"] == int(offs[-1])
    n_bases = lambda kind: int(B.kind_batch(kind)[1][-1])
    # dense outgrows the first capacity of every sequence: n_bases / 48 (filtered), / 16 (direct candidates), / 64 (generic hit buffer)
    assert per["dense"][2]["hits"] > n_bases("dense") // 16 and per["dense"][2]["clusters_kept"] > 2000
    # sparse: mostly off-panel
    assert 0 < per["sparse"][2]["clusters_kept"] < (len(B.kind_batch("sparse")[1]) - 1) // 5
    assert per["sparse"][2]["hits"] < n_bases("sparse") // 48
    for kind in ("none", "empties"):
        assert not per[kind][0].any() and not per[kind][1].any() and per[kind][2]["minimizers"] == 0
    assert per["tiny"][2]["clusters_kept"] >= 5
    for kind in ("repeat", "long", "medium", "ragged", "ragged_clean"):
        assert per[kind][2]["clusters_kept"] >= 200, kind
    # the N positions change the result: what kind 8 leaves behind would show in kind 9
    assert not np.array_equal(per["ragged"][0], per["ragged_clean"][0])
    assert per["ragged"][2]["minimizers"] < per["ragged_clean"][2]["minimizers"]
    assert per["ragged"][2]["hits"] != per["ragged_clean"][2]["hits"]
    # ... and every kind but the two without bases has a vector of its own (a sum that took the wrong kind's share would differ)
    vecs = [per[kind][0].tobytes() for kind in B.KINDS if kind not in ("none", "empties")]
    assert len(set(vecs)) == len(vecs)


def _traces(oracle, kind, w, k, illumina, limit=None):
    from util import cluster_fraction, map_params
    idx = B._CACHE.get(("index", w, k)) or oracle.build_index(B.panel()[0].prgs, w, k)
    md, er = map_params(k, illumina)
    bases, offs = B.kind_batch(kind)
    n = len(offs) - 1 if limit is None else min(limit, len(offs) - 1)
    return [oracle.read_clusters(bases[int(offs[i]):int(offs[i + 1])], idx, w, k, md, cluster_fraction(er, k), 10) for i in range(n)]


def test_repeat_and_long_reads_do_not_fit_the_per_read_kernel(oracle):
    """by the oracle's trace at (11, 15): reads of the 70-copy locus cut more than 64 runs (the lanes of read_cluster_kernel's wave path) in
    several (PRG, strand) groups; long reads hold more hits than a chunk stages (RC_HCAP = 3072)"""
    tr = _traces(oracle, "repeat", 11, 15, True)
    many = sum(len(t["runs"]) > 64 for t in tr)
    groups = sum(len({(int(p), int(f)) for p, f in zip(t["hits"]["prg"], t["hits"]["fwd"])}) > 1 for t in tr)
    print(f"repeat: {many} of {len(tr)} reads with more than 64 runs, {groups} with hits in several groups")
    assert many >= 300 and groups >= 300
    tr = _traces(oracle, "long", 11, 15, True)
    staged = sum(len(t["hits"]) > 3072 for t in tr)
    print(f"long: {staged} of {len(tr)} reads with more than 3072 hits, the most {max(len(t['hits']) for t in tr)}")
    assert staged >= 30
    tr = _traces(oracle, "dense", 11, 15, True, limit=300)
    assert all(len(t["runs"]) <= 8 and len(t["hits"]) <= 64 for t in tr)  # ordinary short reads: nothing the per-read kernel leaves over
