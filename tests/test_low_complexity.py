"""The census of tests/low_complexity.py on the CPU: at every (w, k) the device maps (tests/test_gpu_low_complexity.py), every class of
tie that can exist there holds at least FLOOR accepted reads, each with a kept cluster in the oracle's trace that holds one of the class's
own hits, and each told from the rule by the mutant the class is there to catch.  Conditions, not measurements: a change to the panel or to
the recipe that loses a class fails here, before a GPU is asked."""
import pytest

import low_complexity as L
import minimizer_rule as R


def test_panel_holds_what_it_says(oracle):
    panel, spans = L.lc_panel()
    assert 10 <= len(panel.names) <= 14 and all(300 <= len(r) <= 1500 for r in panel.refs)
    assert sum(" 5 " in p for p in panel.prgs) >= 4  # (sites inside repeats)
    tr = L.Tracer(oracle, 11, 15)
    assert tr.doubles, "no key with two records of one PRG and strand: the direct repeat is gone"


@pytest.mark.parametrize("w,k", L.WK)
def test_census(oracle, w, k):
    classes, left, right, seen = L.census(oracle, w, k)
    line = L.census_line(oracle, w, k)
    assert sorted(classes) == sorted(L.applicable(w, k)), line
    for name, accepted in classes.items():
        assert len(accepted) >= L.FLOOR, (name, line)
        if name in L.TIE_CLASSES:
            assert left[name] >= L.FLOOR and right[name] >= L.FLOOR, (name, line)
    # the accepted reads, traced and classified again: the class, a kept cluster on one of its positions, the mutant
    tr = L.Tracer(oracle, w, k)
    reads = L.reads(w, k)
    for name, accepted in classes.items():
        for i in accepted[:L.FLOOR]:
            found, sets = L.classify(reads[i], w, k, tr)
            t = tr(reads[i])
            kept = set()
            for c in t["clusters"]:
                if c["alive"]:
                    kept.update(t["hits"]["pos"][c["first"]:c["first"] + c["n"]].tolist())
            assert found[name] & kept, (name, i, line)
            assert t["keyed"] == len(sets["rule"]), (name, i)  # (the trace's keyed minimizers are the plain rule's)
            if name in L.TIE_CLASSES:
                assert sets["leftmost"] != sets["rule"] or sets["rightmost"] != sets["rule"], (name, i, line)
            elif name == "selfcomp":
                assert sets["strict"] != sets["rule"], (name, i, line)


def test_reads_are_what_the_recipe_promises():
    reads = L.reads(11, 15)
    lens = [len(r) for r in reads]
    assert 2000 <= len(reads) <= 8000 and min(lens) >= 60 and 700 in lens and 3000 in lens
    assert sum(r != r.upper() for r in reads) > 100                      # lower case
    assert sum(any(c not in b"ACGTacgt" for c in r) for r in reads) > 300  # an N (or another letter that is no base) at the offsets of the repeats
    assert reads == L.reads(11, 15)
    assert R.sketch("ACGTN", 1, 4) == [(0,) + R.kmer("ACGT")]
