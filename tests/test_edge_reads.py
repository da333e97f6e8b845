"""The edge reads of tests/edge_reads.py, checked on the CPU: the census (every class reaches its floor, every accepted read's trace shows
what its class claims), each class decides something (the oracle under the neighbouring rule value keeps other clusters), and the
device's 2 len / (w + 1) equals the plain division wherever the device uses it.

Wall time of this file: 25 s next to 110 s for the non-GPU suite of the parent commit (same machine, one process): a little under the
quarter it may add.  The sweep classes are most of it (eight classes of ~1 400 reads, a bisection of ten traces per length).

strand_tie, containment, equal_first and early_drop are built with the Illumina parameters only: the overlap sweep and the early drop compare
positions and sizes of clusters that exist, neither max_diff nor the fraction enters them."""
import numpy as np
import pytest

import edge_reads as E


@pytest.fixture(scope="module")
def classes(oracle):
    return E.build(oracle)


def _tracer(oracle, cls, **kw):
    return E.Tracer(oracle, cls.panel, cls.w, cls.illumina, cls.mcs, **kw)


EXPECTED = ([f"{r}_{t}" for t in ("illumina", "nanopore") for r in ("gap", "size_mcs", "size_path", "size_len")]
            + [f"sweep_w{w}_{t}" for t in ("illumina", "nanopore") for w in E.SWEEP_W]
            + ["strand_tie", "containment", "equal_first", "early_drop_mcs1", "early_drop_mcs2", "early_drop_mcs10"])
# the sides a class cannot have: two PRGs with the same first position have no "one past"; a read with ONE hit has one group, so with
# min_cluster_size 1 the early drop has its far side only
ONE_SIDED = {"equal_first": "on", "early_drop_mcs1": "off"}


def test_census(oracle, classes):
    """no class missing, every side at its floor, both strands in it, and every accepted read -- traced again here -- shows its property"""
    assert sorted(classes) == sorted(EXPECTED)
    for name, cls in classes.items():
        tr = _tracer(oracle, cls)
        for side, reads in (("on", cls.on), ("off", cls.off)):
            if ONE_SIDED.get(name, side) != side:
                assert not reads, (name, side)
                continue
            if cls.rule != "sweep":
                assert len(reads) >= E.FLOOR, (name, side, len(reads), cls.proposed)
            fwd = 0
            for r in reads:
                t = tr(r)
                assert E.holds(cls, tr, t, side), (name, side, r)
                fwd += int(t["hits"]["fwd"].sum() * 2 >= len(t["hits"]))
            assert 0 < fwd < len(reads) or cls.rule in ("strand_tie",), (name, side, "one strand only")
        if cls.rule == "sweep":
            short = {n: c for n, c in cls.lengths.items() if c < 2}
            assert not short, (name, short)
            assert set(cls.lengths) == set(range(E.K, E.SWEEP_MAX + 1)) | set(E.SWEEP_LONG)
            assert len({len(r) for r in cls.reads()}) == len(cls.lengths) and len(cls.on) >= E.FLOOR and len(cls.off) >= E.FLOOR
            # past the shortest reads the length term sets the threshold and both sides exist at (nearly) every length
            both = {len(r) for r in cls.on} & {len(r) for r in cls.off}
            assert len(both) >= 0.9 * len(cls.lengths), (name, len(both))
    tie = classes["strand_tie"]
    tr = _tracer(oracle, tie)
    later = sum(E.is_strand_tie_later(tr(r)) for r in tie.off)
    assert later >= E.FLOOR and len(tie.off) - later >= E.FLOOR, "sizes one apart: each way round"


def test_each_class_decides_something(oracle, classes):
    """the oracle under the neighbouring value of the rule keeps other clusters of the class than under the rule itself"""
    for name, cls in classes.items():
        tr = _tracer(oracle, cls)
        if cls.rule == "gap":
            assert tr.kept(cls.on) == len(cls.on) and _tracer(oracle, cls, max_diff=tr.md - 1).kept(cls.on) == 0, name
            assert tr.kept(cls.off) == 0 and _tracer(oracle, cls, max_diff=tr.md + 1).kept(cls.off) == len(cls.off), name
        elif cls.rule == "size_mcs":
            lower, higher = (E.Tracer(oracle, cls.panel, cls.w, cls.illumina, cls.mcs + d) for d in (-1, 1))
            assert tr.kept(cls.on) == 0 and lower.kept(cls.on) == len(cls.on), name
            assert tr.kept(cls.off) == len(cls.off) and higher.kept(cls.off) == 0, name
        elif cls.rule in ("size_path", "size_len"):
            # thr = floor(m * fraction) >= 11 here (it exceeds min_cluster_size 10): a tenth less of the fraction takes at least one hit off
            # it, a tenth more adds at least one
            assert tr.kept(cls.on) == 0 and _tracer(oracle, cls, fraction=tr.frac * 0.9).kept(cls.on) == len(cls.on), name
            assert tr.kept(cls.off) == len(cls.off) and _tracer(oracle, cls, fraction=tr.frac * 1.1).kept(cls.off) == 0, name
        elif cls.rule == "sweep":
            assert tr.kept(cls.on) == 0 and tr.kept(cls.off) >= len(cls.off), name
        elif cls.rule == "strand_tie":
            assert tr.kept(cls.on) == len(cls.on) and tr.kept(cls.off) == len(cls.off)  # one of the two, always: WHICH one is the rule
            assert not any(E.is_strand_tie_later(tr(r)) for r in cls.on) and any(E.is_strand_tie_later(tr(r)) for r in cls.off)
        elif cls.rule == "containment":
            assert tr.kept(cls.on) == len(cls.on) and tr.kept(cls.off) == 2 * len(cls.off), name
        elif cls.rule == "equal_first":
            assert tr.kept(cls.on) == len(cls.on), name
        else:
            # the early drop is a shortcut of the device, not a rule: no cluster of such a read passes on either side of it, so on the device
            # the class is a parity check of the shortcut's bookkeeping (handled marks, leftover count, the wave path it hands the far side to),
            # not of its comparison: a `<` for the `<=` there would only send the on side through the wave path, to the same result
            assert cls.rule == "early_drop" and tr.kept(cls.reads()) == 0, name


def test_device_reciprocal_is_the_division():
    """device_common.h expected_minimizers: below len = 2^23 and w = 200 the device computes 2 len / (w + 1) as
    umulhi(2 len, 2^32 / (w + 1) + 1); the oracle divides.  Both are step functions of 2 len, so they are compared at every multiple of
    w + 1 and the value just below it, for every 2 len < 2^24 and w in 1 .. 199.  (What the sweep classes then show on the device can only
    fail through a kernel, not through the formula -- and this fails the day someone widens the range the formula is used for.)"""
    import pathlib
    import re
    src = re.sub(r"\s+", "", (pathlib.Path(__file__).resolve().parent.parent / "drprg_amd" / "csrc" / "device_common.h").read_text())
    # what is restated below: the magic number, the range it is used in, the product (white space aside)
    assert "0x100000000ull/(uint32_t)(w+1))+1u" in src and "w<200&&len<(1ull<<23)" in src and "__umulhi((uint32_t)len*2u,magic)" in src
    for w in range(1, 200):
        d = np.uint64(w + 1)
        magic = np.uint64((1 << 32) // (w + 1) + 1)
        x = np.arange(1, ((1 << 24) - 1) // (w + 1) + 1, dtype=np.uint64) * d
        for v in (x, x - np.uint64(1)):
            assert np.array_equal((v * magic) >> np.uint64(32), v // d), w
    # From w = 200 on the device divides: `return len * 2 / (uint64_t)(w + 1)` -- the oracle's own expression.  What is restated here is why the
    # switch must stay where it is: past it the product x * M no longer has its quotient in the high word for every 2 len < 2^24
    # (x * (d * M - 2^32) < 2^32 fails), so a wider `w <` would be wrong at some w in 200 .. 1024 and some length the hit key takes.
    assert "returnlen*2/(uint64_t)(w+1);" in src and src.count("w<200&&") == 1
    wrong = 0
    for w in range(200, 1025):
        d = np.uint64(w + 1)
        magic = np.uint64((1 << 32) // (w + 1) + 1)
        x = np.arange(1, ((1 << 24) - 1) // (w + 1) + 1, dtype=np.uint64) * d
        for v in (x, x - np.uint64(1)):
            wrong += int(((v * magic) >> np.uint64(32) != v // d).any())
    assert wrong > 0, "the reciprocal would serve every w: the device's w < 200 could go"
