"""The batches of tests/wk_range.py, checked on the CPU: at every (w, k) the product's index equals the oracle's, the oracle's sketch equals
the plain rule of tests/minimizer_rule.py on the reads that hold one window more or less, every batch decides something (kept clusters,
both sides of every class populated, read starts on the promised tile offsets), and the parameter gate refuses what lies outside the range.

tests/test_gpu_wk_range.py maps the same batches on the device."""
import numpy as np
import pytest

import edge_reads as E
import minimizer_rule as R
import wk_range as W
from test_index_oracle import _assert_same_index, _product_index
from util import cluster_fraction, map_params

EINVAL = 22  # DependencyError.code of DRPRG_EINVAL (csrc/common.h)


def _kept(oracle, panel, bases, offs, w, k, illumina, mcs):
    md, er = map_params(k, illumina)
    idx = oracle.build_index(panel.prgs, w, k)
    return oracle.map_reads(bases, offs, idx, w, k, md, float(cluster_fraction(er, k)), mcs)[2]


def _same_index(tmp_path, oracle, panel, w, k):
    ctx, _ = _product_index(tmp_path, panel.names, panel.prgs, w, k)
    idx = ctx.export_index()
    _assert_same_index(idx, oracle.build_index(panel.prgs, w, k))
    ctx.close()
    return idx


def _rule_equals_oracle(oracle, read, w, k):
    """the oracle's sketch of one read == the plain rule's; returns the number of minimizers"""
    want = R.sketch(read, w, k)
    h, p, s = oracle.sketch(read, w, k)
    assert list(zip(p.tolist(), h.tolist(), s.tolist())) == want, (w, k, len(read))
    return len(want)


# ---- key width ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,k", W.K_EDGE)
def test_key_width_index_and_census(tmp_path, oracle, w, k):
    panel = W.k_edge_panel()
    idx = _same_index(tmp_path, oracle, panel, w, k)
    assert len(idx["keys"]) > 500
    if k == 16:  # (hash64 is a bijection of the 2k-bit values: a key of 2^32 - 1 needs the all-T 16-mer.  That the keys span the upper half
        # of the 32 bits is what a u32 table would truncate)
        assert int(idx["keys"].max()) >= 1 << 31
    if k > 16:
        assert int(idx["keys"].max()) >= 1 << 32
    bases, offs, census = W.k_edge_reads()
    assert census["short"] == 1200 and census["long"] == 40 and census["cut"] > 100
    assert census["long_lengths"].min() >= 1500 and census["long_lengths"].max() <= 9000
    assert int(offs[-1]) < 330_000
    cnt = _kept(oracle, panel, bases, offs, w, k, True, W.MCS)
    assert cnt["clusters_kept"] > 0, cnt


def test_key_width_even_k_holds_its_own_reverse_complement(oracle):
    """k = 16: the palindrome locus puts a 16-mer that is its own reverse complement into the index and into the reads cut across it"""
    panel = W.k_edge_panel()
    g = panel.refs[panel.names.index("perfect_palindrome")]
    own = [p for p in range(len(g) - 15) if g[p:p + 16].encode() == W.rc(g[p:p + 16].encode())]
    assert own
    keys = set(oracle.build_index(panel.prgs, 1, 16)["keys"].tolist())
    assert R.kmer(g[own[0]:own[0] + 16])[0] in keys
    bases, offs, _ = W.k_edge_reads()
    text = bases.tobytes()
    kmer = g[own[0]:own[0] + 16].encode()
    assert sum(kmer in text[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])) >= 4


# ---- window and halo ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", W.W_EDGE_K)
@pytest.mark.parametrize("w", W.W_EDGE)
def test_window_edge_index_and_census(tmp_path, oracle, w, k):
    panel, seqs = W.w_edge_panel()
    assert sum(len(s) >= 4000 for s in seqs) >= 6
    _same_index(tmp_path, oracle, panel, w, k)
    bases, offs, census = W.w_edge_batch(w, k)
    n_bases, n_reads = int(offs[-1]), len(offs) - 1
    te = 4096 - 2 * max(16, (w - 1 + 15) // 16 * 16)
    assert census["t_eval"] == te
    assert n_bases <= 300_000 and n_reads <= 4000 and (n_bases + te - 1) // te >= 64
    # the read starts land on the promised tile offsets: every d on at least 8 tiles, the first tile (d > 0 there) and the last among them
    starts = set(offs.tolist())
    last = (n_bases - 1) // te
    for d in (-(w - 1), -(k - 1), -1, 0, 1, k - 1, w - 1):
        tiles = [m for m in range(last + 1) if m * te + d in starts and (m * te + d > 0 or (m == 0 and d == 0))]
        assert len(tiles) >= 8 and last in tiles and (0 in tiles or d < 0), (w, k, d, tiles)
    assert sorted(census["starts"]) == sorted((m, d) for m in W.EDGE_TILES for d in W.offsets_of(w, k) if m * te + d > 0 or (m, d) == (0, 0))
    # the boundary reads against the plain rule: one window short holds no minimizer, one window at least one -- or whatever the rule says
    read = lambda i: bases[int(offs[i]):int(offs[i + 1])].tobytes()
    for name, length in (("short", w + k - 2), ("one", w + k - 1), ("two", w + k)):
        assert len(census[name]) >= 6
        for i in census[name]:
            r = read(i)
            assert len(r) == length
            n = _rule_equals_oracle(oracle, r, w, k)
            assert (n == 0) if name == "short" else (n >= 1), (w, k, name, n)
    # the N-split reads: a run of w - 1 k-mers holds no minimizer, a run of w at least one; the oracle's sketch is the rule's
    assert len(census["n_split"]) >= 12
    for i, left, right in census["n_split"]:
        r = read(i)
        assert r[left:left + 1] == b"N" and r.count(b"N") == 1 and len(r) == left + 1 + right
        _rule_equals_oracle(oracle, r, w, k)
        pos = [p for p, _, _ in R.sketch(r, w, k)]
        for lo, hi, run in ((0, left, left), (left + 1, len(r), right)):
            inside = [p for p in pos if lo <= p < hi]
            assert (not inside) if run - k + 1 < w else inside, (w, k, left, right)
    # reads with fewer than w k-mers are most of a short-read batch from w = 137 on (k = 15): 150-base reads of the loci are in the batch
    lengths = np.diff(offs.astype(np.int64))
    assert (lengths == 150).sum() >= 50 and census["long"] >= 3 and lengths.max() <= 9000
    cnt = _kept(oracle, panel, bases, offs, w, k, W.w_illumina(w), W.W_MCS)
    assert cnt["clusters_kept"] > 0 and cnt["minimizers"] > 50, cnt


# ---- the length-governed threshold at the reciprocal's limit --------------------------------------------------------------------------
@pytest.mark.parametrize("w", W.SIZE_LEN_W)
def test_size_len_classes_at_the_reciprocal_limit(tmp_path, oracle, w):
    cls = W.size_len_class(oracle, w)
    panel = E.panel_of(oracle, cls.panel)[0]
    _same_index(tmp_path, oracle, panel, w, E.K)
    assert (cls.w, cls.illumina, cls.mcs, cls.rule) == (w, False, 1, "size_len")
    tr = E.Tracer(oracle, cls.panel, w, False, cls.mcs)
    thresholds = set()
    for side, reads in (("on", cls.on), ("off", cls.off)):
        assert len(reads) >= E.FLOOR, (w, side, len(reads), cls.proposed)
        for r in reads:
            t = tr(r)
            assert E.is_size(t, tr, side, "len"), (w, side)
            thresholds.add(int(E._largest(t)["thr"]))
    assert len(thresholds) >= 2 and min(thresholds) > cls.mcs  # (the length term, at more than one of its values)
    # some reads are of the first length at which floor(fraction * 2 len / (w + 1)) takes its value, some one base short of it
    steps = E._step_lengths(tr, w, 1500, 6000)
    lengths = [len(r) for r in cls.reads()]
    assert sum(n in steps[1::2] for n in lengths) >= 8 and sum(n in steps[0::2] for n in lengths) >= 8, (w, steps)
    # it decides.  thr = floor(m * fraction) is 2 .. 5 here: half the fraction takes at least one hit off it (and leaves it above
    # min_cluster_size 1 or at it), twice the fraction adds at least two
    assert tr.kept(cls.on) == 0 and E.Tracer(oracle, cls.panel, w, False, cls.mcs, fraction=tr.frac / 2).kept(cls.on) >= len(cls.on)
    assert tr.kept(cls.off) == len(cls.off) and E.Tracer(oracle, cls.panel, w, False, cls.mcs, fraction=tr.frac * 2).kept(cls.off) == 0
    assert int((np.diff(E.batch(cls.reads())[1].astype(np.int64))).max()) < 6000


# ---- tiny k ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,k", W.K_TINY)
def test_tiny_k_index_and_census(tmp_path, oracle, w, k):
    panel, seqs = W.tiny_panel()
    assert [len(s) for s in seqs] == [len(seqs[0])] * 2 + [300, 300] and abs(len(seqs[0]) - 300) < 40
    _same_index(tmp_path, oracle, panel, w, k)
    reads = W.tiny_reads(w, k)
    assert len(reads) == 600 and all(len(r) == 150 for r in reads)
    hits = W.tiny_census(oracle, w, k)
    assert (hits > 1024).sum() >= 1 and ((hits >= 64) & (hits <= 1024)).sum() >= 1, (w, k, np.sort(hits)[::60])
    bases, offs = W.batch(reads)
    cnt = _kept(oracle, panel, bases, offs, w, k, True, W.MCS)
    assert cnt["clusters_kept"] > 0 and cnt["hits"] == int(hits.sum())
    for r in reads[:40]:
        _rule_equals_oracle(oracle, r, w, k)


# ---- the parameter gate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,k", [(1025, 15), (11, 32), (11, 0), (0, 15)])
def test_parameters_outside_the_range_are_refused(tmp_path, w, k):
    """a host-only context, and the index builder, refuse what Mapper::set_params refuses, with the same code"""
    from drprg_amd import DependencyError
    from drprg_amd._lib import lib
    with pytest.raises(DependencyError) as err:
        _product_index(tmp_path, ["a"], ["ACGTACGTTTGACCAGTAGGACCATTAGACCAGATTACAGGATC"], w, k)
    assert err.value.code == EINVAL and "must be in [1," in str(err.value)
    assert lib.drprg_hip_index(str(tmp_path / "dr.prg").encode(), w, k, 1) == -EINVAL


@pytest.mark.parametrize("w,k", [(1024, 31), (1, 1), (1024, 1), (1, 31)])
def test_the_corners_of_the_range_are_served(tmp_path, oracle, w, k):
    panel = W.w_edge_panel()[0]
    _same_index(tmp_path, oracle, panel, w, k)
