"""The panels and batches of tests/filter_tiers.py, checked on the CPU: every panel has exactly the records that put it on its side of its
step, the restated size rules give the expected arrays there, the restated arrays reject no index k-mer at any alignment of the kernel's
groups of four in either orientation and none of the batch's hits, their fill is what PrgIndex::filter_selfcheck reports for the product's own
arrays, and every index record is hit at all four alignments in both orientations.  The census says how many hits each wrong shift would
lose: what a device that took a block or a word with one bit less, or tested three bits where one was entered, must lose too.  Everything is
printed (pytest -s)."""
import os
import re

import numpy as np
import pytest

import filter_tiers as F
from util import ROOT

# name: what the two sides of the step must be (tier, then the size that steps)
EXPECT = {f"words{8 + j}_k13": (("levels12", 8 + j), ("levels12", 9 + j)) for j in range(6)}
EXPECT["words13_k11"] = (("levels12", 13), ("levels12", 14))
EXPECT["none_k13"] = EXPECT["none_k11"] = (("levels12", 14), (None, None))
EXPECT.update({f"blkc{cw}": (("level0", cw), ("level0", cw + 1)) for cw in range(10, 16)})
EXPECT["level0"] = (("level0", 16), ("middle", 15))      # (blkc_wbits | midc_wbits)
EXPECT.update({"midc15": (("middle", 15), ("middle", 16)), "midc16": (("middle", 16), ("middle", 17)), "midc17": (("middle", 17), ("middle", 17))})
EXPECT["direct"] = (("middle", 17), (None, None))
EXPECT["mid0"] = (("middle", 3), ("middle", 1))          # (mid0_bits)
RECORDS = {"words13_k11": 5120, "none_k13": 24_576, "none_k11": 24_576, "level0": 21_845, "midc15": 32_768, "midc16": 65_536, "midc17": 131_072,
           "direct": 180_000}
RECORDS.update({f"words{8 + j}_k13": 160 << j for j in range(6)})
RECORDS.update({f"blkc{cw}": 1 << (cw - 1) for cw in range(10, 16)})


def _stepping_size(t, name):
    if t.tier is None:
        return None
    if name == "mid0":
        return t.mid0_bits
    return {"levels12": lambda: t.wbits, "level0": lambda: t.blkc_wbits, "middle": lambda: t.midc_wbits}[t.tier]()


def _host_context(tmp_path, monkeypatch, panel, w, k, mid_max):
    from test_index_oracle import _product_index
    monkeypatch.setenv("DRPRG_MID_MAX_RECORDS", str(mid_max))
    return _product_index(tmp_path, panel.names, panel.prgs, w, k, threads=8)[0]


def _check_case(tmp_path, monkeypatch, oracle, case, threshold):
    """everything that holds for one panel and its batch; returns (tables, census, fewest hits of a record)"""
    panel, w, k, n_records, mid_max = F.panel_of(oracle, case)
    assert max(len(r) for r in panel.refs) < 10_000
    t = F.tables_of(oracle, case)
    assert t.n_records == n_records
    assert (t.tier,) + t.array_bytes() == F.tier_sizes(n_records, k, mid_max)
    # ---- the product's side: the same records, the same fill of every array it reports, and its own check finds nothing -----------------
    ctx = _host_context(tmp_path, monkeypatch, panel, w, k, mid_max)
    assert ctx.n_records == n_records, (case, ctx.n_records)
    sc = ctx.filter_selfcheck()
    ctx.close()
    assert sc["codes"] == (2 * n_records if t.tier else 0), (case, sc)
    assert (sc["level0_fill_permille"], sc["level12_fill_permille"], sc["stage2_fill_permille"]) == t.selfcheck_fills(), (case, sc, t.selfcheck_fills())
    assert sc["level0_false_negatives"] == sc["level12_false_negatives"] == sc["stage2_false_negatives"] == sc["shared_array_false_negatives"] == 0
    # ---- no false negative: every index code, at every alignment, through every second stage the tier has -------------------------------
    for stage2 in F.forms_of(t.tier) if t.tier else ():
        assert t.index_rejected(stage2) == 0, (case, stage2)
    # ---- the batch -----------------------------------------------------------------------------------------------------------------------
    bases, offs, starts = F.batch_of(oracle, case)
    lengths = np.diff(offs.astype(np.int64))
    assert [s % 4 for s in starts] == [0, 1, 2, 3] and starts[0] == 0
    size = min(b - a for a, b in zip(starts, starts[1:])) - 3   # (a filler of at most three bases lies between two sections)
    first = bases[starts[0]:starts[0] + size]
    for s in starts[1:]:
        assert np.array_equal(bases[s:s + size], first)
    assert lengths.max() <= F.READ_MAX and (lengths == 150).sum() >= F.N_BACKGROUND
    assert (lengths == 0).sum() >= 3 and ((lengths > 0) & (lengths < k)).sum() >= 3
    background = np.nonzero(lengths == 150)[0][-F.N_BACKGROUND:]
    text = bases.tobytes()
    assert all(b"N" in text[int(offs[i]):int(offs[i + 1])] for i in background[::10])
    assert int(offs[-1]) < (2_000_000 if threshold and not case.startswith("mid0") else 4_100_000)
    c = F.census(oracle, case)
    h = F.batch_hits(oracle, case)
    assert np.isin(h["code"], t.codes).all()   # every hit of the oracle stands on an index code, as the kernel packs it
    fewest = int(h["per_record"].min())
    assert all(c[key] == 0 for key in c if key in ("lost", "lost_lds", "lost_l2")), (case, c)
    return t, c, fewest


@pytest.mark.parametrize("name", list(EXPECT))
def test_threshold_pair(tmp_path, monkeypatch, oracle, name):
    trees, counts = [], []
    for side, (tier, size) in zip(F.SIDES, EXPECT[name]):
        case = f"{name}-{side}"
        panel, w, k, n_records, _ = F.panel_of(oracle, case)
        assert w == 1 and all(" " not in p for p in panel.prgs)
        if name in RECORDS:
            assert n_records == RECORDS[name] + F.SIDES.index(side), (case, n_records)
        t, c, fewest = _check_case(tmp_path, monkeypatch, oracle, case, True)
        assert (t.tier, _stepping_size(t, name)) == (tier, size), (case, t.tier, _stepping_size(t, name))
        if name == "mid0":
            assert t.distinct_12mers == F.MID0_DISTINCT + F.SIDES.index(side) and t.midc_wbits == F.MID_C_MAX_WBITS
        elif t.tier == "middle":
            assert t.mid0_bits == 3
        # every record is hit at the four alignments in both orientations
        assert fewest >= 8, (case, fewest)
        print(f"{case} (k={k}): {n_records} records, {F.THRESHOLDS[name][2] if name in F.THRESHOLDS else 'middle tier: three bits -> one'}; "
              f"tier {t.tier}, size {_stepping_size(t, name)}, fill {t.selfcheck_fills()}; {len(F.batch_of(oracle, case)[1]) - 1} reads, "
              f"{int(F.batch_of(oracle, case)[1][-1])} bases, fewest hits of a record {fewest}: {c}")
        # every wrong shift and the wrong test lose hits of this batch: a device that had one could not pass the case
        for key in ("lost_word_shift", "lost_block_shift", "lost_three_bit_test"):
            if key in c:
                assert c[key] > 0, (case, key, c)
        if t.tier == "level0":
            assert c["lost_without_offset3"] > 0, (case, c)
        trees.append(panel.prgs)
        counts.append(n_records)
        F.forget(case)
    # the two panels differ in the last base of the last locus alone
    assert counts[1] == counts[0] + 1
    assert trees[0][:-1] == trees[1][:-1] and trees[1][-1][:-1] == trees[0][-1]


@pytest.mark.parametrize("case", list(F.SITES))
def test_panel_with_sites(tmp_path, monkeypatch, oracle, case):
    w, k, edge, aim = F.SITES[case]
    panel, _, _, n_records, _ = F.panel_of(oracle, case)
    assert sum("5" in p for p in panel.prgs) == len(panel.prgs) - 1 and " " not in panel.prgs[-1]
    if aim < edge:
        assert 0.99 * edge <= n_records <= edge
    else:
        assert edge < n_records <= 1.01 * edge
    t, c, fewest = _check_case(tmp_path, monkeypatch, oracle, case, False)
    assert t.tier == F.tier_of(aim, k) == {"sites_below_level0": "level0", "sites_above_level0": "middle", "sites_below_none_k13": "levels12"}[case]
    if t.tier == "levels12":
        assert t.wbits == F.MAX_WBITS       # 64 KB of LDS
    elif t.tier == "level0":
        assert t.wbits == F.MAX_WBITS - 1 and t.blkc_wbits == 16
    print(f"{case} (w={w}, k={k}): {n_records} records in {len(panel.prgs)} loci; tier {t.tier}, fill {t.selfcheck_fills()}; "
          f"{len(F.batch_of(oracle, case)[1]) - 1} reads, {int(F.batch_of(oracle, case)[1][-1])} bases, fewest hits of a record {fewest}: {c}")
    assert c["hits"] > 100_000
    F.forget(case)


def test_every_row_of_the_table_has_both_sides():
    assert sorted(F.all_cases()) == sorted([f"{n}-{s}" for n in EXPECT for s in F.SIDES] + list(F.SITES))
    assert {F.THRESHOLDS[n][:2] for n in F.THRESHOLDS} == {(13 if "k13" in n else 11 if "k11" in n else 15, RECORDS[n]) for n in RECORDS}


def _source(name):
    return open(os.path.join(ROOT, "drprg_amd", "csrc", name)).read()


def test_the_constants_of_the_restatement_are_the_sources():
    common, index_cpp, switches, filt = (_source(n) for n in ("common.h", "index.cpp", "switches.h", "sketch_filter.hip"))
    for name in ("BLOOM_C0", "BLOOM_C1", "BLOOM_C2", "BLOOM_CR"):
        assert int(re.search(rf"constexpr uint32_t {name} = (0x[0-9A-Fa-f]+)u;", common).group(1), 16) == getattr(F, name)
    assert int(re.search(r"constexpr uint32_t MAX_WBITS = (\d+);", index_cpp).group(1)) == F.MAX_WBITS
    assert int(re.search(r"constexpr uint32_t L0_WBITS = (\d+);", index_cpp).group(1)) == F.L0_WBITS
    assert int(re.search(r"constexpr uint32_t BLOOMR_WBITS = (\d+);", common).group(1)) == F.BLOOMR_WBITS
    assert int(re.search(r"constexpr uint32_t MID_C_MAX_WBITS = (\d+);", common).group(1)) == F.MID_C_MAX_WBITS
    assert 1 << int(re.search(r"constexpr uint32_t MID_BITMAP_WORDS = 1u << (\d+);", common).group(1)) == F.MID_BITMAP_WORDS
    assert int(re.search(r"constexpr size_t MID_MAX_RECORDS = (\d+);", switches).group(1)) == F.MID_MAX_RECORDS
    # the size rules
    assert re.search(r"small_tier = k <= 15 && entries > 0 && entries <= 3 \* \(size_t\(1\) << MAX_WBITS\);", index_cpp)
    assert re.search(r"level0 = small_tier && k == 15 && 4 \* entries \* 3 <= \(size_t\(32\) << L0_WBITS\) / 2;", index_cpp)
    assert re.search(r"max_wbits = level0 \? MAX_WBITS - 1 : MAX_WBITS;\s*uint32_t wbits = 8;\s*while \(wbits < max_wbits && \(size_t\(1\) << wbits\) \* 5 < entries \* 4\)",
                     index_cpp)
    assert len(re.findall(r"uint32_t cw = 10;\s*while \(cw < MID_C_MAX_WBITS && \(size_t\((?:4|8)\) << cw\) < 4 \* entries\) \+\+cw;", index_cpp)) == 2
    assert re.search(r"mid0_bits = distinct \* 5 <= \(size_t\(32\) << L0_WBITS\) \* 2 \? 3 : 1;", index_cpp)
    assert re.search(r"recs\.size\(\) <= sw\.mid_max_records", index_cpp)
    # the kernel's shifts and which 12-mer keys a group
    assert re.search(r"const int sh_w = 32 - \(int\)fw\.bloom_wbits;", filt) and re.search(r"const uint32_t sh_c = 32u - fw\.midc_wbits;", filt)
    assert re.search(r"const int j = 4 \* g \+ 3;", filt) and re.search(r"lds_at\(L12_BASE \+ \(\(h2 >> sh_w\) << 2\)\)", filt)
    assert len(re.findall(r"group_key\(__funnelshift_r\(r[ab]\.z, r[ab]\.w, 6\)\), BLOOM_C0\) >> sh_c\]", filt)) == 2
    # ... and the restatement's own arithmetic at the edges
    assert [F.bloom_wbits(160 << j, False) for j in range(6)] == list(range(8, 14)) and [F.bloom_wbits((160 << j) + 1, False) for j in range(6)] == list(range(9, 15))
    assert F.bloom_wbits(24_576, False) == 14 and F.bloom_wbits(21_845, True) == 13
    assert [F.blkc_wbits(1 << (cw - 1)) for cw in range(10, 16)] == list(range(10, 16)) and F.blkc_wbits(21_845) == 16
    assert [F.midc_wbits(n) for n in (32_768, 32_769, 65_536, 65_537, 131_072, 131_073, 452_883)] == [15, 16, 16, 17, 17, 17, 17]
    assert [F.tier_of(n, 15) for n in (21_845, 21_846, 180_000, 180_001)] == ["level0", "middle", "middle", None]
    assert [F.tier_of(n, k) for k in (11, 13) for n in (24_576, 24_577)] == ["levels12", None] * 2 and F.tier_of(24_576, 16) is None
    assert [F.mid0_bits(n) for n in (419_430, 419_431)] == [3, 1] and F.MID0_DISTINCT == 419_430
    assert int(F.canon12(np.array([0], np.uint64))[0]) == 0 and int(F.rc_codes(np.array([0], np.uint64), 12)[0]) == 0xAAAAAA  # A x 12 <-> T x 12
    assert int(F.codes_at(F.letters_of("ACTGacgtN"), [0], 9)[0]) == 0 | 1 << 2 | 2 << 4 | 3 << 6 | 0 << 8 | 1 << 10 | 3 << 12 | 2 << 14 | 3 << 16
