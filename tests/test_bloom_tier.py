"""The panels and batches of tests/bloom_tier.py, checked on the CPU with the oracle alone: every panel's index is past the switch (or
exactly at it), and every batch sends enough minimizers down each way through the restated Bloom array and probe table -- index keys,
minimizers the array rejects, minimizers it lets through to a table that does not hold them, keys stored outside their home slot's group of
four, keys whose chain wraps -- that no case of tests/test_gpu_bloom_tier.py passes empty.  The census of every panel is printed."""
import os
import re

import numpy as np
import pytest

import bloom_tier as B
from util import ROOT, cluster_fraction, map_params

MATRIX_BITS, MATRIX_WBITS = 18, 15  # 65 537 .. 131 072 keys


def _tables(oracle, panel, w, k):
    return B.Tables(oracle.build_index(panel.prgs, w, k)["keys"], k)


def _kept(oracle, panel, bases, offs, w, k):
    """clusters the oracle keeps of the batch (Illumina parameters, as the device cases map it)"""
    md, er = map_params(k, True)
    return oracle.map_reads(bases, offs, oracle.build_index(panel.prgs, w, k), w, k, md, float(cluster_fraction(er, k)), B.MCS)[2]["clusters_kept"]


@pytest.mark.parametrize("name", list(B.MATRIX))
def test_matrix_panel_and_batch(oracle, name):
    w, k = B.MATRIX[name][:2]
    panel = B.matrix_panel(name)
    assert max(len(r) for r in panel.refs) < 10_000
    t = _tables(oracle, panel, w, k)
    assert B.KEY_RANGE[0] <= t.n <= B.KEY_RANGE[1], (name, t.n)
    assert t.tier and t.bits == MATRIX_BITS and t.wbits == MATRIX_WBITS, (name, t.n, t.tier, t.bits, t.wbits)
    assert B.bloom_passes(t.bloom, t.wbits, t.keys).all()
    bases, offs = B.matrix_batch(name)
    lengths = np.diff(offs.astype(np.int64))
    assert (lengths == 150).sum() >= 2400 and ((lengths >= 3000) & (lengths <= 9000)).sum() >= 40 and lengths.max() <= 9000
    assert (lengths == 0).sum() >= 3 and ((lengths > 0) & (lengths < k)).sum() >= 3 and int(offs[-1]) < 1_000_000
    text = bases.tobytes()
    assert all(b"N" in text[int(offs[i]):int(offs[i + 1])] for i in range(0, len(lengths), 10) if lengths[i])
    c = B.census(oracle, t, bases, offs, w, k)
    high = float((t.keys >> np.uint64(32) != 0).mean())
    print(f"{name} (w={w}, k={k}): {t.n} keys, 2^{t.bits} slots at {t.load:.4f}, 2^{t.wbits} words, {high:.4f} of the keys with a high half; "
          f"{len(lengths)} reads, {int(offs[-1])} bases: {c}")
    few = w == 33  # (minimizers are sparse)
    assert c["keyed_rejected"] == 0                         # no false negative in the restatement
    assert c["keyed"] >= (1000 if few else 5000), c
    assert c["rejected"] >= (1000 if few else 5000), c
    assert c["pass_not_key"] >= (50 if few else 200), c
    assert c["other_group"] >= 100, c
    assert _kept(oracle, panel, bases, offs, w, k) > 1000
    if name in B.FOLDED:
        assert high >= 0.99
        assert c["keyed_found_without_the_fold"] < 0.10 * c["keyed"], c  # (a device that dropped the fold would lose nine hits in ten)
    else:
        assert c["keyed_found_without_the_fold"] == c["keyed"]
    if name == "P0116":
        assert high == 0.0 and int(t.keys.max()) >= 1 << 31  # 16-byte slots, keys that fill 32 bits, nothing for the fold to do


@pytest.mark.parametrize("k", B.THRESHOLD_K)
def test_threshold_panels_and_batches(tmp_path, oracle, k):
    from test_index_oracle import _product_index
    wrapping = {}
    trees = []
    for n_keys, bits, tier, wbits in zip(B.THRESHOLD_KEYS, (17, 18, 18), (False, True, True), (14, 14, 15)):
        panel = B.threshold_panel(oracle, k, n_keys)
        t = B.threshold_tables(oracle, k, n_keys)
        assert t.n == n_keys and t.bits == bits and t.tier == tier and t.wbits == wbits, (k, n_keys, t.n, t.bits, t.tier, t.wbits)
        assert B.bloom_passes(t.bloom, t.wbits, t.keys).all()
        trees.append(panel.prgs)
        assert "5" not in panel.prgs[-1]  # (the last locus is site-free)
        bases, offs, first_planted = B.threshold_batch(oracle, k, n_keys)
        c = B.census(oracle, t, bases, offs, 1, k)
        print(f"k={k}, {n_keys} keys: 2^{t.bits} slots at {t.load:.6f}, tier {t.tier}, 2^{t.wbits} words, {int(t.wraps.sum())} wrapping keys, "
              f"{int((t.behind >= 4).sum())} keys four or more slots from home (farthest {int(t.behind.max())}), "
              f"{len(offs) - 1 - first_planted} planted reads: {c}")
        assert c["keyed_rejected"] == 0 and c["keyed"] >= 5000 and c["rejected"] >= 5000 and c["pass_not_key"] >= 200, c
        assert c["behind4"] >= 100 and c["other_group"] >= 100, c
        assert _kept(oracle, panel, bases, offs, 1, k) > 1000
        wrapping[n_keys] = c["wrapping"]
        # the host's side of the switch: the product's table is the size the restatement says (a host-only context: no device)
        ctx, _ = _product_index(tmp_path, panel.names, panel.prgs, 1, k)
        assert ctx.n_keys == n_keys and ctx.n_slots == 1 << bits
        ctx.close()
    # the three panels differ in the last locus alone, by one base each
    assert trees[0][:-1] == trees[1][:-1] == trees[2][:-1]
    assert trees[1][-1][:-1] == trees[0][-1] and trees[2][-1][:-1] == trees[1][-1]
    full = B.threshold_tables(oracle, k, B.THRESHOLD_KEYS[0])
    assert full.load > 0.4999 and full.wraps.any()
    assert wrapping[B.THRESHOLD_KEYS[0]] >= 1, wrapping  # (found on both k: see THRESHOLD_SEED)


def test_the_recorded_seeds_are_the_first_with_a_wrapping_chain(oracle):
    """the search is not run again in full: the recorded seed has a wrapping chain, the seed before it has none"""
    for k, seed in B.THRESHOLD_SEED.items():
        assert B.find_threshold_seed(oracle, k, range(seed - 1, seed + 1)) == seed


def _source(name):
    return open(os.path.join(ROOT, "drprg_amd", "csrc", name)).read()


def test_the_constants_of_the_restatement_are_the_sources():
    hx = lambda s: int(s, 16)
    kernels, index_h, index_cpp, mapper, common, wave = (_source(n) for n in ("kernels.h", "index.h", "index.cpp", "mapper.cpp", "device_common.h",
                                                                               "sketch_wave.hip"))
    # the Bloom mix, on the host and device (kernels.h) and where the wave form spells it out for a 32-bit key
    m = re.search(r"pbloom_mix\(uint64_t key\) \{ return \(\(uint32_t\)key \^ \(uint32_t\)\(key >> 32\)\) \* (0x[0-9A-Fa-f]+)u; \}", kernels)
    assert hx(m.group(1)) == B.MUL32
    assert re.search(r"pbloom_word\(uint32_t m, uint32_t wbits\) \{ return m >> \(32 - wbits\); \}", kernels)
    assert re.search(r"pbloom_bits\(uint32_t m\) \{ return \(1u << \(m & 31\)\) \| \(1u << \(\(m >> 5\) & 31\)\); \}", kernels)
    assert hx(re.search(r"\(hvs\[p\[u\]\] - 1u\) \* (0x[0-9A-Fa-f]+)u", wave).group(1)) == B.MUL32
    # the home slot, on the host (index.h) and on the device (device_common.h)
    for text in (index_h, common):
        assert hx(re.search(r"key \* (0x[0-9A-Fa-f]+)u\) >> \(32 - bits\)", text).group(1)) == B.MUL32
        assert hx(re.search(r"key \* (0x[0-9A-Fa-f]+)ULL\) >> \(64 - bits\)", text).group(1)) == B.MUL64
    # the table's size and the insertion
    assert int(re.search(r"uint32_t bits = (\d+);\s*while \(\(1ULL << bits\) < 2 \* f\.keys\.size\(\) \+ 1\) \+\+bits;", index_cpp).group(1)) == B.BITS_START
    assert re.search(r"table_slot\(f\.keys\[i\], bits, k <= 15\)", index_cpp) and re.search(r"s = \(s \+ 1\) & \(uint32_t\)\(nslot - 1\)", index_cpp)
    # the tier's condition and the array's size
    m = re.search(r"nslot \* \(size_t\)\(wide_hash \? (\d+) : (\d+)\) > \(\(size_t\)(\d+) << (\d+)\)", mapper)
    assert (int(m.group(1)), int(m.group(2))) == (B.slot_bytes(16), B.slot_bytes(15)) and int(m.group(3)) << int(m.group(4)) == B.TIER_ABOVE_BYTES
    assert re.search(r"tables_\.fill\(idx, p\.k > 15,", mapper)
    m = re.search(r"pbloom_wbits = (\d+);\s*while \(\(\(size_t\)(\d+) << pbloom_wbits\) < idx\.keys\.size\(\)\) \+\+pbloom_wbits;", mapper)
    assert int(m.group(1)) == B.WBITS_START and int(m.group(2)) == 4
    # ... and the restatement's own arithmetic at the switch
    assert [B.table_bits(n) for n in B.THRESHOLD_KEYS] == [17, 18, 18] and [B.bloom_wbits(n) for n in B.THRESHOLD_KEYS] == [14, 14, 15]
    assert [B.tier_present(n, k) for k in (15, 16) for n in B.THRESHOLD_KEYS] == [False, True, True] * 2
    assert int(B.pbloom_mix([0x0000000100000003])[0]) == (2 * B.MUL32) & 0xFFFFFFFF and int(B.mix_without_the_fold([0x0000000100000003])[0]) == (3 * B.MUL32) & 0xFFFFFFFF
    assert int(B.home_slots([0xFFFFFFFFFFFFFFFF], 18, 16)[0]) == ((0xFFFFFFFFFFFFFFFF * B.MUL64) % (1 << 64)) >> 46
