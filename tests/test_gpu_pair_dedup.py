"""Duplicate read pairs dropped from the resident sample (drprg_hip_dedup_pairs, csrc/pair_dedup.hip; pytest -m gpu).  Keys, keep flags,
copies, counts and levels come from the rule in plain Python (tests/pair_dedup_rule.py) on the mates the mate-overlap rule
(tests/pair_overlap_rule.py) leaves, the vectors and counters from the oracle and from contexts that were given the kept reads alone --
never from the code under test."""
import numpy as np
import pytest

import pair_dedup_rule as rule
import pair_overlap_rule as overlap_rule
from test_gpu_max_covg import _panel
from test_gpu_pair_overlap import LAYOUT1, LAYOUT2, _DECOY, _expected_readback, _layouts, _map_sides, _pair_fixture, _side, _state
from test_gpu_parity import _ctx

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
EINVAL, ENODATA = 22, 61
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 150, 151, 1025)
DEEP = 20_000
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_FIXTURE = {}
# the classes of the issue's list and what the rule must say of each of their units
CLASSES = dict(same_a_other_b=1, other_a_same_b=1, swapped=1, lower_case=0, n_against_r=0, unknown_elsewhere=1, orphan_again=0, no_bases=1, first_copy=1,
               later_copy=0, last_base_of_b=1, first_base_of_a=1, mask_at_word_edge=1, one_base_shorter=1)


def _other(rng, m, at):
    """m with another letter at `at`"""
    r = bytearray(m)
    r[at] = b"CGTA"[b"ACGT".index(bytes([r[at]]).upper())]
    return bytes(r)


def _fixture():
    """about 3 000 units of every class above over all the lengths, two stacks of 31 and 32 copies, and (kept apart: `deep`) one of 20 000.
    A derived unit stands behind the unit it is derived from, far from it.  Returns (units, tags, deep): tags[i] the class of unit i or None"""
    if _FIXTURE:
        return _FIXTURE["v"]
    rng = np.random.default_rng(61)
    rows = []  # (sort key, a, b, tag)

    def rand(L):
        return rng.choice(_ACGT, size=L).tobytes()

    for k in range(210):
        La, Lb = int(rng.choice(LENGTHS)), int(rng.choice(LENGTHS))
        if La < 31 and Lb < 31:  # (a unit of two very short mates would meet its like by chance: 16 units of two single bases exist)
            Lb = int(rng.choice(LENGTHS[4:]))
        a, b = rand(La), rand(Lb)
        step = iter(range(1, 40))

        def add(x, y, tag):
            rows.append((next(step) + rng.random(), x, y, tag))

        rows.append((rng.random(), a, b, "first_copy"))
        add(a, rand(Lb), "same_a_other_b")
        add(rand(La), b, "other_a_same_b")
        add(b, a, "swapped")
        add(a.lower() if k % 2 else a, b if k % 2 else b.lower(), "lower_case")
        long_is_a = La >= Lb
        m, L = (a, La) if long_is_a else (b, Lb)  # (at least 31 bases)
        p = int(rng.integers(0, L))
        q = (p + 1 + int(rng.integers(0, L - 1))) % L
        with_n, with_r, elsewhere = m[:p] + b"N" + m[p + 1:], m[:p] + b"R" + m[p + 1:], m[:q] + b"n" + m[q + 1:]
        pair = (lambda x: (x, b)) if long_is_a else (lambda x: (a, x))
        add(*pair(with_n), None)
        add(*pair(with_r), "n_against_r")
        add(*pair(elsewhere), "unknown_elsewhere")
        edge = 15 + k % 2  # the last base of word 0, the first of word 1
        add(*pair(m[:edge] + b"N" + m[edge + 1:]), "mask_at_word_edge")
        add(*pair(m[:-1]), "one_base_shorter")
        add(a, _other(rng, b, Lb - 1), "last_base_of_b")
        add(_other(rng, a, 0), b, "first_base_of_a")
        if k % 2:
            add(a, b"", None)
            add(a, b"", "orphan_again")
        else:
            add(b"", b, None)
            add(b"", b, "orphan_again")
        add(a, b, "later_copy")
        if k % 3 == 0:
            add(a.lower(), b.lower(), "later_copy")
        if k % 7 == 0:
            add(b"", b"", "no_bases")
    for copies in (31, 32):
        a, b = rand(150), rand(151)
        rows += [(40 * rng.random(), a, b, None) for _ in range(copies)]
    rows.sort(key=lambda r: r[0])
    units, tags = [(r[1], r[2]) for r in rows], [r[3] for r in rows]
    _FIXTURE["v"] = (units, tags, (rand(150), rand(150)))
    return _FIXTURE["v"]


def _with_deep(units, deep):
    """the deep stack spread over the fixture: five copies in six units are the stack's"""
    rng = np.random.default_rng(62)
    out, rest = [], list(units)
    where = np.sort(rng.integers(0, len(units) + 1, size=DEEP))
    at = 0
    for i in range(len(units) + 1):
        n = int(np.searchsorted(where, i, side="right")) - at
        out += [deep] * n
        at += n
        if i < len(units):
            out.append(rest[i])
    assert len(out) == len(units) + DEEP
    return out


_KEYS = {}


def _unit_key(a, b):
    if (a, b) not in _KEYS:
        _KEYS[(a, b)] = rule.unit_key(a, b)
    return _KEYS[(a, b)]


def _device(ctx, torch, units, key_bits, shift_words=0):
    n = len(units)
    sa, hold_a = _side(torch, [u[0] for u in units], shift_words)
    sb, hold_b = _side(torch, [u[1] for u in units])
    d_keys = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")  # (stale on purpose, all three)
    d_keep = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    d_copies = torch.full((max(n, 1),), 9, dtype=torch.int32, device="cuda")
    out = ctx.dedup_pairs_device(sa, sb, n, key_bits, d_keys.data_ptr(), d_keep.data_ptr(), d_copies.data_ptr())
    torch.cuda.synchronize()
    return d_keys.cpu().numpy().view(np.uint64)[:n].tolist(), d_keep.cpu().numpy()[:n].tolist(), d_copies.cpu().numpy()[:n].tolist(), out


def _want(units):
    keep, copies, cnt, lv, _, _ = rule.run([u[0] for u in units], [u[1] for u in units])
    return [_unit_key(a, b) for a, b in units], keep, copies, dict(cnt, levels=lv)


def _assert_equal(got, want, what):
    for name, g, w in zip(("keys", "keep", "copies"), got[:3], want[:3]):
        bad = [s for s in range(len(w)) if g[s] != w[s]]
        assert not bad, (what, name, [(s, g[s], w[s]) for s in bad[:6]])
    assert got[3] == want[3], (what, got[3], want[3])


# ---- 1. the kernels equal the rule --------------------------------------------------------------------------------------------------------
def test_the_kernels_equal_the_rule(tmp_path):
    import torch
    from drprg_amd.pandora import DependencyError
    units, tags, deep = _fixture()
    n = len(units)
    assert 2800 <= n <= 3600
    want = _want(units)
    # (a fixture without the hard cases cannot pass: every class holds 20 units or more of which the rule says what the class is about)
    census = {c: sum(1 for t, k in zip(tags, want[1]) if t == c and k == v) for c, v in CLASSES.items()}
    print(census, want[3])
    assert min(census.values()) >= 20, census
    assert {len(m) for u in units for m in u} >= set(LENGTHS) | {0}
    assert want[3]["levels"][30] == 1 and want[3]["levels"][31] == 1 and sorted(c for c in want[2] if c >= 31) == [31, 32]
    assert sum(1 for a, b in units if not a and b) >= 20 and sum(1 for a, b in units if a and not b) >= 20
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    for key_bits in (64, 8, 2, 1):
        _assert_equal(_device(ctx, torch, units, key_bits), want, f"key_bits {key_bits}")
    _assert_equal(_device(ctx, torch, units, 64, shift_words=1), want, "side 1 off 16-byte alignment")
    # the deep stack: 20 000 copies of one unit among the others
    big = _with_deep(units, deep)
    want_big = _want(big)
    assert want_big[3]["levels"][31] == 2 and max(want_big[2]) == DEEP and want_big[3]["units_dropped"] == want[3]["units_dropped"] + DEEP - 1
    _assert_equal(_device(ctx, torch, big, 64), want_big, "with the deep stack")
    # a part of the fixture behind other offsets; no pairs at all: nothing is touched
    _assert_equal(_device(ctx, torch, units[7:907], 64), _want(units[7:907]), "units 7 .. 906")
    assert _device(ctx, torch, [], 64)[3] == dict(dict.fromkeys(rule.COUNT_NAMES, 0), levels=[0] * 32)
    # refused: key_bits outside 1 .. 64, offsets that do not end at n_bases
    plain = [np.random.default_rng(s).choice(_ACGT, size=40).tobytes() for s in range(50)]
    sa, hold_a = _side(torch, plain)
    sb, hold_b = _side(torch, plain)
    d = torch.zeros(200, dtype=torch.int64, device="cuda")
    for call in (lambda: ctx.dedup_pairs_device(sa, sb, 50, 0, d.data_ptr(), d.data_ptr() + 800, d.data_ptr() + 1000),
                 lambda: ctx.dedup_pairs_device(sa, sb, 50, 65, d.data_ptr(), d.data_ptr() + 800, d.data_ptr() + 1000),
                 lambda: ctx.dedup_pairs_device((sa[0], sa[1], sa[2] - 40, sa[3], sa[4]), sb, 50, 64, d.data_ptr(), d.data_ptr() + 800, d.data_ptr() + 1000)):
        with pytest.raises(DependencyError) as err:
            call()
        assert err.value.code == EINVAL
    ctx.close()


# ---- the resident stage -------------------------------------------------------------------------------------------------------------------
_PLANTED = {}


def _planted_fixture():
    """the pair fixture of tests/test_gpu_pair_overlap.py (1 200 pairs cut from the haplotype genomes) with copies planted from earlier
    pairs: whole pairs, first mates alone, second mates alone -- across the blocks of either side's layout"""
    if _PLANTED:
        return _PLANTED["v"]
    panel, side1, side2, from_decoy = _pair_fixture()
    side1, side2, from_decoy = list(side1), list(side2), list(from_decoy)
    rng = np.random.default_rng(43)
    for s in range(60, len(side1)):
        h = int(rng.integers(0, s))
        if s % 7 == 1 or s % 7 == 2:  # the whole pair
            side1[s], side2[s], from_decoy[s] = side1[h], side2[h], from_decoy[h]
        elif s % 7 == 3:  # the first mate alone
            side1[s], from_decoy[s] = side1[h], (from_decoy[h][0], from_decoy[s][1])
        elif s % 7 == 5:  # the second mate alone
            side2[s], from_decoy[s] = side2[h], (from_decoy[s][0], from_decoy[h][1])
    _PLANTED["v"] = (panel, side1, side2, from_decoy)
    return _PLANTED["v"]


def _expect(s1, s2, O, e_milli, clip):
    """the overlap rule, then the pair rule on what it leaves: (overlap counts, cut side 1, cut side 2, the pair rule's run)"""
    shifts, keep1, keep2, ocnt = overlap_rule.run(s1, s2, O, e_milli, clip)
    A = [None if m is None else m[:k] for m, k in zip(s1, keep1)]
    B = [None if m is None else m[:k] for m, k in zip(s2, keep2)]
    return ocnt, (keep1, keep2), A, B, rule.run(A, B)


def _resident_flags(run):
    """one byte per resident read: side 1 in file order, then side 2"""
    return [f for f in run[4] if f is not None] + [f for f in run[5] if f is not None]


# ---- 2. the resident call equals the rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
def test_the_resident_call_equals_the_rule(tmp_path, filtered):
    import resident_readback as rb
    panel, side1, side2, from_decoy = _planted_fixture()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    s1, s2 = list(side1), list(side2)
    if filtered:  # reads of either side dropped at ingest: their mates are orphans
        fa = tmp_path / "decoy.fa"
        fa.write_bytes(b">decoy\n" + _DECOY + b"\n")
        ctx.set_read_filter(min_len=40)
        ctx.set_decoy([str(fa)])
        s1 = [None if len(m) < 40 or d[0] else m for m, d in zip(side1, from_decoy)]
        s2 = [None if len(m) < 40 or d[1] else m for m, d in zip(side2, from_decoy)]
        assert sum(m is None for m in s1) > 20 and sum(m is None for m in s2) > 40
    f1, p1, f2, p2 = _layouts(tmp_path, side1, side2, "f" if filtered else "u")
    for clip, key_bits in ((False, 64), (True, 64), (True, 3)):
        ocnt, keeps, A, B, want = _expect(s1, s2, 30, 50, clip)
        cnt, lv = want[2], want[3]
        ctx.set_pair_overlap(30, "0.05", clip)
        ctx.set_dedup_pairs(True)
        _map_sides(ctx, f1, p1, f2, p2)
        assert ctx.pair_overlap() == ocnt
        assert ctx.dedup_pairs_info() == dict(dict.fromkeys(rule.COUNT_NAMES, 0), levels=[0] * 32)  # (none since the reset)
        got = ctx.dedup_pairs(key_bits)
        print(filtered, clip, key_bits, got, lv[:6])
        assert got == cnt, (filtered, clip)
        # duplicates of every kind came up: whole pairs, orphans, and pairs that share one mate only (which stay)
        assert cnt["units_dropped"] > 200 and lv[1] > 50 and lv[2] > 5
        shared = sum(1 for s in range(len(A)) if want[0][s] and A[s] and any(A[s] == A[h] for h in range(s)))
        assert shared > 100
        if filtered or clip:
            assert sum(1 for a, b, k in zip(A, B, want[0]) if not k and (not a or not b)) >= 3  # (a dropped orphan)
        flags = _resident_flags(want)
        assert len(flags) == cnt["reads_before"] and ctx.dedup_pairs_flags(len(flags)).tolist() == flags
        assert ctx.dedup_pairs_info() == dict(cnt, levels=lv)
        back, _ = rb.read_back(ctx)
        kept1 = [k if f else None for k, f in zip(keeps[0], want[4])]
        kept2 = [k if f else None for k, f in zip(keeps[1], want[5])]
        assert back == _expected_readback(s1, s2, kept1, kept2)
        c = ctx.counters()
        assert c["reads"] == cnt["reads_kept"] and c["bases"] == cnt["bases_kept"] and ctx.resident_info()["complete"]
    ctx.close()


# ---- 3. the context afterwards is that of a file of the kept reads -----------------------------------------------------------------------
def test_the_context_afterwards_is_that_of_the_kept_reads(tmp_path, oracle):
    from test_gpu_dedup import _batch, _write_fastq
    from test_gpu_parity import _oracle_index, _oracle_map
    from test_gpu_subsample import _assert_oracle, _map_files
    panel, side1, side2, _ = _planted_fixture()
    ocnt, keeps, A, B, want = _expect(side1, side2, 30, 50, True)
    kept = rule.kept_reads(A, B, want[4], want[5])
    assert len(kept) == want[2]["reads_kept"] < want[2]["reads_before"]
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    ctx.set_pair_overlap(30, "0.05", True)
    ctx.set_dedup_pairs(True)
    f1, p1, f2, p2 = _layouts(tmp_path, side1, side2, "c")
    _map_sides(ctx, f1, p1, f2, p2)
    assert ctx.pair_overlap() == ocnt and ctx.dedup_pairs() == want[2]
    kb, ko = _batch(kept)
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    omap = _oracle_map(oracle, idx, kb, ko, W, K, True)
    assert omap[2]["clusters_kept"] > 5
    _assert_oracle(ctx, omap, len(kept), int(ko[-1]), "behind the stage")
    # a fresh context given the kept reads as one file: the same vectors and counters, and the same subsample (numbered from 0 alike)
    other = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    other.keep_reads(1 << 28)
    _map_files(other, [_write_fastq(tmp_path / "kept.fq", kept)], [True])
    for step in (lambda c: None, lambda c: c.subsample(int(ko[-1]) // 2, 7)):
        a, b = step(ctx), step(other)
        assert a == b, (a, b)
        (ca, pa), (cb, pb) = ctx.coverage(), other.coverage()
        assert np.array_equal(ca, cb) and np.array_equal(pa, pb) and ctx.counters() == other.counters()
        assert ctx.resident_info()["complete"] and other.resident_info()["complete"]
    assert a["reads_before"] == len(kept) and a["reads_kept"] < a["reads_before"]
    assert np.array_equal(ctx.subsample_flags(len(kept)), other.subsample_flags(len(kept)))
    other.close()
    ctx.close()


# ---- 4. a sample without duplicate units is left untouched ------------------------------------------------------------------------------
def test_a_sample_without_duplicate_units_is_left_untouched(tmp_path):
    import resident_readback as rb
    from test_gpu_dedup import _write_fastq
    from test_gpu_subsample import _map_files
    panel, side1, side2, _ = _pair_fixture()
    # forty first mates, each ten times, in front of four hundred second mates that all differ: what --dedup gets wrong
    idx = [s for s in range(len(side1)) if len(side1[s]) >= 100 and len(side2[s]) >= 90][:400]
    s1, s2 = [side1[idx[s % 40]] for s in range(400)], [side2[s] for s in idx]
    ocnt, keeps, A, B, want = _expect(s1, s2, 30, 50, False)
    assert want[2]["units_dropped"] == 0 and want[3][0] == want[2]["units_with_bases"] == 400 and len(set(A)) <= 80
    r1, r2 = _write_fastq(tmp_path / "n1.fq", s1), _write_fastq(tmp_path / "n2.fq", s2)
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    ctx.set_pair_overlap(30, "0.05", False)
    ctx.set_dedup_pairs(True)
    _map_sides(ctx, [r1], [True], [r2], [False])
    assert ctx.pair_overlap() == ocnt
    before, back = _state(ctx), rb.read_back(ctx)
    assert ctx.dedup_pairs() == want[2] and want[2]["reads_kept"] == want[2]["reads_before"] == 800
    assert ctx.dedup_pairs_flags(800).tolist() == [1] * 800 and ctx.dedup_pairs_info()["levels"] == want[3]
    assert _state(ctx) == before and rb.read_back(ctx) == back
    ctx.close()
    # plain dedup on the same reads judges every read alone: it drops first mates of pairs that are no duplicates
    (tmp_path / "twin").mkdir()
    twin = _ctx(tmp_path / "twin", panel, W, K, True, genome_size=G)
    twin.keep_reads(1 << 28)
    _map_files(twin, [r1, r2], [True, False])
    out = twin.dedup()
    assert out["reads_before"] == 800 and out["reads_kept"] <= 800 - 300
    twin.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(tmp_path):
    from drprg_amd.pandora import DependencyError
    from test_gpu_dedup import _write_fastq
    panel, side1, side2, _ = _planted_fixture()
    f1, f2 = _write_fastq(tmp_path / "r1.fq", side1[:400]), _write_fastq(tmp_path / "r2.fq", side2[:400])
    ocnt, keeps, A, B, want = _expect(side1[:400], side2[:400], 30, 50, False)
    assert want[2]["units_dropped"] > 30
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)

    def refused(code, text, call=None, c=None):
        c = c or ctx
        before = _state(c)
        with pytest.raises(DependencyError) as err:
            (call or c.dedup_pairs)()
        assert err.value.code == code and text in str(err.value), str(err.value)
        assert _state(c) == before

    def staged(switch=True, overlap=True):
        ctx.set_pair_overlap(30, "0.05", False)
        ctx.set_dedup_pairs(switch)
        _map_sides(ctx, [f1], [True], [f2], [True])
        if overlap:
            assert ctx.pair_overlap() == ocnt

    refused(EINVAL, "drprg_hip_set_pair_overlap", lambda: ctx.set_dedup_pairs(True))  # no mate-overlap setting
    staged(overlap=False)  # nothing is kept
    refused(ENODATA, "resident")
    ctx.keep_reads(1 << 28)
    staged()
    refused(EINVAL, "key_bits", lambda: ctx.dedup_pairs(0))
    refused(EINVAL, "key_bits", lambda: ctx.dedup_pairs(65))
    assert ctx.dedup_pairs() == want[2]  # (the refusals have left the sample fit for the stage)
    refused(EINVAL, "compacted")  # an earlier call of itself
    staged(switch=False)
    refused(EINVAL, "drprg_hip_set_dedup_pairs")
    staged(overlap=False)
    refused(EINVAL, "drprg_hip_pair_overlap")
    staged()
    assert ctx.dedup()["reads_kept"] < ocnt["reads"]
    refused(EINVAL, "compacted")
    staged()
    assert ctx.subsample(ocnt["bases_kept"] // 2, 3)["reads_kept"] < ocnt["reads"]
    refused(EINVAL, "compacted")
    # a dedup or a subsample that drops nothing compacts nothing: the stage still runs behind it
    staged()
    assert ctx.subsample(ocnt["bases_kept"], 3)["reads_kept"] == ocnt["reads"]
    assert ctx.dedup_pairs() == want[2]
    # switching the mate-overlap setting off switches the stage off
    ctx.set_pair_overlap(0)
    ctx.set_pair_overlap(30, "0.05", False)
    _map_sides(ctx, [f1], [True], [f2], [True])
    assert ctx.pair_overlap() == ocnt
    refused(EINVAL, "drprg_hip_set_dedup_pairs")
    ctx.close()
    from drprg_amd import Context
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=[0, 0])
    multi.set_opts(illumina=True, genome_size=G)
    multi.keep_reads(1 << 28)
    multi.set_pair_overlap(30, "0.05", False)
    multi.set_dedup_pairs(True)
    multi.set_ordered_ingest(True)
    multi.map_fastx(f1)
    multi.map_fastx(f2)
    refused(EINVAL, "several devices", c=multi)
    assert multi.counters()["reads"] == 800
    multi.close()


# ---- 6. the executables -------------------------------------------------------------------------------------------------------------------
QC_STAGES = ["read_trim", "adapter_trim", "front_adapter", "poly_trim", "base_mask", "read_filter", "complexity", "decoy", "max_covg", "pair_overlap", "dedup",
             "subsample"]


def _count_line(c):
    return "pair dedup: " + " ".join(f"{k}={c[k]}" for k in rule.COUNT_NAMES) + " duplication_rate=%.6f" % (c["units_dropped"] / c["units_with_bases"])


def test_pandora_map_dedup_pairs_equals_the_run_on_the_kept_reads(tmp_path):
    import json
    import os
    import subprocess
    from drprg_amd._lib import PANDORA_EXE
    from test_gpu_dedup import _write_fastq
    from test_gpu_pair_overlap import _pandora
    panel, side1, side2, _ = _planted_fixture()
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    panel.write(prg, genes)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r1, r2 = _write_fastq(tmp_path / "R1.fq", side1), _write_fastq(tmp_path / "R2.fq", side2)
    ocnt, keeps, A, B, want = _expect(side1, side2, 30, 50, False)
    cnt = want[2]
    kept = _write_fastq(tmp_path / "kept.fq", rule.kept_reads(A, B, want[4], want[5]))
    _, ref = _pandora(PANDORA_EXE, tmp_path / "ref", prg, genes, kept, ["--max-covg", "4294967295"])
    runs = []
    for name, threads, env in (("t1", 1, None), ("t4", 4, None), ("ascii", 2, dict(DRPRG_HIP_INPUT="ascii"))):
        extra = ["--mate", r2, "--dedup-pairs"] + (["--qc-json", str(tmp_path / "qc.json")] if name == "t1" else [])
        stdout, vcf = _pandora(PANDORA_EXE, tmp_path / name, prg, genes, r1, extra, threads=threads, env=env)
        assert _count_line(cnt) in stdout and f"reads={cnt['reads_kept']} bases={cnt['bases_kept']} " in stdout, (name, stdout)
        runs.append(vcf)
    assert runs[0] == runs[1] == runs[2] == ref
    stages = json.load(open(tmp_path / "qc.json"))["stages"]
    assert stages["pair_dedup"] == [cnt[k] for k in rule.COUNT_NAMES] + want[3]
    assert list(stages) == QC_STAGES[:10] + ["pair_dedup"] + QC_STAGES[10:]
    # without the flag the report holds no key of the stage, and the pairs are all there
    stdout, vcf = _pandora(PANDORA_EXE, tmp_path / "plain", prg, genes, r1, ["--mate", r2, "--qc-json", str(tmp_path / "plain.json")])
    text = open(tmp_path / "plain.json").read()
    assert list(json.loads(text)["stages"]) == QC_STAGES and "pair_dedup" not in text and "pair dedup" not in stdout
    assert f"reads={ocnt['reads']} bases={ocnt['bases_kept']} " in stdout
    # the sample must be resident
    r = subprocess.run([PANDORA_EXE, "map", "-o", str(tmp_path / "off"), "-g", str(G), "--mate", r2, "--dedup-pairs", "-w", str(W), "-k", str(K), "-I", prg, r1],
                       capture_output=True, text=True, env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "pandora_genotyped.vcf").exists()


def test_drprg_predict_dedup_pairs_equals_the_run_on_the_kept_reads(tmp_path):
    import json
    import os
    import re
    import subprocess
    from test_gpu_dedup import _write_fastq
    from test_gpu_pair_overlap import _revcomp
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    from util import vcf_without_date
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 3000, seed=1)
    block = bases.reshape(3000, 150)
    side1, side2 = [], []
    for s, row in enumerate(block):  # mates that do not reach each other; every third pair is an earlier one again, every fifth shares its first mate
        R = block[s // 2].tobytes() if s % 3 == 0 and s else row.tobytes()
        first = block[s - 5].tobytes() if s % 5 == 0 and s % 3 and s else R
        side1.append(first[:70])
        side2.append(_revcomp(R[80:]))
    ocnt, keeps, A, B, want = _expect(side1, side2, 30, 50, False)
    cnt = want[2]
    assert cnt["units_dropped"] > 300 and want[3][1] > 100
    for d in ("p", "k"):
        (tmp_path / d).mkdir()
    r1, r2 = _write_fastq(tmp_path / "p" / "wt.fq", side1), _write_fastq(tmp_path / "p" / "wt_2.fq", side2)
    kept = _write_fastq(tmp_path / "k" / "wt.fq", rule.kept_reads(A, B, want[4], want[5]))

    def run(fq, out, extra, env=None):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "-o", str(tmp_path / out), "-s", "wt", "-I", "-v"] + extra
        return subprocess.run(argv, capture_output=True, text=True, env=env)

    def report(out):
        return (vcf_without_date(str(tmp_path / out / "pandora_genotyped.vcf")),
                re.sub(r'"vcfid": "[0-9a-f]{8}"', '"vcfid": "ID"', open(tmp_path / out / "wt.drprg.json").read()))

    a, b = run(r1, "m", ["--mate", r2, "--dedup-pairs", "--qc-json", str(tmp_path / "qc.json")]), run(kept, "r", [])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert report("m") == report("r")
    assert _count_line(cnt) in a.stderr and f"] reads={cnt['reads_kept']} " in a.stderr, a.stderr
    assert json.load(open(tmp_path / "qc.json"))["stages"]["pair_dedup"] == [cnt[k] for k in rule.COUNT_NAMES] + want[3]
    r = run(r1, "off", ["--mate", r2, "--dedup-pairs"], env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "wt.drprg.json").exists()
