"""Overlapping mates merged into one read (csrc/pair_merge.hip; pytest -m gpu).  Shifts, merged reads and all twenty counts come from the
rules in plain Python (tests/pair_merge_rule.py over tests/pair_overlap_rule.py), never from the code under test."""
import numpy as np
import pytest

import pair_merge_rule as rule
import pair_overlap_rule as po
from test_gpu_dedup import _pack
from test_gpu_max_covg import _panel
from test_gpu_pair_overlap import (G, K, LAYOUT1, LAYOUT2, W, _layouts, _map_sides, _pair_fixture, _pandora, _pandora_files, _revcomp, _side,
                                   _state)
from test_gpu_parity import _ctx

pytestmark = pytest.mark.gpu

EINVAL, EOVERFLOW = 22, 75
LENGTHS = (8, 15, 16, 17, 31, 32, 33, 150, 1023, 1024)
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_FIXTURE = {}


def _plant(rng, La, Lb, d, dis=(), unk_a=(), unk_b=()):
    """mates a (La) and b (Lb) of one random molecule with B = revcomp(b) at shift d.  Columns are positions of a (and of the merged read):
    B differs at the columns `dis`, a holds an N at `unk_a` and B one at `unk_b`, wherever the mate covers the column"""
    lo, hi = min(0, d), max(La, Lb + d)
    mol = rng.choice(_ACGT, size=hi - lo)
    a = bytearray(mol[-lo:-lo + La].tobytes())
    B = bytearray(mol[d - lo:d - lo + Lb].tobytes())
    for p in dis:
        if 0 <= p - d < Lb and p < La:
            B[p - d] = b"CGTA"[b"ACGT".index(B[p - d])]
    for p in unk_a:
        if 0 <= p < La:
            a[p] = ord("N")
    for p in unk_b:
        if 0 <= p - d < Lb:
            B[p - d] = ord("n")
    return bytes(a), _revcomp(bytes(B))


def _fixture():
    """about 400 pairs; the conditions they must meet are checked in test_the_kernel_equals_the_rule from the rule alone"""
    if _FIXTURE:
        return _FIXTURE["v"]
    rng = np.random.default_rng(31)
    pairs = []
    # every combination of the lengths, at a shift of either sign where one leaves eight columns or more
    for La in LENGTHS:
        for Lb in LENGTHS:
            ov = min(La, Lb)
            for sign in (-1, 1):
                c = int(rng.integers(max(8, ov // 2), ov + 1))  # columns both cover
                d = La - c if sign > 0 else c - Lb             # B's tail on a's tail, or B's head under a's head
                if -(Lb - 1) <= d <= La - 1:
                    pairs.append(_plant(rng, La, Lb, d))
    # the merged length at 16 k - 1, 16 k, 16 k + 1
    for k in (1, 2, 3, 5, 9):
        for I in (16 * k - 1, 16 * k, 16 * k + 1):
            for La, Lb in ((33, 33), (150, 150), (17, 150)):
                if I >= 8 and -(Lb - 1) <= I - Lb <= La - 1 and min(La, I) + min(Lb, I) - I >= 8:
                    pairs.append(_plant(rng, La, Lb, I - Lb))
    # the longest merge O = 8 allows, and its neighbours
    for c in (8, 9, 24):
        pairs.append(_plant(rng, 1024, 1024, 1024 - c))
    # every phase of d, both signs; the five kinds of column at the edges of M's words: a disagreement in the first and the last column
    # of a word, unknown bases of either mate and of both, an unknown base of b behind a's end and one of a in front of B
    for La, Lb, d0 in ((150, 150, -47), (150, 150, 20), (150, 33, 40), (150, 31, 60), (33, 150, -70), (150, 151, 0)):
        for ph in range(16):
            d = d0 + ph if d0 else 0
            c0, c1 = max(0, d), min(La, Lb + d)
            w = (c0 + 15) // 16 * 16  # the first word of M that lies inside the overlap
            dis = (w, w + 15) if c1 - c0 >= 31 and ph % 2 == 0 else ((w + 15,) if c1 - c0 >= 31 else ())
            pairs.append(_plant(rng, La, Lb, d, dis=dis, unk_a=(c0 + 1, w + 16, 2), unk_b=(c0 + 2, w + 16, w + 17, Lb + d - 1, La + 3)))
    # d = 0 at every length (mates of equal and of different lengths)
    for L in LENGTHS:
        pairs.append(_plant(rng, L, L, 0))
        pairs.append(_plant(rng, L, max(8, L - 3), 0))
    merging = len(pairs)
    # pairs that do not merge, standing between those that do: unrelated mates, orphans of either side, a mate of 1025 bases
    for k in range(10):
        pairs.append((rng.choice(_ACGT, size=150).tobytes(), rng.choice(_ACGT, size=int(rng.choice((17, 150)))).tobytes()))
    for k in range(12):
        m = rng.choice(_ACGT, size=int(rng.choice(LENGTHS))).tobytes()
        pairs.append((m, b"") if k % 2 else (b"", m))
    for k in range(8):
        pairs.append(_plant(rng, 1025, 150, 20) if k % 2 else _plant(rng, 150, 1025, -900))
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    side1, side2 = [p[0] for p in pairs], [p[1] for p in pairs]
    tables = [po.shift_counts(po.codes(a), po.codes(b)) if a and b and max(len(a), len(b)) <= po.PO_MAX_LEN else None for a, b in pairs]
    _FIXTURE["v"] = (side1, side2, tables, merging)
    return _FIXTURE["v"]


def _expected_batch(new1, shifts):
    """the merged batch: an unmerged pair is a read of no bases"""
    reads = [m if d > po.NOT_JUDGED else b"" for m, d in zip(new1, shifts)]
    return _pack(reads)


def _device(ctx, torch, side1, side2, shift_words=0, cap_words=None, cap_npos=None, room=8):
    n = len(side1)
    sa, hold_a = _side(torch, side1, shift_words)
    sb, hold_b = _side(torch, side2)
    total = sum(len(a) + len(b) for a, b in zip(side1, side2))
    cw = (total + 15) // 16 if cap_words is None else cap_words
    cn = total if cap_npos is None else cap_npos
    d_s = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")  # (stale on purpose)
    d_o = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_w = torch.full((cw + room,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_n = torch.full((cn + room,), -3, dtype=torch.int64, device="cuda")
    c12, c8, n_list = ctx.pair_merge_device(sa, sb, n, d_s.data_ptr(), d_o.data_ptr(), d_w.data_ptr(), cw, d_n.data_ptr(), cn)
    torch.cuda.synchronize()
    words, npos = d_w.cpu().numpy().view(np.uint32), d_n.cpu().numpy()
    assert (words[cw:] == 0x5A5A5A5A).all() and (npos[cn:] == -3).all()  # nothing behind the capacities is touched
    return d_s.cpu().numpy()[:n].tolist(), d_o.cpu().numpy().astype(np.uint64), words[:cw], npos[:n_list].astype(np.uint64), c12, c8


def _assert_batch(got, want, side1, what):
    shifts, new1, new2, c12, c8 = want
    words, npos, offs = _expected_batch(new1, shifts)
    assert got[0] == shifts, what
    assert np.array_equal(got[1], offs), what
    bad = np.flatnonzero(got[2][:words.size] != words)
    assert bad.size == 0, (what, bad[:5], [hex(int(got[2][i])) for i in bad[:5]], [hex(int(words[i])) for i in bad[:5]])
    assert (got[2][words.size:] == 0x5A5A5A5A).all(), what  # the room behind the batch's last word, inside the capacity, is not touched
    assert np.array_equal(got[3], npos), what
    assert got[4] == c12 and got[5] == c8, (what, got[4], c12, got[5], c8)


# ---- 1. the kernel equals the rule --------------------------------------------------------------------------------------------------------
def test_the_kernel_equals_the_rule(tmp_path):
    import torch
    from drprg_amd.pandora import DependencyError
    side1, side2, tables, merging = _fixture()
    n = len(side1)
    assert 300 <= n <= 600
    O, e = 8, "0.1"
    want = rule.run(side1, side2, O, po.error_milli(e), tables=tables)
    shifts = want[0]
    # ---- the conditions, from the rule ----
    assert shifts == po.run(side1, side2, O, 100, False, tables=tables)[0]
    shape = dict.fromkeys(("d < 0", "d = 0", "0 < d", "d + Lb < La"), 0)
    kinds = np.zeros(4, np.int64)
    first_last = [0, 0, 0]  # disagreements in the first / the last column of a word of M; unknown bases of b alone in M
    seen_d, merged_lens = set(), set()
    for a, b, d in zip(side1, side2, shifts):
        if d <= po.NOT_JUDGED:
            continue
        La, Lb = len(a), len(b)
        shape["d < 0" if d < 0 else "d = 0" if d == 0 else "d + Lb < La" if d + Lb < La else "0 < d"] += 1
        M, k4, kind = rule.merge(a, b, d)
        kinds += k4
        first_last[0] += int(((kind == 1) & (np.arange(len(M)) % 16 == 0)).sum())
        first_last[1] += int(((kind == 1) & (np.arange(len(M)) % 16 == 15)).sum())
        first_last[2] += sum(1 for p in range(La, len(M)) if M[p:p + 1] == b"N")
        seen_d.add(d)
        merged_lens.add(len(M))
    unmerged = dict(none=sum(d == po.NONE for d in shifts), orphan=sum((not a) != (not b) for a, b in zip(side1, side2)),
                    too_long=sum(bool(a) and bool(b) and max(len(a), len(b)) > po.PO_MAX_LEN for a, b in zip(side1, side2)))
    print(shape, kinds, first_last, unmerged, want[3], want[4])
    assert min(shape.values()) >= 20 and kinds.min() >= 20 and min(unmerged.values()) >= 5 and min(first_last) >= 5
    assert {d % 16 for d in seen_d if d >= 0} == set(range(16)) and {d % 16 for d in seen_d if d < 0} == set(range(16))
    assert 2040 in merged_lens and any(L % 16 == 15 for L in merged_lens) and any(L % 16 == 0 for L in merged_lens) and any(L % 16 == 1 for L in merged_lens)
    assert {(len(a), len(b)) for a, b, d in zip(side1, side2, shifts) if d > po.NOT_JUDGED} >= {(x, y) for x in LENGTHS for y in LENGTHS}
    assert any(d >= 0 and d + len(b) < len(a) for a, b, d in zip(side1, side2, shifts) if d > po.NOT_JUDGED)  # B inside a
    assert any(d < 0 and d + len(b) > len(a) for a, b, d in zip(side1, side2, shifts) if d > po.NOT_JUDGED)   # a inside B
    z = list(zip(shifts[:-2], shifts[1:-1], shifts[2:]))
    assert any(x > po.NOT_JUDGED and y <= po.NOT_JUDGED and t > po.NOT_JUDGED for x, y, t in z)  # an unmerged pair between merged ones
    # ---- the kernel ----
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.set_pair_overlap(O, e, False)
    with pytest.raises(DependencyError) as err:  # without the switch the entry refuses
        _device(ctx, torch, side1[:4], side2[:4])
    assert err.value.code == EINVAL
    ctx.set_pair_merge(True)
    got = _device(ctx, torch, side1, side2)
    _assert_batch(got, want, side1, "the whole fixture")
    # word buffers that are not 16-byte aligned: the same answers
    _assert_batch(_device(ctx, torch, side1, side2, shift_words=1), want, side1, "shifted words")
    # sides whose first read starts at each of the 16 phases of a word (an orphan of p bases in front of either side)
    sub = slice(0, 60)
    for p in range(16):
        q = (7 * p + 3) % 16
        lead1, lead2 = [(b"ACGT" * 4)[:p], b""], [b"", (b"TTGCA" * 4)[:q]]
        a1, a2 = lead1 + side1[sub], lead2 + side2[sub]
        w = rule.run(a1, a2, O, 100, tables=[None, None] + tables[sub])
        _assert_batch(_device(ctx, torch, a1, a2), w, a1, f"phase {p}/{q}")
    # another setting: the defaults
    ctx.set_pair_overlap(30, "0.05", False)
    w = rule.run(side1, side2, 30, 50, tables=tables)
    assert 0 < w[4]["pairs_merged"] < want[4]["pairs_merged"]
    _assert_batch(_device(ctx, torch, side1, side2), w, side1, "the defaults")
    # too little room for the words or for the list: -EOVERFLOW, and nothing behind the capacity is written (checked in _device)
    ctx.set_pair_overlap(O, e, False)
    n_words, n_list = (int(got[1][-1]) + 15) // 16, got[3].size
    assert n_list > 50
    _assert_batch(_device(ctx, torch, side1, side2, cap_words=n_words, cap_npos=n_list), want, side1, "exact capacities")
    for cw, cn in ((n_words - 1, n_list), (n_words, n_list - 1)):
        with pytest.raises(DependencyError) as err:
            _device(ctx, torch, side1, side2, cap_words=cw, cap_npos=cn)
        assert err.value.code == EOVERFLOW
    # no pairs: nothing is touched
    empty = _device(ctx, torch, [], [])
    assert empty[4] == dict.fromkeys(po.COUNT_NAMES, 0) and empty[5] == dict.fromkeys(rule.COUNT_NAMES, 0)
    # the switch: refused beside the clip and without a setting, and each refusal leaves the setting as it was
    ctx.set_pair_merge(False)
    ctx.set_pair_overlap(30, "0.05", True)
    with pytest.raises(DependencyError) as err:
        ctx.set_pair_merge(True)
    assert err.value.code == EINVAL
    ctx.set_pair_overlap(30, "0.05", False)
    ctx.set_pair_merge(True)
    with pytest.raises(DependencyError) as err:
        ctx.set_pair_overlap(30, "0.05", True)
    assert err.value.code == EINVAL
    _assert_batch(_device(ctx, torch, side1, side2), w, side1, "behind the refusal")  # (still merging, still without the clip)
    ctx.set_pair_overlap(0)
    with pytest.raises(DependencyError) as err:
        ctx.set_pair_merge(True)
    assert err.value.code == EINVAL
    ctx.close()


# ---- 2. the resident stage ------------------------------------------------------------------------------------------------------------------
def _expected_readback(new1, new2):
    import resident_readback as rb
    out = []
    for side, (cuts, forms) in ((new1, LAYOUT1), (new2, LAYOUT2)):
        for i, form in enumerate(forms):
            out += rb.expected([m for m in side[cuts[i]:cuts[i + 1]] if m is not None], form != "ascii")[0]
    return out


@pytest.mark.parametrize("filtered", [False, True])
def test_the_resident_call_equals_the_rule(tmp_path, filtered):
    import resident_readback as rb
    from test_gpu_pair_overlap import _DECOY
    panel, side1, side2, from_decoy = _pair_fixture()
    n = len(side1)
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    s1, s2 = list(side1), list(side2)
    if filtered:
        fa = tmp_path / "decoy.fa"
        fa.write_bytes(b">decoy\n" + _DECOY + b"\n")
        ctx.set_read_filter(min_len=40)
        ctx.set_decoy([str(fa)])
        s1 = [None if len(m) < 40 or d[0] else m for m, d in zip(side1, from_decoy)]
        s2 = [None if len(m) < 40 or d[1] else m for m, d in zip(side2, from_decoy)]
    f1, p1, f2, p2 = _layouts(tmp_path, side1, side2, "f" if filtered else "u")
    for O, e in ((30, "0.05"), (12, "0.1")):
        want = rule.run(s1, s2, O, po.error_milli(e))
        ctx.set_pair_overlap(O, e, False)
        ctx.set_pair_merge(True)
        _map_sides(ctx, f1, p1, f2, p2)
        got = ctx.pair_overlap()
        print(O, e, got, ctx.pair_merge_info())
        assert got == want[3] and ctx.pair_merge_info() == want[4], (O, e)
        assert want[4]["pairs_merged"] > 300 and want[4]["columns_disagreeing"] + want[4]["columns_filled"] > 5 and got["orphans"] > 5 and got["pairs_too_long"] > 5
        assert ctx.pair_overlap_shifts(n).tolist() == want[0] and ctx.pair_overlap_info() == got
        back, _ = rb.read_back(ctx)
        assert back == _expected_readback(want[1], want[2])
        cnt = ctx.counters()
        assert cnt["reads"] == got["reads"] and cnt["bases"] == got["bases_kept"] and ctx.resident_info()["complete"]
        # with the switch off the stage is the parent's: the rule of "mate overlap" alone
        ctx.set_pair_merge(False)
        plain = po.run(s1, s2, O, po.error_milli(e), False)
        _map_sides(ctx, f1, p1, f2, p2)
        assert ctx.pair_overlap() == plain[3] and ctx.pair_merge_info() == dict.fromkeys(rule.COUNT_NAMES, 0)
        from test_gpu_pair_overlap import _expected_readback as cut_readback
        assert rb.read_back(ctx)[0] == cut_readback(s1, s2, plain[1], plain[2])
    ctx.close()


def test_the_context_afterwards_is_that_of_the_merged_file(tmp_path):
    import resident_readback as rb
    from test_gpu_dedup import _write_fastq
    from test_gpu_subsample import _map_files
    panel, side1, side2, _ = _pair_fixture()
    want = rule.run(side1, side2, 30, 50)
    merged = rule.merged_file(want[1], want[2])
    total = sum(len(r) for r in merged)
    f1, p1, f2, p2 = _layouts(tmp_path, side1, side2, "c")
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    ctx.set_pair_overlap(30, "0.05", False)
    ctx.set_pair_merge(True)
    _map_sides(ctx, f1, p1, f2, p2)
    assert ctx.pair_overlap() == want[3]
    # a fresh context given the rule's file as one file: the same device vectors, counters and resident bytes, the same dedup and subsample
    other = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    other.keep_reads(1 << 28)
    _map_files(other, [_write_fastq(tmp_path / "merged.fq", merged)], [True])
    assert b"".join(rb.read_back(ctx)[0]) == b"".join(rb.read_back(other)[0])
    where = ctx.device_coverage(), other.device_coverage()  # (addresses: the vectors coverage() reads stay where they are)
    for step in (lambda c: None, lambda c: c.dedup(), lambda c: c.subsample(total // 2)):
        a, b = step(ctx), step(other)
        assert a == b, (a, b)
        (ca, pa), (cb, pb) = ctx.coverage(), other.coverage()
        assert np.array_equal(ca, cb) and np.array_equal(pa, pb) and ctx.counters() == other.counters() and (ctx.device_coverage(), other.device_coverage()) == where
        assert ctx.resident_info()["complete"] and other.resident_info()["complete"]
    assert a["reads_kept"] < a["reads_before"]
    # ... and the same duplicate pairs: the rule's two sides mapped as mates (nothing merges a second time: every merged b is empty)
    n1, n2 = _write_fastq(tmp_path / "new1.fq", want[1]), _write_fastq(tmp_path / "new2.fq", want[2])
    results = []
    for c, files in ((ctx, None), (other, (n1, n2))):
        c.set_pair_overlap(30, "0.05", False)
        c.set_pair_merge(files is None)
        c.set_dedup_pairs(True)
        if files:
            _map_sides(c, [files[0]], [True], [files[1]], [False])
            assert c.pair_overlap()["bases_kept"] == want[3]["bases_kept"]
        else:
            _map_sides(c, f1, p1, f2, p2)
            assert c.pair_overlap() == want[3]
        results.append((c.dedup_pairs(), c.coverage()[0].tobytes(), c.counters()))
    assert results[0] == results[1] and results[0][0]["units"] == len(side1)
    other.close()
    ctx.close()


def test_a_sample_without_a_mergeable_pair_is_left_untouched(tmp_path):
    from test_gpu_dedup import _write_fastq
    panel, side1, side2, _ = _pair_fixture()
    all_want = po.run(side1, side2, 30, 50, False)
    idx = [s for s, d in enumerate(all_want[0]) if d in (po.NONE, po.NOT_JUDGED)]
    s1, s2 = [side1[s] for s in idx], [side2[s] for s in idx]
    assert len(idx) > 300
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    ctx.set_pair_overlap(30, "0.05", False)
    ctx.set_pair_merge(True)
    _map_sides(ctx, [_write_fastq(tmp_path / "n1.fq", s1)], [True], [_write_fastq(tmp_path / "n2.fq", s2)], [False])
    before = _state(ctx)
    got = ctx.pair_overlap()
    want = rule.run(s1, s2, 30, 50)
    assert got == want[3] and got["bases_kept"] == got["bases_before"] and ctx.pair_merge_info() == want[4] == dict.fromkeys(rule.COUNT_NAMES, 0)
    assert _state(ctx) == before
    ctx.close()


# ---- 3. the executables ---------------------------------------------------------------------------------------------------------------------
def _lines(c12, c8):
    return ("mate overlap: " + " ".join(f"{k}={c12[k]}" for k in po.COUNT_NAMES), "mate merging: " + " ".join(f"{k}={c8[k]}" for k in rule.COUNT_NAMES))


def test_pandora_map_pair_merge_equals_the_run_on_the_merged_file(tmp_path):
    import gzip
    import os
    import subprocess
    from test_gpu_dedup import _write_fastq
    exe, prg, genes, side1, side2, r1, r2 = _pandora_files(tmp_path)
    nocap = ["--max-covg", "4294967295"]
    want = rule.run(side1, side2, 30, 50)
    merged = _write_fastq(tmp_path / "merged.fq", rule.merged_file(want[1], want[2]))
    flags = ["--mate", r2, "--pair-merge"]
    stdout, got = _pandora(exe, tmp_path / "m", prg, genes, r1, flags)
    _, ref = _pandora(exe, tmp_path / "r", prg, genes, merged, nocap)
    l12, l8 = _lines(want[3], want[4])
    assert got == ref and l12 in stdout and l8 in stdout and f"reads={want[3]['reads']} bases={want[3]['bases_kept']} " in stdout, stdout
    _, clipped = _pandora(exe, tmp_path / "clip", prg, genes, r1, ["--mate", r2, "--pair-clip-overlap"])
    assert got != clipped  # (merging does change what the files report)
    behind = ["--dedup", "--subsample-covg", "8", "--seed", "3"]
    _, got_b = _pandora(exe, tmp_path / "ms", prg, genes, r1, flags + behind)
    _, ref_b = _pandora(exe, tmp_path / "rs", prg, genes, merged, behind)
    assert got_b == ref_b and want[3]["bases_kept"] > 8 * G
    # the same run under -t 1 and -t 4, from FASTQ text, gz and packed input
    g1, g2 = str(tmp_path / "R1.fq.gz"), str(tmp_path / "R2.fq.gz")
    for src, dst in ((r1, g1), (r2, g2)):
        with open(src, "rb") as fi, gzip.open(dst, "wb") as fo:
            fo.write(fi.read())
    runs = []
    for name, threads, env, a, b in (("t1", 1, None, r1, r2), ("t4", 4, None, r1, r2), ("ascii", 2, dict(DRPRG_HIP_INPUT="ascii"), r1, r2), ("gz", 2, None, g1, g2)):
        out, vcf = _pandora(exe, tmp_path / name, prg, genes, a, ["--mate", b, "--pair-merge"], threads=threads, env=env)
        assert l12 in out and l8 in out, (name, out)
        runs.append((vcf, [l for l in out.splitlines() if l.startswith("[pandora-hip] reads=")][0].split(" in ")[0]))
    assert all(r == runs[0] for r in runs) and runs[0][0] == got
    # the two usage errors
    base = [exe, "map", "-o", str(tmp_path / "u"), "-g", str(G), "-w", str(W), "-k", str(K), "-I", prg, r1]
    for extra in (["--pair-merge"], ["--mate", r2, "--pair-merge", "--pair-clip-overlap"]):
        assert subprocess.run(base + extra, capture_output=True, text=True).returncode == 2
    # the sample must be resident
    r = subprocess.run(base + flags, capture_output=True, text=True, env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "u" / "pandora_genotyped.vcf").exists()


def test_drprg_predict_pair_merge_equals_the_run_on_the_merged_file(tmp_path):
    import json
    import os
    import re
    import subprocess
    from test_gpu_dedup import _write_fastq
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    from util import vcf_without_date
    idx, panel, sites = _make_index(tmp_path)
    n = 4500
    bases, offs = _reads(panel, lambda g, i: 0, n, seed=1)
    block = bases.reshape(n, 150)
    rng = np.random.default_rng(8)
    side1, side2 = [], []
    for s, row in enumerate(block):
        R = bytearray(row.tobytes())
        if s % 3 == 0:    # an insert of 100 bases under reads of 150: both mates run into the adapter
            a, b = bytes(R[:100]) + rng.choice(_ACGT, size=50).tobytes(), _revcomp(bytes(R[:100])) + rng.choice(_ACGT, size=50).tobytes()
        elif s % 3 == 1:  # mates of 110 bases over an insert of 150: 70 columns overlap, one of them disagrees in every fifth pair
            B = bytearray(R[40:])
            if s % 5 == 0:
                B[30] = b"CGTA"[b"ACGT".index(B[30])]
            a, b = bytes(R[:110]), _revcomp(bytes(B))
        else:             # mates that do not reach each other
            a, b = bytes(R[:75]), _revcomp(bytes(R[76:]))
        side1.append(a)
        side2.append(b)
    tables = [po.shift_counts(po.codes(a), po.codes(b)) for a, b in zip(side1, side2)]
    for d in ("p", "m"):
        (tmp_path / d).mkdir()
    r1, r2 = _write_fastq(tmp_path / "p" / "wt.fq", side1), _write_fastq(tmp_path / "p" / "wt_2.fq", side2)

    def run(fq, out, extra, env=None):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "-o", str(tmp_path / out), "-s", "wt", "-I", "-v"] + extra
        return subprocess.run(argv, capture_output=True, text=True, env=env)

    def report(out):
        return (vcf_without_date(str(tmp_path / out / "pandora_genotyped.vcf")),
                re.sub(r'"vcfid": "[0-9a-f]{8}"', '"vcfid": "ID"', open(tmp_path / out / "wt.drprg.json").read()))

    want = rule.run(side1, side2, 30, 50, tables=tables)
    assert want[4]["pairs_merged"] >= 2 * n // 3 - 2 and want[4]["columns_disagreeing"] >= n // 15 - 2
    merged = _write_fastq(tmp_path / "m" / "wt.fq", rule.merged_file(want[1], want[2]))
    flags = ["--mate", r2, "--pair-merge"]
    a, b = run(r1, "got", flags + ["--qc-json", str(tmp_path / "qc.json")]), run(merged, "ref", [])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert report("got") == report("ref")
    l12, l8 = _lines(want[3], want[4])
    assert l12 in a.stderr and l8 in a.stderr and f"] reads={want[3]['reads']} " in a.stderr, a.stderr
    stages = json.load(open(tmp_path / "qc.json"))["stages"]
    assert stages["pair_overlap"] == [want[3][k] for k in po.COUNT_NAMES] and stages["pair_merge"] == [want[4][k] for k in rule.COUNT_NAMES]
    # the same run from gz under -t 1, and from FASTQ text handed over as ASCII under -t 4
    import gzip
    (tmp_path / "z").mkdir()
    g1, g2 = str(tmp_path / "z" / "wt.fq.gz"), str(tmp_path / "z" / "wt_2.fq.gz")
    for src, dst in ((r1, g1), (r2, g2)):
        with open(src, "rb") as fi, gzip.open(dst, "wb", compresslevel=1) as fo:
            fo.write(fi.read())
    for out, fq, extra, env in (("gz1", g1, ["--mate", g2, "--pair-merge", "-t", "1"], None),
                                ("a4", r1, flags + ["-t", "4"], dict(os.environ, DRPRG_HIP_INPUT="ascii"))):
        z = run(fq, out, extra, env=env)
        assert z.returncode == 0, z.stderr
        assert report(out) == report("got") and l12 in z.stderr and l8 in z.stderr, (out, z.stderr)
    behind = ["--dedup", "--subsample-covg", "0.05", "--seed", "3"]
    a, b = run(r1, "gots", flags + behind), run(merged, "refs", behind)
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert report("gots") == report("refs")
    # without the flag the report is what it was: no new key, the stage's entry that of "mate overlap" alone, and the same bytes every time
    plain = po.run(side1, side2, 30, 50, False, tables=tables)
    texts = []
    for k in range(2):
        q = run(r1, f"q{k}", ["--mate", r2, "--qc-json", str(tmp_path / f"q{k}.json")])
        assert q.returncode == 0 and "mate merging:" not in q.stderr
        texts.append(open(tmp_path / f"q{k}.json", "rb").read())
    assert texts[0] == texts[1] and b"pair_merge" not in texts[0]
    assert json.loads(texts[0])["stages"]["pair_overlap"] == [plain[3][k] for k in po.COUNT_NAMES]
    assert list(json.loads(texts[0])["stages"]) == [k for k in stages if k != "pair_merge"]
    # the usage errors, and a sample that is not resident
    for extra in (["--pair-merge"], flags + ["--pair-clip-overlap"]):
        assert run(r1, "u", extra).returncode == 2
    r = run(r1, "off", flags, env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "wt.drprg.json").exists()
