"""Read-through adapters cut by mate overlap (csrc/pair_overlap.hip; pytest -m gpu).  Shifts, kept lengths and the twelve counts come from
the rule in plain Python (tests/pair_overlap_rule.py), never from the code under test."""
import numpy as np
import pytest

import pair_overlap_rule as rule
from test_gpu_dedup import _pack
from test_gpu_max_covg import _panel
from test_gpu_parity import _ctx

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
EINVAL = 22
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 150, 151, 1024, 1025)
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGTacgtNR", b"TGCAtgcaNY")
_FIXTURE = {}


def _revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def _planted(rng, La, Lb, d, subs=0, unknown=()):
    """mates a (La) and b (Lb) of one random molecule with B = revcomp(b) lying at shift d; `subs` letters of b inside the overlap are
    changed, and the columns `unknown` (counted in a) get an N in a (even) or b (odd), where they are inside the overlap"""
    lo, hi = min(0, d), max(La, Lb + d)
    mol = rng.choice(_ACGT, size=hi - lo)
    a = bytearray(mol[-lo:-lo + La].tobytes())
    B = bytearray(mol[d - lo:d - lo + Lb].tobytes())
    c0, c1 = max(0, d), min(La, Lb + d)
    cols = list(range(c0, c1))
    for i in unknown:
        if c0 <= i < c1:
            if i % 2 == 0:
                a[i] = ord("N")
            else:
                B[i - d] = ord("n")
    free = [i for i in cols if i not in set(unknown)]
    for i in (rng.choice(free, size=min(subs, len(free)), replace=False) if free and subs else []):
        j = int(i) - d
        B[j] = b"CGTA"[b"ACGT".index(bytes([B[j]]).upper())]
    if rng.random() < 0.2:
        a = bytearray(bytes(a).lower())
    return bytes(a), _revcomp(B)


def _fixture():
    """about 2 000 pairs: planted read-through and plain overlaps at every phase of d and both signs, the edge shifts, substitutions at the
    threshold, unknown bases at word edges, unrelated mates, mates of 1025 bases and empty mates"""
    if _FIXTURE:
        return _FIXTURE["v"]
    rng = np.random.default_rng(23)
    pairs = []
    short = [L for L in LENGTHS if L <= 151]
    edges = (15, 16, 17, 31, 32, 47, 48, 63, 64)
    # the edge shifts of every combination of lengths: one column, and exactly O columns (O = 8 and 30)
    for La in LENGTHS[:-1]:
        for Lb in LENGTHS[:-1]:
            if max(La, Lb) == 1024 and min(La, Lb) < 150:
                continue
            pairs.append(_planted(rng, La, Lb, -(Lb - 1)))
            for O in (8, 30):
                if La >= O and Lb >= O:
                    pairs.append(_planted(rng, La, Lb, La - O))
                    pairs.append(_planted(rng, La, Lb, La - O + 1))  # one column short
                    pairs.append(_planted(rng, La, Lb, O - Lb))  # O columns at the other end: a read-through
    # read-through: the insert is shorter than a mate (d < La - Lb or d < 0); every residue of d mod 16 comes up many times
    for k in range(520):
        La, Lb = (int(rng.choice(short[1:])), int(rng.choice(short[1:]))) if k % 12 else (1024, int(rng.choice((150, 151, 1024))))
        ins = int(rng.integers(8, max(9, max(La, Lb))))
        d = ins - Lb
        c = min(La, Lb + d) - max(0, d)
        if c < 1:
            continue
        allowed = (100 * c) // 1000
        subs = int(rng.choice((0, 1, 2, 3, min(3, allowed), min(3, allowed + 1))))
        pairs.append(_planted(rng, La, Lb, d, subs, edges if k % 3 == 0 else ()))
    # plain overlap: the insert is at least as long as both mates
    for k in range(520):
        La, Lb = (int(rng.choice(short[3:])), int(rng.choice(short[3:]))) if k % 12 else (int(rng.choice((151, 1024))), 1024)
        c = int(rng.integers(8, min(La, Lb) + 1))
        d = La - c
        if Lb + d < La:
            continue
        allowed = (50 * c) // 1000
        subs = int(rng.choice((0, 1, 2, 3, min(3, allowed), min(3, allowed + 1))))
        pairs.append(_planted(rng, La, Lb, d, subs, edges if k % 3 == 0 else ()))
    # unrelated mates
    for k in range(260):
        La, Lb = int(rng.choice(LENGTHS[:-2])), int(rng.choice(LENGTHS[:-2]))
        pairs.append((rng.choice(_ACGT, size=La).tobytes(), rng.choice(_ACGT, size=Lb).tobytes()))
    # a mate of 1025 bases: the pair passes whatever it holds
    for k in range(130):
        La, Lb = (1025, int(rng.choice(LENGTHS))) if k % 2 else (int(rng.choice(LENGTHS)), 1025)
        pairs.append(_planted(rng, La, Lb, int(rng.integers(-20, 20))))
    # empty mates
    for k in range(60):
        L = int(rng.choice(LENGTHS))
        pairs.append(((b"", rng.choice(_ACGT, size=L).tobytes()), (rng.choice(_ACGT, size=L).tobytes(), b""), (b"", b""))[k % 3])
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    side1, side2 = [p[0] for p in pairs], [p[1] for p in pairs]
    tables = [rule.shift_counts(rule.codes(a), rule.codes(b)) if a and b and max(len(a), len(b)) <= rule.PO_MAX_LEN else None for a, b in pairs]
    _FIXTURE["v"] = (side1, side2, tables)
    return _FIXTURE["v"]


def _classes(side1, side2, shifts, keep1, keep2):
    n = dict(read_through=0, plain=0, none=0, too_long=0)
    for a, b, d, ka, kb in zip(side1, side2, shifts, keep1, keep2):
        if a and b and max(len(a), len(b)) > rule.PO_MAX_LEN:
            n["too_long"] += 1
        elif d == rule.NONE:
            n["none"] += 1
        elif d != rule.NOT_JUDGED:
            n["read_through" if min(len(a), len(b) + d) < len(a) or min(len(b), len(b) + d) < len(b) else "plain"] += 1
    return n


def _side(torch, reads, shift_words=0):
    words, npos, offs = _pack(reads)
    buf = np.zeros(words.size + 4 + shift_words, np.uint32)
    buf[shift_words:shift_words + words.size] = words
    d_w = torch.from_numpy(buf.view(np.int32)).cuda()
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_n = torch.from_numpy(npos.astype(np.int64)).cuda() if npos.size else None
    return (d_w.data_ptr() + 4 * shift_words, d_o.data_ptr(), int(offs[-1]), d_n.data_ptr() if npos.size else None, int(npos.size)), (d_w, d_o, d_n)


def _device(ctx, torch, side1, side2, shift_words=0):
    n = len(side1)
    sa, hold_a = _side(torch, side1, shift_words)
    sb, hold_b = _side(torch, side2)
    d_s = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")  # (stale on purpose)
    d_ka = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    d_kb = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    counts = ctx.pair_overlap_device(sa, sb, n, d_s.data_ptr(), d_ka.data_ptr(), d_kb.data_ptr())
    torch.cuda.synchronize()
    return d_s.cpu().numpy()[:n].tolist(), d_ka.cpu().numpy()[:n].tolist(), d_kb.cpu().numpy()[:n].tolist(), counts


# ---- 1. the kernel equals the rule --------------------------------------------------------------------------------------------------------
def test_the_kernel_equals_the_rule(tmp_path):
    import torch
    from drprg_amd.pandora import DependencyError
    side1, side2, tables = _fixture()
    n = len(side1)
    assert 1800 <= n <= 2600
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    seen_d = set()
    for O, e, clip in ((8, "0.1", False), (30, "0.05", True), (30, "0", False)):
        want = rule.run(side1, side2, O, rule.error_milli(e), clip, tables=tables)
        cls = _classes(side1, side2, *want[:3])
        print(O, e, clip, cls, want[3])
        # (a fixture without hard cases cannot pass.  At e = 0 every planted substitution disqualifies its pair, so the overlapping classes
        # are held to the pairs planted without one: a sixth of about 1 000, less those with fewer than 30 known columns)
        assert min(cls.values()) >= (100 if e != "0" else 40), cls
        if clip:
            assert want[3]["bases_clipped"] > 1000 and want[3]["reads_emptied"] > 10
        seen_d |= {d for d in want[0] if d > rule.NOT_JUDGED}
        ctx.set_pair_overlap(O, e, clip)
        got = _device(ctx, torch, side1, side2)
        bad = [s for s in range(n) if (got[0][s], got[1][s], got[2][s]) != (want[0][s], want[1][s], want[2][s])]
        assert not bad, (O, e, clip, [(s, len(side1[s]), len(side2[s]), [g[s] for g in got[:3]], [w[s] for w in want[:3]]) for s in bad[:6]])
        assert got[3] == want[3], (O, e, clip)
    assert {d % 16 for d in seen_d if d >= 0} == set(range(16)) and {d % 16 for d in seen_d if d < 0} == set(range(16))
    # word buffers that are not 16-byte aligned, and the first pairs alone behind other offsets: the same answers
    ctx.set_pair_overlap(8, "0.1", False)
    want = rule.run(side1, side2, 8, 100, False, tables=tables)
    got = _device(ctx, torch, side1, side2, shift_words=1)
    assert (got[0], got[1], got[2]) == tuple(want[:3])
    sub = rule.run(side1[5:305], side2[5:305], 8, 100, False, tables=tables[5:305])
    got = _device(ctx, torch, side1[5:305], side2[5:305])
    assert (got[0], got[1], got[2]) == tuple(sub[:3]) and got[3] == sub[3]
    # no pairs: nothing is touched; no setting, or offsets that leave the batch: refused
    assert _device(ctx, torch, [], [])[3] == dict.fromkeys(rule.COUNT_NAMES, 0)
    plain = [np.random.default_rng(s).choice(_ACGT, size=40).tobytes() for s in range(50)]  # (no listed position: nothing else reads n_bases)
    sa, hold_a = _side(torch, plain)
    sb, hold_b = _side(torch, plain)
    d_s, d_k = torch.zeros(50, dtype=torch.int32, device="cuda"), torch.zeros(100, dtype=torch.int64, device="cuda")
    with pytest.raises(DependencyError) as err:
        ctx.pair_overlap_device((sa[0], sa[1], sa[2] - 40, sa[3], sa[4]), sb, 50, d_s.data_ptr(), d_k.data_ptr(), d_k.data_ptr() + 400)
    assert err.value.code == EINVAL
    ctx.set_pair_overlap(0)
    with pytest.raises(DependencyError) as err:
        ctx.pair_overlap_device(sa, sb, 50, d_s.data_ptr(), d_k.data_ptr(), d_k.data_ptr() + 400)
    assert err.value.code == EINVAL
    with pytest.raises(ValueError):  # (more than three places: the binding refuses it as the executables do, it never rounds)
        ctx.set_pair_overlap(30, "0.0501")
    for bad_setting in ((7, "0.05"), (1025, "0.05"), (30, "0.251")):
        with pytest.raises(DependencyError) as err:
            ctx.set_pair_overlap(*bad_setting)
        assert err.value.code == EINVAL
    ctx.close()


# ---- the resident stage ---------------------------------------------------------------------------------------------------------------------
_PAIRS = {}
_DECOY = np.random.default_rng(77).choice(_ACGT, size=3000).tobytes()


def _pair_fixture():
    """about 1 200 pairs of mates cut from the haplotype genomes, upper-case ACGTN (what the oracle maps): a quarter read through into a
    random adapter, a third overlap, the rest do not; some mates hold an N, a few are empty, short, of 1025 bases, or come from the decoy"""
    if _PAIRS:
        return _PAIRS["v"]
    panel, genomes = _panel()
    rng = np.random.default_rng(41)
    side1, side2, from_decoy = [], [], []
    n = 1200
    for s in range(n):
        La, Lb = (150, 150) if s % 5 else (int(rng.choice((75, 100, 151))), int(rng.choice((90, 150, 151))))
        what = rng.random()
        ins = int(rng.integers(35, min(La, Lb))) if what < 0.25 else (int(rng.integers(max(La, Lb), La + Lb - 29)) if what < 0.6 else int(rng.integers(La + Lb + 10, 600)))
        decoy = (s % 40 == 7, s % 40 in (7, 23))  # either mate, or the second alone, is a contaminant
        if s % 97 == 11:
            La, ins = 1025, 1400
        h = genomes.haps[int(rng.integers(0, len(genomes.haps)))]
        at = int(rng.integers(0, len(h) - ins + 1))
        frag = h[at:at + ins].tobytes()
        if rng.random() < 0.5:
            frag = _revcomp(frag)
        mates = []
        for L, f, dec in ((La, frag, decoy[0]), (Lb, _revcomp(frag), decoy[1])):
            m = bytearray((f + rng.choice(_ACGT, size=max(0, L - len(f))).tobytes())[:L])
            if dec:
                p = int(rng.integers(0, len(_DECOY) - L))
                m = bytearray(_DECOY[p:p + L])
            if rng.random() < 0.06:
                m[int(rng.integers(0, L))] = ord("N")
            mates.append(bytes(m))
        if s % 101 == 5:
            mates[s % 2] = b""
        if s % 89 == 3:
            mates[0] = mates[0][:int(rng.integers(1, 38))]  # (below the --min-read-len of the filtered case)
        side1.append(mates[0])
        side2.append(mates[1])
        from_decoy.append(decoy)
    _PAIRS["v"] = (panel, side1, side2, from_decoy)
    return _PAIRS["v"]


LAYOUT1 = ([0, 500, 900, 1200], ["packed", "ascii", "bam"])
LAYOUT2 = ([0, 300, 1000, 1200], ["ascii", "bam", "packed"])


def _map_sides(ctx, files1, formats1, files2, formats2, threads=1, begin=True):
    ctx.reset()
    ctx.set_threads(threads)
    ctx.set_ordered_ingest(True)
    for k, (files, formats) in enumerate(((files1, formats1), (files2, formats2))):
        if k and begin:
            ctx.begin_mates()
        for f, packed in zip(files, formats):
            ctx.set_input_format(packed)
            ctx.map_fastx(f)
    ctx.set_input_format(False)


def _layouts(tmp_path, side1, side2, tag):
    from test_gpu_dedup import _write_layout
    f1, p1 = _write_layout(tmp_path, side1, LAYOUT1[0], LAYOUT1[1], tag + "1")
    f2, p2 = _write_layout(tmp_path, side2, LAYOUT2[0], LAYOUT2[1], tag + "2")
    return f1, p1, f2, p2


def _expected_readback(side1, side2, keep1, keep2):
    """what the resident sample reads back as: block by block, a packed block normalised, a block without a base gone"""
    import resident_readback as rb
    out = []
    for side, keep, (cuts, forms) in ((side1, keep1, LAYOUT1), (side2, keep2, LAYOUT2)):
        for i, form in enumerate(forms):
            part = [m[:k] for m, k in zip(side[cuts[i]:cuts[i + 1]], keep[cuts[i]:cuts[i + 1]]) if k is not None]
            out += rb.expected(part, form != "ascii")[0]
    return out


def _state(ctx):
    cov, prg = ctx.coverage()
    return cov.tobytes(), prg.tobytes(), ctx.counters(), ctx.resident_info(), ctx.device_coverage()


# ---- 2. the resident call equals the rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
def test_the_resident_call_equals_the_rule(tmp_path, filtered):
    import resident_readback as rb
    panel, side1, side2, from_decoy = _pair_fixture()
    n = len(side1)
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    s1, s2 = list(side1), list(side2)
    if filtered:  # reads of either side dropped at ingest: their mates are orphans, and the shifts keep the size of the files
        fa = tmp_path / "decoy.fa"
        fa.write_bytes(b">decoy\n" + _DECOY + b"\n")
        ctx.set_read_filter(min_len=40)
        ctx.set_decoy([str(fa)])
        s1 = [None if len(m) < 40 or d[0] else m for m, d in zip(side1, from_decoy)]
        s2 = [None if len(m) < 40 or d[1] else m for m, d in zip(side2, from_decoy)]
        assert sum(m is None for m in s1) > 20 and sum(m is None for m in s2) > 40
    f1, p1, f2, p2 = _layouts(tmp_path, side1, side2, "f" if filtered else "u")
    for O, e, clip in ((30, "0.05", False), (30, "0.05", True), (12, "0.1", False)):
        want = rule.run(s1, s2, O, rule.error_milli(e), clip)
        ctx.set_pair_overlap(O, e, clip)
        _map_sides(ctx, f1, p1, f2, p2)
        if filtered:
            assert ctx.decoy_info()["reads_dropped"] == sum(d[k] and len(m[k]) >= 40 for d, m in zip(from_decoy, zip(side1, side2)) for k in (0, 1))
            assert ctx.read_filter_info()["dropped_short"] == sum(len(m) < 40 for m in side1 + side2)
        got = ctx.pair_overlap()
        print(O, e, clip, got)
        assert got == want[3], (O, e, clip)
        assert got["pairs_read_through"] > 150 and got["pairs_overlapping"] - got["pairs_read_through"] > 150 and got["orphans"] > 5 and got["pairs_too_long"] > 5
        assert ctx.pair_overlap_shifts(n).tolist() == want[0] and ctx.pair_overlap_info() == got
        back, _ = rb.read_back(ctx)
        assert back == _expected_readback(s1, s2, want[1], want[2])
        cnt = ctx.counters()
        assert cnt["reads"] == got["reads"] and cnt["bases"] == got["bases_kept"] and ctx.resident_info()["complete"]
    ctx.close()


# ---- 3. the context afterwards is that of the cut reads -----------------------------------------------------------------------------------
def test_the_context_afterwards_is_that_of_the_cut_reads(tmp_path, oracle):
    from test_gpu_dedup import _batch, _write_fastq
    from test_gpu_parity import _oracle_index, _oracle_map
    from test_gpu_subsample import _assert_oracle, _map_files
    panel, side1, side2, _ = _pair_fixture()
    want = rule.run(side1, side2, 30, 50, True)
    cut = rule.cut_reads(side1, side2, want[1], want[2])
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    ctx.set_pair_overlap(30, "0.05", True)
    f1, p1, f2, p2 = _layouts(tmp_path, side1, side2, "c")
    _map_sides(ctx, f1, p1, f2, p2)
    assert ctx.pair_overlap() == want[3]
    cb, co = _batch(cut)
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    omap = _oracle_map(oracle, idx, cb, co, W, K, True)
    assert omap[2]["clusters_kept"] > 5
    _assert_oracle(ctx, omap, len(cut), int(co[-1]), "behind the stage")
    # a fresh context given the cut reads as one file: the same vectors, counters and resident bytes, and the same dedup and subsample
    other = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    other.keep_reads(1 << 28)
    _map_files(other, [_write_fastq(tmp_path / "cut.fq", cut)], [True])
    for step in (lambda c: None, lambda c: c.dedup(), lambda c: c.subsample(int(co[-1]) // 2)):
        a, b = step(ctx), step(other)
        assert a == b, (a, b)
        (ca, pa), (cb2, pb) = ctx.coverage(), other.coverage()
        assert np.array_equal(ca, cb2) and np.array_equal(pa, pb) and ctx.counters() == other.counters()
        assert ctx.resident_info()["complete"] and other.resident_info()["complete"]
    assert a["reads_kept"] < a["reads_before"]  # (the subsample cut something: both numbered the reads alike)
    other.close()
    ctx.close()


# ---- 4. a sample in which no pair overlaps is left untouched ----------------------------------------------------------------------------
def test_a_sample_without_overlaps_is_left_untouched(tmp_path):
    from test_gpu_dedup import _write_fastq
    panel, side1, side2, _ = _pair_fixture()
    all_want = rule.run(side1, side2, 30, 50, False)
    idx = [s for s, d in enumerate(all_want[0]) if d in (rule.NONE, rule.NOT_JUDGED)]
    s1, s2 = [side1[s] for s in idx], [side2[s] for s in idx]
    assert len(idx) > 300
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    ctx.set_pair_overlap(30, "0.05", False)
    _map_sides(ctx, [_write_fastq(tmp_path / "n1.fq", s1)], [True], [_write_fastq(tmp_path / "n2.fq", s2)], [False])
    before = _state(ctx)
    got = ctx.pair_overlap()
    want = rule.run(s1, s2, 30, 50, False)
    assert got == want[3] and got["bases_kept"] == got["bases_before"] and got["pairs_overlapping"] == 0
    assert ctx.pair_overlap_shifts(len(idx)).tolist() == want[0]
    assert _state(ctx) == before
    ctx.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(tmp_path):
    from drprg_amd.pandora import DependencyError
    from test_gpu_dedup import _write_fastq
    panel, side1, side2, _ = _pair_fixture()
    f1, f2 = _write_fastq(tmp_path / "r1.fq", side1[:400]), _write_fastq(tmp_path / "r2.fq", side2[:400])
    f2_short = _write_fastq(tmp_path / "r2s.fq", side2[:399])
    big1, big2 = _write_fastq(tmp_path / "b1.fq", side1 * 5), _write_fastq(tmp_path / "b2.fq", side2 * 5)  # more than one ingest block each
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)

    def refused(code, text, call=None, c=None):
        c = c or ctx
        before = _state(c)
        with pytest.raises(DependencyError) as err:
            (call or c.pair_overlap)()
        assert err.value.code == code and text in str(err.value), str(err.value)
        assert _state(c) == before

    ctx.set_pair_overlap(30, "0.05", False)
    _map_sides(ctx, [f1], [True], [f2], [True])  # nothing is kept
    refused(61, "resident")
    # ... and discover, which would pile up the first file alone, says so too (both files are mapped: the call is refused, not served from a file)
    (tmp_path / "disc").mkdir()
    refused(61, "two mate files", lambda: ctx.discover_reads(f1, str(tmp_path / "genes.fa"), str(tmp_path / "disc")))
    ctx.keep_reads(1 << 28)
    _map_sides(ctx, [f1], [True], [f2], [True], begin=False)
    refused(EINVAL, "drprg_hip_begin_mates")
    _map_sides(ctx, [f1], [True], [f2], [True])
    refused(EINVAL, "twice", ctx.begin_mates)
    ctx.set_max_covg(5)
    refused(EINVAL, "depth cap")
    ctx.set_max_covg(None)
    refused(EINVAL, "drprg_hip_map_host", lambda: ctx.map_host(np.frombuffer(b"ACGT", np.uint8), np.array([0, 4], np.uint64)))
    _map_sides(ctx, [f1], [True], [f2_short], [True])
    refused(84, "400 and 399")
    ctx.reset()
    ctx.set_threads(2)
    ctx.set_ordered_ingest(False)
    ctx.map_fastx(big1)
    ctx.begin_mates()
    ctx.map_fastx(big2)
    refused(EINVAL, "order")
    # without the setting: every entry of the stage refuses, and the sample is numbered by nothing
    ctx.set_pair_overlap(0)
    _map_sides(ctx, [f1], [True], [f2], [True], begin=False)
    refused(EINVAL, "drprg_hip_set_pair_overlap")
    refused(EINVAL, "drprg_hip_set_pair_overlap", ctx.begin_mates)
    # and the stage runs once per sample: a second call finds the numbers gone
    ctx.set_pair_overlap(30, "0.05", False)
    _map_sides(ctx, [f1], [True], [f2], [True])
    assert ctx.pair_overlap()["pairs_read_through"] > 50
    refused(EINVAL, "compacted")
    # behind the stage discover takes the cut reads of both files from device memory
    ctx.discover_reads(f1, str(tmp_path / "genes.fa"), str(tmp_path / "disc"))
    assert ctx.resident_info()["last_discover_from_hbm"]
    ctx.close()
    # a context over several devices (one device listed twice, as tests/test_gpu_dedup.py does): both entries refuse, the sample stays
    from drprg_amd import Context
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=[0, 0])
    multi.set_opts(illumina=True, genome_size=G)
    multi.keep_reads(1 << 28)
    multi.set_pair_overlap(30, "0.05", False)
    multi.set_ordered_ingest(True)
    multi.map_fastx(f1)
    refused(EINVAL, "several devices", multi.begin_mates, c=multi)
    multi.map_fastx(f2)
    refused(EINVAL, "several devices", c=multi)
    assert multi.counters()["reads"] == 800
    multi.close()


# ---- 6. the executables -------------------------------------------------------------------------------------------------------------------
def _count_line(c):
    return "mate overlap: " + " ".join(f"{k}={c[k]}" for k in rule.COUNT_NAMES)


def _pandora(exe, out, prg, genes, reads, extra, threads=2, env=None):
    import os
    import subprocess
    from util import vcf_without_date
    argv = [exe, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(G)] + extra + [
        "--vcf-refs", genes, "-t", str(threads), "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
    r = subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return r.stdout, vcf_without_date(str(out / "pandora_genotyped.vcf"))


def _pandora_files(tmp_path):
    import subprocess
    from drprg_amd._lib import PANDORA_EXE
    from test_gpu_dedup import _write_fastq
    panel, side1, side2, _ = _pair_fixture()
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    panel.write(prg, genes)
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return PANDORA_EXE, prg, genes, side1, side2, _write_fastq(tmp_path / "R1.fq", side1), _write_fastq(tmp_path / "R2.fq", side2)


def test_pandora_map_mate_equals_the_run_on_the_cut_file(tmp_path):
    import os
    import subprocess
    from test_gpu_dedup import _write_fastq
    exe, prg, genes, side1, side2, r1, r2 = _pandora_files(tmp_path)
    nocap = ["--max-covg", "4294967295"]
    seen = []
    for clip in (False, True):
        want = rule.run(side1, side2, 30, 50, clip)
        cut = _write_fastq(tmp_path / f"cut{int(clip)}.fq", rule.cut_reads(side1, side2, want[1], want[2]))
        flags = ["--mate", r2] + (["--pair-clip-overlap"] if clip else [])
        stdout, got = _pandora(exe, tmp_path / f"m{int(clip)}", prg, genes, r1, flags)  # (the default cap gives way)
        _, ref = _pandora(exe, tmp_path / f"c{int(clip)}", prg, genes, cut, nocap)
        assert got == ref and _count_line(want[3]) in stdout and f"reads={want[3]['reads']} bases={want[3]['bases_kept']} " in stdout, stdout
        seen.append(got)
        behind = ["--dedup", "--subsample-covg", "8", "--seed", "3"]
        _, got = _pandora(exe, tmp_path / f"ms{int(clip)}", prg, genes, r1, flags + behind)
        _, ref = _pandora(exe, tmp_path / f"cs{int(clip)}", prg, genes, cut, behind)
        assert got == ref and want[3]["bases_kept"] > 8 * G
    _, uncut = _pandora(exe, tmp_path / "cat", prg, genes, _write_fastq(tmp_path / "cat.fq", side1 + side2), nocap)
    assert seen[0] != uncut and seen[1] != seen[0]  # (the cuts do change what the files report)
    # other settings reach the stage
    want = rule.run(side1, side2, 100, 0, False)
    stdout, _ = _pandora(exe, tmp_path / "o", prg, genes, r1, ["--mate", r2, "--pair-min-overlap", "100", "--pair-error", "0"])
    assert _count_line(want[3]) in stdout and want[3]["pairs_overlapping"] < 400
    # the sample must be resident: with that switched off the run fails, it never maps the files unpaired
    r = subprocess.run([exe, "map", "-o", str(tmp_path / "off"), "-g", str(G), "--mate", r2, "-w", str(W), "-k", str(K), "-I", prg, r1],
                       capture_output=True, text=True, env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "pandora_genotyped.vcf").exists()
    # files that are not mates of each other
    r = subprocess.run([exe, "map", "-o", str(tmp_path / "odd"), "-g", str(G), "--mate", _write_fastq(tmp_path / "short.fq", side2[:-1]), "-w", str(W), "-k", str(K),
                        "-I", prg, r1], capture_output=True, text=True)
    assert r.returncode != 0 and "1200 and 1199" in r.stderr


def test_drprg_predict_mate_equals_the_run_on_the_cut_file(tmp_path):
    import json
    import re
    from util import vcf_without_date
    import os
    import subprocess
    from test_gpu_dedup import _write_fastq
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 9000, seed=1)
    block = bases.reshape(9000, 150)
    rng = np.random.default_rng(8)
    side1, side2 = [], []
    for s, row in enumerate(block):
        R = row.tobytes()
        if s % 3 == 0:  # an insert of 100 bases under reads of 150: both mates run into the adapter
            a, b = R[:100] + rng.choice(_ACGT, size=50).tobytes(), _revcomp(R[:100]) + rng.choice(_ACGT, size=50).tobytes()
        elif s % 3 == 1:  # mates of 110 bases over an insert of 150: 70 columns overlap
            a, b = R[:110], _revcomp(R[40:])
        else:  # mates that do not reach each other
            a, b = R[:75], _revcomp(R[76:])
        side1.append(a)
        side2.append(b)
    tables = [rule.shift_counts(rule.codes(a), rule.codes(b)) for a, b in zip(side1, side2)]
    for d in ("p", "c0", "c1"):
        (tmp_path / d).mkdir()
    r1, r2 = _write_fastq(tmp_path / "p" / "wt.fq", side1), _write_fastq(tmp_path / "p" / "wt_2.fq", side2)

    def run(fq, out, extra, env=None):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", fq, "-o", str(tmp_path / out), "-s", "wt", "-I", "-v"] + extra
        return subprocess.run(argv, capture_output=True, text=True, env=env)

    def report(out):
        """the run's outputs; the record IDs of the annotated VCF are random (as the reference's are), so they are excepted as
        tests/test_gpu_predict_e2e.py excepts them"""
        return (vcf_without_date(str(tmp_path / out / "pandora_genotyped.vcf")),
                re.sub(r'"vcfid": "[0-9a-f]{8}"', '"vcfid": "ID"', open(tmp_path / out / "wt.drprg.json").read()))

    reports = []
    for clip in (False, True):
        want = rule.run(side1, side2, 30, 50, clip, tables=tables)
        assert want[3]["pairs_read_through"] >= 3000 and want[3]["pairs_overlapping"] >= 6000
        cut = _write_fastq(tmp_path / f"c{int(clip)}" / "wt.fq", rule.cut_reads(side1, side2, want[1], want[2]))
        flags = ["--mate", r2] + (["--pair-clip-overlap"] if clip else [])
        a, b = run(r1, f"m{int(clip)}", flags + ["--qc-json", str(tmp_path / f"qc{int(clip)}.json")]), run(cut, f"k{int(clip)}", [])
        assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
        assert report(f"m{int(clip)}") == report(f"k{int(clip)}")
        assert _count_line(want[3]) in a.stderr and f"] reads={want[3]['reads']} " in a.stderr, a.stderr
        assert json.load(open(tmp_path / f"qc{int(clip)}.json"))["stages"]["pair_overlap"] == [want[3][k] for k in rule.COUNT_NAMES]
        behind = ["--dedup", "--subsample-covg", "0.05", "--seed", "3"]
        a, b = run(r1, f"ms{int(clip)}", flags + behind), run(cut, f"ks{int(clip)}", behind)
        assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
        assert report(f"ms{int(clip)}") == report(f"ks{int(clip)}")
        assert "subsample: reads_before=" in a.stderr and "reads_kept=" in a.stderr and [l for l in a.stderr.splitlines() if "subsample:" in l][0].split("] ")[1] == \
            [l for l in b.stderr.splitlines() if "subsample:" in l][0].split("] ")[1]
        reports.append(report(f"m{int(clip)}"))
    # a report without --mate has no entry of the stage
    q = run(str(tmp_path / "c0" / "wt.fq"), "q", ["--qc-json", str(tmp_path / "q.json")])
    assert q.returncode == 0 and "pair_overlap" not in json.load(open(tmp_path / "q.json"))["stages"]
    r = run(r1, "off", ["--mate", r2], env=dict(os.environ, DRPRG_HIP_KEEP_READS_GB="0"))
    assert r.returncode != 0 and "DRPRG_HIP_KEEP_READS_GB" in r.stderr and not (tmp_path / "off" / "wt.drprg.json").exists()


# ---- 7. bit-exactness across -t and the input form ----------------------------------------------------------------------------------------
def test_the_run_does_not_depend_on_threads_or_the_input_form(tmp_path):
    exe, prg, genes, side1, side2, r1, r2 = _pandora_files(tmp_path)
    want = rule.run(side1, side2, 30, 50, True)
    runs = []
    for name, threads, env in (("t1", 1, None), ("t4", 4, None), ("ascii", 2, dict(DRPRG_HIP_INPUT="ascii"))):
        stdout, vcf = _pandora(exe, tmp_path / name, prg, genes, r1, ["--mate", r2, "--pair-clip-overlap"], threads=threads, env=env)
        assert _count_line(want[3]) in stdout, (name, stdout)
        runs.append((vcf, [l for l in stdout.splitlines() if l.startswith("[pandora-hip] reads=")][0].split(" in ")[0]))
    assert runs[0] == runs[1] == runs[2]

