"""The decoy screen (drprg_hip_set_decoy, csrc/decoy_screen.hip; pytest -m gpu).  The set, V, H and the verdicts come from the rule in plain
Python (tests/decoy_rule.py), the vectors and counters from the oracle on the reads the rule keeps -- never from the code under test.

How the blocks come about: the ingest hands a worker's first block over at 750 000 bases, so the small sample (under that) is one block
and the big one several, whatever the number of parser threads."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import adapter_rule
import decoy_rule as rule
import read_trim_rule as rtrim
import resident_readback as rb
from dedup_rule import keep_flags_fast
from max_covg_rule import accepted_reads
from subsample_rule import keep_flags
from test_gpu_max_covg import _panel, _reads_of
from test_gpu_parity import _ctx, _oracle_index, _oracle_map
from test_gpu_read_filter import _assert_oracle, _file_of, _write_bam, _write_fastq
from util import vcf_without_date

pytestmark = pytest.mark.gpu

W, K = 11, 15  # the mapper's minimizers
DK = 31        # the screen's k-mers (the default)
G = 10_000
EINVAL, ENODATA, ENOENT = 22, 61, 2
TILE, LANE = 16384, 64  # starts per workgroup and per lane of decoy_screen_kernel
INFO_KEYS = ("reads_seen", "bases_seen", "reads_dropped", "bases_dropped", "valid", "hits")
NO_SCREEN = dict(kmers=0, slots=0, reads_seen=0, bases_seen=0, reads_dropped=0, bases_dropped=0, valid=0, hits=0)
OTHER = bytes.maketrans(b"ACGT", b"TGCA")


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _flat(reads):
    o = np.zeros(len(reads) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), o


def _fasta(path, records, gz=False, width=70):
    op = gzip.open if gz else open
    with op(path, "wb") as fh:
        for i, r in enumerate(records):
            fh.write(b">rec%d some text\n" % i)
            for p in range(0, len(r), width):
                fh.write(r[p:p + width] + b"\n")
    return str(path)


def _decoy_genome():
    return rule.random_dna(np.random.default_rng(71), 30_000)


def _counts(ctx):
    info = ctx.decoy_info()
    return {k: info[k] for k in INFO_KEYS}


def _filter_counts(ctx):
    info = ctx.read_filter_info()
    info.pop("T")
    return info


def _planted(decoy, other, k, V, H, at):
    """a read of V windows of which exactly the H that lie inside decoy[at : at + H + k - 1] are decoy windows: that stretch in the middle of
    bases of `other`, the two bases next to it set to differ from the decoy's own neighbours"""
    L, core = V + k - 1, H + k - 1
    left = (L - core) // 2
    r = bytearray(other[:left] + decoy[at:at + core] + other[left:L - core])
    if left:
        r[left - 1:left] = decoy[at - 1:at].translate(OTHER)
    if left + core < L:
        r[left + core:left + core + 1] = decoy[at + core:at + core + 1].translate(OTHER)
    return bytes(r)


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------------
def _check_table(ctx, records, paths, k, rng, what):
    D = rule.decoy_set(records, k)
    ctx.set_decoy(paths, k=k)
    info = ctx.decoy_info()
    assert info["kmers"] == len(D) and info["slots"] == rule.slots_for(rule.windows_of(records, k)), (what, info, len(D))
    members = sorted(D)
    both = members + [rule.revcomp_code(c, k) for c in members]
    assert ctx.decoy_lookup(both).tolist() == [1] * len(both), what
    out = []
    while len(out) < len(both):
        c = int(rng.integers(0, 1 << (2 * k)))
        if rule.canonical(c, k) not in D:
            out.append(c)
    assert ctx.decoy_lookup(out).tolist() == [0] * len(out), what
    return D


@pytest.mark.parametrize("k", [9, 15, 16, 31])
def test_the_table_holds_the_rules_set(tmp_path, k):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    rng = np.random.default_rng(100 + k)
    sizes = set()
    for n in list(range(1, 13)) + [4, 8, 12]:  # with the other three k: sixty tiny sets; 4, 8 and 12 k-mers fill 8, 16 and 32 slots to half
        rec = rule.random_dna(rng, k + n - 1)
        D = _check_table(ctx, [rec], [_fasta(tmp_path / f"tiny{n}.fa", [rec])], k, rng, ("tiny", n))
        sizes.add((len(D), ctx.decoy_info()["slots"]))
    assert {(4, 8), (8, 16), (12, 32)} <= sizes, sizes
    # a few thousand k-mers: lower case, letters that are no bases, a record shorter than k, several records and files, copies
    a, b, c = bytearray(rule.random_dna(rng, 2500)), rule.random_dna(rng, 1800), rule.random_dna(rng, k - 1)
    a[100:400] = bytes(a[100:400]).lower()
    a[1000:1001] = b"N"
    a[1500:1503] = b"RYn"
    recs1, recs2 = [bytes(a), c, b], [rule.revcomp(b), bytes(a[:700]), b""]
    D = _check_table(ctx, recs1 + recs2, [_fasta(tmp_path / "one.fa", recs1), _fasta(tmp_path / "two.fa.gz", recs2, gz=True)], k, rng, "large")
    assert 3000 < len(D) < 4300 and rule.windows_of(recs1 + recs2, k) > len(D) + 2000
    ctx.close()


# ---- 2. the kernel against the rule, on device buffers ------------------------------------------------------------------------------------------
_BATCH = {}


def _ragged(k=DK):
    """about 100 kb over six tiles of 16 384 starts: runs of empty reads at the start, at the end and on a tile edge; lengths 0, 1, k - 1, k,
    k + 1; a read over three tiles; reads that end on a lane edge and on a tile edge; then the reads with a letter that is no base, and the
    reads planted at the boundaries of the settings the test runs"""
    if k in _BATCH:
        return _BATCH[k]
    L = [0, 0, 0, 1, k - 1, k, k + 1, TILE - 2 - 3 * k, 16400, 1, 16368, 0, 0, 0, 16383, 1, 16384, 10 * LANE, 16385 - 10 * LANE, 16, 0, 0]
    o = np.concatenate([[0], np.cumsum(L)])
    assert o[8] == TILE - 1 and o[9] == 2 * TILE + 15 and o[11] == o[14] == 3 * TILE and o[16] == 4 * TILE and o[17] == 5 * TILE  # three tiles; tile edges
    assert o[18] % LANE == 0 and o[18] % TILE != 0  # a lane edge inside a tile
    rng = np.random.default_rng(72)
    decoy, (_, genomes) = _decoy_genome(), _panel()
    hap = bytes(genomes.haps[0]) * 2
    reads = []
    for i, n in enumerate(L):
        s = int(rng.integers(0, len(decoy) - n + 1)) if n <= len(decoy) else 0
        kind = i % 4  # decoy, its reverse complement, panel, half and half
        reads.append(decoy[s:s + n] if kind == 0 else rule.revcomp(decoy[s:s + n]) if kind == 1 else hap[s:s + n] if kind == 2 else decoy[s:s + n // 2] + hap[s:s + n - n // 2])
    # a letter that is no base: at the first position of a window, at its last, and in the last window of a read; lower case
    for at in (0, k - 1, 149, 150 - k, 70):
        r = bytearray(decoy[500:650])
        r[at:at + 1] = b"N"
        reads.append(bytes(r))
    reads.append(decoy[700:900].lower())
    # the boundaries: 1000 H - f V == 0 and one hit fewer, for f = 500, 1000 and 1; and M = 3 where f = 1 asks for one hit only
    planted = [(100, 50), (100, 49), (80, 80), (80, 79), (1000, 1), (1001, 1), (1000, 3), (1000, 2), (3000, 3), (3001, 3)]
    reads += [_planted(decoy, hap[3000:], k, V, H, 1000 + 300 * j) for j, (V, H) in enumerate(planted)]
    reads += [b"", b""]
    D = rule.decoy_set([decoy], k)
    vh = [(V, H) for V, H, _ in rule.verdicts(reads, D, k)]
    assert vh[-12:-2] == planted, vh[-12:-2]
    assert vh[4] == (0, 0) and vh[5][0] == 1 and vh[6][0] == 2 and vh[8][0] == 16400 - k + 1 and vh[0] == vh[3] == (0, 0)
    for j, at in enumerate((0, k - 1, 149, 150 - k, 70)):  # the windows that hold the letter are gone from V and from H
        lost = min(at, 150 - k) - max(0, at - k + 1) + 1
        assert vh[len(L) + j] == (151 - k - lost, 151 - k - lost), (at, vh[len(L) + j])
    assert vh[len(L) + 5] == (200 - k + 1, 200 - k + 1)
    _BATCH[k] = dict(reads=reads, vh=vh, decoy=decoy)
    return _BATCH[k]


def _device_screen(ctx, torch, reads, form, want_counts=True):
    text, offs = _flat(reads)
    n_reads, n_bases = len(reads), int(offs[-1])
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_v = torch.full((n_reads,), -7, dtype=torch.int32, device="cuda")  # (stale on purpose)
    d_h = torch.full((n_reads,), -7, dtype=torch.int32, device="cuda")
    d_f = torch.full((n_reads,), 7, dtype=torch.uint8, device="cuda")
    pv, ph = (d_v.data_ptr(), d_h.data_ptr()) if want_counts else (None, None)
    if form == "packed":
        words, npos = adapter_rule.packed_form(text.tobytes())
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_n = torch.from_numpy(npos.astype(np.int64)).cuda() if npos.size else None
        out = ctx.decoy_screen_device(None, d_w.data_ptr(), d_n.data_ptr() if npos.size else None, int(npos.size), d_o.data_ptr(), n_reads, n_bases, pv, ph, d_f.data_ptr())
    else:
        shift = 1 if form == "text off by one" else 0
        buf = np.zeros(n_bases + (1 if shift else 64), dtype=np.uint8)  # (one byte off: read byte by byte, and the buffer ends with its last base)
        buf[shift:shift + n_bases] = text
        d_t = torch.from_numpy(buf).cuda()
        assert d_t.data_ptr() % 16 == 0
        out = ctx.decoy_screen_device(d_t.data_ptr() + shift, None, None, 0, d_o.data_ptr(), n_reads, n_bases, pv, ph, d_f.data_ptr())
    torch.cuda.synchronize()
    return out, list(zip(d_v.cpu().numpy().tolist(), d_h.cpu().numpy().tolist())), d_f.cpu().numpy().tolist()


@pytest.mark.parametrize("form", ["text", "text off by one", "packed"])
@pytest.mark.parametrize("f,M", [(500, 1), (1000, 1), (1, 1), (1, 3), (500, 3)])
def test_the_kernels_equal_the_rule(tmp_path, form, f, M):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    b = _ragged()
    ctx.set_decoy([_fasta(tmp_path / "decoy.fa", [b["decoy"]])], k=DK, min_frac=f / 1000, min_kmers=M)
    keep = [not rule.drops(V, H, f, M) for V, H in b["vh"]]
    # on the CPU first: a read on the boundary that is dropped, and one a single hit short of it that is kept
    assert any(H >= M and 1000 * H == f * V for V, H in b["vh"])
    assert any(k and H >= M and 1000 * (H + 1) >= f * V for k, (V, H) in zip(keep, b["vh"])) and 5 < sum(keep) < len(keep) - 5
    if M == 3:
        assert (1000, 2) in b["vh"] and (1000, 3) in b["vh"] and rule.drops(1000, 3, f, M) == (f == 1) and not rule.drops(1000, 2, f, M)

    def check(reads, vh, keep, what):
        out, got, flags = _device_screen(ctx, torch, reads, form)
        diff = [i for i in range(len(reads)) if got[i] != vh[i]]
        assert not diff, (what, [(i, len(reads[i]), got[i], vh[i]) for i in diff[:8]])
        assert flags == [int(x) for x in keep], (what, [i for i in range(len(reads)) if flags[i] != int(keep[i])][:8])
        assert out == (len(keep) - sum(keep), sum(len(r) for r, x in zip(reads, keep) if not x), sum(V for V, _ in vh), sum(H for _, H in vh)), (what, out)

    check(b["reads"], b["vh"], keep, "ragged")
    # a second, smaller launch on the same context: nothing of the first one is left behind; V and H need not be asked for
    d = b["decoy"]
    small = [b"", d[:DK], b"", d[100:100 + DK - 1], rule.revcomp(d[200:260]), b"ACGT" * 20]
    vh2 = [(0, 0), (1, 1), (0, 0), (0, 0), (30, 30), (50, 0)]
    check(small, vh2, [not rule.drops(V, H, f, M) for V, H in vh2], "small")
    out, _, flags = _device_screen(ctx, torch, small, form, want_counts=False)
    assert flags == [int(not rule.drops(V, H, f, M)) for V, H in vh2] and out[2:] == (81, 31)
    # offsets that do not ascend to n_bases
    text, offs = _flat(small)
    d_t, d_f = torch.from_numpy(np.concatenate([text, np.zeros(64, np.uint8)])).cuda(), torch.zeros(len(small), dtype=torch.uint8, device="cuda")
    for bad in (offs + 1, np.concatenate([offs[:-1], [offs[-1] - 1]]), offs[::-1].copy()):
        d_o = torch.from_numpy(bad.astype(np.int64)).cuda()
        with pytest.raises(DependencyError) as e:
            ctx.decoy_screen_device(d_t.data_ptr(), None, None, 0, d_o.data_ptr(), len(small), int(offs[-1]), None, None, d_f.data_ptr())
        assert e.value.code == EINVAL
    ctx.close()


# ---- 3. a contaminated sample equals the sample of its kept reads ------------------------------------------------------------------------------
_SAMPLES = {}


def _sample(which, oracle, ctx):
    """panel reads, decoy reads and chimeras cut to the boundary, in random order, a letter that is no base in every tenth read; the rule's
    verdicts and the oracle's vectors of the kept reads: made once, shared, left unchanged"""
    if which not in _SAMPLES:
        _, genomes = _panel()
        decoy = _decoy_genome()
        rng = np.random.default_rng(73 if which == "small" else 74)
        n_short, n_long = (350, 80) if which == "small" else (1000, 250)
        lengths = np.concatenate([rng.integers(150, 401, size=n_short), rng.integers(3000, 9001, size=n_long)])
        rng.shuffle(lengths)
        lengths[3::50] = rng.integers(0, 40, size=len(lengths[3::50]))  # a few reads of under k bases, some of none
        pb, po = _reads_of(genomes, [int(x) for x in lengths], seed=75)
        reads, kinds = [], []
        for i, L in enumerate(int(x) for x in lengths):
            r = pb[int(po[i]):int(po[i + 1])].tobytes()
            kind = ("panel", "panel", "decoy", "panel", "chimera")[i % 5] if L >= 2 * DK else "panel"
            if kind == "decoy":
                s = int(rng.integers(0, len(decoy) - L + 1))
                r = decoy[s:s + L] if rng.random() < 0.5 else rule.revcomp(decoy[s:s + L])
            elif kind == "chimera":  # half of the windows, or one fewer, from the decoy
                V = L - DK + 1
                r = _planted(decoy, r, DK, V, (V + 1) // 2 - (i // 5) % 2, int(rng.integers(1, len(decoy) - L - 1)))
            if i % 10 == 0 and L > 40:  # packed blocks list positions
                r = r[:7] + b"N" + r[8:]
            reads.append(r)
            kinds.append(kind)
        D = rule.decoy_set([decoy], DK)
        census, keep = rule.census(reads, [True] * len(reads), D, DK)
        vh = rule.verdicts(reads, D, DK)
        assert all(not k for k, kind in zip(keep, kinds) if kind == "decoy") and all(k for k, kind in zip(keep, kinds) if kind == "panel")
        chim = [(V, H, k) for (V, H, k), kind in zip(vh, kinds) if kind == "chimera"]
        assert any(1000 * H == 500 * V and not k for V, H, k in chim) and any(1000 * (H + 1) >= 500 * V > 1000 * H and k for V, H, k in chim)
        assert sum(k for _, _, k in chim) > len(chim) // 4 and sum(not k for _, _, k in chim) > len(chim) // 4
        kept = [r for r, k in zip(reads, keep) if k]
        b, o = _flat(reads)
        kb, ko = _flat(kept)
        s = dict(reads=reads, bases=b, offs=o, quals=[np.full(len(r), 30, dtype=np.uint8) for r in reads], keep=keep, census=census, kept=kept, kbases=kb, koffs=ko,
                 klengths=[len(r) for r in kept], decoy=decoy, D=D)
        s["want"] = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
        assert s["want"][2]["clusters_kept"] > 5
        _SAMPLES[which] = s
    return _SAMPLES[which]


def _assert_screened(ctx, s, what, calls=1):
    n, nb = len(s["reads"]), int(s["offs"][-1])
    nk, nkb = len(s["kept"]), int(s["koffs"][-1])
    if calls == 1:
        _assert_oracle(ctx, s["want"], nk, nkb, what)
    assert _counts(ctx) == {k: calls * v for k, v in s["census"].items()}, (what, _counts(ctx), s["census"])
    assert ctx.decoy_info()["kmers"] == len(s["D"]), what
    # seen = short + long + low quality + decoy + kept
    assert _filter_counts(ctx) == dict(reads_seen=calls * n, bases_seen=calls * nb, dropped_short=0, dropped_long=0, dropped_low_qual=0, reads_kept=calls * nk,
                                       bases_kept=calls * nkb), what


def _fasta_reads(path, reads):
    with open(path, "wb") as fh:
        for i, r in enumerate(reads):
            fh.write(b">r%d\n" % i + r + b"\n")
    return str(path)


FORMS = ["fastq ascii", "fastq packed", "bam", "fastq.gz", "fasta"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["small", "big"])
def test_a_contaminated_sample_equals_the_sample_of_its_kept_reads(tmp_path, oracle, which, form):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample(which, oracle, ctx)
    path = _fasta_reads(tmp_path / "all.fa", s["reads"]) if form == "fasta" else _file_of(tmp_path, form, s["bases"], s["offs"], s["quals"], "all")
    ctx.set_decoy([_fasta(tmp_path / "decoy.fa", [s["decoy"][:17_000]]), _fasta(tmp_path / "decoy2.fa.gz", [s["decoy"][16_000:]], gz=True)])
    for packed in ((True,) if form == "fastq packed" else (False,) if form == "fastq ascii" else (False, True)):
        ctx.reset()
        ctx.set_threads(1 if which == "small" else 4)
        ctx.set_input_format(packed)
        ctx.keep_reads(1 << 28)
        ctx.map_fastx(path)
        _assert_screened(ctx, s, (which, form, packed))
        info = ctx.resident_info()
        assert info["complete"] and (info["blocks"] == 1 if which == "small" else info["blocks"] >= 2), info
        if which == "small":  # the resident block is the block of the kept reads, byte for byte
            rb.assert_resident(ctx, s["kept"], packed or form == "bam", (form, packed))
    if form == "fastq ascii":  # a context given the file of the kept reads alone, with no decoy set
        ctx.set_decoy([])
        ctx.reset()
        ctx.map_fastx(_write_fastq(tmp_path / "kept.fq", s["kbases"], s["koffs"], [np.full(L, 30, dtype=np.uint8) for L in s["klengths"]]))
        _assert_oracle(ctx, s["want"], len(s["kept"]), int(s["koffs"][-1]), "the kept reads' own file")
        assert ctx.decoy_info() == NO_SCREEN and _filter_counts(ctx)["reads_seen"] == 0
    ctx.close()


def test_the_screen_runs_behind_trimming_adapters_and_the_filter(tmp_path, oracle):
    """every stage on: the crops and the adapter cut first, the length bound next, the screen on what those left.  A read whose decoy tail the
    tail crop removes is kept; the same read uncropped would be dropped."""
    panel, genomes = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    k, f, FRONT, TAIL, MIN_LEN, ADAPTER = 15, 300, 5, 60, 50, adapter_rule.TRUSEQ[:33]
    D = rule.decoy_set([s["decoy"]], k)
    body, _ = _reads_of(genomes, [70, 200, 200], seed=76)
    body = body.tobytes()
    tailed = body[:70] + s["decoy"][2000:2060]
    through = body[70:270] + ADAPTER.encode() + s["decoy"][3000:3200]  # behind the adapter: decoy bases that are cut off with it
    short = s["decoy"][4000:4000 + FRONT + TAIL + MIN_LEN - 1]         # decoy, but too short once cropped: the length bound takes it first
    reads = [r for r in s["reads"] if len(r) < 1000] + [tailed, through, short]
    ranges = [rtrim.kept_range(None, len(r), FRONT, TAIL) for r in reads]
    cut, ainfo = adapter_rule.cut_ranges(reads, ranges, [ADAPTER], 100, 3)
    left = [r[a:b] for r, (a, b) in zip(reads, cut)]
    judged = [len(r) >= MIN_LEN for r in left]
    census, keep = rule.census(left, judged, D, k, f)
    V, H = rule.counts(tailed, D, k)
    assert rule.drops(V, H, f) and keep[-3] and cut[-3][0] == FRONT and cut[-3][1] <= 70 and rule.counts(left[-3], D, k)[1] == 0
    assert cut[-2] == (5, 200) and keep[-2] and not judged[-1] and census["reads_dropped"] > 50 and sum(keep) > 100
    kb, ko = _flat([r for r, x in zip(left, keep) if x])
    want = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), kb, ko, W, K, True, threads=4)
    b, o = _flat(reads)
    quals = [np.full(len(r), 30, dtype=np.uint8) for r in reads]
    ctx.set_decoy([_fasta(tmp_path / "decoy.fa", [s["decoy"]])], k=k, min_frac="0.3")
    ctx.set_read_trim(front=FRONT, tail=TAIL)
    ctx.set_adapters([ADAPTER])
    ctx.set_read_filter(min_len=MIN_LEN)
    for form in ("fastq ascii", "fastq packed", "bam"):
        ctx.reset()
        ctx.set_threads(2)
        ctx.set_input_format(form == "fastq packed")
        ctx.map_fastx(_file_of(tmp_path, form, b, o, quals, "stages"))
        _assert_oracle(ctx, want, sum(keep), int(ko[-1]), form)
        assert _counts(ctx) == census, (form, _counts(ctx), census)
        assert ctx.adapter_trim_info() == ainfo
        assert _filter_counts(ctx) == dict(reads_seen=len(reads), bases_seen=sum(len(r) for r in left), dropped_short=len(reads) - sum(judged), dropped_long=0,
                                           dropped_low_qual=0, reads_kept=sum(keep), bases_kept=int(ko[-1])), form
    ctx.close()


def test_dedup_subsample_and_the_cap_see_the_kept_reads(tmp_path, oracle):
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, ctx)
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    # every read twice: the copies of the dropped reads never arrive, those of the kept ones are numbered among the kept
    reads = s["reads"] + s["reads"][:400]
    keep = s["keep"] + s["keep"][:400]
    kept = [r for r, x in zip(reads, keep) if x]
    b, o = _flat(reads)
    fq = _write_fastq(tmp_path / "twice.fq", b, o, [np.full(len(r), 30, dtype=np.uint8) for r in reads])
    ctx.set_decoy([_fasta(tmp_path / "decoy.fa", [s["decoy"]])])
    ctx.set_threads(4)
    ctx.set_ordered_ingest(True)
    ctx.keep_reads(1 << 28)
    ctx.map_fastx(fq)
    flags = keep_flags_fast(kept)
    assert sum(flags) < len(kept) - 100
    out = ctx.dedup()
    assert out["reads_before"] == len(kept) and out["bases_before"] == sum(len(r) for r in kept) and out["reads_kept"] == sum(flags), out
    assert ctx.dedup_flags(len(kept)).tolist() == flags
    left = [len(r) for r, x in zip(kept, flags) if x]
    total = sum(left)
    sub = keep_flags(left, total // 2, 9)
    out = ctx.subsample(total // 2, 9)
    assert out["reads_before"] == len(left) and out["bases_before"] == total and out["reads_kept"] == sum(sub), out
    assert ctx.subsample_flags(len(left)).tolist() == sub
    # the cap counts kept bases only: in the first block, and in a later one
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    for max_covg, packed in ((3, True), (99, False)):
        n, n_bases, reached = accepted_reads(s["klengths"], G, max_covg)
        assert reached and 0 < n < len(s["klengths"]) and (max_covg == 3 or n_bases > 800_000)
        want = _oracle_map(oracle, idx, s["kbases"][:n_bases], s["koffs"][:n + 1], W, K, True, threads=4)
        ctx.reset()
        ctx.keep_reads(0)
        ctx.set_input_format(packed)
        ctx.set_max_covg(max_covg)
        ctx.map_fastx(fq)
        info = ctx.max_covg_info()
        assert info["reached"] and info["reads"] == n and info["bases"] == n_bases, (max_covg, info)
        _assert_oracle(ctx, want, n, n_bases, ("cap", max_covg, packed))
    ctx.close()


def test_two_devices_give_the_vectors_of_one(tmp_path, oracle):
    """the table is built on every device of the context, and each block is screened on the device that takes it"""
    from drprg_amd import Context
    panel, _ = _panel()
    one = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("big", oracle, one)
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    decoy = _fasta(tmp_path / "decoy.fa", [s["decoy"]])
    multi = Context(str(tmp_path / "dr.prg"), W, K, from_files=False, devices=[0, 0])
    multi.set_opts(illumina=True, genome_size=G)
    for c in (one, multi):
        c.set_threads(4)
        c.set_decoy([decoy])
        c.map_fastx(fq)
        _assert_screened(c, s, "devices")
    one.close()
    multi.close()


# ---- 4. refusals and state ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(tmp_path, oracle):
    import torch
    from drprg_amd.pandora import DependencyError
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    n = len(s["reads"])
    fq = _write_fastq(tmp_path / "all.fq", s["bases"], s["offs"], s["quals"])
    decoy = _fasta(tmp_path / "decoy.fa", [s["decoy"]])
    ctx.set_threads(2)
    full = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), s["bases"], s["offs"], W, K, True, threads=4)
    # every refusal of the settings entry leaves the context without a set
    nothing = _fasta(tmp_path / "short.fa", [s["decoy"][:DK - 1], b"N" * 100])
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    for bad, code in ((dict(fasta_paths=[decoy] * 9), EINVAL), (dict(fasta_paths=[decoy], k=8), EINVAL), (dict(fasta_paths=[decoy], k=32), EINVAL),
                      (dict(fasta_paths=[nothing]), EINVAL), (dict(fasta_paths=[decoy, str(tmp_path / "missing.fa")]), ENOENT)):
        ctx.set_decoy([decoy])
        with pytest.raises(DependencyError) as e:
            ctx.set_decoy(**bad)
        assert e.value.code == code, bad
        assert ctx.decoy_info() == NO_SCREEN, bad
        for call in (lambda: ctx.decoy_lookup([1, 2]), lambda: ctx.decoy_screen_device(d.data_ptr(), None, None, 0, d.data_ptr(), 1, 0, None, None, d.data_ptr())):
            with pytest.raises(DependencyError) as e:
                call()
            assert e.value.code == EINVAL
    import ctypes as C
    from drprg_amd._lib import lib
    one = (C.c_char_p * 1)(decoy.encode())
    assert lib.drprg_hip_set_decoy(ctx._h, None, 1, 0, 0, 0) == -EINVAL and lib.drprg_hip_set_decoy(ctx._h, one, 1, 0, 1001, 0) == -EINVAL
    assert lib.drprg_hip_set_decoy(ctx._h, (C.c_char_p * 2)(decoy.encode(), None), 2, 0, 0, 0) == -EINVAL and ctx.decoy_info() == NO_SCREEN
    with pytest.raises(ValueError):
        ctx.set_decoy([decoy], min_frac="0.1234")
    ctx.map_fastx(fq)  # the context still maps, with no set: every read
    _assert_oracle(ctx, full, n, int(s["offs"][-1]), "nothing set")
    assert ctx.decoy_info() == NO_SCREEN and _filter_counts(ctx)["reads_seen"] == 0
    # map_host and map_device would map the reads unscreened: refused while a set is loaded
    ctx.set_decoy([decoy])
    ctx.reset()
    d_b, d_o = torch.from_numpy(s["kbases"].copy()).cuda(), torch.from_numpy(s["koffs"].astype(np.int64)).cuda()
    for call in (lambda: ctx.map_host(s["kbases"], s["koffs"]), lambda: ctx.map_device(d_b.data_ptr(), d_o.data_ptr(), len(s["kept"]), int(s["koffs"][-1]))):
        with pytest.raises(DependencyError) as e:
            call()
        assert e.value.code == EINVAL and "drprg_hip_set_decoy" in str(e.value)
    assert ctx.counters()["reads"] == 0
    ctx.map_fastx(fq)
    _assert_screened(ctx, s, "after the refusals")
    # discover without resident reads after the screen dropped one: -61
    (tmp_path / "disc").mkdir()
    with pytest.raises(DependencyError) as e:
        ctx.discover_reads(fq, str(tmp_path / "genes.fa"), str(tmp_path / "disc"))
    assert e.value.code == ENODATA and "decoy" in str(e.value)
    # a second call adds to the counts; a reset clears them and keeps the set
    ctx.map_fastx(fq)
    _assert_screened(ctx, s, "two calls", calls=2)
    ctx.reset()
    assert _counts(ctx) == dict.fromkeys(INFO_KEYS, 0) and ctx.decoy_info()["kmers"] == len(s["D"])
    ctx.map_fastx(fq)
    _assert_screened(ctx, s, "after a reset")
    # cleared: map_host is served again, and the file maps with every read
    ctx.set_decoy([])
    ctx.reset()
    ctx.map_host(s["kbases"], s["koffs"])
    _assert_oracle(ctx, s["want"], len(s["kept"]), int(s["koffs"][-1]), "map_host, nothing set")
    ctx.reset()
    ctx.map_fastx(fq)
    _assert_oracle(ctx, full, n, int(s["offs"][-1]), "cleared")
    assert ctx.decoy_info() == NO_SCREEN
    ctx.close()


# ---- 5. the executables ---------------------------------------------------------------------------------------------------------------------
def _verbose_line(s):
    c = s["census"]
    return f"decoy screen: kmers={len(s['D'])} " + " ".join(f"{key}={c[key]}" for key in INFO_KEYS[:4])


def test_pandora_map_writes_the_vcf_of_the_kept_reads(tmp_path, oracle):
    from drprg_amd._lib import PANDORA_EXE
    panel, _ = _panel()
    ctx = _ctx(tmp_path, panel, W, K, True, genome_size=G)
    s = _sample("small", oracle, ctx)
    ctx.close()
    prg, genes = str(tmp_path / "dr.prg"), str(tmp_path / "genes.fa")
    r = subprocess.run([PANDORA_EXE, "index", "-t", "2", "-w", str(W), "-k", str(K), prg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bam = _write_bam(tmp_path / "all.bam", s["bases"], s["offs"], s["quals"])
    kept_fq = _write_fastq(tmp_path / "kept.fq", s["kbases"], s["koffs"], [np.full(L, 30, dtype=np.uint8) for L in s["klengths"]])
    decoy = _fasta(tmp_path / "decoy.fa", [s["decoy"]])

    def run(out, reads, extra):
        argv = [PANDORA_EXE, "map", "--genotype", "--local", "--gt-conf", "0", "-v", "-o", str(out), "-g", str(G), "--max-covg", "4294967295"] + extra + [
            "--vcf-refs", genes, "-t", "2", "-w", str(W), "-k", str(K), "-c", "10", "-I", prg, reads]
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout

    stdout = run(tmp_path / "screened", bam, ["--decoy", decoy, "--decoy-k", str(DK), "--decoy-min-frac", "0.5", "--decoy-min-kmers", "1"])
    run(tmp_path / "kept", kept_fq, [])
    assert vcf_without_date(str(tmp_path / "screened" / "pandora_genotyped.vcf")) == vcf_without_date(str(tmp_path / "kept" / "pandora_genotyped.vcf"))
    assert _verbose_line(s) in stdout and "read filter:" not in stdout, stdout
    assert f"reads={len(s['kept'])} bases={int(s['koffs'][-1])} " in stdout, stdout


def test_drprg_predict_takes_the_same_flags(tmp_path):
    from test_gpu_predict_e2e import BIN, _make_index, _reads
    idx, panel, sites = _make_index(tmp_path)
    bases, offs = _reads(panel, lambda g, i: 0, 6000, seed=1)
    decoy = _decoy_genome()
    rng = np.random.default_rng(77)
    reads = []
    for i in range(len(offs) - 1):
        reads.append(bases[int(offs[i]):int(offs[i + 1])].tobytes())
        if i % 8 == 0:
            at = int(rng.integers(0, len(decoy) - 150))
            reads.append(decoy[at:at + 150])
    D = rule.decoy_set([decoy], DK)
    census, keep = rule.census(reads, [True] * len(reads), D, DK)
    assert census["reads_dropped"] == 750 and census["hits"] == 750 * 120
    b, o = _flat(reads)
    fq = _write_fastq(tmp_path / "wt.fq", b, o, [np.full(len(r), 30, dtype=np.uint8) for r in reads])
    kept = [r for r, x in zip(reads, keep) if x]
    kb, ko = _flat(kept)
    kept_fq = _write_fastq(tmp_path / "kept.fq", kb, ko, [np.full(len(r), 30, dtype=np.uint8) for r in kept])

    def run(out, path, extra):
        argv = [os.path.join(BIN, "drprg"), "predict", "-x", str(idx), "-i", path, "-o", str(out), "-s", "wt", "-I", "-v"] + extra
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        calls = json.load(open(out / "wt.drprg.json"))["susceptibility"]
        for drug in calls.values():
            for ev in drug["evidence"]:
                ev.pop("vcfid")  # (a fresh identifier per run)
        return r.stderr, (open(out / "pandora_genotyped.vcf").read(), calls)

    err, got = run(tmp_path / "screened", fq, ["--decoy", _fasta(tmp_path / "decoy.fa", [decoy])])
    _, want = run(tmp_path / "kept", kept_fq, [])
    assert got == want
    assert f"decoy screen: kmers={len(D)} " + " ".join(f"{key}={census[key]}" for key in INFO_KEYS[:4]) in err, err
    assert f"] reads={len(kept)} " in err
