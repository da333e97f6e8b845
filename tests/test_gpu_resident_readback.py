"""The resident sample read back byte for byte after every compaction (pytest -m gpu).  drprg_hip_select_reads with the four one-base anchors
returns every resident read that holds an ACGT base: what ss_pack_kernel, gather_reads_kernel, ss_npos_kernel / trim_npos_kernel and
bam_pack_kernel wrote, and where the depth cap cut, compared exactly -- there is no tolerance anywhere -- with the rule modules composed
(tests/resident_readback.py).  The census of every batch used here is taken on the CPU in tests/test_resident_readback.py.

Reading a failure: (a) holds the observer itself to the file with no stage set.  If a later test fails while (a) passes, the fault is in a
compaction, not in select_reads or the unpacking; the message names the read, its length, its source and destination phase mod 16 and the
first differing position.

How the reads get resident: one small file = one block (every file here stays below the 750 000 bases at which the ingest hands a block
over), one parser thread, ordered hand-over; keep_reads comes first in every context."""
import numpy as np
import pytest

import bam_writer
import read_trim_rule
import resident_readback as rb
from resident_readback import assert_resident, pipeline
from test_gpu_max_covg import _panel
from test_gpu_parity import _ctx, _oracle_index, _oracle_map

pytestmark = pytest.mark.gpu

W, K = 11, 15
G = 10_000
TEXT_AND_PACKED = ["fastq packed", "fastq ascii"]
INGEST_FORMS = ["fastq packed", "fastq ascii", "bam"]


def _open(tmp_path, panel=None):
    ctx = _ctx(tmp_path, panel or _panel()[0], W, K, True, genome_size=G)
    ctx.keep_reads(1 << 28)
    ctx.set_threads(1)
    ctx.set_ordered_ingest(1)
    return ctx


def _ingest(ctx, tmp_path, tag, form, b, reads=None):
    """a fresh sample: the batch's blocks as files of that form, each through map_fastx"""
    files = rb.write_blocks(tmp_path, tag, form, b.reads if reads is None else reads, b.quals, b.rev, b.cuts)
    ctx.reset()
    ctx.set_input_format(form == "fastq packed")
    for f in files:
        ctx.map_fastx(f)


def _check(ctx, stage, form, what, n_blocks):
    alive = stage.alive
    assert_resident(ctx, rb.as_form([a.seq for a in alive], form), rb.is_packed(form), (what, form, stage.name), blocks=rb.block_counts(alive, n_blocks),
                    src=[a.src for a in alive])


def _step(ctx, step, stage, form, what, n_blocks):
    """one resident step: the four numbers and the flags against the pipeline's stage, then the read-back"""
    n_before = len(stage.flags)
    out = ctx.dedup(step[1]) if step[0] == "dedup" else ctx.subsample(step[1], step[2])
    kept = [a.seq for a in stage.alive]
    assert out["reads_before"] == n_before and out["reads_kept"] == len(kept) and out["bases_kept"] == sum(len(s) for s in kept), (what, form, step, out)
    flags = ctx.dedup_flags(n_before) if step[0] == "dedup" else ctx.subsample_flags(n_before)
    assert flags.tolist() == stage.flags, (what, form, step, np.flatnonzero(flags != np.array(stage.flags))[:8])
    _check(ctx, stage, form, what, n_blocks)


# ---- a. the observer itself -------------------------------------------------------------------------------------------------------------------
def _observer_batch():
    """three blocks of 200 reads.  The first sixteen reads hold 48 bases each -- so each starts on a word edge of its block -- and read c holds
    the letter of BAM's 4-bit code c, '=' among them, at its first base, either side of a word edge, and its last base ('=' stands as n in
    the text forms).  The rest: 0 to 200 bases with lower case, IUPAC letters and N"""
    rng = np.random.default_rng(2)
    reads = []
    for c in range(16):
        r = bytearray(rb._random_read(rng, 48))
        for p in (0, 15, 16, 31, 47):
            r[p] = ord(bam_writer.CODES[c])
        reads.append(bytes(r))
    for i in range(16, 600):
        reads.append(rb.sprinkle(rng, rb._random_read(rng, int(rng.integers(0, 201))), 0.05))
    reads[300], reads[301], reads[599] = b"", b"NNNN", b"acgtn"
    return rb.Batch(reads, None, rb.reverse_flags(600), [0, 200, 400, 600], {})


def test_a_the_read_back_of_an_untouched_sample_is_the_file(tmp_path):
    b = _observer_batch()
    ctx = _open(tmp_path)
    for form in rb.FORMS:
        reads = b.reads if form == "bam" else [r.replace(b"=", b"n") for r in b.reads]
        _ingest(ctx, tmp_path, form.replace(" ", "_"), form, b, reads)
        if form == "bam":
            info = ctx.bam_info()
            assert info["records"] == 600 and info["reversed"] == 200, info
            assert b"=" in rb.as_form(reads, form)[0] and set(bam_writer.CODES.encode()) <= set(b"".join(rb.as_form(reads[:16], form)))
        else:
            assert any(c in b"acgt" for c in b"".join(reads)) and any(c in rb.IUPAC for c in b"".join(reads))
        assert_resident(ctx, rb.as_form(reads, form), rb.is_packed(form), ("observer", form), blocks=[200, 200, 200])
    ctx.close()


# ---- b. each stage alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TEXT_AND_PACKED)
def test_b_subsample_alone(tmp_path, form):
    b = rb.edge_batch()
    step = ("subsample", b.notes["T"], b.notes["seed"])
    st = pipeline(b.reads, None, b.rev, dict(cuts=b.cuts, steps=[step]))
    ctx = _open(tmp_path, b.notes["panel"])
    _ingest(ctx, tmp_path, "edge", form, b)
    _check(ctx, st[2], form, "before the subsample", 3)
    _step(ctx, step, st[3], form, "subsample", 3)
    ctx.close()


@pytest.mark.parametrize("form", TEXT_AND_PACKED)
def test_b_dedup_alone(tmp_path, form):
    b = rb.dedup_batch()
    st = pipeline(b.reads, None, b.rev, dict(cuts=b.cuts, steps=[("dedup", 64)]))
    ctx = _open(tmp_path)
    _ingest(ctx, tmp_path, "dup", form, b)
    _check(ctx, st[2], form, "before the dedup", 4)
    _step(ctx, ("dedup", 64), st[3], form, "dedup", 4)
    ctx.close()


@pytest.mark.parametrize("form", INGEST_FORMS)
def test_b_read_filter_alone(tmp_path, form):
    b = rb.filter_batch()
    st = pipeline(b.reads, b.quals, b.rev, dict(rb.FILTER_SETTINGS, cuts=b.cuts))
    ctx = _open(tmp_path, b.notes["panel"])
    ctx.set_read_filter(**rb.FILTER_SETTINGS)
    _ingest(ctx, tmp_path, "filter", form, b)
    info = ctx.read_filter_info()
    assert info["reads_seen"] == len(b.reads) and info["reads_kept"] == len(st[1].alive), info
    _check(ctx, st[1], form, "read filter", 3)
    ctx.close()


@pytest.mark.parametrize("form", INGEST_FORMS)
@pytest.mark.parametrize("name", list(rb.TRIM_SETTINGS))
def test_b_read_trim_alone(tmp_path, name, form):
    b = rb.trim_batch()
    kw = rb.TRIM_SETTINGS[name]
    st = pipeline(b.reads, b.quals, b.rev, dict(kw, cuts=b.cuts))
    if form == "bam":
        # the kept range of a reverse-strand record is the mirror of the stored one: the rule on the stored qualities, front and tail swapped
        i = next(i for i, (a, _, t) in enumerate(b.notes["spec"]) if b.rev[i] and a != t and len(st[0].alive[i].seq) > 0)
        L, milli = len(b.reads[i]), read_trim_rule.qual_milli(kw.get("trim_qual", 0))
        sa, sb = read_trim_rule.kept_range(b.quals[i][::-1] if milli else None, L, kw.get("tail", 0), kw.get("front", 0), milli, kw.get("window", 0))
        assert b.reads[i][L - sb:L - sa] == st[0].alive[i].seq and (sa, sb) != (L - sb, L - sa)
    ctx = _open(tmp_path)
    ctx.set_read_trim(front=kw.get("front", 0), tail=kw.get("tail", 0), qual=kw.get("trim_qual", 0), window=kw.get("window", 0))
    _ingest(ctx, tmp_path, "trim", form, b)
    lengths = [len(r) for r in b.reads]
    ranges = [(0, 0) if not a.seq else (a.src - s, a.src - s + len(a.seq)) for a, s in zip(st[0].alive, rb._starts(b.reads, [1500] * 3))]
    assert ctx.read_trim_info() == read_trim_rule.info(lengths, ranges, kw.get("front", 0), kw.get("tail", 0))
    _check(ctx, st[0], form, name, 3)
    ctx.close()


@pytest.mark.parametrize("form", INGEST_FORMS)
def test_b_depth_cap_cutting_inside_the_second_block(tmp_path, form):
    b = rb.cap_batch()
    st = pipeline(b.reads, None, b.rev, dict(cuts=b.cuts, max_covg=rb.CAP_COVG, genome_size=rb.CAP_G))
    assert rb.CAP_G == G
    ctx = _open(tmp_path)
    ctx.set_max_covg(rb.CAP_COVG)
    _ingest(ctx, tmp_path, "cap", form, b)
    info = ctx.max_covg_info()
    assert info["reached"] and info["reads"] == b.notes["cut"] + 1, info
    _check(ctx, st[2], form, "depth cap", 3)
    ctx.close()


# ---- c. a block that vanishes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TEXT_AND_PACKED)
@pytest.mark.parametrize("kind", rb.VANISH_KINDS)
def test_c_a_middle_block_that_vanishes(tmp_path, kind, form):
    b, settings = rb.vanish_batch(kind)
    L = sum(len(r) for r in b.reads)
    steps = [("dedup", 64), ("subsample", L // 4, 5)]
    st = pipeline(b.reads, b.quals, b.rev, dict(settings, cuts=b.cuts, steps=steps))
    ctx = _open(tmp_path)
    ctx.set_read_trim(qual=settings.get("trim_qual", 0), window=settings.get("window", 0))
    ctx.set_read_filter(min_qual=settings.get("min_qual", 0))
    _ingest(ctx, tmp_path, "gone", form, b)
    assert ctx.resident_info()["blocks"] == 2
    _check(ctx, st[2], form, kind, 3)  # the blocks either side intact, the third under the number 1
    _step(ctx, steps[0], st[3], form, kind, 3)
    _step(ctx, steps[1], st[4], form, kind, 3)
    assert 0 < len(st[4].alive) < len(st[3].alive) < len(st[2].alive)
    ctx.close()


# ---- d. the stages composed -------------------------------------------------------------------------------------------------------------------
def _composed(tmp_path, form):
    """the composed run in one context: ingest under trim + filter + cap, then the resident steps, the read-back checked behind each"""
    b = rb.composed_batch()
    s = b.notes["settings"]
    st = pipeline(b.reads, b.quals, b.rev, s)
    ctx = _open(tmp_path, b.notes["panel"])
    ctx.set_read_trim(front=s["front"], tail=s["tail"], qual=s["trim_qual"], window=s["window"])
    ctx.set_read_filter(min_len=s["min_len"], max_len=s["max_len"], min_qual=s["min_qual"])
    ctx.set_max_covg(s["max_covg"])
    _ingest(ctx, tmp_path, "all", form, b)
    info = ctx.max_covg_info()
    assert info["reached"] and info["reads"] == len(st[2].alive), info
    _check(ctx, st[2], form, "ingest", 3)
    ctx.set_max_covg(None)  # (the subsample refuses a context with a cap set: the cap has done its work at ingest)
    for step, stage in zip(s["steps"], st[3:]):
        _step(ctx, step, stage, form, "composed", 3)
    return ctx, st, b


@pytest.mark.parametrize("form", rb.FORMS)
def test_d_the_stages_composed(tmp_path, form):
    ctx, st, b = _composed(tmp_path, form)
    assert st[4].flags == [1] * len(st[3].alive)  # the second dedup drops nothing more
    # the invariance the headers promise: upper-cased and N-masked, the final read-back is the same sample whatever the input form -- the
    # pipeline's last stage normalised, which does not know the form
    got, _ = rb.read_back(ctx)
    same_for_all, blind = rb.expected([a.seq.translate(rb.NORMAL) for a in st[-1].alive], True)
    assert [r.translate(rb.NORMAL) for r in got] == same_for_all and len(got) > 300 and blind
    ctx.close()


# ---- e. qualities behind the trim -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("form", INGEST_FORMS)
def test_e_the_filter_sums_the_qualities_of_the_kept_range_alone(tmp_path, form, shift):
    """the tripwire batch: one cut quality byte among those the filter sums fails the read (tests/test_resident_readback.py).  shift: a read of
    one base in front, so that every read's qualities -- a block's quality bytes lie as its bases do -- start one byte further on"""
    b = rb.tripwire_batch()
    if shift:
        b = b._replace(reads=[b"A"] + b.reads, quals=[np.full(1, 40, dtype=np.uint8)] + b.quals, rev=[False] + b.rev, cuts=[0, len(b.reads) + 1])
    st = pipeline(b.reads, b.quals, b.rev, dict(rb.TRIPWIRE_TRIM, **rb.TRIPWIRE_FILTER))
    assert len(st[1].alive) == len(b.reads) and any(b.rev) and not all(b.rev)
    ctx = _open(tmp_path)
    ctx.set_read_trim(qual=rb.TRIPWIRE_TRIM["trim_qual"], window=rb.TRIPWIRE_TRIM["window"])
    ctx.set_read_filter(min_qual=rb.TRIPWIRE_FILTER["min_qual"])
    _ingest(ctx, tmp_path, "wire", form, b)
    info = ctx.read_filter_info()
    assert info["dropped_low_qual"] == 0 and info["reads_kept"] == len(b.reads), info
    _check(ctx, st[1], form, "tripwire", 1)
    ctx.close()


# ---- f. map_resident from a compacted context ---------------------------------------------------------------------------------------------------
def test_f_map_resident_maps_what_was_read_back(tmp_path, oracle):
    form = "fastq packed"
    ctx, st, b = _composed(tmp_path, form)
    final = st[-1].alive
    got, _ = rb.read_back(ctx)
    want, omitted = rb.expected([a.seq for a in final], True)
    assert got == want
    # the read-back's reads as a file; the reads it cannot return stand where they stood (they count as reads and bases, and hold no k-mer)
    assert any(final[i].seq for i in omitted)  # a read with bases among them
    reads, k, omitted = [], 0, set(omitted)
    for i, a in enumerate(final):
        if i in omitted:
            reads.append(a.seq)
        else:
            reads.append(got[k])
            k += 1
    (tmp_path / "second").mkdir()
    (tmp_path / "third").mkdir()
    second, third = _open(tmp_path / "second", b.notes["panel"]), _open(tmp_path / "third", b.notes["panel"])
    second.map_resident(ctx)
    third.map_fastx(rb.write_file(tmp_path / "readback.fq", "fastq ascii", reads, None, [False] * len(reads)))
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    ocov, oprg, ocnt = _oracle_map(oracle, _oracle_index(oracle, ctx.prg_strings, W, K), bases, offs, W, K, True)
    assert ocnt["clusters_kept"] > 5
    for c in (ctx, second, third):
        cov, prg = c.coverage()
        cnt = c.counters()
        assert cnt["reads"] == len(reads) and cnt["bases"] == int(offs[-1])
        assert all(cnt[key] == ocnt[key] for key in ("hits", "clusters_kept", "hits_kept")), (cnt, ocnt)
        assert np.array_equal(cov, ocov) and np.array_equal(prg, oprg)
    for c in (ctx, second, third):
        c.close()
