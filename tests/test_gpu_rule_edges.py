"""The clustering rules' edges and the per-read kernel's limits on the device, against the oracle (pytest -m gpu).

The reads come from tests/edge_reads.py: built by recipe, accepted by the oracle's trace, checked on the CPU by tests/test_edge_reads.py.
Every class is a batch of its own -- two wrong decisions cannot cancel across classes --, through kernel sequences 1, 2 and 3, ASCII and
packed (test_gpu_parity._compare), vectors and counters bit-exact; a class that fails names the rule a kernel broke."""
import numpy as np
import pytest

import edge_reads as E
from test_gpu_parity import FORCED_GENERIC, _compare, _ctx

pytestmark = pytest.mark.gpu

CLASSES = ([f"{r}_{t}" for t in ("illumina", "nanopore") for r in ("gap", "size_mcs", "size_path", "size_len")]
           + [f"sweep_w{w}_{t}" for t in ("illumina", "nanopore") for w in E.SWEEP_W]
           + ["strand_tie", "containment", "equal_first", "early_drop_mcs1", "early_drop_mcs2", "early_drop_mcs10"])


def _compare_named(ctx, oracle, bases, offs, w, illumina, kernel, mcs, what):
    """_compare; a difference is reported with the class and the reads the per-read kernel left to the generic pipeline"""
    try:
        return _compare(ctx, oracle, bases, offs, w, E.K, illumina, kernel, min_cluster_size=mcs)
    except AssertionError as e:
        raise AssertionError(f"{what}, kernel sequence {kernel}: leftover_reads={ctx.counters()['leftover_reads']}: {e}") from e


def _keyed_minimizers(oracle, cls_key, reads):
    """the read minimizers whose hash is an index key, by the oracle's trace"""
    panel, w, illumina, mcs = cls_key
    tr = E.Tracer(oracle, panel, w, illumina, mcs)
    return sum(tr(r)["keyed"] for r in reads)


@pytest.mark.parametrize("name", CLASSES)
def test_class_on_the_device(tmp_path, oracle, name):
    """one class, one batch: the on side and the off side together, then each side alone"""
    cls = E.build(oracle)[name]
    panel = E.panel_of(oracle, cls.panel)[0]
    sides = [("both", cls.reads())] + [(s, r) for s, r in (("on", cls.on), ("off", cls.off)) if r]
    for kernel in (1, 2, 3):
        ctx = _ctx(tmp_path, panel, cls.w, E.K, cls.illumina, kernel=kernel, min_cluster_size=cls.mcs)
        for side, reads in sides:
            bases, offs = E.batch(reads)
            ocnt = _compare_named(ctx, oracle, bases, offs, cls.w, cls.illumina, kernel, cls.mcs, f"{name} ({side})")
            if kernel == 2 and side == "both":
                # the filtered sequence's `minimizers` (which _compare leaves out): the minimizers that are index keys
                ctx.reset()
                ctx.map_host(bases, offs)
                got, want = ctx.counters()["minimizers"], _keyed_minimizers(oracle, cls.key, reads)
                assert got == want, f"{name}: minimizers {got} (filtered sequence), {want} keyed by the trace, {ocnt['minimizers']} in all"
        ctx.close()


@pytest.mark.parametrize("panel_name,w,illumina", [("main", 11, True), ("main", 11, False), ("sweep", 11, True), ("sweep", 14, False)])
def test_all_classes_shuffled_into_one_batch(tmp_path, oracle, panel_name, w, illumina):
    """every read of every class in one batch, in random order, under one panel and technology: no read is on an edge it was built for any
    more than by chance, but every path of the per-read kernel is taken next to every other"""
    reads = [r for c in E.build(oracle).values() for r in c.reads()]
    order = np.random.default_rng(7).permutation(len(reads))
    bases, offs = E.batch([reads[i] for i in order])
    panel = E.panel_of(oracle, panel_name)[0]
    for kernel in (1, 2, 3):
        ctx = _ctx(tmp_path, panel, w, E.K, illumina, kernel=kernel, min_cluster_size=2)
        cnt = _compare_named(ctx, oracle, bases, offs, w, illumina, kernel, 2, "all classes")
        assert cnt["clusters_kept"] > 1000
        ctx.close()


# ---- the look-ahead forms of read_cluster_kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", [300, 301, 600, 601])
def test_lookahead_forms_at_their_limits(tmp_path, oracle, mean):
    """launch_read_cluster picks 128, 256 or 512 slots of look-ahead by the batch's mean read length (<= 300, <= 600, above): the same
    2 000 on-panel reads (150, 400 and 3 000 bases) padded with off-panel reads to a mean of exactly 300, 301, 600 and 601 bases"""
    panel, info = E.main_panel(oracle)
    rng = np.random.default_rng(11)
    srcs = [info["seqs"]["a"], info["seqs"]["b"]]
    on = []
    for n, length in ((1200, 150), (600, 400), (200, 3000)):
        for i in range(n):
            src = srcs[i % 2]
            s = int(rng.integers(0, len(src) - length + 1))
            r = src[s:s + length]
            on.append(E.rc(r) if rng.random() < 0.5 else r)
    n_pad = 4000 if mean < 510 else 2000
    total = mean * (len(on) + n_pad) - sum(len(r) for r in on)
    assert total > 0
    fill = E._seq(rng, 200000)
    pads = []
    for i in range(n_pad):
        ln = total // n_pad + (1 if i < total % n_pad else 0)
        s = int(rng.integers(0, len(fill) - ln))
        pads.append(fill[s:s + ln])
    reads = on + pads
    reads = [reads[i] for i in rng.permutation(len(reads))]
    bases, offs = E.batch(reads)
    assert int(offs[-1]) // (len(offs) - 1) == mean and int(offs[-1]) % (len(offs) - 1) == 0
    for kernel in (2, 3):  # (dense candidate list and tile slices)
        ctx = _ctx(tmp_path, panel, 11, E.K, False, kernel=kernel)
        cnt = _compare_named(ctx, oracle, bases, offs, 11, False, kernel, 10, f"mean read length {mean}")
        assert cnt["clusters_kept"] >= 2000
        ctx.close()


# ---- the limits of read_cluster_kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last", [65533, 65534, 65535, 65536])
def test_last_hit_at_the_16_bit_position_limit(tmp_path, oracle, last):
    """A read of ~66 000 off-panel bases with one block of locus b planted so that its last hit lies at position 65 533 .. 65 536 (by the
    trace).  read_cluster_kernel keeps positions in 16 bits: from 65 534 on the read must be left to the generic pipeline, at 65 533 it must
    not be -- the off-panel stretch holds no minimizer that is an index key (the trace: every hit lies on b), so the read's ~100 candidates
    fit any chunk and the position alone decides; the fifty short reads beside it never are leftovers.  Both sides equal the oracle."""
    panel, info = E.main_panel(oracle)
    tr = E.Tracer(oracle, "main", 11, False, 10)
    read = _planted(oracle, tr, info["seqs"]["b"][700:1300], last, last)
    cls = E.build(oracle)["gap_nanopore"]
    bases, offs = E.batch(cls.on[:25] + [read] + cls.off[:25])
    for kernel in (1, 2, 3):
        ctx = _ctx(tmp_path, panel, 11, E.K, False, kernel=kernel)
        _compare_named(ctx, oracle, bases, offs, 11, False, kernel, 10, f"last hit at {last}")
        if kernel != 1 and not FORCED_GENERIC:
            left = ctx.counters()["leftover_reads"]
            assert left == (1 if last >= 65534 else 0), f"last hit at {last}, kernel sequence {kernel}: leftover_reads {left}"
        ctx.close()


def _planted(oracle, tr, block, last, seed, pure=True):
    """a read of off-panel bases with `block` planted so that its last hit lies at position `last` (by the trace; one cluster kept),
    400 off-panel bases behind the block.  pure: every hit lies on the block's PRG (megabases of random sequence do hold a few minimizers
    that are index keys: single hits, never a cluster)"""
    rng = np.random.default_rng(seed)
    fill = E._seq(rng, last + 1000)
    at = last - len(block) + 20
    for _ in range(5):  # (the block's last minimizer depends on what follows it: place, look, move)
        read = fill[:at] + block + fill[at:at + 400]
        t = tr(read)
        assert len(t["hits"]) > 20 and (not pure or len(set(t["hits"]["prg"].tolist())) == 1)
        if int(t["hits"]["pos"].max()) == last:
            break
        at += last - int(t["hits"]["pos"].max())
    assert int(t["hits"]["pos"].max()) == last and t["clusters"]["alive"].sum() == 1, "the recipe missed: not a kernel's fault"
    return read


EOVERFLOW = 75  # DependencyError.code of DRPRG_EOVERFLOW (csrc/common.h)


@pytest.mark.parametrize("kernel", [1, 2, 3])
def test_a_hit_at_position_2_to_the_23(tmp_path, oracle, kernel):
    """The hit key holds 23 bits of read position.  A read a little longer than 2^23 bases whose last hit lies at 2^23 - 1 maps and equals the
    oracle; the same read with that hit at 2^23 makes every entry point fail with DRPRG_EOVERFLOW -- map_host, map_host_packed, map_device, and
    map_device_async followed by a good batch, where the error surfaces while the next batch is in flight (at the latest in sync()) --, and
    after reset() the same context maps an ordinary batch and equals the oracle.  A checked error return: nothing faults."""
    import torch
    from drprg_amd import DependencyError
    from drprg_amd.pandora import pack_reads
    panel, info = E.main_panel(oracle)
    tr = E.Tracer(oracle, "main", 11, False, 10)
    block = info["seqs"]["b"][700:1300]
    cls = E.build(oracle)["gap_nanopore"]
    short = cls.on[:25] + cls.off[:25]
    good = E.batch(short[:25] + [_planted(oracle, tr, block, (1 << 23) - 1, 23, pure=False)] + short[25:])
    bad = E.batch(short[:25] + [_planted(oracle, tr, block, 1 << 23, 24, pure=False)] + short[25:])
    ordinary = E.batch(cls.reads())
    ctx = _ctx(tmp_path, panel, 11, E.K, False, kernel=kernel)
    _compare_named(ctx, oracle, *good, 11, False, kernel, 10, "last hit at 2^23 - 1")
    dev = torch.device("cuda", 0)
    d_bad = (torch.from_numpy(bad[0]).to(dev), torch.from_numpy(bad[1].astype(np.int64)).to(dev))
    d_ord = (torch.from_numpy(ordinary[0]).to(dev), torch.from_numpy(ordinary[1].astype(np.int64)).to(dev))
    torch.cuda.synchronize()
    words, npos = pack_reads(bad[0])

    def deferred():
        ctx.map_device_async(d_bad[0].data_ptr(), d_bad[1].data_ptr(), len(bad[1]) - 1, int(bad[1][-1]))
        ctx.map_device_async(d_ord[0].data_ptr(), d_ord[1].data_ptr(), len(ordinary[1]) - 1, int(ordinary[1][-1]))
        ctx.sync()

    entries = [("map_host", lambda: ctx.map_host(*bad)), ("map_host_packed", lambda: ctx.map_host_packed(words, bad[1], npos)),
               ("map_device", lambda: ctx.map_device(d_bad[0].data_ptr(), d_bad[1].data_ptr(), len(bad[1]) - 1, int(bad[1][-1]))),
               ("map_device_async", deferred)]
    for name, call in entries:
        ctx.reset()
        with pytest.raises(DependencyError) as err:
            call()
        assert err.value.code == EOVERFLOW, (name, kernel, str(err.value))
        ctx.sync()  # (the deferred path: the good batch behind the bad one is complete, and completing it raises nothing)
        cnt = _compare_named(ctx, oracle, *ordinary, 11, False, kernel, 10, f"an ordinary batch after {name} failed")
        assert cnt["clusters_kept"] >= len(cls.on)
    ctx.close()


@pytest.mark.parametrize("copies", [63, 64, 65])
def test_64_and_65_clusters_in_a_read(tmp_path, oracle, copies):
    """one read of a locus that the panel holds 63, 64 or 65 times (a cluster on each; lane j of the wave path holds cluster j), next to thirty
    ordinary reads -- few enough for the chunk's staged hits: with 65 copies that one read, and no other, goes to the generic pipeline"""
    from drprg_amd import synth
    rng = np.random.default_rng(64)
    rep, single = E._seq(rng, 400), E._seq(rng, 900)
    panel = synth.Panel([f"rep{i}" for i in range(copies)] + ["single"], [[rep.decode()]] * copies + [[single.decode()]])
    reads = [single[s:s + 150] for s in rng.integers(0, 750, size=30)]
    reads.insert(15, rep[100:250])
    bases, offs = E.batch(reads)
    for kernel in (1, 2, 3):
        ctx = _ctx(tmp_path, panel, 11, E.K, True, kernel=kernel, min_cluster_size=2)
        cnt = _compare_named(ctx, oracle, bases, offs, 11, True, kernel, 2, f"{copies} copies")
        assert cnt["clusters_kept"] == 31
        if kernel != 1 and not FORCED_GENERIC:
            assert ctx.counters()["leftover_reads"] == (1 if copies > 64 else 0), (copies, kernel, ctx.counters())
        ctx.close()


def test_more_multi_group_reads_than_a_chunk_pools(tmp_path, oracle):
    """6 000 reads of 26 .. 30 bases from the stretch of `a` the panel holds twice, min_cluster_size 1: a hit or two in each of two groups, not
    dropped early (more hits than min_cluster_size), and a chunk of 1 920 owned candidates holds well over the 512 the wave path pools"""
    panel, info = E.main_panel(oracle)
    a = info["seqs"]["a"]
    rng = np.random.default_rng(512)
    reads = []
    for i in range(6000):
        ln, s = int(rng.integers(26, 31)), int(rng.integers(0, 1400))
        reads.append(E._both_strands(a[s:s + ln], i))
    bases, offs = E.batch(reads)
    for kernel in (2, 3):
        ctx = _ctx(tmp_path, panel, 11, E.K, True, kernel=kernel, min_cluster_size=1)
        cnt = _compare_named(ctx, oracle, bases, offs, 11, True, kernel, 1, "pool")
        assert cnt["hits"] > 2 * 4000
        if not FORCED_GENERIC:
            left = ctx.counters()["leftover_reads"]
            assert left > 0, left
        ctx.close()
