"""The accepted (w, k) range at its edges on the device, against the oracle (pytest -m gpu).

The batches come from tests/wk_range.py (checked on the CPU by tests/test_wk_range.py): the key-width switch at k = 15 | 16, windows of 20 ..
1 024 k-mers (halos of 32 .. 1 024 positions, tiles of 4 032 .. 2 048), the length-governed size threshold either side of the w at which
expected_minimizers stops multiplying and divides, and k <= 7.  Everything goes through test_gpu_parity._ctx / _compare: ASCII and packed,
vectors and counters bit-exact; a difference names (w, k), the kernel sequence and the reads the per-read kernel left over."""
import numpy as np
import pytest

import edge_reads as E
import wk_range as W
from test_gpu_parity import FORCED_GENERIC, ORACLE_THREADS, _compare, _ctx
from test_gpu_regrow import RERUNS, _no_regrow_cap, _open

pytestmark = pytest.mark.gpu

THREADS = min(8, ORACLE_THREADS)
DEFAULT_MIN_CAPACITY = 1 << 20  # entries (csrc/mapper.h min_capacity_)


def _compare_named(ctx, oracle, bases, offs, w, k, illumina, kernel, mcs, what=""):
    try:
        return _compare(ctx, oracle, bases, offs, w, k, illumina, kernel, min_cluster_size=mcs, threads=THREADS)
    except AssertionError as e:
        raise AssertionError(f"(w={w}, k={k}){what}, kernel sequence {kernel}, sketch_form {ctx.table_tier()['sketch_form']}: "
                             f"leftover_reads={ctx.counters()['leftover_reads']}: {e}") from e


# ---- key width ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,k", W.K_EDGE)
def test_key_width_edge(tmp_path, oracle, w, k):
    panel = W.k_edge_panel()
    bases, offs, _ = W.k_edge_reads()
    for kernel in (1, 2, 3) if (w, k) == (11, 15) else (1, 3):
        ctx = _ctx(tmp_path, panel, w, k, True, kernel=kernel, min_cluster_size=W.MCS)
        tier = ctx.table_tier()
        assert ctx.n_slots & (ctx.n_slots - 1) == 0
        if k >= 16:  # u64 keys: the sequential scan on 16-byte slots, whichever direct sequence
            assert tier["sketch_form"] == 4 and tier["table_bytes"] == 16 * ctx.n_slots, (w, k, kernel, tier)
        else:        # u32 keys: the wave form (candidate sequence) or the compile-time window (generic pipeline) at w = 11; 12-byte slots
            assert tier["sketch_form"] == {1: 2, 3: 1}.get(kernel, tier["sketch_form"]) and tier["sketch_form"] in (1, 2, 3, 10, 11, 12)
            assert tier["table_bytes"] == 12 * ctx.n_slots, (w, k, kernel, tier)
        cnt = _compare_named(ctx, oracle, bases, offs, w, k, True, kernel, W.MCS)
        assert cnt["clusters_kept"] > 0
        ctx.close()


@pytest.mark.parametrize("w,k", [(11, 16), (17, 15)])
def test_the_filtered_sequence_refuses_wide_keys_and_wide_windows(tmp_path, w, k):
    from drprg_amd import DependencyError
    with pytest.raises(DependencyError):
        _ctx(tmp_path, W.k_edge_panel(), w, k, True, kernel=2)


# ---- window and halo ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", W.W_EDGE_K)
@pytest.mark.parametrize("w", W.W_EDGE)
def test_window_edge(tmp_path, oracle, w, k):
    panel, _ = W.w_edge_panel()
    bases, offs, _ = W.w_edge_batch(w, k)
    illumina = W.w_illumina(w)
    for kernel in (1, 3, 0):
        ctx = _ctx(tmp_path, panel, w, k, illumina, kernel=kernel, min_cluster_size=W.W_MCS)
        form = ctx.table_tier()["sketch_form"]
        assert form == (3 if k <= 15 else 4), (w, k, kernel, form)  # (kernel 0: w > 16 leaves the direct sequence, never the filter)
        cnt = _compare_named(ctx, oracle, bases, offs, w, k, illumina, kernel, W.W_MCS)
        assert cnt["clusters_kept"] > 0
        if w == 1024:  # test_batches_accumulate's property: three pieces == the whole (every piece has its own tile origins)
            ctx.reset()
            ctx.map_host(bases, offs)
            one, one_prg = ctx.coverage()
            ctx.reset()
            n = len(offs) - 1
            for lo, hi in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)):
                ctx.map_host(bases[int(offs[lo]):int(offs[hi])], offs[lo:hi + 1] - offs[lo])
            three, three_prg = ctx.coverage()
            assert np.array_equal(one, three) and np.array_equal(one_prg, three_prg), (w, k, kernel)
        ctx.close()


# ---- the length-governed threshold at the reciprocal's limit --------------------------------------------------------------------------
@pytest.mark.parametrize("w", W.SIZE_LEN_W)
def test_size_len_at_the_reciprocal_limit(tmp_path, oracle, w):
    """the on side and the off side together, then each alone (test_gpu_rule_edges.test_class_on_the_device).  On the candidate sequence no
    read is left to the generic pipeline: it is read_cluster_kernel's expected_minimizers that sets every threshold"""
    cls = W.size_len_class(oracle, w)
    panel = E.panel_of(oracle, cls.panel)[0]
    for kernel in (1, 3):
        ctx = _ctx(tmp_path, panel, w, E.K, False, kernel=kernel, min_cluster_size=cls.mcs)
        for side, reads in (("both", cls.reads()), ("on", cls.on), ("off", cls.off)):
            bases, offs = E.batch(reads)
            cnt = _compare_named(ctx, oracle, bases, offs, w, E.K, False, kernel, cls.mcs, f" size_len ({side})")
            assert cnt["clusters_kept"] == (0 if side == "on" else len(cls.off)), (w, side, cnt)
            if kernel == 3 and not FORCED_GENERIC:
                assert ctx.counters()["leftover_reads"] == 0, (w, side, ctx.counters())
        ctx.close()


# ---- tiny k ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2, 3])
@pytest.mark.parametrize("w,k", W.K_TINY)
def test_tiny_k(tmp_path, oracle, monkeypatch, w, k, kernel):
    """keys with hundreds of records: reads with more hits than read_cluster_kernel stages go through the generic pipeline, and the buffers
    grow no more often than on a context opened with room to spare"""
    panel, _ = W.tiny_panel()
    bases, offs = W.batch(W.tiny_reads(w, k))
    hits = int(W.tiny_census(oracle, w, k).sum())
    # (one kernel sequence per case: at (1, 1) the batch carries 48 M hits)
    ctx = _ctx(tmp_path, panel, w, k, True, kernel=kernel, min_cluster_size=W.MCS)
    before = ctx.buffer_info()
    cnt = _compare_named(ctx, oracle, bases, offs, w, k, True, kernel, W.MCS)
    assert cnt["clusters_kept"] > 0 and cnt["hits"] == hits
    if kernel != 1 and not FORCED_GENERIC:
        assert ctx.counters()["leftover_reads"] > 0, (w, k, kernel, ctx.counters())
    cov, after = ctx.coverage(), ctx.buffer_info()
    ctx.close()
    roomy = _open(monkeypatch, tmp_path, panel, w, k, kernel, max(_no_regrow_cap(int(offs[-1])), 2 * hits))
    roomy.set_opts(illumina=True, genome_size=20000, kernel=kernel, min_cluster_size=W.MCS)
    r_before = roomy.buffer_info()
    roomy.map_host(bases, offs)
    r_cov, r_after = roomy.coverage(), roomy.buffer_info()
    roomy.close()
    assert np.array_equal(cov[0], r_cov[0]) and np.array_equal(cov[1], r_cov[1]), (w, k, kernel)
    # _compare maps the batch twice, ASCII and packed; capacity only grows, so the second run needs nothing the first did not.  A tile's
    # candidate slice starts at 256 entries whatever the smallest capacity: the roomy context needs those reruns too.  The hit buffer
    # of the generic pipeline is what the smallest capacity sizes: where the batch's hits exceed it the aborted attempt reports their
    # exact number and the buffer grows to it, once
    grew = {key: after[key] - before[key] for key in RERUNS}
    need = {key: r_after[key] - r_before[key] for key in RERUNS}
    if kernel == 1 and hits > max(DEFAULT_MIN_CAPACITY, int(offs[-1]) // 64):
        need["hit_regrows"] += 1
        # (and grew to exactly what that attempt asked for, as test_gpu_regrow.test_generic_hit_buffer_regrows_once has it: no second cause)
        assert after["hit_capacity"] == hits + hits // 8 + 1024, (w, k, after, hits)
    print(f"(w={w}, k={k}) kernel sequence {kernel}: reruns {grew}, with room to spare {need}, capacities {after} / {r_after}")
    assert all(grew[key] <= need[key] for key in RERUNS), (w, k, kernel, grew, need)
