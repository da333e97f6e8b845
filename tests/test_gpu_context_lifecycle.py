"""A context's device memory over its life: opened and closed again and again, closed with a batch in flight, kept after a refused call
(pytest -m gpu).

Every buffer, pinned block, event and stream of the mapper belongs to one owner that frees it; what could still go wrong is an owner
that comes back in a stale state (a lane, tile set or staging set that believes it still has room), an order of destruction that frees
what a queued batch reads, or a refusal that leaves the context half set up.  The batch is test_gpu_regrow.py's dense one (20 000 x 150 bp,
every read inside the panel), which with the smallest capacity at 4 096 entries outgrows the first buffers of all three sequences: the
filtered one starts at n_bases / 48 candidates, the direct candidate form at n_bases / 16, the generic hit buffer at n_bases / 64.
Nothing here provokes a device fault: every refusal is a host-side check that returns before any launch."""
import numpy as np
import pytest

from test_gpu_batch_refusals import EINVAL, MSG_ALIGN, MSG_NPOS, _call, _Device
from test_gpu_regrow import _dense, _dense_panel, _open, _Oracle, _to_device

pytestmark = pytest.mark.gpu

W, K, MIN_CAP = 11, 15, 4096
CYCLES = 6


def _case(oracle):
    panel = _dense_panel()[0]
    bases, offs = _dense()
    ocov, oprg, ocnt = _Oracle.of(oracle, panel.prgs, bases, offs, W, K)
    assert ocnt["hits"] > 100000
    return panel, bases, offs, ocov, oprg, ocnt


def _assert_oracle(ctx, ocov, oprg, what):
    cov, prg = ctx.coverage()  # (completes a deferred batch)
    assert np.array_equal(cov, ocov), what
    assert np.array_equal(prg, oprg), what


def _map_device(ctx, tens, offs, packed, deferred):
    tb, to, tn, nn = tens
    n_reads, n_bases = len(offs) - 1, int(offs[-1])
    if packed:
        ctx.map_device_packed(tb.data_ptr(), to.data_ptr(), n_reads, n_bases, tn.data_ptr() if tn is not None else None, nn, deferred=deferred)
    elif deferred:
        ctx.map_device_async(tb.data_ptr(), to.data_ptr(), n_reads, n_bases)
    else:
        ctx.map_device(tb.data_ptr(), to.data_ptr(), n_reads, n_bases)


@pytest.mark.parametrize("kernel", [2, 3, 1], ids=["filtered", "direct_candidates", "generic"])
def test_repeated_open_map_close(tmp_path, oracle, monkeypatch, kernel):
    """Six times in one process: open, the batch from the host and deferred from device memory, ASCII and packed, each against the
    oracle, close.  Every cycle reruns and regrows exactly as the first did, and ends at the capacities the growth rules give: lanes
    n_bases / 48 x 4 per filtered rerun, n_bases / 16 x 2 per direct rerun; the hit buffer hits + hits / 8 + 1024 after its one regrow."""
    import torch
    from drprg_amd.pandora import pack_reads
    panel, bases, offs, ocov, oprg, ocnt = _case(oracle)
    n_bases = int(offs[-1])
    words, npos = pack_reads(bases)
    tens = {packed: _to_device(torch, bases, offs, packed) for packed in (False, True)}
    torch.cuda.synchronize()
    infos = []
    for cycle in range(CYCLES):
        ctx = _open(monkeypatch, tmp_path, panel, W, K, kernel, MIN_CAP)
        assert ctx.counters()["kernel"] == kernel
        for packed in (False, True):
            ctx.reset()
            if packed:
                ctx.map_host_packed(words, offs, npos)
            else:
                ctx.map_host(bases, offs)
            _assert_oracle(ctx, ocov, oprg, (cycle, "host", packed))
            ctx.reset()
            _map_device(ctx, tens[packed], offs, packed, deferred=True)
            _assert_oracle(ctx, ocov, oprg, (cycle, "deferred", packed))
        infos.append(ctx.buffer_info())
        ctx.close()
    print(f"kernel {kernel}: {infos[0]}")
    first = infos[0]
    own = {2: "filter_reruns", 3: "direct_reruns", 1: "hit_regrows"}[kernel]
    for key in ("filter_reruns", "direct_reruns", "hit_regrows"):
        assert (first[key] >= 1) if key == own else (first[key] == 0), first
    if kernel == 1:
        assert first["hit_regrows"] == 1 and first["hit_capacity"] == ocnt["hits"] + ocnt["hits"] // 8 + 1024, first
    else:
        start, factor = (n_bases // 48, 4) if kernel == 2 else (n_bases // 16, 2)
        assert start > MIN_CAP
        assert first["lane_capacity"] in [start * factor ** r for r in range(1, first[own] + 1)], first
    for cycle, info in enumerate(infos):
        assert info == first, (cycle, info, first)


@pytest.mark.parametrize("kernel", [2, 3], ids=["filtered", "direct_candidates"])
def test_close_with_a_batch_in_flight(tmp_path, oracle, monkeypatch, kernel):
    """close() right behind a deferred map (which, on buffers this small, still has its rerun ahead of it): the context completes the
    batch and frees everything in an order the device agrees with; a fresh context on the same device maps the same batch exactly."""
    import torch
    panel, bases, offs, ocov, oprg, _ = _case(oracle)
    tens = _to_device(torch, bases, offs, False)
    torch.cuda.synchronize()
    ctx = _open(monkeypatch, tmp_path, panel, W, K, kernel, MIN_CAP)
    _map_device(ctx, tens, offs, False, deferred=True)
    ctx.close()
    torch.cuda.synchronize()
    ctx = _open(monkeypatch, tmp_path, panel, W, K, kernel, MIN_CAP)
    _map_device(ctx, tens, offs, False, deferred=False)
    _assert_oracle(ctx, ocov, oprg, "fresh context")
    ctx.close()


def test_a_refused_call_leaves_the_context_usable(tmp_path, oracle, monkeypatch):
    """Two batches Mapper::check refuses (misaligned d_bases; n_npos > 0 without the positions) and an option set_params refuses, each
    returning its error on the host; the next valid batch on the same context is the oracle's and close() succeeds.  (The window size w
    is fixed when a context opens and is no field of drprg_hip_map_opts, so no set_opts call can carry w = 0; kernel = 4 is refused by the
    same block of set_params, before any state changes.)"""
    from drprg_amd import DependencyError
    panel, bases, offs, ocov, oprg, _ = _case(oracle)
    dev = _Device(bases, offs)
    ctx = _open(monkeypatch, tmp_path, panel, W, K, 0, MIN_CAP)
    data, d_offs = dev.bases.data_ptr(), dev.offs.data_ptr()
    assert _call(ctx, "device", data + 4, d_offs, dev.n_reads, dev.n_bases) == (EINVAL, MSG_ALIGN[False])
    assert _call(ctx, "device_async", data + 4, d_offs, dev.n_reads, dev.n_bases) == (EINVAL, MSG_ALIGN[False])
    assert _call(ctx, "device_packed", dev.words.data_ptr(), d_offs, dev.n_reads, dev.n_bases, None, 1) == (EINVAL, MSG_NPOS)
    assert _call(ctx, "device_packed_async", dev.words.data_ptr(), d_offs, dev.n_reads, dev.n_bases, None, 1) == (EINVAL, MSG_NPOS)
    with pytest.raises(DependencyError, match="kernel must be 0") as refused:
        ctx.set_opts(illumina=True, genome_size=20000, kernel=4)
    assert refused.value.code == -EINVAL
    assert not ctx.coverage()[0].any() and ctx.counters()["reads"] == 0 and ctx.counters()["kernel"] == 2
    assert _call(ctx, "device_async", data, d_offs, dev.n_reads, dev.n_bases)[0] == 0
    _assert_oracle(ctx, ocov, oprg, "after the refusals")
    ctx.close()
    assert ctx._h is None
