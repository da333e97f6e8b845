"""Unlike batches back to back on one context, against the oracle (pytest -m gpu).

tests/batch_sequences.py has the recipes -- ten kinds of small batches in ASCII and packed, one schedule in which every ordered pair of
the twenty states is adjacent somewhere and two apart somewhere, every batch through one of the six entry points, a few reset() points --
and tests/test_batch_sequences.py the census that the schedule and the kinds are what they say.  Here every form of the mapper that carries
state of its own maps that schedule twice on ONE context whose buffers start at their production ratios (DRPRG_HIP_MIN_CAPACITY=0: the
reruns and regrows happen inside the sequence):

  stepwise   coverage, reads per PRG and the counters are read after every batch and must equal the oracle's running sum
  in flight  the same schedule, read only at eight evenly spaced points, at the end, and in front of each reset() (which completes what is
             in flight anyway): in between the lanes stay busy and deferred batches overlap

Bit-exact everywhere.  A failure names the index in the schedule, the batch's state and entry point and the two batches before it."""
import numpy as np
import pytest

import batch_sequences as B
from test_gpu_parity import ORACLE_THREADS, _ctx

pytestmark = pytest.mark.gpu

# (form, kernel sequence, switches, w, k, illumina, table_tier()["sketch_form"], the buffer of its own that must have overflowed)
FORMS = [
    ("small_tier_stage2_lds", 2, {"DRPRG_FILTER_STAGE2": "lds"}, 11, 15, True, 10, "filter_reruns"),
    ("small_tier_stage2_l2", 2, {"DRPRG_FILTER_STAGE2": "l2"}, 11, 15, True, 10, "filter_reruns"),
    ("middle_tier", 2, {"DRPRG_FORCE_MID_TIER": "1"}, 11, 15, True, 12, "filter_reruns"),
    ("levels_1_2", 2, {}, 11, 14, True, 11, "filter_reruns"),
    ("sketch_wave_native_packed", 3, {}, 11, 15, True, 1, "direct_reruns"),
    ("probe_candidates_u32_keys", 3, {}, 12, 15, True, 3, "direct_reruns"),
    ("probe_candidates_u64_keys", 3, {}, 19, 21, True, 4, "direct_reruns"),
    ("generic_pipeline", 1, {}, 11, 15, True, 2, "hit_regrows"),
    ("generic_pipeline_behind_the_filter", 2, {"DRPRG_FT_DEBUG": "8"}, 11, 15, True, 10, "filter_reruns"),
    ("small_tier_nanopore", 2, {}, 11, 15, False, 10, "filter_reruns"),
]
READ_POINTS = 8

_DEVICE = {}


def _pad16(t_np, itemsize_words):
    """the array followed by 64 zero bytes: a batch without bases still has a 16-byte aligned address to give"""
    return np.concatenate([t_np, np.zeros(64 // itemsize_words, t_np.dtype)])


def _device_state(kind, packed):
    """the state's batch in device memory, uploaded once and left there: a deferred batch is run again from its buffers"""
    import torch
    key = (kind, packed)
    if key not in _DEVICE:
        dev = torch.device("cuda", 0)
        bases, offs = B.kind_batch(kind)
        d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
        if packed:
            words, npos = B.kind_packed(kind)
            d_data = torch.from_numpy(_pad16(words, 4).view(np.int32)).to(dev)
            d_npos = torch.from_numpy(npos.astype(np.int64)).to(dev) if npos.size else None
        else:
            d_data, d_npos = torch.from_numpy(_pad16(bases, 1)).to(dev), None
        torch.cuda.synchronize()
        assert d_data.data_ptr() % 16 == 0
        _DEVICE[key] = (d_data, d_offs, d_npos)
    return _DEVICE[key]


def _map(ctx, st):
    bases, offs = B.kind_batch(st.kind)
    n_reads, n_bases = len(offs) - 1, int(offs[-1])
    if st.entry == "map_host":
        return ctx.map_host(bases, offs)
    if st.entry == "map_host_packed":
        words, npos = B.kind_packed(st.kind)
        return ctx.map_host_packed(words, offs, npos)
    d_data, d_offs, d_npos = _device_state(st.kind, st.packed)
    if st.entry == "map_device":
        return ctx.map_device(d_data.data_ptr(), d_offs.data_ptr(), n_reads, n_bases)
    if st.entry == "map_device_async":
        return ctx.map_device_async(d_data.data_ptr(), d_offs.data_ptr(), n_reads, n_bases)
    assert st.entry in ("map_device_packed", "map_device_packed_async"), st
    return ctx.map_device_packed(d_data.data_ptr(), d_offs.data_ptr(), n_reads, n_bases, d_npos.data_ptr() if d_npos is not None else None,
                                 0 if d_npos is None else int(d_npos.numel()), deferred=st.entry == "map_device_packed_async")


def _check(ctx, want, kernel, steps, i, what):
    """coverage, reads per PRG and the counters _compare holds (test_gpu_parity.py), against the running sum after batch i"""
    cov, prg = ctx.coverage()  # (completes a deferred batch)
    cnt = ctx.counters()
    where = f"{what}, {B.describe(steps, i)}"
    bad = np.nonzero(cov != want.cov)[0]
    assert bad.size == 0, f"{where}: coverage differs at {bad.size} entries, the first {bad[0]}: {cov[bad[0]]} != {want.cov[bad[0]]}"
    bad = np.nonzero(prg != want.prg)[0]
    assert bad.size == 0, f"{where}: reads per PRG differ at {bad.size} PRGs, the first {bad[0]}: {prg[bad[0]]} != {want.prg[bad[0]]}"
    for key in B.COUNTERS:
        if key == "minimizers" and kernel == 2:  # (the filtered sequence counts only the minimizers that are index keys)
            continue
        assert cnt[key] == want.cnt[key], f"{where}: {key} {cnt[key]} != {want.cnt[key]}"
    return cnt


def _pass(ctx, per_kind, kernel, steps, read_after, what):
    """the schedule once from a reset; results read after the batches in read_after, in front of every reset() and at the end"""
    ctx.reset()
    want = B.RunningSum(per_kind)
    leftover = 0
    for i, st in enumerate(steps):
        if st.reset_before:
            leftover = max(leftover, _check(ctx, want, kernel, steps, i - 1, what + " (in front of reset())")["leftover_reads"])
            ctx.reset()
            want.reset()
        try:
            _map(ctx, st)
        except Exception as e:
            raise AssertionError(f"{what}, {B.describe(steps, i)}: {e!r}") from e
        want.add(st.kind)
        if i in read_after or i == len(steps) - 1:
            leftover = max(leftover, _check(ctx, want, kernel, steps, i, what)["leftover_reads"])
    return leftover


@pytest.mark.parametrize("form,kernel,env,w,k,illumina,sketch_form,own", FORMS, ids=[f[0] for f in FORMS])
def test_unlike_batches_back_to_back(tmp_path, oracle, monkeypatch, form, kernel, env, w, k, illumina, sketch_form, own):
    import time
    for name, value in env.items():
        monkeypatch.setenv(name, value)  # (read when the context opens, and again by reset())
    monkeypatch.setenv("DRPRG_HIP_MIN_CAPACITY", "0")
    panel = B.panel()[0]
    per_kind = B.oracle_of_kinds(oracle, w, k, illumina, threads=ORACLE_THREADS)
    steps = B.schedule()
    ctx = _ctx(tmp_path, panel, w, k, illumina, kernel=kernel)
    tier = ctx.table_tier()
    assert (tier["kernel"], tier["sketch_form"]) == (kernel, sketch_form), tier  # the form the case is named after serves it
    if form == "middle_tier":
        assert tier["l2_filter_bytes"] > 0
    assert ctx.counters()["kernel"] == kernel and ctx.n_knodes * 2 == per_kind["dense"][0].size
    before = ctx.buffer_info()
    t0 = time.perf_counter()
    leftover = _pass(ctx, per_kind, kernel, steps, set(range(len(steps))), f"{form}, stepwise")
    t1 = time.perf_counter()
    mid = ctx.buffer_info()
    points = {len(steps) * (j + 1) // (READ_POINTS + 1) - 1 for j in range(READ_POINTS)}
    assert len(points) == READ_POINTS
    _pass(ctx, per_kind, kernel, steps, points, f"{form}, in flight")
    t2 = time.perf_counter()
    after = ctx.buffer_info()
    print(f"{form}: {len(steps)} batches stepwise {t1 - t0:.2f} s, in flight {t2 - t1:.2f} s; buffers {before} -> {mid} -> {after}; leftover reads {leftover}")
    # the batches did outgrow the form's own buffer inside the sequence, and no other
    for key in ("filter_reruns", "direct_reruns", "hit_regrows"):
        if key == own:
            assert mid[key] - before[key] >= 1, (before, mid)
        else:  # (the leftovers of a candidate sequence size the hit buffer up front: no regrow is counted for them)
            assert after[key] == before[key], (key, before, after)
    if kernel != 1:
        assert leftover > 0  # reads went through the generic pipeline behind the candidate sequence
    ctx.close()
