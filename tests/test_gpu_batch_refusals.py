"""What a device batch is refused for, and that every door of the library maps the same batch to the same result.

The refusals (code and drprg_hip_last_error text) are those of the table in the mapper's contract: n_npos > 0 without the positions (even for
n_reads == 0), n_reads == 0 is OK whatever the pointers, a null pointer, a pointer that is not 16-byte aligned, more than 2^28 reads -- in
that order, on the host, before anything is launched or dereferenced.  The library is called through ctypes directly, so that no Python
wrapper adds checks of its own.  A refused call changes nothing: counters, depth-cap state, coverage.

The doors: map_host(_packed), map_device(_async), map_device_packed(_async), map_fastx in both input formats, and keep_reads + map_fastx +
map_resident into a second context, for the three kernel sequences.  tests/test_gpu_parity.py holds the two host doors against the oracle on
other ragged reads (test_ragged_and_degenerate_inputs) and the packed device doors and the packed ingest for the default sequence without
empty reads (test_packed_reads_on_the_device_and_through_the_ingest), but compares no door's counters with another door's and counts no
batch of empty reads: every door is in the matrix here."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _ctx, _oracle_index, _oracle_map

pytestmark = pytest.mark.gpu

W, K = 11, 15
OK, EINVAL, EOVERFLOW = 0, -22, -75
MSG_NPOS = "n_npos > 0 without the positions"
MSG_NULL = "null device pointer"
MSG_ALIGN = {False: "d_bases must be 16-byte aligned", True: "d_words must be 16-byte aligned"}
MSG_READS = "at most 268435456 reads per batch"
DEVICE_DOORS = ("device", "device_async", "device_packed", "device_packed_async")
_SHARED = {}


def _shared():
    """panel, the valid 2 000 x 150 bp batch, the ragged batch (N, lower case, three empty reads) and the batch of five empty reads"""
    if not _SHARED:
        from drprg_amd import synth
        panel = synth.small_panel(seed=42)
        gen = synth.HaplotypeGenomes(panel, genome_size=20000, n_hap=4, seed=3)
        bases, offs = synth.sample_short_reads(gen, 2000, seed=7)
        rng = np.random.default_rng(5)
        ragged = bases.copy()
        ragged[rng.integers(0, ragged.size, ragged.size // 200)] = ord("N")
        ragged[rng.integers(0, ragged.size, ragged.size // 200)] |= 0x20
        roffs = np.concatenate([offs[:1], offs[:1001], offs[1000:], offs[-1:]]).astype(np.uint64)  # empty reads: first, 1002nd, last
        assert roffs.size == 2004 and roffs[1] == 0 and roffs[1001] == roffs[1002] and roffs[-1] == roffs[-2]
        _SHARED.update(panel=panel, valid=(bases, offs), ragged=(ragged, roffs), empty=(np.zeros(0, np.uint8), np.zeros(6, np.uint64)))
    return _SHARED


class _Device:
    """one batch in device memory, ASCII and packed"""

    def __init__(self, bases, offs):
        import torch
        from drprg_amd.pandora import pack_reads
        self.n_reads, self.n_bases = len(offs) - 1, int(offs[-1])
        self.bases = torch.from_numpy(np.concatenate([bases, np.zeros(64, np.uint8)])).cuda()
        self.offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        words, npos = pack_reads(bases)
        self.words = torch.from_numpy(np.concatenate([words, np.zeros(16, np.uint32)]).view(np.int32)).cuda()
        self.n_npos = int(npos.size)
        self.npos = torch.from_numpy(np.concatenate([npos, np.zeros(1, np.uint64)]).astype(np.int64)).cuda()
        torch.cuda.synchronize()
        assert self.bases.data_ptr() % 16 == 0 and self.words.data_ptr() % 16 == 0


def _call(ctx, door, d_data, d_offs, n_reads, n_bases, d_npos=None, n_npos=0):
    """the C entry point itself; returns (code, last error)"""
    from drprg_amd._lib import lib
    if door.startswith("device_packed"):
        fn = lib.drprg_hip_map_device_packed_async if door.endswith("async") else lib.drprg_hip_map_device_packed
        rc = fn(ctx._h, d_data, d_offs, n_reads, n_bases, d_npos, n_npos, None, None, None)
    else:
        fn = lib.drprg_hip_map_device_async if door.endswith("async") else lib.drprg_hip_map_device
        rc = fn(ctx._h, d_data, d_offs, n_reads, n_bases, None, None, None)
    return rc, (lib.drprg_hip_last_error(ctx._h) or b"").decode()


def _state(ctx):
    from drprg_amd._lib import lib
    cnt, info = (C.c_uint64 * 8)(), (C.c_uint64 * 4)()
    assert lib.drprg_hip_counters(ctx._h, cnt) == OK and lib.drprg_hip_max_covg_info(ctx._h, info) == OK
    return list(cnt), list(info)


def _offers(door, dev):
    """(what, arguments after the door, code, text): every row of the table that applies to the door's format"""
    packed = door.startswith("device_packed")
    data = (dev.words if packed else dev.bases).data_ptr()
    offs, n, nb = dev.offs.data_ptr(), dev.n_reads, dev.n_bases
    rows = [
        ("null data", (None, offs, n, nb), EINVAL, MSG_NULL),
        ("null offsets", (data, None, n, nb), EINVAL, MSG_NULL),
        ("misaligned", (data + 4, offs, n, nb), EINVAL, MSG_ALIGN[packed]),
        ("too many reads", (data, offs, 2 ** 28 + 1, nb), EOVERFLOW, MSG_READS),
        ("no reads, null pointers", (None, None, 0, 0), OK, None),
    ]
    if packed:
        rows += [
            ("npos missing", (data, offs, n, nb, None, 1), EINVAL, MSG_NPOS),
            ("npos missing, no reads", (data, offs, 0, 0, None, 1), EINVAL, MSG_NPOS),
            ("npos missing, no reads, null pointers", (None, None, 0, 0, None, 1), EINVAL, MSG_NPOS),
            ("no reads, null pointers, positions given", (None, None, 0, 0, dev.npos.data_ptr(), 1), OK, None),
        ]
    return rows


def _map(ctx, door, bases, offs, dev, tmp_path=None, other=None):
    from drprg_amd import synth
    from drprg_amd.pandora import pack_reads
    if door == "host":
        ctx.map_host(bases, offs)
    elif door == "host_packed":
        words, npos = pack_reads(bases)
        ctx.map_host_packed(words, offs, npos)
    elif door in ("device", "device_async"):
        assert _call(ctx, door, dev.bases.data_ptr(), dev.offs.data_ptr(), dev.n_reads, dev.n_bases)[0] == OK
    elif door in ("device_packed", "device_packed_async"):
        rc = _call(ctx, door, dev.words.data_ptr(), dev.offs.data_ptr(), dev.n_reads, dev.n_bases, dev.npos.data_ptr() if dev.n_npos else None, dev.n_npos)
        assert rc[0] == OK, rc
    else:  # fastx, fastx_packed, resident (ASCII ingest, kept, mapped again by `other`)
        fq = str(tmp_path / f"reads_{len(offs)}.fq")
        synth.write_fastq(fq, bases, offs)
        ctx.set_input_format(door == "fastx_packed")
        if door == "resident":
            ctx.keep_reads(1 << 28)
        ctx.map_fastx(fq)
        ctx.set_input_format(False)
        if door == "resident":
            assert ctx.resident_info()["complete"]
            other.reset()
            other.map_resident(ctx)
            ctx.keep_reads(0)
    ctx.sync()


def test_refused_batches_change_nothing_and_the_context_maps_on(tmp_path, oracle):
    s = _shared()
    bases, offs = s["valid"]
    dev = _Device(bases, offs)
    ctx = _ctx(tmp_path, s["panel"], W, K, True, genome_size=20000)
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    ocov, oprg, ocnt = _oracle_map(oracle, idx, bases, offs, W, K, True)
    assert ocnt["clusters_kept"] > 5
    before = _state(ctx)
    assert before[0][0] == 0 and before[1] == [0, 0, 0, 0]
    for door in DEVICE_DOORS:
        for what, args, code, text in _offers(door, dev):
            rc, err = _call(ctx, door, *args)
            print(f"{door}: {what}: {rc} {err!r}")
            assert rc == code, (door, what)
            if code != OK:
                assert err == text, (door, what)
            assert _state(ctx) == before, (door, what)
            assert not ctx.coverage()[0].any() and not ctx.coverage()[1].any(), (door, what)
    # under a depth cap the batch would cross (T = 4 * 1000 bases of its 300 000) the refusal comes before the cut is looked for
    ctx.set_opts(illumina=True, genome_size=1000)
    ctx.set_max_covg(3)
    for door in DEVICE_DOORS:
        for what, args, code, text in _offers(door, dev)[:3]:
            rc, err = _call(ctx, door, *args)
            print(f"capped {door}: {what}: {rc} {err!r}")
            assert (rc, err) == (code, text), (door, what)
            assert _state(ctx) == before, (door, what)  # (cap_reached == 0, dropped_reads == 0 among them)
            assert not ctx.coverage()[0].any() and not ctx.coverage()[1].any(), (door, what)
    # (the cap was armed and these batches would have crossed it: the valid batch does, at read 27 of its 2 000 -- 27 * 150 >= T)
    for door in DEVICE_DOORS:
        ctx.reset()
        _map(ctx, door, bases, offs, dev)
        assert _state(ctx)[1] == [1, 27, 27 * 150, 2000 - 27], door
    ctx.reset()
    ctx.set_max_covg(None)
    ctx.set_opts(illumina=True, genome_size=20000)
    # ... and the context that refused all this maps the valid batch through every door
    counters = {}
    for door in DEVICE_DOORS + ("host", "host_packed"):
        ctx.reset()
        _map(ctx, door, bases, offs, dev)
        cov, prg = ctx.coverage()
        assert np.array_equal(cov, ocov) and np.array_equal(prg, oprg), door
        counters[door] = ctx.counters()
        assert counters[door] == counters["device"], door
    assert counters["host"]["reads"] == 2000 and counters["host"]["hits"] == ocnt["hits"] and counters["host"]["clusters_kept"] == ocnt["clusters_kept"]
    ctx.close()


DOORS = ("host", "host_packed", "device", "device_async", "device_packed", "device_packed_async", "fastx", "fastx_packed", "resident")


@pytest.mark.parametrize("kernel", [0, 1, 3])
def test_every_door_every_sequence(tmp_path, oracle, kernel):
    """the ragged batch and the batch of empty reads through every door: the oracle's vectors, and within a sequence the same counters"""
    s = _shared()
    ctx = _ctx(tmp_path, s["panel"], W, K, True, kernel=kernel)
    other = _ctx(tmp_path, s["panel"], W, K, True, kernel=kernel)
    idx = _oracle_index(oracle, ctx.prg_strings, W, K)
    for name in ("ragged", "empty"):
        bases, offs = s[name]
        ocov, oprg, ocnt = _oracle_map(oracle, idx, bases, offs, W, K, True)
        dev = _Device(bases, offs)
        assert (dev.n_npos > 1000 and ocnt["clusters_kept"] > 5) if name == "ragged" else not ocov.any()
        first = None
        for door in DOORS:
            ctx.reset()
            _map(ctx, door, bases, offs, dev, tmp_path, other)
            cnt = ctx.counters()
            print(f"kernel {kernel} {name} {door}: {cnt}")
            # (the resident door: the ingesting context AND the one that maps its kept reads.  A batch of empty reads keeps nothing in
            # HBM -- there is nothing to copy --, so the second context is offered no batch and counts no read: only its vector is checked)
            for c in (ctx, other) if door == "resident" else (ctx,):
                cov, prg = c.coverage()
                assert np.array_equal(cov, ocov) and np.array_equal(prg, oprg), (name, door)
                if name == "ragged" or c is ctx:
                    first = first or c.counters()
                    assert c.counters() == first, (name, door)
        assert first["reads"] == len(offs) - 1 and first["bases"] == int(offs[-1])
        assert first["hits"] == ocnt["hits"] and first["clusters_kept"] == ocnt["clusters_kept"] and first["hits_kept"] == ocnt["hits_kept"]
    ctx.close()
    other.close()
