"""The filter tiers of the filtered sequence on both sides of every step of their sizes, against the oracle (pytest -m gpu).

The panels and batches come from tests/filter_tiers.py (their census is held on the CPU by tests/test_filter_tiers.py): indexes of exactly the
record counts at which PrgIndex::flatten changes an array's size, the tier or the bits of the middle tier's level 0, and one record more.
Every case first asserts what Context.table_tier() reports -- sketch_form, lds_filter_bytes, l2_filter_bytes against the restated size rules
-- and then maps the panel's one batch through test_gpu_parity._compare: ASCII and packed, coverage vector, reads per PRG and counters
bit-exact.  The small tier runs with its second stage as the input format chooses, in LDS and in the L2.  The batches are dense with hits
(w = 1), so the buffers start larger than a batch needs (DRPRG_HIP_MIN_CAPACITY) and nothing is said about reruns."""
import pytest

import filter_tiers as F
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

THREADS = min(8, P.ORACLE_THREADS)
CAPACITY = 1 << 23          # entries: the largest batch has 3.9 M bases, every one a candidate
_ORACLE_MAP = {}


def _open(tmp_path, monkeypatch, panel, w, k, kernel=0, stage2=None, mid_max=F.MID_MAX_RECORDS):
    """a context opened with the switches set or unset (they are read when a context opens)"""
    monkeypatch.setenv("DRPRG_HIP_MIN_CAPACITY", str(CAPACITY))
    for name, value in (("DRPRG_FILTER_STAGE2", stage2), ("DRPRG_MID_MAX_RECORDS", str(mid_max) if mid_max != F.MID_MAX_RECORDS else None)):
        if value:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)
    monkeypatch.delenv("DRPRG_FORCE_MID_TIER", raising=False)
    return P._ctx(tmp_path, panel, w, k, True, kernel=kernel, min_cluster_size=F.MCS)


def _compare(monkeypatch, ctx, oracle, case, w, k, what):
    """test_gpu_parity._compare on the case's batch; the oracle maps a batch once however many contexts it is compared with"""
    bases, offs, _ = F.batch_of(oracle, case)
    plain = P._oracle_map

    def once(orc, idx, b, o, w_, k_, illumina, min_cluster_size=10, threads=1):
        if case not in _ORACLE_MAP:
            _ORACLE_MAP.clear()
            _ORACLE_MAP[case] = plain(orc, idx, b, o, w_, k_, illumina, min_cluster_size, THREADS)
        return _ORACLE_MAP[case]

    filtered = ctx.table_tier()["sketch_form"] in F.FILTER_FORMS.values()
    with monkeypatch.context() as m:
        m.setattr(P, "_oracle_map", once)
        try:
            cnt = P._compare(ctx, oracle, bases, offs, w, k, True, 2 if filtered else 3, min_cluster_size=F.MCS, threads=THREADS)
        except AssertionError as e:
            raise AssertionError(f"{what}: {ctx.table_tier()}, the device's counters of its last map {ctx.counters()}: {e}") from e
    assert cnt["hits"] > 30_000 and cnt["clusters_kept"] > 0, (what, cnt)
    return cnt


def _assert_tier(ctx, n_records, k, mid_max, what):
    """the context serves the index from the tier, and with the array sizes, that the restated rules give for its records"""
    tier, lds_bytes, l2_bytes = F.tier_sizes(n_records, k, mid_max)
    got = ctx.table_tier()
    assert ctx.n_records == n_records, (what, ctx.n_records)
    if tier is None:
        assert got["sketch_form"] not in F.FILTER_FORMS.values() and got["kernel"] != 2, (what, got)
    else:
        assert got["sketch_form"] == F.FILTER_FORMS[tier] and got["kernel"] == 2, (what, got)
    assert (got["lds_filter_bytes"], got["l2_filter_bytes"]) == (lds_bytes, l2_bytes), (what, got, lds_bytes, l2_bytes)
    return tier


def _assert_no_tier(ctx, n_records, what):
    got = ctx.table_tier()
    assert ctx.n_records == n_records and got["sketch_form"] not in F.FILTER_FORMS.values() and got["kernel"] != 2 and got["l2_filter_bytes"] == 0, (what, got)


def _run_case(tmp_path, oracle, monkeypatch, case, what=None):
    what = what or case
    panel, w, k, n_records, mid_max = F.panel_of(oracle, case)
    tier = F.tier_of(n_records, k, mid_max)
    for stage2 in (None,) + (F.forms_of(tier) if tier == "level0" else ()):
        ctx = _open(tmp_path, monkeypatch, panel, w, k, stage2=stage2, mid_max=mid_max)
        assert _assert_tier(ctx, n_records, k, mid_max, what) == tier
        _compare(monkeypatch, ctx, oracle, case, w, k, f"{what} (w={w}, k={k}), {n_records} records, second stage {stage2 or 'by format'}")
        ctx.close()
    return panel, w, k, n_records


@pytest.mark.parametrize("case", F.all_cases())
def test_the_filter_tier_on_each_side_of_each_step(tmp_path, oracle, monkeypatch, case):
    panel, w, k, n_records = _run_case(tmp_path, oracle, monkeypatch, case)
    # ---- the form on the far side of the edges where the filtered sequence begins or ends ----
    if case in ("direct-below", "none_k13-below", "none_k11-below"):   # the last index a tier serves, through the direct sequence
        ctx = _open(tmp_path, monkeypatch, panel, w, k, kernel=3)
        _assert_no_tier(ctx, n_records, case)
        _compare(monkeypatch, ctx, oracle, case, w, k, f"{case}, direct sequence")
        ctx.close()
    if case == "direct-above":                                         # the first index the middle tier leaves to the direct sequence, through it
        ctx = _open(tmp_path, monkeypatch, panel, w, k, mid_max=F.MID0_MAX_RECORDS)
        assert _assert_tier(ctx, n_records, k, F.MID0_MAX_RECORDS, case) == "middle"
        _compare(monkeypatch, ctx, oracle, case, w, k, f"{case}, middle tier")
        ctx.close()
    if case in ("none_k13-above", "none_k11-above"):                   # no array is built past this edge: the filtered sequence is refused
        from drprg_amd import DependencyError
        ctx = _open(tmp_path, monkeypatch, panel, w, k)
        with pytest.raises(DependencyError):
            ctx.set_opts(illumina=True, genome_size=20000, kernel=2, min_cluster_size=F.MCS)
        ctx.close()


def test_one_context_after_another_across_the_level0_edge(tmp_path, oracle, monkeypatch):
    """no array of a closed context is left in use and the tier does not stick: all-LDS, middle tier, all-LDS again, in one process"""
    for step, side in enumerate(("below", "above", "below")):
        _run_case(tmp_path, oracle, monkeypatch, f"level0-{side}", f"context {step + 1} of 3, level0-{side}")
