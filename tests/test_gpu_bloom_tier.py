"""Every direct form behind the Bloom tier and on the large probe table, against the oracle (pytest -m gpu).

The panels and batches come from tests/bloom_tier.py (their census is held on the CPU by tests/test_bloom_tier.py): indexes of 70 000 ..
125 000 keys at the (w, k) of each sketch form, and indexes of exactly 65 535 | 65 536 | 65 537 keys, where the table doubles and the tier
appears.  Everything goes through test_gpu_parity._ctx / _compare: ASCII and packed, vectors and counters bit-exact; a difference names
(w, k), the kernel sequence, the sketch form and the reads the per-read kernel left over."""
import pytest

import bloom_tier as B
from test_gpu_parity import FORCED_GENERIC, ORACLE_THREADS, _compare, _ctx, _oracle_index

pytestmark = pytest.mark.gpu

THREADS = min(8, ORACLE_THREADS)


def _open(tmp_path, monkeypatch, panel, w, k, kernel, direct_form=None):
    """a context opened with DRPRG_DIRECT_FORM set or unset; the switch stays for the test (a context reads it again at every reset)"""
    if direct_form:
        monkeypatch.setenv("DRPRG_DIRECT_FORM", direct_form)
    else:
        monkeypatch.delenv("DRPRG_DIRECT_FORM", raising=False)
    return _ctx(tmp_path, panel, w, k, True, kernel=kernel, min_cluster_size=B.MCS)


def _assert_tables(ctx, oracle, w, k, bits, pbloom_words, what):
    tier = ctx.table_tier()
    assert ctx.n_keys == len(_oracle_index(oracle, ctx.prg_strings, w, k)["keys"]), what
    assert ctx.n_slots == 1 << bits, (what, ctx.n_slots)
    assert tier["pbloom_words"] == pbloom_words, (what, tier)
    assert tier["table_bytes"] == B.slot_bytes(k) * ctx.n_slots, (what, tier)
    return tier


def _compare_named(ctx, oracle, bases, offs, w, k, kernel, what):
    try:
        return _compare(ctx, oracle, bases, offs, w, k, True, kernel or 2, min_cluster_size=B.MCS, threads=THREADS)
    except AssertionError as e:
        raise AssertionError(f"{what} (w={w}, k={k}), kernel sequence {kernel}, sketch_form {ctx.table_tier()['sketch_form']}: "
                             f"leftover_reads={ctx.counters()['leftover_reads']}: {e}") from e


@pytest.mark.parametrize("name,kernel,direct_form,form", B.matrix_cases(),
                         ids=[f"{n}-kernel{kn}{'lds' if env else ''}-form{f}" for n, kn, env, f in B.matrix_cases()])
def test_every_direct_form_behind_the_tier(tmp_path, oracle, monkeypatch, name, kernel, direct_form, form):
    w, k = B.MATRIX[name][:2]
    bases, offs = B.matrix_batch(name)
    ctx = _open(tmp_path, monkeypatch, B.matrix_panel(name), w, k, kernel, direct_form)
    n_keys = len(_oracle_index(oracle, ctx.prg_strings, w, k)["keys"])
    tier = _assert_tables(ctx, oracle, w, k, B.table_bits(n_keys), 1 << B.bloom_wbits(n_keys), name)
    assert B.tier_present(n_keys, k) and tier["sketch_form"] == form, (name, kernel, direct_form, tier)
    if kernel == 0:  # the middle tier of the filter: its candidates are verified against the large table
        assert tier["l2_filter_bytes"] > 0, tier
    cnt = _compare_named(ctx, oracle, bases, offs, w, k, kernel, name)
    assert cnt["clusters_kept"] > 1000, (name, cnt)
    if kernel == 3 and not FORCED_GENERIC:  # the long reads outgrow the per-read kernel: the generic pipeline's expand and sort ran behind the tier
        assert ctx.counters()["leftover_reads"] > 0, (name, kernel, direct_form, ctx.counters())
    ctx.close()


def _threshold_case(tmp_path, oracle, monkeypatch, k, n_keys, kernel, what):
    """one context on a threshold panel: its tables are on the expected side of the switch and its batch maps as the oracle maps it"""
    i = B.THRESHOLD_KEYS.index(n_keys)
    bases, offs, _ = B.threshold_batch(oracle, k, n_keys)
    ctx = _open(tmp_path, monkeypatch, B.threshold_panel(oracle, k, n_keys), 1, k, kernel)
    assert ctx.n_keys == n_keys
    tier = _assert_tables(ctx, oracle, 1, k, (17, 18, 18)[i], (0, 1 << 14, 1 << 15)[i], what)
    assert tier["sketch_form"] == (3 if k <= 15 else 4), tier
    cnt = _compare_named(ctx, oracle, bases, offs, 1, k, kernel, what)
    assert cnt["clusters_kept"] > 1000, (what, cnt)
    ctx.close()


@pytest.mark.parametrize("n_keys", B.THRESHOLD_KEYS)
@pytest.mark.parametrize("k", B.THRESHOLD_K)
def test_the_tier_switches_on_at_65536_keys(tmp_path, oracle, monkeypatch, k, n_keys):
    for kernel in (1, 3):
        _threshold_case(tmp_path, oracle, monkeypatch, k, n_keys, kernel, f"{n_keys} keys")


def test_one_context_after_another_across_the_threshold(tmp_path, oracle, monkeypatch):
    """no table and no Bloom array of a closed context is left in use: below the switch, above it, below it again, in one process"""
    for step, n_keys in enumerate((B.THRESHOLD_KEYS[0], B.THRESHOLD_KEYS[2], B.THRESHOLD_KEYS[0])):
        _threshold_case(tmp_path, oracle, monkeypatch, 15, n_keys, 3, f"context {step + 1} of 3, {n_keys} keys")
