"""The random subsample's rule on the CPU: a census of tests/subsample_rule.py on seeded inputs (its two statements against each other and
against the properties the rule promises), and the executables' handling of --subsample-covg / --seed, which fails before any device is
opened."""
import os
import subprocess

import numpy as np
import pytest

from subsample_rule import keep_flags, keep_flags_blocks, key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lengths(seed, n=600, zero_runs=True):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 401, size=n)
    if zero_runs:
        for at in rng.integers(0, n - 8, size=6):
            L[at:at + int(rng.integers(1, 8))] = 0
        L[:2] = 0
        L[-3:] = 0
    return [int(x) for x in L]


def _key_order(n, seed):
    return sorted(range(n), key=lambda i: (key(seed, i), i))


def test_key_is_splitmix64_of_the_weyl_sequence():
    # splitmix64's published first outputs for state 0: the finaliser of 1 x GOLDEN, 2 x GOLDEN, 3 x GOLDEN
    assert [key(0, i) for i in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert len({key(7, i) for i in range(20000)}) == 20000


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 64 - 1])
def test_census(seed):
    L = _lengths(seed)
    S, n = sum(L), len(L)
    order = _key_order(n, seed)
    for T in (S, S + 1, 10 * S):  # sum <= T keeps all, sum == T included
        assert keep_flags(L, T, seed) == [1] * n
    for T in (S - 1, S // 2, S // 10, S * 999 // 1000, 1, 0):
        flags = keep_flags(L, T, seed)
        kept = [i for i in order if flags[i]]
        assert kept == order[:len(kept)] and kept  # a prefix of the key order, never empty
        total = sum(L[i] for i in kept)
        assert total >= T
        if T > 0:
            assert total - L[kept[-1]] < T  # without the last read in key order the target is missed
        else:
            assert kept == order[:1]  # T = 0: exactly the first read in key order
    # T = 1: the reads in key order up to and including the first that holds a base
    flags = keep_flags(L, 1, seed)
    first = next(j for j, i in enumerate(order) if L[i] > 0)
    assert [i for i in range(n) if flags[i]] == sorted(order[:first + 1])


def test_two_seeds_select_differently():
    L = _lengths(3)
    a, b = keep_flags(L, sum(L) // 2, 1), keep_flags(L, sum(L) // 2, 2)
    assert a != b and 0 < sum(a) < len(L) and 0 < sum(b) < len(L)


def test_equal_lengths():
    L = [150] * 1000
    for T, want in ((150 * 1000, 1000), (150 * 1000 - 1, 1000), (150 * 999, 999), (150 * 999 + 1, 1000), (150 * 500, 500), (150 * 500 - 149, 500), (1, 1), (0, 1)):
        flags = keep_flags(L, T, 9)
        assert sum(flags) == want, T
        assert [i for i in range(1000) if flags[i]] == sorted(_key_order(1000, 9)[:want])


def test_zero_length_reads_take_part():
    L = [0, 0, 5, 0, 7, 0, 0, 3, 0]
    assert keep_flags(L, 15, 4) == [1] * 9 and keep_flags([0, 0, 0], 0, 4) == [1, 1, 1]
    for T in range(0, 15):
        flags = keep_flags(L, T, 4)
        order = _key_order(9, 4)
        kept = [i for i in order if flags[i]]
        assert kept == order[:len(kept)]
        # the empty reads in front of the cut in key order are kept, those behind it are not
        assert all(flags[i] for i in order[:len(kept)]) and not any(flags[i] for i in order[len(kept):])


@pytest.mark.parametrize("seed", [5, 6])
def test_any_block_partition_gives_the_same_flags(seed):
    L = _lengths(seed, n=900)
    rng = np.random.default_rng(seed)
    for T in (sum(L) // 3, sum(L) - 1, sum(L), 0, 1):
        want = keep_flags(L, T, seed)
        for cuts in ([], [1], [899], [300, 600], sorted(rng.integers(0, 901, size=7).tolist()), [0, 0, 450, 450, 900]):
            edges = [0] + list(cuts) + [900]
            blocks = [L[edges[i]:edges[i + 1]] for i in range(len(edges) - 1)]
            got = keep_flags_blocks(blocks, T, seed)
            assert [len(g) for g in got] == [len(b) for b in blocks]
            assert [int(x) for g in got for x in g] == want, (T, cuts)


# ---- the executables' arguments: usage errors, exit 2, before anything is opened (the files named do not exist) ----------------------
def _exe(name):
    from util import ensure_built
    ensure_built()
    return os.path.join(ROOT, "drprg_amd", "bin", name)


@pytest.mark.parametrize("cmd", ["map", "discover"])
def test_pandora_refuses_both_sampling_rules_at_once(cmd, tmp_path):
    missing = str(tmp_path / "no_such.prg")
    r = subprocess.run([_exe("pandora"), cmd, "--max-covg", "9", "--subsample-covg", "10", "-o", str(tmp_path / "out"), missing, missing], capture_output=True, text=True)
    assert r.returncode == 2 and "--max-covg and --subsample-covg are alternatives" in r.stderr, r.stderr
    assert "cannot open" not in r.stderr and not (tmp_path / "out").exists()
    # either order; "no cap" beside it is not a conflict (that run gets as far as the missing index: exit 1)
    r = subprocess.run([_exe("pandora"), cmd, "--subsample-covg", "10", "--seed", "7", "--max-covg", "300", missing, missing], capture_output=True, text=True)
    assert r.returncode == 2 and "alternatives" in r.stderr
    r = subprocess.run([_exe("pandora"), cmd, "--subsample-covg", "10", "--max-covg", "4294967295", "-o", str(tmp_path / "o2"), missing, missing], capture_output=True,
                       text=True)
    assert r.returncode == 1 and "alternatives" not in r.stderr


@pytest.mark.parametrize("argv", [["pandora", "map"], ["pandora", "discover"], ["drprg", "predict", "-x", "no_such_index", "-i", "no_such_reads"]])
def test_seed_without_subsample_covg_is_a_usage_error(argv, tmp_path):
    r = subprocess.run([_exe(argv[0])] + argv[1:] + ["--seed", "3"] + (["a", "b"] if argv[0] == "pandora" else []), capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2 and "--seed belongs to --subsample-covg" in r.stderr, r.stderr
    assert "does not exist" not in r.stderr and "cannot open" not in r.stderr


def test_subsample_covg_needs_a_number(tmp_path):
    for exe, head in (("pandora", ["map"]), ("drprg", ["predict"])):
        r = subprocess.run([_exe(exe)] + head + ["--subsample-covg", "ten"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 2 and "--subsample-covg needs a depth" in r.stderr, r.stderr
