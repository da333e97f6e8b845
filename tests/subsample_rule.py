"""The random subsample's rule (include/drprg_hip.h "random subsample"), stated twice and independently of the product: what the tests of
drprg_hip_subsample expect comes from here and from the oracle on the selected reads, never from the code under test."""
import numpy as np

MASK = 2 ** 64 - 1
GOLDEN = 0x9E3779B97F4A7C15
DEFAULT_SEED = 1  # the executables' --seed when none is given


def key(seed, i):
    """splitmix64(seed + GOLDEN * (i + 1)) in 64-bit unsigned arithmetic"""
    z = (seed + GOLDEN * (i + 1)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def keep_flags(lengths, target, seed):
    """lengths in, one keep flag per read out: everything if the sum is at most the target, else the reads in (key, i) order up to and
    including the first at which the running sum reaches the target"""
    lengths = [int(x) for x in lengths]
    if sum(lengths) <= target:
        return [1] * len(lengths)
    flags, total = [0] * len(lengths), 0
    for i in sorted(range(len(lengths)), key=lambda i: (key(seed, i), i)):
        flags[i] = 1
        total += lengths[i]
        if total >= target:
            break
    return flags


def keep_flags_blocks(blocks, target, seed):
    """the same from numpy, for reads that arrive in blocks (lists of lengths): numbered through the blocks, one flag array per block"""
    lengths = np.concatenate([np.asarray(b, dtype=np.uint64) for b in blocks]) if blocks else np.zeros(0, np.uint64)
    n = lengths.size
    flags = np.ones(n, dtype=np.uint8)
    if int(lengths.sum(dtype=np.uint64)) > target:
        with np.errstate(over="ignore"):
            z = np.uint64(seed) + np.uint64(GOLDEN) * (np.arange(n, dtype=np.uint64) + np.uint64(1))
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        order = np.lexsort((np.arange(n), z))
        cut = int(np.searchsorted(np.cumsum(lengths[order], dtype=np.uint64), np.uint64(target), side="left"))
        flags[:] = 0
        flags[order[:cut + 1]] = 1
    ends = np.cumsum([len(b) for b in blocks])
    return [f for f in np.split(flags, ends[:-1])] if blocks else []
