"""The depth cap's rule (include/drprg_hip.h: drprg_hip_set_max_covg), stated twice and independently of the product: what the tests of
the cap expect comes from here and from the oracle on the accepted reads, never from the code under test.

[UPSTREAM-MEMORY] pandora's read loop is not part of the reference tree; the loop below is the rule as recalled, nothing in the reference
pins it."""
import numpy as np

OFF = 2 ** 32 - 1  # this value and anything above it: no cap


def pandora_loop(lengths, genome_size, max_covg, total=0):
    """reads in order, each read's length added to a running total; stop after the first read for which total // genome_size > max_covg.
    Returns how many reads were taken."""
    n = 0
    for length in lengths:
        total += int(length)
        n += 1
        if max_covg < OFF and total // genome_size > max_covg:
            break
    return n


def accepted_reads(lengths, genome_size, max_covg, total=0):
    """the same from np.cumsum: T = (max_covg + 1) * genome_size, n = the smallest i with B(i) >= T (B counted from `total`, what the
    context has mapped already), all reads if there is none.  Returns (n, bases of those n reads, cap reached)."""
    lengths = np.asarray(lengths, dtype=np.uint64)
    B = np.cumsum(lengths, dtype=np.uint64)
    if max_covg >= OFF or lengths.size == 0:
        return int(lengths.size), int(B[-1]) if lengths.size else 0, False
    T = (max_covg + 1) * genome_size
    if total >= T:
        return 0, 0, True
    i = int(np.searchsorted(B, np.uint64(T - total), side="left"))
    if i == lengths.size:
        return int(lengths.size), int(B[-1]), False
    return i + 1, int(B[i]), True
