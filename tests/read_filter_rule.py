"""The read filter's rule (include/drprg_hip.h "read filter": drprg_hip_set_read_filter), stated in plain Python and independently of the
product: what the tests of the filter expect comes from here and from the oracle on the reads this rule keeps, never from the code under
test.  Also the fixtures the GPU tests filter -- lengths and qualities only, so that their census can be taken without a device.

The rule is this build's own, stated from memory of what nanoq and chopper compute: nothing in the reference pins it."""
from decimal import ROUND_HALF_UP, Decimal, getcontext

import numpy as np

getcontext().prec = 60

MAX_QUAL = 93
TWO31 = Decimal(2) ** 31


def _e(q_tenths_of_milli):
    """round(2^31 * 10^(-q / 10)) for q given as q * 10000 (an integer), half up, in decimal arithmetic"""
    x = TWO31 * (Decimal(10) ** (Decimal(-q_tenths_of_milli) / Decimal(100000)))
    return int(x.to_integral_value(rounding=ROUND_HALF_UP))


E = [_e(q * 10000) for q in range(MAX_QUAL + 1)]
E_NP = np.array(E, dtype=np.uint64)


def qual_milli(q):
    """a decimal mean quality as thousandths"""
    return int((Decimal(str(q)) * 1000).to_integral_value(rounding=ROUND_HALF_UP))


def threshold(min_qual_milli):
    """T of the rule, in decimal arithmetic (the product computes a fractional one in double: it may differ from this by one)"""
    return E[min_qual_milli // 1000] if min_qual_milli % 1000 == 0 else _e(min_qual_milli * 10)


def qual_sum(quals):
    """S of a read: the sum of E over its Phred qualities"""
    q = np.asarray(quals, dtype=np.int64)
    assert q.size == 0 or (0 <= q.min() and q.max() <= MAX_QUAL)
    return int(E_NP[q].sum(dtype=np.uint64)) if q.size else 0


KEEP, SHORT, LONG, LOWQ = "keep", "short", "long", "lowq"


def fate(length, quals, min_len=0, max_len=0, T=0):
    """what the rule does with one read; T = 0: no quality test (quals may then be None)"""
    if length < min_len:
        return SHORT
    if max_len != 0 and length > max_len:
        return LONG
    if T != 0 and qual_sum(quals) > length * T:
        return LOWQ
    return KEEP


def fates(lengths, quals, min_len=0, max_len=0, T=0):
    return [fate(int(l), None if quals is None else quals[i], min_len, max_len, T) for i, l in enumerate(lengths)]


def census(f):
    """the seven counts of drprg_hip_read_filter_info from the fates and lengths: pass (fates, lengths)"""
    what, lengths = f
    kept = [int(l) for w, l in zip(what, lengths) if w == KEEP]
    return dict(reads_seen=len(what), bases_seen=int(sum(int(l) for l in lengths)), dropped_short=what.count(SHORT), dropped_long=what.count(LONG),
                dropped_low_qual=what.count(LOWQ), reads_kept=len(kept), bases_kept=sum(kept))


# ---- the fixtures of tests/test_gpu_read_filter.py ----------------------------------------------------------------------------------------
MIN_LEN, MAX_LEN, MIN_QUAL = 200, 5000, 10  # the settings the samples below are filtered with


def sample(n_short, n_long, seed):
    """lengths and qualities of a sample of short reads (150-400 bases) and long ones (3-9 kb) in random order.  Qualities: most reads are
    good (15-40 per base), a quarter bad (2-12), and a few sit on the threshold of MIN_QUAL = 10 -- every base at 10 (S = L * T: kept), the
    same with one base at 9 (dropped), a read of 0s and 93s that passes, one of 93s with enough 0s to fail."""
    rng = np.random.default_rng(seed)
    lengths = np.concatenate([rng.integers(150, 401, size=n_short), rng.integers(3000, 9001, size=n_long)])
    rng.shuffle(lengths)
    quals = []
    for i, L in enumerate(int(x) for x in lengths):
        kind = i % 40
        if kind == 7:
            q = np.full(L, 10)
        elif kind == 17:
            q = np.full(L, 10)
            q[L // 2] = 9
        elif kind == 27:
            q = np.full(L, 93)
            q[:L // 11] = 0  # mean error just above 1 / 11 < 0.1: passes Q 10
        elif kind == 37:
            q = np.full(L, 93)
            q[:L // 9 + 1] = 0  # above 1 / 9 > 0.1: fails
        elif rng.random() < 0.27:
            q = rng.integers(2, 13, size=L)
        else:
            q = rng.integers(15, 41, size=L)
        quals.append(q.astype(np.uint8))
    return [int(x) for x in lengths], quals


def small_sample():
    """under 750 000 bases: the ingest hands such a file over as one block"""
    return sample(350, 80, seed=31)


def big_sample():
    """well over 750 000 bases: several blocks"""
    return sample(1000, 250, seed=32)


TILE = 16384   # bytes of the quality buffer per workgroup of read_qual_kernel
SLOTS = 1024   # per-workgroup sums it keeps in LDS: a tile's reads beyond them go to global memory one by one


def overflow_batch(seed=17):
    """lengths of a batch that sends read_qual_kernel down its overflow route, in three tiles.  The first holds 1 300 reads of 1 to 15 bases
    (lane pieces of 16 bytes hold up to 16 reads) and is filled to its edge: more read starts than the kernel has slots, so the sums of the
    reads beyond them go to global memory one by one.  Exactly on that edge a run of 1 100 empty reads starts, followed by a read with bases.
    That run does NOT overflow the second tile: the kernel takes as a tile's first read the LAST read that starts at or before the tile's
    first byte, which is the read behind the run (slot 0), and no workgroup touches the empty reads -- what the run holds the kernel to is
    that search, and sums of 0 for reads nobody visits.  The second tile's last lane piece holds the start of a read that ends in the third.
    Returns (lengths, index of the read behind the empty run, index of the straddler)"""
    rng = np.random.default_rng(seed)
    L = [int(x) for x in rng.integers(1, 16, size=1300)]
    L[:16] = [1] * 16  # one lane piece of sixteen reads
    while TILE - sum(L) > 300:
        L.append(int(rng.integers(20, 300)))
    L.append(TILE - sum(L))
    L += [0] * 1100
    behind = len(L)
    L.append(40)
    while 2 * TILE - 8 - sum(L) > 300:
        L.append(int(rng.integers(1, 300)))
    L.append(2 * TILE - 8 - sum(L))
    straddler = len(L)
    L += [100, 0, 7, 1, 333]
    return L, behind, straddler
