"""Read trimming's rule (include/drprg_hip.h "read trimming": drprg_hip_set_read_trim), stated in plain Python and independently of the
product: what the tests of the trimming expect comes from here and from the oracle on the reads this rule leaves, never from the code
under test.  Also the fixtures the GPU tests trim -- lengths, qualities and reverse flags only, so that their census can be taken without
a device.

The rule is this build's own, stated from memory of what fastp (--cut_front --cut_tail, -f, -t) and Trimmomatic (LEADING, TRAILING) compute:
nothing in the reference pins it.  The window test compares the MEAN PHRED VALUE of a window, not the mean error probability the read
filter uses."""
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

MAX_QUAL = 93
MAX_QUAL_MILLI = 93000
MAX_WINDOW = 32
DEFAULT_WINDOW = 4


def qual_milli(q):
    """a decimal quality as thousandths"""
    return int((Decimal(str(q)) * 1000).to_integral_value(rounding=ROUND_HALF_UP)) if q else 0


def kept_range(quals, length, front=0, tail=0, milli=0, window=0):
    """[a, b) of one read in read orientation; quals: its Phred values in read orientation (may be None when milli == 0)"""
    L = int(length)
    W = (window or DEFAULT_WINDOW) if milli else 0
    a0 = min(front, L)
    b0 = L - min(tail, L - a0)
    if not milli:
        return (a0, b0) if a0 < b0 else (0, 0)
    q = [int(x) for x in quals]
    assert len(q) == L
    good = [i for i in range(a0, b0 - W + 1) if 1000 * sum(q[i:i + W]) >= milli * W]
    if not good:
        return (0, 0)
    a, b = good[0], good[-1] + W
    while a < b and 1000 * q[a] < milli:
        a += 1
    while b > a and 1000 * q[b - 1] < milli:
        b -= 1
    return (a, b) if a < b else (0, 0)


def kept_range_stored(stored_quals, length, reverse, front=0, tail=0, milli=0, window=0):
    """the same from the qualities in STORED order (a BAM record with flag 0x10 stores them mirrored): trim the stored order with front and
    tail swapped, then mirror the range"""
    if not reverse:
        return kept_range(stored_quals, length, front, tail, milli, window)
    L = int(length)
    a, b = kept_range(stored_quals, L, tail, front, milli, window)
    return (L - b, L - a) if a < b else (0, 0)


UNTOUCHED, FRONT, TAIL, BOTH, EMPTY_CROP, EMPTY_QUAL, SHORTER_THAN_W = "untouched", "front", "tail", "both", "emptied by crop", "emptied by quality", "shorter than W"
CLASSES = (UNTOUCHED, FRONT, TAIL, BOTH, EMPTY_CROP, EMPTY_QUAL, SHORTER_THAN_W)


def classify(length, rng, front=0, tail=0, milli=0, window=0):
    """what the quality trimming did to a read behind its fixed crop [a0, b0) (without crops: to the read)"""
    L = int(length)
    a, b = rng
    W = (window or DEFAULT_WINDOW) if milli else 0
    a0 = min(front, L)
    b0 = L - min(tail, L - a0)
    if a == b:
        if L == 0:
            return UNTOUCHED
        if a0 == b0:
            return EMPTY_CROP
        return SHORTER_THAN_W if b0 - a0 < W else EMPTY_QUAL
    if a == a0 and b == b0:
        return UNTOUCHED
    if a > a0 and b < b0:
        return BOTH
    return FRONT if a > a0 else TAIL


def info(lengths, ranges, front=0, tail=0):
    """the eight counts of drprg_hip_read_trim_info"""
    out = dict(reads_seen=len(lengths), bases_seen=int(sum(lengths)), reads_lost_base=0, cut_front=0, cut_tail=0, qual_cut_front=0, qual_cut_tail=0, reads_emptied=0)
    for L, (a, b) in zip(lengths, ranges):
        L = int(L)
        a0 = min(front, L)
        b0 = L - min(tail, L - a0)
        out["reads_lost_base"] += (b - a) != L
        out["cut_front"] += a0
        out["cut_tail"] += L - b0
        if a < b:
            out["qual_cut_front"] += a - a0
            out["qual_cut_tail"] += b0 - b
        else:
            out["qual_cut_front"] += b0 - a0  # (a read without a good window: its cropped bases count at the front)
            out["reads_emptied"] += L > 0
    return out


# ---- the fixtures of tests/test_gpu_read_trim.py ---------------------------------------------------------------------------------------------
FRONT_N, TAIL_N, QUAL, WINDOW = 5, 3, 20, 4  # --trim-front 5 --trim-tail 3 --trim-qual 20 (W = 4)


def sample(n_short, n_long, seed):
    """lengths, qualities (read orientation) of short reads (150-400 bases) and long ones (3-9 kb) in random order: a good middle (25-40)
    with, by turns, nothing bad, a bad start, a bad end, both, everything bad; and a few reads of 0..8 bases, which the crop or the window
    empties"""
    rng = np.random.default_rng(seed)
    lengths = np.concatenate([rng.integers(150, 401, size=n_short), rng.integers(3000, 9001, size=n_long)])
    rng.shuffle(lengths)
    lengths[3::50] = rng.integers(0, 9, size=len(lengths[3::50]))
    lengths[4] = 8   # emptied by the crop: front 5 + tail 3
    lengths[5] = 10  # two bases behind the crop: shorter than W
    quals = []
    for i, L in enumerate(int(x) for x in lengths):
        q = rng.integers(25, 41, size=L)
        kind = i % 8
        n_bad_front = int(rng.integers(8, 60)) if kind in (1, 3) else 0
        n_bad_tail = int(rng.integers(8, 90)) if kind in (2, 3, 6) else 0
        if kind == 4 and i % 16 == 4:
            q[:] = rng.integers(2, 12, size=L)
        q[:min(n_bad_front, L)] = rng.integers(2, 15, size=min(n_bad_front, L))
        if n_bad_tail:
            q[max(L - n_bad_tail, 0):] = rng.integers(2, 15, size=min(n_bad_tail, L))
        quals.append(q.astype(np.uint8))
    return [int(x) for x in lengths], quals


def small_sample():
    """under 750 000 bases: the ingest hands such a file over as one block"""
    return sample(350, 80, seed=51)


def big_sample():
    """well over 750 000 bases: several blocks"""
    return sample(1000, 250, seed=52)


def reverse_flag(i):
    """which records the BAM fixtures store on the reverse strand (as tests/test_gpu_read_filter.py writes them)"""
    return i % 3 == 0


def sample_ranges(lengths, quals, front=FRONT_N, tail=TAIL_N, qual=QUAL, window=WINDOW):
    m = qual_milli(qual)
    return [kept_range(quals[i] if m else None, L, front, tail, m, window) for i, L in enumerate(lengths)]


def kernel_batch(W):
    """the ragged batch of the kernel test, about four tiles of 16 384 quality bytes: (lengths, qualities in stored order, reverse flags,
    milli).  Q is 20.5, so windows of W bases at 21 are good and at 20 are not; see the comments for what each read is there for."""
    TILE = 16384
    milli = 20500
    rng = np.random.default_rng(7 + W)
    L, Q = [], []

    def add(q):
        q = np.asarray(q, dtype=np.uint8)
        L.append(int(q.size))
        Q.append(q)

    def pos():
        return int(sum(L))

    good, bad = 30, 10
    for n in (0, 1, W - 1, W, W + 1):  # reads of 0, 1, W - 1, W and W + 1 bases, all good
        add(np.full(n, good))
    add(np.full(0, good))
    # lane pieces of 16 bytes that hold two and three reads
    for n in (7, 9, 5, 5, 6, 16, 3, 13):
        add(rng.integers(15, 30, size=n))
    # all-good and all-bad reads
    add(np.full(300, good))
    add(np.full(300, bad))
    # a window sum exactly on the threshold (kept) and one below (not kept): W bases summing to ceil(20.5 W), the rest bad
    for delta in (0, -1):
        q = np.full(64, bad)
        need = -(-milli * W // 1000) + delta
        w = np.full(W, need // W)
        w[:need - int(w.sum())] += 1
        q[20:20 + W] = w
        add(q)
    # front + tail >= L (with the crops of the test: 5 + 3)
    add(np.full(8, good))
    add(np.full(6, good))
    # reads whose first good window starts on the first and on the last lane of a wave: pad to a wave edge (1024 bytes), then place it
    for lane in (0, 63):
        add(np.full((-pos()) % 1024 or 1024, bad))
        q = np.full(2048, bad)
        q[lane * 16 + 15:lane * 16 + 15 + 2 * W] = good  # (starts in that lane's last byte and runs into the next lane's)
        add(q)
    # a read that starts in one tile and ends in the next, its only good window straddling the tile edge
    add(np.full(TILE - 100 - pos(), 28))
    q = np.full(200, bad)
    at = 100 - W // 2 if W > 1 else 99
    q[at:at + W] = good
    add(q)
    assert pos() == TILE + 100
    # a run of more than 1 024 reads of 1..15 bases inside one tile: the overflow route
    for _ in range(1300):
        n = int(rng.integers(1, 16))
        add(rng.integers(12, 32, size=n))
    assert pos() < 2 * TILE - 200
    # a read over three tiles whose only good window lies in the middle one
    q = np.full(2 * TILE + 300, bad)
    mid = 2 * TILE + 5000 - pos()
    first = pos()
    q[mid:mid + W + 3] = good
    add(q)
    assert first < 2 * TILE and first + q.size > 3 * TILE
    # random reads to the end of the fourth tile
    while pos() < 4 * TILE - 700:
        n = int(rng.integers(20, 600))
        q = rng.integers(5, 41, size=n)
        add(q)
    rev = [i % 3 == 1 for i in range(len(L))]
    return L, Q, rev, milli
