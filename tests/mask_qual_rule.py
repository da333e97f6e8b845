"""Base masking's rule (include/drprg_hip.h "base masking": drprg_hip_set_base_mask), stated in plain Python and independently of the
product: what the tests of the masking expect comes from here and from the oracle on the reads this rule leaves, never from the code
under test.  Also the fixtures the GPU tests mask -- lengths, qualities and reverse flags only, so that their census can be taken without
a device.

The rule is this build's own: a base whose Phred quality is below Q becomes the letter N; nothing else changes."""
import numpy as np

MAX_QUAL = 93
ACGT = set(b"ACGTacgt")
TILE, LANE, WORD = 16384, 64, 16  # bases per workgroup and per lane of base_mask_kernel, and per packed word
Q = 10                            # the threshold of the samples
GOOD = 35


def _stored(quals, n, reverse):
    q = np.asarray(quals, dtype=np.int64).reshape(-1)
    assert q.size == n and (q.size == 0 or (0 <= q.min() and q.max() <= MAX_QUAL))
    return q[::-1] if reverse else q


def masked(bases, quals, Q, reverse=False):
    """the read (bytes, read orientation) as the file with N would hold it.  quals: its Phred values -- in read orientation, or, reverse=True,
    in STORED order (a BAM record with flag 0x10 stores them mirrored): base p is then judged by quals[L - 1 - p]"""
    assert 1 <= Q <= MAX_QUAL
    b = np.frombuffer(bytes(bases), dtype=np.uint8).copy()
    b[_stored(quals, b.size, reverse) < Q] = ord("N")
    return b.tobytes()


_IS_BASE = np.zeros(256, dtype=bool)
_IS_BASE[list(ACGT)] = True


def info(reads, quals, Q, rev=None):
    """the five counts of drprg_hip_base_mask_info over reads given as for masked (rev: per read, or None)"""
    out = dict(reads_seen=len(reads), bases_seen=sum(len(r) for r in reads), reads_masked=0, bases_masked=0, bases_already_unknown=0)
    for i, (r, q) in enumerate(zip(reads, quals)):
        b = np.frombuffer(bytes(r), dtype=np.uint8)
        low = b[_stored(q, b.size, rev is not None and bool(rev[i])) < Q]
        out["reads_masked"] += int(low.size > 0)
        out["bases_masked"] += int(_IS_BASE[low].sum())
        out["bases_already_unknown"] += int((~_IS_BASE[low]).sum())
    return out


# ---- the fixtures of tests/test_gpu_base_mask.py --------------------------------------------------------------------------------------------
def _dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)) if n else b""


def kernel_batch(listed=True, low=True):
    """the ragged batch of the kernel test, a little over three tiles of 16 384 bases: (reads in read orientation, qualities in STORED order,
    reverse flags).  listed: some bases are not ACGT before the mask; low: some qualities are below Q = 10.  See the comments for what each
    read is there for."""
    rng = np.random.default_rng(91)
    reads, quals, rev = [], [], []

    def pos():
        return sum(len(r) for r in reads)

    def add(n, q=None, r=None, reverse=None):
        q = rng.choice([GOOD, GOOD, GOOD, 30, 40, Q, Q - 1, 2, 5], size=n, p=[.3, .3, .2, .07, .07, .02, .02, .01, .01]) if q is None else np.asarray(q)
        assert len(q) == n
        reads.append(_dna(rng, n) if r is None else r)
        quals.append(q.astype(np.uint8))
        rev.append(len(reads) % 3 == 1 if reverse is None else reverse)  # (random qualities: asymmetric, so a mirrored read shows)
        return len(reads) - 1

    for n in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 0, 0):  # the word and lane edges as read lengths; empty reads
        add(n)
    add(1, [2], reverse=False)                                 # one base, masked
    add(200, np.full(200, 2))                                  # masked entirely
    add(200, np.full(200, GOOD))                               # nothing masked
    q = np.full(150, GOOD)
    q[0], q[-1] = Q - 1, 2                                     # the first and the last base of a read
    add(150, q, reverse=False)
    q = np.full(150, GOOD)
    q[0], q[1] = 3, Q                                          # stored order: a reversed read is masked at its LAST base only
    add(150, q, reverse=True)
    # a base that is not ACGT with a low quality (listed already), and a listed base of good quality right beside a masked one
    r = bytearray(_dna(rng, 100))
    q = np.full(100, GOOD)
    r[10:11], q[10] = b"N", 2
    r[40:41], q[41] = b"R", 4
    r[70:72], q[70], q[71] = b"ny", 2, GOOD
    add(100, q, bytes(r), reverse=False)
    # the first and the last base of a 16-base word and of a lane's 64 bases, in a forward read and in a reversed one
    for reverse in (False, True):
        start, n = pos(), 400
        q = np.full(n, GOOD)
        for p in range(start, start + n):
            if p % WORD in (0, WORD - 1) and (p // WORD) % 3 == 0 or p % LANE in (0, LANE - 1):
                q[n - 1 - (p - start) if reverse else p - start] = 2
        add(n, q, reverse=reverse)
    # a read that straddles the first tile edge, low on both sides of it, and a read longer than a tile
    n = TILE - pos() + 300
    q = np.full(n, GOOD)
    q[n - 301:n - 298] = 2
    add(n, q, reverse=False)
    assert pos() == TILE + 300
    add(TILE + 777)
    add(0)
    while pos() < 3 * TILE + 1000:  # short reads to behind the third tile edge
        add(int(rng.integers(1, 300)))
    # the first and the last base of the block
    quals[1][0] = 2
    quals[-1][0 if rev[-1] else -1] = 2
    if listed:  # letters that are no bases, here and there, of either case and in reads of either strand
        for i in range(25, len(reads), 7):
            if len(reads[i]) > 3:
                r = bytearray(reads[i])
                r[len(r) // 2:len(r) // 2 + 1] = b"NRnYKM"[i % 6:i % 6 + 1]
                reads[i] = bytes(r)
    else:
        reads = [r.translate(bytes.maketrans(b"NRYKMnry", b"ACGTACGT")) for r in reads]
    if not low:
        quals = [np.maximum(q, Q) for q in quals]
    return reads, quals, rev


def sample(n_short, n_long, seed):
    """lengths and qualities (read orientation) of short reads (150-400 bases) and long ones (3-9 kb) in random order, a few of 0 to 8 bases:
    good bases at 35, about four in a hundred -- a run of them here and there -- at 2..9; every twentieth read good throughout"""
    rng = np.random.default_rng(seed)
    lengths = np.concatenate([rng.integers(150, 401, size=n_short), rng.integers(3000, 9001, size=n_long)])
    rng.shuffle(lengths)
    lengths[3::50] = rng.integers(0, 9, size=len(lengths[3::50]))
    quals = []
    for i, L in enumerate(int(x) for x in lengths):
        q = np.full(L, GOOD, dtype=np.uint8)
        if i % 20 != 7:
            low = rng.random(L) < 0.04
            q[low] = rng.integers(2, Q, size=int(low.sum()))
            if i % 9 == 0 and L > 40:
                at = int(rng.integers(0, L - 12))
                q[at:at + 12] = rng.integers(2, Q, size=12)
        quals.append(q)
    return [int(x) for x in lengths], quals


def small_sample():
    """under 750 000 bases: the ingest hands such a file over as one block"""
    return sample(350, 80, seed=61)


def big_sample():
    """well over 750 000 bases: several blocks"""
    return sample(1000, 250, seed=62)
