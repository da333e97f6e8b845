"""Poly-tail trimming's and the low-complexity filter's rules (include/drprg_hip.h "poly tails" and "read complexity":
drprg_hip_set_poly_trim, drprg_hip_set_min_complexity), stated in plain Python and independently of the product: what the tests of either
expect comes from here and from the oracle on the reads these rules leave, never from the code under test.  Also the fixtures the GPU tests
cut and judge.

Both rules are this build's own, after fastp.  One comparison serves both: case-insensitive; every byte that is not one of ACGTacgt is the
one unknown base U, which equals U and differs from every letter."""
import numpy as np

MAX_MISS = 5
M = 10     # the tails' shortest length in the samples
P = 30     # the complexity threshold of the samples
TILE, LANE, WORD = 16384, 64, 16  # bases per workgroup and per lane of read_diff_kernel, and per packed word


def symbols(read):
    """the read as the comparison sees it: one of A, C, G, T, U per base"""
    return "".join(chr(b).upper() if chr(b).upper() in "ACGT" else "U" for b in bytes(read))


def allowance(n):
    return min(n // 8, MAX_MISS)


def qualifies(sym, n, X):
    """the suffix of n >= 1 bases of `sym` (symbols) qualifies for the letter X (no word about M here)"""
    suffix = sym[len(sym) - n:]
    return suffix[0] == X and sum(c != X for c in suffix) <= allowance(n)


def tail_cut(read, letters, M=M):
    """how many bases the read loses: its longest qualifying suffix of at least M bases over the letters -- the obvious quadratic form"""
    sym = symbols(read)
    assert letters and set(letters.upper()) <= set("ACGT") and len(set(letters.upper())) == len(letters) and 2 <= M <= 255
    return max([n for X in letters.upper() for n in range(M, len(sym) + 1) if qualifies(sym, n, X)], default=0)


def tail_cut_fast(read, letters, M=M):
    """tail_cut in one pass per letter, for the fixtures' long reads: the bases that are not X only grow in number with n, so no suffix
    qualifies behind the sixth of them.  tests/test_polyx_rule.py holds it against tail_cut."""
    sym = symbols(read)
    L, best = len(sym), 0
    for X in letters.upper():
        mm = 0
        for n in range(1, L + 1):
            mm += sym[L - n] != X
            if mm > MAX_MISS:
                break
            if sym[L - n] == X and n >= M and mm <= allowance(n):
                best = max(best, n)
    return best


def cut_ranges(reads, ranges, letters, M=M):
    """[(begin, end)] behind the tail cut of every read's range, and the five counts of drprg_hip_poly_trim_info"""
    out = []
    info = dict(reads_seen=len(reads), bases_seen=0, reads_cut=0, bases_cut=0, reads_emptied=0)
    for r, (x, y) in zip(reads, ranges):
        c = tail_cut_fast(r[x:y], letters, M)
        info["bases_seen"] += y - x
        info["reads_cut"] += c > 0
        info["bases_cut"] += c
        info["reads_emptied"] += c > 0 and c == y - x
        out.append((x, y - c))
    return out, info


def cut(reads, letters, M=M):
    """the reads behind the tail cut, and the five counts"""
    ranges, info = cut_ranges(reads, [(0, len(r)) for r in reads], letters, M)
    return [r[x:y] for r, (x, y) in zip(reads, ranges)], info


def differing_pairs(read):
    """D: the neighbouring pairs of the read that differ"""
    sym = symbols(read)
    return sum(sym[i] != sym[i + 1] for i in range(len(sym) - 1))


def differing_pairs_fast(read):
    b = np.frombuffer(bytes(read), dtype=np.uint8)
    u = b & 0xDF
    s = np.where(np.isin(u, np.frombuffer(b"ACGT", np.uint8)), u, ord("U"))
    return int((s[1:] != s[:-1]).sum())


def dropped(read, P=P, D=None):
    """the read is dropped as low complexity"""
    assert 1 <= P <= 100
    L = len(read)
    D = differing_pairs_fast(read) if D is None else D
    return L >= 2 and 100 * D < P * (L - 1)


def census(reads, judged, P=P):
    """the four counts of drprg_hip_complexity_info over the reads the other tests kept (judged: one flag per read), and the keep flags"""
    info = dict(reads_seen=0, bases_seen=0, reads_dropped=0, bases_dropped=0)
    keep = []
    for r, j in zip(reads, judged):
        d = bool(j) and dropped(r, P)
        info["reads_seen"] += bool(j)
        info["bases_seen"] += len(r) if j else 0
        info["reads_dropped"] += d
        info["bases_dropped"] += len(r) if d else 0
        keep.append(bool(j) and not d)
    return info, keep


# ---- the fixtures of tests/test_gpu_polyx.py ----------------------------------------------------------------------------------------------
def _dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(letters, np.uint8), size=n)) if n else b""


def kernel_batch(listed=True, long_reads=True):
    """the ragged batch of the kernel tests: (reads, ranges).  Tails are runs of G (S = {G} and S = {A, C, G, T} are both asked of it).
    listed: some bases are not ACGT; long_reads: the tails of 5 000 and of 70 000 bases, longer than any tile, and a 70 000-base read of
    random bases.  See the comments for what each read is there for."""
    rng = np.random.default_rng(97)
    reads, ranges = [], []

    def pos():
        return sum(len(r) for r in reads)

    def add(r, x=0, y=None):
        reads.append(bytes(r))
        ranges.append((x, len(r) if y is None else y))

    def body(n):  # (no G: what a tail stands behind is never part of it by chance)
        return _dna(rng, n, b"ACT")

    for n in (0, 1, M - 1, M, 0):                     # reads of 0, 1, M - 1 and M bases: all G, and random
        add(b"G" * n)
        add(_dna(rng, n))
    for n in (15, 16, 17, 63, 64, 65, 127, 128, 129): # all-X reads across the word and the lane's solo limit
        add(b"G" * n)
        add(b"c" * n)
    add(body(40) + b"G" * (M - 1))                   # one base short
    add(body(40) + b"G" * M)
    add(body(40) + b"GGGGAGGGGG")                    # one other base in ten: floor(10 / 8) = 1
    add(body(40) + b"GGGAGGGGGGGGGGGTGGGGGG")        # two in 22
    add(b"TTTT" + b"GACGT" + b"G" * 40)              # takes four other bases along
    add(b"C" * 30 + b"G" * 100 + b"AAAAA")           # five at the very end
    add(b"C" * 30 + b"G" * 100 + b"AAAAAA")          # six: nothing
    add(body(30) + b"gggggNGGGGGG")                  # U and lower case inside a tail
    add(body(30) + b"G" * 30 + b"NN" + b"G" * 30)
    for mod in (WORD, LANE):                         # a tail whose first base lies exactly on, one before and one past a word and a lane edge
        for at in (mod - 1, 0, 1):
            for t in (12, 40, 100):
                pad = (at - pos() - 30) % mod
                add(body(30 + pad) + b"G" * t)
                assert (pos() - t) % mod == at
    # ranges already narrowed: the tail ends where the range ends, junk behind it; and a range that holds less than the tail
    add(body(50) + b"G" * 30 + body(20), 5, 80)
    add(body(50) + b"G" * 30 + body(20), 5, 100)
    add(body(20) + b"G" * 60, 50, 80)
    add(b"G" * 60, 60, 60)
    add(b"G" * 60, 0, M - 1)
    if long_reads:
        add(body(100) + b"G" * 5000)
        add(body(3000) + b"G" * 2000 + b"T" + b"G" * 3000 + b"AC" + b"G" * 1000)
        add(body(77) + b"G" * 70_000)
        add(_dna(rng, 70_000))
        add(b"A" * 35_000 + b"N" * 10 + b"a" * 35_000)
    while pos() % TILE < 300 or len(reads) < 400:    # short reads, a third of them with a tail, some with other bases in it
        n = int(rng.integers(1, 300))
        t = int(rng.integers(0, n + 1)) if len(reads) % 3 == 0 else 0
        r = bytearray(_dna(rng, n - t) + b"G" * t)
        for _ in range(int(rng.integers(0, 3))):
            if n:
                r[int(rng.integers(0, n))] = rng.choice(list(b"ACGT"))
        add(r)
    add(body(33) + b"G" * 77)                        # the last read ends at the block's last byte, and is cut
    if listed:
        for i in range(60, len(reads), 5):
            if len(reads[i]) > 3:
                r = bytearray(reads[i])
                at = len(r) - 1 - (i % 13) if len(r) > 13 else len(r) // 2
                r[at:at + 1] = b"NRnYKM"[i % 6:i % 6 + 1]
                reads[i] = bytes(r)
    else:
        reads = [r.translate(bytes.maketrans(b"NRYKMnry", b"GGGGGGGG")) for r in reads]
    return reads, ranges


def complexity_batch(listed=True):
    """the reads of the D kernel's test: kernel_batch's, and in front of them what decides its two sites -- the pair of two reads' last and
    first bases never counts, the pair across a word, a lane and a tile edge inside a read always does -- and thresholds met exactly"""
    rng = np.random.default_rng(98)
    reads = []
    for a, b in ((b"AAAA", b"CCCC"), (b"AAAA", b"AAAA"), (b"AC", b"CA"), (b"AA", b"AA"), (b"A", b"C"), (b"", b"G"), (b"GT", b"")):
        reads += [a, b]                              # neighbouring reads whose last and first bases differ and are equal; reads of 2, 1, 0 bases
    reads += [b"NNNN", b"ANNA", b"A" * 10 + b"C" * 10, b"AnNRc", b"NNNNNNNNNNNNNNNNNNNNNNNNA"]  # runs of U
    reads += [b"A" * 8 + b"CAC", b"A" * 9 + b"CA"]   # L - 1 = 10 pairs: D = 3 meets P = 30 exactly (kept), D = 2 is one below (dropped)
    reads += [b"ACGT" * 25 + b"A", b"AC" * 15 + b"C" * 71]  # 100 pairs: D = 100; D = 30 exactly
    for n in (15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129):  # alternating and constant reads across the word and lane edges
        reads += [(b"AC" * n)[:n], b"T" * n]
    reads += [_dna(rng, int(n)) for n in rng.integers(0, 200, size=150)]
    more, _ = kernel_batch(listed=listed)
    reads += more
    if not listed:
        reads = [r.translate(bytes.maketrans(b"NRYKMnry", b"GGGGGGGG")) for r in reads]
    assert sum(len(r) for r in reads) > 9 * TILE
    return reads


def tailed_sample(reads, seed):
    """reads of a sample with the artefacts the two rules are for, by turns: a G tail of 20 to 100 bases in place of the read's end (one
    other base in some), a read that is all G, a poly-A tail, a dinucleotide repeat, and nothing.  Returns (reads as bytes, kinds)."""
    rng = np.random.default_rng(seed)
    out, kinds = [], []
    for i, r in enumerate(reads):
        kind = ("g tail", "plain", "plain", "all g", "plain", "a tail", "plain", "plain", "repeat", "plain", "plain")[i % 11] if len(r) >= 120 else "plain"
        if kind in ("g tail", "a tail"):
            t = int(rng.integers(20, 101))
            tail = bytearray((b"G" if kind == "g tail" else b"A") * t)
            if i % 4 == 0:
                tail[int(rng.integers(1, t))] = ord("C")
            r = r[:len(r) - t] + bytes(tail)
        elif kind == "all g":
            r = b"G" * len(r)
        elif kind == "repeat":
            r = (b"AAAAAAAAAT" * len(r))[:len(r)]
        out.append(bytes(r))
        kinds.append(kind)
    return out, kinds
