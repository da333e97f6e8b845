"""The plain-Python statement of the duplicate-read rule (tests/dedup_rule.py) against a naive all-pairs comparison, and the identities
the rule promises.  No GPU."""
import numpy as np

from dedup_rule import G, MASK64, fin, keep_flags, keep_flags_fast, key, letters_and_mask, words


def _naive_identical(a, b):
    """straight from the rule's words: same length, masked bases at the same places, same letters elsewhere"""
    if len(a) != len(b):
        return False
    for x, y in zip(letters_and_mask(a), letters_and_mask(b)):
        if x != y:
            return False
    return True


def _random_reads(seed, n):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTacgtNRn", np.uint8)
    pool = []
    for _ in range(n // 3):
        L = int(rng.choice([0, 1, 2, 15, 16, 17, 31, 32, 33, 40]))
        # a small alphabet of short reads: plenty of chance duplicates; the long ones repeat by copying
        pool.append(bytes(rng.choice(alphabet[:4] if rng.random() < 0.7 else alphabet, size=L)) if L > 2 else bytes(rng.choice(alphabet, size=L)))
    reads = []
    for _ in range(n):
        r = pool[int(rng.integers(0, len(pool)))]
        what = rng.random()
        if what < 0.15 and r:
            r = r.swapcase()
        elif what < 0.25 and r:
            r = r[:-1]
        elif what < 0.35:
            r = r + b"A"
        reads.append(r)
    return reads


def test_keep_flags_equal_an_all_pairs_comparison():
    reads = _random_reads(3, 400)
    want = []
    for i, r in enumerate(reads):
        want.append(0 if len(r) and any(_naive_identical(reads[h], r) for h in range(i)) else 1)
    got = keep_flags(reads)
    assert got == want
    assert keep_flags_fast(reads) == want
    assert 0.2 < 1 - sum(got) / len(got) < 0.9  # (the fixture holds duplicates, and reads that are none)


def test_the_identities_the_rule_promises():
    assert keep_flags([b"ACGTACGTACGTACGTAC", b"acgtacgtACGTACGTac"]) == [1, 0]  # case
    assert keep_flags([b"ACGNACGT", b"ACGRACGT", b"ACGnACGT"]) == [1, 0, 0]  # any byte that is not ACGT is the same masked base
    assert keep_flags([b"ACGNACGT", b"ACGAACGT"]) == [1, 1] and keep_flags([b"ACGAACGT", b"ACGNACGT"]) == [1, 1]  # N is not A
    assert keep_flags([b"ACGTACGTACGTACGTACGT", b"ACGTACGTACGTACGT", b"ACGTACGTACGTACGTACGTA"]) == [1, 1, 1]  # a prefix is not a duplicate
    assert keep_flags([b"ACGTAAAA", b"ACGT", b"ACGTA"]) == [1, 1, 1]  # ... not even when what is missing is letter 0
    assert keep_flags([b"", b"", b"ACGT", b"", b"ACGT"]) == [1, 1, 1, 1, 0]  # empty reads are kept
    assert keep_flags([b"AACC", b"GGTT"]) == [1, 1]  # forward strand only: the reverse complement is another read
    assert keep_flags([b"ACGT", b"TTTT", b"ACGT", b"acgt"]) == [1, 1, 0, 0]  # the first copy stays, every later one goes


def test_letters_words_and_key():
    assert letters_and_mask(b"AaCcTtGgN.") == [(0, 0), (0, 0), (1, 0), (1, 0), (2, 0), (2, 0), (3, 0), (3, 0), (0, 1), (0, 1)]
    assert words(b"C" * 16 + b"GN") == [0x55555555, 3 | (2 << 32)]
    assert words(b"") == [] and key(b"") == 0
    r = b"ACGTTGCAN"
    x = (0 | 1 << 2 | 3 << 4 | 2 << 6 | 2 << 8 | 3 << 10 | 1 << 12 | 0 << 14) | (1 << 8) << 32
    assert words(r) == [x]
    assert key(r) == (fin(G * 9) + fin(x + G)) & MASK64
    # L is in the key: a poly-A tail changes it although it adds only zero letters
    assert key(b"ACGT") != key(b"ACGTA") != key(b"ACGTAA")
    assert key(b"ACGNACGT") == key(b"ACGRACGT") != key(b"ACGAACGT")


def _pack_batch(batch):
    """a batch as the device holds it: 16 bases per 32-bit word (letter = bits 2:1 of the byte), one 16-bit row of mask bits per word"""
    ws, ms = [], []
    for j in range(0, len(batch), 16):
        w = m = 0
        for t, c in enumerate(batch[j:j + 16]):
            w |= ((c >> 1) & 3) << (2 * t)
            m |= (0 if c in b"ACGTacgt" else 1) << t
        ws.append(w)
        ms.append(m)
    return ws + [0], ms + [0]


def _words_from_batch(ws, ms, start, L):
    """x_j of the read at bases [start, start + L) of a packed batch: a funnel shift of two adjacent batch words at the read's phase, bases
    behind the read's end cleared, letters under mask bits forced to 0"""
    xs = []
    for j in range(0, L, 16):
        at, n = start + j, min(16, L - j)
        w, phase = at // 16, at % 16
        v = ((ws[w + 1] << 32 | ws[w]) >> (2 * phase)) & ((1 << (2 * n)) - 1)
        m = ((ms[w + 1] << 16 | ms[w]) >> phase) & ((1 << n) - 1)
        for t in range(n):
            if m >> t & 1:
                v &= ~(3 << (2 * t))
        xs.append(v | m << 32)
    return xs


def test_key_does_not_depend_on_where_the_read_sits_in_a_batch():
    """the same read behind prefixes of 0 .. 33 bases of a packed batch: its words, taken out of the batch's words by a funnel shift at
    every phase, are the rule's words of the read alone -- so is the key, and a sum of its terms in any order is the same bits"""
    rng = np.random.default_rng(9)
    for L in (1, 15, 16, 17, 33, 70):
        read = bytes(rng.choice(np.frombuffer(b"ACGTNacgtR", np.uint8), size=L))
        for shift in range(34):
            batch = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=shift)) + read + b"TGN" * 3
            ws, ms = _pack_batch(batch)
            xs = _words_from_batch(ws, ms, shift, L)
            assert xs == words(read), (L, shift)
            terms = [fin(G * L)] + [fin(x + G * (j + 1)) for j, x in enumerate(xs)]
            rng.shuffle(terms)
            assert sum(terms) & MASK64 == key(read)
