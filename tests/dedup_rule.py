"""The duplicate-read rule of include/drprg_hip.h ("duplicate reads") in plain Python: what the tests of drprg_hip_dedup compare with.
Nothing here is taken from the code under test."""

MASK64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
_LETTER = {ord("A"): 0, ord("a"): 0, ord("C"): 1, ord("c"): 1, ord("T"): 2, ord("t"): 2, ord("G"): 3, ord("g"): 3}


def fin(z):
    """the splitmix64 finaliser"""
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def letters_and_mask(read_bytes):
    """per base: (letter 0..3, masked 0/1); any byte that is not one of ACGTacgt is masked and has letter 0"""
    out = []
    for c in bytes(read_bytes):
        l = _LETTER.get(c)
        out.append((0, 1) if l is None else (l, 0))
    return out


def words(read_bytes):
    """x_0, x_1, ... of the rule"""
    lm = letters_and_mask(read_bytes)
    xs = []
    for j in range(0, len(lm), 16):
        v = m = 0
        for t, (l, k) in enumerate(lm[j:j + 16]):
            v |= l << (2 * t)
            m |= k << t
        xs.append(v | m << 32)
    return xs


def identity(read_bytes):
    """what two identical reads share: (L, (x_0, x_1, ...))"""
    return len(bytes(read_bytes)), tuple(words(read_bytes))


def key(read_bytes):
    """the content key; 0 for a read of no bases (the device entry leaves 0 there)"""
    L = len(bytes(read_bytes))
    if L == 0:
        return 0
    k = fin(G * L)
    for j, x in enumerate(words(read_bytes)):
        k = (k + fin(x + G * (j + 1))) & MASK64
    return k


def keep_flags(reads):
    """1 for every read that no read before it is identical to; a read of no bases is always kept and never makes a duplicate"""
    seen, flags = set(), []
    for r in reads:
        ident = identity(r)
        if ident[0] == 0:
            flags.append(1)
            continue
        flags.append(0 if ident in seen else 1)
        seen.add(ident)
    return flags


_NORMAL = bytes(c if c in b"ACGT" else (c - 32 if c in b"acgt" else ord("N")) for c in range(256))


def keep_flags_fast(reads):
    """keep_flags for large fixtures: a read's bytes with ACGT upper-cased and every other byte turned into N say exactly what (L, x) says
    (tests/test_dedup_rule.py holds the two against each other)"""
    seen, flags = set(), []
    for r in reads:
        t = bytes(r).translate(_NORMAL)
        flags.append(1 if not t or t not in seen else 0)
        seen.add(t)
    return flags
