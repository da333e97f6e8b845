"""DESIGN section 4's minimizer rule in plain Python, by brute force: the statement every sketch (the oracle's, the index builder's, the four
device forms) is held against where hashes tie.

hash64 is oracle/oracle.c's invertible mix on 2k bits, restated on Python integers.  The canonical hash of a k-mer is min(fwd, rc), its
strand is fwd <= rc (1 = the forward k-mer is the canonical one; a k-mer that is its own reverse complement has fwd == rc and strand 1).
Within one maximal ACGT run (either letter case), every window of w consecutive k-mers makes every k-mer whose canonical hash equals the
window's minimum a minimizer: ties kept, each k-mer reported once.

rule="leftmost" / "rightmost" (one tied k-mer per window only) and strict_strand=True (strand = fwd < rc) are MUTANTS: wrong on purpose,
used only by the census of tests/low_complexity.py to show that a class of reads would tell them from the rule."""
import functools

_CODE = {c: i for i, c in enumerate("ACGT")}


def hash64(key, mask):
    key = (~key + (key << 21)) & mask
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & mask
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & mask
    key = key ^ key >> 28
    return (key + (key << 31)) & mask


@functools.lru_cache(maxsize=1 << 18)
def kmer(s, strict_strand=False):
    """(canonical hash, strand) of the k-mer s (upper case); None if it holds a letter that is not ACGT"""
    if any(c not in _CODE for c in s):
        return None
    mask = (1 << 2 * len(s)) - 1
    f = r = 0
    for i, c in enumerate(s):
        f = f << 2 | _CODE[c]
        r |= (3 - _CODE[c]) << 2 * i
    hf, hr = hash64(f, mask), hash64(r, mask)
    return min(hf, hr), int(hf < hr if strict_strand else hf <= hr)


def kmers(seq, k, strict_strand=False):
    """kmer() of every position of seq (str or bytes, either letter case)"""
    seq = (seq.decode() if isinstance(seq, (bytes, bytearray)) else seq).upper()
    return [kmer(seq[p:p + k], strict_strand) for p in range(len(seq) - k + 1)]


def pick(km, w, rule="all"):
    """positions of the minimizers among kmers()' list: every window of w k-mers without a None, window by window"""
    hs = [x and x[0] for x in km]
    marked = set()
    for s in range(len(hs) - w + 1):
        win = hs[s:s + w]
        if None in win:
            continue
        m = min(win)
        tied = [s + j for j in range(w) if win[j] == m]
        marked.update(tied if rule == "all" else tied[:1] if rule == "leftmost" else tied[-1:])
    return sorted(marked)


def sketch(seq, w, k, rule="all", strict_strand=False):
    """[(position, canonical hash, strand)] of seq's minimizers, by position"""
    km = kmers(seq, k, strict_strand)
    return [(p,) + km[p] for p in pick(km, w, rule)]
