"""The decoy screen (include/drprg_hip.h "decoy screen") in plain Python: the set, V, H and the verdict per read.  Nothing here knows the
library; the tests hold the library against it."""
import gzip

import numpy as np

DEFAULT_K, DEFAULT_F, DEFAULT_M = 31, 500, 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(seq):
    return bytes(seq).translate(COMP)[::-1]


def code_of(window):
    """the code of a window (str or bytes) of letters ACGT in either case, first base in the high bits; None when it holds another letter"""
    v = 0
    for ch in (window.decode() if isinstance(window, (bytes, bytearray)) else window).upper():
        if ch not in CODE:
            return None
        v = v << 2 | CODE[ch]
    return v


def revcomp_code(v, k):
    r = 0
    for _ in range(k):
        r = r << 2 | (3 - (v & 3))
        v >>= 2
    return r


def canonical(v, k):
    return min(v, revcomp_code(v, k))


def kmers_plain(seq, k):
    """the canonical k-mer of every start of seq, None where the window holds a letter other than ACGT: the rule, window by window"""
    seq = bytes(seq)
    return [None if (v := code_of(seq[p:p + k])) is None else canonical(v, k) for p in range(len(seq) - k + 1)]


_LETTER = np.full(256, 4, dtype=np.uint64)
for _ch, _v in CODE.items():
    _LETTER[ord(_ch)] = _LETTER[ord(_ch.lower())] = _v


def kmer_arrays(seq, k):
    """the same for every start at once: (canonical codes u64, valid bool), one entry per start (tests/test_decoy_rule.py holds it against
    kmers_plain)"""
    c = _LETTER[np.frombuffer(bytes(seq), dtype=np.uint8)]
    n = c.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    bad = np.concatenate([[0], np.cumsum(c == 4)])
    valid = bad[k:k + n] == bad[:n]
    c = c & np.uint64(3)
    fwd, rev = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        fwd |= c[j:j + n] << np.uint64(2 * (k - 1 - j))
        rev |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    return np.minimum(fwd, rev), valid


def kmers(seq, k):
    codes, valid = kmer_arrays(seq, k)
    return [int(c) if v else None for c, v in zip(codes, valid)]


def records_of(path):
    """the records of a FASTA file, plain or .gz: one sequence (bytes) each"""
    op = gzip.open if str(path).endswith(".gz") else open
    recs, cur = [], None
    with op(path, "rb") as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(b">"):
                cur = []
                recs.append(cur)
            elif cur is not None:
                cur.append(line)
    return [b"".join(r) for r in recs]


def decoy_set(records, k):
    """the canonical k-mers of every window of every record: windows never span two records"""
    return {c for rec in records for c in kmers(rec, k) if c is not None}


def windows_of(records, k):
    return sum(max(0, len(r) - k + 1) for r in records)


def slots_for(windows):
    n = 8
    while n < 2 * windows:
        n *= 2
    return n


def _array(D):
    return D if isinstance(D, np.ndarray) else np.array(sorted(D), dtype=np.uint64)


def counts(read, D, k):
    """(V, H) of one read"""
    codes, valid = kmer_arrays(read, k)
    return int(valid.sum()), int(np.isin(codes[valid], _array(D)).sum())


def drops(V, H, f=DEFAULT_F, M=DEFAULT_M):
    return H >= M and 1000 * H >= f * V


def verdicts(reads, D, k, f=DEFAULT_F, M=DEFAULT_M):
    """per read (V, H, kept)"""
    out, D = [], _array(D)
    for r in reads:
        V, H = counts(r, D, k)
        out.append((V, H, not drops(V, H, f, M)))
    return out


def census(reads, judged, D, k, f=DEFAULT_F, M=DEFAULT_M):
    """what drprg_hip_decoy_info counts since a reset (without the table's two words): judged[i]: the other tests kept read i"""
    c = dict(reads_seen=0, bases_seen=0, reads_dropped=0, bases_dropped=0, valid=0, hits=0)
    keep, D = [], _array(D)
    for r, j in zip(reads, judged):
        if not j:
            keep.append(False)
            continue
        V, H = counts(r, D, k)
        d = drops(V, H, f, M)
        c["reads_seen"] += 1
        c["bases_seen"] += len(r)
        c["valid"] += V
        c["hits"] += H
        c["reads_dropped"] += d
        c["bases_dropped"] += len(r) * d
        keep.append(not d)
    return c, keep


def chimera(decoy_seq, other_seq, k, n_decoy_windows, n_windows):
    """a read of n_windows windows whose first n_decoy_windows are windows of decoy_seq: decoy_seq[:n_decoy_windows + k - 1] followed by
    bases of other_seq (the windows across the join hold both and are in the set only by chance)"""
    head = bytes(decoy_seq[:n_decoy_windows + k - 1])
    return head + bytes(other_seq[:n_windows + k - 1 - len(head)])


def random_dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))
