"""What a BAM file means as reads (include/drprg_hip.h "BAM input"), stated in plain Python on the records the test itself wrote: the
expected side of every BAM test.  It never looks at the library under test.

The rule is this build's own (the reference refuses BAM) and restates from memory what `samtools fastq` does by default."""
import numpy as np

CODES = "=ACMGRSVTWYHKDBN"
# complement in code space = the four bits reversed: A(1) <-> T(8), C(2) <-> G(4), M(3) <-> K(12), R(5) <-> Y(10), V(7) <-> B(14),
# H(11) <-> D(13); '=', S(6), W(9), N(15) map to themselves
COMPLEMENT = {CODES[c]: CODES[int(f"{c:04b}"[::-1], 2)] for c in range(16)}
assert COMPLEMENT["A"] == "T" and COMPLEMENT["C"] == "G" and COMPLEMENT["M"] == "K" and COMPLEMENT["R"] == "Y" and COMPLEMENT["N"] == "N"
assert COMPLEMENT["="] == "=" and COMPLEMENT["S"] == "S" and COMPLEMENT["W"] == "W" and COMPLEMENT["V"] == "B" and COMPLEMENT["H"] == "D"


def read_of(rec):
    """the read a kept record stands for, as upper-case text (bytes)"""
    s = rec.seq
    if rec.flag & 0x10:
        s = "".join(COMPLEMENT[ch] for ch in reversed(s))
    return s.encode()


def reads_of(recs):
    """file order; secondary (0x100) and supplementary (0x800) records are skipped, nothing else is"""
    return [read_of(r) for r in recs if not r.flag & 0x900]


def batch_of(reads):
    """(bases u8, offsets u64) of a list of reads"""
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        offs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offs


def fastq_of(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


def digest(reads):
    """drprg_hip_parse_fastx's: the sum of the FNV-1a hashes of the reads"""
    s = 0
    for r in reads:
        h = 1469598103934665603
        for b in r:
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        s = (s + h) & 0xFFFFFFFFFFFFFFFF
    return s


def digest_ordered(reads):
    """drprg_hip_parse_fastx_ordered's: the sum of (index + 1) x FNV-1a of the read"""
    s = 0
    for i, r in enumerate(reads):
        h = 1469598103934665603
        for b in r:
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        s = (s + (i + 1) * h) & 0xFFFFFFFFFFFFFFFF
    return s
