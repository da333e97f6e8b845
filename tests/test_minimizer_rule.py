"""oracle.sketch against the plain statement of the minimizer rule (tests/minimizer_rule.py): positions, hashes and strands, on examples
worked by hand and on the repeat-rich strings of tests/test_index_oracle.py (REPEAT_PRGS, spelled out allele by allele)."""
import pytest

import minimizer_rule as R
from test_index_oracle import EVEN_WK, REPEAT_PRGS, WK, run_prgs
from util import prg_language


def _oracle_sketch(oracle, seq, w, k):
    h, p, s = oracle.sketch(seq.encode(), w, k)
    return list(zip(p.tolist(), h.tolist(), s.tolist()))


def test_hash64_is_the_oracle_hash(oracle):
    for k in (1, 5, 8, 15, 16, 21, 30, 31):
        mask = (1 << 2 * k) - 1
        for key in (0, 1, mask, mask // 3, 0x123456789ABCDEF & mask, 0xFEDCBA9876543210 & mask):
            assert R.hash64(key, mask) == oracle.lib.orc_hash64(key, mask), (k, key)


def _h(s):
    return R.kmer(s)[0]


def test_examples_worked_by_hand(oracle):
    """k = 3, small enough to follow: the expected positions are written down from the hashes of the 3-mers, not from R.sketch"""
    # a tied pair: the 3-mers of AACGAAC hash to AAC 6, ACG 20, CGA 11, GAA 35, AAC 6 (hash64 on 6 bits; each the smaller of the k-mer's and
    # its reverse complement's, AAC's own being the smaller: strand 1) -- one window of w = 5, its minimum 6 twice: both are reported
    seq, w, k = "AACGAAC", 5, 3
    assert [R.kmer(seq[p:p + 3]) for p in range(5)] == [(6, 1), (20, 0), (11, 1), (35, 1), (6, 1)]
    assert _oracle_sketch(oracle, seq, w, k) == [(0, 6, 1), (4, 6, 1)] == R.sketch(seq, w, k)
    assert R.sketch(seq, w, k, "leftmost") == [(0, 6, 1)] and R.sketch(seq, w, k, "rightmost") == [(4, 6, 1)]
    assert _h("AAC") == _h("GTT")
    # a tied triple: a homopolymer of k + w - 1 bases is one window of w equal hashes, all of them minimizers, each once
    seq, w, k = "AAAAAAA", 5, 3
    sa = R.kmer("AAA")[1]  # (which of AAA and TTT hashes lower is hash64's business; the two strands are opposite)
    assert R.kmer("TTT") == (_h("AAA"), 1 - sa)
    assert _oracle_sketch(oracle, seq, w, k) == [(p, _h("AAA"), sa) for p in range(5)] == R.sketch(seq, w, k)
    assert [p for p, _, _ in R.sketch(seq, w, k, "leftmost")] == [0] and [p for p, _, _ in R.sketch(seq, w, k, "rightmost")] == [4]
    # on the other strand: the other strand flag, the same hash
    assert _oracle_sketch(oracle, "TTTTTTT", w, k) == [(p, _h("AAA"), 1 - sa) for p in range(5)]
    # a tie cut by an N: 4 + 4 k-mers on the two sides of it, no window of 5 on either
    assert _oracle_sketch(oracle, "AAAAAANAAAAAA", 5, 3) == [] == R.sketch("AAAAAANAAAAAA", 5, 3)
    # ... and with one base more to the left there is one window there, its five k-mers tied; lower case reads as upper case
    assert _oracle_sketch(oracle, "aaaaaaAnAAAAAA", 5, 3) == [(p, _h("AAA"), sa) for p in range(5)] == R.sketch("aaaaaaAnAAAAAA", 5, 3)
    # a tie cut by the read end: 4 k-mers, no window; 5 k-mers, one
    assert _oracle_sketch(oracle, "AAAAAA", 5, 3) == [] == R.sketch("AAAAAA", 5, 3)
    # w = 1: every k-mer is its own window, repeats included
    seq = "ACACACAN" + "ACA"
    want = [(0, _h("ACA"), R.kmer("ACA")[1]), (1, _h("CAC"), R.kmer("CAC")[1])] * 2
    want = [(i,) + x[1:] for i, x in enumerate(want)] + [(4, _h("ACA"), R.kmer("ACA")[1]), (8, _h("ACA"), R.kmer("ACA")[1])]
    assert _oracle_sketch(oracle, seq, 1, 3) == want == R.sketch(seq, 1, 3)
    # a k-mer that is its own reverse complement (even k): fwd == rc, strand 1 on both read orientations; the strand mutant says 0
    assert R.kmer("ACGT") == (R.hash64(0b00011011, 255), 1) and R.kmer("ACGT", True)[1] == 0
    for seq in ("ACGT", "ACGTACGT"[2:6]):  # ACGT, GTAC
        assert _oracle_sketch(oracle, seq, 1, 4) == [(0, R.kmer(seq)[0], 1)] == R.sketch(seq, 1, 4)
    # strand = (fwd <= rc): a k-mer and its reverse complement share the hash and have opposite strands, unless they are one k-mer
    assert R.kmer("AAC")[0] == R.kmer("GTT")[0] and R.kmer("AAC")[1] + R.kmer("GTT")[1] == 1


@pytest.mark.parametrize("w,k", WK + EVEN_WK)
def test_oracle_sketch_is_the_plain_rule_on_the_repeat_strings(oracle, w, k):
    prgs = dict(REPEAT_PRGS, **run_prgs(w, k))
    ties = 0
    for name, prg in prgs.items():
        for seq in sorted(prg_language(prg)):
            for s in (seq, seq.lower(), seq[:len(seq) // 2] + "N" + seq[len(seq) // 2 + 1:]):
                got = _oracle_sketch(oracle, s, w, k)
                assert got == R.sketch(s, w, k), (name, w, k, s)
                ties += len(got) - len({h for _, h, _ in got})
    assert ties > 100 or w == 1
