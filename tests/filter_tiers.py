"""The filter tiers of the filtered sequence at every step of their sizes: a plain restatement of the arrays, panels and read batches.

sketch_filter_kernel may only skip a k-mer that its filter arrays reject, so the whole sequence rests on one claim: no array rejects an index
k-mer.  PrgIndex::flatten (csrc/index.cpp) changes the arrays' shape with the number R of index records (E = 2 R entries: both orientations):

  step                                                          rule in index.cpp                            edge (R)
  levels 1+2 words (k < 15)                                     wbits from 8 while 2^wbits 5 < 4 E, cap 14   160 2^j | + 1, j = 0 .. 5
  filtered -> none, k < 15                                      E <= 3 2^14                                  24 576 | 24 577
  small tier's block filter blkc                                cw from 10 while 4 << cw < 4 E               2^(cw - 1) | + 1, cw = 10 .. 15
  level 0 (all-LDS) -> middle tier, k = 15                      12 E <= 2^19                                 21 845 | 21 846
  middle tier's blocks midc                                     cw from 10 while 8 << cw < 4 E, cap 17       32 768 | + 1, 65 536 | + 1, 131 072 | + 1
  middle tier's level 0, three bits -> one                      distinct canonical 12-mers 5 <= 2^21         419 430 | 419 431 distinct
  middle tier -> direct sequence                                mid_max_records                              180 000 | 180 001

The restatement below is written from csrc/index.cpp (the arrays), csrc/common.h (multipliers, canonical 12-mers), csrc/index.h and
csrc/sketch_filter.hip (the kernel's side: which 12-mer a position's group is keyed on, the word and block taken by shift, the bit tests) in
plain numpy; it never calls the product.  tests/test_filter_tiers.py holds the census on the CPU, tests/test_gpu_filter_tiers.py maps the
batches on the device.

  alphabet   letter = bits 2:1 of the ASCII byte (A 0, C 1, T 2, G 3), complement = letter ^ 2, first base in the lowest bits
  THRESHOLD  w = 1 (every k-mer is a minimizer: R = the sum of length - k + 1 over the loci), random site-free loci of 3 000 bases from one pool
             and a last locus whose length sets R; the two panels of a pair differ by that locus's last base.  MID0 extends the last locus
             base by base until the canonical 12-mers are 419 430 | 419 431 (one more base brings one more 12-mer).
  SITES      synth.small_panel(site_every=400) at (11, 15) and (14, 13) plus a last site-free locus, searched so that R lies within 1 % of
             an edge: the widest arrays with variant paths and a realistic w.
  batches    every locus (SITES: two haplotypes of it) as reads of at most 4 000 bases, forward and reverse complement, four times: behind 0,
             1, 2 and 3 more bases from the start of the batch, so that every index k-mer meets every alignment of the kernel's groups of
             four positions in both orientations (the kernel tiles batch positions, not reads); then 2 000 reads of 150 bases with 1 %
             errors from two haplotype genomes twice the panel's size, a non-ACGT byte in every tenth of them, three empty reads and three
             shorter than k."""
import numpy as np

# ---- constants (tests/test_filter_tiers.py reads them out of the sources) -----------------------------------------------------------------
BLOOM_C0, BLOOM_C1, BLOOM_C2, BLOOM_CR = 0xC2B2AF, 0x9E3779, 0x85EBCA6B, 0xC2B2AE35
MAX_WBITS, L0_WBITS, BLOOMR_WBITS = 14, 15, 14
MID_C_MAX_WBITS, MID_BITMAP_WORDS, MID_MAX_RECORDS = 17, 1 << 19, 180_000
M32 = np.uint64(0xFFFFFFFF)
M24 = np.uint64(0xFFFFFF)
_U = np.uint64


# ---- the size rules -----------------------------------------------------------------------------------------------------------------------
def tier_of(n_records, k, mid_max_records=MID_MAX_RECORDS):
    """'level0' | 'levels12' | 'middle' | None (no filter tier: a direct sequence serves the index)"""
    e = 2 * n_records
    small = k <= 15 and 0 < e <= 3 * (1 << MAX_WBITS)
    level0 = small and k == 15 and 4 * e * 3 <= (32 << L0_WBITS) // 2
    if small and (level0 or k < 15):
        return "level0" if level0 else "levels12"
    if k == 15 and e > 0 and n_records <= mid_max_records:
        return "middle"
    return None


def bloom_wbits(n_records, level0):
    wbits, cap = 8, MAX_WBITS - 1 if level0 else MAX_WBITS
    while wbits < cap and (1 << wbits) * 5 < 2 * n_records * 4:
        wbits += 1
    return wbits


def blkc_wbits(n_records):
    cw = 10
    while cw < MID_C_MAX_WBITS and (4 << cw) < 4 * 2 * n_records:
        cw += 1
    return cw


def midc_wbits(n_records):
    cw = 10
    while cw < MID_C_MAX_WBITS and (8 << cw) < 4 * 2 * n_records:
        cw += 1
    return cw


def mid0_bits(distinct_12mers):
    return 3 if distinct_12mers * 5 <= (32 << L0_WBITS) * 2 else 1


FILTER_FORMS = {"level0": 10, "levels12": 11, "middle": 12}   # Context.table_tier()["sketch_form"]


def tier_sizes(n_records, k, mid_max_records=MID_MAX_RECORDS):
    """(tier, lds_filter_bytes, l2_filter_bytes) as Context.table_tier() reports them (mapper.cpp device_tables): level 0 + levels 1+2 + the
    retired second-stage array | levels 1+2 | the middle tier's level 0; the block filter | nothing | the 12-mer bitmap + the blocks"""
    tier = tier_of(n_records, k, mid_max_records)
    if tier == "level0":
        return tier, (4 << bloom_wbits(n_records, True)) + (4 << L0_WBITS) + (4 << BLOOMR_WBITS), 16 << blkc_wbits(n_records)
    if tier == "levels12":
        return tier, 4 << bloom_wbits(n_records, False), 0
    if tier == "middle":
        return tier, 4 << L0_WBITS, MID_BITMAP_WORDS * 4 + (16 << midc_wbits(n_records))
    return None, 0, 0


# ---- codes --------------------------------------------------------------------------------------------------------------------------------
def letters_of(seq):
    s = seq if isinstance(seq, np.ndarray) else np.frombuffer(seq.encode() if isinstance(seq, str) else seq, np.uint8)
    return ((s >> 1) & 3).astype(np.uint64)


def codes_at(letters, pos, k):
    """the code of the k-mer that starts at each position of pos"""
    pos = np.asarray(pos, np.int64)
    code = np.zeros(len(pos), np.uint64)
    for j in range(k):
        code |= letters[pos + j] << _U(2 * j)
    return code


def rc_codes(codes, k):
    out = np.zeros(len(codes), np.uint64)
    for j in range(k):
        out |= (((codes >> _U(2 * j)) & _U(3)) ^ _U(2)) << _U(2 * (k - 1 - j))
    return out


def canon12(x):
    x = x & M24
    r = rc_codes(x, 12)
    return np.minimum(x, r)


def sequence_codes(seq, k):
    """the codes of every k-mer of a sequence, in both orientations: what a site-free locus brings into the index at w = 1"""
    le = letters_of(seq)
    fw = codes_at(le, np.arange(len(le) - k + 1), k)
    return np.concatenate([fw, rc_codes(fw, k)])


def oracle_codes(oracle, prg, w, k):
    """the codes of the index k-mers of one PRG string, both orientations, from the oracle's k-mer paths (intervals of the PRG string)"""
    g = oracle.sketch_prg(prg, w, k, paths=True)
    text = np.frombuffer(prg.encode(), np.uint8)
    n = len(g["paths"])
    flat = np.zeros((n, k), np.int64)
    for i, path in enumerate(g["paths"]):
        at = 0
        for a, b in path:
            flat[i, at:at + b - a] = np.arange(a, b)
            at += b - a
        assert at == k, (i, path)
    seqs = text[flat]
    assert np.isin(seqs, np.frombuffer(b"ACGT", np.uint8)).all()
    le = ((seqs >> 1) & 3).astype(np.uint64)
    fw = np.zeros(n, np.uint64)
    for j in range(k):
        fw |= le[:, j] << _U(2 * j)
    return np.concatenate([fw, rc_codes(fw, k)]), g


# ---- the arrays (index.cpp) and the kernel's tests (sketch_filter.hip) ----------------------------------------------------------------------
def _mul(a, c):
    return (a * _U(c)) & M32


def _or_at(arr, at, bits):
    np.bitwise_or.at(arr, at.astype(np.int64), bits)


def _bit(n):
    return _U(1) << n


def _b31(n):
    """the bit that bloom_test reaches by shifting the word LEFT by n"""
    return _U(1) << (_U(31) - (n & _U(31)))


def _three(key, mult):
    """(word selector before masking, the three bits) of level 0 | level 1 for a 24-bit key"""
    g = _mul(key, mult)
    return g, _b31(g) | _b31(g >> _U(8)) | _b31(key >> _U(16))


def _block_bits(codes):
    h = _mul(codes, BLOOM_CR)
    return [_bit(h >> _U(27)), _bit((h >> _U(22)) & _U(31)), _bit((h >> _U(17)) & _U(31)), _bit((h >> _U(12)) & _U(31))]


def _stage_bits(codes):
    """(word of the shared level-0 array, six bits) of the all-LDS second stage"""
    hr, hs = _mul(codes, BLOOM_CR), _mul(codes, BLOOM_C2)
    bits = _bit(hr & _U(31)) | _bit((hr >> _U(5)) & _U(31)) | _bit((hr >> _U(10)) & _U(31)) | _bit(hs >> _U(27)) | _bit((hs >> _U(22)) & _U(31)) \
        | _bit((hs >> _U(17)) & _U(31))
    return hr >> _U(32 - L0_WBITS), bits


def _block_array(keys_per_offset, codes, cw):
    arr = np.zeros((1 << cw, 4), np.uint64)
    bits = _block_bits(codes)
    for key in keys_per_offset:
        blk = (_mul(key, BLOOM_C0) >> _U(32 - cw)).astype(np.int64)
        for i in range(4):
            np.bitwise_or.at(arr[:, i], blk, bits[i])
    return arr


def fill_permille(arr):
    a = np.ascontiguousarray(arr, np.uint64).reshape(-1)
    bits = int(np.unpackbits(a.view(np.uint8)).sum())
    return bits * 1000 // (32 * a.size)


class Tables:
    """every array flatten builds for an index of these codes (both orientations of every record's k-mer), and the kernel's tests on them"""

    def __init__(self, codes, k, mid_max_records=MID_MAX_RECORDS, l0_offsets=(0, 1, 2, 3)):
        codes = np.asarray(codes, np.uint64)
        assert len(codes) % 2 == 0
        self.codes, self.k, self.n_records = codes, k, len(codes) // 2
        self.tier = tier_of(self.n_records, k, mid_max_records)
        r = self.n_records
        wmask0 = _U((1 << L0_WBITS) - 1)
        if self.tier in ("level0", "levels12"):
            self.wbits = bloom_wbits(r, self.tier == "level0")
            self.bloom = np.zeros(1 << self.wbits, np.uint64)
            h, bits = _three(codes & M24, BLOOM_C1)
            _or_at(self.bloom, (h >> _U(18)) & _U((1 << self.wbits) - 1), bits)
            h2 = _mul(codes, BLOOM_C2)
            _or_at(self.bloom, h2 >> _U(32 - self.wbits), _bit(h2 & _U(31)) | _bit((h2 >> _U(5)) & _U(31)) | _bit((h2 >> _U(10)) & _U(31)))
        if self.tier == "level0":
            self.bloom0 = np.zeros(1 << L0_WBITS, np.uint64)
            for o in l0_offsets:  # (every offset: index.cpp; fewer: what the census measures an array without one of them by)
                g, bits = _three((codes >> _U(2 * o)) & M24, BLOOM_C0)
                _or_at(self.bloom0, (g >> _U(17)) & wmask0, bits)
            self.bloom0f = self.bloom0.copy()
            word, bits = _stage_bits(codes)
            _or_at(self.bloom0f, word, bits)
            self.bloomr = np.zeros(1 << BLOOMR_WBITS, np.uint64)
            hr = _mul(codes, BLOOM_CR)
            _or_at(self.bloomr, hr >> _U(32 - BLOOMR_WBITS),
                   _bit(hr & _U(31)) | _bit((hr >> _U(5)) & _U(31)) | _bit((hr >> _U(10)) & _U(31)) | _bit((hr >> _U(15)) & _U(31)))
            self.blkc_wbits = blkc_wbits(r)
            self.blkc = _block_array([(codes >> _U(2 * o)) & M24 for o in range(4)], codes, self.blkc_wbits)
        if self.tier == "middle":
            keys = [canon12(codes >> _U(2 * o)) for o in range(4)]
            distinct = np.unique(np.concatenate(keys))
            self.distinct_12mers = len(distinct)
            self.mid_bitmap = np.zeros(MID_BITMAP_WORDS, np.uint64)
            _or_at(self.mid_bitmap, distinct >> _U(5), _bit(distinct & _U(31)))
            self.mid0_bits = mid0_bits(self.distinct_12mers)
            self.mid0 = {}
            for nbits in (1, 3):  # (both bit counts are restated; mid0_bits says which one flatten keeps)
                g, bits = _three(distinct, BLOOM_C0)
                arr = np.zeros(1 << L0_WBITS, np.uint64)
                _or_at(arr, (g >> _U(17)) & wmask0, bits if nbits == 3 else _b31(g))
                self.mid0[nbits] = arr
            self.midc_wbits = midc_wbits(r)
            self.midc = _block_array(keys, codes, self.midc_wbits)

    def array_bytes(self):
        """(bytes of the arrays held in LDS, bytes of those held in the L2), counted on the arrays themselves (tier_sizes: by the rules)"""
        if self.tier == "middle":
            return 4 * len(self.mid0[self.mid0_bits]), 4 * len(self.mid_bitmap) + 4 * self.midc.size
        if self.tier == "level0":
            return 4 * (len(self.bloom) + len(self.bloom0) + len(self.bloomr)), 4 * self.blkc.size
        return (4 * len(self.bloom), 0) if self.tier == "levels12" else (0, 0)

    # ---- the kernel's side: the k-mer with this code stands at a batch position p with p % 4 == align ------------------------------------
    def _block_passes(self, arr, cw, key, codes, less=0):
        blk = (_mul(key, BLOOM_C0) >> _U(32 - cw + less)).astype(np.int64)
        bits = _block_bits(codes)
        ok = np.ones(len(codes), bool)
        for i in range(4):
            ok &= (arr[blk, i] & bits[i]) != 0
        return ok

    def passes(self, codes, align, stage2="lds", mutation=None):
        """which of these k-mers the kernel keeps.  stage2: 'lds' | 'l2' (the small tier's two second stages).  mutation: None, 'block' (the
        block taken with one bit less), 'word' (the level-2 word taken with one bit less), 'mid0' (the three-bit test on the array that
        flatten keeps): each keeps every index in range"""
        codes, align = np.asarray(codes, np.uint64), np.asarray(align, np.uint64)
        wmask0 = _U((1 << L0_WBITS) - 1)
        if self.tier == "levels12":
            h, bits = _three(codes & M24, BLOOM_C1)
            ok = (self.bloom[((h >> _U(18)) & _U((1 << self.wbits) - 1)).astype(np.int64)] & bits) == bits
            h2 = _mul(codes, BLOOM_C2)
            bits2 = _bit(h2 & _U(31)) | _bit((h2 >> _U(5)) & _U(31)) | _bit((h2 >> _U(10)) & _U(31))
            word = h2 >> _U(32 - self.wbits + (1 if mutation == "word" else 0))
            return ok & ((self.bloom[word.astype(np.int64)] & bits2) == bits2)
        # the level-0 forms probe ONE 12-mer per group of four positions, the one at 4 g + 3: at offset 3 - align of this k-mer
        y = (codes >> (_U(2) * (_U(3) - align))) & M24
        if self.tier == "level0":
            l0 = self.bloom0 if stage2 == "l2" else self.bloom0f
            g, bits = _three(y, BLOOM_C0)
            ok = (l0[((g >> _U(17)) & wmask0).astype(np.int64)] & bits) == bits
            if stage2 == "l2":
                return ok & self._block_passes(self.blkc, self.blkc_wbits, y, codes, 1 if mutation == "block" else 0)
            word, bits = _stage_bits(codes)
            return ok & ((self.bloom0f[word.astype(np.int64)] & bits) == bits)
        assert self.tier == "middle"
        key = canon12(y)
        g, bits = _three(key, BLOOM_C0)
        if self.mid0_bits == 1 and mutation != "mid0":
            bits = _b31(g)
        ok = (self.mid0[self.mid0_bits][((g >> _U(17)) & wmask0).astype(np.int64)] & bits) == bits
        ok &= (self.mid_bitmap[(key >> _U(5)).astype(np.int64)] & _bit(key & _U(31))) != 0
        return ok & self._block_passes(self.midc, self.midc_wbits, key, codes, 1 if mutation == "block" else 0)

    def index_rejected(self, stage2="lds", mutation=None):
        """index codes (both orientations) that the kernel would reject at any of the four alignments"""
        bad = np.zeros(len(self.codes), bool)
        for align in range(4):
            bad |= ~self.passes(self.codes, np.full(len(self.codes), align), stage2, mutation)
        return int(bad.sum())

    def selfcheck_fills(self):
        """level0_fill_permille, level12_fill_permille, stage2_fill_permille as PrgIndex::filter_selfcheck reports them for this tier"""
        if self.tier == "middle":
            return fill_permille(self.mid0[self.mid0_bits]), fill_permille(self.mid_bitmap), fill_permille(self.midc)
        if self.tier == "level0":
            return fill_permille(self.bloom0), fill_permille(self.bloom), fill_permille(self.bloomr)
        return (0, fill_permille(self.bloom), 0) if self.tier == "levels12" else (0, 0, 0)


# ---- panels -------------------------------------------------------------------------------------------------------------------------------
LOCUS_LENGTH, TAIL_MAX, POOL_SEED, TAIL_SEED = 3000, 9000, 91_000, 92_000
_CACHE = {}


def pool_locus(i):
    if ("locus", i) not in _CACHE:
        from drprg_amd import synth
        _CACHE["locus", i] = synth.random_seq(np.random.default_rng(POOL_SEED + i), LOCUS_LENGTH)
    return _CACHE["locus", i]


def tail_sequence(k, length):
    """the last locus of a threshold panel: a prefix of one random sequence per k"""
    if ("tail", k) not in _CACHE:
        from drprg_amd import synth
        _CACHE["tail", k] = synth.random_seq(np.random.default_rng(TAIL_SEED + k), TAIL_MAX)
    assert k <= length <= TAIL_MAX
    return _CACHE["tail", k][:length]


# name: (k, R below the edge, what changes there).  The panel above the edge has one base and one record more.
THRESHOLDS = {}
for _j in range(6):
    THRESHOLDS[f"words{8 + _j}_k13"] = (13, 160 << _j, f"levels 1+2: 2^{8 + _j} -> 2^{9 + _j} words")
THRESHOLDS["words13_k11"] = (11, 5120, "levels 1+2, k < 12: 2^13 -> 2^14 words")
THRESHOLDS["none_k13"] = (13, 24_576, "levels 1+2 -> no filter tier")
THRESHOLDS["none_k11"] = (11, 24_576, "levels 1+2, k < 12 -> no filter tier")
for _cw in range(10, 16):
    THRESHOLDS[f"blkc{_cw}"] = (15, 1 << (_cw - 1), f"small tier: 2^{_cw} -> 2^{_cw + 1} blocks")
THRESHOLDS["level0"] = (15, 21_845, "level 0 (all-LDS) -> middle tier")
for _cw in (15, 16, 17):
    THRESHOLDS[f"midc{_cw}"] = (15, 1 << _cw, f"middle tier: 2^{_cw} -> 2^{min(_cw + 1, MID_C_MAX_WBITS)} blocks" + (" (the cap)" if _cw == 17 else ""))
THRESHOLDS["direct"] = (15, MID_MAX_RECORDS, "middle tier -> direct sequence")
MID0_DISTINCT = (32 << L0_WBITS) * 2 // 5   # 419 430: the last count of canonical 12-mers that keeps three bits
MID0_MAX_RECORDS = 1_000_000                # DRPRG_MID_MAX_RECORDS for the MID0 pair: its 430 k records are past the default
SIDES = ("below", "above")


def threshold_cases():
    return [(name, side) for name in list(THRESHOLDS) + ["mid0"] for side in SIDES]


def _threshold_loci(k, n_records, n_pool):
    per = LOCUS_LENGTH - k + 1
    return [pool_locus(i) for i in range(n_pool)] + [tail_sequence(k, n_records - n_pool * per + k - 1)]


def _mid0_lengths():
    """(loci of the pool, length of the last locus below the edge): the pool's loci while their canonical 12-mers stay 3 000 under the edge,
    then the last locus base by base -- every base brings one 12-mer, a new one or not -- to the LAST length with 419 430 of them"""
    if "mid0" not in _CACHE:
        seen = np.zeros(1 << 24, bool)
        n_pool = 0
        while True:
            keys = canon12(codes_at(letters_of(pool_locus(n_pool)), np.arange(LOCUS_LENGTH - 11), 12)).astype(np.int64)
            if int(seen.sum()) + len(np.unique(keys[~seen[keys]])) > MID0_DISTINCT - 3000:
                break
            seen[keys] = True
            n_pool += 1
        tail = tail_sequence(15, TAIL_MAX)
        keys = canon12(codes_at(letters_of(tail), np.arange(len(tail) - 11), 12)).astype(np.int64)
        _, first = np.unique(keys, return_index=True)
        new = np.zeros(len(keys), bool)
        new[first] = True
        new &= ~seen[keys]
        total = int(seen.sum()) + np.cumsum(new)   # total[i]: the 12-mers at 0 .. i are in: a last locus of i + 12 bases
        at = np.nonzero(total == MID0_DISTINCT)[0]
        assert len(at) and total[at[-1] + 1] == MID0_DISTINCT + 1
        _CACHE["mid0"] = (n_pool, int(at[-1]) + 12)
    return _CACHE["mid0"]


def threshold_panel(name, side):
    """(panel, w, k, intended n_records)"""
    if ("tpanel", name, side) not in _CACHE:
        from drprg_amd import synth
        up = SIDES.index(side)
        if name == "mid0":
            k = 15
            n_pool, length = _mid0_lengths()
            loci = [pool_locus(i) for i in range(n_pool)] + [tail_sequence(k, length + up)]
            n_records = sum(len(s) - k + 1 for s in loci)
        else:
            k, below = THRESHOLDS[name][:2]
            n_records = below + up
            loci = _threshold_loci(k, n_records, (below - 1) // (LOCUS_LENGTH - k + 1))
        panel = synth.Panel([f"t{i}" for i in range(len(loci))], [[s] for s in loci])
        _CACHE["tpanel", name, side] = (panel, 1, k, n_records)
    return _CACHE["tpanel", name, side]


def mid_max_records(name):
    return MID0_MAX_RECORDS if name == "mid0" else MID_MAX_RECORDS


# name: (w, k, edge, aim for R).  Within 1 % below | above the edge
SITES = {"sites_below_level0": (11, 15, 21_845, 21_845 - 110), "sites_above_level0": (11, 15, 21_845, 21_845 + 110),
         "sites_below_none_k13": (14, 13, 24_576, 24_576 - 120)}
SITE_LOCI, SITE_LENGTH = 48, 4000   # (loci made; a panel takes as many of them as fit under its aim)


def sites_panel(oracle, name):
    """(panel, w, k, n_records): loci with sites and a last site-free locus whose length brings R to within 20 records of the aim"""
    if ("spanel", name) not in _CACHE:
        from drprg_amd import synth
        w, k, _, aim = SITES[name]
        base = synth.small_panel(seed=300 + k, n_loci=SITE_LOCI, length=SITE_LENGTH, site_every=400)
        records = np.cumsum([len(oracle.sketch_prg(p, w, k)["hash"]) for p in base.prgs])
        n_loci = int(np.searchsorted(records, aim - 400))   # as many loci as leave 400 records or more to the last one
        base, have = synth.Panel(base.names[:n_loci], base.trees[:n_loci]), int(records[n_loci - 1])
        tail = synth.random_seq(np.random.default_rng(TAIL_SEED + 100 + k), 3 * SITE_LENGTH)
        length = max(k + w, (aim - have) * (w + 1) // 2)
        for _ in range(40):
            assert k + w <= length <= len(tail), (name, have, length)
            n = have + len(oracle.sketch(tail[:length], w, k)[0])
            if abs(n - aim) <= 20:
                break
            length += (aim - n) * (w + 1) // 2 or (1 if aim > n else -1)
        assert abs(n - aim) <= 20, (name, n)
        _CACHE["spanel", name] = (synth.Panel(base.names + ["tail"], base.trees + [[tail[:length]]]), w, k, n)
    return _CACHE["spanel", name]


def all_cases():
    return [f"{n}-{s}" for n, s in threshold_cases()] + list(SITES)


def panel_of(oracle, case):
    """(panel, w, k, n_records, mid_max_records) of a case of all_cases()"""
    if case in SITES:
        return sites_panel(oracle, case) + (MID_MAX_RECORDS,)
    name, side = case.rsplit("-", 1)
    return threshold_panel(name, side) + (mid_max_records(name),)


def panel_codes(oracle, panel, w, k):
    """the index codes of a panel from the oracle's k-mer paths, PRG by PRG; a site-free locus's at w = 1 also straight from its sequence"""
    out = []
    for prg in panel.prgs:
        if ("codes", prg, w, k) not in _CACHE:
            codes, _ = oracle_codes(oracle, prg, w, k)
            if w == 1 and " " not in prg:
                assert np.array_equal(codes, sequence_codes(prg, k))
            _CACHE["codes", prg, w, k] = codes
        out.append(_CACHE["codes", prg, w, k])
    return out


def tables_of(oracle, case):
    if ("tables", case) not in _CACHE:
        panel, w, k, _, mid_max = panel_of(oracle, case)
        per_prg = panel_codes(oracle, panel, w, k)
        # (all forward codes, then all reverse complements: the order means nothing to the arrays)
        codes = np.concatenate([c[:len(c) // 2] for c in per_prg] + [c[len(c) // 2:] for c in per_prg])
        _CACHE["tables", case] = Tables(codes, k, mid_max)
    return _CACHE["tables", case]


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
READ_MAX, N_BACKGROUND, MCS = 4000, 2000, 2
_COMP = np.zeros(256, np.uint8)
_COMP[list(b"ACGT")] = list(b"TGCA")


def _cut(seq, k):
    """reads of at most READ_MAX bases that together hold every k-mer of seq"""
    s = np.frombuffer(seq.encode(), np.uint8)
    return [s[a:a + READ_MAX] for a in range(0, max(1, len(s) - k + 1), READ_MAX - k + 1)]


def batch_of(oracle, case):
    """(bases, offsets, section starts): the panel's sequences four times, section a beginning at a batch position that is a mod 4"""
    if ("batch", case) not in _CACHE:
        from drprg_amd import synth
        panel, w, k, _, _ = panel_of(oracle, case)
        rng = np.random.default_rng(500 + len(panel.prgs))
        if case in SITES:
            seqs = [synth.sample_haplotype(rng, t) for t in panel.trees for _ in range(2)]
        else:
            seqs = [t[0] for t in panel.trees]
        fw = [r for s in seqs for r in _cut(s, k)]
        section = fw + [_COMP[r[::-1]] for r in fw]
        size = sum(len(r) for r in section)
        filler = np.frombuffer(b"GATC", np.uint8)
        reads, starts, at = [], [], 0
        for a in range(4):
            pad = (a - at) % 4   # (a read of 0 .. 3 bases: shorter than any k here)
            if a:
                reads.append(filler[:pad])
                at += pad
            starts.append(at)
            reads += section
            at += size
        gen = synth.HaplotypeGenomes(panel, genome_size=2 * sum(len(r) for r in panel.refs), n_hap=2, seed=600 + k)
        bb, bo = synth.sample_short_reads(gen, N_BACKGROUND, seed=700 + k, sub_rate=0.01)
        back = [bb[int(a):int(b)].copy() for a, b in zip(bo[:-1], bo[1:])]
        for i in range(0, len(back), 10):
            back[i][int(rng.integers(0, 150))] = ord("N")
        g = gen.haps[0]
        tiny = [g[s:s + n] for s, n in zip(rng.integers(0, len(g) - 40, size=6).tolist(), (0, k - 1, 0, 1, k // 2, 0))]
        third = len(back) // 3
        reads += tiny[:2] + back[:third] + tiny[2:4] + back[third:2 * third] + tiny[4:] + back[2 * third:]
        offs = np.zeros(len(reads) + 1, np.uint64)
        offs[1:] = np.cumsum([len(r) for r in reads])
        _CACHE["batch", case] = (np.concatenate(reads), offs, starts)
    return _CACHE["batch", case]


def batch_hits(oracle, case):
    """every hit of the batch by the oracle's trace, read by read: dict(code, align, knode): the code of the read's k-mer at the hit's
    position (from the batch's own bytes), that position's place in the kernel's group of four, the global k-mer node"""
    if ("hits", case) not in _CACHE:
        from util import cluster_fraction, map_params
        panel, w, k, _, _ = panel_of(oracle, case)
        bases, offs, _ = batch_of(oracle, case)
        idx = oracle.build_index(panel.prgs, w, k)
        md, er = map_params(k, True)
        frac = float(cluster_fraction(er, k))
        pos, knode = [], []
        for a, b in zip(offs[:-1].tolist(), offs[1:].tolist()):
            if b - a >= k:
                t = oracle.read_clusters(bases[a:b], idx, w, k, md, frac, MCS)["hits"]
                pos.append(t["pos"].astype(np.int64) + a)
                knode.append(t["knode"].astype(np.int64))
        pos, knode = np.concatenate(pos), np.concatenate(knode)
        le = ((bases >> 1) & 3).astype(np.uint64)
        per_record = np.bincount(knode, minlength=int(idx["knode_base"][-1]))[idx["rec_knode"].astype(np.int64)]
        _CACHE["hits", case] = dict(code=codes_at(le, pos, k), align=(pos & 3).astype(np.uint64), pos=pos, per_record=per_record)
    return _CACHE["hits", case]


def forget(case):
    """drops a case's hits and tables (the largest batch has 3.7 M hits)"""
    for what in ("hits", "tables"):
        _CACHE.pop((what, case), None)


def forms_of(tier):
    """the second stages a tier runs with: the small tier has two"""
    return ("lds", "l2") if tier == "level0" else ("lds",)


def census(oracle, case):
    """hits of the batch that the restated kernel would lose: as it is (none may be), and under each wrong shift or test"""
    t, h = tables_of(oracle, case), batch_hits(oracle, case)
    out = dict(hits=len(h["code"]))
    if t.tier is None:
        return out
    for stage2 in forms_of(t.tier):
        tag = f"_{stage2}" if t.tier == "level0" else ""
        out["lost" + tag] = int((~t.passes(h["code"], h["align"], stage2)).sum())
    if t.tier == "levels12":
        out["lost_word_shift"] = int((~t.passes(h["code"], h["align"], mutation="word")).sum())
    if t.tier in ("level0", "middle"):
        out["lost_block_shift"] = int((~t.passes(h["code"], h["align"], "l2", mutation="block")).sum())
    if t.tier == "level0":
        without3 = Tables(t.codes, t.k, l0_offsets=(0, 1, 2))
        out["lost_without_offset3"] = int((~without3.passes(h["code"], h["align"], "l2")).sum())
    if t.tier == "middle" and t.mid0_bits == 1:
        out["lost_three_bit_test"] = int((~t.passes(h["code"], h["align"], mutation="mid0")).sum())
    return out
