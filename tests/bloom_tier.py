"""The Bloom tier and the large probe table of the direct sequences: panels, read batches and a plain restatement of both structures.

An index of 65 536 distinct keys or more changes what sketch_wave_kernel and sketch_probe_kernel look a minimizer up in: the probe table
doubles to 2^18 slots (csrc/index.cpp: the smallest power of two >= 2 n + 1), and Mapper::IndexTables::fill (csrc/mapper.cpp) puts a Bloom
array in front of it once the table's 12 | 16 bytes per slot pass 2 MB.  The restatement below is written from csrc/kernels.h (pbloom_mix,
pbloom_word, pbloom_bits), csrc/index.h (table_slot) and csrc/index.cpp (the table's size, ascending insertion, linear probing) in plain
numpy; it never calls the product.  tests/test_bloom_tier.py holds the recipes' census on the CPU, tests/test_gpu_bloom_tier.py maps the
batches on the device.

  MATRIX     eight panels of 70 000 .. 125 000 keys (synth.small_panel(seed=5, site_every=400): a locus is a few kb), one per (w, k), each
             with the kernel sequences to run on it.  P0116 (k = 16) holds the 16-byte slots and NOT the fold of key >> 32 in pbloom_mix:
             every 16-mer's key fits 32 bits, its high half is zero.  P0521 and P1131 hold the fold: almost every key has a high half.
  THRESHOLD  w = 1, k = 15 | 16: three panels per k of exactly 65 535, 65 536 and 65 537 keys that differ only in the length of a last,
             site-free locus (17 bits, no tier | 18 bits, 2^14 words | 18 bits, 2^15 words).  The 65 535-key table is as full as the builder
             makes one (49.999 %).  THRESHOLD_SEED[k] is the first panel seed of 0 .. 199 whose 65 535-key table has a key whose chain runs
             from the last slot on to slot 0 (find_threshold_seed: a search over seeds on the CPU, no key is engineered); reads are planted
             over such keys and over keys stored four or more slots behind their home slot.
  batches    2 500 reads of 150 bases and 60 of 3 .. 9 kb (1 % errors) from two haplotype genomes twice the panel's size (the background
             gives the off-panel minimizers), three empty reads and three shorter than k, a non-ACGT byte in every tenth read."""
import numpy as np

# ---- the restatement --------------------------------------------------------------------------------------------------------------------
MUL32 = 0x9E3779B1              # kernels.h pbloom_mix, index.h table_slot (k <= 15)
MUL64 = 0x9E3779B97F4A7C15      # index.h table_slot (k >= 16)
TIER_ABOVE_BYTES = 2 << 20      # mapper.cpp: a table larger than this gets the Bloom array
WBITS_START, BITS_START = 10, 4
U32 = np.uint64(0xFFFFFFFF)


def slot_bytes(k):
    """bytes of one slot on the device: key (4 | 8) + record offset and count (8)"""
    return 12 if k <= 15 else 16


def table_bits(n_keys):
    bits = BITS_START
    while (1 << bits) < 2 * n_keys + 1:
        bits += 1
    return bits


def bloom_wbits(n_keys):
    wbits = WBITS_START
    while (4 << wbits) < n_keys:
        wbits += 1
    return wbits


def tier_present(n_keys, k):
    return (1 << table_bits(n_keys)) * slot_bytes(k) > TIER_ABOVE_BYTES


def pbloom_mix(keys):
    """((u32)key ^ (u32)(key >> 32)) * 0x9E3779B1, as u32"""
    keys = np.asarray(keys, np.uint64)
    return (((keys & U32) ^ (keys >> np.uint64(32))) * np.uint64(MUL32)) & U32


def mix_without_the_fold(keys):
    """what a lookup would mix that dropped the high half (the census measures how little of the index it would find)"""
    keys = np.asarray(keys, np.uint64)
    return ((keys & U32) * np.uint64(MUL32)) & U32


def bloom_word(m, wbits):
    return m >> np.uint64(32 - wbits)


def bloom_need(m):
    one = np.uint64(1)
    return (one << (m & np.uint64(31))) | (one << ((m >> np.uint64(5)) & np.uint64(31)))


def bloom_array(keys, wbits):
    arr = np.zeros(1 << wbits, np.uint64)
    m = pbloom_mix(keys)
    np.bitwise_or.at(arr, bloom_word(m, wbits).astype(np.int64), bloom_need(m))
    return arr


def bloom_passes(arr, wbits, keys, mix=pbloom_mix):
    m = mix(keys)
    need = bloom_need(m)
    return (arr[bloom_word(m, wbits).astype(np.int64)] & need) == need


def home_slots(keys, bits, k):
    keys = np.asarray(keys, np.uint64)
    if k <= 15:
        return ((((keys & U32) * np.uint64(MUL32)) & U32) >> np.uint64(32 - bits)).astype(np.int64)
    with np.errstate(over="ignore"):
        return ((keys * np.uint64(MUL64)) >> np.uint64(64 - bits)).astype(np.int64)  # (u64 arithmetic wraps)


def probe_table(keys, k):
    """(bits, slot, home) of every key: ascending keys, each put into the first free slot from its home slot on, around the end"""
    keys = np.asarray(keys, np.uint64)
    assert np.all(keys[1:] > keys[:-1])
    bits = table_bits(len(keys))
    mask = (1 << bits) - 1
    home = home_slots(keys, bits, k)
    taken = bytearray(1 << bits)
    slot = np.zeros(len(keys), np.int64)
    for i, s in enumerate(home.tolist()):
        while taken[s]:
            s = (s + 1) & mask
        taken[s] = 1
        slot[i] = s
    return bits, slot, home


class Tables:
    """the restated structures of one index (its sorted distinct keys)"""

    def __init__(self, keys, k):
        self.keys, self.k, self.n = np.asarray(keys, np.uint64), k, len(keys)
        self.bits, self.slot, self.home = probe_table(self.keys, k)
        self.mask = (1 << self.bits) - 1
        self.behind = (self.slot - self.home) & self.mask     # slots between a key and its home slot
        self.wraps = self.slot < self.home                    # its chain runs from the last slot on to slot 0
        self.other_group = (self.slot >> 2) != (self.home >> 2)  # not in the aligned group of four that table_find4 loads first
        self.tier = tier_present(self.n, k)
        self.wbits = bloom_wbits(self.n)
        self.bloom = bloom_array(self.keys, self.wbits)       # (restated whether the tier is present or not)
        self.load = self.n / float(1 << self.bits)

    def index_of(self, h):
        """(is an index key, its index among the keys) of every hash"""
        h = np.asarray(h, np.uint64)
        at = np.minimum(np.searchsorted(self.keys, h), self.n - 1)
        return self.keys[at] == h, at

    def passes(self, h, mix=pbloom_mix):
        return bloom_passes(self.bloom, self.wbits, h, mix)


# ---- the matrix panels ------------------------------------------------------------------------------------------------------------------
MCS = 2                 # min_cluster_size (Illumina parameters): at w = 33 a 150-base read holds eight minimizers
KEY_RANGE = (70_000, 125_000)
N_SHORT, N_LONG, LONG_MEAN = 2500, 60, 5500
# w = 33: a read's 3 .. 9 kb hold few minimizers; the long reads are as long as the range allows, and as many as keep the batch's mean read
# length under 300 bases (read_cluster_kernel sizes a chunk's look-ahead by it: only a read that outgrows the look-ahead is left over)
LONG_READS = {"P3315": (46, 8000)}
LDS = "lds"             # DRPRG_DIRECT_FORM
# name: (w, k, loci, length, [(kernel, DRPRG_DIRECT_FORM or None, sketch_form)])
MATRIX = {
    "P1415": (14, 15, 130, 4000, [(3, None, 1), (3, LDS, 2), (1, None, 2), (0, None, 12)]),
    "P1115": (11, 15, 110, 4000, [(3, LDS, 2)]),  # (test_gpu_parity.test_config4_500_locus_index holds forms 1 and 2's hit list at this (w, k))
    "P0313": (3, 13, 48, 4000, [(1, None, 3), (3, None, 3)]),
    "P0115": (1, 15, 24, 2900, [(1, None, 3), (3, None, 3)]),
    "P0116": (1, 16, 24, 2900, [(1, None, 4), (3, None, 4)]),
    "P0521": (5, 21, 70, 3500, [(1, None, 4), (3, None, 4)]),
    "P1131": (11, 31, 120, 4000, [(1, None, 4), (3, None, 4)]),
    "P3315": (33, 15, 330, 4000, [(1, None, 3), (3, None, 3)]),
}
# the seed of a panel's batch is 1000 + w.  P3315's is the first of 1033 .. 1040 at which, counting the keyed minimizers of every read in
# batch order by the oracle's sketch, three long reads begin in one run of 1 920 candidates and end past its 2 048th (what read_cluster_kernel
# owns and stages): most seeds give one or two such reads, some none, and the candidate form's cases want the expand path behind the tier run
BATCH_SEED = {"P3315": 1038}
FOLDED = ("P0521", "P1131")  # the panels on which the fold of key >> 32 decides
_CACHE = {}


def matrix_cases():
    """[(panel, kernel, DRPRG_DIRECT_FORM or None, sketch_form)]"""
    return [(name, kernel, env, form) for name, (_, _, _, _, forms) in MATRIX.items() for kernel, env, form in forms]


def matrix_panel(name):
    if ("panel", name) not in _CACHE:
        from drprg_amd import synth
        _, _, n_loci, length, _ = MATRIX[name]
        _CACHE["panel", name] = synth.small_panel(seed=5, n_loci=n_loci, length=length, site_every=400)
    return _CACHE["panel", name]


def matrix_batch(name):
    """(bases, offsets) of the panel's one batch"""
    if ("batch", name) not in _CACHE:
        n_long, mean = LONG_READS.get(name, (N_LONG, LONG_MEAN))
        _CACHE["batch", name] = batch_of(matrix_panel(name), MATRIX[name][1], seed=BATCH_SEED.get(name, 1000 + MATRIX[name][0]), n_long=n_long,
                                         long_mean=mean)[:2]
    return _CACHE["batch", name]


# ---- read batches -----------------------------------------------------------------------------------------------------------------------
def genomes_of(panel, seed):
    from drprg_amd import synth
    return synth.HaplotypeGenomes(panel, genome_size=2 * sum(len(r) for r in panel.refs), n_hap=2, seed=seed)


def batch_of(panel, k, seed, planted=(), genomes=None, n_long=N_LONG, long_mean=LONG_MEAN):
    """(bases, offsets, index of the first planted read): half the short reads, the long reads, the other half, the planted reads, with
    three empty reads and three shorter than k among them; then every tenth read gets one non-ACGT byte"""
    from drprg_amd import synth
    gen = genomes or genomes_of(panel, seed)
    sb, so = synth.sample_short_reads(gen, N_SHORT, seed=seed + 1)
    lb, lo = synth.sample_long_reads(gen, n_long, seed=seed + 2, mean_len=long_mean, sigma=0.35 if long_mean < 7000 else 0.08, min_len=3100,
                                     max_len=8800, err=0.01)  # (1 % indels: the lengths move a little, and stay within 3 .. 9 kb)
    short = [sb[int(a):int(b)] for a, b in zip(so[:-1], so[1:])]
    long_ = [lb[int(a):int(b)] for a, b in zip(lo[:-1], lo[1:])]
    rng = np.random.default_rng(seed + 3)
    g = gen.haps[0]
    tiny = [g[s:s + n] for s, n in zip(rng.integers(0, len(g) - 40, size=6).tolist(), (0, k - 1, 0, 1, k // 2, 0))]
    half = N_SHORT // 2
    reads = tiny[:2] + short[:half] + tiny[2:4] + long_ + short[half:] + tiny[4:]
    first_planted = len(reads)
    reads += [np.asarray(r, np.uint8) for r in planted]
    reads = [r.copy() for r in reads]
    for i in range(0, len(reads), 10):
        if len(reads[i]):
            reads[i][int(rng.integers(0, len(reads[i])))] = ord("N")
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads), offs, first_planted


def read_minimizers(oracle, bases, offs, w, k):
    """(hash of every minimizer of every read, the read it belongs to), by the oracle's sketch"""
    text = bases.tobytes()
    hs, rs = [], []
    for i, (a, b) in enumerate(zip(offs[:-1].tolist(), offs[1:].tolist())):
        if b - a >= k:
            h = oracle.sketch(text[a:b], w, k)[0]
            hs.append(h)
            rs.append(np.full(len(h), i, np.int64))
    return np.concatenate(hs), np.concatenate(rs)


def census(oracle, tables, bases, offs, w, k):
    """what the batch's minimizers meet in the restated structures (counts of minimizers, not of distinct hashes)"""
    h, read = read_minimizers(oracle, bases, offs, w, k)
    keyed, at = tables.index_of(h)
    passes = tables.passes(h)
    at = at[keyed]
    return dict(minimizers=len(h), keyed=int(keyed.sum()), keyed_rejected=int((keyed & ~passes).sum()), rejected=int((~passes).sum()),
                pass_not_key=int((passes & ~keyed).sum()), other_group=int(tables.other_group[at].sum()),
                behind4=int((tables.behind[at] >= 4).sum()), wrapping=int(tables.wraps[at].sum()),
                keyed_found_without_the_fold=int(tables.passes(h[keyed], mix_without_the_fold).sum()))


# ---- the threshold panels ---------------------------------------------------------------------------------------------------------------
THRESHOLD_K = (15, 16)
THRESHOLD_KEYS = (65_535, 65_536, 65_537)
THRESHOLD_LOCI, THRESHOLD_LENGTH, TAIL_MAX = 20, 2850, 6000   # ~63 000 keys at w = 1; the last locus brings the count to the key
THRESHOLD_SEED = {15: 3, 16: 12}      # find_threshold_seed's answers (seeds 0 .. 2 | 0 .. 11 give no wrapping chain)
N_PLANTED = 40


def tail_lengths(oracle, base, tail, k):
    """{n_keys: length of the last locus} for THRESHOLD_KEYS, or None if this base panel and tail cannot reach them.  w = 1: a locus of L
    bases brings the k-mers at 0 .. L - k, and each is a key"""
    have = oracle.build_index(base.prgs, 1, k)["keys"]
    h, p, _ = oracle.sketch(tail, 1, k)
    assert np.array_equal(p, np.arange(len(tail) - k + 1))
    _, first = np.unique(h, return_index=True)
    new = np.zeros(len(h), bool)
    new[first] = True
    new &= ~np.isin(h, have)
    total = len(have) + np.cumsum(new)
    out = {}
    for n in THRESHOLD_KEYS:
        hit = np.nonzero(total == n)[0]
        if len(have) >= n or not len(hit):
            return None
        out[n] = int(hit[0]) + k
    return out


def _threshold_parts(seed):
    from drprg_amd import synth
    base = synth.small_panel(seed=seed, n_loci=THRESHOLD_LOCI, length=THRESHOLD_LENGTH, site_every=400)
    tail = synth.random_seq(np.random.default_rng(70_000 + seed), TAIL_MAX)
    return base, tail


def threshold_panel(oracle, k, n_keys, seed=None):
    seed = THRESHOLD_SEED[k] if seed is None else seed
    if ("tpanel", k, n_keys, seed) not in _CACHE:
        from drprg_amd import synth
        base, tail = _threshold_parts(seed)
        lengths = tail_lengths(oracle, base, tail, k)
        assert lengths, (k, seed)
        for n, length in lengths.items():
            _CACHE["tpanel", k, n, seed] = synth.Panel(base.names + ["tail"], base.trees + [[tail[:length]]])
    return _CACHE["tpanel", k, n_keys, seed]


def threshold_tables(oracle, k, n_keys, seed=None):
    seed = THRESHOLD_SEED[k] if seed is None else seed
    if ("ttables", k, n_keys, seed) not in _CACHE:
        _CACHE["ttables", k, n_keys, seed] = Tables(oracle.build_index(threshold_panel(oracle, k, n_keys, seed).prgs, 1, k)["keys"], k)
    return _CACHE["ttables", k, n_keys, seed]


def find_threshold_seed(oracle, k, seeds=range(200)):
    """the first seed whose 65 535-key table has a wrapping chain (None: none of them has).  THRESHOLD_SEED records the answer"""
    for seed in seeds:
        base, tail = _threshold_parts(seed)
        if tail_lengths(oracle, base, tail, k) and threshold_tables(oracle, k, THRESHOLD_KEYS[0], seed).wraps.any():
            return seed
    return None


def planted_reads(oracle, tables, genomes, k, which, n=N_PLANTED):
    """150-base reads of the haplotypes over up to n positions whose k-mer is a key of the class `which` (a mask over the keys)"""
    want = tables.keys[which]
    out = []
    for hap in genomes.haps:
        h, p, _ = oracle.sketch(hap.tobytes(), 1, k)
        for pos in p[np.isin(h, want)].tolist():
            s = min(max(0, pos - 60), len(hap) - 150)
            out.append(hap[s:s + 150])
    step = max(1, len(out) // n)
    return out[::step][:n]


def threshold_batch(oracle, k, n_keys):
    """(bases, offsets, index of the first planted read): the planted reads cover every wrapping key the haplotypes hold and N_PLANTED
    positions of keys four or more slots behind their home slot"""
    if ("tbatch", k, n_keys) not in _CACHE:
        panel, tables = threshold_panel(oracle, k, n_keys), threshold_tables(oracle, k, n_keys)
        gen = genomes_of(panel, seed=2000 + k)
        planted = planted_reads(oracle, tables, gen, k, tables.wraps) + planted_reads(oracle, tables, gen, k, tables.behind >= 4)
        _CACHE["tbatch", k, n_keys] = batch_of(panel, k, seed=2000 + k, planted=planted, genomes=gen)
    return _CACHE["tbatch", k, n_keys]
