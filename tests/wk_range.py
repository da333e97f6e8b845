"""The accepted (w, k) range at its edges: panels and read batches for the values of w and k at which the device code switches form.

Four groups, each built deterministically and returned with a census (tests/test_wk_range.py holds it on the CPU, tests/test_gpu_wk_range.py
maps the batches on the device):

  K_EDGE   the key-width switch at k = 15 | 16 (u32 | u64 keys, 12- | 16-byte slots, 1 << 2k = 2^32 at k = 16): one small panel with the
           palindrome and homopolymer strings of test_index_oracle.REPEAT_PRGS as extra loci, short and long reads and reads cut from those.
  W_EDGE   the window and the halo: halo = max(16, round16(w - 1)) shrinks a tile of sketch_probe_kernel to t_eval = 4096 - 2 halo positions.
           A batch is laid out base by base: `edge blocks` -- one stretch of a locus cut into consecutive reads that start at m * t_eval + d,
           d in OFFSETS(w, k), so a k-mer that straddles two of them IS a k-mer of the index --, between them reads of exactly w + k - 2,
           w + k - 1 and w + k bases, reads with one N that leaves runs of exactly w - 1 and w k-mers, 150-base reads, long reads, and an
           off-panel pad read sized so that the next block starts where it must.
  size_len the length-governed size threshold floor(fraction * 2 len / (w + 1)) at w = 199, 200, 201 -- either side of the w at which the
           device stops multiplying by a reciprocal and divides --, edge_reads' size_len recipe on its long locus, accepted by the trace.
  K_TINY   k <= 7: every key has many records; 150-base reads with more hits than the per-read kernels hold, and N-masked ones with few.

Nothing here looks at the product."""
import numpy as np

import edge_reads as E

K_EDGE = [(11, 15), (11, 16), (11, 17), (1, 16), (19, 16), (11, 31)]
W_EDGE = [20, 32, 33, 48, 49, 136, 137, 199, 200, 201, 512, 1023, 1024]
W_EDGE_K = (15, 21)
SIZE_LEN_W = (199, 200, 201)
K_TINY = [(3, 2), (5, 4), (11, 7), (16, 7), (1, 1)]
MCS = 2            # K_EDGE, K_TINY (Illumina parameters)
W_MCS = 1          # W_EDGE: at w = 1024 a 4 000-base locus holds eight minimizers
N_TILES = 66       # tiles of a W_EDGE batch
EDGE_TILES = (0, 4, 9, 15, 22, 30, 39, 49, 58, N_TILES - 1)
SK_NPOS = 4096     # positions of one tile of sketch_probe_kernel (csrc/sketch_probe.hip)
_CACHE = {}

rc, batch, _seq = E.rc, E.batch, E._seq


def halo(w):
    return max(16, (w - 1 + 15) // 16 * 16)


def t_eval(w):
    return SK_NPOS - 2 * halo(w)


def offsets_of(w, k):
    """the distances from a tile's first evaluated position at which reads must start"""
    return sorted({-(w - 1), -(k - 1), -1, 0, 1, k - 1, w - 1})


def w_illumina(w):
    """Illumina parameters (max_diff 2k + 1) while consecutive minimizers are that close, Nanopore (250) above"""
    return w <= 33


def all_wk():
    """every (w, k) of this module"""
    return K_EDGE + [(w, k) for k in W_EDGE_K for w in W_EDGE] + [(w, E.K) for w in SIZE_LEN_W] + K_TINY


# ---- key width ------------------------------------------------------------------------------------------------------------------------
REPEAT_LOCI = ("perfect_palindrome", "hairpin_with_a_3_base_loop", "homopolymer", "a_120")


def k_edge_panel():
    if "k_panel" not in _CACHE:
        from drprg_amd import synth
        from test_index_oracle import REPEAT_PRGS
        small = synth.small_panel(seed=16)
        _CACHE["k_panel"] = synth.Panel(small.names + list(REPEAT_LOCI), small.trees + [[REPEAT_PRGS[n]] for n in REPEAT_LOCI])
    return _CACHE["k_panel"]


def k_edge_reads():
    """(bases, offsets, census): 1 200 short reads, 40 long ones (1 500 .. 9 000 bases), and reads of 40 .. 150 bases cut at every fourth
    offset of the repeat loci, both strands"""
    if "k_reads" not in _CACHE:
        from drprg_amd import synth
        panel = k_edge_panel()
        gen = synth.HaplotypeGenomes(panel, genome_size=20000, n_hap=4, seed=3)
        sb, so = synth.sample_short_reads(gen, 1200, seed=5)
        lb, lo = synth.sample_long_reads(gen, 40, seed=6, mean_len=2500, min_len=1700, max_len=8000)  # (5 % indels: the lengths move a little)
        rng = np.random.default_rng(16)
        cut = []
        for name in REPEAT_LOCI:
            g = panel.refs[panel.names.index(name)].encode()
            for s in range(0, len(g) - 40, 4):
                r = g[s:s + int(rng.integers(40, 151))]
                cut.append(rc(r) if (s // 4) % 2 else r)
        cb, co = batch(cut)
        bases = np.concatenate([sb, lb, cb])
        offs = np.concatenate([so, lo[1:] + so[-1], co[1:] + so[-1] + lo[-1]]).astype(np.uint64)
        _CACHE["k_reads"] = (bases, offs, dict(short=len(so) - 1, long=len(lo) - 1, long_lengths=np.diff(lo.astype(np.int64)), cut=len(cut)))
    return _CACHE["k_reads"]


# ---- window and halo ------------------------------------------------------------------------------------------------------------------
def w_edge_panel():
    """(Panel, sequences): seven loci of 4 400 bases (an edge block at w = 1024 is 4 150 bases of one locus), one of them with two sites
    that no window of 1 024 k-mers spans both of"""
    if "w_panel" not in _CACHE:
        from drprg_amd import synth
        rng = np.random.default_rng(1024)
        seqs = [_seq(rng, 4400) for _ in range(7)]
        trees = [[s.decode()] for s in seqs]
        s = seqs[6].decode()
        trees[6] = [s[:1300], synth.Site([["A"], ["C"]]), s[1301:2700], synth.Site([["GT"], ["G"]]), s[2702:]]
        panel = synth.Panel([f"w{i}" for i in range(7)], trees)
        _CACHE["w_panel"] = (panel, [r.encode() for r in panel.refs])
    return _CACHE["w_panel"]


def boundary_reads(w, k, seqs, rng, n=6):
    """{'short' | 'one' | 'two': on-panel reads of w + k - 2 | w + k - 1 | w + k bases (one window short, one window, two windows)}"""
    out = {}
    for name, ln in (("short", w + k - 2), ("one", w + k - 1), ("two", w + k)):
        out[name] = []
        for i in range(n):
            g = seqs[i % len(seqs)]
            s = int(rng.integers(0, len(g) - ln + 1))
            out[name].append(g[s:s + ln] if i % 2 else rc(g[s:s + ln]))
    return out


def n_split_reads(w, k, seqs, rng, n=3):
    """on-panel reads with one N: the runs on its two sides hold (w - 1, w), (w, w - 1), (w - 1, many) and (many, w) k-mers"""
    out = []
    short, full = w + k - 2, w + k - 1  # bases of a run of w - 1 and of w k-mers
    for i in range(n):
        g = seqs[(i + 3) % len(seqs)]
        for left, right in ((short, full), (full, short), (short, 1500), (1500, full)):
            s = int(rng.integers(0, len(g) - (left + 1 + right) + 1))
            r = bytearray(g[s:s + left + 1 + right])
            r[left] = ord("N")
            out.append((bytes(r), left, right))
    return out


def w_edge_batch(w, k):
    """(bases, offsets, census) of the batch for (w, k); census: starts (the promised read starts), n_tiles, the indices of the boundary
    and N-split reads"""
    key = ("w_batch", w, k)
    if key in _CACHE:
        return _CACHE[key]
    panel, seqs = w_edge_panel()
    rng = np.random.default_rng(100 * w + k)
    te, ds = t_eval(w), offsets_of(w, k)
    n_bases = N_TILES * te - 5
    margin = w + k + 10
    fill = _seq(rng, 400000)
    reads, census = [], dict(starts=[], n_tiles=N_TILES, t_eval=te, short=[], one=[], two=[], n_split=[], long=0)
    pos = 0

    def put(r):
        nonlocal pos
        reads.append(r)
        pos += len(r)

    def block(m):
        """consecutive pieces of one locus, cut at m * te + d"""
        cuts = [m * te + d for d in ds if m * te + d > 0]
        first = max(0, cuts[0] - margin)
        last = min(n_bases, cuts[-1] + margin)
        g = seqs[m % len(seqs)]
        s = int(rng.integers(0, len(g) - (last - first) + 1))
        text = g[s:s + last - first] if m % 2 else rc(g)[s:s + last - first]
        return first, [first] + cuts + [last], text

    boundary = boundary_reads(w, k, seqs, rng)
    specials = [(name, r) for name in ("short", "one", "two") for r in boundary[name]] + [("n_split", r) for r in n_split_reads(w, k, seqs, rng)]
    specials = [specials[i] for i in rng.permutation(len(specials))]
    for m in EDGE_TILES:
        first, cuts, text = block(m)
        assert first >= pos, (w, k, m)
        # what lies between the previous block and this one: special reads, ordinary reads, and one pad read that ends at `first`
        gaps_left = sum(1 for x in EDGE_TILES if x >= m and x)
        quota = (len(specials) + gaps_left - 1) // gaps_left + 1 if m else 0
        while pos < first:
            room = first - pos
            fits = [i for i, (name, r) in enumerate(specials) if len(r[0] if name == "n_split" else r) < room] if quota else []
            if fits:
                name, r = specials.pop(fits[0])
                census[name].append((len(reads),) + r[1:] if name == "n_split" else len(reads))
                put(r[0] if name == "n_split" else r)
                quota -= 1
                continue
            kind = int(rng.integers(0, 8))
            if room > 6000 and kind < 2:        # a long read: a locus, or most of one, inside off-panel flanks
                g = seqs[int(rng.integers(0, len(seqs)))]
                a, b = sorted(int(x) for x in rng.integers(0, len(g), size=2))
                if b - a < 1500:
                    a, b = 0, len(g)
                pre, post = int(rng.integers(0, 700)), int(rng.integers(0, 700))
                f = int(rng.integers(0, len(fill) - 5000))
                r = fill[f:f + pre] + g[a:b] + fill[f + pre:f + pre + post]
                put(rc(r) if kind else r)
                census["long"] += 1
            elif room > 400 and kind < 7:       # a 150-base read of a locus
                g = seqs[int(rng.integers(0, len(seqs)))]
                s = int(rng.integers(0, len(g) - 150))
                put(rc(g[s:s + 150]) if kind % 2 else g[s:s + 150])
            else:                               # off-panel; the last one ends where the block starts
                ln = room if room <= 400 else int(rng.integers(30, 300))
                f = int(rng.integers(0, len(fill) - ln))
                put(fill[f:f + ln])
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a > first or m == 0:
                census["starts"].append((m, a - m * te))
            assert pos == a
            put(text[a - first:b - first])
    assert not specials, (w, k, len(specials))
    if pos < n_bases:
        put(fill[:n_bases - pos])
    bases, offs = batch(reads)
    assert int(offs[-1]) == n_bases
    _CACHE[key] = (bases, offs, census)
    return _CACHE[key]


# ---- the length-governed threshold at the reciprocal's limit --------------------------------------------------------------------------
def size_len_class(oracle, w):
    """edge_reads' size_len class at window w: Nanopore parameters, min_cluster_size 1, on the 72 000-base locus of edge_reads.sweep_panel()
    (on the 3 000-base loci of its main panel the PRG's shortest path would set the threshold at these w, not the read's length)"""
    key = ("size_len", w)
    if key not in _CACHE:
        _CACHE[key] = E._build_size(oracle, "len", False, E.FLOOR, w=w, panel="sweep", mcs=1)
    return _CACHE[key]


# ---- tiny k ---------------------------------------------------------------------------------------------------------------------------
def tiny_panel():
    """four loci of 300 bases: two with sites, one with a run of 60 A, one with a tandem repeat of period 3"""
    if "t_panel" not in _CACHE:
        from drprg_amd import synth
        rng = np.random.default_rng(7)
        small = synth.small_panel(seed=2, n_loci=2, length=300)
        poly = _seq(rng, 100) + b"A" * 60 + _seq(rng, 140)
        tandem = _seq(rng, 120) + b"CAG" * 20 + _seq(rng, 120)
        panel = synth.Panel(small.names + ["poly", "tandem"], small.trees + [[poly.decode()], [tandem.decode()]])
        _CACHE["t_panel"] = (panel, [r.encode() for r in panel.refs])
    return _CACHE["t_panel"]


def tiny_reads(w, k):
    """600 reads of 150 bases: on-panel, off-panel, across the A run, and on-panel reads masked with N but for one stretch of a few windows"""
    key = ("t_reads", w, k)
    if key not in _CACHE:
        _, seqs = tiny_panel()
        rng = np.random.default_rng(10 * w + k)
        reads = []
        for i in range(600):
            g = seqs[i % len(seqs)]
            s = int(rng.integers(0, len(g) - 150 + 1))
            r = g[s:s + 150]
            kind = i % 5
            if kind == 1:
                r = _seq(rng, 150)
            elif kind == 2:    # all N but a stretch of w + k - 1 .. w + k + 11 bases
                ln = int(rng.integers(w + k - 1, w + k + 12))
                a = int(rng.integers(0, 150 - ln + 1))
                r = b"N" * a + r[a:a + ln] + b"N" * (150 - a - ln)
            elif kind == 3:    # off-panel but for a stretch of the locus
                ln = int(rng.integers(k, 60))
                a = int(rng.integers(0, 150 - ln + 1))
                f = _seq(rng, 150)
                r = f[:a] + r[a:a + ln] + f[a + ln:]
            reads.append(rc(r) if i % 2 else r)
        _CACHE[key] = reads
    return _CACHE[key]


def tiny_census(oracle, w, k):
    """hits per read by the oracle's trace (Illumina parameters, min_cluster_size MCS)"""
    from util import cluster_fraction, map_params
    key = ("t_census", w, k)
    if key not in _CACHE:
        panel, _ = tiny_panel()
        idx = oracle.build_index(panel.prgs, w, k)
        md, er = map_params(k, True)
        frac = float(cluster_fraction(er, k))
        _CACHE[key] = np.array([len(oracle.read_clusters(r, idx, w, k, md, frac, MCS)["hits"]) for r in tiny_reads(w, k)])
    return _CACHE[key]
