"""Reads that sit exactly on a value one of the clustering rules compares with, and the same reads one value past it.

Every read is PROPOSED by a recipe -- exact-match blocks cut from a locus, separated by off-panel filler; one more filler base moves every
later hit by one position, one base less at the read's end removes hits one at a time -- and ACCEPTED by the oracle's trace of that read
(Oracle.read_clusters, the body of orc_map_reads' loop): the predicates below look at the trace only, never at the recipe's arithmetic.
A proposal the trace rejects is discarded.  tests/test_edge_reads.py holds the census (floors, properties, "decides something") on the CPU,
tests/test_gpu_rule_edges.py maps the classes on the device.

Panel (plain sequences, k = 15): `a` with a copy of its first half (`a_dup`) and a reverse-complemented copy of its last third (`a_rc`) --
reads from those stretches have hits in two (prg, strand) groups --, `b` on its own, two short PRGs whose shortest path sets the size
threshold, an inverted repeat, and pairs (`c`, `q*`) that share a stretch of sequence and part ways by one base right behind a minimizer."""
import numpy as np

from util import cluster_fraction, map_params

K = 15
FLOOR = 64          # accepted reads per class and technology
_RC = bytes.maketrans(b"ACGT", b"TGCA")
SWEEP_W = (11, 14, 15, 12)   # the two sketch_wave_kernel forms, w + 1 a power of two, w + 1 = 13
SWEEP_MAX = 700
SWEEP_LONG = (701, 1023, 1024, 1500, 2047, 4095, 4096, 8191, 16384, 32767, 32768, 50001, 65533, 65536, 69999, 70000)


def rc(s):
    return s.translate(_RC)[::-1]


def tech_params(illumina):
    md, er = map_params(K, illumina)
    return md, float(cluster_fraction(er, K))


class EdgeClass:
    """the accepted reads of one class: `on` the edge, `off` one value past it; everything a context needs to map them"""

    def __init__(self, name, rule, illumina, mcs, w=11, panel="main"):
        self.name, self.rule, self.illumina, self.mcs, self.w, self.panel = name, rule, illumina, mcs, w, panel
        self.on, self.off = [], []
        self.proposed = 0

    @property
    def key(self):
        return (self.panel, self.w, self.illumina, self.mcs)

    def reads(self):
        return self.on + self.off


def batch(reads):
    """(bases, offsets) of a list of reads (bytes)"""
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return (np.frombuffer(b"".join(reads), np.uint8).copy() if reads else np.zeros(0, np.uint8)), offs


# ---- panels ---------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])


def _sketch_pos(oracle, s, w):
    return [int(p) for p in oracle.sketch(s, w, K)[1]]


def _fork_loci(oracle, rng, c, n, w=11):
    """n sequences q = c[s : p + K] + x: the K-mer of c at p is a minimizer of q and of c (shared), q's last K-mer (at p + 1 of c, ending in
    x != c[p + K]) is a minimizer of q alone.  A read c[r : p + K] ends on the shared K-mer, the same read + x one position later on q only."""
    out, tried = [], set()
    mins = set(_sketch_pos(oracle, c, w))
    cand = [p for p in sorted(mins) if 120 <= p < len(c) - 40]
    rng.shuffle(cand)
    for p in cand:
        for x in b"ACGT":
            if x == c[p + K] or len(out) == n:
                continue
            s = p - int(rng.integers(45, 60))
            q = c[s:p + K] + bytes([x])
            pos = _sketch_pos(oracle, q, w)
            if len(pos) >= 4 and pos[-1] == p + 1 - s and pos[-2] == p - s and (p, x) not in tried:
                tried.add((p, x))
                out.append((s, p, q))
    assert len(out) == n, "no fork loci found: lengthen c"
    return out


def main_panel(oracle):
    """(Panel, dict of the sequences and fork points the recipes cut from)"""
    if "main" not in _CACHE:
        from drprg_amd import synth
        rng = np.random.default_rng(20261)
        a, b = _seq(rng, 3000), _seq(rng, 3000)
        x = _seq(rng, 300)
        c, d = _seq(rng, 1500), _seq(rng, 1500)
        forks = [(c,) + f for f in _fork_loci(oracle, rng, c, 6)] + [(d,) + f for f in _fork_loci(oracle, rng, d, 6)]
        seqs = dict(a=a, a_dup=a[:1500], a_rc=rc(a[2000:]), b=b, s200=_seq(rng, 200), s800=_seq(rng, 800),
                    inv=x + _seq(rng, 40) + rc(x) + _seq(rng, 60), c=c, d_rc=rc(d))
        for i, (base, _, _, q) in enumerate(forks):
            # c's forks as they are; d's reverse-complemented like d itself: a read cut from d meets the same fork on the other strand
            seqs[f"q{i}"] = q if base is c else rc(q)
        names = list(seqs)
        panel = synth.Panel(names, [[seqs[n].decode()] for n in names])
        _CACHE["main"] = (panel, dict(seqs=seqs, forks=forks, prg={n: i for i, n in enumerate(names)}))
    return _CACHE["main"]


def sweep_panel():
    if "sweep" not in _CACHE:
        from drprg_amd import synth
        rng = np.random.default_rng(20262)
        long = _seq(rng, 72000)
        seqs = dict(long=long, dup=long[:1200])
        _CACHE["sweep"] = (synth.Panel(list(seqs), [[s.decode()] for s in seqs.values()]), dict(seqs=seqs))
    return _CACHE["sweep"]


def panel_of(oracle, name):
    return main_panel(oracle) if name == "main" else sweep_panel()


class Tracer:
    """the oracle's trace of one read under one set of parameters"""
    _index = {}

    def __init__(self, oracle, panel_name, w, illumina, mcs, max_diff=None, fraction=None):
        self.oracle, self.w, self.mcs = oracle, w, mcs
        self.md, self.frac = tech_params(illumina)
        if max_diff is not None:
            self.md = max_diff
        if fraction is not None:
            self.frac = fraction
        key = (panel_name, w)
        if key not in Tracer._index:
            Tracer._index[key] = oracle.build_index(panel_of(oracle, panel_name)[0].prgs, w, K)
        self.idx = Tracer._index[key]

    def __call__(self, read):
        return self.oracle.read_clusters(read, self.idx, self.w, K, self.md, self.frac, self.mcs)

    def thr(self, length, min_path=0xFFFFFFFF, mcs=None):
        return self.oracle.cluster_threshold(length, self.w, self.frac, self.mcs if mcs is None else mcs, min_path)

    def kept(self, reads):
        """clusters_kept of the oracle's batch mapper over these reads"""
        bases, offs = batch(reads)
        return self.oracle.map_reads(bases, offs, self.idx, self.w, K, self.md, self.frac, self.mcs)[2]["clusters_kept"]


# ---- predicates: what a class claims, read off a trace ------------------------------------------------------------------------------------
def _largest(t):
    runs = t["runs"]
    return runs[int(np.argmax(runs["n"]))] if len(runs) else None


def is_gap(t, tr, side):
    """on: a kept cluster holds two consecutive hits exactly max_diff apart and neither part alone would pass its threshold;
    off: two runs of one group max_diff + 1 apart, neither passes, together they would"""
    if side == "on":
        for c in t["clusters"]:
            if not c["alive"]:
                continue
            pos = t["hits"]["pos"][c["first"]:c["first"] + c["n"]].astype(np.int64)
            d = np.diff(pos)
            for j in np.nonzero(d == tr.md)[0]:
                if j + 1 <= c["thr"] and c["n"] - (j + 1) <= c["thr"] and d.max() == tr.md:
                    return True
        return False
    runs = t["runs"]
    for r1, r2 in zip(runs[:-1], runs[1:]):
        if (r1["prg"], r1["fwd"]) == (r2["prg"], r2["fwd"]) and int(r2["first_pos"]) - int(r1["last_pos"]) == tr.md + 1 \
                and not r1["alive"] and not r2["alive"] and r1["n"] + r2["n"] > r1["thr"]:
            return len(t["clusters"]) == 0
    return False


def governs(t, tr, r):
    """which term of the threshold the run r was measured against sets it: 'mcs', 'path' or 'len' (None: two of them agree)"""
    idx_path = int(tr.idx["min_path_len"][r["prg"]])
    t_path, t_len = tr.thr(1 << 40, idx_path, mcs=0), tr.thr(t["length"], mcs=0)  # (each term alone, by the oracle's own function)
    if min(t_path, t_len) < tr.mcs:
        return "mcs" if r["thr"] == tr.mcs else None
    if t_path < t_len:
        return "path" if r["thr"] == t_path > tr.mcs else None
    if t_len < t_path:
        return "len" if r["thr"] == t_len > tr.mcs else None
    return None


def is_size(t, tr, side, term):
    """the read's largest run holds exactly thr hits (on: dropped, nothing of the read is kept) or thr + 1 (off: kept), and `term` sets thr"""
    r = _largest(t)
    if r is None or governs(t, tr, r) != term:
        return False
    if side == "on":
        return r["n"] == r["thr"] and not r["alive"] and len(t["clusters"]) == 0
    return r["n"] == r["thr"] + 1 and bool(r["alive"])


def sweep_state(t, tr, min_path):
    """(hits of the largest run, its threshold): a read without a hit is measured against the threshold a run of it would have met"""
    r = _largest(t)
    if r is None:
        return 0, tr.thr(t["length"], min_path)
    return int(r["n"]), int(r["thr"])


def is_sweep(t, tr, side, min_path):
    """on: the largest run is at its threshold or one hit short of it, nothing is kept; off: one hit past it.  (A read shorter than k + w - 1
    has no minimizer at all: the lengths below that are in the sweep with n = 0 against the threshold 1, only to show that the device keeps
    nothing there either.)"""
    n, thr = sweep_state(t, tr, min_path)
    return (thr - 1 <= n <= thr and len(t["clusters"]) == 0) if side == "on" else n == thr + 1


def _pair(t):
    cl = t["clusters"]
    return (cl[0], cl[1]) if len(cl) == 2 else (None, None)


def is_strand_tie(t, tr, side):
    """two clusters pass, same PRG, other strand.  on: equal sizes, the earlier one stays; off: one hit apart, the larger stays --
    'off' covers both ways round, is_strand_tie_later tells them apart"""
    c0, c1 = _pair(t)
    if c0 is None or c0["prg"] != c1["prg"] or c0["fwd"] == c1["fwd"] or c0["first_pos"] == c1["first_pos"]:
        return False
    if side == "on":
        return c0["n"] == c1["n"] and c0["alive"] and not c1["alive"]
    if c0["n"] == c1["n"] + 1:
        return bool(c0["alive"]) and not c1["alive"]
    return c1["n"] == c0["n"] + 1 and bool(c1["alive"]) and not c0["alive"]


def is_strand_tie_later(t):
    c0, c1 = _pair(t)
    return c0 is not None and bool(c1["alive"])


def is_containment(t, tr, side):
    """two clusters pass on two PRGs, the second starts later.  on: it ends where the first ends (the smaller dies); off: one position
    behind (both live)"""
    c0, c1 = _pair(t)
    if c0 is None or c0["prg"] == c1["prg"] or c1["first_pos"] <= c0["first_pos"] or c0["n"] == c1["n"]:
        return False
    if side == "on":
        return c1["last_pos"] == c0["last_pos"] and c0["alive"] + c1["alive"] == 1
    return c1["last_pos"] == c0["last_pos"] + 1 and c0["alive"] and c1["alive"]


def is_equal_first(t, tr, side):
    """two clusters pass on two PRGs with the same first position and different sizes: the larger is the first in cluster order and the one
    the smaller is measured against (it ends at or before the larger's end, so it dies)"""
    c0, c1 = _pair(t)
    if c0 is None or c0["prg"] == c1["prg"] or c1["first_pos"] != c0["first_pos"]:
        return False
    return c0["n"] > c1["n"] and c1["last_pos"] <= c0["last_pos"] and c0["alive"] and not c1["alive"]


def is_early_drop(t, tr, side):
    """hits in several (prg, strand) groups, all of them together exactly min_cluster_size (on) or one more (off)"""
    h = t["hits"]
    groups = len(set(zip(h["prg"].tolist(), h["fwd"].tolist())))
    return groups >= 2 and len(h) == tr.mcs + (0 if side == "on" else 1)


# ---- recipes --------------------------------------------------------------------------------------------------------------------------------
def _both_strands(read, i):
    return read if i % 2 == 0 else rc(read)


def _build_gap(oracle, illumina, n_pairs):
    cls = EdgeClass("gap_" + ("illumina" if illumina else "nanopore"), "gap", illumina, 10)
    tr = Tracer(oracle, "main", 11, illumina, 10)
    seqs = main_panel(oracle)[1]["seqs"]
    rng = np.random.default_rng(1 if illumina else 2)
    i = 0
    while len(cls.on) < n_pairs and cls.proposed < 60 * n_pairs:
        cls.proposed += 1
        src = seqs["b"] if cls.proposed % 2 else seqs["a"][:1500]  # (one group; two groups: the wave path of read_cluster_kernel)
        l1, l2 = (int(x) for x in rng.integers(45, 80, size=2))
        s1 = int(rng.integers(0, len(src) - l1 - l2 - 10))
        b1, b2 = src[s1:s1 + l1], src[s1 + l1 + 5:s1 + l1 + 5 + l2]
        fill = _seq(rng, 300)
        f0 = 8 if illumina else 230
        t = tr(b1 + fill[:f0] + b2)
        hits = t["hits"]
        g0 = hits[hits["prg"] == hits["prg"][0]] if len(hits) else hits
        if len(g0) < 4:
            continue
        f = f0 + tr.md - int(np.diff(np.sort(g0["pos"].astype(np.int64))).max())
        if f < 1 or f + 1 > len(fill):
            continue
        on = _both_strands(b1 + fill[:f // 2] + fill[len(fill) - (f - f // 2):] + b2, i)
        off = _both_strands(b1 + fill[:f // 2 + 1] + fill[len(fill) - (f - f // 2):] + b2, i)
        if is_gap(tr(on), tr, "on") and is_gap(tr(off), tr, "off"):
            cls.on.append(on)
            cls.off.append(off)
            i += 1
    return cls


def _walk_end(tr, cls, pred, make, lo, hi, i):
    """reads make(b) for b = hi down to lo (each step takes a base off the matching block): where make(b) is on the edge and make(b + 1) one
    past it, both are accepted"""
    prev = None
    for b in range(hi, lo - 1, -1):
        read = _both_strands(make(b), i)
        t = tr(read)
        if pred(t, "off"):
            prev = read
        elif pred(t, "on") and prev is not None:
            cls.on.append(read)
            cls.off.append(prev)
            return True
        else:
            prev = None
    return False


def _step_lengths(tr, w, lo, hi):
    """the read lengths in [lo, hi) at which floor(fraction * (2 len / (w + 1))) takes a value for the first time, and the length before each"""
    out = []
    for e in range(2 * lo // (w + 1), 2 * hi // (w + 1) + 1):
        length = (e * (w + 1) + 1) // 2  # the first length with 2 len / (w + 1) == e
        if lo <= length < hi and tr.thr(length, mcs=0) > tr.thr(length - 1, mcs=0):
            out += [length - 1, length]
    return out


def _bisect_block(tr, make, lo, hi):
    """narrows [lo, hi] to a dozen block lengths around the one at which the largest run of make(b) first exceeds its threshold (the hits grow
    with the block): _walk_end then takes them a base at a time"""
    over = lambda b: (lambda r: r is not None and r["n"] > r["thr"])(_largest(tr(make(b))))
    if over(lo) or not over(hi):
        return lo, lo
    while hi - lo > 8:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if over(mid) else (mid, hi)
    return max(K, lo - 2), hi + 2


def _build_size(oracle, term, illumina, n_pairs, w=11, panel="main", mcs=10):
    """w, panel, mcs: the `len` term at another window, on the long locus of sweep_panel() (tests/wk_range.py)"""
    tech = "illumina" if illumina else "nanopore"
    cls = EdgeClass(f"size_{term}_{tech}" + (f"_w{w}" if w != 11 else ""), "size_" + term, illumina, mcs, w=w, panel=panel)
    tr = Tracer(oracle, panel, w, illumina, mcs)
    seqs = panel_of(oracle, panel)[1]["seqs"]
    rng = np.random.default_rng(10 + 2 * ("mcs", "path", "len").index(term) + illumina + (1000 * w if w != 11 else 0))
    pred = lambda t, side: is_size(t, tr, side, term)
    i = 0
    steps = []
    while len(cls.on) < n_pairs and cls.proposed < 40 * n_pairs:
        cls.proposed += 1
        fill = _seq(rng, 3000 if panel == "main" else 6000)
        if term == "mcs":      # a block that holds about min_cluster_size hits; the read is short (Illumina) or its fraction small (Nanopore)
            src = seqs["b"] if i % 2 else seqs["a"][:1500]
            s = int(rng.integers(0, len(src) - 130))
            pad = int(rng.integers(0, 20)) if illumina else int(rng.integers(0, 300))
            make = lambda b: fill[:pad] + src[s:s + b]
            lo, hi = 40, 120
        elif term == "path":   # a read longer than the short PRG it matches a part of: floor(shortest path * fraction) hits are not enough
            src = seqs["s800"]
            total = 1000 + int(rng.integers(0, 200))
            s = int(rng.integers(0, 60))
            make = lambda b: fill[:100] + src[s:s + b] + fill[100:100 + total - 100 - b]
            lo, hi = (360, 520) if illumina else (60, 160)
        elif panel == "sweep":  # the same at a window of hundreds of k-mers: reads of thousands of bases, half of them of a length at which
            # the threshold steps (or one base short of it)
            src = seqs["long"][1300:]  # (behind the stretch the panel holds twice)
            if not steps:
                steps.extend(_step_lengths(tr, w, 1500, 6000))
            total = steps[cls.proposed // 2 % len(steps)] if cls.proposed % 2 else int(rng.integers(int((w + 1) / tr.frac) + 200, 6000))
            s = int(rng.integers(0, len(src) - total))
            make = lambda b: src[s:s + b] + fill[:total - b]
            lo, hi = K, min(total, 3 * (w + 1) + (w + 1) * tr.thr(total) // 2 * 3)
            lo, hi = _bisect_block(tr, make, lo, hi)
            hi = min(hi, total)
        else:                  # a read shorter than the locus: floor(2 len / (w + 1) * fraction)
            src = seqs["b"] if i % 2 else seqs["a"][:1500]
            total = int(rng.integers(140, 400)) if illumina else int(rng.integers(700, 1400))
            s = int(rng.integers(0, len(src) - total))
            make = lambda b: src[s:s + b] + fill[:total - b]
            lo, hi = (total * 2 // 5, min(total, total * 3 // 4)) if illumina else (60, 200)
        if _walk_end(tr, cls, pred, make, lo, hi, i):
            i += 1
    return cls


def _build_sweep(oracle, w, illumina):
    tech = "illumina" if illumina else "nanopore"
    cls = EdgeClass(f"sweep_w{w}_{tech}", "sweep", illumina, 1, w=w, panel="sweep")
    tr = Tracer(oracle, "sweep", w, illumina, 1)
    long = sweep_panel()[1]["seqs"]["long"]
    min_path = int(tr.idx["min_path_len"][0])
    rng = np.random.default_rng(100 + w * 2 + illumina)
    fill = _seq(rng, 72000)
    cls.lengths = {}

    def attempt(length, s, flip):
        """[(side, read)] of this length from the stretch of the locus at s: the longest block that does not pass and the block one base longer"""
        make = lambda b: (rc if flip else bytes)(long[s:s + b] + fill[:length - b])
        state = lambda b: sweep_state(tr(make(b)), tr, min_path)
        cls.proposed += 1
        lo, hi = 0, length
        n, thr = state(hi)
        if n <= thr:  # (too short to pass at all)
            return [("on", make(hi))] if is_sweep(tr(make(hi)), tr, "on", min_path) else []
        while hi - lo > 1:  # n - thr grows with the block, a hit at a time
            mid = (lo + hi) // 2
            n, thr = state(mid)
            cls.proposed += 1
            lo, hi = (lo, mid) if n > thr else (mid, hi)
        return [(side, make(b)) for side, b in (("on", lo), ("off", hi)) if is_sweep(tr(make(b)), tr, side, min_path)]

    for length in list(range(K, SWEEP_MAX + 1)) + list(SWEEP_LONG):
        got = []
        for go in range(8):
            if length > SWEEP_MAX:
                s = int(rng.integers(0, len(long) - length))
            elif (length + go) % 2:  # inside the duplicated stretch: two groups
                s = int(rng.integers(0, 300))
            else:
                s = int(rng.integers(1300, 60000))
            new = [x for x in attempt(length, s, (length + go) % 4 < 2) if x not in got]
            if go == 0 or len(got) < 2:
                got.extend(new)
            if len(got) >= 2:
                break
        for side, read in got:
            (cls.on if side == "on" else cls.off).append(read)
        cls.lengths[length] = len(got)
    return cls


def _build_strand_tie(oracle, n_each):
    cls = EdgeClass("strand_tie", "strand_tie", True, 10)
    tr = Tracer(oracle, "main", 11, True, 10)
    src = main_panel(oracle)[1]["seqs"]["s200"]
    rng = np.random.default_rng(30)
    cls.off_later = 0
    i = 0
    while (len(cls.on) < n_each or len(cls.off) < 2 * n_each or cls.off_later < n_each) and cls.proposed < 4000:
        cls.proposed += 1
        fill = _seq(rng, 200)
        l1 = int(rng.integers(120, 200))
        s1, s2 = int(rng.integers(0, 200 - l1 + 1)), int(rng.integers(0, 30))
        pad, gap = int(rng.integers(0, 30)), int(rng.integers(20, 60))
        for l2 in range(200 - s2, 110, -1):
            read = _both_strands(fill[:pad] + src[s1:s1 + l1] + fill[40:40 + gap] + rc(src[s2:s2 + l2]), i)
            t = tr(read)
            if is_strand_tie(t, tr, "on") and len(cls.on) < n_each + 8:
                cls.on.append(read)
            elif is_strand_tie(t, tr, "off"):
                later = is_strand_tie_later(t)
                if later or len(cls.off) - cls.off_later < n_each + 8:
                    cls.off.append(read)
                    cls.off_later += later
        i += 1
    return cls


def _build_forks(oracle, n_each):
    """containment and equal first position, from the fork loci: a read of c (or d) that ends on the shared K-mer (on) and the same read one
    base longer, its last K-mer on q alone (off); the reverse complement of the first STARTS on the shared K-mer: equal first positions"""
    cont = EdgeClass("containment", "containment", True, 2)
    eq = EdgeClass("equal_first", "equal_first", True, 2)
    tr = Tracer(oracle, "main", 11, True, 2)
    info = main_panel(oracle)[1]
    rng = np.random.default_rng(40)
    for c, s, p, q in info["forks"]:
        taken = 0
        for r0 in range(max(0, s - 110), s - 4):
            if taken >= 12:  # (of every fork alike: half of them are met on the other strand)
                break
            pad = _seq(rng, int(rng.integers(0, 12)))
            on, off = pad + c[r0:p + K], pad + c[r0:p + K] + q[-1:]
            cont.proposed += 1
            eq.proposed += 1
            if is_containment(tr(on), tr, "on") and is_containment(tr(off), tr, "off"):
                cont.on.append(on)
                cont.off.append(off)
                taken += 1
            if is_equal_first(tr(rc(on)), tr, "on"):
                eq.on.append(rc(on))
    return cont, eq


def _build_early_drop(oracle, mcs, n_each):
    cls = EdgeClass(f"early_drop_mcs{mcs}", "early_drop", True, mcs)
    tr = Tracer(oracle, "main", 11, True, mcs)
    a = main_panel(oracle)[1]["seqs"]["a"]
    rng = np.random.default_rng(50 + mcs)
    i = 0
    want_on = n_each if mcs > 1 else 0  # (a read with ONE hit has one group: with min_cluster_size 1 the edge has its far side only)
    while (len(cls.on) < want_on or len(cls.off) < n_each) and cls.proposed < 3000:
        cls.proposed += 1
        left = int(rng.integers(26, 26 + 6 * mcs))   # bases of the duplicated half (every hit there counts twice) ...
        fill = _seq(rng, 40)
        pad = int(rng.integers(0, 10))
        for right in range(0, 26 + 7 * mcs):         # ... and of the stretch behind it that `a` alone holds
            read = _both_strands(fill[:pad] + a[1500 - left:1500 + right], i)
            t = tr(read)
            if is_early_drop(t, tr, "on") and len(cls.on) < want_on + 8:
                cls.on.append(read)
            elif is_early_drop(t, tr, "off") and len(cls.off) < n_each + 8:
                cls.off.append(read)
        i += 1
    return cls


def build(oracle, n=FLOOR + 8):
    """every class, keyed by name"""
    if "classes" not in _CACHE:
        out = []
        for illumina in (True, False):
            out.append(_build_gap(oracle, illumina, n))
            for term in ("mcs", "path", "len"):
                out.append(_build_size(oracle, term, illumina, n))
            for w in SWEEP_W:
                out.append(_build_sweep(oracle, w, illumina))
        out.append(_build_strand_tie(oracle, n))
        out.extend(_build_forks(oracle, n))
        for mcs in (1, 2, 10):
            out.append(_build_early_drop(oracle, mcs, n))
        _CACHE["classes"] = {c.name: c for c in out}
    return _CACHE["classes"]


PREDICATES = {"gap": is_gap, "strand_tie": is_strand_tie, "containment": is_containment, "equal_first": is_equal_first,
              "early_drop": is_early_drop}


def holds(cls, tr, t, side):
    """does the trace t show what cls claims for `side`?"""
    if cls.rule.startswith("size_"):
        return is_size(t, tr, side, cls.rule[5:])
    if cls.rule == "sweep":
        return is_sweep(t, tr, side, int(tr.idx["min_path_len"][0]))
    return PREDICATES[cls.rule](t, tr, side)
