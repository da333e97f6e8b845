"""Reads over repeats, palindromes and homopolymers: the inputs on which two k-mers of one window share a canonical hash, so that the
"ties kept" sentence of DESIGN section 4 (and strand = fwd <= rc) decides the result.

lc_panel() is a dozen loci, each random flanks around one repeat feature; reads(w, k) draws a batch across them; census(oracle,
w, k) sorts the reads into classes.  A read is PROPOSED by a recipe and ACCEPTED into a class by the oracle's trace of it
(Oracle.read_clusters) and the plain rule of tests/minimizer_rule.py -- never by the recipe.  Classes (a read may be in several):

  tandem      a window holds >= 2 keyed minimizers (hash is an index key) of equal hash on the same strand
  strand      a window holds >= 2 keyed minimizers of equal hash on opposite strands
  cut         a keyed minimizer with a tied partner d < w positions to one side, whose partner d positions to the OTHER side is removed:
              it lies across the read's end or holds a letter that is not ACGT, and agrees with the k-mer in every base the read does hold
  run_short   a tied run (maximal stretch of k-mer positions p with hash(p) == hash(p + d), one d < w) exactly w - 1 k-mers long
  run_window  ... exactly w k-mers long (one full tied window)
  run_long    ... at least 2w - 1 k-mers long (more than the steps verify_one_lane walks); each run holding >= 2 keyed minimizers
  double      a keyed minimizer whose key has >= 2 records of one PRG and strand (two hits at one read position in one group)
  selfcomp    (even k) a keyed minimizer whose k-mer is its own reverse complement

An accepted read has a cluster the oracle keeps that holds a hit at one of the class's own positions, so the tied hits land in the coverage
vector.  For the tie and run classes the leftmost-only or the rightmost-only mutant of the rule gives another set of keyed minimizers on
the read (and each of the two does on at least FLOOR reads of the class); for selfcomp the strand mutant (fwd < rc) does.

Census at this commit (tests/test_low_complexity.py prints it on failure).  The reads of a batch are in random order and are classified until
every class holds FLOOR accepted reads and each one-sided mutant changes FLOOR reads of every tie class -- `first n of m` --, so a count of
exactly 64 is where the count stopped; the device maps all m.  In brackets: the reads of the class the leftmost-only / rightmost-only
mutant changes.
  (w=11, k=15) first 493 of 5747 reads: double 351, tandem 289 (left 239, right 247), strand 105 (left 104, right 105), cut 270 (left 221, right 231), run_window 71 (left 64, right 66), run_long 105 (left 92, right 97), run_short 129 (left 106, right 111)
  (w=14, k=15) first 584 of 5814 reads: double 417, tandem 345 (left 279, right 291), strand 109 (left 108, right 105), cut 323 (left 259, right 276), run_window 128 (left 114, right 117), run_long 121 (left 98, right 105), run_short 76 (left 64, right 64)
  (w=1, k=15) first 94 of 2504 reads: double 64
  (w=16, k=15) first 558 of 5937 reads: double 406, tandem 339 (left 275, right 276), strand 85 (left 82, right 80), cut 318 (left 258, right 260), run_window 100 (left 89, right 83), run_long 101 (left 88, right 81), run_short 77 (left 64, right 68)
  (w=12, k=15) first 547 of 5798 reads: double 402, tandem 334 (left 280, right 283), strand 108 (left 107, right 107), cut 314 (left 267, right 266), run_window 116 (left 109, right 110), run_long 123 (left 107, right 104), run_short 80 (left 64, right 70)
  (w=5, k=9) first 913 of 5050 reads: double 608, tandem 439 (left 345, right 367), strand 180 (left 165, right 166), cut 420 (left 329, right 353), run_window 131 (left 108, right 120), run_long 166 (left 140, right 145), run_short 103 (left 64, right 73)
  (w=16, k=13) first 511 of 5814 reads: double 371, tandem 311 (left 285, right 274), strand 80 (left 76, right 77), cut 291 (left 268, right 256), run_window 76 (left 67, right 64), run_long 90 (left 79, right 76), run_short 102 (left 99, right 97)
  (w=11, k=14) first 883 of 5695 reads: double 667, tandem 520 (left 436, right 432), strand 111 (left 110, right 106), cut 487 (left 409, right 402), run_window 199 (left 178, right 181), run_long 202 (left 186, right 176), run_short 103 (left 71, right 70), selfcomp 64
  (w=7, k=12) first 940 of 5347 reads: double 663, tandem 521 (left 421, right 433), strand 91 (left 65, right 76), cut 482 (left 393, right 406), run_window 200 (left 164, right 175), run_long 224 (left 184, right 183), run_short 97 (left 64, right 71), selfcomp 114
  (w=5, k=8) first 2981 of 4994 reads: double 2196, tandem 1358 (left 1120, right 1111), strand 90 (left 68, right 68), cut 1267 (left 1039, right 1040), run_window 447 (left 404, right 397), run_long 492 (left 411, right 422), run_short 144 (left 81, right 64), selfcomp 677
  (w=19, k=21) first 637 of 6517 reads: double 394, tandem 341 (left 303, right 303), strand 73 (left 71, right 71), cut 308 (left 275, right 275), run_window 85 (left 84, right 85), run_long 75 (left 64, right 71), run_short 109 (left 98, right 93)
  (w=11, k=31) first 725 of 6592 reads: double 470, tandem 363 (left 336, right 334), strand 89 (left 89, right 89), cut 340 (left 317, right 314), run_window 103 (left 96, right 97), run_long 72 (left 64, right 68), run_short 175 (left 166, right 172)
  (w=11, k=20) first 868 of 5990 reads: double 609, tandem 500 (left 434, right 451), strand 77 (left 66, right 64), cut 464 (left 406, right 419), run_window 166 (left 149, right 148), run_long 158 (left 131, right 138), run_short 115 (left 96, right 108), selfcomp 70
  (w=11, k=30) first 1788 of 6548 reads: double 1072, tandem 790 (left 685, right 685), strand 145 (left 143, right 141), cut 724 (left 635, right 628), run_window 322 (left 304, right 296), run_long 217 (left 183, right 187), run_short 128 (left 107, right 109), selfcomp 64
"""
import numpy as np

import minimizer_rule as R
from util import cluster_fraction, map_params

FLOOR = 64
MCS = 2
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
# every (w, k) tests/test_gpu_low_complexity.py maps
WK = [(11, 15), (14, 15), (1, 15), (16, 15), (12, 15), (5, 9), (16, 13), (11, 14), (7, 12), (5, 8), (19, 21), (11, 31), (11, 20), (11, 30)]
TIE_CLASSES = ("tandem", "strand", "cut", "run_short", "run_window", "run_long")
CLASSES = TIE_CLASSES + ("double", "selfcomp")
_CACHE = {}


def rc(s):
    return s.translate(_RC)[::-1]


def _seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])


def applicable(w, k):
    """the classes that can exist at (w, k): a window of one k-mer holds no tie, a run of w - 1 k-mers holds one only from w = 3 on, and an
    odd k-mer is never its own reverse complement"""
    out = ["double"]
    if w >= 2:
        out += ["tandem", "strand", "cut", "run_window", "run_long"]
    if w >= 3:
        out.append("run_short")
    if k % 2 == 0:
        out.append("selfcomp")
    return out


# ---- the panel ----------------------------------------------------------------------------------------------------------------------------
def lc_panel():
    """(Panel, {locus name: [(start, end) of every repeat feature on the locus' first-allele sequence]})"""
    if "panel" in _CACHE:
        return _CACHE["panel"]
    from drprg_amd import synth
    rng = np.random.default_rng(20270)
    S = lambda *alleles: synth.Site([[a] for a in alleles])
    F = lambda n=130: ("flank", _seq(rng, n).decode())
    rep = lambda s: ("feature", s)
    x = [_seq(rng, 45) for _ in range(6)]
    y = [_seq(rng, 40) for _ in range(4)]
    u = _seq(rng, 110).decode()
    unit5 = "GACCT"
    loci = {
        "homopolymer": [F(), rep("A" * 52), F(), rep("C" * 41), F()],
        "ac": [F(), rep("AC" * 34), F()],
        "cgg_site": [F(), rep("CGG" * 14), rep(S("CGG", "CGA")), rep("CGG" * 14), F()],
        "period7": [F(), rep("GACTTCA" * 11), F()],
        "palindromes": sum([[F(60), rep((s + rc(s)).decode())] for s in x], []) + [F(40)],
        "hairpins": sum([[F(60), rep((s + b"ACG" + rc(s)).decode())] for s in y], []) + [F(40)],
        "direct_repeat": [F(), rep(u), F(25), rep(u), F()],
        "t_run_site": [F(), rep("T" * 24), rep(S("T", "C")), rep("T" * 24), F()],
        "unit_site": [F(), rep(unit5 * 6), rep(S(unit5, unit5 * 2)), rep(unit5 * 6), F()],
        "empty_allele": [F(), rep("G" * 22), rep(S("G", "")), rep("G" * 22), F()],
        "at_cg": [F(), rep("AT" * 30), F(), rep("CG" * 30), F(), rep("TA" * 12 + "T"), F()],
        "periods": sum([[F(30), rep((_seq(rng, d).decode() * (60 // d + 2))[:60 + d])] for d in (3, 4, 6, 9, 11, 12)], [])
        + [F(30)],
    }
    spans, trees = {}, []
    for name, parts in loci.items():
        pos, sp, tree = 0, [], []
        for kind, seg in parts:
            n = len(seg) if isinstance(seg, str) else len(seg.alleles[0][0])
            if kind == "feature":
                if sp and sp[-1][1] == pos:
                    sp[-1] = (sp[-1][0], pos + n)
                else:
                    sp.append((pos, pos + n))
            pos += n
            if isinstance(seg, str) and tree and isinstance(tree[-1], str):
                tree[-1] += seg
            else:
                tree.append(seg)
        assert 300 <= pos <= 1500, (name, pos)
        spans[name] = sp
        trees.append(tree)
    _CACHE["panel"] = (synth.Panel(list(loci), trees), spans)
    return _CACHE["panel"]


# ---- the reads ----------------------------------------------------------------------------------------------------------------------------
def batch(reads):
    """(bases, offsets) of a list of reads (bytes)"""
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return (np.frombuffer(b"".join(reads), np.uint8).copy() if reads else np.zeros(0, np.uint8)), offs


def reads(w, k, n_random=400):
    """the proposals for (w, k), in a fixed order: reads that start or end at every offset of every feature, one N (or another letter that is
    not ACGT) at every offset of every feature, random reads of 60 .. 300 bases across the features of random haplotypes, a few of 700 and
    3000 bases; both strands, one in eight in lower case, one in six with a substitution or two"""
    key = ("reads", w, k, n_random)
    if key in _CACHE:
        return _CACHE[key]
    from drprg_amd import synth
    panel, spans = lc_panel()
    rng = np.random.default_rng(1000 * w + k)
    refs = {n: r.encode() for n, r in zip(panel.names, panel.refs)}
    haps = {n: [synth.sample_haplotype(rng, t).encode() for _ in range(3)] for n, t in zip(panel.names, panel.trees)}
    span = k + w + 20
    out = []
    period = lambda g, a, b: next((d for d in range(1, (b - a) // 2) if g[a + d:b] == g[a:b - d]), b - a)
    # how many features can hold a tie in a stretch of t bases (their period is at most t - k): the run-limit reads are shared among them
    short_period = {t: max(1, sum(period(refs[n], a, b) <= t - k and t <= b - a for n in panel.names for a, b in spans[n]))
                    for t in (k + w - 2, k + w - 1)}

    def finish(r):
        if len(r) < 60:  # (cut short by the locus' end)
            return
        r = bytearray(r)
        if rng.random() < 1 / 6:
            for p in rng.integers(0, len(r), size=int(rng.integers(1, 3))):
                r[p] = b"ACGT"[int(rng.integers(0, 4))]
        r = bytes(r)
        if rng.random() < 0.5:
            r = rc(r)
        out.append(r.lower() if rng.random() < 1 / 8 else r)

    for name in panel.names:
        g = refs[name]
        for a, b in spans[name]:
            for e in range(a, min(b, a + span) + 1):  # (every offset of the feature's first k + w + 20 bases: every phase of its period)
                ln = int(rng.integers(max(60, k + w + 8), 160))
                if e % 2:  # the read ends at e ...
                    finish(g[max(0, e - ln):e])
                else:      # ... or starts there
                    finish(g[e:e + ln])
            d = period(g, a, b)
            for t, budget in ((k + w - 2, 2400), (k + w - 1, 400)):  # (the read's end leaves exactly w - 1 and w k-mers of the feature)
                if d > t - k or t > b - a:
                    continue
                for _ in range(max(1, budget // (2 * short_period[t]))):
                    ln = int(rng.integers(max(60, t + 20), 160))
                    finish(g[max(0, a + t - ln):a + t])
                    finish(g[b - t:b - t + ln])
            for e in range(a, min(b, a + span)):
                ln = int(rng.integers(max(60, 2 * (k + w)), 200))
                s = max(0, min(len(g) - ln, e - int(rng.integers(k, ln - k))))
                r = bytearray(g[s:s + ln])
                r[e - s] = b"NNNnRYKM"[int(rng.integers(0, 8))]
                finish(bytes(r))
    names = panel.names
    for i in range(n_random):
        name = names[i % len(names)]
        g = haps[name][i % 3]
        a, b = spans[name][int(rng.integers(0, len(spans[name])))]
        ln = int(rng.integers(60, 301))
        c = int(rng.integers(a, b + 1))
        s = max(0, min(len(g) - ln, c - int(rng.integers(0, ln))))
        finish(g[s:s + ln])
    for i, name in enumerate(names):  # long reads: the locus inside off-panel sequence
        g = haps[name][0]
        for total in (700, 3000):
            pre = int(rng.integers(0, max(1, total - len(g))))
            finish((_seq(rng, pre) + g + _seq(rng, max(0, total - pre - len(g))))[:max(total, 0)])
    out = [out[i] for i in rng.permutation(len(out))]
    _CACHE[key] = out
    return out


# ---- classification -----------------------------------------------------------------------------------------------------------------------
class Tracer:
    """the oracle's index of lc_panel() and its trace of one read, at one (w, k) (Illumina parameters, min_cluster_size 2)"""

    def __init__(self, oracle, w, k):
        self.oracle, self.w, self.k = oracle, w, k
        md, er = map_params(k, True)
        self.md, self.frac = md, float(cluster_fraction(er, k))
        self.idx = idx = oracle.build_index(lc_panel()[0].prgs, w, k)
        self.keys = set(int(x) for x in idx["keys"])
        self.doubles = set()
        for i, key in enumerate(idx["keys"]):
            lo, hi = int(idx["rec_off"][i]), int(idx["rec_off"][i + 1])
            if hi - lo >= 2:
                groups = list(zip(idx["rec_prg"][lo:hi].tolist(), idx["rec_strand"][lo:hi].tolist()))
                if len(set(groups)) < len(groups):
                    self.doubles.add(int(key))

    def __call__(self, read):
        return self.oracle.read_clusters(read, self.idx, self.w, self.k, self.md, self.frac, MCS)


def keyed(km, pos, keys):
    return {(p,) + km[p] for p in pos if km[p][0] in keys}


def _agrees(text, q, kmer_text):
    """the k-mer position q of `text` is cut -- it lies across an end or holds a letter that is not ACGT -- and every base the read does hold
    there is kmer_text's"""
    k, cut, seen = len(kmer_text), False, 0
    for j in range(k):
        c = text[q + j] if 0 <= q + j < len(text) else None
        if c is None or c not in "ACGT":
            cut = True
        elif c != kmer_text[j]:
            return False
        else:
            seen += 1
    return cut and seen > 0


def classify(read, w, k, tr):
    """{class: positions} of the classes the plain rule and the index find in `read` (positions: the keyed minimizers the class is about),
    and the keyed minimizers under the rule and under its three mutants"""
    text = read.decode().upper()
    km = R.kmers(text, k)
    nk = len(km)
    rule = R.pick(km, w)
    kd = {p for p in rule if km[p][0] in tr.keys}
    found = {}

    def add(name, pos):
        found.setdefault(name, set()).update(pos)

    hs = [x and x[0] for x in km]
    for s in range(nk - w + 1):
        win = hs[s:s + w]
        if None in win:
            continue
        m = min(win)
        if win.count(m) >= 2 and m in tr.keys:
            tied = [s + j for j in range(w) if win[j] == m]
            strands = [km[p][1] for p in tied]
            if strands.count(0) >= 2 or strands.count(1) >= 2:
                add("tandem", tied)
            if 0 in strands and 1 in strands:
                add("strand", tied)
    for p in kd:
        kt = text[p:p + k]
        for d in range(1, w):
            for near, far in ((p - d, p + d), (p + d, p - d)):
                if near in kd and text[near:near + k] == kt and -k < far < len(text) and _agrees(text, far, kt):
                    add("cut", (p, near))
        if km[p][0] in tr.doubles:
            add("double", (p,))
        if k % 2 == 0 and kt.encode() == rc(kt.encode()):
            add("selfcomp", (p,))
    valid = np.array([x is not None for x in km], bool)
    h = np.array([x or 0 for x in hs], np.uint64)
    for d in range(1, min(w, nk)):
        same = np.concatenate([[False], valid[:-d] & valid[d:] & (h[:-d] == h[d:]), [False]])
        edge = np.flatnonzero(same[1:] != same[:-1])
        for a, e in zip(edge[::2].tolist(), edge[1::2].tolist()):
            b = e - 1 + d  # the run is the k-mers a .. b
            n = b - a + 1
            name = "run_short" if n == w - 1 else "run_window" if n == w else "run_long" if n >= 2 * w - 1 else None
            if name is None:
                continue
            inside = [q for q in kd if a <= q <= b]
            tiedpair = [q for q in inside if any(q != r and hs[q] == hs[r] and abs(q - r) < w for r in inside)]
            if tiedpair:
                add(name, tiedpair)
    sets = dict(rule=keyed(km, rule, tr.keys), leftmost=keyed(km, R.pick(km, w, "leftmost"), tr.keys),
                rightmost=keyed(km, R.pick(km, w, "rightmost"), tr.keys))
    kms = R.kmers(text, k, strict_strand=True)
    sets["strict"] = keyed(kms, rule, tr.keys)
    return found, sets


def census(oracle, w, k):
    """{class: [indices into reads(w, k)]} of the accepted reads, plus per tie class how many of them each one-sided mutant changes:
    (classes, leftmost_differs, rightmost_differs, reads classified).  The reads are classified in order until every class holds FLOOR reads
    and each one-sided mutant changes FLOOR reads of every tie class."""
    key = ("census", w, k)
    if key in _CACHE:
        return _CACHE[key]
    tr = Tracer(oracle, w, k)
    classes = {c: [] for c in applicable(w, k)}
    left = {c: 0 for c in TIE_CLASSES}
    right = {c: 0 for c in TIE_CLASSES}
    for i, read in enumerate(reads(w, k)):
        if all(len(v) >= FLOOR for v in classes.values()) and all(min(left[c], right[c]) >= FLOOR for c in classes if c in TIE_CLASSES):
            break  # (the reads are in random order: the rest is more of the same, and the device maps it all the same)
        found, sets = classify(read, w, k, tr)
        if not found:
            continue
        t = tr(read)
        kept = set()
        for c in t["clusters"]:
            if c["alive"]:
                kept.update(t["hits"]["pos"][c["first"]:c["first"] + c["n"]].tolist())
        dl, dr, ds = sets["leftmost"] != sets["rule"], sets["rightmost"] != sets["rule"], sets["strict"] != sets["rule"]
        for name, pos in found.items():
            if name not in classes or not (pos & kept):
                continue
            if name in TIE_CLASSES:
                if not (dl or dr):
                    continue
                left[name] += dl
                right[name] += dr
            elif name == "selfcomp" and not ds:
                continue
            classes[name].append(i)
    _CACHE[key] = (classes, left, right, i + 1)
    return _CACHE[key]


def census_line(oracle, w, k):
    classes, left, right, seen = census(oracle, w, k)
    return f"(w={w}, k={k}) first {seen} of {len(reads(w, k))} reads: " + ", ".join(
        f"{c} {len(v)}" + (f" (left {left[c]}, right {right[c]})" if c in TIE_CLASSES else "") for c, v in classes.items())
