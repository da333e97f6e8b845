"""Adapter trimming under the indel rule (include/drprg_hip.h "adapter trimming", THE INDEL RULE) in plain Python, written from the rule's
text and not from the kernel, and the fixtures of tests/test_adapter_edit_rule.py and tests/test_gpu_adapter_edit.py.

The rule.  Settings: 0 to 4 3' adapters and 0 to 4 5' adapters of 1 to 64 letters ACGTacgt, an error rate held as per-mille e, a minimum
overlap O shared by both sides, L(c) = floor(c * e / 1000).  ed is the Levenshtein distance with unit costs, case-insensitive; a base that is
not ACGT differs from every letter.  3' side, in the range r[0..n) the crops and the quality trim left: full(p) = min over p <= q <= n of
ed(A, r[p..q)), full(n) = m; a start p matches A iff (a) c = n - p < m, c >= O and at most L(c) of the j < c have r[p + j] != A[j], or (b)
full(p) <= L(m) and full(p + 1) >= full(p).  The read is cut at the smallest matching p over all 3' adapters.  5' side: behind the 3' cut,
the same on the reversed read with every 5' adapter reversed letter by letter; a cut at p' there moves the begin to x + (n' - p')."""
import numpy as np

from adapter_rule import NEXTERA, TRUSEQ, _upper, adapters_of, error_milli, min_overlap, mutate  # noqa: F401  (shared helpers and letters)

# adapter_edit_points_kernel's geometry: bases per lane, wave and workgroup, reads per workgroup table
STRETCH, WAVE, TILE, SLOTS = 64, 64 * 64, 256 * 64, 1024
INFO_KEYS = ("reads_seen", "bases_seen", "reads_cut", "bases_cut", "reads_emptied")

# a 5' adapter of 64 letters: Oxford Nanopore's ligation adapter (top strand, 28 letters) behind 36 letters of a barcode flank; a 5' adapter
# is met by its END, so the shorter ones are its suffixes
FRONT = "GGTGCTGAAGAAAGTTGTCGGTGTCTTTGTGTTAAC" + "AATGTACTTCGTTCAGTTACGTATTGCT"
assert len(FRONT) == 64


def warmup(m, e):
    """how far outside its stretch a lane begins: the rule's bounded window"""
    return m + m * e // 1000 + 2


def front_adapters_of(name):
    return [FRONT[-33:], NEXTERA[::-1]] if name == "33+19" else [FRONT[-int(name):]]


def _arr(A):
    return _upper(A.encode() if isinstance(A, str) else A)


def scores(r, a):
    """full[p] for p in 0..n over upper-cased arrays (0: not ACGT): a column D[i] over the LAST i letters of the adapter, walked from the
    range's end to its start with D[0] = 0 in every column"""
    n, m = r.size, a.size
    full = np.empty(n + 1, dtype=np.int64)
    full[n] = m
    idx = np.arange(m + 1, dtype=np.int64)
    col = idx.copy()
    P = a[::-1]
    t = np.zeros(m + 1, dtype=np.int64)
    for p in range(n - 1, -1, -1):
        b = r[p]
        np.minimum(col[:-1] + ((P != b) | (b == 0)), col[1:] + 1, out=t[1:])
        col = np.minimum.accumulate(t - idx) + idx  # (the step down the column: D[i] <= D[i - 1] + 1)
        full[p] = col[m]
    return full


def matches(r, adapters, e, O):
    """for every start p of r (upper-cased array) whether it is a match of one of the adapters"""
    n = r.size
    ok = np.zeros(n, dtype=bool)
    for A in adapters:
        a = _arr(A)
        m = a.size
        full = scores(r, a)
        ok |= (full[:-1] <= m * e // 1000) & (full[1:] >= full[:-1])
        for c in range(max(O, 1), min(m - 1, n) + 1):  # clause (a): c = n - p < m
            tail = r[n - c:]
            if int(((tail != a[:c]) | (tail == 0)).sum()) <= c * e // 1000:
                ok[n - c] = True
    return ok


def cut_point(read, adapters, e, O, x=0, y=None):
    """3' side: the smallest matching start counted from x, or None"""
    r = _upper(read)[x:len(read) if y is None else y]
    if r.size == 0 or not adapters:
        return None
    hit = np.flatnonzero(matches(r, adapters, e, O))
    return int(hit[0]) if hit.size else None


def front_cut_point(read, adapters, e, O, x=0, y=None):
    """5' side: the largest matching end counted from x, or None -- the 3' rule on the reversed range with the reversed adapters"""
    r = bytes(read)[x:len(read) if y is None else y]
    p = cut_point(r[::-1], [A[::-1] for A in adapters], e, O)
    return None if p is None else len(r) - p


def cut_range(read, ad3, ad5, e, O, x=0, y=None):
    y = len(read) if y is None else y
    p = cut_point(read, ad3, e, O, x, y) if y > x else None
    if p is not None:
        y = x + p
    q = front_cut_point(read, ad5, e, O, x, y) if y > x else None
    if q is not None:
        x = x + q
    return x, y


def cut_ranges(reads, ranges, ad3, ad5, e, O, known=None):
    """[(begin, end)] behind both cuts, and the five counts of either side (drprg_hip_adapter_trim_info, drprg_hip_front_adapter_info);
    a side without adapters counts nothing.  known: ranges already worked out by cut_range, to spare the work"""
    out = []
    i3 = dict(reads_seen=len(reads) if ad3 else 0, bases_seen=0, reads_cut=0, bases_cut=0, reads_emptied=0)
    i5 = dict(reads_seen=len(reads) if ad5 else 0, bases_seen=0, reads_cut=0, bases_cut=0, reads_emptied=0)
    for k, (r, (x, y)) in enumerate(zip(reads, ranges)):
        nx, ny = known[k] if known is not None else cut_range(r, ad3, ad5, e, O, x, y)
        if ad3:
            i3["bases_seen"] += y - x
            if ny != y:
                i3["reads_cut"] += 1
                i3["bases_cut"] += y - ny
                i3["reads_emptied"] += ny == x
        if ad5:
            i5["bases_seen"] += ny - x
            if nx != x:
                i5["reads_cut"] += 1
                i5["bases_cut"] += nx - x
                i5["reads_emptied"] += nx == ny
        out.append((nx, ny))
    return out, i3, i5


def scores_many(rs, a):
    """scores() for many ranges at once (upper-cased arrays), the same column walked for all of them in step from their ENDS: a list of the
    full arrays.  For whole samples, where one range at a time is too slow; held against scores() in tests/test_adapter_edit_rule.py"""
    R, m = len(rs), a.size
    lens = np.array([r.size for r in rs], dtype=np.int64)
    nmax = int(lens.max()) if R else 0
    B = np.zeros((R, nmax), dtype=np.uint8)  # B[i, k] = base n_i - 1 - k of range i
    for i, r in enumerate(rs):
        B[i, :r.size] = r[::-1]
    idx = np.arange(m + 1, dtype=np.int32)
    col = np.tile(idx, (R, 1))
    t = np.zeros((R, m + 1), dtype=np.int32)
    out = np.full((R, nmax + 1), m, dtype=np.int32)
    P = a[::-1][None, :]
    for k in range(nmax):
        b = B[:, k][:, None]
        np.minimum(col[:, :-1] + ((P != b) | (b == 0)), col[:, 1:] + 1, out=t[:, 1:])
        col = np.minimum.accumulate(t - idx, axis=1) + idx
        out[:, k + 1] = col[:, m]
    return [out[i, :int(lens[i]) + 1][::-1] for i in range(R)]


def _cut_points_many(rs, adapters, e, O):
    """cut_point for many ranges (upper-cased arrays): a list of the smallest matching start, or None"""
    best = [None] * len(rs)
    order = sorted(range(len(rs)), key=lambda i: rs[i].size)
    for A in adapters:
        a = _arr(A)
        m = a.size
        for g in range(0, len(order), 256):  # (ranges of like length together: the walk is as long as the longest)
            group = order[g:g + 256]
            for i, full in zip(group, scores_many([rs[i] for i in group], a)):
                r, n = rs[i], rs[i].size
                ok = (full[:-1] <= m * e // 1000) & (full[1:] >= full[:-1])
                for c in range(max(O, 1), min(m - 1, n) + 1):
                    tail = r[n - c:]
                    if int(((tail != a[:c]) | (tail == 0)).sum()) <= c * e // 1000:
                        ok[n - c] = True
                hit = np.flatnonzero(ok)
                if hit.size and (best[i] is None or hit[0] < best[i]):
                    best[i] = int(hit[0])
    return best


def cut_ranges_many(reads, ranges, ad3, ad5, e, O):
    """cut_ranges for a whole sample: the same rule, the columns of many reads walked in step"""
    up = [_upper(r) for r in reads]
    p3 = _cut_points_many([u[x:y] for u, (x, y) in zip(up, ranges)], ad3, e, O) if ad3 else [None] * len(reads)
    mid = [(x, y if p is None else x + p) for (x, y), p in zip(ranges, p3)]
    p5 = _cut_points_many([u[x:y][::-1] for u, (x, y) in zip(up, mid)], [A[::-1] for A in ad5], e, O) if ad5 else [None] * len(reads)
    known = [(x if p is None else x + (y - x - p), y) for (x, y), p in zip(mid, p5)]
    return cut_ranges(reads, ranges, ad3, ad5, e, O, known=known)


def plant(bases, offs, A, F, e, seed):
    """A sample's reads with adapters put in, by turns: both (the 5' adapter in front, the read's end replaced by the 3' adapter and up to
    20 random bases), the 5' adapter alone (every fourth of them cut short at its start), the 3' adapter alone (every other of them cut
    short by the read's end), nothing -- the turn shifted by one every twelve reads, and four turns against three strands, so that the records the BAM fixtures store on the
    reverse strand are of every kind.  A whole adapter carries up to L(m) edits of any kind.  Returns (reads as bytes, kinds)."""
    rng = np.random.default_rng(seed)
    reads, kinds = [], []

    def worn(X):
        k = int(rng.integers(0, len(X) * e // 1000 + 1))
        parts = rng.multinomial(k, [1 / 3] * 3)
        return edit(rng, X, int(parts[0]), int(parts[1]), int(parts[2]))

    for i in range(len(offs) - 1):
        r = bytes(bases[int(offs[i]):int(offs[i + 1])])
        kind = ("both", "front", "end", "none")[(i + i // 12) % 4] if len(r) >= 40 else "none"
        if kind in ("both", "end"):
            if kind == "end" and i % 2:
                r = r + A[:int(rng.integers(8, len(A)))].encode()
            else:
                r = r[:int(rng.integers(len(r) // 2, len(r)))] + worn(A) + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(0, 21))))
        if kind in ("both", "front"):
            r = (F[-int(rng.integers(8, len(F))):].encode() if kind == "front" and i % 4 == 1 else worn(F)) + r
        reads.append(r)
        kinds.append(kind)
    return reads, kinds


def edit(rng, seq, subs=0, ins=0, dels=0, keep=2):
    """seq with that many substitutions, inserted letters and deleted letters at distinct places, none among its first and last `keep`
    letters (so that the occurrence still begins and ends where it was put)"""
    s = [bytes([c]) for c in (seq.encode() if isinstance(seq, str) else bytes(seq))]
    places = [int(i) for i in rng.permutation(np.arange(keep, len(s) - keep))[:subs + ins + dels]]
    assert len(places) == subs + ins + dels, (len(s), subs, ins, dels)
    for k, i in enumerate(places):
        if k < subs:
            s[i] = bytes([ord(rng.choice([c for c in "ACGT" if c != s[i].decode().upper()]))])
        elif k < subs + ins:
            s[i] = s[i] + bytes([ord(rng.choice(list("ACGT")))])
        else:
            s[i] = b""
    return b"".join(s)


def kernel_batch(name, E):
    """The ragged batch of the kernel test for one adapter set and error rate, a few tiles: dict(reads, ranges, want, classes, ad3, ad5,
    e, O, partial_lengths).  classes: name -> (read indices, kind); kind says what the rule must say of the class -- "cut3": every read loses bases at its end
    and none at its start, "cut5": the other way round, "both", "none", "mixed", "any".  Every read with an intended range is redrawn until
    the rule gives exactly that range, so that filler cannot match by accident; want is the rule's range of every read.

    Clean text.  An occurrence of A inside text over a set S of letters costs at least one edit for every letter of A outside S.  Up to
    E = 0.2 every adapter here has more G and T letters than L(m), so random text of A and C is provably clean of it: the long reads are made
    of that, and the reads around planted occurrences of random ACGT, redrawn until they say what they are meant to.  At E = 0.5 random
    letters lie within m / 2 edits of an adapter nearly everywhere, and the only provably clean text is a run of one letter that makes up
    less than half of every adapter, of each of its prefixes (3') and of each of its suffixes (5') from O letters on: C for the single
    adapters here, G for the pair (asserted below).  There all filler is a run of that letter; the occurrences keep their random edits, so the redraw still has something to
    draw.  One thing no filler mends at E = 0.5: an adapter of one side is text to the other side, and lies within m / 2 edits of it
    somewhere -- the 3' rule, which runs first, cuts inside the ligation adapter itself.  So at E = 0.5 a class that belongs to one side
    is held to its intended range WITH THAT SIDE'S ADAPTERS ALONE SET (want3, want5: the rule's ranges of every read under either
    setting, which the GPU test runs as launches of their own beside the launch with both), and only the few classes that need both
    sides in one read are left to whatever the rule says.  A class that still cannot be drawn at E = 0.5 is named in `relaxed` with
    the rule's verdict left open; the census test pins that list."""
    e = error_milli(E)
    ad3, ad5 = adapters_of(name), front_adapters_of(name)
    A, F = ad3[0], ad5[0]
    m = len(A)
    O = min_overlap(ad3 + ad5)
    noisy = e > 200  # (random ACGT is no filler any more)
    rng = np.random.default_rng(7000 * len(name) + m + e)
    reads, ranges, want, classes, partial_lengths = [], [], [], {}, {}
    want3, want5, sides, relaxed = [], [], {}, []
    RUN = "G" if len(ad3) > 1 else "C"  # (the second 3' adapter begins with C and is mostly C and T: next to a run of C its first letters pass as an overlap)
    for X in ad3 + ad5:
        if not noisy:
            assert sum(c in "GT" for c in X) > len(X) * e // 1000, X
    for X, part in [(X, lambda X, c: X[:c]) for X in ad3] + [(X, lambda X, c: X[-c:]) for X in ad5]:
        for c in range(O, len(X) + 1):  # a run of C against the adapter's first (3') or last (5') c letters, whole adapter included
            assert not noisy or c - part(X, c).count(RUN) > c * e // 1000, (X, c)

    def lim(c):
        return c * e // 1000

    def filler(n):
        return RUN.encode() * n if noisy else bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))

    def clean(n):
        return RUN.encode() * n if noisy else bytes(rng.choice(np.frombuffer(b"AC", dtype=np.uint8), size=n))

    def pos():
        return sum(len(r) for r in reads)

    def add(cls, kind, make, to="?"):
        """make() -> bytes or (bytes, (begin, end)); to: the intended range behind both cuts, a test (range behind the cuts, range before) ->
        bool, or "?" for whatever the rule says"""
        side = sides.setdefault(cls, 0 if kind in ("both", "mixed", "any") or cls == "edge lengths" else 5 if "front" in cls or cls.startswith("5'") else 3)
        if noisy and side == 0 and kind == "both":
            kind, to = "any", "?"  # (both sides in one read: each is text to the other)
        if cls in relaxed:
            kind, to = "any", "?"
        prev = None
        for _ in range(300 if not noisy else 60):
            made = make()
            if made == prev:  # (nothing random in it: no draw will change the verdict)
                continue
            prev = made
            r, rg = made if isinstance(made, tuple) else (made, (0, len(made)))
            got = cut_range(r, ad3 if not (noisy and side == 5) else [], ad5 if not (noisy and side == 3) else [], e, O, rg[0], rg[1])
            if to == "?" or (to(got, rg) if callable(to) else got == to):
                break
        else:
            if not noisy:
                raise AssertionError((cls, got))
            relaxed.append(cls)
            classes[cls] = (classes.get(cls, ([], kind))[0], "any")
        reads.append(r)
        ranges.append(rg)
        want.append(cut_range(r, ad3, ad5, e, O, rg[0], rg[1]) if noisy and side else got)
        if noisy:
            want3.append(got if side == 3 else cut_range(r, ad3, [], e, O, rg[0], rg[1]))
            want5.append(got if side == 5 else cut_range(r, [], ad5, e, O, rg[0], rg[1]))
        classes.setdefault(cls, ([], kind))[0].append(len(reads) - 1)

    untouched = lambda got, rg: got == rg
    only3 = lambda got, rg: got[0] == rg[0] and got[1] < rg[1]
    only5 = lambda got, rg: got[0] > rg[0] and got[1] == rg[1]

    def pad_to(at):
        """filler reads up to at most absolute position `at`, at least 40 bases short of it"""
        while at - pos() > 700:
            add("filler", "any", lambda: filler(int(rng.integers(100, 600))))
        assert at - pos() >= 40, (at, pos())

    def three(cls, occ, at, by_end=False, lead_min=40):
        """a read with the 3' occurrence occ() starting (or, by_end, ending) at absolute position `at`, random bases behind it"""
        pad_to(at - 200)
        start = pos()

        def make():
            o = occ()
            lead = at - start - (len(o) if by_end else 0)
            assert lead >= lead_min
            make.lead = lead
            return filler(lead) + o + filler(int(rng.integers(5, 20)))
        add(cls, "cut3", make, lambda got, rg: got == (0, make.lead))

    def five(cls, occ, at, by_end=False):
        """a read with the 5' occurrence occ() ending (or, by_end False, starting) at absolute position `at`, 60 random bases behind it"""
        pad_to(at - 200)
        start = pos()

        def make():
            o = occ()
            lead = at - start - (len(o) if by_end else 0)
            assert lead >= 0
            make.cut = lead + len(o)
            return clean(lead) + o + filler(60)
        add(cls, "cut5", make, lambda got, rg: got == (make.cut, rg[1]))

    # ---- the classes of the plain batch ------------------------------------------------------------------------------------------------
    # more reads of 3 to 8 bases inside the first tile than a workgroup's table holds, some ending in a prefix of the 3' adapter, some
    # beginning with a suffix of the 5' adapter
    for i in range(SLOTS + 176):
        n = int(rng.integers(3, 9))
        add("short run", "mixed", (lambda n=n: filler(n - O) + A[:O].encode()) if i % 4 == 0 else (lambda n=n: F[-O:].encode() + filler(n - O)) if i % 4 == 1 else (lambda n=n: filler(n)))
    assert len(reads) > SLOTS + 100 and pos() < TILE - 1000
    for n in (0, 1, O - 1, O, m - 1, m, m + 1):
        add("edge lengths", "none", lambda n=n: clean(n), (0, n))
    add("the adapter itself", "cut3", lambda: A.encode(), (0, 0))
    add("the front adapter itself", "cut5", lambda: F.encode(), (len(F), len(F)))
    for k in range(1, m):  # a partial overlap of every length at either end
        add("partial below O" if k < O else "partial from O", "none" if k < O else "cut3", lambda k=k: filler(30) + A[:k].encode(), (0, 30 + k) if k < O else (0, 30))
    for k in range(1, len(F)):
        add("front partial below O" if k < O else "front partial from O", "none" if k < O else "cut5", lambda k=k: F[-k:].encode() + filler(30), (0, 30 + k) if k < O else (k, 30 + k))
    # a partial overlap with exactly the allowed number of mismatches, and one more, on both sides of a step of the floor (clause (a)'s own
    # threshold); for an adapter over 32 letters also overlaps of more than 32 letters whose mismatches lie in the letters past the 32nd
    # met, as far as there is room: the second word of the comparison
    def worn_part(X, c, k, side):
        """the first (3') or last (5') c letters of X with k substitutions, as many of them as fit in the letters past the 32nd met"""
        part = X[:c] if side == 3 else X[-c:]
        far = set(range(32, c)) if side == 3 else set(range(0, c - 32))  # (a 5' overlap is met from its end)
        k_far = min(k, len(far)) if c > 32 else 0
        out, _ = mutate(rng, part, k_far, forbid=set(range(c)) - far) if k_far else (part.encode(), [])
        out, _ = mutate(rng, out, k - k_far, forbid=far)
        return out
    for side, X in ((3, A), (5, F)):
        mx = len(X)
        steps = [c for c in range(max(O, 2), mx) if lim(c) != lim(c - 1)]
        partial = sorted({c for s in steps[:2] for c in (s - 1, s) if c >= O} | {c for s in [t for t in steps if t > 34][:1] for c in (s - 1, s)}
                         | ({48} if mx == 64 else set()) | (set() if steps else {min(O + 2, mx - 1), mx - 1}))
        partial_lengths[side] = partial
        for c in partial:
            for extra in (0, 1):
                if lim(c) + extra > c:
                    continue
                cls = f"{side}' partial {'one over' if extra else 'at'} the limit" + (" past letter 32" if c > 32 else "")
                if side == 3:
                    add(cls, "none" if extra else "cut3", lambda c=c, extra=extra: filler(40) + worn_part(A, c, lim(c) + extra, 3), untouched if extra else (0, 40))
                else:
                    add(cls, "none" if extra else "cut5", lambda c=c, extra=extra: worn_part(F, c, lim(c) + extra, 5) + filler(40), untouched if extra else (c, 40 + c))
    # a worse but acceptable match outside a perfect one: the leftmost wins at the 3' end, the rightmost at the 5' end
    add("worse to the left", "cut3", lambda: filler(30) + mutate(rng, A, lim(m))[0] + filler(20) + A.encode(), (0, 30))
    add("worse to the right", "cut5", lambda: F.encode() + clean(20) + mutate(rng, F, lim(len(F)))[0] + filler(50), (2 * len(F) + 20, 2 * len(F) + 70))
    # neighbours: A[0:2] | A[2:] cuts nothing at the boundary, A[0:5] | A[5:] takes five bases off the first read; and the mirror
    add("split 2", "none", lambda: filler(30) + A[:2].encode(), (0, 32))
    add("split rest", "any", lambda: A[2:].encode() + filler(20))
    add("split 5", "cut3", lambda: filler(30) + A[:5].encode(), (0, 30))
    add("split rest", "any", lambda: A[5:].encode() + filler(20))
    add("split rest", "any", lambda: filler(20) + F[:-2].encode())
    add("front split 2", "none", lambda: F[-2:].encode() + filler(30), (0, 32))
    add("split rest", "any", lambda: filler(20) + F[:-5].encode())
    add("front split 5", "cut5", lambda: F[-5:].encode() + filler(30), (5, 35))
    # ---- exactly L(m) and L(m) + 1 edits of each kind, and mixed --------------------------------------------------------------------------
    L = lim(m)
    kinds = dict(subs=(1, 0, 0), ins=(0, 1, 0), dels=(0, 0, 1))
    for side, X in ((3, A), (5, F)):
        LX = lim(len(X))
        for kname, (s, i, d) in kinds.items():
            for extra in (0, 1):
                k = LX + extra
                if 2 * 2 + k > len(X):
                    continue
                occ = lambda X=X, k=k, s=s, i=i, d=d: edit(rng, X, s * k, i * k, d * k)
                cls = f"{side}' {kname} {'at' if not extra else 'one over'} the limit"
                if side == 3:
                    add(cls, "none" if extra else "cut3", lambda occ=occ: filler(40) + occ() + filler(10), untouched if extra else (0, 40))
                else:
                    add(cls, "none" if extra else "cut5", lambda occ=occ: clean(6) + occ() + filler(50), untouched if extra else only5)
        if LX >= 2:
            a, b = LX // 2, LX - LX // 2
            add(f"{side}' mixed at the limit", "cut3" if side == 3 else "cut5",
                (lambda X=X, a=a, b=b: filler(40) + edit(rng, X, a, b, 0) + filler(10)) if side == 3 else (lambda X=X, a=a, b=b: clean(6) + edit(rng, X, 0, a, b) + filler(50)), only3 if side == 3 else only5)
            add(f"{side}' mixed one over the limit", "any",
                (lambda X=X, a=a, b=b: filler(40) + edit(rng, X, a + 1, 0, b) + filler(10)) if side == 3 else (lambda X=X, a=a, b=b: clean(6) + edit(rng, X, a, b + 1, 0) + filler(50)), "?")
    if m == 64 and L >= 1:  # an indel on either side of letter 32 of a 64-letter adapter: the carry between the words
        for at in (30, 31, 32, 33):
            add("indel beside letter 32", "cut3", lambda at=at: filler(40) + A[:at].encode() + b"T" + A[at:].encode() + filler(10), only3)
            add("indel beside letter 32", "cut3", lambda at=at: filler(40) + A[:at].encode() + A[at + 1:].encode() + filler(10), only3)
            add("front indel beside letter 32", "cut5", lambda at=at: clean(5) + F[:at].encode() + b"A" + F[at:].encode() + filler(50), only5)
            add("front indel beside letter 32", "cut5", lambda at=at: clean(5) + F[:at].encode() + F[at + 1:].encode() + filler(50), only5)

    # ---- N, case, two adapters, both ends ------------------------------------------------------------------------------------------------
    # a base that is not ACGT inside an occurrence: in place of a mismatch it changes nothing, beside the allowed mismatches it tips it over
    def with_n(X, extra):
        s, places = mutate(rng, X, lim(len(X)), forbid=(0, 1, len(X) - 2, len(X) - 1))
        s = bytearray(s)
        at = int(rng.choice([i for i in range(2, len(X) - 2) if i not in places])) if extra or not places else places[0]
        s[at] = ord("N")
        return bytes(s)
    if L:
        add("N for a mismatch", "cut3", lambda: filler(40) + with_n(A, False) + filler(10), (0, 40))
    add("N over the limit", "none", lambda: filler(40) + with_n(A, True) + filler(10), untouched)
    if lim(len(F)):
        add("front N for a mismatch", "cut5", lambda: clean(6) + with_n(F, False) + filler(50), (6 + len(F), 56 + len(F)))
    add("front N over the limit", "none", lambda: clean(6) + with_n(F, True) + filler(50), untouched)
    add("two occurrences", "cut3", lambda: filler(30) + A.encode() + filler(20) + A.encode() + filler(5), (0, 30))
    add("two front occurrences", "cut5", lambda: F.encode() + clean(20) + F.encode() + filler(50), (2 * len(F) + 20, 2 * len(F) + 70))
    add("lower case", "both", lambda: (F.encode() + filler(50) + A.encode() + filler(7)).lower(), (len(F), len(F) + 50))
    add("both adapters in one read", "both", lambda: clean(3) + edit(rng, F, lim(len(F)), 0, 0) + filler(80) + edit(rng, A, L, 0, 0) + filler(9), lambda got, rg: got[0] > rg[0] and got[1] < rg[1])
    add("the two cuts take the read between them", "both", lambda: F.encode() + A.encode() + filler(12), (len(F), len(F)))
    if len(ad3) > 1:
        add("second adapter", "cut3", lambda: filler(30) + ad3[1].encode() + filler(10), (0, 30))
        add("second adapter", "cut3", lambda: filler(30) + ad3[1][:7].encode(), (0, 30))
        add("second front adapter", "cut5", lambda: ad5[1].encode() + filler(40), (len(ad5[1]), len(ad5[1]) + 40))
        add("second front adapter", "cut5", lambda: ad5[1][-7:].encode() + filler(40), (7, 47))
    # a run of genome bases left of an occurrence (right of a 5' one) that clause (b) must keep: the occurrence is whole, so every start up
    # to L(m) bases to its left lies within the limit too, and only the second half of clause (b) tells them apart
    add("genome bases clause (b) keeps", "cut3", lambda: filler(50) + A.encode() + filler(10), (0, 50))
    add("genome bases clause (b) keeps, front", "cut5", lambda: F.encode() + filler(50), (len(F), len(F) + 50))
    # ranges narrower than the read, on both sides
    half = max(O, m // 2)
    add("straddles end", "cut3", lambda: (clean(30) + A.encode() + filler(20), (0, 30 + half)), (0, 30))
    add("straddles end below O", "none", lambda: (clean(30) + A.encode() + filler(20), (3, 30 + O - 1)), (3, 30 + O - 1))
    add("starts before begin", "any", lambda: (clean(30) + A.encode() + filler(20), (32, 50 + m)))
    add("inside the range", "cut3", lambda: (clean(30) + A.encode() + filler(20), (10, 45 + m)), (10, 30))
    add("front straddles begin", "cut5", lambda: (filler(9) + F.encode() + filler(50), (9 + len(F) - half, 59 + len(F))), (9 + len(F), 59 + len(F)))
    add("front inside the range", "cut5", lambda: (filler(9) + F.encode() + filler(50), (4, 49 + len(F))), (9 + len(F), 49 + len(F)))
    add("front ends behind end", "any", lambda: (filler(9) + F.encode() + filler(50), (0, 9 + len(F) - 2)))
    # ---- geometry ----------------------------------------------------------------------------------------------------------------------------
    # an occurrence stretched by L(m) inserted letters that ends exactly at a stretch, a wave and a tile boundary, and one base over it; the
    # 5' one begins there, and one base before
    stretched = lambda: edit(rng, A, 0, L, 0)
    fstretched = lambda: edit(rng, F, 0, lim(len(F)), 0)
    def boundary(label, unit, side, over):
        b = (pos() + 400 + 2 * m) // unit * unit + unit
        if side == 3:
            three(f"ends {'one over' if over else 'at'} a {label} boundary", stretched, b + over, by_end=True)
        else:
            five(f"front begins {'one before' if over else 'at'} a {label} boundary", fstretched, b - over)
    for side in (3, 5):
        for over in (0, 1):
            boundary("stretch", STRETCH, side, over)
    # (a tile boundary, then the wave boundaries inside that tile, four times: the eight classes in four tiles)
    for k, (side, over) in enumerate(((3, 0), (5, 0), (3, 1), (5, 1))):
        boundary("tile", TILE, side, over)
        boundary("wave", WAVE, 5 if side == 3 else 3, 1 - over)
    # an occurrence whose warm-up would start in the previous read (3': in the next read): the neighbour ends (begins) with the adapter's
    # other part, which must not count
    add("warm-up in the neighbour", "cut3", lambda: filler(60) + A[:m // 2].encode(), (0, 60))
    add("the neighbour of a warm-up", "any", lambda: A[m // 2:].encode() + filler(60))
    add("the neighbour of a warm-up", "any", lambda: filler(60) + F[:len(F) // 2].encode())
    add("front warm-up in the neighbour", "cut5", lambda: F[len(F) // 2:].encode() + filler(60), (len(F) - len(F) // 2, len(F) - len(F) // 2 + 60))
    # ---- a read of more than 20 000 bases with the adapter at 18 000, whole waves under one read; the occurrence crosses a tile's
    # start by m - 1 bases (the tile's number is whatever the classes before it come to); a 5' adapter at its start; and a second such read without either ------------------------------------------------
    cross = (pos() + 18000 + 800) // TILE * TILE + TILE - 1  # where the long read's 3' occurrence begins: one base before a tile's start
    pad_to(cross - 18000)
    add("filler", "any", lambda: clean(cross - 18000 - pos()))
    assert pos() == cross - 18000 and (cross + 1) % TILE == 0
    add("long with both adapters", "both", lambda: F.encode() + clean(18000 - len(F)) + A.encode() + filler(2500), (len(F), 18000))
    add("long without adapter", "none", lambda: clean(20500), (0, 20500))
    return dict(reads=reads, ranges=ranges, want=want, classes=classes, ad3=ad3, ad5=ad5, e=e, O=O, partial_lengths=partial_lengths, noisy=noisy, want3=want3, want5=want5, sides=sides, relaxed=relaxed)


def census(batch):
    """per class (reads cut at the 3' end, at the 5' end, untouched), by the rule alone; raises if a class is empty or not what it is meant to be"""
    out = {}
    for name, (idx, kind) in batch["classes"].items():
        w = batch["want"] if not batch["noisy"] or not batch["sides"][name] else batch["want3"] if batch["sides"][name] == 3 else batch["want5"]
        c3 = sum(w[i][1] != batch["ranges"][i][1] for i in idx)
        c5 = sum(w[i][0] != batch["ranges"][i][0] for i in idx)
        un = sum(w[i] == batch["ranges"][i] for i in idx)
        out[name] = (c3, c5, un)
        ok = dict(cut3=c3 == len(idx) and c5 == 0, cut5=c5 == len(idx) and c3 == 0, both=c3 == c5 == len(idx), none=un == len(idx), mixed=0 < un < len(idx), any=True)[kind]
        assert idx and ok, (name, kind, out[name])
    return out
