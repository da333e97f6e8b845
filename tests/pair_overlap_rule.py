"""The mate-overlap rule in plain Python / numpy (include/drprg_hip.h "mate overlap"), written from the rule's text:
what tests hold drprg_hip_pair_overlap_device and drprg_hip_pair_overlap against.  Nothing here looks at the kernel.

A mate is a bytes object as the file holds it.  Letters are compared without case; every byte that is not one of ACGTacgt is the unknown
base.  `unknown` arguments (sets of positions) add bases that a stage in front made unknown."""
import numpy as np

PO_MAX_LEN = 1024
NONE = -2 ** 31          # no shift qualifies
NOT_JUDGED = -2 ** 31 + 1  # a mate is not present, or one is longer than PO_MAX_LEN

_CODE = np.full(256, 4, np.uint8)  # 4: unknown
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i
_COMP = np.array([3, 2, 1, 0, 4], np.uint8)

COUNT_NAMES = ("pairs", "pairs_judged", "orphans", "pairs_too_long", "pairs_overlapping", "pairs_read_through", "bases_cut", "bases_clipped",
               "reads_emptied", "reads", "bases_before", "bases_kept")


def codes(read, unknown=()):
    c = _CODE[np.frombuffer(bytes(read), np.uint8)].copy()
    for p in unknown:
        c[p] = 4
    return c


def error_milli(text):
    """--pair-error as thousandths: a decimal in [0, 0.25] with at most three places, else ValueError"""
    from decimal import Decimal, InvalidOperation
    try:
        v = Decimal(str(text))
    except InvalidOperation:
        raise ValueError(text)
    m = v * 1000
    if not v.is_finite() or m != m.to_integral_value() or not 0 <= m <= 250:
        raise ValueError(text)
    return int(m)


def shift_counts(a, b):
    """shift_counts_plain's answer from five correlations (numpy's integer arithmetic: exact): entry d + Lb - 1 of correlate(u, v, "full") is
    the sum over i of u[i] v[i - d], so the known columns are one correlation and the matching ones one per letter"""
    La, Lb = len(a), len(b)
    if La == 0 or Lb == 0:
        return []
    B = _COMP[b[::-1]]
    c = np.correlate((a != 4).astype(np.int64), (B != 4).astype(np.int64), "full")
    same = sum(np.correlate((a == l).astype(np.int64), (B == l).astype(np.int64), "full") for l in range(4))
    return [(d, int(c[d + Lb - 1]), int(c[d + Lb - 1] - same[d + Lb - 1])) for d in range(-(Lb - 1), La)]


def shift_counts_plain(a, b):
    """(d, c(d), x(d)) for every shift d in -(Lb-1) .. La-1, column by column as the rule states them; a and b are code arrays (codes())"""
    La, Lb = len(a), len(b)
    B = _COMP[b[::-1]]
    out = []
    for d in range(-(Lb - 1), La):
        lo, hi = max(0, d), min(La, Lb + d)
        x, y = a[lo:hi], B[lo - d:hi - d]
        known = (x != 4) & (y != 4)
        out.append((d, int(known.sum()), int((known & (x != y)).sum())))
    return out


def choose_counts(table, min_overlap=30, err_milli=50):
    """the chosen shift among shift_counts' (d, c, x), or None"""
    best = None
    for d, c, x in table:
        if c >= min_overlap and 1000 * x <= err_milli * c:
            k = (c, -x, d)
            if best is None or k > best:
                best = k
    return None if best is None else best[2]


def choose(a, b, min_overlap=30, err_milli=50):
    """the chosen shift of two present mates that are short enough, or None"""
    return choose_counts(shift_counts(a, b), min_overlap, err_milli)


def qualifying_batch(A, B, min_overlap=30, err_milli=50):
    """for code matrices A (n x La) and B (n x Lb) of n pairs of equal lengths: how many shifts qualify in each pair -- the same sums as
    shift_counts, one shift at a time over all pairs"""
    n, La = A.shape
    Lb = B.shape[1]
    RB = _COMP[B[:, ::-1]]
    q = np.zeros(n, np.int64)
    for d in range(-(Lb - 1), La):
        lo, hi = max(0, d), min(La, Lb + d)
        x, y = A[:, lo:hi], RB[:, lo - d:hi - d]
        known = (x != 4) & (y != 4)
        c = known.sum(axis=1)
        xs = (known & (x != y)).sum(axis=1)
        q += (c >= min_overlap) & (1000 * xs <= err_milli * c)
    return q


def judge(a, b, min_overlap=30, err_milli=50, clip=False, unknown_a=(), unknown_b=(), table=None):
    """one pair: (d, keep_a, keep_b); d is NOT_JUDGED when a mate has no base or is longer than PO_MAX_LEN, NONE when no shift qualifies.
    table: shift_counts of the pair, for a caller that judges it under several settings"""
    La, Lb = len(a), len(b)
    if La == 0 or Lb == 0 or La > PO_MAX_LEN or Lb > PO_MAX_LEN:
        return NOT_JUDGED, La, Lb
    if table is None:
        table = shift_counts(codes(a, unknown_a), codes(b, unknown_b))
    d = choose_counts(table, min_overlap, err_milli)
    if d is None:
        return NONE, La, Lb
    insert = Lb + d
    ka = min(La, insert)
    kb = max(0, insert - La) if clip else min(Lb, insert)
    return d, ka, kb


def run(side1, side2, min_overlap=30, err_milli=50, clip=False, extra_reads=0, tables=None):
    """Two sides by source number; an entry is the mate's bytes after the ingest-time stages, or None for a mate that was dropped.  Returns
    (shifts, keep1, keep2, counts): keep is None for a dropped mate; counts is the dict of the twelve counters.  extra_reads: resident reads
    that the sides do not list (none in the tests' use); tables: shift_counts per pair (None where a pair is not judged), or None."""
    assert len(side1) == len(side2)
    n = len(side1)
    shifts, keep1, keep2 = [], [], []
    cnt = dict.fromkeys(COUNT_NAMES, 0)
    cnt["pairs"] = n
    for s, (a, b) in enumerate(zip(side1, side2)):
        for m in (a, b):
            if m is not None:
                cnt["reads"] += 1
                cnt["bases_before"] += len(m)
        pa, pb = a is not None and len(a) > 0, b is not None and len(b) > 0
        if not (pa and pb):
            cnt["orphans"] += int(pa) + int(pb)
            shifts.append(NOT_JUDGED)
            keep1.append(None if a is None else len(a))
            keep2.append(None if b is None else len(b))
        elif len(a) > PO_MAX_LEN or len(b) > PO_MAX_LEN:
            cnt["pairs_too_long"] += 1
            shifts.append(NOT_JUDGED)
            keep1.append(len(a))
            keep2.append(len(b))
        else:
            cnt["pairs_judged"] += 1
            d, ka, kb = judge(a, b, min_overlap, err_milli, clip, table=tables[s] if tables else None)
            shifts.append(d)
            keep1.append(ka)
            keep2.append(kb)
            if d != NONE:
                La, Lb, insert = len(a), len(b), len(b) + d
                cnt["pairs_overlapping"] += 1
                rt_a, rt_b = min(La, insert), min(Lb, insert)
                if rt_a < La or rt_b < Lb:
                    cnt["pairs_read_through"] += 1
                cnt["bases_cut"] += (La - rt_a) + (Lb - rt_b)
                cnt["bases_clipped"] += rt_b - kb
                cnt["reads_emptied"] += int(ka == 0) + int(kb == 0)
        cnt["bases_kept"] += (keep1[-1] or 0) + (keep2[-1] or 0)
    cnt["reads"] += extra_reads
    return shifts, keep1, keep2, cnt


def cut_reads(side1, side2, keep1, keep2):
    """the file the run stands for: side 1's kept mates cut, then side 2's"""
    return [m[:k] for m, k in zip(side1, keep1) if m is not None] + [m[:k] for m, k in zip(side2, keep2) if m is not None]
