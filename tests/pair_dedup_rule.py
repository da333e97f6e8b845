"""The duplicate-pair rule of include/drprg_hip.h ("duplicate pairs") in plain Python: what the tests of drprg_hip_dedup_pairs compare
with.  Nothing here is taken from the code under test; the content key of one read is the host statement of tests/dedup_rule.py."""
import dedup_rule as reads_rule

MASK64 = reads_rule.MASK64
G = reads_rule.G
COUNT_NAMES = ("units", "units_with_bases", "units_both_mates", "units_dropped", "reads_before", "bases_before", "reads_kept", "bases_kept")
_NORMAL = bytes(c if c in b"ACGT" else (c - 32 if c in b"acgt" else ord("N")) for c in range(256))


def _bytes(m):
    """a mate that is not in the resident sample (None) and a mate of no bases are the same thing: the empty read"""
    return b"" if m is None else bytes(m)


def unit_identity(a, b):
    """what two identical units share: the identities of "duplicate reads" of A and of B, in that order"""
    return reads_rule.identity(_bytes(a)), reads_rule.identity(_bytes(b))


def unit_identity_fast(a, b):
    """unit_identity for large fixtures: ACGT upper-cased and every other byte turned into N say what (L, x) says
    (tests/test_pair_dedup_rule.py holds the two against each other)"""
    return _bytes(a).translate(_NORMAL), _bytes(b).translate(_NORMAL)


def unit_key(a, b):
    """U = fin(ka + G) + fin(kb + 2 G); ka, kb the content keys, 0 for the empty read"""
    ka, kb = reads_rule.key(_bytes(a)), reads_rule.key(_bytes(b))
    return (reads_rule.fin(ka + G) + reads_rule.fin(kb + 2 * G)) & MASK64


def has_bases(a, b):
    return len(_bytes(a)) > 0 or len(_bytes(b)) > 0


def select(side1, side2, identity=unit_identity):
    """per source pair: keep (1, or 0 for a duplicate unit) and copies (the size of the class of a kept unit with bases, else 0)"""
    assert len(side1) == len(side2)
    first, keep, copies = {}, [], []
    for s, (a, b) in enumerate(zip(side1, side2)):
        if not has_bases(a, b):
            keep.append(1)
            copies.append(0)
            continue
        ident = identity(a, b)
        if ident in first:
            keep.append(0)
            copies.append(0)
            copies[first[ident]] += 1
        else:
            first[ident] = s
            keep.append(1)
            copies.append(1)
    return keep, copies


def levels(keep, copies):
    lv = [0] * 32
    for k, c in zip(keep, copies):
        if k and c:
            lv[min(c, 32) - 1] += 1
    return lv


def run(side1, side2, extra_reads=0, identity=unit_identity_fast):
    """Two sides by source number; an entry is the mate's bytes as it lies in the resident sample behind the overlap stage, or None for a
    mate that is not there.  Returns (keep, copies, counts, levels, flags1, flags2): flags are per mate, None for a mate that is not
    resident, 1 for a kept one (a mate of no bases always is).  extra_reads: resident reads that the sides do not list."""
    keep, copies = select(side1, side2, identity)
    cnt = dict.fromkeys(COUNT_NAMES, 0)
    cnt["units"] = len(side1)
    flags = ([], [])
    for a, b, k in zip(side1, side2, keep):
        la, lb = len(_bytes(a)), len(_bytes(b))
        cnt["units_with_bases"] += int(la > 0 or lb > 0)
        cnt["units_both_mates"] += int(la > 0 and lb > 0)
        cnt["units_dropped"] += 1 - k
        for m, L, out in ((a, la, flags[0]), (b, lb, flags[1])):
            if m is None:
                out.append(None)
                continue
            f = 1 if k or L == 0 else 0
            out.append(f)
            cnt["reads_before"] += 1
            cnt["bases_before"] += L
            cnt["reads_kept"] += f
            cnt["bases_kept"] += L * f
    cnt["reads_before"] += extra_reads
    cnt["reads_kept"] += extra_reads
    return keep, copies, cnt, levels(keep, copies), flags[0], flags[1]


def kept_reads(side1, side2, flags1, flags2):
    """the file the run stands for: side 1's kept mates in file order, then side 2's"""
    return [m for m, f in zip(side1, flags1) if f] + [m for m, f in zip(side2, flags2) if f]


def brute_keep(side1, side2):
    """selection by comparing every unit with every unit before it"""
    ids = [unit_identity(a, b) for a, b in zip(side1, side2)]
    keep = []
    for s, (a, b) in enumerate(zip(side1, side2)):
        keep.append(0 if has_bases(a, b) and any(ids[h] == ids[s] for h in range(s)) else 1)
    return keep
