"""The mate-merging rule in plain Python / numpy (include/drprg_hip.h "mate merging"), written from the rule's text:
what tests hold drprg_hip_pair_merge_device and drprg_hip_pair_overlap under drprg_hip_set_pair_merge against.  Codes and the chosen shift
come from pair_overlap_rule; nothing here looks at the kernel.

A mate is a bytes object as the file holds it; a merged read is upper-case ACGT and N."""
import numpy as np

import pair_overlap_rule as po

COUNT_NAMES = ("pairs_merged", "columns_both", "columns_agreeing", "columns_disagreeing", "columns_filled", "columns_unknown", "bases_merged",
               "longest_merged")
KINDS = COUNT_NAMES[2:6]
_TEXT = np.frombuffer(b"ACGTN", np.uint8)


def merge(a, b, d):
    """the merged read of mates a and b (bytes) at the chosen shift d: (M as bytes, the four column counts by kind, the kind of every
    position of M: -1 where one mate alone covers it, else the index into KINDS)"""
    ca, cb = po.codes(a), po.codes(b)
    La, Lb = len(ca), len(cb)
    B = po._COMP[cb[::-1]]
    insert = Lb + d
    assert 1 <= insert <= La + Lb - 1
    p = np.arange(insert)
    in_a, in_b = p < La, p >= d
    assert (in_a | in_b).all()  # (the qualifying overlap)
    x = np.where(in_a, ca[np.minimum(p, La - 1)], 4)  # a's base at p; 4 where a does not cover p
    y = np.where(in_b, B[np.clip(p - d, 0, Lb - 1)], 4)
    both, kx, ky = in_a & in_b, x != 4, y != 4
    kind = np.full(insert, -1, np.int64)
    kind[both & kx & ky & (x == y)] = 0   # both known, the same letter: that letter
    kind[both & kx & ky & (x != y)] = 1   # both known and different: unknown
    kind[both & (kx != ky)] = 2           # exactly one known: the known one
    kind[both & ~kx & ~ky] = 3            # both unknown: unknown
    M = np.where(kx, x, y)                # one mate alone, or the known one of two, or an agreed letter (x == y)
    M[kind == 1] = 4
    return _TEXT[M].tobytes(), [int((kind == k).sum()) for k in range(4)], kind


def run(side1, side2, min_overlap=30, err_milli=50, tables=None):
    """Two sides by source number, as pair_overlap_rule.run takes them.  Returns (shifts, new1, new2, counts12, counts8): new1 / new2 hold
    what every mate becomes -- None for a dropped mate, M for a merged a, b"" for a merged b, the mate's own bytes otherwise"""
    shifts, keep1, keep2, cnt = po.run(side1, side2, min_overlap, err_milli, False, tables=tables)
    new1, new2 = [], []
    m = dict.fromkeys(COUNT_NAMES, 0)
    cnt = dict(cnt)
    for a, b, d, ka, kb in zip(side1, side2, shifts, keep1, keep2):
        if d in (po.NONE, po.NOT_JUDGED):
            new1.append(a)
            new2.append(b)
            continue
        M, kinds, _ = merge(a, b, d)
        La, Lb, insert = len(a), len(b), len(b) + d
        both = min(La, insert) + min(Lb, insert) - insert
        assert sum(kinds) == both and len(M) == insert
        new1.append(M)
        new2.append(b"")
        m["pairs_merged"] += 1
        m["columns_both"] += both
        for name, v in zip(KINDS, kinds):
            m[name] += v
        m["bases_merged"] += insert
        m["longest_merged"] = max(m["longest_merged"], insert)
        # the twelve counts: bases_cut stays; bases_clipped is the columns both covered; every merged b is emptied; bases_kept the new lengths
        cnt["bases_clipped"] += both
        cnt["reads_emptied"] += 1  # (the read-through cut never empties a read: min(La, I), min(Lb, I) >= 1)
        cnt["bases_kept"] += insert - (ka + kb)
    return shifts, new1, new2, cnt, m


def merged_file(new1, new2):
    """the file the run stands for: side 1 with every merged a replaced by M, then side 2 with every merged b empty"""
    return [r for r in new1 if r is not None] + [r for r in new2 if r is not None]
