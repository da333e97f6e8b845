"""Recipes for batches that follow each other on ONE context (tests/test_batch_sequences.py holds the census on the CPU,
tests/test_gpu_batch_sequences.py maps the schedule on the device).  Plain Python and numpy, no GPU.

A Mapper carries state from batch to batch: the two lanes deferred batches take in turn (scratch_zero, capacities, candidate buffers),
the epoch marks in cand_pos1, the tile sets (d_nbits / nbits_dirty, a_done, the scan's closing zero), the ASCII expansions behind
ascii_view, the staging sets, the counters counters_home_kernel clears "for the next batch", C_MAXLEN / L_MAXLEN (per-read sort or
radix sort), the mean read length (read_cluster_kernel's look-ahead), ft_share_ and the chunk schedule, the hit buffer.  Each is right
only if the NEXT batch -- smaller, longer-read, in the other input format, with or without N positions, through another entry point --
sees it cleared, regrown or derived again.  So: ten kinds of small batches, each in ASCII and packed (20 states), and one seeded
schedule in which every ordered pair of states is adjacent somewhere and every ordered pair is two apart somewhere (two apart = the same
lane when batches are deferred), every batch through one of the six entry points, with a few reset() points.  The oracle is additive:
what a context holds after batch i is the sum of the kinds mapped since the last reset."""
from collections import namedtuple

import numpy as np

_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
_CACHE = {}

# kind 5 of the issue is two kinds here: a batch without reads and a batch of five empty reads
KINDS = ("dense", "sparse", "repeat", "tiny", "none", "empties", "long", "medium", "ragged", "ragged_clean")
STATES = [(kind, packed) for kind in KINDS for packed in (False, True)]
ENTRIES = {False: ("map_host", "map_device", "map_device_async"), True: ("map_host_packed", "map_device_packed", "map_device_packed_async")}
DEFERRED = ("map_device_async", "map_device_packed_async")
MAX_STEPS = 1500
SEED = 20261018
# read_cluster_kernel's look-ahead by the batch's mean read length (read_cluster.hip launch_read_cluster): <= 300 -> 128, <= 600 -> 256, else 512
LOOK_AHEAD = ((300, 128), (600, 256), (1 << 62, 512))

Step = namedtuple("Step", "kind packed entry reset_before")


def look_ahead(mean_len):
    return next(a for top, a in LOOK_AHEAD if mean_len <= top)


# ---- the panel --------------------------------------------------------------------------------------------------------------------------
def panel():
    """The panel of test_gpu_parity.test_deferred_batches_equal_synchronous_ones (same seed, same draws): 70 copies of one locus, whose reads
    read_cluster_kernel leaves to the generic pipeline, plus `single` and `other`.  Returns (Panel, dict of the three locus trees)."""
    from drprg_amd import synth
    if "panel" not in _CACHE:
        rng = np.random.default_rng(21)
        rep = synth.make_locus(rng, 400, site_every=70)
        single = synth.make_locus(rng, 900, site_every=50)
        other = synth.make_locus(rng, 1200, site_every=40)
        p = synth.Panel([f"rep{i}" for i in range(70)] + ["single", "other"], [rep] * 70 + [single, other])
        _CACHE["panel"] = (p, dict(rep=rep, single=single, other=other))
    return _CACHE["panel"]


def _sources():
    """haplotypes of the three loci, an off-panel background, and a 'genome' in which the loci lie between stretches of background (the
    long, medium and ragged reads are cut from it: a long read crosses several loci, the repeated one among them)"""
    from drprg_amd import synth
    if "sources" not in _CACHE:
        _, loci = panel()
        rng = np.random.default_rng(SEED)
        hap = lambda name: synth.sample_haplotype(rng, loci[name]).encode()
        src = dict(rep=hap("rep"), single=hap("single"), other=hap("other"), background=synth.random_seq(rng, 30000).encode())
        parts = []
        for name in ("single", "rep", "other", "rep", "single", "other", "rep", "other"):
            parts.append(synth.random_seq(rng, int(rng.integers(300, 1500))).encode())
            h = hap(name)
            parts.append(h.translate(_RC)[::-1] if rng.random() < 0.5 else h)
        parts.append(synth.random_seq(rng, 800).encode())
        src["genome"] = b"".join(parts)
        _CACHE["sources"] = src
    return _CACHE["sources"]


def _batch(reads):
    offs = np.zeros(len(reads) + 1, np.uint64)
    if reads:
        offs[1:] = np.cumsum([len(r) for r in reads])
    bases = np.concatenate(reads) if reads else np.zeros(0, np.uint8)
    return np.ascontiguousarray(bases, np.uint8), offs


def _draw(rng, seqs, lengths, sub_rate=0.002):
    """one read per entry of `lengths`, from the sequences in turn (random place and strand, a few substitutions)"""
    reads = []
    for i, ln in enumerate(lengths):
        s = seqs[i % len(seqs)]
        ln = min(int(ln), len(s))
        at = int(rng.integers(0, len(s) - ln + 1))
        r = s[at:at + ln]
        if rng.random() < 0.5:
            r = r.translate(_RC)[::-1]
        a = np.frombuffer(r, np.uint8).copy()
        err = np.nonzero(rng.random(ln) < sub_rate)[0]
        a[err] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=err.size)]
        reads.append(a)
    return reads


def _ragged(rng, genome):
    """N runs and single Ns, lower case, reads shorter than k, empty reads, lengths on sketch_wave_kernel's tile edges (976, 1024)"""
    lengths = rng.choice([0, 0, 1, 14, 15, 16, 24, 25, 26, 40, 150, 151, 300, 976, 1024, 2000], size=1200)
    reads = _draw(rng, [genome], lengths)
    for i, r in enumerate(reads):
        n = len(r)
        if n and rng.random() < 0.3:
            r[rng.integers(0, n, size=max(1, n // 50))] = ord("N")
        if n and rng.random() < 0.15:  # a run of 1 .. 40 bases that are no bases (not every one an N)
            a0 = int(rng.integers(0, n))
            r[a0:a0 + int(rng.integers(1, 41))] = ord("N") if rng.random() < 0.8 else ord("R")
        if n and rng.random() < 0.2:
            reads[i] = np.frombuffer(r.tobytes().lower(), np.uint8).copy()
    return reads


_IS_BASE = np.zeros(256, bool)
_IS_BASE[list(b"ACGTacgt")] = True


def kind_batch(kind):
    """(bases u8, offsets u64) of one kind: seeded, the same on every call"""
    if ("kind", kind) in _CACHE:
        return _CACHE[("kind", kind)]
    src = _sources()
    rng = np.random.default_rng([SEED, KINDS.index(kind)])
    if kind == "dense":  # every read inside the panel: more candidates than the production ratios n_bases / 48, / 16, / 64 give room for
        out = _batch(_draw(rng, [src["single"], src["other"]], [150] * 2500))
    elif kind == "sparse":  # one read in ten inside the panel
        out = _batch(_draw(rng, [src["background"]] * 9 + [src["other"]], [150] * 3000))
    elif kind == "repeat":  # a third of the reads from the 70-copy locus: 70 clusters per read, left to the generic pipeline
        out = _batch(_draw(rng, [src["rep"], src["single"], src["background"]], [150] * 1500))
    elif kind == "tiny":
        out = _batch(_draw(rng, [src["other"]], [150] * 10))
    elif kind == "none":
        out = _batch([])
    elif kind == "empties":
        out = _batch([np.zeros(0, np.uint8)] * 5)
    elif kind == "long":  # 3 - 9 kb: look-ahead 512, the radix sort behind the leftovers, reads with more hits than a chunk stages
        out = _batch(_draw(rng, [src["genome"]], rng.integers(3000, 9001, size=110), sub_rate=0.01))
    elif kind == "medium":  # mean between 300 and 600: look-ahead 256
        reads = _draw(rng, [src["genome"], src["single"] + src["other"]], rng.integers(320, 581, size=700))
        # a few Ns, elsewhere than the ragged kind's and in a shorter batch: a packed batch with N positions behind ANOTHER one with N
        # positions is what shows marks of the first (sketch_wave_kernel's bitmap) that outlive it -- behind itself a batch sets the same bits
        for r in reads[::8]:
            r[rng.integers(0, len(r), size=3)] = ord("N")
        out = _batch(reads)
    elif kind == "ragged":
        out = _batch(_ragged(rng, src["genome"]))
    elif kind == "ragged_clean":  # the ragged batch, every byte that is no base replaced by one: the same lengths, no N position left
        bases, offs = kind_batch("ragged")
        bases = bases.copy()
        bad = np.nonzero(~_IS_BASE[bases])[0]
        bases[bad] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=bad.size)]
        out = (bases, offs.copy())
    else:
        raise KeyError(kind)
    for a in out:
        a.setflags(write=False)
    _CACHE[("kind", kind)] = out
    return out


def kind_packed(kind):
    """(words u32, npos u64) of the kind's batch (drprg_amd.pandora.pack_reads, the host packer)"""
    if ("packed", kind) not in _CACHE:
        from drprg_amd.pandora import pack_reads
        _CACHE[("packed", kind)] = pack_reads(kind_batch(kind)[0])
    return _CACHE[("packed", kind)]


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------
def _build(seed, reset_gap=24):
    """greedy: the next state is one that closes the most open pairs (adjacent with the last batch, two apart with the one before it); a
    reset() goes in front of a batch once per kind that has had none behind it yet, at least reset_gap batches after the last one.  A pair
    across a reset does not count: reset() completes what is in flight."""
    rng = np.random.default_rng(seed)
    n = len(STATES)
    open1 = np.ones((n, n), bool)
    open2 = np.ones((n, n), bool)
    kind_of = [KINDS.index(k) for k, _ in STATES]
    need_reset = set(range(len(KINDS)))
    need_entry = {(k, e) for k in range(len(KINDS)) for es in ENTRIES.values() for e in es}
    steps, ids, since_reset = [], [], 0  # (since_reset: batches since the last reset)
    while len(steps) < MAX_STEPS and (open1.any() or open2.any() or need_reset or need_entry):
        prev = ids[-1] if since_reset >= 1 else None
        prev2 = ids[-2] if since_reset >= 2 else None
        reset = False
        if ids and kind_of[ids[-1]] in need_reset and since_reset >= reset_gap:
            reset, prev, prev2 = True, None, None
        gain = np.zeros(n)
        if prev is not None:
            gain += open1[prev]
        if prev2 is not None:
            gain += open2[prev2]
        # (among equals: the state after which one batch can close two pairs most often, then the one from which the most pairs are open)
        both = (open1 & open2[prev]).sum(axis=1) if prev is not None else np.zeros(n)
        gain = gain * 100000 + both * 100 + open1.sum(axis=1) + open2.sum(axis=1)
        best = np.nonzero(gain == gain.max())[0]
        s = int(best[rng.integers(len(best))])
        kind, packed = STATES[s]
        entries = ENTRIES[packed]
        last_kind = kind_of[ids[-1]] if ids else None
        wanted = [e for e in entries if (last_kind, e) in need_entry]
        entry = (wanted or entries)[int(rng.integers(len(wanted or entries)))]
        if reset:
            need_reset.discard(last_kind)
            since_reset = 0
        need_entry.discard((last_kind, entry))
        if prev is not None:
            open1[prev, s] = False
        if prev2 is not None:
            open2[prev2, s] = False
        steps.append(Step(kind, packed, entry, reset))
        ids.append(s)
        since_reset += 1
    return steps


def schedule():
    """The schedule: the shortest of eight seeded greedy runs (SEED .. SEED + 7), at most MAX_STEPS batches"""
    if "schedule" not in _CACHE:
        _CACHE["schedule"] = min((_build(SEED + i) for i in range(8)), key=len)
    return _CACHE["schedule"]


def coverage_of(steps):
    """what a schedule covers, counted from the schedule alone: dict(pairs1, pairs2 = ordered state pairs adjacent / two apart with no reset
    between them, entry_after = {(kind, entry point of the next batch)}, reset_after = {kind}, resets)"""
    pairs1, pairs2, entry_after, reset_after = set(), set(), set(), set()
    for i, st in enumerate(steps):
        if i >= 1:
            entry_after.add((steps[i - 1].kind, st.entry))
            if st.reset_before:
                reset_after.add(steps[i - 1].kind)
            else:
                pairs1.add(((steps[i - 1].kind, steps[i - 1].packed), (st.kind, st.packed)))
        if i >= 2 and not st.reset_before and not steps[i - 1].reset_before:
            pairs2.add(((steps[i - 2].kind, steps[i - 2].packed), (st.kind, st.packed)))
    return dict(pairs1=pairs1, pairs2=pairs2, entry_after=entry_after, reset_after=reset_after, resets=sum(s.reset_before for s in steps))


# ---- the expected results ------------------------------------------------------------------------------------------------------------------
COUNTERS = ("reads", "bases", "minimizers", "hits", "clusters_kept", "hits_kept")


def oracle_of_kinds(oracle, w, k, illumina, threads=1):
    """{kind: (coverage u32, reads per PRG u32, counters)} by the oracle on its own index of the panel, once per (w, k, illumina)"""
    key = ("oracle", w, k, illumina)
    if key not in _CACHE:
        from util import cluster_fraction, map_params
        p = panel()[0]
        ikey = ("index", w, k)
        if ikey not in _CACHE:
            _CACHE[ikey] = oracle.build_index(p.prgs, w, k)
        idx = _CACHE[ikey]
        md, er = map_params(k, illumina)
        frac = cluster_fraction(er, k)

        def one(kind):
            bases, offs = kind_batch(kind)
            cov, prg, cnt = oracle.map_reads(bases, offs, idx, w, k, md, frac, 10)
            cov.setflags(write=False)
            prg.setflags(write=False)
            return kind, (cov, prg, cnt)

        if threads > 1:  # (the C call releases the GIL)
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(threads) as pool:
                _CACHE[key] = dict(pool.map(one, KINDS))
        else:
            _CACHE[key] = dict(one(kind) for kind in KINDS)
    return _CACHE[key]


class RunningSum:
    """the oracle's vectors and counters summed over the batches mapped since the last reset (u32 vectors wrap as the device's do)"""

    def __init__(self, per_kind):
        self.per_kind = per_kind
        cov, prg, _ = per_kind[KINDS[0]]
        self.cov, self.prg = np.zeros_like(cov), np.zeros_like(prg)
        self.cnt = dict.fromkeys(COUNTERS, 0)

    def reset(self):
        self.cov[:] = 0
        self.prg[:] = 0
        self.cnt = dict.fromkeys(COUNTERS, 0)

    def add(self, kind):
        cov, prg, cnt = self.per_kind[kind]
        self.cov += cov
        self.prg += prg
        for key in COUNTERS:
            self.cnt[key] += cnt[key]


def describe(steps, i):
    """the batch at index i of the schedule, and the two before it, for an assertion message"""
    def one(j):
        st = steps[j]
        return f"{st.kind}/{'packed' if st.packed else 'ascii'} via {st.entry}" + (" after reset()" if st.reset_before else "")
    before = ", ".join(f"[{j}] {one(j)}" for j in range(max(0, i - 2), i))
    return f"schedule index {i}: {one(i)}; before it: {before or 'nothing'}"
