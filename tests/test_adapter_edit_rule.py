"""The indel rule of adapter trimming (tests/adapter_edit_rule.py) against its own statement letter by letter, the plain rule at E = 0, cuts
worked by hand, the mirror, the bounded windows the kernels rely on, the census of the kernel batch, the lane arithmetic walked on the CPU,
the settings on a host-only context and the executables' usage errors.  No device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adapter_edit_rule as rule
import adapter_rule as plain
from adapter_edit_rule import FRONT, cut_point, cut_range, cut_ranges, front_cut_point, kernel_batch
from adapter_rule import NEXTERA, TRUSEQ, error_milli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 22
NO_CUT = dict(reads_seen=0, bases_seen=0, reads_cut=0, bases_cut=0, reads_emptied=0)
NAMES = ["12", "16", "17", "32", "33", "64", "33+19"]
RATES = ["0", "0.1", "0.2", "0.5"]


# ---- the rule's text, as slowly as it reads -------------------------------------------------------------------------------------------------
def _same(b, a):
    return chr(b).upper() in "ACGT" and chr(b).upper() == chr(a).upper()


def _ed(S, T):
    """the Levenshtein distance of two byte strings, unit costs, by the full table"""
    D = [[0] * (len(T) + 1) for _ in range(len(S) + 1)]
    for i in range(len(S) + 1):
        for j in range(len(T) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (0 if _same(T[j - 1], S[i - 1]) else 1), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D[len(S)][len(T)]


def _naive3(r, adapters, e, O):
    """the 3' rule by its text: the smallest matching start of r, or None"""
    n = len(r)
    for p in range(n):
        for A in adapters:
            A = A.encode()
            m = len(A)
            full = lambda s: m if s == n else min(_ed(A, r[s:q]) for q in range(s, n + 1))
            c = n - p
            if c < m and c >= O and sum(not _same(r[p + j], A[j]) for j in range(c)) <= c * e // 1000:
                return p
            f = full(p)
            if f <= m * e // 1000 and full(p + 1) >= f:
                return p
    return None


def _naive5(r, adapters, e, O):
    """the 5' rule as the header states it directly: the largest matching end q of r, or None"""
    n = len(r)
    for q in range(n, 0, -1):
        for A in adapters:
            A = A.encode()
            m = len(A)
            g = lambda t: m if t == 0 else min(_ed(A, r[p:t]) for p in range(0, t + 1))
            if q < m and q >= O and sum(not _same(r[j], A[m - q + j]) for j in range(q)) <= q * e // 1000:
                return q
            v = g(q)
            if v <= m * e // 1000 and g(q - 1) >= v:
                return q
    return None


def test_the_rule_equals_its_text_on_tiny_reads():
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
    cuts3 = cuts5 = 0
    for _ in range(260):
        adapters = ["".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 8)))) for _ in range(int(rng.integers(1, 3)))]
        e = int(rng.choice([0, 100, 200, 334, 500]))
        O = int(rng.integers(1, min(len(a) for a in adapters) + 1))
        r = bytes(rng.choice(letters, size=int(rng.integers(0, 15))))
        if len(r) > 3 and rng.integers(2):
            A = adapters[0].encode()
            at = int(rng.integers(0, len(r)))
            r = r[:at] + A + r[at:]
        want3, want5 = _naive3(r, adapters, e, O), _naive5(r, adapters, e, O)
        assert cut_point(r, adapters, e, O) == want3, (r, adapters, e, O)
        assert front_cut_point(r, adapters, e, O) == want5, (r, adapters, e, O)
        cuts3 += want3 is not None
        cuts5 += want5 is not None
    assert cuts3 > 60 and cuts5 > 60


def test_at_e_0_the_indel_rule_is_the_plain_rule_on_the_whole_plain_batch():
    b = plain.kernel_batch("33", "0")
    cut = 0
    for r, (x, y) in zip(b["reads"], b["ranges"]):
        want = plain.cut_point(r, b["adapters"], 0, b["O"], x, y) if y > x else None
        assert cut_point(r, b["adapters"], 0, b["O"], x, y) == want
        cut += want is not None
    assert cut > 300


def test_cuts_worked_by_hand():
    A, e, O = TRUSEQ[:33], error_milli("0.1"), 3  # L(33) = 3
    genome = b"AC" * 16                            # 32 bases that hold no part of the adapter
    whole = genome + A.encode() + b"ACCA"
    assert cut_point(whole, [A], e, O) == 32 and plain.cut_point(whole, [A], e, O) == 32
    inserted = genome + A[:10].encode() + b"C" + A[10:].encode() + b"ACCA"
    deleted = genome + A[:10].encode() + A[11:].encode() + b"ACCA"
    substituted = genome + A[:10].encode() + b"C" + A[11:].encode() + b"ACCA"
    assert A[10] != "C"
    # one base inserted or deleted at letter 10: every letter behind it is shifted, the plain rule sees 12 or more mismatches and finds nothing
    assert plain.cut_point(inserted, [A], e, O) is None and plain.cut_point(deleted, [A], e, O) is None
    assert cut_point(inserted, [A], e, O) == 32 and cut_point(deleted, [A], e, O) == 32
    assert plain.cut_point(substituted, [A], e, O) == 32 and cut_point(substituted, [A], e, O) == 32
    # the scores around the occurrence: full(32) = 1; full(31) = 2 and full(30) = 3 lie within L(33) too and are no match because the
    # next start scores lower; full(33) = 2, one letter of the adapter gone
    full = rule.scores(plain._upper(inserted), plain._upper(A.encode()))
    assert full[29:35].tolist() == [4, 3, 2, 1, 2, 3]
    # four edits are one too many
    assert cut_point(genome + A[:5].encode() + A[6:12].encode() + A[13:20].encode() + A[21:28].encode() + A[29:].encode() + b"ACCA", [A], e, O) is None
    # a partial overlap takes substitutions only (clause (a)): eleven letters with one wrong pass at L(11) = 1, ten with one missing do not
    assert cut_point(genome + A[:5].encode() + b"A" + A[6:11].encode(), [A], e, O) == 32 and A[5] != "A"
    assert cut_point(genome + A[:5].encode() + A[6:11].encode(), [A], e, 6) is None
    assert cut_point(genome + A[:5].encode() + A[6:11].encode(), [A], e, O) == 39  # (its last three letters, AGA, are an overlap of their own at O = 3)
    # the 5' side: the ligation adapter with a letter missing in front of a read; the cut is behind its last letter
    F = FRONT[-28:]
    assert front_cut_point(F[:7].encode() + F[8:].encode() + genome, [F], e, O) == 27
    assert front_cut_point(b"CA" + F.encode() + genome, [F], e, O) == 30
    assert front_cut_point(F[-9:].encode() + genome, [F], e, O) == 9 and front_cut_point(F[-2:].encode() + genome, [F], e, O) is None
    # both: the 5' adapter is sought in what the 3' cut left, and a read the two consume between them is a read of no bases
    assert cut_range(F.encode() + genome + A.encode(), [A], [F], e, O) == (28, 60)
    assert cut_range(F.encode() + A.encode(), [A], [F], e, O) == (28, 28)
    assert cut_ranges([F.encode() + A.encode(), genome], [(0, 61), (0, 32)], [A], [F], e, O) == (
        [(28, 28), (0, 32)], dict(reads_seen=2, bases_seen=93, reads_cut=1, bases_cut=33, reads_emptied=0),
        dict(reads_seen=2, bases_seen=60, reads_cut=1, bases_cut=28, reads_emptied=1))


def test_the_front_rule_is_the_end_rule_on_the_reversed_read():
    rng = np.random.default_rng(8)
    hits = 0
    for i in range(60):
        F = FRONT[-int(rng.choice([12, 17, 28, 33])):]
        e = int(rng.choice([0, 100, 200]))
        body = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(20, 90))))
        r = (rule.edit(rng, F, *[int(v) for v in rng.integers(0, 2, size=3)]) if i % 3 else b"") + body
        q = front_cut_point(r, [F, NEXTERA], e, 3)
        p = cut_point(r[::-1], [F[::-1], NEXTERA[::-1]], e, 3)
        assert (q is None) == (p is None) and (q is None or q == len(r) - p)
        hits += q is not None
    assert hits > 20


def test_scores_from_a_bounded_window_give_every_verdict():
    """what lets the kernels tile the buffer: scores computed afresh from a window that ends m + L(m) + 2 bases behind p, or at the range's
    end when that is nearer, give clause (b) the verdict of scores over the whole read, at every p"""
    rng = np.random.default_rng(9)
    e = 300
    total = 0
    for A in (TRUSEQ[:12], TRUSEQ[:33], TRUSEQ):
        a, m = plain._upper(A.encode()), len(A)
        W, L = rule.warmup(m, e), len(A) * e // 1000
        for _ in range(6):
            r = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=400))
            for at in (30, 150, 290):
                occ = rule.edit(rng, A, int(rng.integers(0, L)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), keep=0)
                r[at:at + len(occ)] = occ
            r = plain._upper(bytes(r))
            full = rule.scores(r, a)
            whole = (full[:-1] <= L) & (full[1:] >= full[:-1])
            for p in range(r.size):
                w = rule.scores(r[p:min(p + W, r.size)], a)
                assert bool(w[0] <= L and w[1] >= w[0]) == bool(whole[p]), (A, p)
            total += int(whole.sum())
    assert total > 50


def test_the_rule_for_whole_samples_is_the_rule():
    rng = np.random.default_rng(1)
    L = [int(x) for x in np.concatenate([rng.integers(0, 300, size=60), rng.integers(1000, 2500, size=4)])]
    bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=sum(L))
    offs = np.concatenate([[0], np.cumsum(L)])
    A, F = TRUSEQ[:33], FRONT[-28:]
    reads, kinds = rule.plant(bases, offs, A, F, 100, seed=3)
    assert all(kinds.count(k) > 5 for k in ("both", "front", "end", "none"))
    rg = [(0, len(r)) for r in reads]
    rg[3], rg[8] = (5, len(reads[3]) - 7), (2, 2)
    for ad3, ad5 in (([A, NEXTERA], [F]), ([A], []), ([], [F, NEXTERA[::-1]])):
        one = cut_ranges(reads, rg, ad3, ad5, 100, 3)
        assert rule.cut_ranges_many(reads, rg, ad3, ad5, 100, 3) == one
        assert (one[1]["reads_cut"] > 25) == bool(ad3) and (one[2]["reads_cut"] > 25) == bool(ad5)


# ---- the kernel batch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", RATES)
@pytest.mark.parametrize("name", NAMES)
def test_the_census_of_the_kernel_batch(name, E):
    b = kernel_batch(name, E)
    c = rule.census(b)  # (raises when a class is empty or not what it is meant to be)
    m = len(b["ad3"][0])
    n_bases = sum(len(r) for r in b["reads"])
    assert 5 * rule.TILE < n_bases < 10 * rule.TILE
    for cls in ("short run", "edge lengths", "the adapter itself", "the front adapter itself", "partial from O", "front partial from O", "3' subs at the limit",
                "3' ins one over the limit", "5' dels at the limit", "5' subs one over the limit", "N over the limit", "front N over the limit", "lower case",
                "both adapters in one read", "the two cuts take the read between them", "genome bases clause (b) keeps", "genome bases clause (b) keeps, front",
                "straddles end", "front straddles begin", "front inside the range", "warm-up in the neighbour", "front warm-up in the neighbour",
                "long with both adapters", "long without adapter", "3' partial at the limit", "5' partial at the limit", "worse to the left", "worse to the right",
                "split 2", "split 5", "front split 2", "front split 5", "split rest"):
        assert cls in c, cls
    if b["e"]:
        for cls in ("3' partial one over the limit", "5' partial one over the limit", "N for a mismatch", "front N for a mismatch"):
            assert cls in c, cls
    for label in ("stretch", "wave", "tile"):
        for cls in (f"ends at a {label} boundary", f"ends one over a {label} boundary", f"front begins at a {label} boundary", f"front begins one before a {label} boundary"):
            assert cls in c, cls
    if m == 64:  # overlaps of more than 32 letters with their mismatches past the 32nd letter met: the comparison's second word
        assert max(b["partial_lengths"][3]) > 32 and "3' partial at the limit past letter 32" in c and "5' partial at the limit past letter 32" in c
        if b["e"]:
            assert "3' partial one over the limit past letter 32" in c and "5' partial one over the limit past letter 32" in c
            assert len(b["classes"]["indel beside letter 32"][0]) == 8 and len(b["classes"]["front indel beside letter 32"][0]) == 8
    if len(b["ad3"]) > 1:
        assert "second adapter" in c and "second front adapter" in c
    # What could not be drawn.  Up to E = 0.2: nothing.  At E = 0.5 half the letters may be wrong, and these are left to whatever the rule
    # says: an occurrence with L + 1 edits still holds a shorter stretch within the limit (the "one over" classes and N over the limit);
    # one or two adapter letters in front of the run make a longer overlap pass (front partial below O); the worse match to the right
    # reaches past where it was put.  The pair: the second adapter of a side finds itself in the letters of the first, which takes the
    # overlaps, the splits and the narrowed ranges with it.  Everything else holds its intended range at E = 0.5 as well.
    one_over = {"3' ins one over the limit", "5' ins one over the limit", "front partial below O", "worse to the right"}
    noisy = {"12": one_over, "16": one_over, "17": one_over, "32": one_over, "33": one_over,
             "64": one_over | {"3' partial one over the limit past letter 32", "3' subs one over the limit", "5' subs one over the limit", "N over the limit",
                               "front N over the limit"},
             "33+19": one_over | {"3' subs one over the limit", "N over the limit", "front inside the range", "front partial from O", "front split 2", "front split 5",
                                  "front straddles begin", "front warm-up in the neighbour", "genome bases clause (b) keeps, front", "partial below O", "partial from O",
                                  "split 2", "split 5", "straddles end below O", "two front occurrences"}}
    assert set(b["relaxed"]) == (noisy[name] if b["noisy"] else set()), sorted(set(b["relaxed"]))
    # the geometry classes lie where they say: the stretched occurrence ends (3') or begins (5') at a multiple of the unit, or one base off
    # (at E = 0.5 each side's classes are held with that side alone set: want3, want5)
    starts = np.concatenate([[0], np.cumsum([len(r) for r in b["reads"]])])
    w3, w5 = (b["want3"], b["want5"]) if b["noisy"] else (b["want"], b["want"])
    for label, unit in (("stretch", rule.STRETCH), ("wave", rule.WAVE), ("tile", rule.TILE)):
        for over in (0, 1):
            (i,) = b["classes"][f"ends {'one over' if over else 'at'} a {label} boundary"][0]
            tail = len(b["reads"][i]) - w3[i][1]  # the occurrence and the 5 to 19 random bases behind it
            end = int(starts[i + 1]) - over
            assert any((end - t) % unit == 0 for t in range(5, 20)) and tail >= m + 5, (label, over)
            (i,) = b["classes"][f"front begins {'one before' if over else 'at'} a {label} boundary"][0]
            lead = w5[i][0]
            assert any((int(starts[i]) + lead - k + over) % unit == 0 for k in range(len(b["ad5"][0]) - 2, len(b["ad5"][0]) + len(b["ad5"][0]) * b["e"] // 1000 + 1)), (label, over)
    (i,) = b["classes"]["long with both adapters"][0]
    assert len(b["reads"][i]) > 20000 and (int(starts[i]) + 18000 + 1) % rule.TILE == 0
    # (at E = 0.5 the 3' rule cuts inside the 5' adapter at the read's start, and the 5' rule alone finds the 3' adapter at 18 000)
    assert b["noisy"] or b["want"][i] == (len(b["ad5"][0]), 18000)
    (i,) = b["classes"]["the two cuts take the read between them"][0]
    assert b["noisy"] or b["want"][i] == (len(b["ad5"][0]),) * 2
    # more short reads inside the first tile than the workgroup's table holds
    assert len(b["classes"]["short run"][0]) > rule.SLOTS + 100 and int(starts[rule.SLOTS + 100]) < rule.TILE


def test_the_constants_of_the_header_are_the_rules():
    text = open(os.path.join(ROOT, "drprg_amd", "csrc", "adapter_edit.h")).read()

    def const(name):
        return int(re.search(r"constexpr uint32_t %s = (\d+)" % name, text).group(1))

    assert const("AE_STRETCH") == rule.STRETCH and const("AE_THREADS") * rule.STRETCH == rule.TILE and 64 * rule.STRETCH == rule.WAVE and const("AE_SLOTS") == rule.SLOTS
    assert "AE_TILE = AE_THREADS * AE_STRETCH" in text and "AE_WAVE = 64 * AE_STRETCH" in text
    assert "return ad.max_len + ae_limit(ad.max_len, ad.error_milli) + 2u;" in text and rule.warmup(33, 100) == 38


def test_the_lane_arithmetic_walked_on_the_cpu(tmp_path):
    """adapter_edit.h is host code as well: every lane's walk against the rule as a plain table, three input forms, two geometries.  Built as
    plain C++ by $CXX or, without one, by the compiler the Makefile builds everything with; no compiler fails the test."""
    exe = str(tmp_path / "adapter_edit_walk")
    cxx = os.environ.get("CXX")
    argv = [cxx] if cxx and shutil.which(cxx) else [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    r = subprocess.run(argv + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "drprg_amd", "csrc"), os.path.join(ROOT, "tools", "adapter_edit_walk.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ranges checked" in r.stdout, (r.stdout, r.stderr)


def test_the_settings_on_a_host_only_context(tmp_path):
    from drprg_amd import Context
    from drprg_amd.pandora import DependencyError
    f = str(tmp_path / "dr.prg")
    open(f, "w").write(">g0\nACGTTGCAAGGCTTAACCGGATATCGCGATTAGGCATCAGT\n")
    ctx = Context(f, 5, 7, device=-1, from_files=False)
    A, F = TRUSEQ[:33], FRONT[-28:]
    for bad in (dict(seqs=[A], front=[F]),                                  # 5' adapters exist only with the flag
                dict(seqs=[A] * 5, indels=True), dict(seqs=[A], front=[F] * 5, indels=True), dict(seqs=[A], front=[""], indels=True),
                dict(seqs=[A], front=[F + F + F], indels=True), dict(seqs=[A], front=["ACGN"], indels=True), dict(seqs=["AC-T"], indels=True),
                dict(seqs=[A], front=[F], indels=True, error="0.501"), dict(seqs=[A], front=["ACGT"], indels=True, min_overlap=5),
                dict(seqs=["ACGT"], front=[F], indels=True, min_overlap=5), dict(seqs=[], front=[F], indels=True, min_overlap=29)):
        with pytest.raises(DependencyError) as e:
            ctx.set_adapters(**bad)
        assert e.value.code == EINVAL, bad
    from drprg_amd._lib import lib
    import ctypes as C
    arr = (C.c_char_p * 1)(A.encode())
    assert lib.drprg_hip_set_adapters2(ctx._h, arr, 1, arr, 0, 100, 0, 2) == -EINVAL  # an unknown flag bit
    assert lib.drprg_hip_set_adapters2(ctx._h, arr, 1, arr, 0, 100, 0, 0) == 0        # no flag, no 5' adapter: the plain rule
    ctx.set_adapters([A, NEXTERA], front=[F, "acgt", FRONT], indels=True, error="0.5", min_overlap=4)
    ctx.set_adapters([], front=[F], indels=True)
    ctx.set_adapters([A], indels=True, error=0, min_overlap=33)
    ctx.set_adapters([A])
    ctx.set_adapters([], indels=True)  # (nothing on either side clears)
    assert ctx.adapter_trim_info() == NO_CUT and ctx.front_adapter_info() == NO_CUT
    ctx.close()


@pytest.mark.parametrize("exe", ["pandora", "drprg"])
def test_usage_errors_exit_2_and_need_no_device(tmp_path, exe):
    path = os.path.join(ROOT, "drprg_amd", "bin", exe)
    head = [path, "map"] if exe == "pandora" else [path, "predict", "-x", str(tmp_path), "-i", "reads.fq"]
    tail = ["dr.prg", "reads.fq"] if exe == "pandora" else []
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a usage error comes before one is looked for)
    A, F = TRUSEQ[:12], FRONT[-12:]
    for flags, word in ((["--front-adapter", F], "--adapter-indels"), (["--adapter", A, "--front-adapter", F], "--front-adapter"),
                        (["--adapter-indels"], "--adapter-indels"), (["--adapter-indels", "--adapter-error", "0.2"], "--adapter-indels"),
                        (["--adapter-indels"] + ["--front-adapter", F] * 5, "--front-adapter"), (["--adapter-indels", "--front-adapter", ""], "--front-adapter"),
                        (["--adapter-indels", "--front-adapter", "A" * 65], "--front-adapter"), (["--adapter-indels", "--front-adapter", "ACGTN"], "--front-adapter"),
                        (["--adapter-indels", "--front-adapter"], "--front-adapter"),
                        (["--adapter-indels", "--adapter", A, "--front-adapter", "ACGT", "--adapter-min-overlap", "5"], "--adapter-min-overlap"),
                        (["--adapter-indels", "--adapter", "ACGT", "--front-adapter", F, "--adapter-min-overlap", "5"], "--adapter-min-overlap"),
                        (["--adapter-indels", "--front-adapter", F, "--adapter-min-overlap", "13"], "--adapter-min-overlap"),
                        (["--adapter-indels", "--adapter", A, "--adapter-error", "0.51"], "--adapter-error")):
        r = subprocess.run(head + flags + tail, capture_output=True, text=True, env=env)
        assert r.returncode == 2 and word in r.stderr, (flags, r.returncode, r.stderr)
