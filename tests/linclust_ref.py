"""Restatement and case list of the linear-time pre-step (spec UC-1 E8a, unicore_amd/csrc/uc_linclust.hip), shared by tests/test_linclust_cases.py
(CPU) and tests/test_linclust_kernels_gpu.py (device).

pairs(s3, pattern, m) is written from the text of E8a in oracle/uc_oracle.h in plain Python integers and owes nothing to uc_oracle.c: every sequence
keeps the m k-mers with the smallest (hash, position) among its k-mers without an X under a `1` of the pattern, hash = SplitMix64 finaliser of the
k-mer value; the kept entries are grouped by k-mer value; the centre of a group is its longest member (ties: smallest id); every other member
gives a pair (centre, member); the list is unique and sorted.  Alongside the pairs it counts the events the cases were built for, so that the case
list proves on the CPU that it holds what it was meant to hold (EVENTS; the totals are pinned in test_linclust_cases.py).

A case is a list of 3Di code arrays; the amino-acid track plays no part in E8a and is all zero.  Every case is deterministic (seeded), no sequence
is longer than 65,535 and each is the smallest shape at which its branch can go wrong."""
import numpy as np

import util

X = 20
KA = 20
MASK = (1 << 64) - 1
PATTERNS = ("1101010011", "111111", "".join("1" if i in (0, 5, 13, 20, 30, 31) else "0" for i in range(32)))
PATTERN_IDS = ("default", "contiguous", "wide32")
MS = (1, 5, 20, 300)
LMAX = 65535

EVENTS = ("seq_no_kmer", "seq_fewer_than_m", "seq_exactly_m", "kmers_dropped_for_x", "picks_with_x_under_zero", "seq_repeated_value_in_picks",
          "groups_length_tie", "groups_all_lengths_equal", "groups_centre_first", "groups_centre_last", "groups_centre_middle",
          "groups_over_256", "groups_cross_256", "groups_head_on_last_thread", "pairs_from_2plus_groups", "members_with_2plus_centres",
          "seqs_centre_and_member", "chains_of_three", "centre_is_id0", "centre_is_last_id", "no_entries", "no_pairs")


def offsets(pattern):
    return [i for i, c in enumerate(pattern) if c == "1"], len(pattern)


def splitmix64(v):
    z = (v + 0x9E3779B97F4A7C15) & MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


_CAND = {}


def candidates(seq, pattern):
    """the k-mers of one sequence without an X under a `1`, sorted by (hash, position) -> (list of (hash, position, value, X under a `0`), dropped)"""
    key = (pattern, np.asarray(seq, np.uint8).tobytes())
    if key in _CAND:
        return _CAND[key]
    offs, span = offsets(pattern)
    zeros = [i for i in range(span) if i not in offs]
    s = [int(c) for c in seq]
    out, dropped = [], 0
    for j in range(0, len(s) - span + 1):
        if j > 65535:          # the spec's cap on the k-mer position; the engine refuses sequences it could bind on
            break
        letters = [s[j + o] for o in offs]
        if any(c >= KA for c in letters):
            dropped += 1
            continue
        v = 0
        for t in range(5, -1, -1):
            v = v * KA + letters[t]
        out.append((splitmix64(v), j, v, any(s[j + z] >= KA for z in zeros)))
    out.sort()
    _CAND[key] = (out, dropped)
    return out, dropped


def pairs(s3, pattern, m):
    """-> (uint32 [np, 2] sorted unique (centre, member) pairs, dict of event counts)"""
    n = len(s3)
    ev = dict.fromkeys(EVENTS, 0)
    lens = [len(x) for x in s3]
    ent = []
    for sid, seq in enumerate(s3):
        cand, dropped = candidates(seq, pattern)
        ev["kmers_dropped_for_x"] += dropped
        ev["seq_no_kmer"] += len(cand) == 0
        ev["seq_fewer_than_m"] += 0 < len(cand) < m
        ev["seq_exactly_m"] += len(cand) == m
        picks = cand[:m]
        ev["picks_with_x_under_zero"] += sum(1 for c in picks if c[3])
        ev["seq_repeated_value_in_picks"] += len({c[2] for c in picks}) < len(picks)
        ent.extend((c[2], sid) for c in picks)
    ent.sort()
    made = {}          # pair -> number of groups that produced it
    b = 0
    while b < len(ent):
        e = b
        while e < len(ent) and ent[e][0] == ent[b][0]:
            e += 1
        members = sorted({sid for _, sid in ent[b:e]})
        top = max(lens[x] for x in members)
        centre = min(x for x in members if lens[x] == top)
        if len(members) >= 2:
            ev["groups_length_tie"] += sum(1 for x in members if lens[x] == top) >= 2
            ev["groups_all_lengths_equal"] += all(lens[x] == top for x in members)
            ev["groups_centre_first"] += centre == members[0]
            ev["groups_centre_last"] += centre == members[-1]
            ev["groups_centre_middle"] += members[0] < centre < members[-1]
        ev["groups_over_256"] += e - b > 256
        ev["groups_cross_256"] += b // 256 != (e - 1) // 256
        ev["groups_head_on_last_thread"] += b % 256 == 255 and e - b >= 2
        for x in members:
            if x != centre:
                made[(centre, x)] = made.get((centre, x), 0) + 1
        b = e
    out = sorted(made)
    ev["pairs_from_2plus_groups"] = sum(1 for k in made.values() if k >= 2)
    centres_of = {}
    for c, x in out:
        centres_of.setdefault(x, set()).add(c)
    centres = {c for c, _ in out}
    ev["members_with_2plus_centres"] = sum(1 for v in centres_of.values() if len(v) >= 2)
    ev["seqs_centre_and_member"] = len(centres & set(centres_of))
    ev["chains_of_three"] = sum(1 for c, x in out if c in centres_of)      # a > c > x: the centre of this pair is the member of another
    ev["centre_is_id0"] = int(0 in centres)
    ev["centre_is_last_id"] = int(n - 1 in centres)
    ev["no_entries"] = int(not ent)
    ev["no_pairs"] = int(not out)
    return np.array(out, np.uint32).reshape(-1, 2), ev


# ---------------------------------------------------------------- case builders
def _rnd(rng, L):
    return rng.integers(0, 20, L, dtype=np.uint8)


def lengths_case(pattern, seed=1):
    """prefixes of ONE random sequence: lengths 0, 1, span - 1, span, span + 1, exactly m - 1 / m / m + 1 k-mers for m = 5 and 20, and 63 .. 129
    candidates (the 64-lane stride and the wave reduction); in a seeded order, so that the longest of a group stands anywhere in it"""
    _, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    base = _rnd(rng, 129 + span - 1)
    ncand = [4, 5, 6, 19, 20, 21, 63, 64, 65, 127, 128, 129]
    L = [0, 1, span - 1, span, span + 1] + [c + span - 1 for c in ncand]
    return [base[:L[i]].copy() for i in rng.permutation(len(L))]


def longest_case(pattern, seed=2):
    """one sequence of 65,535 residues (65,536 - span candidates), copies of its first 2,000 and last 300 residues, and a short sequence made of
    the windows around its three smallest k-mers (a pair at every m; the windows lie anywhere in the 65,526 positions)"""
    _, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    a = _rnd(rng, LMAX)
    cand, _ = candidates(a, pattern)
    small = np.concatenate([a[max(c[1] - 2, 0):c[1] + span + 2] for c in cand[:3]])
    return [a[:2000].copy(), a, a[-300:].copy(), small]


def _cover_period(offs):
    """the largest g in 2 .. 6 at which an X on every g-th residue falls under a `1` of every k-mer"""
    return max(g for g in range(2, 7) if {o % g for o in offs} == set(range(g)))


def x_case(pattern, seed=3):
    """an all-X sequence; one whose every k-mer has an X under a `1`; a normal sequence, and its copy with an X under the first `0` of the k-mer
    with the smallest hash (that k-mer must survive and stay the copy's first pick) and of a few more k-mers; a copy with an X under a `1` of it"""
    offs, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    dead = _rnd(rng, 60)
    dead[::_cover_period(offs)] = X
    base = _rnd(rng, 90)
    out = [np.full(40, X, np.uint8), dead, base]
    zeros = [i for i in range(span) if i not in offs]
    cand, _ = candidates(base, pattern)
    if zeros:
        cp = base.copy()
        for c in cand[:3]:          # (a later X may not fall under a `1` of the smallest k-mer)
            if c is cand[0] or c[1] + zeros[0] - cand[0][1] not in offs:
                cp[c[1] + zeros[0]] = X
        out.append(cp)
    hit = base.copy()
    hit[cand[0][1] + offs[-1]] = X
    out.append(hit)
    return out


def no_valid_case(pattern, seed=4):
    """no sequence has a valid k-mer: all-X, too short, empty, and an X under a `1` of every k-mer"""
    offs, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    dead = _rnd(rng, 70)
    dead[::_cover_period(offs)] = X
    return [np.full(40, X, np.uint8), _rnd(rng, span - 1), np.zeros(0, np.uint8), dead, np.full(span, X, np.uint8)]


def repeats_case(pattern, seed=5):
    """homopolymers of two lengths, period-2 and period-3 repeats, and - for m = 5 and 20 - a sequence whose smallest k-mer occurs twice with a
    one-k-mer partner that holds its (m + 1)-th pick: m picks including the repeat stop short of it, m distinct values would reach it"""
    offs, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    p2, p3 = np.tile(np.array([3, 7], np.uint8), 40), np.tile(np.array([1, 4, 9], np.uint8), 30)
    out = [np.full(span + 20, 2, np.uint8), np.full(span + 37, 2, np.uint8), p2[:span + 31].copy(), p2[1:span + 31].copy(), p3[:span + 33].copy(), p3[2:span + 28].copy()]
    t = _rnd(rng, 100)
    j0 = candidates(t, pattern)[0][0][1]
    r = np.concatenate([t, t[j0:j0 + span]])          # the smallest k-mer of t once more, behind span - 1 junction k-mers
    cand, _ = candidates(r, pattern)
    assert cand[0][2] == cand[1][2] and cand[0][1] < cand[1][1]
    out.append(r)
    for m in (5, 20):
        assert len({c[2] for c in cand[:m + 1]}) == m and cand[m][2] not in {c[2] for c in cand[:m]}
        out.append(r[cand[m][1]:cand[m][1] + span].copy())
    return out


def _family(rng, lens, span):
    """sequences that share one random core of 30 k-mers and differ in their random tails (lens: the lengths without span)"""
    k = _rnd(rng, 29 + span)
    return [np.concatenate([k, _rnd(rng, L - 29)]) for L in lens]


def centre_case(pattern, seed=6):
    """families around a shared core with the longest member first (id 0), in the middle and last, with two longest members, with all members
    equal in length (three near copies), and a last family whose longest member is id n - 1"""
    _, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    out = _family(rng, [120, 70, 60], span) + _family(rng, [60, 125, 70, 50], span) + _family(rng, [75, 75, 50], span) + _family(rng, [50, 80, 80], span)
    eq = _rnd(rng, 66)
    for pos in (5, 33, 60):
        c = eq.copy()
        c[pos] = (c[pos] + 1) % 20
        out.append(c)
    return out + _family(rng, [55, 65, 130], span)


BIG_PAD = {PATTERNS[0]: 12, PATTERNS[1]: 27, PATTERNS[2]: 5}      # chosen on the CPU: at m = 20 a group of > 256 entries then starts at an index = 255 mod 256


def big_case(pattern, seed=7, pad=None):
    """300 exact copies of one 150-residue sequence, relatives of it (mutated, extended at either end, the longest last) and `pad` unrelated short
    sequences in front: groups of hundreds of entries, every pair made by up to m groups.  The padding moves the groups in the sorted entry order;
    test_linclust_cases.py asserts that a group's head falls on the last thread of a 256-thread block."""
    _, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    base = _rnd(rng, 150)
    out = [_rnd(rng, span + 14 + k % 7) for k in range(BIG_PAD[pattern] if pad is None else pad)]
    mut = base.copy()
    mut[::17] = (mut[::17] + 3) % 20
    out.append(np.concatenate([_rnd(rng, 20), base]))           # a longer relative in front of the copies: centre first
    out += [base.copy() for _ in range(150)]
    out.append(mut)
    out.append(base[:90].copy())
    out += [base.copy() for _ in range(150)]
    out.append(np.concatenate([base[40:], _rnd(rng, 80)]))      # shares the second half only, longest of its groups: centre last
    return out


def overlap_case(pattern, seed=8):
    """a member with two centres (x shares one block with p and another with q), and a chain a > b > c > d in which b and c are both centre and member"""
    _, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    B = 24 + span          # a block of 25 k-mers
    k1, k2 = _rnd(rng, B), _rnd(rng, B)
    p, q, x = np.concatenate([k1, _rnd(rng, 70)]), np.concatenate([_rnd(rng, 80), k2]), np.concatenate([k1, k2])
    c1, c2, c3 = _rnd(rng, B), _rnd(rng, B), _rnd(rng, B)
    a = np.concatenate([_rnd(rng, 60), c1, _rnd(rng, 60)])
    b = np.concatenate([c1, _rnd(rng, 10), c2])
    c = np.concatenate([c2, c3[:B - 4]])
    d = c3[:B - 4].copy()
    return [x, p, q, d, c, b, a]


def combined(pattern, with_longest=False):
    """every edge case in one database (the 65,535-residue sequence only on request)"""
    out = []
    for f in (lengths_case, x_case, repeats_case, centre_case, overlap_case, big_case, no_valid_case):
        out += f(pattern)
    if with_longest:
        out += longest_case(pattern)
    return out


SIZES = (1, 2, 3, 4, 5, 255, 256, 257)


def sized_case(pattern, n, seed=9):
    """n sequences for the 32 + nbits key of the pair sort: a family whose longest member comes LAST (centre n - 1: the top bit of the key), in front
    of it the centre families and unrelated short sequences as padding"""
    _, span = offsets(pattern)
    rng = np.random.default_rng(seed)
    tail = _family(rng, [45, 52, 90], span)
    if n <= 3:
        return tail[3 - n:]
    head = centre_case(pattern)[:n - 3]
    pad = [_rnd(rng, 12 + k % 19) for k in range(n - 3 - len(head))]
    return head + pad + tail


CAMPAIGN_SEEDS = (101, 102, 103, 104, 105)


def cases(pattern):
    """-> list of (name, s3, tuple of m): the whole list for one pattern.  m = 1000 runs on two small cases everywhere and on the longest sequence
    under the default pattern only (one wave, about a million loop trips)."""
    out = [("lengths", lengths_case(pattern), MS), ("x", x_case(pattern), MS), ("no_valid", no_valid_case(pattern), MS),
           ("repeats", repeats_case(pattern), MS + (1000,)), ("centre", centre_case(pattern), MS + (1000,)), ("big", big_case(pattern), MS),
           ("overlap", overlap_case(pattern), MS), ("longest", longest_case(pattern), MS + ((1000,) if pattern == PATTERNS[0] else ()))]
    out += [("n%d" % n, sized_case(pattern, n), MS) for n in SIZES]
    out.append(("combined", combined(pattern), (5, 20)))
    out += [("family%d" % seed, util.family_db(seed, with_x=True)[0], MS) for seed in CAMPAIGN_SEEDS]
    return out


def oracle_pairs(O, s3, pattern, m):
    """the oracle's E8a on the same input -> uint32 [np, 2]"""
    odb = O.OracleDb(s3=s3, sa=[np.zeros(len(x), np.uint8) for x in s3])
    return np.asarray(O.linclust_pairs(odb, O.default_params(pattern=pattern), m), np.uint32).reshape(-1, 2)


_REF = {}


def reference(pattern):
    """the restatement on the whole list of one pattern, computed once per session and shared: -> {(name, m): (pairs, events)}"""
    if pattern not in _REF:
        _REF[pattern] = {(name, m): pairs(s3, pattern, m) for name, s3, ms in cases(pattern) for m in ms}
    return _REF[pattern]
