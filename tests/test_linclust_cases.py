"""CPU tier of the linear-time pre-step (spec UC-1 E8a): the oracle's uco_linclust_pairs against the plain-Python restatement of tests/linclust_ref.py on
every (case, m, pattern) of the shared case list, and the proof that the case list holds what it was built for - the restatement counts the events
(sequences without a k-mer, repeated picks, length ties, groups across a 256-entry boundary ...) and their totals are pinned here.  The device runs
the same list in tests/test_linclust_kernels_gpu.py."""
import numpy as np
import pytest

import linclust_ref as LR
from oracle import oracle_py as O

# totals of linclust_ref.EVENTS over every (case, m, pattern) of linclust_ref.cases(): a condition on the INPUTS, satisfied by the restatement alone
EVENT_TOTALS = {"seq_no_kmer": 3292, "seq_fewer_than_m": 5338, "seq_exactly_m": 152, "kmers_dropped_for_x": 6144, "picks_with_x_under_zero": 980,
                "seq_repeated_value_in_picks": 126, "groups_length_tie": 5260, "groups_all_lengths_equal": 2975, "groups_centre_first": 11518, "groups_centre_last":
                6178, "groups_centre_middle": 3388, "groups_over_256": 558, "groups_cross_256": 691, "groups_head_on_last_thread": 89, "pairs_from_2plus_groups":
                12658, "members_with_2plus_centres": 5937, "seqs_centre_and_member": 1244, "chains_of_three": 9326, "centre_is_id0": 99, "centre_is_last_id": 96,
                "no_entries": 12, "no_pairs": 38}


@pytest.fixture(scope="module")
def oracle():
    """{pattern: {(name, m): pairs}} by the oracle, once"""
    return {pat: {(name, m): LR.oracle_pairs(O, s3, pat, m) for name, s3, ms in LR.cases(pat) for m in ms} for pat in LR.PATTERNS}


@pytest.mark.parametrize("pattern", LR.PATTERNS, ids=LR.PATTERN_IDS)
def test_oracle_equals_the_restatement(oracle, pattern):
    ref = LR.reference(pattern)
    assert set(ref) == set(oracle[pattern])
    for key, (pr, _) in ref.items():
        got = oracle[pattern][key]
        assert got.shape == pr.shape and np.array_equal(got, pr), (key, got[:8].tolist(), pr[:8].tolist())


def test_oracle_lists_are_strictly_ascending_without_self_pairs(oracle):
    for pat in LR.PATTERNS:
        for key, pr in oracle[pat].items():
            k = pr[:, 0].astype(np.uint64) << np.uint64(32) | pr[:, 1].astype(np.uint64)
            assert (k[1:] > k[:-1]).all(), key
            assert (pr[:, 0] != pr[:, 1]).all(), key


def test_event_totals_are_pinned_and_none_is_missing():
    tot = dict.fromkeys(LR.EVENTS, 0)
    for pat in LR.PATTERNS:
        for _, ev in LR.reference(pat).values():
            for k, v in ev.items():
                tot[k] += int(v)
    assert all(v >= 1 for v in tot.values()), {k: v for k, v in tot.items() if v < 1}
    assert tot == EVENT_TOTALS, tot


def test_case_list_is_deterministic_and_within_the_length_limit():
    for pat in LR.PATTERNS:
        a, b = LR.cases(pat), LR.cases(pat)
        assert [c[0] for c in a] == [c[0] for c in b]
        for (_, x, _), (_, y, _) in zip(a, b):
            assert len(x) == len(y) and all(np.array_equal(u, v) and u.dtype == np.uint8 for u, v in zip(x, y))
            assert max(len(u) for u in x) <= LR.LMAX
        by = {c[0]: c for c in a}
        assert [len(by["n%d" % n][1]) for n in LR.SIZES] == list(LR.SIZES)
        assert max(len(u) for u in by["longest"][1]) == LR.LMAX and all(len(u) < LR.LMAX for u in by["combined"][1])
    assert 1000 in dict((c[0], c[2]) for c in LR.cases(LR.PATTERNS[0]))["longest"]
    assert sum(1000 in c[2] for pat in LR.PATTERNS for c in LR.cases(pat) if c[0] == "longest") == 1      # the million loop trips: one pattern only


@pytest.mark.parametrize("pattern", LR.PATTERNS, ids=LR.PATTERN_IDS)
def test_cases_hold_what_they_were_built_for(pattern):
    """per case, not only in the totals: the branch a case was built for is reached by that case"""
    ref = LR.reference(pattern)
    _, span = LR.offsets(pattern)
    # lengths: exactly m - 1, m, m + 1 k-mers for m = 5 and 20; 63 .. 129 candidates
    nc = sorted(len(LR.candidates(s, pattern)[0]) for s in dict((c[0], c[1]) for c in LR.cases(pattern))["lengths"])
    assert nc == [0, 0, 0, 1, 2, 4, 5, 6, 19, 20, 21, 63, 64, 65, 127, 128, 129]
    for m in (5, 20):
        ev = ref[("lengths", m)][1]
        assert ev["seq_exactly_m"] == 1 and ev["seq_no_kmer"] == 3 and ev["seq_fewer_than_m"] >= 1
    # the longest sequence: LMAX - span + 1 candidates
    longest = dict((c[0], c[1]) for c in LR.cases(pattern))["longest"][1]
    assert len(longest) == LR.LMAX and len(LR.candidates(longest, pattern)[0]) == LR.LMAX - span + 1
    assert all(len(ref[("longest", m)][0]) >= 1 for m in LR.MS)
    # X: dropped k-mers, survivors with an X under a `0` (where the pattern has one), and a pair at m = 1 that rests on such a survivor
    for m in LR.MS:
        ev = ref[("x", m)][1]
        assert ev["kmers_dropped_for_x"] >= 1 and ev["seq_no_kmer"] == 2
        if "0" in pattern:
            assert ev["picks_with_x_under_zero"] >= 1 and [2, 3] in ref[("x", m)][0].tolist()
        assert ref[("no_valid", m)][1]["no_entries"] == 1 and len(ref[("no_valid", m)][0]) == 0
    # repeats: m picks INCLUDING the repeat stop short of the partner's k-mer; the partner pairs up once m is larger
    assert [6, 7] not in ref[("repeats", 5)][0].tolist() and [6, 7] in ref[("repeats", 20)][0].tolist()
    assert [6, 8] not in ref[("repeats", 20)][0].tolist() and [6, 8] in ref[("repeats", 300)][0].tolist()
    assert all(ref[("repeats", m)][1]["seq_repeated_value_in_picks"] >= 1 for m in (5, 20, 300, 1000))
    # centre rule
    tot = {k: sum(ref[("centre", m)][1][k] for m in LR.MS) for k in LR.EVENTS}
    for k in ("groups_centre_first", "groups_centre_middle", "groups_centre_last", "groups_length_tie", "groups_all_lengths_equal", "centre_is_id0", "centre_is_last_id"):
        assert tot[k] >= 1, k
    # big groups: hundreds of entries, pairs made by many groups, and a head on the last thread of a block with its body in the next
    tot = {k: sum(ref[("big", m)][1][k] for m in LR.MS) for k in LR.EVENTS}
    for k in ("groups_over_256", "groups_cross_256", "groups_head_on_last_thread", "pairs_from_2plus_groups"):
        assert tot[k] >= 1, k
    assert ref[("big", 20)][1]["groups_head_on_last_thread"] >= 1 and ref[("big", 20)][1]["groups_over_256"] == 20      # at the default m, every group a big one
    # overlap
    tot = {k: sum(ref[("overlap", m)][1][k] for m in LR.MS) for k in LR.EVENTS}
    for k in ("members_with_2plus_centres", "seqs_centre_and_member", "chains_of_three"):
        assert tot[k] >= 1, k
    # database sizes: the centre n - 1 sets the top bit of the pair key
    for n in LR.SIZES[1:]:
        assert any(ref[("n%d" % n, m)][1]["centre_is_last_id"] for m in LR.MS), n
