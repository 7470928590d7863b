"""The reference side of the long-alignment tests (tests/long_aln_cases.py): the byte-per-cell traceback equals the oracle's traceback()
wherever both can run, every case reaches the event it is named for, and the fixture of the default-cost pairs belongs to the seeds."""
import json

import numpy as np
import pytest

import long_aln_cases as L
import util


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _mutated(rng, a3, aa):
    b3, ba = a3.copy(), aa.copy()
    m = rng.random(len(b3)) < 0.2; b3[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    m = rng.random(len(ba)) < 0.3; ba[m] = rng.integers(0, 20, int(m.sum()), dtype=np.uint8)
    for _ in range(int(rng.integers(0, 4))):
        if len(b3) < 8:
            break
        pos, w = int(rng.integers(1, len(b3) - 3)), int(rng.integers(1, 4))
        if rng.random() < 0.5:
            b3 = np.delete(b3, slice(pos, pos + w)); ba = np.delete(ba, slice(pos, pos + w))
        else:
            b3 = np.insert(b3, pos, rng.integers(0, 20, w, dtype=np.uint8)); ba = np.insert(ba, pos, rng.integers(0, 20, w, dtype=np.uint8))
    return b3, ba


def test_lean_traceback_equals_traceback_on_small_boxes(O):
    """720 random boxes under three gap-cost settings: length, identities and gaps equal traceback()'s; the tie mark, which traceback()
    does not have, equals the definition evaluated on plain numpy matrices of the box (some cell on the path where the walk turns into F
    also has H == E)"""
    rng = np.random.default_rng(2024)
    n = with_gaps = with_tie = 0
    for opts in ("", L.Z_OPTS, L.TIE_OPTS):
        p = L.params(O, opts)
        x, y, _ = L.tie_letters(p)
        for k in range(120):
            a3, aa = L._rnd(rng, int(rng.integers(4, 90)))
            b3, ba = _mutated(rng, a3, aa)
            if k % 3 == 0 and min(len(a3), len(b3)) > 12:          # a residue pair that costs more than two gap openings of 6
                pos = int(rng.integers(4, min(len(a3), len(b3)) - 4))
                a3[pos], aa[pos] = x
                b3[pos], ba[pos] = y
            odb = O.OracleDb(s3=[a3, b3], sa=[aa, ba])
            seqs = [(a3, aa), (b3, ba)]
            for q, t in ((0, 1), (1, 0)):
                s, qe, te = O.sw(*seqs[q], *seqs[t], p)
                if s <= 0:
                    continue
                qs, ts = int(rng.integers(0, qe + 1)), int(rng.integers(0, te + 1))     # any box is a valid input, not only an optimal one
                if k % 2 == 0:
                    _, dq, dt = O.sw(seqs[q][0][:qe + 1], seqs[q][1][:qe + 1], seqs[t][0][:te + 1], seqs[t][1][:te + 1], p, rev_q=1, rev_t=1)
                    qs, ts = qe - dq, te - dt
                want = O.traceback(odb, p, q, t, qs, qe, ts, te)
                got = O.traceback_lean(odb, p, q, t, qs, qe, ts, te)
                assert got[:3] == want, (opts, k, q, t)
                assert got[3] == _tie_by_definition(p, seqs[q], seqs[t], qs, qe, ts, te), (opts, k, q, t)
                n += 1; with_gaps += want[2] > 0; with_tie += got[3]
    assert n >= 300
    assert (n, with_gaps, with_tie) == PINNED, (n, with_gaps, with_tie)


PINNED = (720, 360, 24)     # boxes compared, with at least one gap, with the tie mark set


def _tie_by_definition(p, q, t, qs, qe, ts, te):
    S3 = np.array(p.S3[:], np.int64).reshape(21, 21); SA = np.array(p.SA[:], np.int64).reshape(21, 21)
    q3, qa, t3, ta = q[0][qs:qe + 1], q[1][qs:qe + 1], t[0][ts:te + 1], t[1][ts:te + 1]
    n, m, NEG = len(q3), len(t3), -(1 << 28)
    H = np.zeros((n + 1, m + 1), np.int64); E = np.full((n + 1, m + 1), NEG, np.int64); F = np.full((n + 1, m + 1), NEG, np.int64)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i, j] = max(E[i, j - 1] - p.gap_ext, H[i, j - 1] - p.gap_open)
            F[i, j] = max(F[i - 1, j] - p.gap_ext, H[i - 1, j] - p.gap_open)
            H[i, j] = max(0, H[i - 1, j - 1] + S3[q3[i - 1], t3[j - 1]] + SA[qa[i - 1], ta[j - 1]], E[i, j], F[i, j])
    i, j, state, tie = n, m, 0, 0
    while i > 0 and j > 0:
        if state == 0:
            if H[i, j] == 0:
                break
            if H[i, j] == H[i - 1, j - 1] + S3[q3[i - 1], t3[j - 1]] + SA[qa[i - 1], ta[j - 1]]:
                i -= 1; j -= 1
            elif H[i, j] == F[i, j]:
                tie |= int(H[i, j] == E[i, j]); state = 1
            else:
                state = 2
        elif state == 1:
            state = 0 if F[i, j] == H[i - 1, j] - p.gap_open else 1
            i -= 1
        else:
            state = 0 if E[i, j] == H[i, j - 1] - p.gap_open else 2
            j -= 1
    return tie


def _both(c):
    return [r for r, _ in c["ref"]], [tie for _, tie in c["ref"]]


@pytest.mark.parametrize("name,cols", [("z-walk-32767", L.LIMIT15 - 1), ("z-walk-32768", L.LIMIT15), ("z-long-32767", L.LIMIT15 - 1),
                                       ("z-long-32768", L.LIMIT15)])
def test_z_cases_reach_exactly_their_length(name, cols):
    """A.B against A.J.B under free extension: exactly `cols` columns in both orders, every query residue an identity, one gap, no tie; the
    swapped order's query has more rows than any systolic class, z-long's more than 2,048 in both orders"""
    c = L.z_case(name)
    recs, ties = _both(c)
    lq = len(c["q"][0])
    assert lq == (200 if "walk" in name else 2200) and len(c["t"][0]) == cols
    for r in recs:
        assert (r["aln_len"], r["idents"], r["gap_opens"]) == (cols, lq, 1)
    assert ties == [0, 0]
    assert (recs[0]["qend"] - recs[0]["qstart"] + 1, recs[0]["tend"] - recs[0]["tstart"] + 1) == (lq, cols)
    assert (recs[1]["qend"] - recs[1]["qstart"] + 1, recs[1]["tend"] - recs[1]["tstart"] + 1) == (cols, lq)


def test_z_wide_wraps_sixteen_bits_with_many_gaps_and_a_tie():
    c = L.z_case("z-wide")
    recs, ties = _both(c)
    assert (len(c["q"][0]), len(c["t"][0])) == (2100, 65535)
    for r in recs:
        assert r["aln_len"] >= L.LIMIT16 and r["gap_opens"] >= 100
    assert ties == [1, 1]
    assert (recs[0]["aln_len"], recs[0]["idents"]) != (recs[1]["aln_len"], recs[1]["idents"])      # a mirror may not copy its partner


def test_tie_cases_have_a_genuine_tie(O):
    p = L.params(O, L.TIE_OPTS)
    assert L.tie_letters(p)[2] < -2 * p.gap_open and p.gap_open == 6
    small, big = L.z_case("tie-small"), L.z_case("tie-z")
    for c in (small, big):
        recs, ties = _both(c)
        assert ties == [1, 1]
        assert all(r["gap_opens"] >= 2 for r in recs)              # the two single-residue gaps around x / y
    assert all(r["aln_len"] >= L.LIMIT15 for r in _both(big)[0])
    assert all(r["aln_len"] == len(small["q"][0]) + 1 for r in _both(small)[0])


def test_every_case_has_a_threshold_on_either_side():
    """the pipeline tests run each group under --min-seq-id values of which one accepts and one rejects every case"""
    for name in L.Z_CASES:
        for r in _both(L.z_case(name))[0]:
            sid = L.seq_id(r)
            assert any(sid >= np.float32(x) for x in L.seq_ids_of(name)) and any(sid < np.float32(x) for x in L.seq_ids_of(name)), (name, sid)


def test_fixture_belongs_to_the_seeds():
    fx = json.load(open(L.FIXTURE))
    assert set(fx["cases"]) == set(L.NAT_CASES) and fx["fields"] == list(L.FIELDS) and fx["min_seq_ids"] == list(L.NAT_SEQ_IDS)
    for name, c in L.NAT_CASES.items():
        f = fx["cases"][name]
        q, t = L.nat_sequences(name)
        assert (f["seed"], f["n"], f["len_q"], f["len_t"]) == (c["seed"], c["n"], len(q[0]), len(t[0]))
        assert (f["sha256_q"], f["sha256_t"]) == (L.sha(q), L.sha(t))
        assert L.nat_case(name)["ref"][0][0] == f["records"][0]


@pytest.mark.parametrize("name,n", [("nat-32767", L.LIMIT15 - 1), ("nat-32768", L.LIMIT15)])
def test_identical_nat_pairs_have_the_closed_form(O, name, n):
    """a sequence against its copy: the diagonal, all of it (every diagonal score of the matrices is positive: asserted)"""
    p = L.params(O, L.NAT_OPTS)
    assert all(p.S3[a * 21 + a] + p.SA[b * 21 + b] > 0 for a in range(20) for b in range(20))
    c = L.nat_case(name)
    q = c["q"]
    S3 = np.array(p.S3[:], np.int64).reshape(21, 21); SA = np.array(p.SA[:], np.int64).reshape(21, 21)
    score = int(S3[q[0], q[0]].sum() + SA[q[1], q[1]].sum())
    for r, tie in c["ref"]:
        assert (r["aln_len"], r["idents"], r["gap_opens"], tie) == (n, n, 0, 0)
        assert (r["qstart"], r["qend"], r["tstart"], r["tend"]) == (0, n - 1, 0, n - 1)
        assert r["score"] == score and r["accepted"] == 1


def test_mutated_nat_pair_lies_between_the_thresholds():
    c = L.nat_case("nat-mutated")
    lo, hi = (np.float32(x) for x in L.NAT_SEQ_IDS)
    for r, _ in c["ref"]:
        assert r["aln_len"] >= L.LIMIT15 and r["gap_opens"] >= 50
        assert lo < L.seq_id(r) < hi
