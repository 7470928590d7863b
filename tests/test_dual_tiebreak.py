"""The property the shared known-score DP of mutual hits rests on (uc_sw_pk_impl.hpp key2, uc_align.hip amb_dual_kernel / sm_resolve_kernel):
with symmetric substitution matrices the DP of (t, q) is the transpose of the DP of (q, t), so what the spec reports for (t, q) - the
optimal cell in the first optimal column, then the first row - is the optimal cell of (q, t) in the first optimal ROW, then the first
column, with the roles swapped.  Checked against the scalar oracle's answers for both directions, forward pass and start pass, on random
pairs and on pairs built for tied optima (several optimal rows, several optimal columns, anti-ordered optimal cells).  CPU only."""
import numpy as np
import pytest

import dual_util as D
from test_sw_kernels import Dp, _mutate

LENGTHS = (1, 2, 3, 17, 32, 33, 64, 65, 97, 160, 200, 256, 300)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def cases(O):
    p = O.default_params()
    dp = Dp(p)
    assert np.array_equal(dp.S3, dp.S3.T) and np.array_equal(dp.SA, dp.SA.T)       # what the sharing assumes
    s3, sa, pairs, kinds = D.tie_pairs(7, LENGTHS, dp)
    rng = np.random.default_rng(11)
    kinds = list(kinds)
    for _ in range(60):                                                             # random pairs: unrelated, and homologues with indels
        L = int(rng.integers(1, 200))
        a = (rng.integers(0, 20, L, dtype=np.uint8), rng.integers(0, 20, L, dtype=np.uint8))
        b = _mutate(rng, a[0], a[1], 0.2) if rng.random() < 0.5 else (rng.integers(0, 20, L + 7, dtype=np.uint8), rng.integers(0, 20, L + 7, dtype=np.uint8))
        s3 += [a[0], np.ascontiguousarray(b[0])]; sa += [a[1], np.ascontiguousarray(b[1])]
        pairs.append((len(s3) - 2, len(s3) - 1)); kinds.append("random")
    return dict(O=O, p=p, dp=dp, s3=s3, sa=sa, pairs=pairs, kinds=np.array(kinds))


def test_second_answer_is_the_mirrors_first_answer(cases):
    C = cases
    O, p, dp, s3, sa = C["O"], C["p"], C["dp"], C["s3"], C["sa"]
    n_rows = n_cols = n_differ = n_start_rows = n_start_differ = 0
    for (q, t), kind in zip(C["pairs"], C["kinds"]):
        H, Hm = dp.H(s3[q], sa[q], s3[t], sa[t]), dp.H(s3[t], sa[t], s3[q], sa[q])
        assert np.array_equal(Hm, H.T), (q, t, kind)                                # the two DPs are transposes: same H in every cell
        f1, f2 = D.first_answer(H), D.second_answer(H)
        fwd = tuple(int(x) for x in O.sw(s3[q], sa[q], s3[t], sa[t], p))            # the oracle, both directions
        mir = tuple(int(x) for x in O.sw(s3[t], sa[t], s3[q], sa[q], p))
        assert f1 == fwd, (q, t, kind)
        assert (f2[0], f2[2], f2[1]) == mir, (q, t, kind, f2, mir)                  # second answer of (q, t), roles swapped = (t, q)'s answer
        assert D.second_answer(Hm) == (fwd[0], fwd[2], fwd[1]), (q, t, kind)        # and the other way round
        r, c = D.optimal_rows_cols(H)
        n_rows += r > 1; n_cols += c > 1; n_differ += f1 != f2
        if fwd[0] == 0:
            continue
        # start pass: (q, t) from its end cell (qe, te), the mirror from the transposed cell (te, qe) - the condition under which the
        # gapped stage shares the start pass (sm_flag_kernel)
        qe, te = fwd[1], fwd[2]
        a = D.start_reference(dp, s3, sa, q, t, qe, te)
        b = D.start_reference(dp, s3, sa, t, q, te, qe)
        so = tuple(int(x) for x in O.sw(s3[q][:qe + 1], sa[q][:qe + 1], s3[t][:te + 1], sa[t][:te + 1], p, rev_q=1, rev_t=1))
        sm = tuple(int(x) for x in O.sw(s3[t][:te + 1], sa[t][:te + 1], s3[q][:qe + 1], sa[q][:qe + 1], p, rev_q=1, rev_t=1))
        assert a["st1"] == so and b["st1"] == sm, (q, t, kind)
        assert so[0] == fwd[0] and sm[0] == fwd[0]                                  # the start pass reaches the forward optimum
        assert (a["st2"][0], a["st2"][2], a["st2"][1]) == sm, (q, t, kind, a, sm)
        assert (b["st2"][0], b["st2"][2], b["st2"][1]) == so, (q, t, kind, b, so)
        n_start_rows += a["srows"] > 1; n_start_differ += a["st1"] != a["st2"]
    # not vacuous: the inputs hold ties of every kind, among them pairs where the two orders pick different cells
    assert n_rows >= 30 and n_cols >= 30 and n_differ >= 10, (n_rows, n_cols, n_differ)
    assert n_start_rows >= 10 and n_start_differ >= 3, (n_start_rows, n_start_differ)


def test_tie_break_helpers_on_a_hand_made_matrix():
    H = np.array([[0, 5, 0, 0],
                  [0, 0, 0, 5],
                  [5, 0, 0, 0]], np.int32)
    assert D.first_answer(H) == (5, 2, 0)          # first optimal column 0, its first row 2
    assert D.second_answer(H) == (5, 0, 1)         # first optimal row 0, its first column 1
    assert D.optimal_rows_cols(H) == (3, 3)
    assert D.first_answer(H.T) == (5, 1, 0) and D.second_answer(H.T) == (5, 0, 2)
    assert D.first_answer(np.zeros((2, 2), np.int32)) == (0, -1, -1)
