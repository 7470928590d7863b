"""Rule UC-1/X (--prefilter-mode 1), the part that needs no GPU: the option parser and the numpy restatement of E3x
(tests/ungapped_all_ref.py, the reference of the GPU tests) against the oracle's per-diagonal score."""
import numpy as np
import pytest

import ungapped_all_ref as R
import util

UC_ERR_ARGS = 2


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    oracle_py.lib()
    return oracle_py


def test_option_parser_knows_prefilter_mode():
    import unicore_amd as U
    L = U.lib()
    assert L.uc_option_arity(b"--prefilter-mode") == 1
    for ok in ("--prefilter-mode 0", "--prefilter-mode 1", "-c 0.8 --prefilter-mode 1 --single-step-clustering", "--prefilter-mode 1 --k-score 90 --min-diag-hits 3 -s 7.5"):
        assert U.check_options(ok) == 0, (ok, L.uc_last_error())
    for bad in ("--prefilter-mode 2", "--prefilter-mode -1", "--prefilter-mode", "--prefilter-mode 3", "--prefilter-mode x"):
        assert U.check_options(bad) == UC_ERR_ARGS, bad
        assert b"--prefilter-mode" in L.uc_last_error(), bad
    assert U.check_options("--gpu 1") == UC_ERR_ARGS                      # out of scope: still unknown


@pytest.mark.parametrize("opts", ["", "--comp-bias-corr 1", "--comp-bias-corr 1 --comp-bias-corr-scale 2.5"])
def test_restatement_against_the_oracle_per_diagonal(O, opts):
    """score = max over ALL diagonals of the oracle's E3 score, diag = the smallest diagonal reaching it; checked exhaustively on small pairs and on a
    random sample of (q, t, d) - both ends of the diagonal range included - on the test database of the GPU suite"""
    p = util.oracle_params(O, opts)
    s3, _, info = R.mode1_db()
    S = R.matrix(p)
    rng = np.random.default_rng(5)
    queries = [info["short"], info["periodic"][0], info["identical"][0], 6, 8, 11, 12, 20, 40, 63]
    targets = list(range(1, 128))
    n_samples = n_full = 0
    for q in queries:
        bias = R.comp_bias(O, s3[q], p)
        if not opts:
            assert not bias.any()
        sc, dg = R.e3x(s3[q], bias, [s3[t] for t in targets], S)
        lq = len(s3[q])
        for k, t in enumerate(targets):
            lt = len(s3[t])
            if lt == 0:                                                              # an empty target: no diagonal, score 0, diag 0
                assert sc[k] == 0 and dg[k] == 0
                continue
            u = lambda d: R.oracle_ungapped_bias(O, s3[q], s3[t], d, p, bias)
            lo, hi = -(lt - 1), lq - 1
            assert lo <= dg[k] <= hi
            assert u(int(dg[k])) == sc[k], (q, t)                                    # the reported diagonal has the reported score
            if lq * lt <= 2000 or (q, t) in ((info["periodic"][0], info["periodic"][1]), (info["identical"][0], info["identical"][1])):
                all_u = [u(d) for d in range(lo, hi + 1)]                            # every diagonal of the pair
                assert sc[k] == max(all_u) and dg[k] == lo + all_u.index(max(all_u)), (q, t)
                n_full += 1
            else:
                for d in {lo, hi, *rng.integers(lo, hi + 1, 3).tolist()}:            # both ends + random ones: none beats the maximum, none before diag reaches it
                    v = u(int(d))
                    assert v <= sc[k] and (v < sc[k] or d >= dg[k]), (q, t, d)
                    n_samples += 1
    assert n_samples >= 300 and n_full >= 100
    z = info["empty"]                                                                # ... and an empty query
    sc, dg = R.e3x(s3[z], R.comp_bias(O, s3[z], p), [s3[t] for t in targets], S)
    assert len(s3[z]) == 0 and z in targets and not sc.any() and not dg.any()
    # the tie rule is exercised: the periodic pair reaches the cap on several diagonals
    a, b = info["periodic"]
    bias = R.comp_bias(O, s3[a], p)
    capped = [d for d in range(-(len(s3[b]) - 1), len(s3[a])) if R.oracle_ungapped_bias(O, s3[a], s3[b], d, p, bias) == 255]
    sc, dg = R.e3x(s3[a], bias, [s3[b]], S)
    assert len(capped) >= 3 and sc[0] == 255 and dg[0] == capped[0]


def test_restatement_long_sequence(O):
    """the ~5,000-residue sequence as query and as target (its own group of the restatement)"""
    p = util.oracle_params(O, "")
    s3, _, info = R.mode1_db()
    S = R.matrix(p)
    L = info["long"]
    rng = np.random.default_rng(9)
    for q, t in ((L, 20), (20, L), (info["short"], L)):
        bias = R.comp_bias(O, s3[q], p)
        sc, dg = R.e3x(s3[q], bias, [s3[t]], S)
        assert O.ungapped(s3[q], s3[t], int(dg[0]), p) == sc[0]
        lo, hi = -(len(s3[t]) - 1), len(s3[q]) - 1
        for d in [lo, hi] + rng.integers(lo, hi + 1, 40).tolist():
            v = O.ungapped(s3[q], s3[t], int(d), p)
            assert v <= sc[0] and (v < sc[0] or d >= dg[0])
