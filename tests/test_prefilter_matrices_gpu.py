"""The k-mer prefilter (uc_kmer_match.hip .. uc_hit_lists.hip and the driver uc_prefilter.hip, stages E1-E4) under matrices that reach +-48 and under every k-mer pattern of tests/linclust_ref.py:
Engine.prefilter() against the oracle's E1-E4 one query at a time (per-query counts, every hit in list order, the four stage counters - all
EQUAL), and for homopolymers against the closed form of spec UC-1 with the pattern's span.  Case builders: tests/matrix_cases.py; the preconditions
(how many k-mers of each case leave the 8-bit field the similar-k-mer search used to keep its bound in, which X variants leave a k-mer under which
pattern) are proven on the CPU in tests/test_matrix_cases.py.

Observed on the parent of the commit that adds this module (restpack of sim_runs_kernel in 8-bit fields biased by 64): test_matrices_beyond_the_
byte_field[hot] and [mixed_hot] are RED - under `hot` the device finds no similar k-mer at all (the bound 240 + 64 = 304 reads back as -16 and spills
into the next field), under `mixed_hot` it loses the k-mers rich in the hot letters; [negative] is green there: a negative biased value sets the bits
of every higher field, the bounds read back too LARGE, and a bound that is too large only prunes less.  With 10-bit fields biased by 256 all three
are green.  Of the five mutations recorded in tests/test_custom_matrices_gpu.py none turns a test of this module red (its matrices are symmetric and
its databases have no amino-acid track); the mutations recorded in tests/test_prefilter_kernels_gpu.py are the ones that bear on the pattern tests.
The whole module takes 4.1 s on an MI355X, oracle side included (13 tests, none above 0.5 s)."""
import numpy as np
import pytest

import linclust_ref as LR
import matrix_cases as MC
import prefilter_cases as PC
import util
from test_prefilter_kernels_gpu import _assert_equals_closed_form, _assert_equals_oracle, _assert_same_run

pytestmark = pytest.mark.gpu

PATTERN_PARAMS = pytest.mark.parametrize("pattern", LR.PATTERNS, ids=LR.PATTERN_IDS)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


# ---------------------------------------------------------------- matrices at the edge of [-48, 48]
@pytest.mark.parametrize("name", ["hot", "mixed_hot", "negative"])
def test_matrices_beyond_the_byte_field(O, tmp_path, name):
    """hot: every 3Di diagonal entry 48 - the best score five letters can still add is 240 for every k-mer, derived --k-score 283, every k-mer similar
    to itself only.  mixed_hot: eight diagonal entries 48 - 350 of the 1,755 k-mers that pass the threshold are beyond 191.  negative: ten letters
    whose whole rows are <= -25, derived --k-score -63 - 159 k-mers whose bound is below -64 pass the threshold and are similar to themselves."""
    _, _, mo = MC.write_case(O, name, tmp_path)
    s3 = MC.family_case_db()[0]
    opts = "-c 0.8 " + mo.split(" --mat-aa")[0]
    ref = PC.oracle_prefilter(O, s3, opts, key="matrix_" + name)
    assert ref["totals"]["n_prefilter_hits"] >= 80
    got = PC.run_engine(s3, opts)
    print(name, {k: got[2][k] for k in PC.COUNTERS}, ref["totals"])
    _assert_equals_oracle(got, ref)


def test_engine_after_a_refused_matrix(O, tmp_path):
    """a value of 49 is refused with the limit in the message, and the next engine of the process works"""
    import unicore_amd as U
    S3, _ = MC.matrices(O, "hot")
    S3[3, 3] = 49
    path = MC.write_matrix(str(tmp_path / "m49.out"), S3)
    with pytest.raises(U.UcError) as err:
        U.Engine("-c 0.8 --mat3di " + path, verbosity=1)
    assert err.value.code == U.UC_ERR_ARGS and "[-48,48]" in str(err.value)
    s3 = PC.hom([12, 15])
    cnt, _, _ = PC.run_engine(s3, "-c 0.8 --min-diag-hits 1 " + PC.ALL)
    assert cnt.tolist() == [2, 2]


# ---------------------------------------------------------------- k-mer patterns
def _opts(base, pattern):
    return base + " --spaced-kmer-pattern " + pattern


@PATTERN_PARAMS
def test_window_edge_sweep(O, pattern):
    """homopolymers of span - 1 (no k-mer), span (exactly one) and up to span + 29 residues: j + span <= len at every length, against the closed form
    with this span and against the oracle"""
    lengths = MC.pattern_sweep_lengths(len(pattern))
    opts = _opts("-c 0.8 --min-diag-hits 1 " + PC.ALL, pattern)
    got = PC.run_engine(PC.hom(lengths), opts)
    _assert_equals_closed_form(got, O, lengths, opts)
    _assert_equals_oracle(got, PC.oracle_prefilter(O, PC.hom(lengths), opts, key=("pattern_sweep", pattern)))
    assert got[0][0] == 0 and got[0][1] == len(lengths) - 1 and not (got[1]["target"] == 0).any()


@PATTERN_PARAMS
def test_x_residues(O, pattern):
    """the X variants rebuilt for the pattern: which k-mers stay valid depends on the offsets (every letter load of kmer_extract_kernel and
    query_kmer_at goes through koff)"""
    span = len(pattern)
    offs = [i for i, c in enumerate(pattern) if c == "1"]
    homs = [(MC.with_x_for(np.full(L, PC.HOM, np.uint8), v, pattern), v) for L in range(span + 2, min(span + 26, 51), 3) for v in MC.PATTERN_X_VARIANTS]
    reps = [(MC.with_x_for(s, v, pattern), v) for s in PC.tandem_repeats()[::6] for v in MC.PATTERN_X_VARIANTS]
    for tag, fam, base in (("hom", homs, "-c 0.8 --min-diag-hits 1 " + PC.ALL), ("rep", reps, PC.REPEAT_OPTS)):
        s3 = [s for s, _ in fam]
        opts = _opts(base, pattern)
        got = PC.run_engine(s3, opts)
        _assert_equals_oracle(got, PC.oracle_prefilter(O, s3, opts, key=("pattern_x", tag, pattern)))
        cnt, hits, _ = got
        dead = [i for i, s in enumerate(s3) if not PC.valid_kmer_positions(s, offs, span)]
        assert {i for i, (_, v) in enumerate(fam) if v == "x_none_valid"} <= set(dead)
        assert not np.isin(hits["target"], dead).any() and cnt[dead].sum() == 0
        assert all(cnt[i] > 0 for i in range(len(s3)) if i not in dead)


@PATTERN_PARAMS
def test_tandem_repeats(O, pattern):
    s3 = PC.tandem_repeats()
    opts = _opts(PC.REPEAT_OPTS, pattern)
    base = PC.run_engine(s3, opts)
    ref = PC.oracle_prefilter(O, s3, opts, key=("pattern_repeat", pattern))
    _assert_equals_oracle(base, ref)
    if pattern == LR.PATTERNS[0]:
        return                                  # the default pattern's chunked runs are test_prefilter_kernels_gpu.py's
    # >= 3 target chunks, as the mirrored upper triangle and as the full grid: fewer keys reach the sort under the triangle, so the chunks were taken
    sym = PC.run_engine(s3, opts, {"UC_PREFILTER_CHUNK_RES": PC.REPEAT_CHUNK_RES})
    full = PC.run_engine(s3, opts, {"UC_PREFILTER_CHUNK_RES": PC.REPEAT_CHUNK_RES, "UC_PREFILTER_SYMMETRIC": "0"})
    _assert_equals_oracle(sym, ref)
    _assert_same_run(sym, base)
    _assert_same_run(full, base)
    assert sym[2]["n_filtered_hits"] < full[2]["n_filtered_hits"]
    assert sum(len(x) for x in s3) >= 3 * int(PC.REPEAT_CHUNK_RES)
