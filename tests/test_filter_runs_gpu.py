"""filter_kernel and expand_kernel (uc_kmer_filter.hip) read a query's runs from the plan of its super-batch: Engine.prefilter() on the cases of
tests/filter_runs_cases.py against the oracle's E1-E4 - per-query counts, target / score / diag of every hit in list order and the four stage
counters must be EQUAL - and, where a case runs under a non-default environment, against the default-environment run of the same case (byte-identical
hit arrays).  The preconditions that make each case reach its path are proven on the CPU in tests/test_filter_runs_cases.py.  The comparisons are
those of tests/test_prefilter_kernels_gpu.py.  The whole module takes a few seconds on an MI355X, oracle side included."""
import numpy as np
import pytest

import filter_runs_cases as FC
import prefilter_cases as PC
from test_prefilter_kernels_gpu import _assert_equals_closed_form, _assert_equals_oracle, _assert_same_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


_RUNS = {}


def _default_run(key, s3, opts):
    """the engine's run of a case under the default environment, once per session"""
    if (key, opts) not in _RUNS:
        _RUNS[(key, opts)] = PC.run_engine(s3, opts)
    return _RUNS[(key, opts)]


def test_a_run_list_across_a_tile_boundary(O):
    """A: the long query's 6,402 runs take four tiles, and run 2,048 lies inside the list of position 93"""
    s3 = FC.case_a(O)
    _assert_equals_oracle(_default_run("fr_a", s3, FC.OPTS), PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_a"))


@pytest.mark.parametrize("env", [None, {"UC_HIT_CAP": "1048576"}], ids=["default", "hit_cap_floor"])
def test_b_one_list_shared_by_every_position(O, env):
    """B: homopolymers - every position of every query points at the same run list; the long one has 2,091 runs in two tiles and 2,100 positions, of
    which a workgroup holds every fourth prefix (the search goes on in d_cumr).  At the floor of UC_HIT_CAP it is a batch of its own behind three
    queries"""
    s3 = FC.case_b()
    base = _default_run("fr_b", s3, FC.OPTS)
    got = base if env is None else PC.run_engine(s3, FC.OPTS, env)
    _assert_equals_closed_form(got, O, FC.B_LENGTHS, FC.OPTS)
    _assert_equals_oracle(got, PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_b"))
    _assert_same_run(got, base)


@pytest.mark.parametrize("opts", [FC.OPTS, FC.OPTS_PLAIN], ids=["double_hit_filter", "min_diag_hits_1"])
def test_c_positions_and_queries_without_runs(O, opts):
    """C: zero-run positions at the start, in the middle (a stretch longer than a k-mer's span) and at the end of a query's range are skipped, and a
    query without any run takes nothing from its neighbours' ranges"""
    s3 = FC.case_c(O)
    got = PC.run_engine(s3, opts)
    _assert_equals_oracle(got, PC.oracle_prefilter(O, s3, opts, key="fr_c"))
    assert got[0][FC.C_DEAD] == 0 and not (got[1]["target"] == FC.C_DEAD).any()


@pytest.mark.parametrize("env", [{"UC_HIT_CAP": "1048576"}, {"UC_DRUN_MAX": "8"}], ids=["hit_cap_floor", "drun_max"])
def test_d_batches_and_super_batches_behind_the_first_position(O, env):
    """D: several exact batches (a batch starts behind its super-batch's first position) and several super-batches (a plan starts behind position 0)"""
    s3 = FC.case_d(O)
    base = _default_run("fr_d", s3, FC.OPTS)
    _assert_equals_oracle(base, PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_d"))
    _assert_same_run(PC.run_engine(s3, FC.OPTS, env), base)


def test_e_plain_expansion(O):
    """E: --min-diag-hits 1 - expand_kernel finds a run's position by a search in the batch's run prefix"""
    s3 = FC.case_a(O)
    got = PC.run_engine(s3, FC.OPTS_PLAIN)
    _assert_equals_oracle(got, PC.oracle_prefilter(O, s3, FC.OPTS_PLAIN, key="fr_a"))
    assert got[2]["n_filtered_hits"] == got[2]["n_kmer_hits"]


def test_e_wide_keys(O):
    """E: UC_PREFILTER_WIDE=1 - filter_kernel<false>"""
    s3 = FC.case_a(O)
    got = PC.run_engine(s3, FC.OPTS, {"UC_PREFILTER_WIDE": "1"})
    _assert_equals_oracle(got, PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_a"))
    _assert_same_run(got, _default_run("fr_a", s3, FC.OPTS))


def test_e_two_target_chunks(O):
    """E: two target chunks - the second pass matches only the queries from its chunk on and mirrors the rest, its index is chunk-relative.  That the
    two chunks were really taken shows in fewer keys reaching the sort than under the full grid"""
    s3 = FC.case_a(O)
    ref = PC.oracle_prefilter(O, s3, FC.OPTS, key="fr_a")
    sym = PC.run_engine(s3, FC.OPTS, {"UC_PREFILTER_CHUNK_RES": FC.A_CHUNK_RES})
    full = PC.run_engine(s3, FC.OPTS, {"UC_PREFILTER_CHUNK_RES": FC.A_CHUNK_RES, "UC_PREFILTER_SYMMETRIC": "0"})
    for got in (sym, full):
        _assert_equals_oracle(got, ref)
        _assert_same_run(got, _default_run("fr_a", s3, FC.OPTS))
    assert sym[2]["n_filtered_hits"] < full[2]["n_filtered_hits"]
