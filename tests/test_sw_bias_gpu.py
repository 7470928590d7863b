"""The packed gapped kernels in the biased score domain (uc_sw_pk_impl.hpp: H' = H + 128, E' = E + 128 in every mode but 7) against the scalar
oracle, exact integers, through Engine.sw_pass raw and not raw: tests/sw_bias_cases.py holds the cases (the smallest shapes that can break the
domain: its module comment lists them) and the checks.  Matrices at the option limit of +-48 per track, gap open 31 (the widest) and 1 (the
narrowest the options take: --gap-open 0 is rejected, so the open-0 recurrence is checked on the CPU only, tests/test_sw_bias_model.py).

Every check runs twice: in this process, where the short lists of the G = 16 classes take the two-task variant (K = 2, asserted through
Engine.stats()), and in a child process with UC_SW_TASK_QUERIES=1, which the library reads once per process (K = 1 everywhere, asserted likewise)."""
import os
import subprocess
import sys

import pytest

import sw_bias_cases as BC
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def cases(O, tmp_path_factory):
    return BC.build(O, tmp_path_factory.mktemp("sw_bias"))


@pytest.fixture(scope="module", params=BC.GAPS, ids=lambda g: "open%d_ext%d" % g)
def run(O, cases, request):
    import unicore_amd as U
    Rf = BC.references(O, cases, request.param)
    BC.cases_are_what_they_claim(cases, Rf)
    return BC.engine(U, cases, request.param), cases, Rf


def test_forward_pass(run):
    BC.check_forward(*run)


def test_reversed_query_pass(run):
    BC.check_reversed_query(*run)


def test_start_pass(run):
    BC.check_start(*run)


@pytest.mark.parametrize("tab", [1, 3])
def test_known_score_passes(run, tab):
    BC.check_known(*run, tab)


def test_two_task_variant_was_taken(run):
    """the same lists once more, counted: the G = 16 classes with R >= 4 ran sw_pk_kernel<.., K = 2> in modes 0, 1, 4 and 6"""
    assert BC.check_all(*run) >= 4


def test_same_checks_with_one_task_per_workgroup(tmp_path):
    env = dict(os.environ, UC_ALLOW_SYNTHETIC="1", UC_SW_TASK_QUERIES="1")
    env.pop("UC_SW_TASK_SLOTS", None)
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, "tests", "sw_bias_cases.py"), str(tmp_path)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "multiquery_launches=0" in r.stdout, r.stdout[-500:]
