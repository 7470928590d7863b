"""The first optimal column as the packed gapped kernels track it (one packed register: the age of the maximum) and the target letters of the
G = 16 / 32 classes (two columns per 32-bit load), against the scalar oracle, exact integers, through Engine.sw_pass raw and not raw:
tests/sw_firstcol_cases.py holds the cases (its module comment lists them and what each is there for) and the checks.

Every check runs twice: in this process, where the short lists of the (16, 12) class take the two-task variant (K = 2, asserted through
Engine.stats()), and in a child process with UC_SW_TASK_QUERIES=1, which the library reads once per process (K = 1 everywhere, asserted likewise)."""
import os
import subprocess
import sys

import pytest

import sw_firstcol_cases as FC
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import unicore_amd as U
    from oracle import oracle_py as O
    C = FC.build(O)
    Rf = FC.references(O, C)
    FC.cases_are_what_they_claim(C, Rf)
    return FC.engine(U, C), C, Rf


def test_forward_pass(run):
    FC.check_forward(*run)


def test_reversed_query_pass(run):
    FC.check_reversed_query(*run)


def test_start_pass(run):
    FC.check_start(*run)


def test_known_score_passes(run):
    FC.check_known(*run)


def test_two_task_variant_was_taken(run):
    """the same lists once more, counted: the (16, 12) class ran sw_pk_kernel<.., K = 2> in modes 0, 1, 4 and 6"""
    assert FC.check_all(*run) >= 4


def test_same_checks_with_one_task_per_workgroup(tmp_path):
    env = dict(os.environ, UC_ALLOW_SYNTHETIC="1", UC_SW_TASK_QUERIES="1")
    env.pop("UC_SW_TASK_SLOTS", None)
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, "tests", "sw_firstcol_cases.py"), str(tmp_path)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "multiquery_launches=0" in r.stdout, r.stdout[-500:]
