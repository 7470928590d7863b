"""Rule UC-1/G (--cluster-mode 2, greedy incremental) without a GPU: the option parser, the host variant (uc_cluster_graph) against known
answers, the Python reference (greedy_incremental_ref.py) and the rule's properties, and the committed fixture tests/golden/clust_mode2.tsv."""
import os
import sys

import numpy as np
import pytest

import cluster_mode2_cases as K
import util
from greedy_incremental_ref import greedy_incremental

GOLD = os.path.join(util.ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


def test_parser_accepts_0_2_3_and_refuses_the_rest(U):
    for ok in ("--cluster-mode 0", "--cluster-mode 2", "--cluster-mode 3", "-c 0.8 --cluster-mode 2 --cov-mode 1", "--single-step-clustering --cluster-mode 2"):
        assert U.check_options(ok) == 0, ok
    for bad in ("--cluster-mode 1", "--cluster-mode 4", "--cluster-mode -1", "--cluster-mode x", "--cluster-mode"):
        assert U.check_options(bad) == U.UC_ERR_ARGS, bad
    assert U.check_options("--cluster-mode 4") == U.UC_ERR_ARGS
    msg = U.lib().uc_last_error().decode()
    assert "0" in msg and "2" in msg and "3" in msg and "unsupported" in msg, msg      # the error names the supported set
    assert U.lib().uc_option_arity(b"--cluster-mode") == 1


def test_abi_9_exports_both_entries(U):
    assert U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "uc_cluster_graph" in U.SYMBOLS and "uc_engine_cluster_graph" in U.SYMBOLS
    assert hasattr(U.lib(), "uc_cluster_graph") and hasattr(U.lib(), "uc_engine_cluster_graph")
    hdr = open(os.path.join(util.ROOT, "include", "unicore_cluster.h")).read()
    assert "#define UC_ABI_VERSION 9" in hdr and "int uc_cluster_graph(" in hdr and "int uc_engine_cluster_graph(" in hdr


def test_known_answers(U):
    path = [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert U.cluster_graph(5, path, [7] * 5, 2).tolist() == [0, 0, 2, 2, 4]
    star = [(0, 1), (0, 2), (0, 3)]
    assert U.cluster_graph(4, star, [3, 9, 9, 9], 2).tolist() == [1, 1, 2, 3]        # the centre is shorter than its leaves: it joins the first of them
    assert U.cluster_graph(4, star, [9, 3, 3, 3], 2).tolist() == [0, 0, 0, 0]
    # self loops, duplicate pairs in both directions, the empty graph
    noisy = path + [(i, i) for i in range(5)] + [(b, a) for a, b in path] + path
    assert U.cluster_graph(5, noisy, [7] * 5, 2).tolist() == [0, 0, 2, 2, 4]
    assert U.cluster_graph(5, np.zeros((0, 2), np.uint32), [7] * 5, 2).tolist() == [0, 1, 2, 3, 4]
    assert U.cluster_graph(0, np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32), 2).tolist() == []
    # the longest sequence wins whatever its id; a tie goes to the smaller id
    assert U.cluster_graph(3, [(0, 1), (1, 2)], [5, 5, 9], 2).tolist() == [0, 2, 2]
    assert U.cluster_graph(3, [(0, 1), (1, 2)], [5, 9, 9], 2).tolist() == [1, 1, 1]


def test_bad_arguments(U):
    for ed in ([(0, 5)], [(5, 0)], [(0, 1), (1, 0xFFFFFFFF)]):
        with pytest.raises(U.UcError) as ei:
            U.cluster_graph(5, ed, [7] * 5, 2)
        assert ei.value.code == U.UC_ERR_ARGS
    for mode in (1, 3, -1, 7):
        with pytest.raises(U.UcError) as ei:
            U.cluster_graph(5, [(0, 1)], [7] * 5, mode)
        assert ei.value.code == U.UC_ERR_ARGS
    with pytest.raises(U.UcError) as ei:        # mode 2 ranks by length: no lengths, no answer
        U.cluster_graph(5, [(0, 1)], None, 2)
    assert ei.value.code == U.UC_ERR_ARGS
    assert U.cluster_graph(5, [(0, 1)], None, 0).tolist() == U.setcover(5, [(0, 1)]).tolist()


@pytest.mark.parametrize("n", K.SIZES)
def test_random_graphs_equal_the_reference(U, n):
    rng = np.random.default_rng(1000 + n)
    for tag, ed in K.shapes(n, rng).items():
        assert np.array_equal(U.cluster_graph(n, ed, None, 0), U.setcover(n, ed)), (n, tag, "mode 0 is the set cover")
        for pat in K.LENGTH_PATTERNS:
            ln = K.lengths(n, pat, rng)
            a = U.cluster_graph(n, ed, ln, 2)
            assert np.array_equal(a, greedy_incremental(n, ed, ln)), (n, tag, pat)
            K.check_properties(n, ed, ln, a, (n, tag, pat))
    if n >= 64:
        ed, ln = K.hub_chain(n), K.hub_chain_late_lengths(n)
        a = U.cluster_graph(n, ed, ln, 2)
        assert np.array_equal(a, greedy_incremental(n, ed, ln)), (n, "hub chain, late representative")
        K.check_properties(n, ed, ln, a, (n, "hub chain, late representative"))


def test_reference_knows_the_rule():
    """the reference itself against the answers written out by hand in the rule's statement"""
    assert greedy_incremental(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [7] * 5).tolist() == [0, 0, 2, 2, 4]
    assert greedy_incremental(4, [(0, 1), (0, 2), (0, 3)], [3, 9, 9, 9]).tolist() == [1, 1, 2, 3]
    # hub chain with late lengths: hub 48 (the shortest node) is adjacent to its leaves, representatives from the start, and to hub 32, a
    # representative that outranks them: it belongs to hub 32
    a = greedy_incremental(64, K.hub_chain(64), K.hub_chain_late_lengths(64))
    assert a[48] == 32 and a[49] == 49 and a[32] == 32 and a[16] == 0


def test_committed_fixture_on_the_golden_database(U, tmp_path):
    """tests/golden/clust_mode2.tsv (make_clust_mode2.py: the oracle's accepted pairs -> the Python reference -> the oracle's write_tsv):
    the generator still reproduces it, the host variant reproduces it from the same pairs, it satisfies the consumer contract, and it is
    not the set cover's answer"""
    from oracle import oracle_py as O
    sys.path.insert(0, GOLD)
    try:
        import make_clust_mode2 as G
    finally:
        sys.path.remove(GOLD)
    odb = O.OracleDb(os.path.join(GOLD, "db"))
    edges, lens = G.oracle_accepted_pairs(odb)
    want = open(os.path.join(GOLD, "clust_mode2.tsv"), "rb").read()
    for name, assign in (("ref", greedy_incremental(odb.n, edges, lens)), ("host", U.cluster_graph(odb.n, edges, lens, 2))):
        O.write_tsv(str(tmp_path / (name + ".tsv")), odb, assign)
        assert open(tmp_path / (name + ".tsv"), "rb").read() == want, name
        K.check_properties(odb.n, edges, lens, assign, name)
    names = [l.split("\t")[1] for l in open(os.path.join(GOLD, "db.lookup"))]
    util.tsv_invariants(os.path.join(GOLD, "clust_mode2.tsv"), names)
    assert want != open(os.path.join(GOLD, "clust_default.tsv"), "rb").read()
