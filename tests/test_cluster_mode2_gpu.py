"""Rule UC-1/G (--cluster-mode 2, greedy incremental) on the GPU: the device rounds (uc_greedy_inc.hip) against the Python reference
(greedy_incremental_ref.py) on every graph shape, at a size that spans many blocks and on a path that takes the host tail; then the
rule through every caller - uc_cluster's plain step, the default workflow round by round, two (virtual) ranks, and both CLIs."""
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_mode2_cases as K
import util
from greedy_incremental_ref import greedy_incremental

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
SHIM = os.path.join(util.ROOT, "bin", "foldseek")
EXE = os.path.join(util.ROOT, "bin", "unicore")
TIMING = re.compile(r"cluster_graph_device: greedy incremental on the GPU [0-9.]+ ms in (\d+) rounds(, the chain-like rest \((\d+) nodes\) on the host)?")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def db_of_lengths(e, lens):
    """the engine's database becomes len(lens) sequences of these lengths (the letters do not matter to the clustering rule)"""
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    z = np.zeros(int(off[-1]), np.uint8)
    e.set_db(off, z, z)


def accepted_pairs(eng):
    """(query, target) of every accepted alignment record of the engine's hit lists"""
    cnt, hits = eng.hits_range(0, eng.n)
    al = eng.alns_range(0, eng.n)
    q = np.repeat(np.arange(eng.n, dtype=np.uint32), cnt)
    acc = al["accepted"] == 1
    return np.stack([q[acc], hits["target"][acc].astype(np.uint32)], 1)


def test_device_rounds_equal_the_reference_on_every_shape():
    import unicore_amd as U
    e = U.Engine("-c 0.8", verbosity=1)
    rng = np.random.default_rng(2026)
    for n in K.SIZES:
        sh = K.shapes(n, rng)
        cases = [(pat, K.lengths(n, pat, rng), sh) for pat in K.LENGTH_PATTERNS]
        if n >= 64:      # a representative of lower rank that is decided in a later round than one of higher rank
            cases.append(("late", K.hub_chain_late_lengths(n), {"hub chain": K.hub_chain(n)}))
        for pat, ln, graphs in cases:
            db_of_lengths(e, ln)
            assert e.n == n
            for tag, ed in graphs.items():
                a = e.cluster_graph(ed, 2)
                assert np.array_equal(a, greedy_incremental(n, ed, ln)), (n, tag, pat)
                assert np.array_equal(a, U.cluster_graph(n, ed, ln, 2)), (n, tag, pat, "host variant")
                K.check_properties(n, ed, ln, a, (n, tag, pat))
                if pat == "equal":      # mode 0 through the new entry is the set cover
                    assert np.array_equal(e.cluster_graph(ed, 0), e.setcover(ed)), (n, tag)
                    assert np.array_equal(e.cluster_graph(ed, 0), U.setcover(n, ed)), (n, tag)
    e.close()


def test_bad_arguments_on_the_device():
    import unicore_amd as U
    e = U.Engine("-c 0.8", verbosity=1)
    db_of_lengths(e, [5] * 7)
    for mode in (1, 3, -1):
        with pytest.raises(U.UcError) as ei:
            e.cluster_graph([(0, 1)], mode)
        assert ei.value.code == U.UC_ERR_ARGS
    with pytest.raises(U.UcError) as ei:
        e.cluster_graph([(0, 7)], 2)
    assert ei.value.code == U.UC_ERR_ARGS
    assert e.cluster_graph([(0, 1), (3, 3)], 2).tolist() == [0, 0, 2, 3, 4, 5, 6]      # the engine is usable after the refusals
    e.close()


def test_a_graph_that_spans_many_blocks(capfd, monkeypatch):
    """2 x 10^5 nodes, 2 x 10^6 random edges, random lengths: 65,536 blocks of four waves do not cover the work list in one stride"""
    import unicore_amd as U
    n, m = 200_000, 2_000_000
    rng = np.random.default_rng(7)
    ln = rng.integers(1, 61, n).astype(np.uint32)
    ed = rng.integers(0, n, (m, 2)).astype(np.uint32)
    e = U.Engine("-c 0.8", verbosity=1)
    db_of_lengths(e, ln)
    monkeypatch.setenv("UC_TIMING", "1")
    capfd.readouterr()
    a = e.cluster_graph(ed, 2)
    err = capfd.readouterr().err
    monkeypatch.delenv("UC_TIMING")
    tm = TIMING.search(err)
    assert tm, err[-2000:]
    print("rounds:", tm.group(1), "host tail:", bool(tm.group(2)))
    assert int(tm.group(1)) > 1, tm.group(0)
    assert np.array_equal(a, greedy_incremental(n, ed, ln))
    assert np.array_equal(a, U.cluster_graph(n, ed, ln, 2))
    K.check_properties(n, ed, ln, a, "large")
    assert np.array_equal(e.cluster_graph(ed, 0), e.setcover(ed))
    e.close()


def test_an_equal_length_path_takes_the_host_tail(capfd, monkeypatch):
    """20,000 nodes of one length on a path: the ranks ascend along it, a round decides two nodes, and after 32 rounds the host finishes;
    the UC_TIMING line says so"""
    import unicore_amd as U
    n = 20_000
    ids = np.arange(n)
    ed = np.stack([ids[:-1], ids[1:]], 1).astype(np.uint32)
    ln = np.full(n, 5, np.uint32)
    e = U.Engine("-c 0.8", verbosity=1)
    db_of_lengths(e, ln)
    monkeypatch.setenv("UC_TIMING", "1")
    capfd.readouterr()
    a = e.cluster_graph(ed, 2)
    err = capfd.readouterr().err
    monkeypatch.delenv("UC_TIMING")
    tm = TIMING.search(err)
    assert tm and tm.group(2), err[-2000:]
    assert int(tm.group(1)) == 32 and int(tm.group(3)) == n - 64
    assert np.array_equal(a, (ids // 2 * 2).astype(np.uint32))
    assert np.array_equal(a, greedy_incremental(n, ed, ln))
    # the tail keeps the rank order of UNEQUAL lengths too: the path read backwards is the ascending chain when the lengths grow with the id
    ln2 = (1 + ids % 1000 + ids // 1000).astype(np.uint32)
    db_of_lengths(e, ln2)
    a2 = e.cluster_graph(ed, 2)
    assert np.array_equal(a2, greedy_incremental(n, ed, ln2))
    K.check_properties(n, ed, ln2, a2, "tail, unequal lengths")
    e.close()


def _cluster_tsv(U, db, d, tag, opts, num_gpus=1):
    st = U.cluster(db, os.path.join(d, tag + "_cluster"), os.path.join(d, "tmp"), opts, threads=4, num_gpus=num_gpus)
    U.createtsv(db, os.path.join(d, tag + "_cluster"), os.path.join(d, tag + ".tsv"))
    return open(os.path.join(d, tag + ".tsv"), "rb").read(), st


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mode2"))
    s3, sa = util.family_db(11, n_fam=14, members=7, extra=(500,))
    names = util.write_db(os.path.join(d, "db"), s3, sa)
    return dict(dir=d, prefix=os.path.join(d, "db"), s3=s3, sa=sa, names=names)


def test_plain_step_end_to_end(O, family, tmp_path):
    """uc_cluster --single-step-clustering --cluster-mode 2: clust.tsv == the engine's accepted pairs -> the reference -> the oracle's write_tsv,
    byte for byte; mode 3 is the same rule; on the golden database the committed fixture comes out"""
    import unicore_amd as U
    opts = "-c 0.8 --single-step-clustering --cluster-mode 2"
    got, st = _cluster_tsv(U, family["prefix"], family["dir"], "plain2", opts)
    e = U.Engine("-c 0.8", verbosity=1)
    e.load_db(family["prefix"])
    e.prefilter()
    e.align()
    ed = accepted_pairs(e)
    assert len(ed) == len(e.edges()) and len(ed) > 100
    ln = np.array([len(x) for x in family["s3"]], np.uint32)
    ref = greedy_incremental(e.n, ed, ln)
    assert np.array_equal(e.cluster_graph(ed, 2), ref)
    e.close()
    odb = O.OracleDb(family["prefix"])
    O.write_tsv(str(tmp_path / "ref.tsv"), odb, ref)
    assert got == open(tmp_path / "ref.tsv", "rb").read()
    assert st["n_clusters"] == int((ref == np.arange(len(ref))).sum())
    util.tsv_invariants(os.path.join(family["dir"], "plain2.tsv"), family["names"])
    got0, _ = _cluster_tsv(U, family["prefix"], family["dir"], "plain0", "-c 0.8 --single-step-clustering")
    assert got != got0, "the two rules agree on this database: it tests nothing"
    got3, _ = _cluster_tsv(U, family["prefix"], family["dir"], "plain3", "-c 0.8 --single-step-clustering --cluster-mode 3")
    assert got3 == got
    gold, _ = _cluster_tsv(U, os.path.join(GOLD, "db"), family["dir"], "gold2", opts)
    assert gold == open(os.path.join(GOLD, "clust_mode2.tsv"), "rb").read()


def test_default_workflow_round_by_round(O, family, tmp_path):
    """a bare "-c 0.8 --cluster-mode 2" runs the pre-step and the cascade with the rule in EVERY round: each round's accepted pairs
    (workflow observer) -> the reference with the round's lengths, composed as mergeclusters does, is the whole clust.tsv"""
    import unicore_amd as U
    rounds, errors = [], []

    def hook(rnd, ids, kthr, view):
        try:
            rounds.append((rnd, ids, accepted_pairs(view)))
        except Exception as ex:          # an exception cannot cross the C frame
            errors.append(ex)

    U.set_round_hook(hook)
    try:
        got, st = _cluster_tsv(U, family["prefix"], family["dir"], "wf2", "-c 0.8 --cluster-mode 2")
    finally:
        U.set_round_hook(None)
    if errors:
        raise errors[0]
    assert [r[0] for r in rounds] == [-1, 0, 1, 2]
    full_len = np.array([len(x) for x in family["s3"]], np.uint32)
    n = len(full_len)
    assign = np.arange(n, dtype=np.uint32)
    cur = np.arange(n, dtype=np.uint32)
    for rnd, ids, ed in rounds:
        assert np.array_equal(ids, cur), rnd          # the round runs on the representatives of the round before
        sa = greedy_incremental(len(ids), ed, full_len[ids])
        pos = np.zeros(n, np.int64)
        pos[ids] = np.arange(len(ids))
        assign = ids[sa[pos[assign]]]
        cur = ids[sa == np.arange(len(ids))]
    odb = O.OracleDb(family["prefix"])
    O.write_tsv(str(tmp_path / "ref.tsv"), odb, assign)
    assert got == open(tmp_path / "ref.tsv", "rb").read()
    assert st["n_clusters"] == len(cur)
    util.tsv_invariants(os.path.join(family["dir"], "wf2.tsv"), family["names"])
    got0, _ = _cluster_tsv(U, family["prefix"], family["dir"], "wf0", "-c 0.8")
    assert got != got0


def test_two_ranks_give_the_same_file(family, monkeypatch):
    import unicore_amd as U
    want = {}
    for tag, opts in (("s", "-c 0.8 --single-step-clustering --cluster-mode 2"), ("w", "-c 0.8 --cluster-mode 2")):
        want[tag], _ = _cluster_tsv(U, family["prefix"], family["dir"], tag + "1", opts)
    monkeypatch.setenv("UC_VIRTUAL_GPUS", "1")
    for tag, opts in (("s", "-c 0.8 --single-step-clustering --cluster-mode 2"), ("w", "-c 0.8 --cluster-mode 2")):
        got, st = _cluster_tsv(U, family["prefix"], family["dir"], tag + "2", opts, num_gpus=2)
        assert st["n_gpus"] == 2
        assert got == want[tag], tag
    # the staged step of the one-process-per-GPU layout dispatches too (one rank, no communicator)
    e = U.Engine("-c 0.8 --cluster-mode 2", verbosity=1)
    e.load_db(family["prefix"])
    a, _ = e.cluster_step()
    ed = e.edges()
    assert np.array_equal(a, greedy_incremental(e.n, ed, [len(x) for x in family["s3"]]))
    assert np.array_equal(e.setcover(ed), U.setcover(e.n, ed))      # the existing entry stays the set cover whatever the engine's options
    e.close()


def test_both_clis_need_nothing_but_the_parser(family, tmp_path):
    """`unicore cluster DB OUT TMP -c "-c 0.8 --cluster-mode 2"` and the foldseek shim with the reference's argv write the file uc_cluster writes"""
    import unicore_amd as U
    db = family["prefix"]
    want, _ = _cluster_tsv(U, db, family["dir"], "cli_ref", "-c 0.8 --cluster-mode 2")
    out = str(tmp_path / "u" / "clust")
    r = subprocess.run([EXE, "cluster", db, out, str(tmp_path / "tmp"), "-c", "-c 0.8 --cluster-mode 2", "--threads", "4"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert open(out + ".tsv", "rb").read() == want
    out = str(tmp_path / "f" / "clust")
    os.makedirs(os.path.dirname(out))
    for argv in ([SHIM, "cluster", "--threads", "4", "-v", "2", db, out + "_cluster", str(tmp_path / "ftmp"), "-c", "0.8", "--cluster-mode", "2"],
                 [SHIM, "createtsv", "--threads", "4", "-v", "2", db, db, out + "_cluster", out + ".tsv"]):
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, (argv, r.stdout[-2000:], r.stderr[-2000:])
    assert open(out + ".tsv", "rb").read() == want
    r = subprocess.run([EXE, "cluster", db, str(tmp_path / "x" / "clust"), str(tmp_path / "tmp"), "-c", "-c 0.8 --cluster-mode 1"], capture_output=True, text=True)
    assert r.returncode != 0          # connected component stays refused
