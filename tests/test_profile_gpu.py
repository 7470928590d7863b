"""Rule UC-P (`unicore profile`) on the GPU: the device counter (uc_profile_count_dev, uc_profile.hip) == the host counter == the Python
reference (profile_ref.py), exactly, on every output array, at the smallest shapes at which each kernel can still be wrong; and the module end
to end behind `cluster` and `search`, through the C ABI and through bin/unicore."""
import os
import subprocess
import sys

import numpy as np
import pytest

import profile_ref as R
import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
EXE = os.path.join(util.ROOT, "bin", "unicore")
KEYS = ("single", "multiple", "core", "full", "core_off", "core_gene", "core_species")
NO = R.NO_GENE


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


def same(a, b, what=""):
    for k in KEYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, a[k][:20], b[k][:20])


def three_way(U, group, gene, n_groups, sp_off, sp, n_species, threshold, what=""):
    """device == host counter == Python reference; returns the device's outputs"""
    dev = U.profile_count(group, gene, n_groups, sp_off, sp, n_species, threshold, device=-1)
    host = U.profile_count(group, gene, n_groups, sp_off, sp, n_species, threshold)
    same(dev, host, (what, "device vs host"))
    same(dev, R.count(group, gene, n_groups, sp_off, sp, n_species, threshold), (what, "device vs reference"))
    return dev


def groups_of(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)


def one_species_each(n_genes, n_species):
    """gene g -> species g mod n_species"""
    return np.arange(n_genes + 1, dtype=np.uint64), (np.arange(n_genes) % n_species).astype(np.uint32)


# ---- random cases

def random_case(seed):
    rng = np.random.default_rng(seed)
    n_species = int(rng.integers(7, 71))
    n_genes = 1500
    per_gene = rng.integers(1, 4, n_genes)
    sp_off = np.zeros(n_genes + 1, np.uint64)
    sp_off[1:] = np.cumsum(per_gene)
    sp = np.concatenate([np.sort(rng.choice(n_species, k, replace=False)) for k in per_gene]).astype(np.uint32)
    sizes = rng.integers(1, 41, 300)
    sizes[int(rng.integers(0, 300))] = 3000
    group = groups_of(sizes)
    gene = rng.integers(0, n_genes, len(group)).astype(np.uint32)
    dup = np.flatnonzero((rng.random(len(group)) < 0.02) & (np.r_[False, group[1:] == group[:-1]]))
    gene[dup] = gene[dup - 1]                            # 2 % duplicated rows
    gene[rng.random(len(group)) < 0.05] = NO             # 5 % rows whose name is not in the map
    return group, gene, 300, sp_off, sp, n_species, int(rng.choice([0, 20, 50, 80, 100]))


def test_random_cases(U):
    seen_core = seen_multi = 0
    for seed in range(40):
        dev = three_way(U, *random_case(seed), what=seed)
        seen_core += int(dev["core"].sum())
        seen_multi += int((dev["single"] != dev["multiple"]).sum())
    assert seen_core > 100 and seen_multi > 1000      # the cases exercise both the file lines and the multi-copy species


# ---- wave and block edges

EDGE_SIZES = [63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("genes", ["same", "distinct", "last_differs"])
def test_runs_that_end_on_wave_and_block_edges(U, genes):
    """groups of 63 .. 257 rows back to back, one species: every (group, species) run ends on or beside a wave or workgroup edge"""
    group = groups_of(EDGE_SIZES)
    n = len(group)
    last = np.r_[group[1:] != group[:-1], True]
    gene = {"same": group.copy(), "distinct": np.arange(n, dtype=np.uint32), "last_differs": np.where(last, group + 6, group).astype(np.uint32)}[genes]
    sp_off, sp = one_species_each(n, 1)
    dev = three_way(U, group, gene, 6, sp_off, sp, 1, 0, genes)
    assert dev["multiple"].tolist() == [1] * 6 and dev["single"].tolist() == [0] * 6 and dev["core_off"][-1] == (6 if genes == "same" else 0)


def test_length_one_runs_across_the_edges(U):
    """the same groups with every row a different species: all runs have length 1"""
    group = groups_of(EDGE_SIZES)
    within = np.concatenate([np.arange(s) for s in EDGE_SIZES]).astype(np.uint32)
    sp_off, sp = one_species_each(257, 257)
    for threshold in (0, 25, 100):
        dev = three_way(U, group, within, 6, sp_off, sp, 257, threshold, threshold)
        assert dev["single"].tolist() == EDGE_SIZES == dev["multiple"].tolist()
    assert dev["core"].tolist() == [0, 0, 0, 0, 0, 1] and dev["core_off"][-1] == 257


# ---- one long run

def test_one_run_across_hundreds_of_workgroups(U):
    n = 200000
    group = np.zeros(n, np.uint32)
    sp_off, sp = one_species_each(4, 1)
    gene = np.full(n, 2, np.uint32)
    dev = three_way(U, group, gene, 1, sp_off, sp, 1, 0, "one gene")
    assert dev["core_gene"].tolist() == [2] and dev["single"].tolist() == [0] and dev["multiple"].tolist() == [1]
    gene[-1] = 3                                   # the "all genes equal" flag flips on the final element
    dev = three_way(U, group, gene, 1, sp_off, sp, 1, 0, "last differs")
    assert dev["core_gene"].tolist() == [] and dev["core"].tolist() == [1]
    sp_off3, sp3 = one_species_each(3, 3)
    three_way(U, group, (np.arange(n) % 3).astype(np.uint32), 1, sp_off3, sp3, 3, 0, "three species")
    both = np.array([0, 2, 5], np.uint64), np.array([0, 1, 0, 1, 2], np.uint32)      # gene 0 in species 0, 1; gene 1 in all three
    three_way(U, group, (np.arange(n) % 2).astype(np.uint32), 1, both[0], both[1], 3, 0, "genes in several species")


# ---- field width

def test_all_24_bits_of_the_group_field(U):
    """2^24 - 1 groups of one row, gene i -> species i mod 5: the expectation in closed form"""
    n = (1 << 24) - 1
    ids = np.arange(n, dtype=np.uint32)
    sp_off, sp = one_species_each(n, 5)
    threshold = 20      # single = 1 of S = 5: the largest threshold at which every group is core
    dev = U.profile_count(ids, ids, n, sp_off, sp, 5, threshold, device=-1)
    want = {"single": np.ones(n, np.uint32), "multiple": np.ones(n, np.uint32), "core": np.ones(n, np.uint8),
            "full": np.bincount(sp, minlength=5).astype(np.uint32), "core_off": np.arange(n + 1, dtype=np.uint64), "core_gene": ids, "core_species": sp}
    same(dev, want, "device")
    same(U.profile_count(ids, ids, n, sp_off, sp, 5, threshold), want, "host")


def test_all_24_bits_of_the_species_field(U):
    ns = (1 << 24) - 1
    sp_off, sp = np.array([0, 1, 2, 4], np.uint64), np.array([0, ns - 1, 0, ns - 1], np.uint32)      # lowest, highest, both
    group, gene = np.array([0, 0, 1, 1, 2, 3], np.uint32), np.array([0, 1, 2, 2, 1, NO], np.uint32)
    dev = three_way(U, group, gene, 4, sp_off, sp, ns, 0)
    assert dev["core_species"].tolist() == [0, ns - 1, 0, ns - 1, ns - 1] and dev["full"][0] == 1 and dev["full"][ns - 1] == 2 and int(dev["full"].sum()) == 3


def test_2_to_the_24_is_refused(U):
    one = np.zeros(1, np.uint32)
    for kw in (dict(n_groups=1 << 24), dict(n_species=1 << 24)):
        a = dict(dict(n_groups=1, n_species=1), **kw)
        with pytest.raises(U.UcError) as ei:
            U.profile_count(one, one, a["n_groups"], [0, 1], [0], a["n_species"], 80, device=-1)
        assert ei.value.code == U.UC_ERR_ARGS
    with pytest.raises(U.UcError) as ei:
        U.profile_count(one, [NO], 1, np.zeros((1 << 24) + 1, np.uint64), [], 1, 80, device=-1)
    assert ei.value.code == U.UC_ERR_ARGS
    for bad in (dict(group=[0, 1, 0], gene=[0, 0, 0], n_groups=2), dict(group=[0], gene=[7], n_groups=1)):
        with pytest.raises(U.UcError) as ei:
            U.profile_count(bad["group"], bad["gene"], bad["n_groups"], [0, 1], [0], 1, 80, device=-1)
        assert ei.value.code == U.UC_ERR_ARGS


# ---- empty input, boundary thresholds

def test_empty_inputs(U):
    e32 = np.zeros(0, np.uint32)
    sp_off, sp = one_species_each(3, 3)
    for threshold in (0, 80):
        dev = three_way(U, e32, e32, 0, sp_off, sp, 3, threshold, "no rows")
        assert dev["core_off"].tolist() == [0] and dev["full"].tolist() == [0, 0, 0]
        dev = three_way(U, groups_of([2, 1, 3]), np.full(6, NO, np.uint32), 3, sp_off, sp, 3, threshold, "unmapped only")
        assert dev["core"].tolist() == [int(threshold == 0)] * 3 and dev["single"].tolist() == [0, 0, 0] and dev["core_off"].tolist() == [0] * 4
    dev = three_way(U, e32, e32, 0, np.zeros(1, np.uint64), e32, 0, 80, "nothing at all")
    assert dev["full"].tolist() == []


@pytest.mark.parametrize("threshold,core", [(0, [1, 1]), (80, [1, 0]), (81, [0, 0]), (100, [0, 0])])
def test_boundary_thresholds(U, threshold, core):
    """5 species, single = 4: core at 80 and not at 81; beside it a group of unmapped rows"""
    sp_off, sp = one_species_each(5, 5)
    dev = three_way(U, groups_of([4, 2]), np.array([0, 1, 2, 3, NO, NO], np.uint32), 2, sp_off, sp, 5, threshold)
    assert dev["single"].tolist() == [4, 0] and dev["core"].tolist() == core


# ---- end to end

def dir_bytes(path):
    out = {}
    for n in sorted(os.listdir(path)):
        with open(os.path.join(path, n), "rb") as f:
            out[n] = f.read()
    return out


def host_run(db, tsv, out, threshold):
    code = "import sys, unicore_amd as U\nU.profile(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), verbosity=0)\n"
    r = subprocess.run([sys.executable, "-c", code, db, tsv, out, str(threshold)], env=dict(os.environ, UC_PROFILE_HOST="1", PYTHONPATH=util.ROOT),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def check_against_reference_and_host(db, tsv, out, threshold, tmp_path):
    with open(db + ".map", "rb") as f:
        m = f.read()
    with open(tsv, "rb") as f:
        t = f.read()
    ref = R.profile_text(m, t, threshold)
    got = dir_bytes(out)
    assert got == ref["files"]
    host_out = str(tmp_path / ("host_%s" % os.path.basename(out)))
    host_run(db, tsv, host_out, threshold)
    assert got == dir_bytes(host_out)
    return ref


def run(argv):
    env = {k: v for k, v in os.environ.items() if k != "UC_PROFILE_HOST"}
    r = subprocess.run(argv, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (argv, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def test_cluster_then_profile_through_the_c_abi(U, tmp_path, monkeypatch):
    monkeypatch.delenv("UC_PROFILE_HOST", raising=False)
    db = os.path.join(GOLD, "db")
    cdb, tsv, out = str(tmp_path / "clust_cluster"), str(tmp_path / "clust.tsv"), str(tmp_path / "prof")
    U.cluster(db, cdb, str(tmp_path / "tmp"), "-c 0.8")
    U.createtsv(db, cdb, tsv)
    U.profile(db, tsv, out, 80, verbosity=0, device=0)
    ref = check_against_reference_and_host(db, tsv, out, 80, tmp_path)
    with open(os.path.join(GOLD, "clust_linclust_cascade3.tsv"), "rb") as f, open(tsv, "rb") as g:
        assert f.read() == g.read()      # the default workflow's committed clustering: the profile is of that file
    assert len(ref["groups"]) >= 1


def test_cluster_then_profile_through_the_cli(tmp_path):
    db = os.path.join(GOLD, "db")
    out, prof = str(tmp_path / "res" / "clust"), str(tmp_path / "res" / "prof")
    run([EXE, "cluster", db, out, str(tmp_path / "tmp"), "--threads", "4"])
    r = run([EXE, "profile", db, out + ".tsv", prof])
    ref = check_against_reference_and_host(db, out + ".tsv", prof, 80, tmp_path)
    assert "%d structural core genes found from %d candidates" % (ref["n_core"], len(ref["groups"])) in r.stdout
    r = run([EXE, "profile", "-t", "50", "-v", "2", db, out + ".tsv", prof + "50"])
    assert r.stdout == ""
    ref50 = check_against_reference_and_host(db, out + ".tsv", prof + "50", 50, tmp_path)
    assert r.stderr.splitlines() == ref50["warnings"] and ref50["n_core"] >= ref["n_core"]


def test_search_then_profile_through_the_cli(tmp_path):
    db = os.path.join(GOLD, "db")
    out, prof = str(tmp_path / "res" / "OUTPUT"), str(tmp_path / "prof")
    run([EXE, "search", db, db, out, str(tmp_path / "tmp"), "--threads", "4", "-k"])
    with open(out + ".m8") as f:
        assert len(f.readline().split("\t")) == 12
    run([EXE, "profile", db, out + ".m8", prof])
    ref = check_against_reference_and_host(db, out + ".m8", prof, 80, tmp_path)
    assert len(ref["groups"]) >= 1
