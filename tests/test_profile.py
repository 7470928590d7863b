"""Rule UC-P (`unicore profile`) without a GPU: the host counter (uc_profile_count) and the file level under UC_PROFILE_HOST=1 against the
Python reference (profile_ref.py), the committed fixture tests/golden/profile_default_t80.json, the CLI's parser, and the refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import profile_ref as R
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")
KEYS = ("single", "multiple", "core", "full", "core_off", "core_gene", "core_species")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


def read(path):
    with open(path, "rb") as f:
        return f.read()


def same(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, a[k][:20], b[k][:20])


def host_count(U, A, threshold):
    return U.profile_count(A["group"], A["gene"], A["n_groups"], A["sp_off"], A["sp"], A["n_species"], threshold)


def run_profile_host(db, tsv, out, threshold=80, verbosity=0):
    """uc_profile in a child process with UC_PROFILE_HOST=1: the switch is an environment variable"""
    code = ("import sys, unicore_amd as U\n"
            "U.profile(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), verbosity=int(sys.argv[5]))\n")
    env = dict(os.environ, UC_PROFILE_HOST="1", PYTHONPATH=util.ROOT)
    return subprocess.run([sys.executable, "-c", code, db, tsv, out, str(threshold), str(verbosity)], env=env, capture_output=True, text=True)


def dir_bytes(path):
    return {n: read(os.path.join(path, n)) for n in sorted(os.listdir(path))}


def write_case(tmp_path, map_text, tsv_text, tsv_name="clust.tsv"):
    db, tsv = str(tmp_path / "db"), str(tmp_path / tsv_name)
    with open(db + ".map", "wb") as f:
        f.write(map_text)
    with open(tsv, "wb") as f:
        f.write(tsv_text)
    return db, tsv


def check_files(tmp_path, map_text, tsv_text, threshold, tsv_name="clust.tsv"):
    db, tsv = write_case(tmp_path, map_text, tsv_text, tsv_name)
    out = str(tmp_path / ("out_%d" % threshold))
    r = run_profile_host(db, tsv, out, threshold)
    assert r.returncode == 0, r.stderr
    ref = R.profile_text(map_text, tsv_text, threshold)
    assert dir_bytes(out) == ref["files"]
    return ref


# ---- goldens

@pytest.mark.parametrize("case,threshold,n_groups,n_core", [("", 0, 42, 42), ("", 50, 42, 13), ("", 80, 42, 11), ("", 100, 42, 3), ("c1", 80, 160, 1)])
def test_goldens_host_counter_equals_reference(U, case, threshold, n_groups, n_core):
    m = read(os.path.join(GOLD, case, "db.map"))
    t = read(os.path.join(GOLD, case, "clust_workflow.tsv" if case else "clust_default.tsv"))
    A = R.arrays(m, t)
    got, ref = host_count(U, A, threshold), R.count(A["group"], A["gene"], A["n_groups"], A["sp_off"], A["sp"], A["n_species"], threshold)
    same(got, ref, (case, threshold))
    txt = R.profile_text(m, t, threshold)
    assert A["n_groups"] == n_groups == len(txt["groups"]) and int(got["core"].sum()) == n_core == txt["n_core"]
    assert [(int(s), int(mu), bool(c)) for s, mu, c in zip(got["single"], got["multiple"], got["core"])] == [g[1:] for g in txt["groups"]]
    if not case:
        assert A["n_species"] == 5 and int((got["multiple"] != got["single"]).sum()) == 3
        assert len(m.splitlines()) == len(A["gene_names"]) == len(A["sp"]) == 91      # every gene of this map has one line and one species


def test_golden_directory_byte_for_byte(tmp_path):
    with open(os.path.join(GOLD, "profile_default_t80.json")) as f:
        want = {k: v.encode("ascii") for k, v in json.load(f).items()}
    out = str(tmp_path / "out")
    r = run_profile_host(os.path.join(GOLD, "db"), os.path.join(GOLD, "clust_default.tsv"), out, 80)
    assert r.returncode == 0, r.stderr
    assert dir_bytes(out) == want
    assert want == R.profile_text(read(os.path.join(GOLD, "db.map")), read(os.path.join(GOLD, "clust_default.tsv")), 80)["files"]
    assert len(want) == 13 and want["profile.chk"] == b"1"


# ---- the boundary of the core test

BOUNDARY_MAP = b"".join(b"g%d\tsp%d\n" % (k, k) for k in range(5)) + b"h0\tsp0\n"
BOUNDARY_TSV = b"".join(b"q\tg%d\n" % k for k in range(4)) + b"r\tzz\nr\tyy\n"      # q: single = 4 of 5; r: only unmapped rows


def test_core_boundary(U, tmp_path):
    A = R.arrays(BOUNDARY_MAP, BOUNDARY_TSV)
    for threshold, q_core, r_core in ((0, 1, 1), (80, 1, 0), (81, 0, 0), (100, 0, 0)):
        got = host_count(U, A, threshold)
        same(got, R.count(A["group"], A["gene"], A["n_groups"], A["sp_off"], A["sp"], A["n_species"], threshold), threshold)
        assert got["single"].tolist() == [4, 0] and got["core"].tolist() == [q_core, r_core], threshold
    ref = check_files(tmp_path, BOUNDARY_MAP, BOUNDARY_TSV, 0)
    assert ref["files"]["r.txt"] == b"" and ref["files"]["q.txt"] == b"g0\tsp0\ng1\tsp1\ng2\tsp2\ng3\tsp3\n"      # an unmapped-only group at threshold 0: an empty file
    all5 = BOUNDARY_TSV + b"s\tg0\ns\tg1\ns\tg2\ns\tg3\ns\tg4\n"
    ref = check_files(tmp_path, BOUNDARY_MAP, all5, 100)
    assert sorted(ref["files"]) == ["copiness.tsv", "profile.chk", "s.txt"]


def test_one_species(U, tmp_path):
    m, t = b"a x\nb x\n", b"q a\nr a\nr b\nu nope\n"
    ref = check_files(tmp_path, m, t, 100)
    assert [g[1:] for g in ref["groups"]] == [(1, 1, True), (0, 1, False), (0, 0, False)]
    assert ref["files"]["copiness.tsv"] == b"Query\tMultipleCopyPercent\tSingleCopyPercent\nq\t100\t100\nr\t100\t0\nu\t0\t0\n"


# ---- duplicated and split input

def test_duplicated_row_is_not_single_but_is_listed(U, tmp_path):
    m = b"a s1\nb s2\n"
    t = b"q a\nq a\nq b\n"
    A = R.arrays(m, t)
    got = host_count(U, A, 50)
    assert got["single"].tolist() == [1] and got["multiple"].tolist() == [2] and got["core"].tolist() == [1]
    assert got["core_gene"].tolist() == [0, 1] and got["core_species"].tolist() == [0, 1] and got["full"].tolist() == [0, 1]
    ref = check_files(tmp_path, m, t, 50)
    assert ref["files"]["q.txt"] == b"a\ts1\nb\ts2\n"


def test_gene_in_two_species_and_split_group_and_dash_name(U, tmp_path):
    m = b"a s1\na s2\nb s2\nc s3\na s1\n"
    t = b"AF-P12345-F1 a\nAF-P12345-F1 c\nplain a\nplain b\nAF-P12345-F1 c\nx-y b\n"
    A = R.arrays(m, t)
    assert A["n_groups"] == 4 and A["sp_off"].tolist() == [0, 2, 3, 4]
    same(host_count(U, A, 0), R.count(A["group"], A["gene"], A["n_groups"], A["sp_off"], A["sp"], A["n_species"], 0))
    ref = check_files(tmp_path, m, t, 30)
    assert ref["n_core"] == 4      # the name that heads two runs counts twice, and the later file replaces the earlier one
    assert ref["files"]["P12345.txt"] == b"c\ts3\n" and ref["files"]["y.txt"] == b"b\ts2\n" and ref["files"]["plain.txt"] == b"a\ts1\n"
    assert ref["files"]["copiness.tsv"].count(b"AF-P12345-F1\t") == 2


def test_m8_with_12_columns(U, tmp_path):
    m = b"a s1\nb s2\n"
    t = b"q\ta\t1.000\t100\t0\t0\t1\t100\t1\t100\t1.0E-30\t200\nq\tb\t0.500\t90\t40\t2\t1\t90\t5\t95\t1.0E-10\t80\n"
    ref = check_files(tmp_path, m, t, 100, tsv_name="OUTPUT.m8")
    assert ref["files"]["q.txt"] == b"a\ts1\nb\ts2\n"


# ---- formatting

def test_percent_formatting(tmp_path):
    assert [R.percent(x) for x in (50.0, 0.0, 100.0, 300.0 / 7, 200.0 / 3)] == ["50", "0", "100", "42.857142857142854", "66.66666666666667"]
    tiny = R.percent(100.0 / 16777215)
    assert "e" not in tiny.lower() and tiny.startswith("0.00000596")
    # 7 species: 3 / 7 single; 3 species: 2 / 3; the product prints what the reference prints
    m7 = b"".join(b"g%d s%d\n" % (k, k) for k in range(7))
    ref = check_files(tmp_path, m7, b"q g0\nq g1\nq g2\n", 100)
    assert ref["files"]["copiness.tsv"].endswith(b"q\t42.857142857142854\t42.857142857142854\n")
    (tmp_path / "b").mkdir()
    ref = check_files(tmp_path / "b", b"a x\nb y\nc z\n", b"q a\nq b\nr a\nr a\n", 100)
    assert ref["files"]["copiness.tsv"].endswith(b"q\t66.66666666666667\t66.66666666666667\nr\t33.333333333333336\t0\n")


def test_tiny_percentage_has_no_exponent(tmp_path):
    """100 / 16777215 itself is held against the reference's formatting in test_percent_formatting.  Through the file level S is the number of
    distinct species in the map, and a map of 2^24 - 1 species takes the better part of a minute to read, so the product prints
    100 / 1000003 = 9.99997e-05 here: below 1e-4, where every general or scientific float format switches to an exponent."""
    n = 1000003
    k = np.arange(n)
    line = np.zeros((n, 18), np.uint8)
    line[:] = np.frombuffer(b"g0000000 s0000000\n", np.uint8)
    for d in range(7):
        line[:, 7 - d] = line[:, 16 - d] = 48 + (k // 10 ** d) % 10
    m = line.tobytes()
    ref_line = b"q\t" + R.percent(100.0 / n).encode() + b"\t" + R.percent(100.0 / n).encode() + b"\n"
    db, tsv = write_case(tmp_path, m, b"q g0000005\n")
    out = str(tmp_path / "out")
    r = run_profile_host(db, tsv, out, 100)
    assert r.returncode == 0, r.stderr
    got = read(os.path.join(out, "copiness.tsv"))
    assert got == b"Query\tMultipleCopyPercent\tSingleCopyPercent\n" + ref_line and b"e" not in ref_line.lower()[1:]


# ---- parser and CLI

def cli(*args, host=True):
    env = dict(os.environ)
    if host:
        env["UC_PROFILE_HOST"] = "1"
    return subprocess.run([UNICORE, "profile"] + list(args), env=env, capture_output=True, text=True)


def test_cli_parser(tmp_path):
    db, tsv, out = os.path.join(GOLD, "db"), os.path.join(GOLD, "clust_default.tsv"), str(tmp_path / "o")
    r = cli()
    assert r.returncode == 2 and "Usage: unicore profile" in r.stderr and "--threshold" in r.stderr      # arg_required_else_help
    for bad in (["-t", "101", db, tsv, out], ["-t", "x", db, tsv, out], ["--threshold=-1", db, tsv, out], [db, tsv], [db, tsv, out, "extra"], ["-t"],
                ["--nope", db, tsv, out]):
        r = cli(*bad)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and not os.path.exists(out), (bad, r.stderr)
    assert "is not in range 0 to 100" in cli("-t", "101", db, tsv, out).stderr and "Not a number" in cli("-t", "x", db, tsv, out).stderr
    r = cli("-h")
    assert r.returncode == 0 and "Usage: unicore profile" in r.stdout and "[default: 80]" in r.stdout
    # other module names keep failing as before
    r = subprocess.run([UNICORE, "tree"], capture_output=True, text=True)
    assert r.returncode == 0x30 and "Module not implemented" not in r.stdout


def test_cli_on_the_golden(tmp_path):
    db, tsv, out = os.path.join(GOLD, "db"), os.path.join(GOLD, "clust_default.tsv"), str(tmp_path / "deep" / "o")
    r = cli(db, tsv, out)      # the defaults: threshold 80, verbosity 3
    assert r.returncode == 0, r.stderr
    assert "Profiling the taxonomic distribution of the genes... Done\n" in r.stdout
    assert "11 structural core genes found from 42 candidates" in r.stdout
    assert read(os.path.join(out, "profile.chk")) == b"1"
    ref = R.profile_text(read(db + ".map"), read(tsv), 80)
    assert dir_bytes(out) == ref["files"] and r.stderr == ""
    # -p, --threads and -v are accepted; threshold 0 warns per species in ascending order; verbosity 4 prints the per-gene line
    out0 = str(tmp_path / "o0")
    r = cli("-t", "0", "-p", "--threads", "2", "-v", "4", db, tsv, out0)
    assert r.returncode == 0, r.stderr
    ref0 = R.profile_text(read(db + ".map"), read(tsv), 0)
    assert r.stderr.splitlines() == ref0["warnings"] and len(ref0["warnings"]) == 5
    assert "Gene unicore_9310ceaecb reported 80.00% single copy and 100.00% multiple copy" in r.stdout
    assert dir_bytes(out0) == ref0["files"]
    r = cli("-t", "0", "-v", "1", db, tsv, out0)
    assert r.returncode == 0 and r.stdout == "" and r.stderr == ""


def test_no_device_is_class_4_without_the_switch(tmp_path):
    """without UC_PROFILE_HOST the counter runs on the device: on a machine without one the call is class 4, with one it succeeds"""
    import torch
    db, tsv, out = os.path.join(GOLD, "db"), os.path.join(GOLD, "clust_default.tsv"), str(tmp_path / "o")
    code = ("import sys, unicore_amd as U\n"
            "try:\n    U.profile(sys.argv[1], sys.argv[2], sys.argv[3], 80, verbosity=0)\n    print('rc 0')\n"
            "except U.UcError as e:\n    print('rc', e.code)\n")
    env = {k: v for k, v in os.environ.items() if k != "UC_PROFILE_HOST"}
    env["PYTHONPATH"] = util.ROOT
    r = subprocess.run([sys.executable, "-c", code, db, tsv, out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == ("rc 0" if torch.cuda.is_available() else "rc 4"), r.stdout + r.stderr


# ---- refusals

def test_refusals(U, tmp_path):
    one = dict(group=[0], gene=[0], n_groups=1, sp_off=[0, 1], sp=[0], n_species=1)

    def refused(**kw):
        a = dict(one, **kw)
        with pytest.raises(U.UcError) as ei:
            U.profile_count(a["group"], a["gene"], a["n_groups"], a["sp_off"], a["sp"], a["n_species"], 80)
        return ei.value.code

    assert U.profile_count(**one)["core"].tolist() == [1]
    assert refused(n_groups=1 << 24) == U.UC_ERR_ARGS and refused(n_species=1 << 24) == U.UC_ERR_ARGS
    assert refused(sp_off=np.zeros((1 << 24) + 1, np.uint64), gene=[U.NO_GENE]) == U.UC_ERR_ARGS      # 2^24 genes
    assert refused(group=[0, 1, 0], gene=[0, 0, 0], n_groups=2) == U.UC_ERR_ARGS                      # decreases
    assert refused(group=[0, 2], gene=[0, 0], n_groups=3) == U.UC_ERR_ARGS                            # skips
    assert refused(group=[1], n_groups=2) == U.UC_ERR_ARGS                                            # does not start at 0
    assert refused(n_groups=2) == U.UC_ERR_ARGS                                                       # ends early
    assert refused(gene=[1]) == U.UC_ERR_ARGS and refused(gene=[0xFFFFFFFE]) == U.UC_ERR_ARGS         # gene id out of range
    assert refused(sp=[1]) == U.UC_ERR_ARGS                                                           # species id out of range
    assert refused(sp_off=[0, 2], sp=[0, 0], n_species=2) == U.UC_ERR_ARGS                            # not a set
    assert U.profile_count([0], [U.NO_GENE], 1, [0, 1], [0], 1, 80)["core"].tolist() == [0]
    # file level: a short map line, a short TSV row, a missing map, a threshold beyond 100
    for m, t, thr, want in ((b"a s1\nlonely\n", b"q a\n", 80, U.UC_ERR_IO), (b"a s1\n", b"q a\nq\n", 80, U.UC_ERR_IO), (None, b"q a\n", 80, U.UC_ERR_IO),
                            (b"a s1\n", b"q a\n", 101, U.UC_ERR_ARGS)):
        d = tmp_path / ("r%d" % len(os.listdir(tmp_path)))
        d.mkdir()
        db, tsv = write_case(d, m or b"", t)
        if m is None:
            os.remove(db + ".map")
        code = ("import sys, unicore_amd as U\n"
                "try:\n    U.profile(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), verbosity=0)\n    print('rc 0')\n"
                "except U.UcError as e:\n    print('rc', e.code)\n")
        r = subprocess.run([sys.executable, "-c", code, db, tsv, str(d / "out"), str(thr)], env=dict(os.environ, UC_PROFILE_HOST="1", PYTHONPATH=util.ROOT),
                           capture_output=True, text=True)
        assert r.stdout.strip() == "rc %d" % want, (m, t, r.stdout, r.stderr)


# ---- header, binding and ABI

def test_header_binding_and_abi(U):
    hdr = read(os.path.join(util.ROOT, "include", "unicore_cluster.h")).decode()
    for name in ("uc_profile_count", "uc_profile_count_dev", "uc_profile"):
        assert "int %s(" % name in hdr and name in U.SYMBOLS and hasattr(U.lib(), name), name
    assert "#define UC_ABI_VERSION 9" in hdr and U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "#define UC_NO_GENE 0xffffffffu" in hdr and U.NO_GENE == 0xFFFFFFFF
