"""Rule UC-T (`unicore tree --no-inference`) without a GPU: the host twins (uc_msa_center / uc_msa_star / uc_msa_filter) against the Python
reference (msa_ref.py) on the shared case list (tree_cases.py), every refusal, the CLI's parser, and the committed fixture
tests/golden/tree_default_d50.json re-derived from the reference.  The DP behind uc_tree needs the device: test_tree_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msa_ref as R
import tree_cases as TC
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


def same_star(a, b, what=""):
    for k in ("width", "col", "cnt"):
        assert np.array_equal(a[k], b[k]), (what, k, a[k][:20], b[k][:20])
    assert len(a["cells"]) == len(b["cells"])
    for x, y in zip(a["cells"], b["cells"]):
        assert np.array_equal(x, y), (what, "cells")


def same_filter(a, b, what=""):
    for k in ("keep", "fwidth", "fcells"):
        assert np.array_equal(a[k], b[k]), (what, k)


def campaign():
    """40 seeds of synthetic valid backtraces: (seed, groups, case)"""
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        groups = TC.random_groups(rng, [int(x) for x in rng.integers(1, 12, 6)])
        yield seed, groups, TC.build(groups, seed)


# ---- host twins == reference
def test_star_hand_cases(U):
    for name, (_, case) in TC.hand_cases().items():
        same_star(U.msa_star(**case), R.star(**case), name)
    r = U.msa_star(**TC.empty_case())
    assert len(r["width"]) == len(r["col"]) == len(r["cnt"]) == 0 and all(len(c) == 0 for c in r["cells"])
    # one track renders what track 0 of two renders
    _, case = TC.hand_cases()["same_slot_two_lengths"]
    one = U.msa_star(**dict(case, res=case["res"][0]))
    assert len(one["cells"]) == 1 and np.array_equal(one["cells"][0], R.star(**case)["cells"][0])


def test_star_values_by_hand(U):
    """two rows inserting 3 and 5 residues at slot 4 of a centre of 10, a third row inserting 1 at slot 4 as well (its qs = 1)"""
    _, case = TC.hand_cases()["same_slot_two_lengths"]
    r = U.msa_star(**case)
    assert r["width"].tolist() == [15] and r["col"].tolist() == [0, 1, 2, 3, 9, 10, 11, 12, 13, 14]
    rows = [bytes(r["cells"][0][i * 15:(i + 1) * 15]) for i in range(4)]
    aa, off = case["res"][0], case["res_off"]
    row = lambda i: bytes(aa[int(off[i]):int(off[i + 1])])
    assert rows[1] == row(1)[:4] + b"-----" + row(1)[4:]                                           # the centre
    assert rows[0] == row(0)[:4] + row(0)[4:7] + b"--" + row(0)[7:13]                              # left-justified in the block of 5
    assert rows[2] == row(2)[2:6] + row(2)[6:11] + row(2)[11:17]                                   # ts = 2: the residues before the box are not part
    assert rows[3] == b"-" + row(3)[0:3] + row(3)[3:4] + b"----" + row(3)[4:6] + b"----"           # qs = 1, ends at centre position 6
    assert r["cnt"].tolist() == [3, 4, 4, 4, 3, 2, 2, 1, 1, 4, 4, 3, 3, 3, 3]      # column 4: rows 0, 2, 3; columns 5, 6: rows 0, 2; 7, 8: row 2


def test_star_campaign(U):
    tot = {}
    for seed, groups, case in campaign():
        same_star(U.msa_star(**case), R.star(**case), seed)
        for k, v in TC.events(groups).items():
            tot[k] = tot.get(k, 0) + v
    # counted once with the reference when the test was written: 168 / 183 / 148 / 428
    assert tot == dict(shared_unequal=168, trailing=183, unaligned=148, qs_positive=428)


def test_center(U):
    for name, (go, sc, want) in TC.centre_cases().items():
        got = U.msa_center(go, sc)
        assert np.array_equal(got, R.center(go, sc)), name
        if want is not None:
            assert got.tolist() == want, name


def test_filter(U):
    for name, (go, w, cells, thr, want) in TC.filter_cases().items():
        got = U.msa_filter(go, w, cells, thr)
        same_filter(got, R.filter(go, w, cells, thr), name)
        if want is not None:
            assert got["fwidth"].tolist() == want, name
    # the filter of a rendered group: counts of the star call decide the same columns
    _, case = TC.hand_cases()["rows_70"]
    s = U.msa_star(**case)
    f = U.msa_filter(case["grp_off"], s["width"], s["cells"][0], 50)
    assert np.array_equal(f["keep"], (s["cnt"].astype(np.int64) * 100 >= 50 * 70).astype(np.uint8))


# ---- refusals
def test_refusals_of_the_entry_points(U):
    _, ok = TC.hand_cases()["two_rows"]

    def refused(fn, *a, **kw):
        with pytest.raises(U.UcError) as ei:
            fn(*a, **kw)
        return ei.value.code

    star = lambda **kw: refused(U.msa_star, **dict(ok, **kw))
    U.msa_star(**ok)
    assert star(centre=[2]) == U.UC_ERR_ARGS                                                   # centre outside its group
    assert star(runs=[5 << 2 | 0, 2 << 2 | 3, 7 << 2 | 0]) == U.UC_ERR_ARGS                    # op 3
    assert star(runs=[5 << 2 | 0, 0 << 2 | 2, 7 << 2 | 0]) == U.UC_ERR_ARGS                    # length 0
    assert star(runs=[5 << 2 | 0, 2 << 2 | 0, 7 << 2 | 0]) == U.UC_ERR_ARGS                    # adjacent runs of one operation
    assert star(runs=[5 << 2 | 0, 2 << 2 | 2, 8 << 2 | 0]) == U.UC_ERR_ARGS                    # overruns the centre (13 of 12) and the row
    assert star(runs=[5 << 2 | 0, 4 << 2 | 2, 7 << 2 | 0]) == U.UC_ERR_ARGS                    # overruns the row only (16 of 15)
    assert star(qs=[1, 0]) == U.UC_ERR_ARGS                                                    # qs moves the end past the centre
    assert star(qs=[-1, 0]) == U.UC_ERR_ARGS and star(ts=[-1, 0]) == U.UC_ERR_ARGS
    assert star(grp_off=[0, 0, 2], centre=[0, 0]) == U.UC_ERR_ARGS                             # an empty group
    assert star(grp_off=[1, 2], centre=[0]) == U.UC_ERR_ARGS                                   # does not start at 0
    assert star(res_off=[0, 30, 27]) == U.UC_ERR_ARGS                                          # malformed residue CSR
    assert star(run_off=[0, 3, 2]) == U.UC_ERR_ARGS                                            # malformed run CSR
    assert star(run_off=[1, 3, 3]) == U.UC_ERR_ARGS
    # an unaligned row's runs are not read, whatever they hold
    U.msa_star(**dict(ok, aligned=[0, 1], runs=[5 << 2 | 3, 0, 0]))
    # centre: an empty group; more than 65535 rows
    assert refused(U.msa_center, [0, 0], []) == U.UC_ERR_ARGS
    big, c1 = np.array([0, 65536], np.uint64), np.zeros(1, np.uint32)
    assert U.lib().uc_msa_center(1, big.ctypes.data, None, c1.ctypes.data) == U.UC_ERR_ARGS      # refused before a score is read
    # filter: the threshold
    assert refused(U.msa_filter, [0, 1], [1], np.frombuffer(b"A", np.uint8), 101) == U.UC_ERR_ARGS
    assert refused(U.msa_filter, [0, 0], [1], np.zeros(0, np.uint8), 50) == U.UC_ERR_ARGS
    # a capacity that is too small reports what is needed
    import ctypes as C
    go, ce, ro, uo = (np.ascontiguousarray(ok[k], t) for k, t in (("grp_off", np.uint64), ("centre", np.uint32), ("res_off", np.uint64), ("run_off", np.uint64)))
    need, width, col = np.zeros(2, np.uint64), np.zeros(1, np.uint32), np.zeros(12, np.uint32)
    rc = U.lib().uc_msa_star(1, go.ctypes.data, ce.ctypes.data, 1, ro.ctypes.data, ok["res"][0].ctypes.data, None, ok["qs"].ctypes.data, ok["ts"].ctypes.data,
                             uo.ctypes.data, ok["runs"].ctypes.data, ok["aligned"].ctypes.data, width.ctypes.data, col.ctypes.data, None, 0, None, None, 0, need.ctypes.data)
    assert rc == U.UC_ERR_ARGS and need.tolist() == [14, 28] and width.tolist() == [14] and C.sizeof(U.UcTreeStats) == 7 * 8 + 7 * 8
    # a centre without a residue has no col entry: a NULL col is fine there, the trailing insert still makes 4 columns
    _, z = TC.hand_cases()["empty_length_centre"]
    cnt, c0 = np.zeros(4, np.uint32), np.zeros(12, np.uint8)
    rc = U.lib().uc_msa_star(1, z["grp_off"].ctypes.data, z["centre"].ctypes.data, 1, z["res_off"].ctypes.data, z["res"][0].ctypes.data, None, z["qs"].ctypes.data,
                             z["ts"].ctypes.data, z["run_off"].ctypes.data, z["runs"].ctypes.data, z["aligned"].ctypes.data, width.ctypes.data, None, cnt.ctypes.data, 4,
                             c0.ctypes.data, None, 12, need.ctypes.data)
    assert rc == 0 and width.tolist() == [4] and need.tolist() == [4, 12] and cnt.tolist() == [1, 1, 1, 1] and bytes(c0[:4]) == b"----" and bytes(c0[8:]) == b"----"


TREE_CODE = ("import sys, unicore_amd as U\n"
             "try:\n    U.tree(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5], verbosity=int(sys.argv[6]))\n    print('rc 0')\n"
             "except U.UcError as e:\n    print('rc', e.code)\n")


def run_tree(db, prof, out, threshold=50, opts="", verbosity=0, env=None):
    e = dict(os.environ, PYTHONPATH=util.ROOT, **(env or {}))
    return subprocess.run([sys.executable, "-c", TREE_CODE, db, prof, out, str(threshold), opts, str(verbosity)], env=e, capture_output=True, text=True)


def test_refusals_of_the_file_level(tmp_path):
    """every input is read and checked before the device is asked for: these answers do not depend on one"""
    db = os.path.join(GOLD, "db")
    name = open(db + "_h", "rb").read().split(b"\n")[0].strip(b"\0").split()[0]

    def rc_of(lines, threshold=50, opts="", make=True):
        d = tmp_path / ("r%d" % len(os.listdir(tmp_path)))
        d.mkdir()
        if make:
            (d / "prof").mkdir()
            (d / "prof" / "g1.txt").write_bytes(lines)
            (d / "prof" / "copiness.tsv").write_bytes(b"not a gene file\n")
        r = run_tree(db, str(d / "prof"), str(d / "out"), threshold, opts)
        assert not os.path.exists(str(d / "out" / "combined.fasta"))
        return r.stdout.strip()

    assert rc_of(name + b"\ts1\n", threshold=101) == "rc 2"
    assert rc_of(name + b"\ts1\n", opts="--no-such-flag 1") == "rc 2"
    assert rc_of(name + b"\ts1\n", opts="--gap-open 99") == "rc 2"
    assert rc_of(name + b"\ts1\n", make=False) == "rc 3"                           # no profile directory
    assert rc_of(name + b"\ts1\textra\n") == "rc 3"                               # three fields
    assert rc_of(name + b"\n") == "rc 3"                                          # one field
    assert rc_of(name + b"\ts1\n\n" + name + b"\ts2\n") == "rc 3"                 # an empty line has no field
    assert rc_of(b"no_such_gene\ts1\n") == "rc 3"
    assert rc_of((name + b"\ts\n") * 65536) == "rc 2"                             # more than 65535 rows
    d = tmp_path / "nodb"
    (d / "prof").mkdir(parents=True)
    (d / "prof" / "g1.txt").write_bytes(name + b"\ts1\n")
    assert run_tree(str(d / "missing_db"), str(d / "prof"), str(d / "out")).stdout.strip() == "rc 3"


def test_existing_concatenation_is_kept(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    (out / "combined.fasta").write_bytes(b">kept\nAC\n")
    r = run_tree(os.path.join(GOLD, "db"), str(tmp_path / "no_such_dir"), str(out), verbosity=3)
    assert r.stdout.splitlines() == ["Concatenated alignment file %s/combined.fasta already exists, skipping alignment step" % out, "rc 0"], r.stdout + r.stderr
    assert sorted(os.listdir(out)) == ["combined.fasta"] and (out / "combined.fasta").read_bytes() == b">kept\nAC\n"


# ---- the CLI's parser
def cli(*args):
    return subprocess.run([UNICORE, "tree"] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1"), capture_output=True, text=True)


def test_cli_parser(tmp_path):
    db, prof, out = os.path.join(GOLD, "db"), str(tmp_path / "prof"), str(tmp_path / "o")
    r = cli()                                                                      # the bare module name keeps its earlier answer
    assert r.returncode == 0x30 and r.stderr == "Error: tree\n"
    r = cli("-h")
    assert r.returncode == 0 and "Usage: unicore tree" in r.stdout and "[default: 50]" in r.stdout and "--no-inference" in r.stdout
    for bad in (["-n", "-d", "101", db, prof, out], ["-n", "-d", "x", db, prof, out], ["-n", "--threshold=-1", db, prof, out], ["-n", db, prof],
                ["-n", db, prof, out, "extra"], ["-n", "-d"], ["-n", "--nope", db, prof, out], ["-n", "-v", "9", db, prof, out]):
        r = cli(*bad)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and not os.path.exists(out), (bad, r.stderr)
    assert "is not in range 0 to 100" in cli("-n", "-d", "101", db, prof, out).stderr and "Not a number" in cli("-n", "-d", "x", db, prof, out).stderr
    for al in ("foldmason", "mafft", "mafft-linsi"):
        r = cli("-n", "-a", al, db, prof, out)
        assert r.returncode == 1 and "external program" in r.stderr and al in r.stderr and not os.path.exists(out)
    r = cli("-n", "--aligner", "clustal", db, prof, out)
    assert r.returncode == 1 and "Unrecognized aligner" in r.stderr
    r = cli("-n", "-t", "phyml", db, prof, out)
    assert r.returncode == 1 and "Unrecognized tree builder" in r.stderr
    for ok_builder in ("iqtree", "fasttree", "raxml-ng"):                          # validated, then the missing -n refuses before any work
        r = cli("-t", ok_builder, "-p", "-m JTT", "-c", "2", db, prof, out)
        assert r.returncode == 1 and "--no-inference" in r.stderr and ok_builder in r.stderr and not os.path.exists(out)
    # an existing concatenation: the reference's message, status 0, with the built-in aligner named or not
    os.makedirs(out)
    open(os.path.join(out, "combined.fasta"), "w").write(">x\nA\n")
    for extra in ([], ["-a", "star", "-o", "--gap-open 12", "-d", "0"]):
        r = cli("-n", *extra, db, prof, out)
        assert r.returncode == 0 and r.stdout == "Concatenated alignment file %s/combined.fasta already exists, skipping alignment step\n" % out, r.stderr
    assert cli("-n", "-v", "2", db, prof, out).stdout == ""
    for other in ("gene-tree", "easy-core", "createdb"):
        r = subprocess.run([UNICORE, other], capture_output=True, text=True)
        assert r.returncode == 0x30, other


# ---- the committed fixture
def test_golden_is_what_the_reference_gives():
    from oracle import oracle_py as O
    prof = json.load(open(os.path.join(GOLD, "profile_default_t80.json")))
    genes = {k: v.encode("ascii") for k, v in prof.items() if k.endswith(".txt")}
    assert len(genes) == 11
    files, info = R.tree_files(O, util.oracle_params(O, R.FIXED_OPTS), os.path.join(GOLD, "db"), genes, 50)
    assert R.digest(files) == json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    names = [l[1:] for l in files["combined.fasta"].decode().splitlines() if l.startswith(">")]
    seqs = [l for l in files["combined.fasta"].decode().splitlines() if not l.startswith(">")]
    parts = files["combined.fasta.partitions"].decode().splitlines()
    assert len(parts) == 11 and len(set(names)) == len(names) == 5 and len({len(s) for s in seqs}) == 1
    assert parts[0].startswith("JTT+F+I+G, unicore_") and parts[-1].endswith("-%d" % len(seqs[0]))


def test_header_binding_and_abi(U):
    hdr = open(os.path.join(util.ROOT, "include", "unicore_cluster.h")).read()
    for name in ("uc_msa_center", "uc_msa_center_dev", "uc_msa_star", "uc_msa_star_dev", "uc_msa_filter", "uc_msa_filter_dev", "uc_tree"):
        assert "int %s(" % name in hdr and name in U.SYMBOLS and hasattr(U.lib(), name), name
    assert "#define UC_ABI_VERSION 9" in hdr and U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "#define UC_TREE_NPHASE 7" in hdr and len(U.TREE_PHASES) == 7
