"""Rule UC-T/P (`unicore tree -a profile`) without a GPU: the host twin (uc_msa_profile_align / uc_msa_profile_layout) against the
Python reference (msa_profile_ref.py) on the shared case list (msa_profile_cases.py), the m = 2 tie to the oracle's sw, the validity of every
path, every refusal, the CLI's parser, the committed fixture tests/golden/tree_profile_d50.json re-derived from the reference, and the twin under
the address and undefined-behaviour sanitizers in a program of its own (msa_profile_host_check.cpp).  The HIP kernels and the whole module (its
star stage needs the device): test_msa_profile_gpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import bt_ref
import msa_profile_cases as PC
import msa_profile_ref as P
import msa_ref as R
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")
ALIGN_KEYS = ("aligned", "score", "qs", "ts", "qe", "te", "run_off", "runs")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def same_align(a, b, what=""):
    for k in ALIGN_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, a[k][:20], b[k][:20])


def same_layout(a, b, what=""):
    assert np.array_equal(a["width"], b["width"]), (what, a["width"][:20], b["width"][:20])
    for x, y in zip(a["cells"], b["cells"]):
        assert np.array_equal(x, y), (what, "cells")


def layout_kw(kw, a):
    return dict(grp_off=kw["grp_off"], width=kw["width"], cells=kw["cells"], res_off=kw["res_off"], res=kw["res"], aligned=a["aligned"], qs=a["qs"], ts=a["ts"],
                run_off=a["run_off"], runs=a["runs"])


@pytest.fixture(scope="module")
def material(U, O):
    """{name: (keyword set, the reference's alignment, the reference's layout)}, computed once"""
    g = U.msa_profile_geometry()
    out = {}
    for name, kw in PC.cases(O, g["chunk"], g["cap"]).items():
        a = P.align(**kw)
        out[name] = (kw, a, P.layout(**layout_kw(kw, a)))
    return out


# ---- host twin == reference
def test_twin_equals_reference(U, material):
    assert len(material) >= 25
    for name, (kw, want, want_l) in material.items():
        got = U.msa_profile_align(**kw)
        same_align(got, want, name)
        same_layout(U.msa_profile_layout(**layout_kw(kw, got)), want_l, name)


def test_thread_count_does_not_change_the_answer(U, material):
    for name in ("many_groups", "rows_8", "unaligned"):
        kw, want, _ = material[name]
        for threads in (0, 2, 16):
            same_align(U.msa_profile_align(threads=threads, **kw), want, (name, threads))


def test_rounds(U, material):
    for name in ("rows_8", "empty_column_and_single", "unaligned", "asymmetric"):
        kw = material[name][0]
        base = {k: kw[k] for k in ("grp_off", "res_off", "res", "S3", "SA", "gap_open", "gap_ext")}
        w_ref, c_ref, _ = P.refine(width=kw["width"], cells=kw["cells"], rounds=3, **base)
        width, cells = kw["width"], kw["cells"]
        for _ in range(3):
            a = U.msa_profile_align(width=width, cells=cells, **base)
            l = U.msa_profile_layout(**layout_kw(dict(kw, width=width, cells=cells), a))
            width, cells = l["width"], l["cells"]
        same_layout({"width": width, "cells": cells}, {"width": w_ref, "cells": c_ref}, name)


def test_the_cases_hold_what_they_are_for(material):
    """the properties the case list promises, read off the reference's answers"""
    ops = lambda runs: [(int(w) & 3, int(w) >> 2) for w in runs]
    row_runs = lambda a, r: a["runs"][int(a["run_off"][r]):int(a["run_off"][r + 1])]
    assert PC.has_floor_case(material["rounding"][0])
    a = material["gap_bits"][1]
    assert any(o == 1 and n > 1 for o, n in ops(a["runs"])) and any(o == 2 and n > 1 for o, n in ops(a["runs"]))
    kw, a, l = material["unaligned"]
    assert a["aligned"].tolist() == [1, 1, 1, 0, 1, 1, 1, 0] and a["score"][3] == 0 and a["score"][7] == 0
    W0, W1 = int(l["width"][0]), int(l["width"][1])
    assert bytes(l["cells"][0][3 * W0:4 * W0]) == b"-" * W0 and bytes(l["cells"][0][4 * W0 + 3 * W1:]) == b"-" * W1
    kw, a, l = material["realigned"]
    assert bytes(kw["cells"][0][4 * 75:]) == b"-" * 75 and a["aligned"][4] == 1 and a["score"][4] > 100
    kw, a, l = material["ties"]
    assert a["score"][0] == a["score"][1] and row_runs(a, 0).tolist() == row_runs(a, 1).tolist() and a["score"][4] == a["score"][5] > 0
    kw, a, l = material["empty_column_and_single"]
    assert l["width"].tolist()[:2] == [61, 20] and all(any(o == 1 for o, _ in ops(row_runs(a, r))) for r in range(3))
    assert a["aligned"][3] == 0 and bytes(l["cells"][0][3 * 61:3 * 61 + 20]) == bytes(kw["cells"][0][3 * 62:3 * 62 + 20])


def test_two_rows_tie_the_rule_to_the_oracle(U, O):
    """m = 2: the divisor is 1 and the profile is the other row's matrix rows, so score and end are the oracle's sw(other row of the MSA, row).
    The MSA rows hold no gap here (a gap would be a column of zeros, which no letter of the oracle's alphabet gives); the residues behind them
    are mutated copies with indels, and one unrelated row."""
    rng = np.random.default_rng(99)
    for mats in (None, PC.asymmetric(O)):
        p = O.default_params()
        if mats is not None:
            p.S3[:] = [int(x) for x in mats[0].reshape(-1)]
            p.SA[:] = [int(x) for x in mats[1].reshape(-1)]
        S3, SA = bt_ref.matrices(p)
        for W in (40, 64, 150):
            anc = PC._rnd(rng, W)
            rows = []
            for k in range(2):
                c3, ca = bt_ref.mutate(rng, anc[1], anc[0], 0.1)[0][:W], anc[0]
                c3 = np.concatenate([c3, anc[1][len(c3):]])      # W columns again
                r3, ra = bt_ref.mutate(rng, anc[1], anc[0], 0.2) if k == 0 or W != 64 else PC._rnd(rng, 30)[::-1]
                rows.append(([PC.LETTERS[ca], PC.LETTERS[c3]], [PC.LETTERS[ra], PC.LETTERS[r3]]))
            kw = PC.case([rows], S3, SA, p.gap_open, p.gap_ext)
            got = U.msa_profile_align(**kw)
            same_align(got, P.align(**kw), W)
            for r in range(2):
                other, row = rows[1 - r][0], rows[r][1]
                s, qe, te = O.sw(P.CODE[other[1]], P.CODE[other[0]], P.CODE[row[1]], P.CODE[row[0]], p)
                if s > 0:
                    assert (int(got["score"][r]), int(got["qe"][r]), int(got["te"][r])) == (s, qe, te), (W, r)
                else:
                    assert got["aligned"][r] == 0 and got["score"][r] == 0


def test_paths_are_valid(U, material):
    """bt_ref.check_valid's points with s_r in the place of the matrix term: run shapes, the box, the path's own score"""
    for name in ("rows_3", "length_257", "asymmetric", "gap_bits", "gap_bits_open_eq_ext", "ties", "realigned", "width_65"):
        kw = material[name][0]
        got = U.msa_profile_align(**kw)
        go, o = [int(x) for x in kw["grp_off"]], 0
        mats = [np.asarray(kw["SA"]).reshape(21, 21), np.asarray(kw["S3"]).reshape(21, 21)]
        for g in range(len(go) - 1):
            m, W = go[g + 1] - go[g], int(kw["width"][g])
            grids = [c[o:o + m * W].reshape(m, W) for c in kw["cells"]]
            o += m * W
            for r in range(go[g], go[g + 1]):
                if not got["aligned"][r]:
                    continue
                res = [t[int(kw["res_off"][r]):int(kw["res_off"][r + 1])] for t in kw["res"]]
                S = P.cell_scores(grids, res, mats, r - go[g])
                runs = [(int(w) >> 2, int(w) & 3) for w in got["runs"][int(got["run_off"][r]):int(got["run_off"][r + 1])]]
                assert all(n > 0 and op < 3 for n, op in runs) and all(a[1] != b[1] for a, b in zip(runs, runs[1:])) and runs[0][1] == 0 and runs[-1][1] == 0
                i, j, sc = int(got["qs"][r]), int(got["ts"][r]), 0
                for n, op in runs:
                    if op == 0:
                        sc += int(sum(S[i + k, j + k] for k in range(n))); i += n; j += n
                    else:
                        sc -= kw["gap_open"] + (n - 1) * kw["gap_ext"]
                        i, j = (i + n, j) if op == 1 else (i, j + n)
                assert (i - 1, j - 1) == (int(got["qe"][r]), int(got["te"][r])) and i <= W and j <= len(res[0]), (name, r)
                assert sc == int(got["score"][r]) > 0, (name, r, sc)


# ---- refusals
def test_refusals(U, material):
    kw = material["rows_2"][0]
    U.msa_profile_align(**kw)

    def code(fn, **over):
        with pytest.raises(U.UcError) as ei:
            fn(**over)
        return ei.value.code

    al = lambda **over: code(U.msa_profile_align, **dict(kw, **over))
    assert al(gap_open=0, gap_ext=1) == U.UC_ERR_ARGS and al(gap_open=5, gap_ext=-1) == U.UC_ERR_ARGS
    assert al(gap_open=(1 << 20) + 1) == U.UC_ERR_ARGS                                      # scores stay in 32 bits
    U.msa_profile_align(**dict(kw, gap_open=1 << 20))
    for ch in (b"*", b"1", b" ", b"\0"):                                                    # neither a letter nor `-`
        bad = kw["cells"][0].copy()
        bad[3] = ch[0]
        assert al(cells=[bad, kw["cells"][1]]) == U.UC_ERR_ARGS and al(cells=[kw["cells"][0], bad]) == U.UC_ERR_ARGS
    k = int(np.flatnonzero(kw["cells"][0] != P.GAP)[0])
    bad = kw["cells"][0].copy()
    bad[k] = P.GAP
    assert al(cells=[bad, kw["cells"][1]]) == U.UC_ERR_ARGS                                 # the tracks disagree on a gap
    assert al(grp_off=[0, 0, 2], width=[90, 90]) == U.UC_ERR_ARGS and al(grp_off=[1, 2], width=[180]) == U.UC_ERR_ARGS
    ro = kw["res_off"].copy()
    ro[1] = ro[2] + 1
    assert al(res_off=ro) == U.UC_ERR_ARGS
    # width x length of 2^31 and more, and more rows than a group holds: refused from the shapes alone, before a cell is read
    L = U.lib()
    one, big_w, ro2 = np.array([0, 1], np.uint64), np.array([1 << 16], np.uint32), np.array([0, 1 << 15], np.uint64)
    z = np.zeros(8, np.int64)
    S = np.zeros(441, np.int8)
    args = lambda go, w, ro, c: [len(go) - 1, go.ctypes.data, w.ctypes.data, c, c, ro.ctypes.data, z.ctypes.data, z.ctypes.data, S.ctypes.data, S.ctypes.data, 10, 1] + [z.ctypes.data] * 8 + [0, None, 1]
    many = np.array([0, 65535], np.uint64)
    assert L.uc_msa_profile_align(*args(many, np.array([0], np.uint32), np.zeros(65536, np.uint64), None)) == U.UC_ERR_ARGS
    dash = np.full(1 << 16, P.GAP, np.uint8)
    assert L.uc_msa_profile_align(*args(one, big_w, ro2, dash.ctypes.data)) == U.UC_ERR_ARGS and "2^31" in L.uc_last_error().decode()
    # a row whose decision bytes, laid out by chunk and anti-diagonal, reach 2^31: 1 column against 2^25 residues
    assert L.uc_msa_profile_align(*args(one, np.array([1], np.uint32), np.array([0, 1 << 25], np.uint64), dash.ctypes.data)) == U.UC_ERR_ARGS
    assert "decision bytes" in L.uc_last_error().decode()
    # the layout: runs that are no runs, that repeat an operation, that overrun the columns or the row
    a = U.msa_profile_align(**kw)
    lay = lambda **over: code(U.msa_profile_layout, **dict(layout_kw(kw, a), **over))
    n0 = int(a["run_off"][1])
    for first in (5 << 2 | 3, 0 << 2 | 0, 1000 << 2 | 0, 1000 << 2 | 2):
        runs = a["runs"].copy()
        runs[0] = first
        assert lay(runs=runs) == U.UC_ERR_ARGS, first
    if n0 >= 3:
        runs = a["runs"].copy()
        runs[1] = runs[0]
        assert lay(runs=runs) == U.UC_ERR_ARGS
    assert lay(qs=[-1, 0]) == U.UC_ERR_ARGS and lay(ts=[0, -1]) == U.UC_ERR_ARGS and lay(qs=[1000, 0]) == U.UC_ERR_ARGS
    # an unaligned row's runs are not read
    runs = a["runs"].copy()
    runs[0] = 3
    U.msa_profile_layout(**dict(layout_kw(kw, a), aligned=[0, 1], runs=runs))


TREE_CODE = ("import sys, unicore_amd as U\n"
             "try:\n    U.tree(sys.argv[1], sys.argv[2], sys.argv[3], 50, sys.argv[4], verbosity=0, aligner='profile', refine_iters=int(sys.argv[5]))\n    print('rc 0')\n"
             "except U.UcError as e:\n    print('rc', e.code)\nexcept ValueError as e:\n    print('value error')\n")


def test_refusals_of_the_file_level(U, tmp_path):
    """rounds beyond 8 and gaps with open < extend are refused before a file is written or the device is asked for"""
    import ctypes as C
    db = os.path.join(GOLD, "db")
    name = open(db + "_h", "rb").read().split(b"\n")[0].strip(b"\0").split()[0]
    (tmp_path / "prof").mkdir()
    (tmp_path / "prof" / "g1.txt").write_bytes(name + b"\ts1\n")
    run = lambda out, opts, n: subprocess.run([os.sys.executable, "-c", TREE_CODE, db, str(tmp_path / "prof"), str(tmp_path / out), opts, str(n)],
                                              env=dict(os.environ, PYTHONPATH=util.ROOT), capture_output=True, text=True).stdout.strip()
    assert run("a", "--gap-open 1 --gap-extend 2", 1) == "rc 2" and not os.path.exists(str(tmp_path / "a"))
    assert run("b", "", 9) == "value error" and run("c", "", 0) == "value error"
    o = U.make_opts("", 1, 0, -1)
    assert U.lib().uc_tree_refined(db.encode(), str(tmp_path / "prof").encode(), str(tmp_path / "d").encode(), 50, b"", 9, C.byref(o), None) == U.UC_ERR_ARGS
    assert not os.path.exists(str(tmp_path / "d"))


# ---- the CLI's parser
def cli(*args):
    return subprocess.run([UNICORE, "tree"] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1"), capture_output=True, text=True)


def test_cli_parser(tmp_path):
    db, prof, out = os.path.join(GOLD, "db"), str(tmp_path / "prof"), str(tmp_path / "o")
    h = cli("-h")
    assert h.returncode == 0 and "[star, profile]" in h.stdout and "--refine-iters <N>" in h.stdout and "[1 - 8]" in h.stdout
    for bad in (["--refine-iters", "0"], ["--refine-iters", "9"], ["--refine-iters=x"], ["--refine-iters", "-1"], ["--refine-iters", "99999999999"]):
        r = cli("-n", "-a", "profile", *bad, db, prof, out)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and "--refine-iters" in r.stderr and not os.path.exists(out), (bad, r.stderr)
    assert cli("-n", "-a", "profile", "--refine-iters").returncode == 2
    for al in (["-a", "star"], []):                                                # the rounds belong to the profile aligner
        r = cli("-n", *al, "--refine-iters", "2", db, prof, out)
        assert r.returncode == 1 and "--refine-iters" in r.stderr and "profile" in r.stderr and not os.path.exists(out)
    r = cli("-n", "-a", "profiles", db, prof, out)
    assert r.returncode == 1 and "Unrecognized aligner" in r.stderr
    r = cli("-n", "-a", "foldmason", "--refine-iters", "2", db, prof, out)
    assert r.returncode == 1 and "external program" in r.stderr
    # an existing concatenation: the reference's message, status 0, whichever aligner is named
    os.makedirs(out)
    open(os.path.join(out, "combined.fasta"), "w").write(">x\nA\n")
    for extra in (["-a", "profile"], ["--aligner=profile", "--refine-iters=8"]):
        r = cli("-n", *extra, db, prof, out)
        assert r.returncode == 0 and r.stdout == "Concatenated alignment file %s/combined.fasta already exists, skipping alignment step\n" % out, r.stderr
    r = subprocess.run([UNICORE, "gene-tree", "-a", "profile", "-t", "nj", str(tmp_path / "none")], capture_output=True, text=True)
    assert r.returncode == 1 and "Input directory does not exist" in r.stderr      # gene-tree reads over -a as before


# ---- the committed fixture
def test_golden_is_what_the_reference_gives(O):
    prof = json.load(open(os.path.join(GOLD, "profile_default_t80.json")))
    genes = {k: v.encode("ascii") for k, v in prof.items() if k.endswith(".txt")}
    gold, star = json.load(open(os.path.join(GOLD, "tree_profile_d50.json"))), json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    p = util.oracle_params(O, R.FIXED_OPTS)
    for rounds in (1, 2):
        files, info = P.tree_files(O, p, os.path.join(GOLD, "db"), genes, 50, rounds)
        assert R.digest(files) == gold["rounds_%d" % rounds]
        assert all(len(v["refine"]) == rounds for v in info.values()) and len(info) == 11
    # the fixture shows something: the refined alignment is not the star alignment, and the second round moves it again
    assert gold["rounds_1"]["combined.fasta"] != star["combined.fasta"] and gold["rounds_2"]["combined.fasta"] != gold["rounds_1"]["combined.fasta"]
    assert gold["rounds_1"]["sha256"] != star["sha256"] and set(gold["rounds_1"]["sha256"]) == set(star["sha256"])
    zero, _ = P.tree_files(O, p, os.path.join(GOLD, "db"), genes, 50, 0)
    assert R.digest(zero) == star


def test_header_binding_and_abi(U):
    import ctypes as C
    hdr = open(os.path.join(util.ROOT, "include", "unicore_cluster.h")).read()
    for name in ("uc_msa_profile_align", "uc_msa_profile_align_dev", "uc_msa_profile_layout", "uc_msa_profile_layout_dev", "uc_msa_profile_geometry", "uc_tree_refined"):
        assert "int %s(" % name in hdr and name in U.SYMBOLS and hasattr(U.lib(), name), name
    assert "#define UC_ABI_VERSION 9" in hdr and U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "#define UC_TREE_MAX_REFINE 8" in hdr and U.TREE_MAX_REFINE == 8 and "#define UC_TREE_REFINED_NPHASE 3" in hdr and len(U.TREE_REFINED_PHASES) == 3
    assert C.sizeof(U.UcTreeRefinedStats) == C.sizeof(U.UcTreeStats) + 5 * 8 + 2 * 8 * 8 + 3 * 8 and C.sizeof(U.UcTreeStats) == 7 * 8 + 7 * 8
    g = U.msa_profile_geometry()
    assert g["chunk"] == 64 and g["cap"] == 0


# ---- the host twin under the sanitizers, in a program of its own
def test_host_twin_under_sanitizers(tmp_path):
    csrc = os.path.join(util.ROOT, "unicore_amd", "csrc")
    exe = str(tmp_path / "msa_profile_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-pthread",
                         "-I" + os.path.join(util.ROOT, "include"), "-I" + csrc, os.path.join(util.ROOT, "tests", "msa_profile_host_check.cpp"),
                         os.path.join(csrc, "uc_msa_profile_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert run.stdout.strip() == "msa_profile_host_check: ok"
