"""Rule UC-T/G (`unicore tree -a progressive`) without a GPU: the host twins (uc_msa_guide, uc_msa_merge, uc_msa_progressive) equal the Python
reference (msa_progressive_ref.py) byte for byte on the shared case list (msa_progressive_cases.py); the cases hold what they are for; the properties
of the result; the argument refusals; the CLI's parser; the committed fixture tests/golden/tree_progressive_d50.json."""
import json
import os
import subprocess

import numpy as np
import pytest

import msa_progressive_cases as GC
import msa_progressive_ref as G
import msa_ref as R
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")
NEW_SYMBOLS = ("uc_msa_self_scores", "uc_msa_guide", "uc_msa_guide_dev", "uc_msa_merge", "uc_msa_merge_dev", "uc_msa_progressive", "uc_msa_progressive_dev",
               "uc_msa_progressive_geometry", "uc_tree_progressive")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def ref_merges(kw):
    """the reference's answer to a keyword set of msa_merge, as the dict of unicore_amd.msa_merge"""
    mats = [np.asarray(kw["SA"], np.int64), np.asarray(kw["S3"], np.int64)]
    rs = [G.merge(a, b, mats, kw["gap_open"], kw["gap_ext"]) for a, b in GC.tasks_of(kw)]
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    out = {k: np.array([r[k] for r in rs], np.uint32 if k == "width" else np.int32) for k in ("score", "is", "js", "ie", "je", "width")}
    out["run_off"] = np.concatenate([[0], np.cumsum([len(r["runs"]) for r in rs])]).astype(np.uint64)
    out["runs"] = cat([np.array(r["runs"], np.uint32) for r in rs], np.uint32)
    out["cells"] = [cat([r["cells"][t].reshape(-1) for r in rs], np.uint8) for t in range(2)]
    return out


def same_merge(a, b, what=""):
    for k in ("score", "is", "js", "ie", "je", "width", "run_off", "runs"):
        assert np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)), (what, k)
    for t in range(2):
        assert np.array_equal(a["cells"][t], b["cells"][t]), (what, "cells", t)


def same_msa(a, b, what=""):
    assert np.array_equal(a["width"], b["width"]), (what, a["width"], b["width"])
    for t in range(2):
        assert np.array_equal(a["cells"][t], b["cells"][t]), (what, "cells", t)


@pytest.fixture(scope="module")
def merges():
    """{name: (keyword set, the reference's answer)}, computed once"""
    return {name: (kw, ref_merges(kw)) for name, kw in GC.merge_cases().items()}


@pytest.fixture(scope="module")
def trees():
    return {name: (kw, G.progressive(**kw)) for name, kw in GC.progressive_cases().items()}


def test_reference_dp_is_the_recurrence():
    """the reference's row-at-a-time DP gives the cell-by-cell recurrence's H, E and F"""
    rng = np.random.default_rng(3)
    for _ in range(40):
        s = rng.integers(-9, 9, (int(rng.integers(1, 9)), int(rng.integers(1, 9))))
        o = int(rng.integers(0, 12))
        e = int(rng.integers(0, o + 1))
        for x, y in zip(G.dp(s, o, e), G.dp_plain(s, o, e)):
            assert np.array_equal(x[1:, 1:], y[1:, 1:])


def test_twin_equals_reference(U, merges, trees):
    for name, (kw, want) in merges.items():
        same_merge(U.msa_merge(**kw), want, name)
    for name, (kw, want) in trees.items():
        got = U.msa_progressive(**kw)
        same_msa(got, want, name)
        m = np.diff(np.asarray(kw["grp_off"]).astype(np.int64))
        assert got["stats"]["n_merges"] == int((m - 1).sum()) and got["stats"]["n_launches"] == 0


def test_thread_count_does_not_change_the_answer(U, merges, trees):
    for name in ("many", "widths"):
        same_merge(U.msa_merge(threads=7, **merges[name][0]), merges[name][1], name)
    for name in ("balanced_33", "several_groups"):
        same_msa(U.msa_progressive(threads=5, **trees[name][0]), trees[name][1], name)


def test_levels(U, trees):
    """a caterpillar gives m - 1 levels, a balanced tree ceil(log2 m)"""
    for m in GC.TREE_ROWS:
        assert U.msa_progressive(**trees["caterpillar_%d" % m][0])["stats"]["n_levels"] == m - 1
        assert U.msa_progressive(**trees["balanced_%d" % m][0])["stats"]["n_levels"] == int(np.ceil(np.log2(m)))


def path_cells(r):
    """the cells (1-based) a merge's path visits, with the op that reaches them"""
    i, j, out = int(r["is"]), int(r["js"]), []
    for w in r["runs"]:
        for _ in range(int(w) >> 2):
            op = int(w) & 3
            i += op != 2; j += op != 1
            out.append((i, j, op))
    return out


def test_the_cases_hold_what_they_are_for(merges):
    one = lambda name, k=0: (GC.tasks_of(merges[name][0])[k], merges[name][0])
    mats = lambda kw: [np.asarray(kw["SA"], np.int64), np.asarray(kw["S3"], np.int64)]
    kw = merges["widths"][0]
    assert sorted(zip(kw["Wa"], kw["Wb"])) == sorted((a, b) for a in GC.WIDTHS for b in GC.WIDTHS)
    for ma, mb in GC.ROWS:      # the floor division rounds a negative quotient
        (a, b), kw = one("rows_%d_%d" % (ma, mb))
        assert (a[0].shape[0], b[0].shape[0]) == (ma, mb)
        raw = sum(G.counts(a[t]) @ mats(kw)[t] @ G.counts(b[t]).T for t in range(2))
        if ma * mb > 1:
            assert ((raw < 0) & (raw % (ma * mb) != 0)).any(), (ma, mb)
            assert (G.cell_scores(a, b, mats(kw)) != np.trunc(raw / (ma * mb))).any()
    assert len(merges["many"][0]["ma"]) == 300
    # swapping the sides changes the answer
    x, y = merges["asymmetric"][1], merges["asymmetric_swapped"][1]
    assert int(np.asarray(merges["asymmetric"][0]["SA"]).max()) == 48 and int(np.asarray(merges["asymmetric"][0]["SA"]).min()) == -48
    assert int(x["score"][0]) != int(y["score"][0]) or list(x["runs"]) != list(y["runs"])
    # ties on the end cell and in the walk
    end_ties = walk_ties = 0
    kw, want = merges["ties"]
    uo = [int(v) for v in want["run_off"]]
    for k, (a, b) in enumerate(GC.tasks_of(kw)):
        s = G.cell_scores(a, b, mats(kw))
        H, E, F = G.dp(s, kw["gap_open"], kw["gap_ext"])
        Wa, Wb = s.shape
        cand = [int(H[Wa, j]) for j in range(Wb + 1)] + [int(H[i, Wb]) for i in range(Wa)]
        end_ties += cand.count(max(cand)) > 1
        r = {"is": want["is"][k], "js": want["js"][k], "runs": want["runs"][uo[k]:uo[k + 1]]}
        for i, j, op in path_cells(r):
            walk_ties += sum([H[i, j] == H[i - 1, j - 1] + s[i - 1, j - 1], H[i, j] == F[i, j], H[i, j] == E[i, j]]) > 1
    assert end_ties > 0 and walk_ties > 0
    assert merges["open_eq_ext"][0]["gap_open"] == merges["open_eq_ext"][0]["gap_ext"] > 0
    # all negative: the end cell is (Wa, 0), a's columns are followed by b's
    kw, want = merges["all_negative"]
    (a, b) = GC.tasks_of(kw)[0]
    Wa, Wb = kw["Wa"][0], kw["Wb"][0]
    assert (int(want["score"][0]), int(want["ie"][0]), int(want["je"][0]), int(want["is"][0]), int(want["js"][0])) == (0, Wa, 0, Wa, 0) and len(want["runs"]) == 0
    grid = want["cells"][0].reshape(3, Wa + Wb)
    assert np.array_equal(grid[:2, :Wa], a[0]) and (grid[:2, Wa:] == G.GAP).all() and np.array_equal(grid[2:, Wa:], b[0]) and (grid[2:, :Wa] == G.GAP).all()
    # overhangs on both ends, and a path between them
    want = merges["overhangs"][1]
    kw = merges["overhangs"][0]
    assert int(want["is"][0]) + int(want["js"][0]) > 0 and (kw["Wa"][0] - int(want["ie"][0])) + (kw["Wb"][0] - int(want["je"][0])) > 0 and len(want["runs"]) > 0
    assert 0 in merges["width_0"][0]["Wa"] and 0 in merges["width_0"][0]["Wb"]
    seen = set(np.concatenate(merges["letters"][0]["a"] + merges["letters"][0]["b"]).tolist()) - {G.GAP}
    assert seen == set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")


def check_msa(width, cells, rows, what):
    """every row without its gaps is the row's residues on both tracks, the tracks agree on gaps, no column is all gaps"""
    m = len(rows)
    grids = [c.reshape(m, width) for c in cells]
    assert np.array_equal(grids[0] == G.GAP, grids[1] == G.GAP), what
    if width:
        assert (grids[0] != G.GAP).any(axis=0).all(), what
    for r in range(m):
        for t in range(2):
            assert np.array_equal(grids[t][r][grids[t][r] != G.GAP], rows[r][t]), (what, r, t)


def test_properties(U, merges, trees):
    for name, (kw, _) in trees.items():
        got = U.msa_progressive(**kw)
        go, ro, o = [int(x) for x in kw["grp_off"]], [int(x) for x in kw["res_off"]], 0
        for g in range(len(go) - 1):
            m, W = go[g + 1] - go[g], int(got["width"][g])
            rows = [(kw["res"][0][ro[r]:ro[r + 1]], kw["res"][1][ro[r]:ro[r + 1]]) for r in range(go[g], go[g + 1])]
            check_msa(W, [c[o:o + m * W] for c in got["cells"]], rows, (name, g))
            o += m * W
    for name, (kw, _) in merges.items():      # a merge keeps both sides' rows and its runs are a path
        got = U.msa_merge(**kw)
        co, uo = [int(x) for x in got["cell_off"]], [int(x) for x in got["run_off"]]
        for k, (a, b) in enumerate(GC.tasks_of(kw)):
            W, ma = int(got["width"][k]), a[0].shape[0]
            rows = [(a[0][r][a[0][r] != G.GAP], a[1][r][a[1][r] != G.GAP]) for r in range(ma)] + [(b[0][r][b[0][r] != G.GAP], b[1][r][b[1][r] != G.GAP]) for r in range(b[0].shape[0])]
            check_msa(W, [c[co[k]:co[k + 1]] for c in got["cells"]], rows, (name, k))
            runs = got["runs"][uo[k]:uo[k + 1]]
            assert all((int(x) & 3) != (int(y) & 3) for x, y in zip(runs, runs[1:])) and all(int(x) >> 2 for x in runs)
            assert int(got["is"][k]) == 0 or int(got["js"][k]) == 0
            assert W == int(got["is"][k]) + int(got["js"][k]) + sum(int(x) >> 2 for x in runs) + kw["Wa"][k] - int(got["ie"][k]) + kw["Wb"][k] - int(got["je"][k])


def test_two_rows_score_their_residues(U):
    """m = 2, divisor 1: the cell score is SA + S3 of the two residues, so a merge of two single residues scores exactly that"""
    rng = np.random.default_rng(5)
    S = GC.matrices(rng)
    for _ in range(20):
        x, y = (int(v) for v in rng.integers(0, 21, 2)), (int(v) for v in rng.integers(0, 21, 2))
        x, y = list(x), list(y)
        a = [GC.LETTERS[[x[0]]].reshape(1, 1), GC.LETTERS[[x[1]]].reshape(1, 1)]
        b = [GC.LETTERS[[y[0]]].reshape(1, 1), GC.LETTERS[[y[1]]].reshape(1, 1)]
        s = int(S[0][x[0], y[0]]) + int(S[1][x[1], y[1]])
        assert int(G.cell_scores(a, b, [S[0].astype(np.int64), S[1].astype(np.int64)])[0, 0]) == s
        got = U.msa_merge(**GC.merge_kw([(a, b)], S, 30, 2))
        assert int(got["score"][0]) == max(s, 0) and int(got["width"][0]) == (1 if s >= 0 else 2)


def test_guide(U):
    for name, (go, tri, selfs) in GC.guide_cases().items():
        got = U.msa_guide(go, tri, selfs)
        t0 = 0
        for g in range(len(go) - 1):
            b, m = int(go[g]), int(go[g + 1] - go[g])
            D, ml = G.guide(tri[t0:t0 + m * (m - 1) // 2], selfs[b:b + m])
            t0 += m * (m - 1) // 2
            assert got["D"][g].tobytes() == np.array(D, np.float64).reshape(m, m).tobytes(), (name, g)
            assert [tuple(int(v) for v in p) for p in got["merges"][g]] == ml and G.check_merges(m, ml), (name, g)
        assert got["D"][2][0, 1] == 1.0 or got["D"][2][0, 2] == 1.0 or got["D"][1][0, 1] == 1.0      # the row with self score 0
        assert any((d == 0.0).sum() > len(d) for d in got["D"])                                        # a score above the self score clamps at 0


def test_self_scores(U):
    rng = np.random.default_rng(9)
    S = GC.matrices(rng)
    rows = GC.related(rng, 5, 30)
    ro = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])])
    got = U.msa_self_scores(ro, [np.concatenate([r[t] for r in rows]) for t in range(2)], S[1], S[0])
    assert [int(x) for x in got] == [G.self_score(r, S) for r in rows]


def test_refusals(U, merges, trees):
    def refused(fn, **kw):
        with pytest.raises(U.UcError) as ei:
            fn(**kw)
        assert ei.value.code == U.UC_ERR_ARGS, kw.keys()
    kw = trees["balanced_4"][0]
    refused(U.msa_progressive, **dict(kw, grp_off=[1, 5]))                                     # malformed offsets
    refused(U.msa_progressive, **dict(kw, grp_off=[0, 0, 4], merges=[np.zeros((0, 2), np.uint32), kw["merges"][0]]))
    bad = np.array(kw["res_off"]).copy(); bad[2] = bad[1] - 1
    refused(U.msa_progressive, **dict(kw, res_off=bad))
    for ml in ([(0, 1), (0, 2), (5, 3)], [(0, 1), (5, 2), (4, 3)], [(0, 0), (1, 2), (4, 3)], [(0, 1), (2, 3)], [(0, 1), (2, 3), (4, 7)]):      # not a tree over the group
        refused(U.msa_progressive, **dict(kw, merges=[np.array(ml, np.uint32)]))
    refused(U.msa_progressive, **dict(kw, gap_open=1, gap_ext=2))
    refused(U.msa_progressive, **dict(kw, gap_open=1, gap_ext=-1))
    big = np.array(kw["SA"]).copy(); big[3, 4] = 49
    refused(U.msa_progressive, **dict(kw, SA=big))
    # more than 8192 rows
    m = 8193
    refused(U.msa_progressive, grp_off=[0, m], res_off=np.arange(m + 1), res=[np.full(m, 65, np.uint8)] * 2, merges=[np.array(G.caterpillar(m), np.uint32)], SA=kw["SA"], S3=kw["S3"],
            gap_open=10, gap_ext=1)
    refused(U.msa_guide, grp_off=[0, m], scores=np.zeros(m * (m - 1) // 2, np.int32), self_scores=np.ones(m, np.int64))
    one = merges["rows_1_1"][0]
    refused(U.msa_merge, **dict(one, ma=[4097], mb=[4096], a=[np.full(4097 * 37, 65, np.uint8)] * 2, b=[np.full(4096 * 45, 65, np.uint8)] * 2))
    refused(U.msa_merge, **dict(one, gap_open=0, gap_ext=1))
    star = [c.copy() for c in one["a"]]; star[0][0] = ord("*")
    refused(U.msa_merge, **dict(one, a=star))
    gap = [c.copy() for c in one["a"]]; gap[1][0] = ord("-")      # the tracks disagree on a gap
    refused(U.msa_merge, **dict(one, a=gap))
    # the width limits: (Wa + Wb) max(open, 96) < 2^27 and Wa Wb < 2^31
    refused(U.msa_merge, **dict(one, gap_open=(1 << 27) // (37 + 45) + 1, gap_ext=0))
    W = (1 << 27) // 96 // 2 + 1
    refused(U.msa_merge, ma=[1], mb=[1], Wa=[W], Wb=[W], a=[np.full(W, 65, np.uint8)] * 2, b=[np.full(W, 65, np.uint8)] * 2, SA=one["SA"], S3=one["S3"], gap_open=10, gap_ext=1)
    refused(U.msa_progressive, grp_off=[0, 2], res_off=[0, W, 2 * W], res=[np.full(2 * W, 65, np.uint8)] * 2, merges=[np.array([(0, 1)], np.uint32)], SA=one["SA"], S3=one["S3"],
            gap_open=10, gap_ext=1)


def test_limits_hold_on_the_widths_not_on_the_leaf_sums(U):
    """1000 rows of 100 residues along a balanced tree: the top merge joins 512 and 488 rows whose residues sum to 51200 and 48800, a product beyond 2^31, while
    every node is about 100 columns wide.  The rule's limits are on the widths, so the call succeeds; a caterpillar over the same rows too."""
    m, L, kw = GC.leaf_sum_case()
    res, S = kw["res"], [kw["SA"], kw["S3"]]
    kw = dict(kw, threads=8)
    assert 512 * L * 488 * L >= 1 << 31
    for ml in (G.balanced(m), G.caterpillar(m)):
        got = U.msa_progressive(merges=[np.array(ml, np.uint32)], **kw)
        W = int(got["width"][0])
        assert L <= W < 2 * L and got["stats"]["n_merges"] == m - 1
        check_msa(W, got["cells"], [(res[0][r * L:(r + 1) * L], res[1][r * L:(r + 1) * L]) for r in range(m)], "1000 x 100")
    # the limits still hold where the widths themselves break them: two rows of W residues with 2 W x 96 >= 2^27
    W = (1 << 27) // 96 // 2 + 1
    with pytest.raises(U.UcError) as ei:
        U.msa_progressive(grp_off=[0, 2], res_off=[0, W, 2 * W], res=[np.full(2 * W, 65, np.uint8)] * 2, merges=[np.array([(0, 1)], np.uint32)], SA=S[0], S3=S[1], gap_open=10, gap_ext=1)
    assert ei.value.code == U.UC_ERR_ARGS


TREE_CODE = """
import sys, unicore_amd as U
try:
    U.tree(sys.argv[1], sys.argv[2], sys.argv[3], 50, aligner_options=sys.argv[4], aligner='progressive')
    print('ok')
except U.UcError as e:
    print('rc', e.code)
"""


def test_refusals_of_the_file_level(tmp_path):
    """gaps with open < extend are refused before a file is written or the device is asked for"""
    db = os.path.join(GOLD, "db")
    name = open(db + "_h", "rb").read().split(b"\n")[0].strip(b"\0").split()[0]
    (tmp_path / "prof").mkdir()
    (tmp_path / "prof" / "g1.txt").write_bytes(name + b"\ts1\n")
    r = subprocess.run([os.sys.executable, "-c", TREE_CODE, db, str(tmp_path / "prof"), str(tmp_path / "a"), "--gap-open 1 --gap-extend 2"],
                       env=dict(os.environ, PYTHONPATH=util.ROOT, UC_ALLOW_SYNTHETIC="1"), capture_output=True, text=True)
    assert r.stdout.strip() == "rc 2" and not os.path.exists(str(tmp_path / "a")), r.stderr


# ---- the CLI's parser
def cli(*args):
    return subprocess.run([UNICORE, "tree"] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1"), capture_output=True, text=True)


def test_cli_parser(tmp_path):
    db, prof, out = os.path.join(GOLD, "db"), str(tmp_path / "prof"), str(tmp_path / "o")
    h = cli("-h")
    assert h.returncode == 0 and "progressive" in h.stdout and "[star, profile]" in h.stdout and "--refine-iters <N>" in h.stdout and "[1 - 8]" in h.stdout
    r = cli("-n", "-a", "progressive", "--refine-iters", "2", db, prof, out)
    assert r.returncode == 1 and "--refine-iters" in r.stderr and "profile" in r.stderr and not os.path.exists(out)
    r = cli("-n", "-a", "progressiv", db, prof, out)
    assert r.returncode == 1 and "Unrecognized aligner" in r.stderr
    r = cli("-n", "-a", "mafft", db, prof, out)
    assert r.returncode == 1 and "external program" in r.stderr
    os.makedirs(out)
    open(os.path.join(out, "combined.fasta"), "w").write(">x\nA\n")
    for extra in (["-a", "progressive"], ["--aligner=progressive"]):
        r = cli("-n", *extra, db, prof, out)
        assert r.returncode == 0 and r.stdout == "Concatenated alignment file %s/combined.fasta already exists, skipping alignment step\n" % out, r.stderr


# ---- the committed fixture
def test_golden_is_what_the_reference_gives(O):
    prof = json.load(open(os.path.join(GOLD, "profile_default_t80.json")))
    genes = {k: v.encode("ascii") for k, v in prof.items() if k.endswith(".txt")}
    gold, star = json.load(open(os.path.join(GOLD, "tree_progressive_d50.json"))), json.load(open(os.path.join(GOLD, "tree_default_d50.json")))
    files, info = G.tree_files(O, util.oracle_params(O, R.FIXED_OPTS), os.path.join(GOLD, "db"), genes, 50)
    assert R.digest(files) == gold and len(info) == 11
    assert gold["combined.fasta"] != star["combined.fasta"] and set(gold["sha256"]) == set(star["sha256"])
    for gene, v in info.items():      # every residue is in the MSA
        rows = [l for l in files["fasta/%s/%s.fa" % (gene, gene)].split(b"\n")[1::2]]
        raw = [l for l in files["fasta/%s/aa.fasta" % gene].split(b"\n")[1::2]]
        assert [r.replace(b"-", b"") for r in rows] == raw and all(len(r) == v["width"] for r in rows), gene


def test_header_binding_and_abi(U):
    import ctypes as C
    hdr = open(os.path.join(util.ROOT, "include", "unicore_cluster.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in hdr and name in U.SYMBOLS and hasattr(U.lib(), name), name
    assert "#define UC_ABI_VERSION 9" in hdr and U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "#define UC_TREE_PROGRESSIVE_NPHASE 3" in hdr and len(U.TREE_PROGRESSIVE_PHASES) == 3
    assert C.sizeof(U.UcTreeProgressiveStats) == C.sizeof(U.UcTreeStats) + 7 * 8 + 3 * 8 and C.sizeof(U.UcMsaProgressiveStats) == 4 * 8
    g = U.msa_progressive_geometry()
    assert g == {"chunk": 64, "cap": 0, "task_bytes_per_cell": 2}
    with pytest.raises(ValueError):
        U.tree("a", "b", "c", aligner="progressiv")


# ---- the host twin under the sanitizers, in a program of its own
def test_host_twin_under_sanitizers(tmp_path):
    csrc = os.path.join(util.ROOT, "unicore_amd", "csrc")
    exe = str(tmp_path / "msa_progressive_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-pthread",
                         "-I" + os.path.join(util.ROOT, "include"), "-I" + csrc, os.path.join(util.ROOT, "tests", "msa_progressive_host_check.cpp"),
                         os.path.join(csrc, "uc_msa_progressive_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert run.stdout.strip() == "msa_progressive_host_check: ok"
