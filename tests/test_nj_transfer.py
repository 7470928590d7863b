"""Rule UC-N/T (transfer bootstrap support of the tree builder `nj`) without a GPU: the host twin (uc_nj_transfer) and the labelled
line (uc_nj_newick_transfer) against the plain-Python reference (nj_transfer_ref.py) on the shared tree shapes (nj_transfer_cases.py), the hand
example of the rule, the zeros of phi against uc_nj_support, every refusal, uc_tree_infer_support and the CLI under UC_TREE_HOST=1 against the
reference and the committed fixture tests/golden/nj_transfer.json, and the host sources under the address and undefined-behaviour sanitizers in a
program of their own (nj_transfer_host_check.cpp).  The HIP kernels: test_nj_transfer_gpu.py."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import nj_boot_cases as BC
import nj_boot_ref as BR
import nj_cases as NC
import nj_transfer_cases as TC
import nj_transfer_ref as TR
import util

GOLD = os.path.join(util.ROOT, "tests", "golden")
UNICORE = os.path.join(util.ROOT, "bin", "unicore")
NEW_SYMBOLS = ("uc_nj_transfer", "uc_nj_transfer_dev", "uc_nj_newick_transfer", "uc_nj_transfer_geometry", "uc_tree_infer_support")


@pytest.fixture(scope="module")
def U():
    import unicore_amd
    unicore_amd.lib()
    return unicore_amd


def phi_sums(phi):
    return np.asarray(phi, np.uint64).reshape(len(phi), -1).sum(0, dtype=np.uint64)


# ---- the rule by hand
def test_hand_example(U):
    n, names = 7, TC.HAND_NAMES
    sets = TR.leaf_sets(n, TC.HAND_MAIN)
    assert sets == [frozenset({0, 1}), frozenset({0, 1, 2}), frozenset({4, 5}), frozenset({4, 5, 6})] and TR.light(n, TC.HAND_MAIN) == [2, 3, 2, 3]
    abc = sets[1]
    for y in TR.leaf_sets(n, TC.HAND_ABD) + TR.leaf_sets(n, TC.HAND_AB_ONLY):      # the distance is counted on the sets themselves
        assert TR.delta(n, abc, y) == min(len(abc ^ y), n - len(abc ^ y))
    # one replicate holds {a, b, c}, the other {a, b} but not {a, b, c}: phi = 0 and 1, den = 2 (3 - 1) = 4, the label (200 x 3 + 4) div 8 = 75
    reps = [TC.HAND_HOLDS, TC.HAND_AB_ONLY]
    phi, light = U.nj_transfer(n, TC.HAND_MAIN, *TC.arrays(reps))
    assert phi.dtype == light.dtype == np.uint32 and phi.tolist() == [[0, 0, 0, 0], [0, 1, 0, 0]] == TR.transfer(n, TC.HAND_MAIN, reps)[0] and light.tolist() == [2, 3, 2, 3]
    assert TR.labels(phi.tolist(), light.tolist(), 2) == [100, 75, 100, 100]
    line = U.nj_newick(names, TC.HAND_MAIN, None, 2, light=light, phi_sum=phi_sums(phi))
    assert line == TR.newick(names, TC.HAND_MAIN, light.tolist(), phi_sums(phi).tolist(), 2)
    assert line == "(((a:1.000000,b:1.000000)100:1.000000,c:1.000000)75:1.000000,d:1.000000,((e:1.000000,f:1.000000)100:1.000000,g:1.000000)100:1.000000);\n"
    # a replicate whose nearest split is {a, b, d}: h = 2, capped at 2 - it contributes nothing
    assert min(TR.delta(n, abc, y) for y in TR.leaf_sets(n, TC.HAND_ABD)) == 2 and frozenset({0, 1, 3}) in TR.leaf_sets(n, TC.HAND_ABD)
    phi3, _ = U.nj_transfer(n, TC.HAND_MAIN, *TC.arrays([TC.HAND_ABD]))
    assert phi3.tolist() == TR.transfer(n, TC.HAND_MAIN, [TC.HAND_ABD])[0] and phi3[0, 1] == 2
    assert U.nj_newick(names, TC.HAND_MAIN, None, 1, light=light, phi_sum=phi_sums(phi3)).count(")0:") >= 1
    # rounding half up: den = 4 replicates x (2 - 1): 1/4 away -> 75, 1/8 away -> 88 (87.5 up), 199/200 away -> 1 (0.5 up)
    four = BC.FOUR_AB
    for B, total, label in ((4, 1, 75), (8, 1, 88), (200, 199, 1), (3, 1, 67), (3, 2, 33), (1, 1, 0)):
        assert U.nj_newick(list("abcd"), four, None, B, light=[2], phi_sum=[total]) == "((a:0.100000,b:0.200000)%d:0.050000,c:0.300000,d:0.400000);\n" % label
    # B = 0: the unlabelled line byte for byte, with or without arrays; N = 3: no internal branch, no label
    assert U.nj_newick(names, TC.HAND_MAIN, None, 0, light=light, phi_sum=phi_sums(phi)) == U.nj_newick(names, TC.HAND_MAIN)
    D = NC.random_matrix(random.Random(3), 3)
    assert U.nj_newick(list("abc"), U.nj_join(D), None, 5, light=[], phi_sum=[]) == U.nj_newick(list("abc"), U.nj_join(D))
    assert U.nj_transfer(3, U.nj_join(D), np.zeros((5, 0), np.uint32), np.zeros((5, 0), np.uint32))[0].shape == (0, 0)


# ---- twin == reference, zeros == support, TBE >= FBP
def sizes(U):
    g = U.nj_transfer_geometry()
    T, C = g["tile"], g["chunk"]
    assert T >= 16 and C >= 1
    return [4, 5, 6, 9, 32, 33, 64, 65, T - 1 + 3, T + 3, T + 1 + 3, 2 * T + 1 + 3, 32 * C + 1]


def check(U, n, main, reps, want, threads):
    ra, rb = TC.arrays(reps)
    phi, light = U.nj_transfer(n, main, ra, rb, threads=threads)
    assert phi.shape == (len(reps), n - 3) and phi.tolist() == want[0] and light.tolist() == want[1], n
    assert (light >= 2).all() and (phi <= light - 1).all()
    sup = U.nj_support(n, main, ra, rb)
    assert np.array_equal((phi == 0).sum(0), sup) and sup.tolist() == BR.support(n, main, reps), n      # phi == 0 exactly when the replicate holds the split
    B = len(reps)
    tbe, fbp = TR.labels(phi.tolist(), light.tolist(), B), [(200 * int(s) + B) // (2 * B) for s in sup]
    assert all(t >= f for t, f in zip(tbe, fbp)), n
    names = ["l%d" % i for i in range(n)]
    line = U.nj_newick(names, main, None, B, light=light, phi_sum=phi_sums(phi))
    assert line == TR.newick(names, main, light.tolist(), phi_sums(phi).tolist(), B), n
    return phi


@pytest.mark.parametrize("k", range(13))
def test_twin_against_reference(U, k):
    n = sizes(U)[k]
    main, reps = TC.case(n)
    phi = check(U, n, main, reps, TC.reference(n), 1 + k % 3)
    assert (phi[0] == 0).all() and phi[1].max() <= 1 and phi[5].max() <= 1      # a copy of the main tree; one leaf regrafted
    if n > 8:
        assert phi[2].max() > 1                                                 # an unrelated tree


@pytest.mark.parametrize("shape", ("caterpillar", "balanced", "random"))
def test_twin_on_shapes(U, shape):
    T = U.nj_transfer_geometry()["tile"]
    for n in (8, T - 1 + 3, T + 1 + 3):
        main, reps = TC.shaped_case(n, shape)
        phi = check(U, n, main, reps, TR.transfer(n, main, reps), 2)
        assert (phi[-1] == 0).all() and phi[-2].max() <= 1
        if shape != "random" and n > 8:
            assert (phi[:3].min(0) >= 4).any()      # a deep split far from every split of the unrelated replicates


def test_child_order_and_side_do_not_matter(U):
    n = 40
    main, reps = TC.case(n)
    ra, rb = TC.arrays(reps)
    want, light = U.nj_transfer(n, main, ra, rb)
    phi, l2 = U.nj_transfer(n, main, rb, ra)                                    # every replicate join written the other way round
    assert np.array_equal(phi, want) and np.array_equal(light, l2)
    swapped = dict(main, join_a=main["join_b"], join_b=main["join_a"])
    assert np.array_equal(U.nj_transfer(n, swapped, ra, rb)[0], want)


# ---- refusals
def refused(U, fn, *a, **kw):
    with pytest.raises(U.UcError) as ei:
        fn(*a, **kw)
    assert ei.value.code == U.UC_ERR_ARGS, (a, kw)


def refusals(U, device):
    """what uc_nj_transfer / uc_nj_transfer_dev refuse before any work (test_nj_transfer_gpu.py calls this with a device)"""
    ab, one = BC.FOUR_AB, ([[0]], [[1]])
    refused(U, U.nj_transfer, 4, dict(ab, join_b=[0]), *one, device=device)              # the main tree joins a node twice
    refused(U, U.nj_transfer, 4, dict(ab, join_b=[4]), *one, device=device)              # ... a node before it exists
    refused(U, U.nj_transfer, 4, ab, [[0]], [[0]], device=device)                        # a replicate that is no tree
    refused(U, U.nj_transfer, 4, ab, [[0]], [[5]], device=device)
    main, reps = TC.case(9)
    ra, rb = TC.arrays(reps)
    bad = ra.copy()
    bad[-1, 3] = bad[-1, 2]                                                              # the last replicate joins a node twice
    refused(U, U.nj_transfer, 9, main, bad, rb, device=device)
    bad = rb.copy()
    bad[2, 1] = 9 + 1                                                                    # node 10 does not exist at step 1
    refused(U, U.nj_transfer, 9, main, ra, bad, device=device)
    L = U.lib()
    z = np.zeros(4, np.uint32)
    fn = (lambda *a: L.uc_nj_transfer(*a)) if device is None else (lambda *a: L.uc_nj_transfer_dev(device, *a))
    for n, n_rep in ((1, 1), (16385, 1), (0, 0), (4, 100001)):                           # N and B out of range
        assert fn(n, z.ctypes.data, z.ctypes.data, n_rep, z.ctypes.data, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data) == U.UC_ERR_ARGS, (n, n_rep)
    assert fn(4, None, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data) == U.UC_ERR_ARGS
    assert fn(4, z.ctypes.data, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data, 1, None, z.ctypes.data) == U.UC_ERR_ARGS


def test_refusals(U, tmp_path, monkeypatch):
    refusals(U, None)
    names, ab = list("abcd"), BC.FOUR_AB
    refused(U, U.nj_newick, names, ab, None, 2, light=[2], phi_sum=[3])                  # phi_sum above den = 2 x (2 - 1)
    assert U.nj_newick(names, ab, None, 2, light=[2], phi_sum=[2]).count(")0:") == 1
    refused(U, U.nj_newick, names, ab, None, 2, light=[1], phi_sum=[0])                  # no light side of one leaf
    refused(U, U.nj_newick, names, ab, None, 2, light=[3], phi_sum=[0])                  # ... or of more than half
    refused(U, U.nj_newick, names, ab, None, 2, light=[2], phi_sum=None)
    refused(U, U.nj_newick, names, ab, None, 2, light=None, phi_sum=[0])
    refused(U, U.nj_newick, names, ab, None, 100001, light=[2], phi_sum=[0])
    refused(U, U.nj_newick, names, dict(ab, join_b=[0]), None, 2, light=[2], phi_sum=[0])
    with pytest.raises(ValueError):
        U.nj_newick(names, ab, [1], 2, light=[2], phi_sum=[0])
    monkeypatch.setenv("UC_TREE_HOST", "1")
    (tmp_path / "in.fa").write_text(">a\nACDE\n>b\nACDF\n>c\nCCDE\n>d\nACDA\n")
    src, out = str(tmp_path / "in.fa"), str(tmp_path / "o.nwk")
    for boot in (0, 3):                                                                  # an unknown mode, with or without replicates
        refused(U, U.tree_infer, src, out, bootstrap=boot, support="tbe2")
        refused(U, U.tree_infer, src, out, bootstrap=boot, support=None)
    assert U.lib().uc_tree_infer_support(src.encode(), out.encode(), None, 3, 1, 2, None, None) == U.UC_ERR_ARGS
    assert U.lib().uc_tree_infer_support(src.encode(), out.encode(), None, 100001, 1, 1, None, None) == U.UC_ERR_ARGS
    refused(U, U.tree_infer, src, out, "jc69", bootstrap=3, support="tbe")
    assert not os.path.exists(out)
    U.tree_infer(src, out, support="tbe")                                                # without replicates: accepted and unused
    U.tree_infer(src, str(tmp_path / "plain.nwk"))
    assert open(out, "rb").read() == (tmp_path / "plain.nwk").read_bytes()


# ---- the file level through the host twins
def golden_fasta():
    return json.load(open(os.path.join(GOLD, "tree_default_d50.json")))["combined.fasta"]


def test_tree_infer_tbe_host_on_the_golden_alignment(U, tmp_path, monkeypatch):
    monkeypatch.setenv("UC_TREE_HOST", "1")
    fasta, gold = golden_fasta(), json.load(open(os.path.join(GOLD, "nj_transfer.json")))
    (tmp_path / "combined.fasta").write_text(fasta)
    src = str(tmp_path / "combined.fasta")
    B, seed = gold["bootstrap"], gold["seed"]
    ref = TR.transfer_of_fasta(fasta, B, seed)
    assert B == 12 and {k: ref[k] for k in ("nwk", "support", "light", "phi_sum", "tsv", "boottrees")} == {
        "nwk": gold["nj.nwk"], "support": gold["support"], "light": gold["light"], "phi_sum": gold["phi_sum"], "tsv": gold["boot.tsv"], "boottrees": gold["boottrees"]}
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    for threads, budget in ((1, None), (3, "200")):      # a budget of one replicate per batch: the same files
        if budget:
            monkeypatch.setenv("UC_TREE_BUDGET_BYTES", budget)
        st = U.tree_infer(src, str(tmp_path / "t.nwk"), bootstrap=B, seed=seed, threads=threads, support="tbe")
        assert (tmp_path / "t.nwk").read_text() == gold["nj.nwk"] and (tmp_path / "t.nwk.boot.tsv").read_text() == gold["boot.tsv"]
        assert (tmp_path / "t.nwk.boottrees").read_text() == gold["boottrees"] and os.path.exists(tmp_path / "t.nwk.dist.tsv")
        assert st["n_batches"] == (B if budget else 1) and st["support_sum"] == sum(gold["support"]) and st["support_min"] == min(gold["support"])      # their FBP meaning
        assert st["n_replicates"] == B and set(st["seconds"]) == set(U.NJ_BOOT_PHASES)
    monkeypatch.delenv("UC_TREE_BUDGET_BYTES")
    # support="fbp" and the old call: the same bytes in every file, and the same main tree under the tbe labels
    U.tree_infer(src, str(tmp_path / "f.nwk"), bootstrap=B, seed=seed, support="fbp")
    U.tree_infer(src, str(tmp_path / "o.nwk"), bootstrap=B, seed=seed)
    assert U.lib().uc_tree_infer_support(src.encode(), str(tmp_path / "c.nwk").encode(), None, B, seed, 0, None, None) == 0
    for ext in ("", ".boot.tsv", ".boottrees", ".dist.tsv"):
        assert (tmp_path / ("f.nwk" + ext)).read_bytes() == (tmp_path / ("o.nwk" + ext)).read_bytes() == (tmp_path / ("c.nwk" + ext)).read_bytes(), ext
    assert (tmp_path / "o.nwk").read_text() == BR.boot_of_fasta(fasta, B, seed)["nwk"]
    strip = lambda s: __import__("re").sub(r"\)\d+:", "):", s)
    assert strip(gold["nj.nwk"]) == strip((tmp_path / "o.nwk").read_text()) == json.load(open(os.path.join(GOLD, "nj_default.json")))["nj.nwk"]
    assert (tmp_path / "o.nwk.boot.tsv").read_text() == "".join("%d\t%d\n" % (s, v) for s, v in enumerate(gold["support"]))
    # B = 0 in mode tbe: the plain line
    assert U.lib().uc_tree_infer_support(src.encode(), str(tmp_path / "z.nwk").encode(), None, 0, seed, 1, None, None) == 0
    assert (tmp_path / "z.nwk").read_text() == strip(gold["nj.nwk"]) and not os.path.exists(tmp_path / "z.nwk.boot.tsv")


def test_tree_infer_tbe_host_on_evolved_rows(U, tmp_path, monkeypatch):
    """more splits than the golden alignment's two: nine and twenty rows, both models"""
    monkeypatch.setenv("UC_TREE_HOST", "1")
    monkeypatch.setenv("UC_TREE_DUMP", "1")
    for n, w, model, B in ((9, 80, "kimura", 12), (20, 60, "p", 7), (3, 10, "kimura", 4)):
        text = BC.fasta_of(["t%d" % i for i in range(n)], NC.evolved_rows(random.Random(78 + n), n, w, rate=0.3))
        (tmp_path / "in.fa").write_text(text)
        ref = TR.transfer_of_fasta(text, B, 3, model)
        st = U.tree_infer(str(tmp_path / "in.fa"), str(tmp_path / "o.nwk"), model, bootstrap=B, seed=3, threads=2, support="tbe")
        assert (tmp_path / "o.nwk").read_text() == ref["nwk"] and (tmp_path / "o.nwk.boot.tsv").read_text() == ref["tsv"] and (tmp_path / "o.nwk.boottrees").read_text() == ref["boottrees"]
        assert st["support_sum"] == sum(ref["support"]) and st["support_min"] == (min(ref["support"]) if ref["support"] else 0)
        if n == 9:
            assert 0 < sum(ref["phi_sum"]) and any(0 < l < 100 for l in ref["labels"])


# ---- the CLI
def cli(*args, env=None):
    return subprocess.run([UNICORE] + list(args), env=dict(os.environ, UC_ALLOW_SYNTHETIC="1", **(env or {})), capture_output=True, text=True)


def test_cli_parser(tmp_path):
    db, prof, out = os.path.join(GOLD, "db"), str(tmp_path / "prof"), str(tmp_path / "o")
    for cmd in ("tree", "gene-tree"):
        r = cli(cmd, "-h")
        assert r.returncode == 0 and "--support fbp|tbe" in r.stdout and "--bootstrap" in r.stdout
    for opts, word in (("--support", "--support"), ("--support tbe2", "tbe2"), ("--support=TBE", "TBE"), ("--bootstrap 3 --support", "--support"), ("--support= --seed 1", "--support"),
                       ("--support fbp,tbe", "fbp,tbe"), ("--supports tbe", "--supports")):
        r = cli("tree", "-t", "nj", "-p", opts, db, prof, out)
        assert r.returncode == 1 and word in r.stderr and not os.path.exists(out), (opts, r.stderr)
        r = cli("tree", "-n", "-t", "nj", "-p", opts, db, prof, out)                      # refused with -n too: the word is wrong either way
        assert r.returncode == 1 and word in r.stderr and not os.path.exists(out), (opts, r.stderr)
    os.makedirs(out)
    open(os.path.join(out, "combined.fasta"), "w").write(">x\nAC\n>y\nAD\n>z\nCC\n>w\nCD\n")
    r = cli("tree", "-n", "-t", "nj", "-p", "--bootstrap=10 --support=tbe --model p", db, prof, out)      # -n: parsed and not run
    assert r.returncode == 0 and sorted(os.listdir(out)) == ["combined.fasta"]
    os.makedirs(os.path.join(out, "fasta", "g1"))
    r = cli("gene-tree", "-t", "nj", "-p", "--support transfer", out)
    assert r.returncode == 1 and "transfer" in r.stderr and os.listdir(os.path.join(out, "fasta", "g1")) == []


def test_cli_tbe_with_the_host_twin(tmp_path):
    out = tmp_path / "o"
    (out / "fasta" / "gA").mkdir(parents=True)
    (out / "fasta" / "gB").mkdir()
    text = BC.fasta_of(["t%d" % i for i in range(8)], NC.evolved_rows(random.Random(77), 8, 60))
    small = ">x\nAC\n>y\nAD\n>z\nCC\n"                                                   # three rows: no internal branch, no label
    (out / "combined.fasta").write_text(text)
    (out / "fasta" / "gA" / "gA.fa.filtered").write_text(text)
    (out / "fasta" / "gB" / "gB.fa.filtered").write_text(small)
    env = {"UC_TREE_HOST": "1"}
    db, none = os.path.join(GOLD, "db"), str(tmp_path / "none")
    r = cli("tree", "-t", "nj", db, none, str(out), env=env)
    plain = (out / "nj.nwk").read_bytes()
    assert r.returncode == 0
    for opts in ("--support tbe", "--support=tbe --seed 4", "--support fbp", "--bootstrap 0 --support tbe"):      # without replicates: accepted and unused
        r = cli("tree", "-t", "nj", "-p", opts, db, none, str(out), env=env)
        assert r.returncode == 0 and r.stderr == "" and (out / "nj.nwk").read_bytes() == plain and sorted(os.listdir(out)) == ["combined.fasta", "fasta", "nj.nwk", "tree.chk"]
    r = cli("tree", "-t", "nj", "-p", "--bootstrap 12 --seed 3 --support tbe", "-c", "2", db, none, str(out), env=dict(env, UC_TREE_DUMP="1"))
    ref = TR.transfer_of_fasta(text, 12, 3)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert (out / "nj.nwk").read_text() == ref["nwk"] != plain.decode() and (out / "tree.chk").read_text() == "1"
    assert (out / "nj.nwk.boot.tsv").read_text() == ref["tsv"] and (out / "nj.nwk.boottrees").read_text() == ref["boottrees"]
    # fbp by name and by default: the same bytes as before the option
    want = BR.boot_of_fasta(text, 12, 3)["nwk"]
    for opts in ("--bootstrap 12 --seed 3 --support fbp", "--bootstrap 12 --seed 3", "--support=tbe --bootstrap 12 --seed 3 --support=fbp"):
        r = cli("tree", "-t", "nj", "-p", opts, db, none, str(out), env=env)
        assert r.returncode == 0 and (out / "nj.nwk").read_text() == want, opts
    r = cli("gene-tree", "-t", "nj", "-p", "--bootstrap 12 --seed 3 --model p --support tbe", str(out), env=env)
    assert r.returncode == 0 and r.stdout.endswith("\nInferring gene specific phylogenetic trees 2/2...Done\n"), r.stdout + r.stderr
    assert (out / "fasta" / "gA" / "nj.nwk").read_text() == TR.transfer_of_fasta(text, 12, 3, "p")["nwk"]
    assert (out / "fasta" / "gB" / "nj.nwk").read_text() == TR.transfer_of_fasta(small, 12, 3, "p")["nwk"]


def test_header_binding_and_abi(U):
    hdr = open(os.path.join(util.ROOT, "include", "unicore_cluster.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in hdr and name in U.SYMBOLS and hasattr(U.lib(), name), name
    assert "#define UC_ABI_VERSION 9" in hdr and U.ABI_VERSION == 9 and U.lib().uc_abi_version() == 9
    assert "#define UC_NJ_BOOT_NPHASE 7" in hdr and len(U.NJ_BOOT_PHASES) == 7
    assert "#define UC_NJ_SUPPORT_FBP 0" in hdr and "#define UC_NJ_SUPPORT_TBE 1" in hdr and U.NJ_SUPPORT_MODES == {"fbp": 0, "tbe": 1}
    g = U.nj_transfer_geometry()
    assert g["tile"] % 4 == 0 and g["tile"] >= 16 and g["chunk"] >= 1


# ---- the host sources under the sanitizers, in a program of their own
def test_host_sources_under_sanitizers(tmp_path):
    csrc = os.path.join(util.ROOT, "unicore_amd", "csrc")
    exe = str(tmp_path / "nj_transfer_host_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-pthread",
                         "-I" + os.path.join(util.ROOT, "include"), "-I" + csrc, os.path.join(util.ROOT, "tests", "nj_transfer_host_check.cpp"),
                         os.path.join(csrc, "uc_nj_host.cpp"), os.path.join(csrc, "uc_nj_boot_host.cpp"), os.path.join(csrc, "uc_nj_transfer_host.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert run.stdout.strip() == "nj_transfer_host_check: ok"
