"""The progressive MSA of `unicore tree -a progressive` (rule UC-T/G) in figures: python tools/msa_progressive_time.py [genes] [rows]
  speed    cells per second of the score kernel and of the DP kernel (their own times, from the UC_TIMING line) and of the whole device call against the
           host twin (1 and 16 threads), on `genes` synthetic groups (default 500) of `rows` rows (default 51) with the lengths of util.family_db
           (20 .. 260), merged along balanced merge lists (genes x (rows - 1) tasks: 25,000)
  cost     wall time of uc_tree with the star, profile and progressive aligners, launches and levels, on the golden database and on family_dbs with
           indels, fragments and unequal lengths
  quality  the sum-of-pairs score of the three aligners' MSAs (both tracks, the engine's matrices and gaps), same inputs
Needs one GPU.  Everything it prints goes into profiles/msa_progressive/README.md by hand."""
import json
import os
import re
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")

import numpy as np

import matrix_cases as MC
import msa_profile_cases as PC
import msa_profile_ref as P
import msa_progressive_ref as G
import unicore_amd as U
import util
from oracle import oracle_py as O

n_genes = int(sys.argv[1]) if len(sys.argv) > 1 else 500
n_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 51


def timed_stderr(fn):
    """(result, seconds, what the library wrote to stderr meanwhile)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t = time.perf_counter(); r = fn(); dt = time.perf_counter() - t
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        return r, dt, f.read().decode()


# ---- speed
rng = np.random.default_rng(7)
S3, SA = MC.base(O)
t0 = time.perf_counter()
rows = [r for _ in range(n_genes) for _, r in PC.family(rng, int(rng.integers(20, 261)), n_rows)]
kw = dict(grp_off=np.arange(n_genes + 1) * n_rows, res_off=np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.uint64),
          res=[np.concatenate([np.asarray(r[t], np.uint8) for r in rows]) for t in range(2)], merges=[np.array(G.balanced(n_rows), np.uint32)] * n_genes, S3=S3, SA=SA,
          gap_open=10, gap_ext=1)
print("speed: %d groups x %d rows, balanced merge lists (input built in %.1f s)" % (n_genes, n_rows, time.perf_counter() - t0), flush=True)
os.environ["UC_TIMING"] = "1"
for rep in range(3):
    dev, dt, err = timed_stderr(lambda: U.msa_progressive(device=0, **kw))
    cells = dev["stats"]["n_cells"]
    sc, dp = float(re.search(r"score kernel ([0-9.]+) ms", err).group(1)), float(re.search(r"DP kernel ([0-9.]+) ms", err).group(1))
    print("  device pass %d: %d merges, %d levels, %d launches, %.3g cells; call %.3f s (%.3g cells/s), score kernel %.2f ms (%.3g cells/s), DP kernel %.2f ms (%.3g cells/s)" % (
        rep, dev["stats"]["n_merges"], dev["stats"]["n_levels"], dev["stats"]["n_launches"], cells, dt, cells / dt, sc, cells / (sc / 1e3), dp, cells / (dp / 1e3)), flush=True)
os.environ.pop("UC_TIMING")
for threads in (1, 16):
    t = time.perf_counter(); host = U.msa_progressive(threads=threads, **kw); dt = time.perf_counter() - t
    same = np.array_equal(dev["width"], host["width"]) and all(np.array_equal(x, y) for x, y in zip(dev["cells"], host["cells"]))
    print("  host twin, %d thread(s): %.3f s (%.3g cells/s); same answers: %s" % (threads, dt, cells / dt, same), flush=True)


# ---- cost and quality
def msa_of(out):
    """{gene: [aa grid, 3di grid]} of an output directory"""
    r = {}
    for gene in sorted(os.listdir(os.path.join(out, "fasta"))):
        rd = lambda p: np.array([np.frombuffer(l, np.uint8) for l in open(p, "rb").read().split(b"\n")[1::2]])
        d = os.path.join(out, "fasta", gene)
        if os.path.exists(os.path.join(d, gene + ".fa")):
            r[gene] = [rd(os.path.join(d, gene + ".fa")), rd(os.path.join(d, gene + "_3di.fa"))]
    return r


def run(label, db, prof):
    p = O.default_params()
    mats = [np.array(p.SA[:], np.int64).reshape(21, 21), np.array(p.S3[:], np.int64).reshape(21, 21)]
    wd = tempfile.mkdtemp()
    for name, kwargs in (("star", {}), ("profile, 1 round", dict(aligner="profile", refine_iters=1)), ("progressive", dict(aligner="progressive"))):
        walls = []
        for rep in range(3):
            out = os.path.join(wd, "o")
            shutil.rmtree(out, ignore_errors=True)
            t = time.perf_counter(); st = U.tree(db, prof, out, 50, verbosity=0, device=0, **kwargs); walls.append(time.perf_counter() - t)
        msas = msa_of(out)
        sp = sum(P.sum_of_pairs(g, mats, p.gap_open, p.gap_ext) for g in msas.values())
        residues = sum(int((g[0] != P.GAP).sum()) for g in msas.values())
        extra = ""
        if "progressive" in st:
            pg = st["progressive"]
            extra = "; guide %.3f s, merges %.3f s, %d merges, %d levels, %d launches (%.1f per level), %.3g cells" % (
                pg["seconds"]["guide"], pg["seconds"]["merges"], pg["n_merges"], pg["n_levels"], pg["n_launches"], pg["n_launches"] / max(pg["n_levels"], 1), pg["n_cells"])
        print("  %s, %s: wall min %.3f s of 3 (%s); columns %d, kept %d, rows unaligned %d, residues in the MSA %d; sum of pairs %d%s" % (
            label, name, min(walls), " ".join("%.3f" % w for w in walls), st["n_columns"], st["n_columns_kept"], st["n_rows_unaligned"], residues, sp, extra), flush=True)
    shutil.rmtree(wd, ignore_errors=True)


def family_input(wd, tag, seed, fragments, **kw):
    """a family database, every family a gene, every member a species; fragments: every third member keeps a random half of its residues"""
    s3, sa = util.family_db(seed, n_fam=40, members=12, with_x=False, **kw)
    if fragments:
        rng = np.random.default_rng(seed)
        for k in range(0, 40 * 12, 3):
            n = len(s3[k])
            lo = int(rng.integers(0, n // 2 + 1))
            s3[k], sa[k] = s3[k][lo:lo + max(n // 2, 1)], sa[k][lo:lo + max(n // 2, 1)]
    names = util.write_db(os.path.join(wd, tag), s3, sa)
    prof = os.path.join(wd, tag + "_prof")
    os.makedirs(prof)
    for f in range(40):
        open(os.path.join(prof, "fam%02d.txt" % f), "w").write("".join("%s\tsp%d\n" % (names[f * 12 + m], m) for m in range(12)))
    return os.path.join(wd, tag), prof


gold = os.path.join(ROOT, "tests", "golden")
wd = tempfile.mkdtemp()
prof = os.path.join(wd, "prof")
os.makedirs(prof)
for k, v in json.load(open(os.path.join(gold, "profile_default_t80.json"))).items():
    open(os.path.join(prof, k), "w").write(v)
print("cost and quality:", flush=True)
run("golden database, 11 genes", os.path.join(gold, "db"), prof)
run("family_db indel 0.08, 40 genes x 12 rows", *family_input(wd, "fdb", 11, False, indel=0.08))
run("family_db indel 0.08 with fragments (every third row a random half), 40 genes x 12 rows", *family_input(wd, "frag", 11, True, indel=0.08))
shutil.rmtree(wd, ignore_errors=True)
