"""The profile refinement of `unicore tree -a profile` (rule UC-T/P) in figures: python tools/msa_profile_time.py [genes] [rows]
  speed    cells per second of the DP kernel (its own time, from the UC_TIMING line) and of the whole device call against the host twin (1 and 16
           threads), on `genes` synthetic groups (default 500) of `rows` rows (default 50) with the lengths of util.family_db (20 .. 260)
  cost     wall time of uc_tree with the star aligner and with 1 and 2 rounds, on the golden database and on a family_db with indels
  quality  the sum-of-pairs score of the MSAs (both tracks, the engine's matrices and gaps) for the star and after every round, same inputs
Needs one GPU.  Everything it prints goes into profiles/msa_profile/README.md by hand."""
import os
import re
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")
import json

import numpy as np

import matrix_cases as MC
import msa_profile_cases as PC
import msa_profile_ref as P
import unicore_amd as U
import util
from oracle import oracle_py as O

n_genes = int(sys.argv[1]) if len(sys.argv) > 1 else 500
n_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 50


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
kw = PC.case([PC.family(rng, int(rng.integers(20, 261)), n_rows) for _ in range(n_genes)], S3, SA)
cells = sum(int(w) * int(kw["res_off"][r + 1] - kw["res_off"][r]) for g, w in enumerate(kw["width"]) for r in range(int(kw["grp_off"][g]), int(kw["grp_off"][g + 1])))
print("speed: %d groups x %d rows, %.3g cells (input built in %.1f s)" % (n_genes, n_rows, cells, time.perf_counter() - t0), flush=True)
os.environ["UC_TIMING"] = "1"
for rep in range(3):
    dev, dt, err = timed_stderr(lambda: U.msa_profile_align(device=0, **kw))
    ms = float(re.search(r"DP kernel ([0-9.]+) ms", err).group(1))
    print("  device pass %d: call %.3f s (%.3g cells/s), DP kernel %.2f ms (%.3g cells/s)" % (rep, dt, cells / dt, ms, cells / (ms / 1e3)), flush=True)
os.environ.pop("UC_TIMING")
for threads in (1, 16):
    t = time.perf_counter(); host = U.msa_profile_align(threads=threads, **kw); dt = time.perf_counter() - t
    print("  host twin, %d thread(s): %.3f s (%.3g cells/s); same answers: %s" % (threads, dt, cells / dt, all(np.array_equal(dev[k], host[k]) for k in dev)), flush=True)


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
    for name, kwargs in (("star", {}), ("profile, 1 round", dict(aligner="profile", refine_iters=1)), ("profile, 2 rounds", dict(aligner="profile", refine_iters=2)),
                         ("profile, 3 rounds", dict(aligner="profile", refine_iters=3))):
        walls = []
        for rep in range(3):
            out = os.path.join(wd, "o")
            shutil.rmtree(out, ignore_errors=True)
            t = time.perf_counter(); st = U.tree(db, prof, out, 50, verbosity=0, device=0, **kwargs); walls.append(time.perf_counter() - t)
        msas = msa_of(out)
        sp = sum(P.sum_of_pairs(g, mats, p.gap_open, p.gap_ext) for g in msas.values())
        extra = ""
        if "refine" in st:
            extra = "; refinement %.3f s (DP + walk %.3f, layout %.3f), %d tasks, %.3g cells, rows aligned +%d -%d" % (
                st["refine"]["seconds"]["total"], st["refine"]["seconds"]["profile_dp_walk"], st["refine"]["seconds"]["layout_compaction"], st["refine"]["n_tasks"],
                st["refine"]["n_cells"], st["refine"]["n_rows_became_aligned"], st["refine"]["n_rows_became_unaligned"])
        print("  %s, %s: wall min %.3f s of 3; columns %d, kept %d, rows unaligned %d; sum of pairs %d%s" % (
            label, name, min(walls), st["n_columns"], st["n_columns_kept"], st["n_rows_unaligned"], sp, extra), flush=True)
    shutil.rmtree(wd, ignore_errors=True)


gold = os.path.join(ROOT, "tests", "golden")
wd = tempfile.mkdtemp()
prof = os.path.join(wd, "prof")
os.makedirs(prof)
for k, v in json.load(open(os.path.join(gold, "profile_default_t80.json"))).items():
    open(os.path.join(prof, k), "w").write(v)
print("cost and quality:", flush=True)
run("golden database, 11 genes", os.path.join(gold, "db"), prof)
# a family database with indels: 40 families of 12 members, every family a gene, every member a species
s3, sa = util.family_db(11, n_fam=40, members=12, indel=0.08, with_x=False)
names = util.write_db(os.path.join(wd, "fdb"), s3, sa)
prof2 = os.path.join(wd, "prof2")
os.makedirs(prof2)
for f in range(40):
    open(os.path.join(prof2, "fam%02d.txt" % f), "w").write("".join("%s\tsp%d\n" % (names[f * 12 + m], m) for m in range(12)))
run("family_db indel 0.08, 40 genes x 12 rows", os.path.join(wd, "fdb"), prof2)
shutil.rmtree(wd, ignore_errors=True)
