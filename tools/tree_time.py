"""`unicore tree --no-inference` at size: python tools/tree_time.py [c2|c3] [repeats] [proteomes]
Runs the chain of the reference's easy-core on one synthetic input: the default workflow of the configuration (uc_cluster + uc_createtsv),
uc_profile at threshold 80, then uc_tree at threshold 50 with the device kernels and with the host twins (UC_TREE_HOST=1), alternating, in
this process.  Prints per pass the wall time, uc_tree_stats (counts and seconds per phase) and the alignments per second of the all-pairs
score pass; the first pass of each variant is reported, not counted.  The two output directories are compared byte for byte."""
import hashlib, os, shutil, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, unicore_amd as U
cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
proteomes, families, scale, seed, options, label = bench.CONFIGS[cfg]
if len(sys.argv) > 3:
    proteomes = int(sys.argv[3])
wd = os.path.join(os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"), "p%d_f%d_s%g_%x" % (proteomes, families, scale, seed))
prefix = bench.gen_db(wd, proteomes, families, scale, seed)
tsv, prof = os.path.join(wd, "tt_clust.tsv"), os.path.join(wd, "tt_profile")
t = time.perf_counter()
st = U.cluster(prefix, os.path.join(wd, "tt_cluster"), os.path.join(wd, "tmp"), options, threads=16, verbosity=1)
U.createtsv(prefix, os.path.join(wd, "tt_cluster"), tsv)
t_cluster = time.perf_counter() - t
shutil.rmtree(prof, ignore_errors=True)
t = time.perf_counter()
U.profile(prefix, tsv, prof, 80, verbosity=0, device=0)
t_profile = time.perf_counter() - t
genes = [f for f in os.listdir(prof) if f.endswith(".txt")]
print("%s: %d proteomes, %d sequences, %d clusters; cluster + createtsv %.2f s; profile -t 80 %.2f s, %d core genes" % (
    cfg, proteomes, st["n_seqs"], st["n_clusters"], t_cluster, t_profile, len(genes)), flush=True)


def digest(d):
    h = hashlib.sha256()
    for root, _, files in sorted(os.walk(d)):
        for n in sorted(files):
            h.update(os.path.relpath(os.path.join(root, n), d).encode() + b"\0" + open(os.path.join(root, n), "rb").read() + b"\0")
    return h.hexdigest()[:16]


res, sums = {}, {}
for rep in range(reps + 1):
    for host in (False, True):
        out = os.path.join(wd, "tt_tree_host" if host else "tt_tree_dev")
        shutil.rmtree(out, ignore_errors=True)
        if host:
            os.environ["UC_TREE_HOST"] = "1"
        else:
            os.environ.pop("UC_TREE_HOST", None)
        t = time.perf_counter(); s = U.tree(prefix, prof, out, 50, verbosity=0, device=0); wall = time.perf_counter() - t
        res.setdefault(host, []).append((wall, s))
        sums[host] = digest(out)
        sec = s["seconds"]
        print("uc_tree pass %d, %s layout: %.3f s wall; %s; all-pairs pass %.0f alignments/s; sha %s%s" % (
            rep, "host" if host else "device", wall, ", ".join("%s %.3f" % (k, v) for k, v in sec.items()),
            s["n_pairs_scored"] / sec["pair_scores"] if sec["pair_scores"] > 0 else 0.0, sums[host], " (first)" if rep == 0 else ""), flush=True)
os.environ.pop("UC_TREE_HOST", None)
assert sums[False] == sums[True], "device kernels and host twins wrote different directories"
s = res[False][-1][1]
print("counts: " + ", ".join("%s %d" % (k, v) for k, v in s.items() if k != "seconds"))
for host, v in res.items():
    w = sorted(x[0] for x in v[1:]) or [v[0][0]]
    print("uc_tree, %s layout, after the first pass: min %.3f median %.3f max %.3f s" % ("host" if host else "device", w[0], w[len(w) // 2], w[-1]))
