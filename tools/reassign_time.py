"""The default workflow with and without --cluster-reassign through uc_cluster: python tools/reassign_time.py [c2|c3|c4-lite|c4] [repeats] [proteomes]
Every pass is one uc_cluster call at -v 3 with UC_TIMING on: the stage's own line (members verified, rejected, re-search pairs, clusters before ->
after) and its timing line (lists, verify, verdict, re-search, re-cluster) land on stderr beside the wall times printed here.  The first pass of
each variant allocates the work buffers: reported, not counted."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, unicore_amd as U
cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
proteomes, families, scale, seed, options, label = bench.CONFIGS[cfg]
if len(sys.argv) > 3:
    proteomes = int(sys.argv[3])
wd = os.path.join(os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"), "p%d_f%d_s%g_%x" % (proteomes, families, scale, seed))
prefix = bench.gen_db(wd, proteomes, families, scale, seed)
os.environ["UC_TIMING"] = "1"
res = {}
for rep in range(reps + 1):
    for flag in ("", " --cluster-reassign"):
        t = time.perf_counter()
        st = U.cluster(prefix, os.path.join(wd, "rt_cluster"), os.path.join(wd, "tmp"), options + flag, threads=16, verbosity=3)
        s = time.perf_counter() - t
        res.setdefault(flag, []).append(s)
        print("%s pass %d '%s': %.3f s wall, %d sequences, %d gapped alignments, %d clusters%s" % (cfg, rep, options + flag, s, st["n_seqs"], st["n_gapped_alignments"],
                                                                                                    st["n_clusters"], " (cold)" if rep == 0 else ""), flush=True)
for flag, v in res.items():
    w = sorted(v[1:]) or v          # repeats = 0: the cold pass is all there is
    print("'%s' warm: min %.3f median %.3f max %.3f s" % (options + flag, w[0], w[len(w) // 2], w[-1]))
