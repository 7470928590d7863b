"""Clustering stage (E7) under --cluster-mode 0 and 2 on ONE engine and ONE edge list: python tools/cluster_mode_time.py [c2|c3] [repeats]
Runs the plain step of the configuration up to the accepted pairs, then times Engine.cluster_graph(edges, mode) for both rules with
UC_TIMING on, so that the library's own lines (graph build, rounds, round count, host tail) land on stderr beside the wall times."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, unicore_amd as U
cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
proteomes, families, scale, seed, options, label = bench.CONFIGS[cfg]
wd = os.path.join(os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"), "p%d_f%d_s%g_%x" % (proteomes, families, scale, seed))
prefix = bench.gen_db(wd, proteomes, families, scale, seed)
e = U.Engine(options, verbosity=1); e.load_db(prefix)
e.prefilter(); e.align(); ed = e.edges(); n = e.n
print("%s: %d sequences, %d accepted pairs" % (cfg, n, len(ed)), flush=True)
os.environ["UC_TIMING"] = "1"
res = {}
modes = (0, 2) if hasattr(e, "cluster_graph") else (0,)      # a tree from before the rule existed: the set cover alone, as the yardstick
for rep in range(reps + 1):          # the first pass of each rule sizes its buffers: reported, not counted
    for mode in modes:
        t = time.perf_counter(); a = e.setcover(ed) if mode == 0 else e.cluster_graph(ed, mode); ms = (time.perf_counter() - t) * 1e3
        res.setdefault(mode, []).append(ms)
        print("mode %d pass %d: %.2f ms wall, %d clusters%s" % (mode, rep, ms, int((a == np.arange(n)).sum()), " (cold)" if rep == 0 else ""), flush=True)
for mode in modes:
    w = sorted(res[mode][1:])
    print("mode %d warm: min %.2f median %.2f max %.2f ms" % (mode, w[0], w[len(w) // 2], w[-1]))
