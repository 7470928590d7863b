"""`unicore profile` at size: python tools/profile_time.py [c2|c3] [repeats] [proteomes]
Runs the default workflow of the configuration through uc_cluster + uc_createtsv once, then times uc_profile on that clust.tsv with the device
counter and with the host counter (UC_PROFILE_HOST=1), alternating, each pass in this process with UC_TIMING on: the library's own line (map
parse, TSV parse, counting with the device stages by HIP events, file writing) lands on stderr beside the wall times printed here.  Then the
two counters alone on the same arrays (uc_profile_count_dev / uc_profile_count).  The first pass of each variant is reported, not counted.
The output directories of the two counters are compared byte for byte."""
import hashlib, os, shutil, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import bench, unicore_amd as U
cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
proteomes, families, scale, seed, options, label = bench.CONFIGS[cfg]
if len(sys.argv) > 3:
    proteomes = int(sys.argv[3])
wd = os.path.join(os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"), "p%d_f%d_s%g_%x" % (proteomes, families, scale, seed))
prefix = bench.gen_db(wd, proteomes, families, scale, seed)
tsv = os.path.join(wd, "pt_clust.tsv")
t = time.perf_counter()
st = U.cluster(prefix, os.path.join(wd, "pt_cluster"), os.path.join(wd, "tmp"), options, threads=16, verbosity=1)
U.createtsv(prefix, os.path.join(wd, "pt_cluster"), tsv)
print("%s: %d proteomes, %d sequences, %d clusters, default workflow + createtsv %.1f s; clust.tsv %d rows, %.1f MB; db.map %.1f MB" % (
    cfg, proteomes, st["n_seqs"], st["n_clusters"], time.perf_counter() - t, sum(1 for _ in open(tsv, "rb")), os.path.getsize(tsv) / 1e6,
    os.path.getsize(prefix + ".map") / 1e6), flush=True)


def digest(d):
    h = hashlib.sha256()
    for n in sorted(os.listdir(d)):
        h.update(n.encode() + b"\0" + open(os.path.join(d, n), "rb").read() + b"\0")
    return h.hexdigest()[:16], len(os.listdir(d))


os.environ["UC_TIMING"] = "1"
res, sums = {}, {}
for rep in range(reps + 1):
    for host in (False, True):
        out = os.path.join(wd, "pt_prof_host" if host else "pt_prof_dev")
        shutil.rmtree(out, ignore_errors=True)
        if host:
            os.environ["UC_PROFILE_HOST"] = "1"
        else:
            os.environ.pop("UC_PROFILE_HOST", None)
        t = time.perf_counter(); U.profile(prefix, tsv, out, 80, verbosity=0, device=0); s = time.perf_counter() - t
        res.setdefault(host, []).append(s)
        sums[host] = digest(out)
        print("uc_profile pass %d, %s counter: %.3f s wall, %d files, sha %s%s" % (rep, "host" if host else "device", s, sums[host][1], sums[host][0], " (first)" if rep == 0 else ""), flush=True)
os.environ.pop("UC_PROFILE_HOST", None)
assert sums[False] == sums[True], "the two counters wrote different directories"
for host, v in res.items():
    w = sorted(v[1:]) or v
    print("uc_profile, %s counter, after the first pass: min %.3f median %.3f max %.3f s" % ("host" if host else "device", w[0], w[len(w) // 2], w[-1]))

# the counters alone, on the arrays the file level builds (here by the test-side reader: not timed)
import profile_ref as R
A = R.arrays(open(prefix + ".map", "rb").read(), open(tsv, "rb").read())
args = (A["group"], A["gene"], A["n_groups"], A["sp_off"], A["sp"], A["n_species"], 80)
print("arrays: %d rows, %d groups, %d genes, %d species" % (len(A["group"]), A["n_groups"], len(A["gene_names"]), A["n_species"]), flush=True)
alone = {}
for rep in range(reps + 1):
    for dev in (0, None):
        t = time.perf_counter(); r = U.profile_count(*args, device=dev); ms = (time.perf_counter() - t) * 1e3
        alone.setdefault(dev, []).append(ms)
        last = alone.setdefault(("r", dev), r)
        assert all(np.array_equal(r[k], last[k]) for k in r)
for dev in (0, None):
    w = sorted(alone[dev][1:]) or alone[dev]
    print("profile_count (Python wrapper included), %s: first %.2f ms; then min %.2f median %.2f max %.2f ms" % ("device" if dev == 0 else "host", alone[dev][0], w[0], w[len(w) // 2], w[-1]))
assert all(np.array_equal(alone[("r", 0)][k], alone[("r", None)][k]) for k in alone[("r", 0)]), "device and host counters differ"
print("core groups: %d of %d" % (int(alone[("r", 0)]["core"].sum()), A["n_groups"]))
