"""Bootstrap support of the tree builder `nj` at size: python tools/nj_boot_time.py [threads] [NxWxB ...]
(default: 16 threads; 50x200000x100 50x200000x1000 128x200000x100 128x200000x1000 129x200000x100 129x200000x1000 2000x200000x100)
Per case it writes one generated alignment (tools/nj_time.py's: a random root sequence, every row a copy with a fifth of its columns redrawn, gaps
and X sprinkled in) and times
  * uc_tree_infer_boot on it (device kernels), with uc_nj_boot_stats' seconds per phase; UC_TIMING is set, so the library adds the gathering count
    kernel's own time between two events on stderr;
  * the baseline a user of the entry points without a replicate dimension has: per replicate the alignment gathered explicitly on the host (numpy,
    with uc_nj_boot_columns' draws), uc_nj_counts_dev + uc_nj_distances + uc_nj_join_dev.  It runs min(B, BASE) replicates (BASE = 100 up to 200 rows,
    5 above) and is scaled to B; the gather's own seconds are printed apart, the ratio is given with and without them.
The first replicate's join records of both ways are compared."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unicore_amd as U
os.environ.setdefault("UC_TIMING", "1")
args = sys.argv[1:]
threads = int(args[0]) if args and "x" not in args[0] else 16
cases = [tuple(int(v) for v in a.split("x")) for a in args if "x" in a] or [(50, 200000, 100), (50, 200000, 1000), (128, 200000, 100), (128, 200000, 1000), (129, 200000, 100),
                                                                         (129, 200000, 1000), (2000, 200000, 100)]
wd = os.path.join(os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"), "nj_boot_time")
os.makedirs(wd, exist_ok=True)
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
SEED = 1
print("geometry: %s %s; %d host threads" % (U.nj_geometry(), U.nj_boot_geometry(), threads), flush=True)
U.nj_counts(np.full((2, 4), 65, np.uint8), device=0)      # the code object is loaded outside the timed calls
made = {}
for n, w, B in cases:
    if (n, w) not in made:
        rng = np.random.default_rng(n * 1000003 + w)
        root = AA[rng.integers(0, 20, w)]
        rows = np.empty((n, w), np.uint8)
        for i in range(n):
            row = root.copy()
            m = rng.random(w)
            redraw = m < 0.2
            row[redraw] = AA[rng.integers(0, 20, int(redraw.sum()))]
            row[m > 0.95] = ord("-")
            row[(m > 0.94) & (m <= 0.95)] = ord("X")
            rows[i] = row
        fasta = os.path.join(wd, "msa_%dx%d.fasta" % (n, w))
        with open(fasta, "wb") as f:
            for i in range(n):
                f.write(b">sp%05d\n" % i + rows[i].tobytes() + b"\n")
        made = {(n, w): (rows, fasta)}      # one alignment in memory at a time
    rows, fasta = made[(n, w)]
    out = os.path.join(wd, "boot_%dx%dx%d.nwk" % (n, w, B))
    t = time.perf_counter(); s = U.tree_infer(fasta, out, "kimura", verbosity=0, device=0, threads=threads, bootstrap=B, seed=SEED); wall = time.perf_counter() - t
    sec = s["seconds"]
    tri = n * (n - 1) // 2
    print("%d x %d, B = %d: uc_tree_infer_boot %.3f s wall; %s; replicates alone %.3f s = %.3f ms per replicate; count phase %.3g pair-columns/s; joins %.1f us per replicate; %s" % (
        n, w, B, wall, ", ".join("%s %.3f" % kv for kv in sec.items()), sum(sec[k] for k in ("counts", "transform", "join", "support")),
        1e3 * sum(sec[k] for k in ("counts", "transform", "join", "support")) / B, tri * w * B / max(sec["counts"], 1e-9), 1e6 * sec["join"] / B,
        ", ".join("%s %d" % kv for kv in s.items() if kv[0] != "seconds")), flush=True)
    base = min(B, 100 if n <= 200 else 5)
    t_gather = t_counts = t_dist = t_join = 0.0
    first = None
    saved = os.environ.pop("UC_TIMING", None)      # one stderr line per call would drown the output
    for b in range(base):
        t0 = time.perf_counter(); g = np.ascontiguousarray(rows[:, U.nj_boot_columns(w, SEED, b).astype(np.int64)]); t1 = time.perf_counter()
        comp, diff = U.nj_counts(g, device=0); t2 = time.perf_counter()
        D = U.nj_distances(comp, diff, n); t3 = time.perf_counter()
        j = U.nj_join(D, device=0); t4 = time.perf_counter()
        t_gather += t1 - t0; t_counts += t2 - t1; t_dist += t3 - t2; t_join += t4 - t3
        if b == 0:
            first = j
    if saved is not None:
        os.environ["UC_TIMING"] = saved
    scale = B / base
    calls = (t_counts + t_dist + t_join) * scale
    reps = sum(sec[k] for k in ("counts", "transform", "join", "support"))
    print("  baseline, %d replicate(s) scaled to %d: gather on the host %.3f s, uc_nj_counts_dev %.3f s, uc_nj_distances %.3f s, uc_nj_join_dev %.3f s (%.1f us per step); "
          "calls alone %.3f s, with the gather %.3f s; ratio to the batched replicates: %.1fx (calls alone), %.1fx (with the gather)" % (
              base, B, t_gather * scale, t_counts * scale, t_dist * scale, t_join * scale, 1e6 * t_join / base / max(n - 3, 1), calls, calls + t_gather * scale,
              calls / reps, (calls + t_gather * scale) / reps), flush=True)
    # the same replicate both ways: replicate 0's tree is the first line of the dump of a one-replicate run
    os.environ["UC_TREE_DUMP"] = "1"
    U.tree_infer(fasta, out + ".one", "kimura", verbosity=0, device=0, threads=threads, bootstrap=1, seed=SEED)
    os.environ.pop("UC_TREE_DUMP")
    names = ["sp%05d" % i for i in range(n)]
    assert open(out + ".one.boottrees").read() == U.nj_newick(names, first), "the batched replicate 0 and the baseline's differ"
    print("  replicate 0: the batched path and the baseline wrote the same tree", flush=True)
    for ext in ("", ".one", ".one.boottrees", ".one.boot.tsv", ".one.dist.tsv"):
        if os.path.exists(out + ext):
            os.remove(out + ext)
os.remove(fasta)
