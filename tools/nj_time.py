"""The tree builder `nj` at size: python tools/nj_time.py [threads] [NxW ...]      (default: 16 threads, 200x50000 2000x200000 2000x1000000)
Per shape it writes one generated alignment (a random root sequence, every row a copy with a fifth of its columns redrawn, gaps and X sprinkled
in) and runs uc_tree_infer on it with the device kernels and with the host twins (UC_TREE_HOST=1) on `threads` host threads, in this process.
Prints per run the wall time and uc_nj_stats (counts and seconds per phase), the pair-columns per second of the count phase (n (n - 1) / 2 x w
over its seconds: upload, encode pass and download included on the device side) and the join loop's time per step; with UC_TIMING set (it is, below)
the library adds the count kernel's own time between two events on stderr.  The two trees are compared byte for byte."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unicore_amd as U
os.environ.setdefault("UC_TIMING", "1")
args = sys.argv[1:]
threads = int(args[0]) if args and "x" not in args[0] else 16
shapes = [tuple(int(v) for v in a.split("x")) for a in args if "x" in a] or [(200, 50000), (2000, 200000), (2000, 1000000)]
wd = os.path.join(os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"), "nj_time")
os.makedirs(wd, exist_ok=True)
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
print("geometry: %s; %d host threads for the twins" % (U.nj_geometry(), threads), flush=True)
for n, w in shapes:
    rng = np.random.default_rng(n * 1000003 + w)
    fasta = os.path.join(wd, "msa_%dx%d.fasta" % (n, w))
    t = time.perf_counter()
    root = AA[rng.integers(0, 20, w)]
    with open(fasta, "wb") as f:
        for i in range(n):
            row = root.copy()
            m = rng.random(w)
            redraw = m < 0.2
            row[redraw] = AA[rng.integers(0, 20, int(redraw.sum()))]
            row[m > 0.95] = ord("-")
            row[(m > 0.94) & (m <= 0.95)] = ord("X")
            f.write(b">sp%05d\n" % i + row.tobytes() + b"\n")
    print("%d x %d: alignment written in %.1f s (%.0f MB)" % (n, w, time.perf_counter() - t, os.path.getsize(fasta) / 1e6), flush=True)
    trees = {}
    for host in (False, True, False):
        out = os.path.join(wd, "nj_%dx%d_%s.nwk" % (n, w, "host" if host else "dev"))
        if host:
            os.environ["UC_TREE_HOST"] = "1"
        else:
            os.environ.pop("UC_TREE_HOST", None)
        t = time.perf_counter(); s = U.tree_infer(fasta, out, "kimura", verbosity=0, device=0, threads=threads); wall = time.perf_counter() - t
        trees[host] = open(out, "rb").read()
        sec = s["seconds"]
        print("  %-6s %.3f s wall; %s; count phase %.3g pair-columns/s; join %.1f us per step (%d steps); %s" % (
            "host" if host else "device", wall, ", ".join("%s %.3f" % (k, v) for k, v in sec.items()), n * (n - 1) / 2 * w / max(sec["counts"], 1e-9),
            1e6 * sec["join"] / max(n - 3, 1), max(n - 3, 0), ", ".join("%s %d" % (k, v) for k, v in s.items() if k != "seconds")), flush=True)
    os.environ.pop("UC_TREE_HOST", None)
    assert trees[False] == trees[True], "device kernels and host twins wrote different trees"
    print("  device and host wrote the same %d bytes" % len(trees[False]), flush=True)
    os.remove(fasta)
