"""Transfer bootstrap support of the tree builder `nj` (rule UC-N/T) at size: python tools/nj_transfer_time.py [threads] [NxB ...]
(default: 16 threads; 128x1000 2000x100 8000x100)
The transfer phase reads join records alone and no kernel of it branches on what they hold, so the tool makes them itself instead of running
N = 8000 bootstraps: the main tree is a random join order, a replicate is the same tree with children traded between neighbouring joins N / 10
times (most splits stay, some move by a few leaves).  Per case it times
  * uc_nj_transfer_dev (bit sets, comparison, transfers; the second of two calls), and with UC_TIMING set the library adds the comparison kernel's
    own time between two events on stderr; the rate is given against the floor of 2 integer VALU operations per pair and 32-bit word at the
    39.3 T lane-ops/s of DESIGN.md 5;
  * the host twin uc_nj_transfer on `threads` threads, on min(B, HOST) replicates (HOST = 1000 up to 200 leaves, `threads` above) scaled to B.
phi and light of both are compared on the replicates both ran.
An argument `infer=NxWxB` then runs uc_tree_infer_support in mode tbe on a generated alignment (tools/nj_time.py's) and prints the seconds per phase:
the transfer phase ([5], support) next to the joins."""
import os, random, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unicore_amd as U
os.environ.setdefault("UC_TIMING", "1")
args = sys.argv[1:]
threads = int(args[0]) if args and "x" not in args[0] else 16
infer = [tuple(int(v) for v in a[6:].split("x")) for a in args if a.startswith("infer=")]
cases = [tuple(int(v) for v in a.split("x")) for a in args if "x" in a and "=" not in a] or [(128, 1000), (2000, 100), (8000, 100)]
VALU = 39.3e12


def random_parents(n, rng):
    """a random join order as join records: (join_a, join_b)"""
    nodes, ja, jb = list(range(n)), [], []
    for s in range(n - 3):
        a = nodes.pop(rng.randrange(len(nodes))); b = nodes.pop(rng.randrange(len(nodes)))
        ja.append(a); jb.append(b); nodes.append(n + s)
    return ja, jb


def replicate(n, ja, jb, rng, moves):
    """the main tree's records with one child traded between joins s and s + 1, `moves` times, wherever join s + 1 does not hang on join s: every
    record still joins two nodes that exist before it, and no node is joined twice"""
    a, b = list(ja), list(jb)
    for _ in range(moves):
        s = rng.randrange(n - 4)
        if b[s + 1] != n + s and a[s + 1] != n + s:
            b[s], b[s + 1] = b[s + 1], b[s]
    return a, b


print("geometry: %s; %d host threads" % (U.nj_transfer_geometry(), threads), flush=True)
U.nj_transfer(4, {"join_a": [0], "join_b": [1]}, [[0]], [[1]], device=0)      # the code object is loaded outside the timed calls
for n, B in cases:
    rng = random.Random(n * 1000003 + B)
    ja, jb = random_parents(n, rng)
    main = {"join_a": ja, "join_b": jb}
    reps = [replicate(n, ja, jb, rng, max(n // 10, 1)) for _ in range(B)]
    ra, rb = np.array([r[0] for r in reps], np.uint32), np.array([r[1] for r in reps], np.uint32)
    steps, words = n - 3, (n + 31) // 32
    saved = os.environ.pop("UC_TIMING", None)
    U.nj_transfer(n, main, ra[:1], rb[:1], device=0)
    if saved is not None:
        os.environ["UC_TIMING"] = saved
    t = time.perf_counter(); phi, light = U.nj_transfer(n, main, ra, rb, device=0); dev = time.perf_counter() - t
    pw = steps * steps * words * B
    print("%d leaves, B = %d: uc_nj_transfer_dev %.4f s = %.3f ms per replicate, %.3g pair-words/s over the whole call (the floor of 2 VALU per pair-word is %.3g/s); "
          "phi == 0 in %.1f %% of (replicate, join), mean phi / (light - 1) = %.3f" % (n, B, dev, 1e3 * dev / B, pw / dev, VALU / 2, 100.0 * (phi == 0).mean(),
                                                                                      (phi / np.maximum(light - 1, 1)).mean()), flush=True)
    hb = min(B, 1000 if n <= 200 else threads)
    t = time.perf_counter(); hphi, hlight = U.nj_transfer(n, main, ra[:hb], rb[:hb], threads=threads); host = time.perf_counter() - t
    assert np.array_equal(hphi, phi[:hb]) and np.array_equal(hlight, light), "device and host twin differ"
    print("  host twin, %d replicate(s) on %d threads: %.4f s, scaled to %d: %.3f s = %.3f ms per replicate; twin / device = %.1fx; phi and light agree" % (
        hb, threads, host, B, host * B / hb, 1e3 * host / hb, host * B / hb / dev), flush=True)

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
wd = os.path.join(os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"), "nj_transfer_time")
for n, w, B in infer:
    os.makedirs(wd, exist_ok=True)
    rng = np.random.default_rng(n * 1000003 + w)
    root = AA[rng.integers(0, 20, w)]
    fasta, out = os.path.join(wd, "msa_%dx%d.fasta" % (n, w)), os.path.join(wd, "tbe_%dx%dx%d.nwk" % (n, w, B))
    with open(fasta, "wb") as f:
        for i in range(n):
            row, m = root.copy(), rng.random(w)
            row[m < 0.2] = AA[rng.integers(0, 20, int((m < 0.2).sum()))]
            row[m > 0.95] = ord("-")
            f.write(b">sp%05d\n" % i + row.tobytes() + b"\n")
    for mode in ("fbp", "tbe"):
        t = time.perf_counter(); st = U.tree_infer(fasta, out, "kimura", verbosity=0, device=0, threads=threads, bootstrap=B, seed=1, support=mode); wall = time.perf_counter() - t
        print("%d x %d, B = %d, support %s: %.3f s wall; %s; support phase %.3f ms per replicate, joins %.3f ms per replicate; %s" % (
            n, w, B, mode, wall, ", ".join("%s %.3f" % kv for kv in st["seconds"].items()), 1e3 * st["seconds"]["support"] / B, 1e3 * st["seconds"]["join"] / B,
            ", ".join("%s %d" % kv for kv in st.items() if kv[0] != "seconds")), flush=True)
    os.remove(fasta); os.remove(out)
