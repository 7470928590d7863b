#!/usr/bin/env python3
"""Rate of the exhaustive ungapped prefilter (rule UC-1/X, --prefilter-mode 1) on the bench's configs[1] database.

A query slice against the whole database under mode 1: cells/s of the all-diagonals kernel and its VALU fraction (2 lane-operations per cell - 4 VALU
instructions per 2 packed cells - against the 39.3 T lane-ops/s DESIGN.md section 5 uses), the wall of prefilter + gapped stage for the slice under both
modes, and the yardstick measured in the same process: the score-only packed gapped pass (table 1, MODE 0, Engine.sw_pass) on a pair list of the same
queries against a sample of the same targets.  Prints one JSON line; --out writes it to a file as well.

    python tools/ungapped_all_rate.py --queries 256 --sw-targets 4000 --out profiles/prefilter_mode1/rate.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")
import numpy as np  # noqa: E402

try:
    import torch  # noqa: F401,E402  (one HIP runtime per process: the bundled one first, as in bench.py)
except Exception:
    pass
import bench  # noqa: E402
import unicore_amd as U  # noqa: E402

VALU_LANE_OPS = 39.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--sw-targets", type=int, default=4000, help="targets per query of the gapped yardstick's pair list")
    ap.add_argument("--config", default="c2")
    ap.add_argument("--proteomes", type=int)
    ap.add_argument("--workdir", default=os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"))
    ap.add_argument("--out")
    ap.add_argument("--commit", help="recorded as is (default: git rev-parse --short HEAD; for a tree exported without its git metadata)")
    a = ap.parse_args()
    proteomes, families, scale, seed, options, label = bench.CONFIGS[a.config]
    proteomes = a.proteomes or proteomes
    prefix = bench.gen_db(os.path.join(a.workdir, "p%d_f%d_s%g_%x" % (proteomes, families, scale, seed)), proteomes, families, scale, seed)
    lens = bench.read_lens(prefix)
    n = len(lens)
    rng = np.random.default_rng(1)
    q0 = int(rng.integers(0, n - a.queries))
    q1 = q0 + a.queries
    res = {"database": "%s: %d proteomes, %d sequences, %d residues" % (label, proteomes, n, int(lens.sum())), "queries": [q0, q1],
           "commit": a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip(),
           "command": "python tools/ungapped_all_rate.py --queries %d --sw-targets %d --config %s" % (a.queries, a.sw_targets, a.config)}
    cells = int(lens[q0:q1].sum()) * int(lens.sum())
    walls = {}
    for mode in (1, 0):
        e = U.Engine("%s --single-step-clustering --prefilter-mode %d" % (options, mode), verbosity=1, device=0)
        e.load_db(prefix)
        for rep in range(2):                      # the first pass allocates the work buffers
            e.reset_stats()
            t0 = time.time()
            e.prefilter(0, n, q0, q1)
            t1 = time.time()
            e.align(q0, q1)
            t2 = time.time()
        st = e.stats()
        walls[mode] = {"prefilter_s": t1 - t0, "gapped_s": t2 - t1, "hits": e.hits_size(), "prefilter_kernel_ms": st["prefilter_kernel_ms"],
                       "stage_seconds": dict(zip(U.STAGES, st["stage_seconds"]))}
        if mode == 1:
            ung = walls[1]["stage_seconds"]["ungapped"]           # the tile kernels + the compaction of each tile, host-timed around a stream sync (warm call: the tile buffers are kept)
            res["mode1_cells"] = cells
            res["mode1_kernel_s"] = ung
            res["mode1_cells_per_s"] = cells / ung
            res["mode1_valu_fraction"] = 2.0 * cells / ung / VALU_LANE_OPS
            # the yardstick, same engine: score-only packed gapped pass over the same queries x a sample of the targets
            tg = np.sort(rng.choice(n, min(a.sw_targets, n), replace=False)).astype(np.uint32)
            q = np.repeat(np.arange(q0, q1, dtype=np.uint32), len(tg))
            t = np.tile(tg, q1 - q0)
            sw_cells = int(lens[q0:q1].sum()) * int(lens[tg].sum())
            for rep in range(2):
                e.reset_stats()
                t0 = time.time()
                e.sw_pass(1, 0, q, t, raw=True)
                w = time.time() - t0
            k = e.stats()["sw_kernel_ms"] / 1e3
            res["sw_mode0_pairs"] = len(q)
            res["sw_mode0_cells"] = sw_cells
            res["sw_mode0_wall_s"] = w
            res["sw_mode0_kernel_s"] = k
            res["sw_mode0_cells_per_s"] = sw_cells / k           # kernel against kernel: the event time of the raw pass's class kernels (uc_align.hip, sw_pass)
            res["ratio_mode1_over_sw_mode0"] = res["mode1_cells_per_s"] / res["sw_mode0_cells_per_s"]
        e.close()
    res["slice_wall"] = {"mode%d" % m: v for m, v in walls.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
