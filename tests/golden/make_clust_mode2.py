#!/usr/bin/env python3
"""Regenerate tests/golden/clust_mode2.tsv: rule UC-1/G (--cluster-mode 2, greedy incremental) on the small golden database.
The accepted pairs are the CPU oracle's ("-c 0.8", plain step), the clustering is the test-side Python reference
(tests/greedy_incremental_ref.py), the file is written by the oracle's write_tsv.  No product code is involved.
Run from the repo root:  python tests/golden/make_clust_mode2.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import util  # noqa: E402
from greedy_incremental_ref import greedy_incremental  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

OPTS = "-c 0.8"


def oracle_accepted_pairs(odb, opts=OPTS):
    """(edges [k, 2] as (query, target), lengths [n]) of the oracle's plain step"""
    r = O.cluster(odb, util.oracle_params(O, opts), threads=4)
    cnt = r["hit_cnt"]
    q = np.repeat(np.arange(odb.n, dtype=np.uint32), cnt)
    t = np.concatenate([r["hits"][i, : cnt[i]]["t"] for i in range(odb.n)]).astype(np.uint32)
    acc = np.concatenate([r["aln"][i, : cnt[i]]["accepted"] for i in range(odb.n)]) == 1
    return np.stack([q[acc], t[acc]], 1), np.diff(odb.offsets().astype(np.int64)).astype(np.uint32)


def main():
    odb = O.OracleDb(os.path.join(HERE, "db"))
    edges, lens = oracle_accepted_pairs(odb)
    assign = greedy_incremental(odb.n, edges, lens)
    O.write_tsv(os.path.join(HERE, "clust_mode2.tsv"), odb, assign)
    print("clust_mode2:", odb.n, "seqs,", len(edges), "accepted pairs,", int((assign == np.arange(odb.n)).sum()), "clusters")


if __name__ == "__main__":
    main()
