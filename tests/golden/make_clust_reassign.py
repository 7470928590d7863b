#!/usr/bin/env python3
"""Regenerate tests/golden/clust_reassign.tsv: rule UC-1/R (--cluster-reassign) behind the default workflow on the small golden database.
The workflow's assignment, every alignment verdict and the re-search lists are the CPU oracle's; the rule is the test-side Python restatement
(tests/cluster_reassign_ref.py); the final graph is clustered by the host uc_cluster_graph; the file is written by the oracle's write_tsv.
No device is involved.  Run from the repo root:  python tests/golden/make_clust_reassign.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")
import util  # noqa: E402
import cluster_reassign_ref as R  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

OPTS = "-c 0.8 --min-seq-id 0.3 -s 7.5 --cluster-reassign"


def reference(odb, opts=OPTS):
    """(assignment of the workflow without the flag, result dict of the rule) for an option string of uc_cluster"""
    import unicore_amd as U
    base, sw = R.split_options(opts)
    p = util.oracle_params(O, base)
    A = R.workflow_assign(O, odb, p, sw)
    return A, R.reassign(O, U, odb, p, A, sw["cluster_mode"], sw["prefilter_mode"])


def main():
    odb = O.OracleDb(os.path.join(HERE, "db"))
    A, res = reference(odb)
    O.write_tsv(os.path.join(HERE, "clust_reassign.tsv"), odb, res["assign"])
    print("clust_reassign:", odb.n, "seqs; verified, rejected, re-search pairs, clusters =", res["counts"], "; clusters before:", int((A == np.arange(odb.n)).sum()))


if __name__ == "__main__":
    main()
