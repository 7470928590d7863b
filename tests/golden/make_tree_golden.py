#!/usr/bin/env python3
"""Regenerate tests/golden/tree_default_d50.json: the output of `unicore tree --no-inference -d 50` (rule UC-T) on tests/golden/db for the 11 core
genes that `unicore profile -t 80` finds in tests/golden/clust_default.tsv (the gene files of tests/golden/profile_default_t80.json).  It keeps
combined.fasta and combined.fasta.partitions in full and a sha256 per gene file.  The rule is the test-side Python reference (tests/msa_ref.py)
over the CPU oracle; no product code is involved.
Run from the repo root:  python tests/golden/make_tree_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msa_ref  # noqa: E402
import util  # noqa: E402
from oracle import oracle_py as O  # noqa: E402


def gene_files():
    prof = json.load(open(os.path.join(HERE, "profile_default_t80.json")))
    return {k: v.encode("ascii") for k, v in prof.items() if k.endswith(".txt")}


def main():
    files, info = msa_ref.tree_files(O, util.oracle_params(O, msa_ref.FIXED_OPTS), os.path.join(HERE, "db"), gene_files(), 50)
    with open(os.path.join(HERE, "tree_default_d50.json"), "w") as f:
        json.dump(msa_ref.digest(files), f, indent=1, sort_keys=True)
        f.write("\n")
    print("tree_default_d50:", len(info), "genes,", sum(v["unaligned"] for v in info.values()), "unaligned rows,", len(files["combined.fasta"]), "bytes of combined.fasta")
    print(files["combined.fasta.partitions"].decode())


if __name__ == "__main__":
    main()
