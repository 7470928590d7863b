#!/usr/bin/env python3
"""Regenerate tests/golden/nj_default.json: the trees `unicore tree -t nj` and `unicore gene-tree -t nj` (rule UC-N, model kimura) give on
tests/golden/db for the 11 core genes of tests/golden/profile_default_t80.json.  "nj.nwk" is the tree of combined.fasta (the alignment that
tree_default_d50.json pins), "genes" holds the tree of every <gene>.fa.filtered (null for a gene with fewer than 2 rows).  The alignments are the
test-side reference of rule UC-T (tests/msa_ref.py over the CPU oracle) and the trees the plain-Python reference tests/nj_ref.py; no product
code is involved.  Lengths are printed with %.6f, so a last-bit difference of log between C libraries does not reach this file.
Run from the repo root:  python tests/golden/make_nj_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msa_ref  # noqa: E402
import nj_ref  # noqa: E402
import util  # noqa: E402
from oracle import oracle_py as O  # noqa: E402


def trees_of(files):
    """files: what msa_ref.tree_files / msa_ref.read_tree give.  Returns the fixture's dict."""
    out = {"nj.nwk": nj_ref.tree_of_fasta(files["combined.fasta"].decode("latin-1")), "genes": {}}
    for k in sorted(files):
        if k.endswith(".fa.filtered"):
            gene = k.split("/")[1]
            text = files[k].decode("latin-1")
            out["genes"][gene] = nj_ref.tree_of_fasta(text) if text.count(">") >= 2 else None
    return out


def main():
    prof = json.load(open(os.path.join(HERE, "profile_default_t80.json")))
    genes = {k: v.encode("ascii") for k, v in prof.items() if k.endswith(".txt")}
    files, _ = msa_ref.tree_files(O, util.oracle_params(O, msa_ref.FIXED_OPTS), os.path.join(HERE, "db"), genes, 50)
    assert msa_ref.digest(files) == json.load(open(os.path.join(HERE, "tree_default_d50.json")))
    fx = trees_of(files)
    with open(os.path.join(HERE, "nj_default.json"), "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    print("nj_default:", len(fx["genes"]), "genes;", fx["nj.nwk"].strip())


if __name__ == "__main__":
    main()
