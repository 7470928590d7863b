#!/usr/bin/env python3
"""Regenerate tests/golden/nj_transfer.json: what `unicore tree -t nj -p "--bootstrap 12 --seed 7 --support tbe"` and `unicore gene-tree -t nj` with
the same options (rule UC-N/T, model kimura) give on tests/golden/db for the 11 core genes of tests/golden/profile_default_t80.json.  "nj.nwk" is the
tree of combined.fasta (the alignment that tree_default_d50.json pins) with the transfer labels, "support" the replicates that hold every join's
split, "light" and "phi_sum" the rule's terms, "boot.tsv" the dump's table, "boottrees" the 12 replicate trees; "genes" holds the labelled tree of
every <gene>.fa.filtered (null for a gene with fewer than 2 rows).  The alignments are the test-side reference of rule UC-T (tests/msa_ref.py over
the CPU oracle), everything else the plain-Python reference tests/nj_transfer_ref.py over tests/nj_boot_ref.py and tests/nj_ref.py; no product code
is involved.
Run from the repo root:  python tests/golden/make_nj_transfer_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msa_ref  # noqa: E402
import nj_transfer_ref  # noqa: E402
import util  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

BOOTSTRAP, SEED = 12, 7


def main():
    prof = json.load(open(os.path.join(HERE, "profile_default_t80.json")))
    genes = {k: v.encode("ascii") for k, v in prof.items() if k.endswith(".txt")}
    files, _ = msa_ref.tree_files(O, util.oracle_params(O, msa_ref.FIXED_OPTS), os.path.join(HERE, "db"), genes, 50)
    assert msa_ref.digest(files) == json.load(open(os.path.join(HERE, "tree_default_d50.json")))
    top = nj_transfer_ref.transfer_of_fasta(files["combined.fasta"].decode("latin-1"), BOOTSTRAP, SEED)
    fx = {"bootstrap": BOOTSTRAP, "seed": SEED, "nj.nwk": top["nwk"], "support": top["support"], "light": top["light"], "phi_sum": top["phi_sum"], "boot.tsv": top["tsv"],
          "boottrees": top["boottrees"], "genes": {}}
    for k in sorted(files):
        if k.endswith(".fa.filtered"):
            text = files[k].decode("latin-1")
            fx["genes"][k.split("/")[1]] = nj_transfer_ref.transfer_of_fasta(text, BOOTSTRAP, SEED)["nwk"] if text.count(">") >= 2 else None
    with open(os.path.join(HERE, "nj_transfer.json"), "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    print("nj_transfer:", len(fx["genes"]), "genes;", fx["support"], fx["phi_sum"], fx["nj.nwk"].strip())


if __name__ == "__main__":
    main()
