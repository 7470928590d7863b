"""Writes tests/golden/tree_progressive_d50.json: what `unicore tree -n -a progressive` must write on the golden database's 11 genes, from the Python
reference alone (msa_ref.py + msa_progressive_ref.py over the CPU oracle; no product code).  Same digest as tree_default_d50.json: the two
concatenation files in full, a sha256 per gene file.  Run from the repository root:
    python tests/golden/make_tree_progressive_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")

import msa_progressive_ref as G  # noqa: E402
import msa_ref as R  # noqa: E402
import util  # noqa: E402
from oracle import oracle_py as O  # noqa: E402


def main():
    prof = json.load(open(os.path.join(HERE, "profile_default_t80.json")))
    genes = {k: v.encode("ascii") for k, v in prof.items() if k.endswith(".txt")}
    files, _ = G.tree_files(O, util.oracle_params(O, R.FIXED_OPTS), os.path.join(HERE, "db"), genes, 50)
    out = R.digest(files)
    star = json.load(open(os.path.join(HERE, "tree_default_d50.json")))
    assert out["combined.fasta"] != star["combined.fasta"], "the progressive alignment equals the star alignment: the fixture would show nothing"
    json.dump(out, open(os.path.join(HERE, "tree_progressive_d50.json"), "w"), indent=1, sort_keys=True)
    print("written: %d bytes of combined.fasta" % len(out["combined.fasta"]))


if __name__ == "__main__":
    main()
