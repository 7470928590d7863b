#!/usr/bin/env python3
"""Regenerate tests/golden/profile_default_t80.json: the output directory of `unicore profile -t 80` (rule UC-P) for
tests/golden/clust_default.tsv with tests/golden/db.map, file name -> contents.  The rule is the test-side Python reference
(tests/profile_ref.py).  No product code is involved.
Run from the repo root:  python tests/golden/make_profile_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import profile_ref  # noqa: E402


def main():
    r = profile_ref.profile_text(open(os.path.join(HERE, "db.map"), "rb").read(), open(os.path.join(HERE, "clust_default.tsv"), "rb").read(), 80)
    with open(os.path.join(HERE, "profile_default_t80.json"), "w") as f:
        json.dump({k: v.decode("ascii") for k, v in sorted(r["files"].items())}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("profile_default_t80:", len(r["groups"]), "groups,", r["n_core"], "core,", len(r["files"]), "files")


if __name__ == "__main__":
    main()
