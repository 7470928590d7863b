"""Writes tests/golden/long_aln.json: the oracle's records of the nat cases of tests/long_aln_cases.py (default gap costs, boxes of
32,767^2 to about 33,000^2 cells), with the options, the seeds and a sha256 of each input sequence pair.  The sequences themselves are
regenerated from the seeds, never stored.

    python tests/golden/make_long_aln.py            write the fixture
    python tests/golden/make_long_aln.py --check    regenerate and compare with the committed file (exit status 1 on a difference)

Both orders of a pair are recorded.  The two sequences of an identical pair are equal, so its second order is the same computation and is
copied; the mutated pair runs twice.  One run: 86 s on one CPU core (four gapped passes and a byte-per-cell traceback per
record, about 1.1 G cells each).
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")

import long_aln_cases as L  # noqa: E402
from oracle import oracle_py as O  # noqa: E402


def make():
    p = L.params(O, L.NAT_OPTS)
    cases = {}
    for name, c in L.NAT_CASES.items():
        q, t = L.nat_sequences(name)
        if c["kind"] == "identical":
            assert (q[0] == t[0]).all() and (q[1] == t[1]).all()
            odb = O.OracleDb(s3=[q[0], t[0]], sa=[q[1], t[1]])
            r = O.align_pair(odb, p, 0, 1, O.min_score(odb, p, 0))
            rec = {f: int(r[f]) for f in L.FIELDS}
            st = O.traceback_lean(odb, p, 0, 1, rec["qstart"], rec["qend"], rec["tstart"], rec["tend"])
            assert st[:3] == (rec["aln_len"], rec["idents"], rec["gap_opens"])
            ref = [(rec, st[3]), (dict(rec), st[3])]
        else:
            ref = L.reference(O, p, q, t)
        cases[name] = dict(kind=c["kind"], seed=c["seed"], n=c["n"], len_q=len(q[0]), len_t=len(t[0]), sha256_q=L.sha(q), sha256_t=L.sha(t),
                           records=[r for r, _ in ref], tie=[int(x) for _, x in ref])
    return dict(options=("-c 0 " + L.NAT_OPTS).strip(), min_seq_ids=list(L.NAT_SEQ_IDS), fields=list(L.FIELDS), cases=cases)


if __name__ == "__main__":
    t0 = time.time()
    fx = make()
    text = json.dumps(fx, indent=1, sort_keys=True) + "\n"
    if "--check" in sys.argv[1:]:
        same = open(L.FIXTURE).read() == text
        print("long_aln.json: %s (%.0f s)" % ("reproduced" if same else "DIFFERS", time.time() - t0))
        sys.exit(0 if same else 1)
    open(L.FIXTURE, "w").write(text)
    print("wrote %s (%.0f s)" % (L.FIXTURE, time.time() - t0))
