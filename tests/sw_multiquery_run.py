"""Child process of tests/test_sw_multiquery_gpu.py::test_same_answers_with_one_task_per_workgroup: one random pair list on a generated 2-proteome
database through Engine.sw_pass (table 1) in modes 0, 1, 4 and 6, every output array saved to argv[2] (.npz) together with the engine's count of
tasks served several to a workgroup.  A process of its own because UC_SW_TASK_QUERIES is read once per process."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
os.environ.setdefault("UC_ALLOW_SYNTHETIC", "1")

import util                # noqa: E402

N_PAIRS = 4000


def main():
    import unicore_amd as U
    prefix = util.gen_synth_db(os.path.join(sys.argv[1], "db"), 2, 0x5EED0011, 600, 0.7)
    e = U.Engine("-c 0.8", verbosity=1)
    e.load_db(prefix)
    rng = np.random.default_rng(11)
    # ~ 650 sequences of 30 .. 1400 residues: lists of about 6 pairs (1 .. 15) per query, unrelated and (same family) related targets alike
    q = rng.integers(0, e.n, N_PAIRS).astype(np.uint32)
    t = rng.integers(0, e.n, N_PAIRS).astype(np.uint32)
    out = {}
    r = e.sw_pass(1, 0, q, t)
    fwd = r
    for k in ("score", "qe", "te", "cls"):
        out["m0_" + k] = r[k]
    out["m1_score"] = e.sw_pass(1, 1, q, t)["score"]
    pos = np.nonzero(fwd["score"] > 0)[0]
    known = fwd["score"][pos].astype(np.int32)
    ends = np.zeros((len(pos), 4), np.int32)
    ends[:, 1], ends[:, 3] = fwd["qe"][pos], fwd["te"][pos]
    r = e.sw_pass(1, 4, q[pos], t[pos], known=known, raw=True, second=True)
    for k in ("score", "qe", "te", "qe2", "te2"):
        out["m4_" + k] = r[k]
    r = e.sw_pass(1, 6, q[pos], t[pos], box=ends, known=known, raw=True, second=True)
    for k in ("score", "qe", "te", "qe2", "te2"):
        out["m6_" + k] = r[k]
    st = e.stats()
    out["multiquery"] = np.array([st["sw_multiquery_launches"], st["sw_multiquery_tasks"], len(pos)], np.int64)
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
