#!/usr/bin/env python3
"""tools/slot_balance.py - on the GPU box: how many issued wave instructions of the packed gapped passes (MODE 0 / 1 / 6, table 1) compute
nothing because the lane groups of one wave finish at different times, per class, and what a workgroup that pulls the slots of K neighbouring
tasks (merged by step count) would lose instead.  A MODEL of the kernel's slot streaming (uc_sw_pk_impl.hpp), not a measurement:
  * pair lists: the prefilter's hit lists (Engine.hits) oriented and deduplicated as forward_pass does (shorter sequence = query, ties by id);
    MODE 1 = the pairs whose record carries a reversed-query score, MODE 6 = the pairs that pass the E-value gate (Engine.alns), target
    length = end column + 1 there.  (The engine's own MODE 1 list also holds the pairs whose reversed score came out 0: a little larger.)
  * sorted by (class, query, target length descending), cut at tcap; tasks in LPT order inside a class (pairs x longest target, descending)
  * slot i = pairs 2i / 2i+1 of a task, (max(tlenA, tlenB) + G) & ~1 steps; slots go to the NG lane groups of the workgroup greedily in list
    order (the LDS counter); a wave issues for as long as its slowest group runs; 10 R + 35 instructions per step
usage: slot_balance.py [--config c2] [--k 1,2,4] [--groups 8] [--scale-groups] [--times <trace directory>]   (--times: per-class kernel times of a
UC_STREAMS=1 trace beside the model's issued counts: ns per modelled wave instruction should be flat across classes if the model holds)"""
import argparse, collections, csv, os, re, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# table 1 of uc_sw_plan.hip
CAP = np.array([32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 704, 768, 896, 1024, 1152, 1280, 1408, 1536, 1664, 1792, 1920, 2048])
GRP = np.array([16] * 12 + [32] * 6 + [64] * 10)
ROWS = np.array([2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 14, 16, 18, 20, 22, 24, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32])
TCAP = np.array([64] * 18 + [48] * 6 + [24] * 4)


def nwaves(G, R):
    return 2 if G == 16 else (4 if G == 32 else (2 if R < 14 else 8))


def pass_lists(config):
    """(q, tlen) of the three passes, oriented and deduplicated, from one prefilter + align of the bench database"""
    import bench, unicore_amd as U
    proteomes, families, scale, seed, options, _ = bench.CONFIGS[config]
    wd = os.path.join(os.environ.get("UC_BENCH_DIR", "/tmp/uc_bench"), "p%d_f%d_s%g_%x" % (proteomes, families, scale, seed))   # bench.py's own
    prefix = bench.gen_db(wd, proteomes, families, scale, seed)
    lens = bench.read_lens(prefix).astype(np.int64)
    e = U.Engine(options, verbosity=1)
    e.load_db(prefix)
    e.prefilter(); e.align()
    cnt, hits = e.hits()
    al = e.alns()
    q = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt); t = hits["target"].astype(np.int64)
    swap = (lens[q] > lens[t]) | ((lens[q] == lens[t]) & (q > t))            # ukey_kernel: the worse orientation of a mutual hit
    oq, ot = np.where(swap, t, q), np.where(swap, q, t)
    te = np.where(swap, al["qend"], al["tend"]).astype(np.int64)             # end column in the oriented target
    key = np.minimum(q, t) * (1 << 24) + np.maximum(q, t)
    order = np.argsort(key, kind="stable")
    first = np.ones(len(order), bool); first[1:] = key[order][1:] != key[order][:-1]
    grp = np.cumsum(first) - 1                                               # unordered pair of every sorted entry
    n_u = int(grp[-1]) + 1 if len(grp) else 0
    rev = np.zeros(n_u, bool); np.logical_or.at(rev, grp, (al["score_rev"][order] != 0) | (al["pass_evalue"][order] != 0))
    gate = np.zeros(n_u, bool); np.logical_or.at(gate, grp, al["pass_evalue"][order] != 0)
    tend = np.zeros(n_u, np.int64); np.maximum.at(tend, grp, np.where(al["pass_evalue"][order] != 0, te[order], 0))
    uq, ut = oq[order][first], ot[order][first]
    return lens, {0: (uq, lens[ut]), 1: (uq[rev], lens[ut][rev]), 6: (uq[gate], tend[gate] + 1)}


def tasks_of(lens, q, tl):
    """per class: list of tasks (arrays of slot step counts) in LPT order"""
    cls = np.searchsorted(CAP, lens[q], side="left")
    keep = cls < len(CAP)
    q, tl, cls = q[keep], tl[keep], cls[keep]
    o = np.lexsort((-tl, q, cls))
    q, tl, cls = q[o], tl[o], cls[o]
    out = {}
    for c in np.unique(cls):
        m = cls == c
        qc, tc = q[m], tl[m]
        head = np.ones(len(qc), bool); head[1:] = qc[1:] != qc[:-1]
        seg = np.maximum.accumulate(np.where(head, np.arange(len(qc)), 0))
        pos = np.arange(len(qc)) - seg
        thead = pos % TCAP[c] == 0
        tid = np.cumsum(thead) - 1                                           # task of every pair
        tpos = pos % TCAP[c]
        nt = int(tid[-1]) + 1
        count = np.bincount(tid, minlength=nt)
        work = count * tc[thead]
        lpt = np.argsort(-work, kind="stable")
        rank = np.empty(nt, np.int64); rank[lpt] = np.arange(nt)
        S = np.zeros((nt, (TCAP[c] + 1) // 2), np.int64)
        a = tpos % 2 == 0                                                    # the longer pair of a slot (lists are sorted descending)
        S[rank[tid[a]], tpos[a] // 2] = (tc[a] + GRP[c]) & ~1
        out[int(c)] = (S, int(len(qc)))
    return out


def issued(S, G, R, K, ng):
    """(issued wave instructions, of which lost to groups waiting for the slowest of their wave) for workgroups of K neighbouring tasks"""
    nt, ns = S.shape
    nb = (nt + K - 1) // K
    M = np.zeros((nb * K, ns), np.int64); M[:nt] = S
    M = -np.sort(-M.reshape(nb, K * ns), axis=1) if K > 1 else M             # merged by step count, descending
    M = M[:, : max(1, int((M > 0).sum(axis=1).max()))]
    fin = np.zeros((nb, ng), np.int64)
    rows = np.arange(nb)
    for s in range(M.shape[1]):
        j = np.argmin(fin, axis=1) if s >= ng else np.full(nb, s)
        fin[rows, j] += M[:, s]
    gw = 64 // G
    wave = fin.reshape(nb, ng // gw, gw).max(axis=2)
    per_step = 10 * R + 35
    iss = int(wave.sum()) * per_step
    use = int(fin.sum()) * per_step / gw
    return iss, iss - use


def class_times(d):
    agg = collections.defaultdict(float)
    for r in csv.DictReader(open(d.rstrip("/") + "/out_kernel_stats.csv")):
        m = re.search(r"sw_pk_kernel<(\d+), (\d+), (\d+), (\d+)", r["Name"])
        if m:
            G, R, M = int(m.group(1)), int(m.group(2)), int(m.group(3))
            agg[(M, G, R)] += int(r["TotalDurationNs"])
    return agg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--k", default="1,2,4")
    ap.add_argument("--groups", type=int, default=0, help="lane groups per workgroup (0: the kernel's, NW * 64 / G)")
    ap.add_argument("--scale-groups", action="store_true", help="K tasks on K times the lane groups (what sw_pk_kernel<.., NW * K, K> runs), not on the same workgroup")
    ap.add_argument("--times", help="directory of a serialized kernel trace (tools/prof_serial.sh)")
    ap.add_argument("--calls", type=float, default=2.0, help="steps the trace ran (warm-up + timed)")
    args = ap.parse_args()
    ks = [int(x) for x in args.k.split(",")]
    times = class_times(args.times) if args.times else {}
    lens, lists = pass_lists(args.config)
    for mode in (0, 1, 6):
        q, tl = lists[mode]
        T = tasks_of(lens, q, tl)
        print("MODE %d: %d pairs" % (mode, len(q)))
        print("  class  G  R     pairs   tasks slots/task" + "".join("   issued(K=%d)  lost" % k for k in ks) + ("   kernel ms  ns/Minstr" if times else ""))
        tot = {k: [0, 0, 0, 0] for k in ks}
        for c in sorted(T):
            S, npairs = T[c]
            G, R = int(GRP[c]), int(ROWS[c])
            ng = args.groups or nwaves(G, R) * 64 // G
            line = "  %5d %2d %2d %9d %7d %10.1f" % (CAP[c], G, R, npairs, len(S), (S > 0).sum() / len(S))
            for k in ks:
                kk = k if G < 64 else 1
                iss, lost = issued(S, G, R, kk, ng * kk if args.scale_groups else ng)
                line += " %13.4g %5.1f%%" % (iss, 100.0 * lost / iss)
                tot[k][0] += iss; tot[k][1] += lost
                if G < 64: tot[k][2] += iss; tot[k][3] += lost
            if times:
                ns = times.get((mode, G, R), 0.0) / args.calls
                line += " %10.2f %10.1f" % (ns / 1e6, ns / (issued(S, G, R, 1, ng)[0] / 1e6))
            print(line)
        for k in ks:
            print("  K=%d: issued %.4g wave instructions, lost %.1f%% (G < 64 classes: %.1f%%, their share of issued %.2f)" % (
                k, tot[k][0], 100.0 * tot[k][1] / tot[k][0], 100.0 * tot[k][3] / max(tot[k][2], 1), tot[k][2] / tot[k][0]))


if __name__ == "__main__":
    main()
