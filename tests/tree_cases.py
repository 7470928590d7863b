"""Inputs of the rule UC-T tests, shared by test_tree.py (host twins) and test_tree_gpu.py (device): hand-made groups, a seeded generator of valid
backtraces (no DP involved), centre matrices and filter grids.  A *case* is the keyword dict of unicore_amd.msa_star / msa_ref.star."""
import numpy as np

M, I, D = 0, 1, 2
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYXacdxy", np.uint8)      # as stored: lower case and X pass through


def build(groups, seed=0):
    """groups: list of (Lc, centre index, rows); a row is None (unaligned) or (qs, ts, [(length, op), ...], extra tail residues); the centre's
    row sits at `centre index` among them.  Returns the case dict."""
    rng = np.random.default_rng(seed)
    grp_off, centre, lens, qs, ts, aligned, run_off, runs = [0], [], [], [], [], [], [0], []
    for Lc, c, rows in groups:
        rows = list(rows)
        rows.insert(c, "centre")
        centre.append(c)
        for r in rows:
            if r == "centre":
                lens.append(Lc); qs.append(0); ts.append(0); aligned.append(1)
            elif r is None:
                lens.append(int(rng.integers(0, 30))); qs.append(-7); ts.append(-7); aligned.append(0)      # never read
            else:
                q, t, rr, tail = r
                lens.append(t + sum(n for n, op in rr if op != I) + tail)
                qs.append(q); ts.append(t); aligned.append(1)
                runs.extend(n << 2 | op for n, op in rr)
            run_off.append(len(runs))
        grp_off.append(len(lens))
    res_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    tot = int(res_off[-1])
    return dict(grp_off=np.array(grp_off, np.uint64), centre=np.array(centre, np.uint32), res_off=res_off,
                res=[LETTERS[rng.integers(0, len(LETTERS), tot)], LETTERS[rng.integers(0, 20, tot)]],
                qs=np.array(qs, np.int32), ts=np.array(ts, np.int32), run_off=np.array(run_off, np.uint64), runs=np.array(runs, np.uint32),
                aligned=np.array(aligned, np.uint8))


def random_row(rng, Lc):
    if rng.random() < 0.12:
        return None
    qs = int(rng.integers(0, Lc // 3 + 1)) if rng.random() < 0.5 else 0
    end = Lc if rng.random() < 0.5 else int(rng.integers(qs, Lc + 1))
    s, rr, prev = qs, [], None
    while s < end:
        ops = [o for o in (M, M, M, I, D) if o != prev]
        op = ops[int(rng.integers(0, len(ops)))]
        if op == D:
            n = int(rng.integers(1, 6))
        else:
            n = min(int(rng.integers(1, 12)), end - s)
            s += n
        rr.append((n, op)); prev = op
    if rng.random() < 0.3 and prev != D:
        rr.append((int(rng.integers(1, 5)), D))
    return qs, int(rng.integers(0, 4)), rr, int(rng.integers(0, 3))


def random_groups(rng, sizes, lmax=40):
    out = []
    for m in sizes:
        Lc = int(rng.integers(0, lmax + 1))
        out.append((Lc, int(rng.integers(0, m)), [random_row(rng, Lc) for _ in range(m - 1)]))
    return out


def events(groups):
    """what a list of groups exercises: shared insert slots with unequal lengths, inserts behind the last centre residue, unaligned rows, qs > 0"""
    ev = dict(shared_unequal=0, trailing=0, unaligned=0, qs_positive=0)
    for Lc, _, rows in groups:
        slots = {}
        for r in rows:
            if r is None:
                ev["unaligned"] += 1
                continue
            q, _, rr, _ = r
            ev["qs_positive"] += q > 0
            s = q
            for n, op in rr:
                if op == D:
                    slots.setdefault(s, []).append(n)
                    ev["trailing"] += s == Lc
                else:
                    s += n
        ev["shared_unequal"] += sum(1 for v in slots.values() if len(set(v)) > 1)
    return ev


def hand_cases():
    rng = np.random.default_rng(11)
    full = lambda L: (0, 0, [(L, M)], 0)
    cases = {
        "one_row": [(17, 0, [])],
        "two_rows": [(12, 1, [(0, 0, [(5, M), (2, D), (7, M)], 1)])],
        "unaligned_row": [(9, 0, [full(9), None, (2, 1, [(4, M)], 0)])],
        "same_slot_two_lengths": [(10, 1, [(0, 0, [(4, M), (3, D), (6, M)], 0), (0, 2, [(4, M), (5, D), (6, M)], 0), (1, 0, [(3, M), (1, D), (2, M)], 2)])],
        "slot_0_and_slot_Lc": [(8, 0, [(0, 0, [(3, D), (8, M)], 0), (0, 1, [(8, M), (2, D)], 0), (0, 0, [(1, D), (8, M), (4, D)], 0)])],
        "box_inside": [(20, 2, [(6, 3, [(9, M)], 4), (0, 0, [(11, M)], 0), (19, 0, [(1, M)], 0)])],
        "I_then_D": [(14, 0, [(0, 0, [(5, M), (2, I), (3, D), (7, M)], 0), (1, 0, [(4, M), (2, D), (3, I), (6, M)], 0)])],
        "insert_70_in_300": [(300, 1, [(0, 0, [(150, M), (70, D), (150, M)], 0), (10, 5, [(140, M), (3, D), (100, M)], 0)])],
        "rows_70": [(30, 33, [random_row(rng, 30) for _ in range(69)])],
        "empty_length_centre": [(0, 0, [(0, 0, [(4, D)], 1), None])],
        "groups_200": random_groups(rng, [1 + k % 40 for k in range(200)]),
    }
    return {k: (v, build(v, seed=len(k))) for k, v in cases.items()}


def empty_case():
    return build([])


def centre_cases():
    """name -> (grp_off, scores, the expected centres where they are chosen by hand or None)"""
    rng = np.random.default_rng(5)
    tri = lambda m: m * (m - 1) // 2
    out = {
        "one_row": ([0, 1], [], [0]),
        "two_rows_tie": ([0, 2], [9], [0]),
        "all_zero": ([0, 6], [0] * tri(6), [0]),
        # rows 1 and 3 tie at the top (sums 9 + 1 + 5 = 15 = 1 + 9 + 5): the earlier wins
        "tie_later_rows": ([0, 4], [9, 0, 1, 1, 5, 9], [1]),
        "rows_130": ([0, 130], rng.integers(0, 2000, tri(130)).tolist(), None),
        "large_sums": ([0, 3], [2**31 - 1, 2**31 - 1, 2**31 - 1], [0]),       # a row sum past 32 bits
    }
    sizes = [1 + k % 40 for k in range(200)]
    out["groups_200"] = (np.concatenate([[0], np.cumsum(sizes)]).tolist(), rng.integers(0, 50, sum(tri(m) for m in sizes)).tolist(), None)
    out["empty"] = ([0], [], [])
    return out


def filter_cases():
    """name -> (grp_off, width, cells, threshold, expected fwidth or None)"""
    def grid(rows):
        return np.frombuffer("".join(rows).encode(), np.uint8)
    g4 = ["AC-E", "A--E", "-G-E", "---E"]                    # counts 2, 2, 0, 4 of 4 rows
    g3 = ["A--", "---", "---"]
    both = np.concatenate([grid(g4), grid(g3)])
    rng = np.random.default_rng(3)
    big_m, big_w = 70, 333
    big = np.where(rng.random((big_m, big_w)) < 0.5, ord("-"), ord("K")).astype(np.uint8).reshape(-1)
    return {
        "threshold_0": ([0, 4, 7], [4, 3], both, 0, [4, 3]),
        "threshold_100": ([0, 4, 7], [4, 3], both, 100, [1, 0]),
        "exactly_equal": ([0, 4], [4], grid(g4), 50, [3]),       # 2 * 100 == 50 * 4 keeps, 0 drops
        "one_below": ([0, 4], [4], grid(g4), 51, [1]),           # 200 < 204
        "loses_every_column": ([0, 3], [3], grid(g3), 34, [0]),  # 100 < 102
        "one_third_exact": ([0, 3], [3], grid(g3), 33, [1]),     # 100 >= 99
        "rows_70_width_333": ([0, big_m], [big_w], big, 50, None),
        "zero_width_between": ([0, 2, 3, 5], [2, 0, 1], grid(["A-", "-A", "-", "C"]), 50, [2, 0, 1]),
        "empty": ([0], [], np.zeros(0, np.uint8), 50, []),
    }
