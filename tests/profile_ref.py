"""Rule UC-P (`unicore profile`) in plain Python: dicts and sets, written from the rule's statement, for the tests to hold the
host and device counters and the output files against.  No product code is involved.

profile_text(map_text, tsv_text, threshold) -> dict:
    groups   list of (name, single, multiple, core) in group order
    files    {file name: bytes} of the output directory (gene files, copiness.tsv, profile.chk)
    full     {species: core groups in which the species has exactly one row}
    n_core   number of core groups (a name that heads two runs counts twice)
    warnings the warning lines, ascending species
arrays(map_text, tsv_text) -> the counter's inputs (group, gene, n_groups, sp_off, sp, n_species) with the names behind the ids
count(...) -> the counter's outputs from those arrays (same rule, same orders)
"""
from decimal import Decimal

import numpy as np

NO_GENE = 0xFFFFFFFF


def percent(x):
    """a double as the copiness file prints it: shortest round-trip decimal, no exponent, no trailing .0"""
    if x != x:
        return "NaN"
    s = format(Decimal(repr(float(x))), "f")
    return s[:-2] if s.endswith(".0") else s


def read_map(map_text):
    """gene -> set of species, and the species in byte order"""
    species_of = {}
    for line in map_text.split(b"\n"):
        if line == b"":
            continue
        f = line.split()
        species_of.setdefault(f[0], set()).add(f[1])
    species = sorted({s for v in species_of.values() for s in v})
    return species_of, species


def read_groups(tsv_text):
    """[(name, [gene, ...])]: maximal runs of rows with the same first field"""
    groups = []
    for line in tsv_text.split(b"\n"):
        if line == b"":
            continue
        f = line.split()
        if not groups or groups[-1][0] != f[0]:
            groups.append((f[0], []))
        groups[-1][1].append(f[1])
    return groups


def file_name(group_name):
    parts = group_name.split(b"-")
    return (parts[1] if len(parts) > 1 else group_name) + b".txt"


def profile_text(map_text, tsv_text, threshold):
    species_of, species = read_map(map_text)
    S = len(species)
    files = {}
    rows = [b"Query\tMultipleCopyPercent\tSingleCopyPercent\n"]
    full = {s: 0 for s in species}
    out_groups, n_core = [], 0
    for name, genes in read_groups(tsv_text):
        cnt, distinct = {}, {}
        for gene in genes:
            for s in species_of.get(gene, ()):
                cnt[s] = cnt.get(s, 0) + 1
                distinct.setdefault(s, set()).add(gene)
        multiple = len(cnt)
        single = sum(1 for c in cnt.values() if c == 1)
        core = single * 100 >= threshold * S
        out_groups.append((name, single, multiple, core))
        mp = multiple * 100.0 / S if S else float("nan")
        sp = single * 100.0 / S if S else float("nan")
        rows.append(name + b"\t" + percent(mp).encode() + b"\t" + percent(sp).encode() + b"\n")
        if core:
            n_core += 1
            files[file_name(name).decode()] = b"".join(next(iter(distinct[s])) + b"\t" + s + b"\n" for s in sorted(distinct) if len(distinct[s]) == 1)
            for s, c in cnt.items():
                if c == 1:
                    full[s] += 1
    files["copiness.tsv"] = b"".join(rows)
    files["profile.chk"] = b"1"
    half = (n_core + 1) // 2
    warnings = ["Warning: Species %s has only %d core genes out of %d core genes" % (s.decode(), full[s], n_core) for s in species if full[s] < half]
    return {"groups": out_groups, "files": files, "full": full, "n_core": n_core, "warnings": warnings}


def arrays(map_text, tsv_text):
    species_of, species = read_map(map_text)
    sid = {s: k for k, s in enumerate(species)}
    genes = list(species_of)
    gid = {g: k for k, g in enumerate(genes)}
    sp_off, sp = [0], []
    for g in genes:
        sp.extend(sorted(sid[s] for s in species_of[g]))
        sp_off.append(len(sp))
    group, gene, names = [], [], []
    for k, (name, members) in enumerate(read_groups(tsv_text)):
        names.append(name)
        group.extend([k] * len(members))
        gene.extend(gid.get(m, NO_GENE) for m in members)
    return {"group": np.array(group, np.uint32), "gene": np.array(gene, np.uint32), "n_groups": len(names), "sp_off": np.array(sp_off, np.uint64),
            "sp": np.array(sp, np.uint32), "n_species": len(species), "group_names": names, "gene_names": genes, "species_names": species}


def count(group, gene, n_groups, sp_off, sp, n_species, threshold):
    """the counter's outputs (the dict of unicore_amd.profile_count) by the rule, one group at a time"""
    group, gene = np.asarray(group).tolist(), np.asarray(gene).tolist()
    sp_off, sp = np.asarray(sp_off).tolist(), np.asarray(sp).tolist()
    members = [[] for _ in range(n_groups)]
    for g, x in zip(group, gene):
        members[g].append(x)
    single, multiple, core = np.zeros(n_groups, np.uint32), np.zeros(n_groups, np.uint32), np.zeros(n_groups, np.uint8)
    full, core_off, cg, cs = np.zeros(n_species, np.uint32), np.zeros(n_groups + 1, np.uint64), [], []
    for g in range(n_groups):
        cnt, distinct = {}, {}
        for x in members[g]:
            if x == NO_GENE:
                continue
            for s in sp[sp_off[x]:sp_off[x + 1]]:
                cnt[s] = cnt.get(s, 0) + 1
                distinct.setdefault(s, set()).add(x)
        multiple[g] = len(cnt)
        single[g] = sum(1 for c in cnt.values() if c == 1)
        core[g] = int(single[g]) * 100 >= threshold * n_species
        if core[g]:
            for s in sorted(cnt):
                if cnt[s] == 1:
                    full[s] += 1
                if len(distinct[s]) == 1:
                    cg.append(next(iter(distinct[s])))
                    cs.append(s)
        core_off[g + 1] = len(cg)
    return {"single": single, "multiple": multiple, "core": core, "full": full, "core_off": core_off,
            "core_gene": np.array(cg, np.uint32), "core_species": np.array(cs, np.uint32)}
