"""Seeded synthetic NCBI taxdump + blastdbcmd listing for the build-db tests and scripts/db_build_bench.py.

Exact NCBI dump syntax ("\\t|\\t" between fields, "\\t|\\n" at the end).  It controls the node count and depth, the rank mix
(no rank, clade, superkingdom, strains, ...), duplicate and missing names, quotes, the name `null`, non-ASCII names, nodes
without a lineage line, merged and deleted ids (chains included), and an accession listing with unknown, deleted, merged,
merged-into-nothing, negative, zero and beyond-2^31 taxids.  Test data only: the product never calls it."""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np

RANKS = ["no rank", "clade", "superkingdom", "kingdom", "phylum", "class", "order", "family", "genus", "species",
         "strain", "subspecies", "species group", "Domain", "suborder", "tribe", "isolate", "serotype"]
# rank by depth (the rest drawn from RANKS with these weights)
BACKBONE = ["no rank", "superkingdom", "clade", "phylum", "class", "order", "family", "genus", "species", "strain"]
SYL = ["ba", "cte", "ri", "um", "mo", "na", "des", "ul", "fo", "vi", "bri", "o", "the", "rmo", "to", "ga", "ps", "eu",
       "do", "lac", "tis", "xan", "tho", "co", "ccus"]


def _name(rng, k):
    n = rng.integers(2, 5)
    w = "".join(SYL[int(x)] for x in rng.integers(0, len(SYL), n))
    return w.capitalize() + (" " + "".join(SYL[int(x)] for x in rng.integers(0, len(SYL), 2)) if k % 3 == 0 else "")


def make_taxdump(out_dir: str, n_nodes: int = 50_000, depth: int = 12, n_accessions: int = 200_000, seed: int = 1,
                 oddities: bool = True, extra_accessions: Optional[Dict[str, int]] = None) -> Dict[str, str]:
    """Writes nodes.dmp, names.dmp, taxidlineage.dmp, merged.dmp, delnodes.dmp and accessions.txt under out_dir, and one more
    listing per extra_accessions entry (file name -> lines).  Returns the paths (keys: the dump names without .dmp, and
    "accessions")."""
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    # ids: sparse, distinct, in [2, 3 n + 10); 1 is the root
    ids = rng.choice(np.arange(2, 3 * n_nodes + 10, dtype=np.int64), size=n_nodes - 1, replace=False)
    ids = np.concatenate([[1], ids])
    # levels grow geometrically down to `depth`; each node's parent is a random node of the level above
    w = np.geomspace(1, max(n_nodes / depth, 2), depth)
    w = w / w.sum()
    level = np.sort(rng.choice(depth, size=n_nodes - 1, p=w)) + 1
    level = np.concatenate([[0], level])
    parent = np.zeros(n_nodes, dtype=np.int64)
    starts = np.searchsorted(level, np.arange(depth + 2))
    for lv in range(1, depth + 1):
        a, b = starts[lv], starts[lv + 1]
        pa, pb = starts[lv - 1], starts[lv]
        if b > a:
            parent[a:b] = rng.integers(pa, pb, b - a)
    rank_of = []
    for k in range(n_nodes):
        lv = int(level[k])
        if rng.random() < 0.25:
            rank_of.append(RANKS[int(rng.integers(0, len(RANKS)))])
        else:
            rank_of.append(BACKBONE[min(lv, len(BACKBONE) - 1)] if lv < len(BACKBONE) else "no rank")
    # lineages (root excluded, as NCBI's taxidlineage.dmp)
    lin = [""] * n_nodes                                               # "a b c " (NCBI ends it with a space)
    par = parent.tolist()
    idl = ids.tolist()
    for k in range(1, n_nodes):
        p = par[k]
        lin[k] = (lin[p] + f"{idl[p]} ") if p != 0 else ""
    nodes_l, names_l, lin_l = [], [], []
    for k in range(n_nodes):
        t = int(ids[k])
        nodes_l.append(f"{t}\t|\t{int(ids[int(parent[k])])}\t|\t{rank_of[k]}\t|\t\t|\t0\t|\t1\t|\t11\t|\t1\t|\t0\t|\t1\t|\t0\t|\t0\t|\t\t|\n")
        lin_l.append(f"{t}\t|\t{lin[k]}\t|\n")
        nm = _name(rng, k)
        u = rng.random()
        if oddities and u < 0.01:
            continue                                                    # no scientific name: taxid-<id>
        if oddities and u < 0.015:
            nm = "null"
        elif oddities and u < 0.02:
            nm = f'"{nm}" var. "x"'
        elif oddities and u < 0.022:
            nm = nm + " café"
        elif oddities and u < 0.03:
            names_l.append(f"{t}\t|\t{_name(rng, k + 1)}\t|\t\t|\tscientific name\t|\n")   # a duplicate: the last one wins
        names_l.append(f"{t}\t|\t{nm}\t|\t\t|\tscientific name\t|\n")
        if rng.random() < 0.3:
            names_l.append(f"{t}\t|\t{_name(rng, k + 2)}\t|\t\t|\tsynonym\t|\n")
    if oddities:
        # nodes without a lineage line (they do not exist), lineage lines without a node
        drop = set(int(x) for x in rng.choice(np.arange(1, n_nodes), size=max(n_nodes // 500, 1), replace=False))
        lin_l = [l for k, l in enumerate(lin_l) if k not in drop]
        lin_l.append(f"{3 * n_nodes + 20}\t|\t1 \t|\n")
    perm = rng.permutation(len(nodes_l))                               # the files are not in taxid order
    nodes_l = [nodes_l[i] for i in perm]
    # merged / deleted ids: outside the node ids
    spare = np.setdiff1d(np.arange(3 * n_nodes + 10, 3 * n_nodes + 10 + max(n_nodes // 20, 20), dtype=np.int64), ids)
    rng.shuffle(spare)
    q = len(spare) // 5
    merged_ok, merged_missing, deleted, both, chain = spare[:q], spare[q:2 * q], spare[2 * q:3 * q], spare[3 * q:3 * q + q // 2], spare[3 * q + q // 2:4 * q]
    merged_l = [f"{int(o)}\t|\t{int(ids[int(rng.integers(0, n_nodes))])}\t|\n" for o in merged_ok]
    merged_l += [f"{int(o)}\t|\t{int(o) + 10 * n_nodes}\t|\n" for o in merged_missing]
    merged_l += [f"{int(o)}\t|\t{int(ids[1])}\t|\n" for o in both]
    merged_l += [f"{int(o)}\t|\t{int(merged_ok[0]) if len(merged_ok) else 1}\t|\n" for o in chain]   # into a merged id: not followed
    del_l = [f"{int(d)}\t|\n" for d in np.concatenate([deleted, both])]
    pools = (ids, merged_ok, merged_missing, deleted, both, chain)
    acc_path = os.path.join(out_dir, "accessions.txt")
    _write_accessions(acc_path, rng, pools, n_nodes, n_accessions, oddities)
    for name, n in (extra_accessions or {}).items():
        _write_accessions(os.path.join(out_dir, name), np.random.default_rng(seed + n), pools, n_nodes, n, oddities)
    paths = {}
    for name, lines in (("nodes", nodes_l), ("names", names_l), ("taxidlineage", lin_l), ("merged", merged_l),
                        ("delnodes", del_l)):
        paths[name] = os.path.join(out_dir, name + ".dmp")
        with open(paths[name], "w") as f:
            f.write("".join(lines))
    paths["accessions"] = acc_path
    return paths


def _write_accessions(acc_path, rng, pools, n_nodes, n_accessions, oddities):
    ids, merged_ok, merged_missing, deleted, both, chain = pools
    u = rng.random(n_accessions)
    tax = ids[rng.integers(0, n_nodes, n_accessions)].astype(np.int64)
    if oddities:
        pools = [(0.010, merged_ok), (0.015, merged_missing), (0.020, deleted), (0.022, both), (0.024, chain)]
        lo = 0.0
        for hi, pool in pools:
            sel = (u >= lo) & (u < hi)
            if len(pool):
                tax[sel] = pool[rng.integers(0, len(pool), int(sel.sum()))]
            lo = hi
        tax[(u >= 0.024) & (u < 0.026)] = rng.integers(10 * n_nodes, 20 * n_nodes, int(((u >= 0.024) & (u < 0.026)).sum()))
        tax[(u >= 0.026) & (u < 0.0265)] = -rng.integers(1, 1000, int(((u >= 0.026) & (u < 0.0265)).sum()))
        tax[(u >= 0.0265) & (u < 0.027)] = 0
        tax[(u >= 0.027) & (u < 0.0275)] = (1 << 31) + rng.integers(0, 1000, int(((u >= 0.027) & (u < 0.0275)).sum()))
    with open(acc_path, "w") as f:
        chunk = 1 << 20
        for a in range(0, n_accessions, chunk):
            b = min(a + chunk, n_accessions)
            f.write("".join(f"NR_{i:09d}.1  {t}  {i}\n" for i, t in zip(range(a, b), tax[a:b].tolist())))
