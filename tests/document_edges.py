"""Generator and reference of the document-level edge cases: what lies between the engine's records and the
document a user receives — the top-row compaction (`top_rows_kernel`, csrc/engine_dev.hip, and its host twin
`top_rows_from_columns`, csrc/pipeline_render.cpp), the packed / f64 route choice of `device_run_consensus` and
`Renderer::compute` — fed with segments longer than one 64-row sweep, non-rendered queries at chosen wave slots, scores at the
ends of int32, identities on both sides of the packed limit, top groups whose lineages differ in length and bean lists whose
order hangs on the accession bytes.

No product code here.  Every expected value is the faithful oracle's (oracle/blu_oracle.cpp) on an independent Python reading
of the two input files (`oracle_from_files`), never the library's.  The tables are written with their queries in byte order
of the names, so a query's index in name order is its index in the hit table (the `q` of `top_rows_kernel`): `q % 8` is its slot
in a wave, `q % 32` its slot in a block.

A case is one table over one of the two taxonomies documents; each of its queries records what it claims to be (`Query.claim`),
and tests/test_document_edges.py recomputes every claim from the bytes written and from the oracle's output."""
import dataclasses
import functools
import json
import os

import numpy as np

from oracle import oracle as orc

UNMATCHED_TAXID = 999999999
HEADERS = ["zz_fasta_only_1", "a_fasta_only_0"]          # FASTA ids without a hit: before and behind every query name
STRATEGIES = ("relaxed", "cautious")
RENDERED = "rendered"
NOT_RENDERED = {"unmatched": orc.ST_PANIC_PARSE, "bad": orc.ST_PANIC_PARSE, "root": orc.ST_PANIC_ROOT_DISAGREE,
                "below": orc.ST_PANIC_SINGLE_EMPTY}


def oracle_from_files(bt, tj, use_taxid, taxon, strategy, custom):
    """Independent reading of the two files -> faithful oracle.  {query name: the oracle's result}."""
    db = json.load(open(tj, encoding="utf-8"))
    lin = {}                                           # taxid -> its lineages, one per listing (the left join of mod.rs:72-76
    for t in db["taxonomies"]:                         # gives one joined row per matching taxonomy row, in the DB's order)
        lin.setdefault(int(t["taxid"]), []).append(t["numericLineage"] if use_taxid else t["textLineage"])
    lineages = list(dict.fromkeys(s for v in lin.values() for s in v))
    lin_idx = {s: i for i, s in enumerate(lineages)}
    per_q = {}
    for line in open(bt, encoding="utf-8"):
        c = line.rstrip("\n").split("\t")
        per_q.setdefault(c[0], []).append(c)
    names = list(per_q)
    seg, acc_idx, accs, tax_row, pid, aln, bsc = [0], [], {}, [], [], [], []
    for qn in names:
        for c in per_q[qn]:
            for lineage in lin.get(int(c[2]), [None]):
                acc_idx.append(accs.setdefault(c[1], len(accs)))
                tax_row.append(lin_idx[lineage] if lineage is not None else -1)
                pid.append(float(c[3])); aln.append(int(c[4])); bsc.append(int(float(c[12])))
        seg.append(len(acc_idx))
    tab = orc.HitTable(np.array(seg, np.uint64), np.array(acc_idx, np.uint32), list(accs), np.array(tax_row, np.int64),
                       lineages, np.array(pid), np.array(aln, np.int64), np.array(bsc, np.int64))
    res = orc.run(tab, taxon=taxon, strategy=strategy, custom=custom, threads=4).results()
    return dict(zip(names, res))


# ---- the taxonomies documents ------------------------------------------------------------------------------------------------
# Bacteria: six phyla, below each a binary tree down to the species (192 lineages of seven levels).  Phyla 0 and 5 also list
# every inner node as a taxon of its own (lineages of two to six levels, each a proper prefix of the ones below it; the ragged
# family needs the two- and three-level ones), one genus has forty species more, two Archaea disagree with everything at the
# first level, and one lineage has an element without `__`.  The last entry of the file is the two-level lineage of phylum 5:
# the last row of the library's lineage table is a short one.
RANKS = "dpcofgs"
NAMES = ("Ph", "Cl", "Or", "Fa", "Ge", "Sp")
BIG_GENUS = (1, 0, 0, 0, 0)          # species 0 .. 41
ARCHAEA = ("arch", 0), ("arch", 1)
BAD = ("bad",)


def _lineage(path):
    if path[0] == "arch":
        return "d__Archaea;p__Ar;c__Ar;o__Ar;f__Ar;g__Ar;s__Ar%d" % path[1], "d__2157;p__9;c__9;o__9;f__9;g__9;s__9%d" % path[1]
    if path == BAD:
        return "d__Bacteria;broken", "d__2;broken"
    text, num = ["d__Bacteria"], ["d__2"]
    for k in range(len(path)):
        digits = "".join(str(x) for x in path[:k + 1])
        text.append(f"{RANKS[k + 1]}__{NAMES[k]}{digits}")
        num.append(f"{RANKS[k + 1]}__{k + 3}{digits}")
    return ";".join(text), ";".join(num)


@functools.lru_cache(maxsize=None)
def taxa():
    """[(path, taxid)] in file order."""
    paths = []
    for p in range(6):
        for rest in np.ndindex(2, 2, 2, 2, 2):
            paths.append((p,) + tuple(int(x) for x in rest))
    paths += [BIG_GENUS + (s,) for s in range(2, 42)]
    for p in (0, 5):
        for depth in (5, 4, 3, 2, 1):
            for rest in np.ndindex(*([2] * (depth - 1))):
                if (p, depth) != (5, 1):
                    paths.append((p,) + tuple(int(x) for x in rest))
    paths += [ARCHAEA[0], ARCHAEA[1], BAD, (5,)]
    return [(path, 1000 + i) for i, path in enumerate(paths)]


@functools.lru_cache(maxsize=None)
def taxid_of():
    return dict(taxa())


def tid(*path):
    return taxid_of()[tuple(path)]


DUP_PLAIN = (2, 0, 0, 0, 0, 0)        # listed twice with the same lineage
DUP_CROSS = (2, 0, 0, 0, 0, 1)        # listed again with the lineage of DUP_CROSS_AS (another genus of its family)
DUP_CROSS_AS = (2, 0, 0, 0, 1, 0)
DUP_SHORT = (0, 0, 0)                 # a four-level lineage listed again as its own two-level prefix


def taxonomy_document(dup):
    """The `*.blutils.json` text.  dup: with the taxids of DUP_* listed twice (the left join doubles their rows; the library
    reads such a document's tables with the host parser)."""
    entries = []
    for path, taxid in taxa():
        text, num = _lineage(path)
        entries.append({"taxid": taxid, "rank": "species", "numericLineage": num, "textLineage": text, "accessions": []})
    if dup:
        def again(path, as_path, at):
            text, num = _lineage(as_path)
            entries.insert(at, {"taxid": tid(*path), "rank": "species", "numericLineage": num, "textLineage": text, "accessions": []})
        again(DUP_PLAIN, DUP_PLAIN, 150)
        again(DUP_CROSS, DUP_CROSS_AS, 3)
        again(DUP_SHORT, (0,), 40)
    return json.dumps({"blutilsVersion": "8.3.1", "ignoreTaxids": None, "replaceRank": None, "dropNonLinnaeanTaxonomies": None,
                       "sourceDatabase": "document-edges", "taxonomies": entries})


# ---- cases -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Query:
    name: str
    rows: list                     # (accession, taxid, perc_identity text, align_length, bit-score text) in file order
    claim: dict                    # kind, seg_len, top (indices of the rows on the top score), slot8, slot32 + the family's own


@dataclasses.dataclass
class Case:
    family: str
    name: str
    queries: list
    strategies: tuple = STRATEGIES
    dup: bool = False
    headers: tuple = ()
    route: str = ""                # identity routes: "packed" / "f64", the layout the device call must take

    @property
    def id(self):
        return f"{self.family}-{self.name}"

    def n_lines(self):
        return sum(len(q.rows) for q in self.queries)

    def text(self):
        return "".join(f"{q.name}\t{a}\t{t}\t{p}\t{l}\t3\t1\t1\t400\t5\t404\t1e-120\t{s}\n" for q in self.queries for a, t, p, l, s in q.rows)


def _finish(family, name, queries, **kw):
    """Claims every query shares: filled in from the rows as they were MEANT (test_document_edges recomputes them from the bytes)."""
    queries.sort(key=lambda q: q.name.encode())
    for i, q in enumerate(queries):
        q.claim.setdefault("kind", RENDERED)
        q.claim["seg_len"] = len(q.rows)
        q.claim["slot8"], q.claim["slot32"] = i % 8, i % 32
    return Case(family, name, queries, **kw)


def _pid(k):
    """milli-percent -> the text BLAST prints"""
    return f"{k // 1000}.{k % 1000:03d}"


def _species(q):
    """two sister species, by a running number (phyla 2 .. 4: lineages of seven levels, no duplicates)"""
    g = (2 + q % 3, (q >> 1) & 1, (q >> 2) & 1, (q >> 3) & 1, (q >> 4) & 1)
    return tid(*g, 0), tid(*g, 1)


# family: sweeps ---------------------------------------------------------------------------------------------------------------
SWEEP_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 512, 513, 4097)


def sweep_placements(n):
    """{placement: rows on the top score} for a segment of n rows; placements that coincide at this length are listed once"""
    out = {"whole": list(range(n)), "row0": [0], "last": [n - 1]}
    if n >= 65:
        out["r63_64"] = [63, 64]
    if n > 64 and n % 64:
        out["last_partial"] = list(range(n - n % 64, n))
    seen, keep = [], {}
    for k, v in out.items():
        if v not in seen:
            seen.append(v); keep[k] = v
    return keep


def scattered(n_top, n=200):
    """n_top of n rows, every 64-row sweep holding some"""
    rows = {0, 64, 128, 192, 63, 127, 191, n - 1}
    i = 1
    while len(rows) < n_top:
        rows.add(i % n); i += 3
    return sorted(rows)


def _sweep_query(k, name, n, top):
    a, b = _species(k)
    is_top = set(top)
    rows = []
    for i in range(n):
        low = 499 - i % 7
        score = "500" if i in is_top else (f"{low}.5" if i % 5 == 0 else str(low))     # (x.5 truncates: still below the top)
        rows.append((f"SW{k:03d}_{i:05d}.1", a if (i * 7 + k) % 3 else b, _pid(97000 + (i * 37 + k * 11) % 2999), 300 + i * 13 % 100, score))
    return Query(name, rows, {"top": sorted(top), "n_top": len(top)})


def sweeps_case():
    qs, k = [], 0
    for n in SWEEP_LENGTHS:
        for place, top in sweep_placements(n).items():
            qs.append(_sweep_query(k, f"sw{n:04d}_{place}", n, top)); qs[-1].claim["sweep"] = (n, place); k += 1
    for n_top in (64, 65):
        qs.append(_sweep_query(k, f"sw0200_scattered{n_top}", 200, scattered(n_top))); qs[-1].claim["sweep"] = (200, f"scattered{n_top}"); k += 1
    return _finish("sweeps", "all", qs)


# family: wave slots -----------------------------------------------------------------------------------------------------------
SLOT_COUNTS = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097)
BIG_AT = 12                     # the rendered query of 130 top rows, where the table has one


def slot_positions(nq):
    """slots 0, 7 and 8, the first and the last query, and one whole wave (16 .. 23)"""
    return sorted(p for p in {0, 7, 8, nq - 1, *range(16, 24)} if 0 <= p < nq)


def _kind_rows(kind, q):
    a, b = _species(q)
    ok = (f"K{q:05d}_ok.1", a, "98.500", 400, "300")        # a good row below the top score
    if kind == "unmatched":
        return [ok, (f"K{q:05d}_u.1", UNMATCHED_TAXID, "99.000", 400, "400")], [1]
    if kind == "root":
        return [(f"K{q:05d}_b.1", a, "99.000", 400, "400"), ok, (f"K{q:05d}_a.1", tid(*ARCHAEA[q % 2]), "99.100", 400, "400")], [0, 2]
    if kind == "below":
        return [(f"K{q:05d}_l.1", a, "50.000", 400, "400")], [0]
    if kind == "bad":
        return [(f"K{q:05d}_x.1", tid(*BAD), "99.000", 400, "400"), ok], [0]
    raise KeyError(kind)


def slots_case(nq, kind):
    qs = []
    special = set(slot_positions(nq))
    for q in range(nq):
        name = f"w{q:05d}"
        if q in special:
            rows, top = _kind_rows(kind, q)
            qs.append(Query(name, rows, {"kind": kind, "top": top, "n_top": len(top)}))
            continue
        a, b = _species(q)
        if q == BIG_AT and nq > BIG_AT:
            n, n_top = 133, 130
        else:
            h = q * 2654435761 & 0xFFFFFFFF                       # (lengths 1 .. 6 and group sizes 1 .. length, no period of 8 or 32)
            n = 1 + (h >> 8) % 6
            n_top = 1 + (h >> 16) % n
        top = sorted((q + j) % n for j in range(n_top))          # (a run that starts at row q % n and wraps)
        rows = [(f"W{q:05d}_{i:03d}.1", a if (i + q) % 3 else b, _pid(97000 + (q * 13 + i * 7) % 3000), 380 + (q + i) % 30,
                 "400" if i in top else str(399 - i % 4)) for i in range(n)]
        qs.append(Query(name, rows, {"top": top, "n_top": n_top, "big": n_top == 130}))
    strategy = STRATEGIES[(nq + len(kind)) % 2]
    return _finish("slots", f"{nq}-{kind}", qs, strategies=(strategy,), headers=tuple(HEADERS))


# family: scores ---------------------------------------------------------------------------------------------------------------
def scores_case():
    def q(name, scores, n_top):
        a, b = _species(len(qs))
        rows = [(f"SC_{name}_{i}.1", a if i % 2 else b, _pid(98000 + 211 * i), 400 + i, s) for i, s in enumerate(scores)]
        qs.append(Query(f"sc_{name}", rows, {"top": list(range(n_top)), "n_top": n_top, "score": int(float(scores[0]))}))
    qs = []
    q("int32_max", ["2147483647", "2147483647", "2147483646", "5"], 2)
    q("int32_max_single", ["2147483647", "-2147483648"], 1)
    q("int32_min", ["-2147483648", "-2147483648"], 2)
    q("int32_min_single", ["-2147483648"], 1)
    q("negative", ["-5", "-5", "-7", "-6"], 2)
    q("negative_single", ["-5", "-2147483648"], 1)
    q("zero", ["0", "0", "-1", "-3"], 2)
    q("zero_single", ["0"], 1)
    q("truncated", ["700.9", "700", "699.9", "650"], 2)
    return _finish("scores", "all", qs)


# family: identity routes ------------------------------------------------------------------------------------------------------
def routes_case(variant):
    qs = []
    for q in range(300):
        a, b = _species(q)
        rows = [(f"R{q:03d}_{i}.1", a if i % 2 else b, _pid(90000 + (q * 17 + i * 3101) % 9999), 390 + i, "800" if i < 2 else "799") for i in range(4)]
        qs.append(Query(f"r{q:03d}", rows, {"top": [0, 1], "n_top": 2}))
    if variant == "four_decimals":                    # in the last query: the flag is raised by the last rows of the table
        r = qs[299].rows[1]; qs[299].rows[1] = (r[0], r[1], "98.1234", r[3], r[4])
    elif variant in ("at_limit", "below_limit"):      # on a top row in the middle of the table
        r = qs[150].rows[0]; qs[150].rows[0] = (r[0], r[1], "131.071" if variant == "at_limit" else "131.070", r[3], r[4])
    return _finish("routes", variant, qs, route="packed" if variant in ("exact", "below_limit") else "f64")


ROUTE_VARIANTS = ("exact", "four_decimals", "at_limit", "below_limit")


# family: ragged lineages ------------------------------------------------------------------------------------------------------
def _ragged_group(short_len, agree, phylum):
    """(short lineage, the four-level lineages) as paths"""
    other = 5 if phylum == 0 else 0
    if short_len == 2:
        short = (phylum,)
        longs = [(phylum if agree else other, c, o) for c in (0, 1) for o in (0, 1)]          # (they disagree at the phylum: the short row's last level)
    else:
        short = (phylum, 0)
        longs = [(phylum, 0 if agree else 1, o) for o in (0, 1)]                              # (at the class)
    return short, longs


def ragged_case():
    qs = []
    for phylum in (0, 5):                             # (5,) is the last entry of the taxonomies document
        for short_len in (2, 3):
            for pos in ("first", "middle", "last"):
                for tied in (True, False):
                    for agree in (True, False):
                        for n in (4, 65):
                            short, longs = _ragged_group(short_len, agree, phylum)
                            at = {"first": 0, "middle": n // 2, "last": n - 1}[pos]
                            name = f"rg_p{phylum}_{short_len}v4_{pos}_{'tied' if tied else 'untied'}_{'agree' if agree else 'differ'}_{n:02d}"
                            rows = []
                            for i in range(n):
                                path = short if i == at else longs[i % len(longs)]
                                pid = "98.500" if tied else (_pid(99900) if i == at else _pid(97000 + i * 41 % 2500))
                                rows.append((f"RG{len(qs):03d}_{(n - i):03d}.1", tid(*path), pid, 400 if tied else 380 + i % 9, "300"))
                            qs.append(Query(name, rows, {"top": list(range(n)), "n_top": n, "ragged": {
                                "short": short, "short_len": short_len, "at": at, "agree": agree, "tied": tied, "last_db_row": short == (5,)}}))
    return _finish("ragged", "all", qs)


# family: beans ----------------------------------------------------------------------------------------------------------------
def beans_case():
    qs = []
    sp = lambda s: tid(*BIG_GENUS, s)

    def q(name, rows, **claim):
        rows = [(a, t, p, l, "700") for a, t, p, l in rows]
        n = len(rows)
        rows.append((f"BN_{name}_low.1", sp(0), "99.999", 999, "699"))               # one row under the top score
        qs.append(Query(f"bn_{name}", rows, {"top": list(range(n)), "n_top": n, **claim}))
    for n in (65, 130):                               # one lineage: full agreement, the beans come at the last level
        q(f"one_lineage_{n}", [(f"ONE{n}_{i:03d}.1", sp(7), _pid(97000 + i * 53 % 2900), 400 + i % 5) for i in range(n)], beans=1)
    q("two_beans", [(f"TWO_{i}.1", sp(i % 2), _pid(98000 + 100 * i), 400) for i in range(5)], beans=2)
    q("three_beans", [(f"THREE_{i}.1", sp(10 + i % 3), _pid(98000 + 100 * i), 400) for i in range(7)], beans=3)
    q("forty_beans", [(f"FORTY_{i:02d}.1", sp(2 + i % 40), _pid(97500 + 17 * i), 400 + i % 3) for i in range(70)], beans=40)
    q("equal_occurrences", [(f"EQ_{i}.1", sp((5, 3, 4)[i % 3]), _pid(98000 + 50 * i), 400) for i in range(6)], beans=3)
    q("unequal_occurrences", [(f"UN_{i}.1", sp((3, 5, 5, 4, 4, 4)[i]), _pid(98000 + 50 * i), 400) for i in range(6)], beans=3)
    q("same_accession_neighbours", [("NB_A.1", sp(1), "98.500", 400), ("NB_B.1", sp(1), "99.000", 400), ("NB_A.1", sp(1), "98.500", 400),
                                    ("NB_A.1", sp(1), "98.500", 401)], beans=1, accessions=["NB_A.1", "NB_B.1"])
    q("same_accession_separated", [("SP_A.1", sp(1), "98.000", 400), ("SP_A.1", sp(1), "99.000", 400), ("SP_B.1", sp(1), "98.500", 400)],
      beans=1, accessions=["SP_A.1", "SP_B.1", "SP_A.1"])
    q("same_accession_rows_63_64", [(f"X{min(i, 63) if i <= 64 else i:03d}.1", sp(1), "98.500", 400) for i in range(70)], beans=1, n_accessions=69)
    q("same_accession_rows_63_64_apart", [(f"Y{min(i, 63) if i <= 64 else i:03d}.1", sp(1), "99.900" if i == 64 else "98.500", 400) for i in range(70)],
      beans=1, n_accessions=70)
    q("file_order_against_accession_order", [(f"REV_{9 - i}.1", sp(i % 2), "98.500", 400) for i in range(10)], beans=2)
    q("accession_prefix_of_another", [(a, sp(1), "98.500", 400) for a in ("ABC", "AB.1", "AB", "A", "AB0")], beans=1, accessions=["A", "AB", "AB.1", "AB0", "ABC"])
    q("accessions_equal_in_16_bytes", [(a, sp(1), "98.500", 400) for a in ("ABCDEFGHIJKLMNOP_2", "ABCDEFGHIJKLMNOPQ", "ABCDEFGHIJKLMNOP_1", "ABCDEFGHIJKLMNOP")],
      beans=1, accessions=["ABCDEFGHIJKLMNOP", "ABCDEFGHIJKLMNOPQ", "ABCDEFGHIJKLMNOP_1", "ABCDEFGHIJKLMNOP_2"])
    hi = ["é_2", "z_0", "Ä_1", "Z_1", "€_3", "ÿ"]
    q("accession_bytes_above_0x7f", [(a, sp(1), "98.500", 400) for a in hi], beans=1, accessions=sorted(hi, key=lambda s: s.encode()))
    return _finish("beans", "all", qs)


def beans_dup_case():
    """A taxid listed twice: every hit of that subject is two joined rows (mod.rs:72-76)"""
    qs = []

    def q(name, rows, joined_top):
        rows = [(a, t, p, l, "700") for a, t, p, l in rows]
        qs.append(Query(f"bd_{name}", rows, {"top": list(range(len(rows))), "n_top": len(rows), "joined_top": joined_top}))
    q("single_hit_twice", [("DUP_A.1", tid(*DUP_PLAIN), "99.500", 400)], 2)
    q("single_hit_two_lineages", [("DUP_B.1", tid(*DUP_CROSS), "99.500", 400)], 2)
    q("both", [("DUP_C.1", tid(*DUP_PLAIN), "99.100", 400), ("DUP_D.1", tid(*DUP_CROSS), "99.200", 401), ("DUP_E.1", tid(2, 0, 0, 0, 1, 1), "99.000", 400)], 5)
    q("65_lines_130_rows", [(f"DUP65_{i:02d}.1", tid(*DUP_PLAIN), _pid(98000 + 31 * i), 400 + i % 4) for i in range(65)], 130)
    q("two_lineages_across_row_64", [(f"DUP33_{i:02d}.1", tid(*DUP_CROSS), _pid(98000 + 31 * i), 400) for i in range(33)], 66)
    q("ragged_by_the_join", [("DUP_F.1", tid(*DUP_SHORT), "98.500", 400), ("DUP_G.1", tid(0, 0, 1), "98.500", 400)], 3)
    q("not_listed_twice", [("DUP_H.1", tid(3, 0, 0, 0, 0, 0), "99.100", 400), ("DUP_I.1", tid(3, 0, 0, 0, 0, 1), "99.100", 400)], 2)
    return _finish("beans", "taxid_listed_twice", qs, dup=True)


@functools.lru_cache(maxsize=None)
def cases():
    out = [sweeps_case()]
    out += [slots_case(nq, kind) for nq in SLOT_COUNTS for kind in NOT_RENDERED]
    out += [scores_case()]
    out += [routes_case(v) for v in ROUTE_VARIANTS]
    out += [ragged_case(), beans_case(), beans_dup_case()]
    return out


def case_params():
    """[(case, strategy)] with ids, for pytest.mark.parametrize"""
    return [(c, s) for c in cases() for s in c.strategies], [f"{c.id}-{s}" for c in cases() for s in c.strategies]


# ---- files and expected values, made once per process ------------------------------------------------------------------------
_written = {}
_expected = {}


def write(case, directory):
    """(table path, taxonomies path) of the case, written once"""
    key = case.id
    if key not in _written:
        tj = os.path.join(directory, f"tax{int(case.dup)}.blutils.json")
        if not os.path.exists(tj):
            with open(tj, "w", encoding="utf-8") as f:
                f.write(taxonomy_document(case.dup))
        bt = os.path.join(directory, f"{key}.tsv")
        with open(bt, "w", encoding="utf-8") as f:
            f.write(case.text())
        _written[key] = (bt, tj)
    return _written[key]


def expected(case, strategy, directory):
    """{query name: the oracle's result} of the files as written"""
    key = (case.id, strategy)
    if key not in _expected:
        bt, tj = write(case, directory)
        _expected[key] = oracle_from_files(bt, tj, False, "bacteria", strategy, None)
    return _expected[key]


def first_difference(got, want, path="taxon"):
    """The first field in which two JSON values differ, as (path, got, want); None when they are equal."""
    if isinstance(got, dict) and isinstance(want, dict):
        for k in want:
            if k not in got:
                return f"{path}.{k}", "<missing>", want[k]
            d = first_difference(got[k], want[k], f"{path}.{k}")
            if d:
                return d
        extra = [k for k in got if k not in want]
        return (f"{path}.{extra[0]}", got[extra[0]], "<missing>") if extra else None
    if isinstance(got, list) and isinstance(want, list):
        for i, (g, w) in enumerate(zip(got, want)):
            d = first_difference(g, w, f"{path}[{i}]")
            if d:
                return d
        return (f"{path}.length", len(got), len(want)) if len(got) != len(want) else None
    return None if got == want and isinstance(got, bool) == isinstance(want, bool) else (path, got, want)
