"""The hit passes in composition: one table whose queries change their length class between two passes, and the
chain of copies that is its expected value.  No tests in this file; tests/test_pass_chain.py recomputes every claim below from
the bytes and the references, tests/test_gpu_pass_chain.py holds the library to the chain.

The expected value of a run with a set of options is the run without options on the last copy of

    hit_filter_reference.filter_text -> taxon_filter_reference.filter_text -> query_cover_reference.drop_lines
    -> subject_best_reference.rewrite_table -> score_band_reference.rewrite_table -> min_cover_reference.rewrite_table

an option that is off leaving its stage out.  The options are fixed: identity >= 90, the clade p__p7 excluded, query cover >= 50
(from `qcovhsp`), --top-bits 2, --min-cover 50.001 (the lowest value the library takes: a top group may lose almost half).

The table is kept as rows (thirteen reference columns with `0` in the six nobody reads, and a `qcovhsp` value) and written three
ways: `base` (the thirteen columns), `ext` (the thirteen and `qcovhsp`: what the parser stages of the chain read) and `perm`
(PERM_SPEC, a permuted `--blast-outfmt` with `qcovhsp`: what the library reads under a query cover).  `to_reference` of either
is `base`, so every chain ends in a copy in the reference's columns.

A designed query is written from seven counts (`designed`): a lines the parser takes (80.000 % identity, a taxon of p7, cover
40, and the highest score of the query: the top changes with the filter), b second, worse lines of a subject already present,
c majority-genus lines at the top T, d majority-genus lines at T - 2, e other-family lines at T, f other-family lines at T - 2,
g low lines.  With every option on its lengths are n0 = a + .. + g, n1 = n0 - a, n2 = n1 - b, the band takes the top group
from c + e to c + d + e + f, and the cover deletes the e + f outliers when c + d >= need(c + d + e + f).
"""
import os

import numpy as np

from tests import hit_filter_reference as hf
from tests import min_cover_reference as mc
from tests import outfmt_reference as R
from tests import query_cover_reference as Q
from tests import score_band_reference as band_ref
from tests import subject_best_reference as subj_ref
from tests import taxon_filter_reference as tf

HIT_FILTER = {"min_perc_identity": 90.0}
EXCLUDE = ["p__p7"]                                  # taxa 448 .. 511 of min_cover_reference.write_db
QUERY_COVER = {"percent": "50", "source": "qcovhsp"}
TOP_BITS = 2
MIN_COVER, MIN_COVER_MILLI = "50.001", 50001
EXT_SPEC = R.REFERENCE_SPEC + " qcovhsp"
PERM_SPEC = "6 bitscore qcovhsp evalue length staxid pident saccver qseqid"

PARSERS = {"none": (), "hit": ("hit",), "taxon": ("taxon",), "cover": ("cover",), "all": ("hit", "taxon", "cover")}
PASSES = ("subject", "band", "min_cover")
SUBSETS = [tuple(p for k, p in enumerate(PASSES) if m >> k & 1) for m in range(8)]
T = 1000                                             # the top score of a designed query once the parser's lines are gone
SHORT, STREAM = 64, 512                              # a wave's segment; the stream kernel's


def klass(n):
    return "S" if n <= SHORT else "M" if n <= STREAM else "L"


def _row(q, acc, taxid, pid, bs, qcov=100, aln=400):
    return (f"{q}\t{acc}\t{taxid}\t{pid}\t{aln}\t0\t0\t0\t0\t0\t0\t1e-50\t{bs}", qcov)


def _pid(j):
    return f"{97 + (j * 37) % 3000 // 1000}.{(j * 37) % 1000:03d}"


GENERA = list(range(16, 112))                        # phyla 1 .. 6: no bad, empty or excluded taxon among them


class Names:
    """`<sample>.<number>;<tag>`: the sample table reads s0 .. s2 out of the label, the tests find a query by its tag"""

    def __init__(self, first=0):
        self.n = first

    def __call__(self, tag):
        self.n += 1
        return f"s{self.n % 3}.{self.n};{tag}"


class Designed:
    """One designed query: its rows in file order and what it was MEANT to be (the tests recount from the bytes)."""

    def __init__(self, name, rows, **claim):
        self.name, self.rows, self.claim = name, rows, claim


def designed(name, k, a=0, b=0, c=0, d=0, e=0, f=0, g=0, one_subject=False, far=False, place=None, extra=(), kind="designed"):
    """k: picks the genus.  one_subject: every second line names the first kept subject (else they go round the kept ones).
    far: the other family lies in another phylum.  place="band": the T - 2 lines stand at rows 63, 64 and in the last sweep
    first; place="keep": the rows in the order they are made, `extra` last.  extra: rows appended as they are, [(accession, taxid, pid, score, qcov)]."""
    genus = GENERA[(k * 7) % len(GENERA)]
    fam = genus // 4
    other = ((fam - 4 + 8) % 24 + 4) if far else fam ^ 1
    tid = lambda t: mc.FIRST_TAXID + t
    label = name
    name = label.replace(";", "_")                    # (in the accessions)
    major = [(f"{name}_M{j}.1", tid(4 * genus + j % 4), _pid(j), T) for j in range(c)]
    band = [(f"{name}_B{j}.1", tid(4 * genus + (j + 1) % 4), _pid(j + 5), T - 2) for j in range(d)]
    out_top = [(f"{name}_O{j}.1", tid(16 * other + j % 16), _pid(j + 11), T) for j in range(e)]
    out_band = [(f"{name}_P{j}.1", tid(16 * other + (j + 3) % 16), _pid(j + 17), T - 2) for j in range(f)]
    low = [(f"{name}_L{j}.1", tid(64 + (j * 7 + k * 13) % 384), _pid(j + 23), T - 100 - j % 50) for j in range(g)]
    kept = [r + (100,) for r in major + band + out_top + out_band + low] + list(extra)
    if place == "band":
        n = len(kept)
        want = [p for p in (63, 64, n - 1, n - 2) if 0 <= p < n]
        prio = list(dict.fromkeys(want + list(range(n))))
        slots = [None] * n
        ordered = [r + (100,) for r in band + out_band + major + out_top + low]
        for p, r in zip(prio, ordered):
            slots[p] = r
        kept = slots
    filt = [(f"{name}_F{j}.1", tid(448 + (j + k) % 64), "80.000", T + 5, 40) for j in range(a)]
    second = []
    for j in range(b):
        acc, taxid, pid, _, _ = kept[0 if one_subject else j % len(kept)]
        second.append((acc, taxid, _pid(j + 29), 100 + j % 50, 100))
    rows = kept + filt + second
    if place is None:
        rng = np.random.default_rng(1000 + k)
        rows = [rows[i] for i in rng.permutation(len(rows))]
    n_top = c + d + e + f
    drops = e + f if (e + f and n_top > 1 and c + d >= mc.need_rows(n_top, MIN_COVER_MILLI)) else 0
    n0 = len(rows)
    claim = dict(kind=kind, n=(n0, n0 - a, n0 - a - b, n0 - a - b - drops), top=(c + e, n_top)) if not extra else dict(kind=kind)
    return Designed(label, [_row(label, acc, taxid, pid, bs, qcov, aln=300 + i % 200) for i, (acc, taxid, pid, bs, qcov) in enumerate(rows)], **claim)


def short(name, k):
    """a neighbour: three lines of one genus, which no option touches"""
    return designed(name, k, c=2, g=1, kind="short")


ERASED_BY = {"all": ("80.000", 448, 40), "hit": ("80.000", 64, 100), "taxon": ("99.000", 448, 100), "cover": ("99.000", 64, 40)}


def erased(name, k, by="all", n=3):
    """a query all of whose lines the parser takes: under every parser option (all), or under one of them alone"""
    pid, t0, qcov = ERASED_BY[by]
    rows = [_row(name, f"{name.replace(';', '_')}_E{j}.1", mc.FIRST_TAXID + t0 + (j + k) % 64, pid, 700 - j % 3, qcov) for j in range(n)]
    return Designed(name, rows, kind="erased_" + by)


# ---- the table ------------------------------------------------------------------------------------------------------------------
PAIRS = [(65, 64), (65, 65), (64, 63), (129, 65), (513, 512), (513, 513), (600, 64)]       # before -> after of one compacting step
# (the cover keeps more than half of a top group, so 600 -> 64 does not exist for it: 600 -> 301 is the most it takes, need(600))
COVER_PAIRS = PAIRS[:-1] + [(600, 301)]
BAND_TOPS = [(1, 64), (1, 65), (63, 65), (1, None)]                                       # T before -> after; None: the whole segment
BAND_SEGMENTS = (65, 129, 513)
SEAM_TABLE = {"t65_parser": (65, 64, 64, 64), "t513_subject": (513, 513, 512, 512), "t65_cover": (65, 65, 65, 64),
               "t127_need": (127, 127, 127, 64), "t600_cascade": (600, 513, 512, 401), "t1000_cover": (1000, 1000, 1000, 512)}


def _cover_counts(before, after):
    """c, d, e, f, g of a query the cover takes from `before` to `after` rows"""
    drop = before - after
    if drop == 0:                                     # a top group one row short of its need: left as it is
        half = (before - 5) // 2
        return dict(c=half, e=half, g=before - 2 * half, far=True)
    top_major = min(after, max(drop + 10, after // 2))               # the top group: the outliers and enough of the genus
    assert top_major >= mc.need_rows(top_major + drop, MIN_COVER_MILLI) and top_major <= after
    return dict(c=top_major - top_major // 2, d=top_major // 2, e=drop - drop // 2, f=drop // 2, g=after - top_major)


def designed_queries(names):
    """[Designed] of the head of the table; the neighbours are added by `main_table`"""
    out, k = [], 0

    def add(tag, **kw):
        nonlocal k
        k += 1
        out.append(designed(names(tag), k, **kw))

    for before, after in PAIRS:
        add(f"parser_{before}_{after}", a=before - after, c=min(after, 40), g=after - min(after, 40))
    for before, after in PAIRS + [(513, 64)]:
        add(f"subject_{before}_{after}", b=before - after, c=min(after, 40), g=after - min(after, 40), one_subject=(before, after) == (513, 64))
    for before, after in COVER_PAIRS:
        add(f"cover_{before}_{after}", **_cover_counts(before, after))
    for n in BAND_SEGMENTS:
        for t0, t1 in BAND_TOPS:
            t1 = n if t1 is None else t1
            add(f"band_{n}_{t0}_{t1}", c=t0, d=t1 - t0, g=n - t1, place="band")
    add("t65_parser", a=1, c=30, d=4, g=30)
    add("t513_subject", b=1, c=300, d=100, g=112)
    add("t65_cover", c=40, d=24, e=1)
    add("t127_need", c=30, d=34, e=33, f=30)
    add("t600_cascade", a=87, b=1, c=200, d=100, e=60, f=51, g=101)
    add("t1000_cover", c=256, d=256, e=244, f=244, far=True)
    add("cascade_300", a=100, b=70, c=40, d=30, e=20, f=40)                 # 300 -> 200 -> 130 -> 70
    add("cascade_90", a=10, b=10, c=30, d=34, e=3, f=3)                     # 90 -> 80 -> 70 -> 64
    add("cascade_1100", a=500, b=500, c=30, d=30, e=20, f=20)                # 1100 -> 600 -> 100 -> 60: L, L, M, S
    add("long_throughout", a=500, b=300, c=300, d=300, e=250, f=250, g=100)  # 2000 -> 1500 -> 1200 -> 700
    # rows without a usable lineage, in a top group only because the band raised them: the cover leaves the query alone
    for tag, taxid in (("lacking", mc.LACKING_TAXID), ("bad", mc.BAD_TAXID), ("empty", mc.EMPTY_TAXID)):
        for size in (0, 60):
            add(f"unusable_{tag}_{size}", c=6 + size, e=2, g=3, extra=[(f"U_{tag}{size}.1", taxid, "99.000", T - 2, 100)], kind="unusable")
    # a subject's worse line inside the band and first in the file, of another family: the band before the subject pass would tie
    # the two and keep this one
    for size in (0, 70):
        add(f"second_in_band_{size}", c=4 + size, g=2, place="keep", kind="second_in_band",
            extra=[(f"SB{size}.1", mc.FIRST_TAXID + 440, "99.900", T - 2, 100), (f"SB{size}.1", mc.FIRST_TAXID + 441, "97.500", T, 100)])
    # two lines of one subject on the top score: without any other option the subject pass takes one occurrence from the consensus
    for size in (0, 70):
        add(f"tied_pair_{size}", c=3 + size, g=2, place="keep", kind="tied_pair",
            extra=[(f"TP{size}.1", mc.FIRST_TAXID + 300, "98.000", T, 100), (f"TP{size}.1", mc.FIRST_TAXID + 300, "97.000", T, 100)])
    # an unmatched row that is the best line of its subject, and one that is the worse
    for size in (0, 70):
        add(f"unmatched_best_{size}", c=5 + size, g=2, kind="unmatched", extra=[(f"UB{size}.1", mc.LACKING_TAXID + 1, "99.000", T - 50, 100),
                                                                             (f"UB{size}.1", mc.FIRST_TAXID + 70, "98.000", T - 60, 100)])
        add(f"unmatched_worse_{size}", c=5 + size, g=2, kind="unmatched", extra=[(f"UW{size}.1", mc.FIRST_TAXID + 70, "99.000", T - 50, 100),
                                                                              (f"UW{size}.1", mc.LACKING_TAXID + 2, "98.000", T - 60, 100)])
    return out


class Table:
    def __init__(self, name, queries, headers=None):
        self.name, self.queries = name, queries
        self.headers = sorted({q.name for q in queries}) + ["s1.999999;no_hit_at_all"] if headers is None else headers

    def rows(self, order):
        rows = [r for q in self.queries for r in q.rows]
        return rows if order == "grouped" else hf.scramble(rows, np.random.default_rng(77))


def _fillers(n_q, seed, names):
    """min_cover_reference.make_rows as queries: the six unread columns zeroed, cover 90, named by `names`"""
    rows = mc.make_rows(n_q, np.random.default_rng(seed), sample_names=True)
    by, new = {}, {}
    for r in rows:
        f = r.split("\t")
        if f[0] not in new:
            new[f[0]] = names("f")
        f[0] = new[f[0]]
        f[5:11] = ["0"] * 6
        by.setdefault(f[0], []).append(("\t".join(f), 90))
    return [Designed(name, rs, kind="filler") for name, rs in by.items()]


def main_table(n_fillers=1150):
    """Head: four queries every parser option erases, then groups of four [short, long, short, short], once [short, long, long,
    short] — every parser setting erases none or four of the queries in front of a group, so a long query keeps its place in
    its wave.  Then the fillers with single erased queries, one per parser option and one for all, among them and a run of 72
    erased queries; last a short, a long and a 70-row erased query: the table ends in a long query under every setting."""
    qs, k, names = [], 0, Names()

    def nb():
        nonlocal k
        k += 1
        return short(names("n"), k)

    qs += [erased(names(f"first{j}"), j) for j in range(4)]
    longs = designed_queries(names)
    pair = [q for q in longs if q.name.endswith(("t600_cascade", "t1000_cover"))]
    for q in longs:
        if q in pair:
            continue
        qs += [nb(), q, nb(), nb()]
    qs += [nb(), pair[0], pair[1], nb()]
    fill = _fillers(n_fillers, 311, names)
    singles = {100: "all", 200: "hit", 300: "taxon", 400: "cover", 500: "all"}
    for i, q in enumerate(fill):
        if i in singles:
            qs.append(erased(names(f"gone_{singles[i]}"), i, singles[i], n=2 + i // 100))
        if i == 700:
            qs += [erased(names(f"run{j:02d}"), j, n=1 + j % 4) for j in range(72)]
        qs.append(q)
    k += 1
    qs += [nb(), designed(names("last_long"), k, a=3, b=4, c=40, d=30, e=10, f=12, g=20), erased(names("last_erased"), 9, n=70)]
    return Table("main", qs)


def erased_table():
    """every line goes with any parser option"""
    names = Names()
    qs = [erased(names(f"e{j:02d}"), j, n=1 + j % 5) for j in range(40)] + [erased(names("e_long"), 3, n=70)]
    return Table("erased", qs)


IDENTITY_VALUES = {"four_decimals": "98.1234", "at_limit": "131.071"}
IDENTITY_VARIANTS = ("subject", "min_cover", "kept")


def identity_table(value, variant):
    """300 fillers and one query with one row whose identity leaves the packed records: the worse line of a subject (deleted by
    the subject pass), an outlier of the top group (deleted by the cover), or a row of the majority genus (kept)."""
    pid = IDENTITY_VALUES[value]
    if variant == "subject":
        extra = [("ID_S.1", mc.FIRST_TAXID + 80, "99.000", T, 100), ("ID_S.1", mc.FIRST_TAXID + 80, pid, T - 30, 100)]
    elif variant == "min_cover":
        extra = [("ID_C.1", mc.FIRST_TAXID + 64, pid, T, 100)]
    else:
        extra = [("ID_K.1", mc.FIRST_TAXID + 80, pid, T, 100)]
    names = Names()
    name = names("identity")
    q = Designed(name, [_row(name, f"ID_M{j}.1", mc.FIRST_TAXID + 80 + j % 4, _pid(j), T if j < 8 else T - 40) for j in range(12)] +
                 [_row(name, *r) for r in extra], kind="identity")
    fill = _fillers(300, 412, names)
    return Table(f"identity_{value}_{variant}", fill[:150] + [q] + fill[150:])


# ---- files and chains, made once per process --------------------------------------------------------------------------------------
_files, _chains = {}, {}


def write(directory, table, order="grouped"):
    """-> {base, ext, perm, db}: paths"""
    key = (directory, table.name, order)
    if key not in _files:
        rows = table.rows(order)
        base = "".join(r + "\n" for r, _ in rows).encode()
        ext = "".join(f"{r}\t{c}\n" for r, c in rows).encode()
        perm = R.relayout(base, PERM_SPEC, {"qcovhsp": lambda i: b"%d" % rows[i][1]})
        paths = {}
        for tag, blob in (("base", base), ("ext", ext), ("perm", perm)):
            paths[tag] = os.path.join(directory, f"{table.name}_{order}_{tag}.tsv")
            open(paths[tag], "wb").write(blob)
        paths["db"] = os.path.join(directory, "taxonomies.json")
        if not os.path.exists(paths["db"]):
            mc.write_db(paths["db"])
        _files[key] = paths
    return _files[key]


class Stage:
    def __init__(self, step, path, n_in, n_out, counts):
        self.step, self.path, self.n_in, self.n_out, self.counts = step, path, n_in, n_out, counts


def n_lines(path):
    return sum(1 for ln in open(path, "rb").read().split(b"\n") if ln.strip(b"\r"))


def chain(directory, table, order, parser, passes):
    """[Stage]: the table as `ext`, then one stage per option that is on ("hit", "taxon", "cover" on the fourteen columns, "columns"
    — the copy in the reference's thirteen — then "subject", "band", "min_cover").  The last stage's path is the expected table."""
    key = (directory, table.name, order, parser, tuple(passes))
    if key in _chains:
        return _chains[key]
    files = write(directory, table, order)
    if passes:
        stages = list(chain(directory, table, order, parser, passes[:-1]))
        src, step = stages[-1].path, passes[-1]
        dst = os.path.join(directory, f"{table.name}_{order}_{parser}_{'-'.join(passes)}.tsv")
        if step == "subject":
            n_in, n_out, n_thinned, n_q = subj_ref.rewrite_table(src, dst)
            counts = {"n_hits": n_in, "n_kept": n_out, "n_queries": n_q, "n_thinned": n_thinned}
        elif step == "band":
            n_in, n_raised, n_widened, n_q = band_ref.rewrite_table(src, dst, D=TOP_BITS)
            n_out, counts = n_in, {"n_hits": n_in, "n_raised": n_raised, "n_queries": n_q, "n_widened": n_widened}
        else:
            counts = mc.rewrite_table(src, dst, files["db"], False, MIN_COVER_MILLI)
            n_in, n_out = counts["n_hits"], counts["n_kept"]
        stages.append(Stage(step, dst, n_in, n_out, counts))
    else:
        stages = [Stage("table", files["ext"], None, n_lines(files["ext"]), {})]
        for step in PARSERS[parser]:
            src, dst = stages[-1].path, os.path.join(directory, f"{table.name}_{order}_{parser}_ext_{step}.tsv")
            if step == "hit":
                n_in, n_out = hf.filter_text(src, dst, HIT_FILTER)
                counts = {"n_lines": n_in, "n_kept": n_out}
            elif step == "taxon":
                counts = tf.filter_text(src, dst, files["db"], exclude=EXCLUDE)
                n_in, n_out = counts["n_lines"], counts["n_kept"]
            else:
                blob = open(src, "rb").read()
                copy, n_below = Q.drop_lines(blob, EXT_SPEC, QUERY_COVER)
                open(dst, "wb").write(copy)
                n_in = n_lines(src)
                n_out, counts = n_in - n_below, {"n_lines": n_in, "n_below": n_below}
            stages.append(Stage(step, dst, n_in, n_out, counts))
        dst = os.path.join(directory, f"{table.name}_{order}_{parser}_columns.tsv")
        open(dst, "wb").write(R.to_reference(open(stages[-1].path, "rb").read(), EXT_SPEC))
        stages.append(Stage("columns", dst, stages[-1].n_out, stages[-1].n_out, {}))
    _chains[key] = stages
    return stages


def whole_table_counts(directory, table, order):
    """what the parser counts over every line of the table, whatever else is on: the taxon filter's verdicts and the lines below
    the cover"""
    key = (directory, table.name, order, "whole")
    if key not in _chains:
        files = write(directory, table, order)
        taxa = tf.filter_text(files["ext"], os.path.join(directory, "scratch.tsv"), files["db"], exclude=EXCLUDE)
        _, n_below = Q.drop_lines(open(files["ext"], "rb").read(), EXT_SPEC, QUERY_COVER)
        _chains[key] = {"n_lines": taxa["n_lines"], "n_excluded": taxa["n_excluded"], "excluded_by": taxa["excluded_by"], "n_below": n_below}
    return _chains[key]


def by_query(path):
    """{query: [fields of its lines, in file order]}, the queries in the order of their first line"""
    out = {}
    for ln in open(path, "rb").read().split(b"\n"):
        ln = ln.rstrip(b"\r")
        if ln:
            f = ln.split(b"\t")
            out.setdefault(f[0].decode(), []).append(f)
    return out


def top_size(lines):
    scores = [band_ref.truncated(f[12]) for f in lines]
    return scores.count(max(scores))


def options(parser, passes):
    """the keywords of the run: (those of the call, whether the table is read as `perm`)"""
    kw = {}
    if "hit" in PARSERS[parser]:
        kw["hit_filter"] = HIT_FILTER
    if "taxon" in PARSERS[parser]:
        kw["taxon_filter"] = {"exclude": EXCLUDE}
    if "cover" in PARSERS[parser]:
        kw["query_cover"], kw["blast_outfmt"] = QUERY_COVER, PERM_SPEC
    if "subject" in passes:
        kw["best_hit_per_subject"] = True
    if "band" in passes:
        kw["score_band"] = {"top_bits": TOP_BITS}
    if "min_cover" in passes:
        kw["min_cover"] = MIN_COVER
    return kw
