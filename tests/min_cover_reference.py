"""Independent statement of the minimum cover (include/blu_consensus.h: blu_hits_cover_keep) in plain Python, with
no median and no range minimum: every prefix tuple of every top row is counted in a dict.  Test infrastructure in the manner of
tests/subject_best_reference.py: shares no code with the product.  Lineages and their rank normalisation are read as
tests/taxon_filter_reference.py reads them.

The rule under test: a run with --min-cover gives what the run with the same options before it gives on `rewrite_table`'s copy
of the table, from which the top lines outside the covering prefix were deleted.
"""
import json

from tests import taxon_filter_reference as tfr

MILLI_ONE = 100000          # 100 % in thousandths of a percent
LOW, HIGH = 50001, 100000   # min_cover_milli
NONE_U8 = 0xFF              # the depth of a query left alone


def need_rows(n: int, milli: int) -> int:
    """the smallest integer with need * 100000 >= n * milli (Python integers: no overflow, no rounding)"""
    assert LOW <= milli <= HIGH
    return -((-n * milli) // MILLI_ONE)


def covering_prefix(lineages, need):
    """the longest tuple that at least `need` of the lineages (tuples of nodes) start with"""
    count = {}
    for lin in lineages:
        for d in range(len(lin) + 1):
            count[tuple(lin[:d])] = count.get(tuple(lin[:d]), 0) + 1
    good = [p for p, c in count.items() if c >= need]
    best = max(good, key=len)
    assert [p for p in good if len(p) == len(best)] == [best]          # need > n / 2: nested, so the longest is unique
    return best


def decide(top_lineages, milli):
    """One top group: lineages as tuples of nodes, None for a row without a usable one (unmatched, bad, corrupt) and () for an
    empty one.  -> (one bool per row, d* or NONE_U8, 'alone' | 'unresolved' | 'decided')."""
    n = len(top_lineages)
    if n <= 1:
        return [True] * n, NONE_U8, "alone"
    if any(lin is None or len(lin) == 0 for lin in top_lineages):
        return [True] * n, NONE_U8, "unresolved"
    c = covering_prefix(top_lineages, need_rows(n, milli))
    return [tuple(lin[:len(c)]) == c for lin in top_lineages], len(c), "decided"


def keep(seg_off, bitscore, lineages, milli):
    """-> (one 0 / 1 verdict per row, d* per query, the counts).  lineages: one per ROW, as `decide` takes them.  Segments as the
    library reads them: an offset beyond the columns is clamped to their length and a decreasing pair is an empty segment; a row
    that no segment names gets 0."""
    n = len(bitscore)
    out, depth = [0] * n, []
    n_narrowed = n_unresolved = 0
    for q in range(len(seg_off) - 1):
        s1 = min(int(seg_off[q + 1]), n)
        s0 = min(int(seg_off[q]), s1)
        if s0 == s1:
            depth.append(NONE_U8)
            continue
        t = max(int(bitscore[i]) for i in range(s0, s1))
        top = [i for i in range(s0, s1) if int(bitscore[i]) == t]
        verdict, d, what = decide([lineages[i] for i in top], milli)
        for i in range(s0, s1):
            out[i] = 1
        for i, v in zip(top, verdict):
            out[i] = 1 if v else 0
        depth.append(d)
        n_narrowed += 0 if all(verdict) else 1
        n_unresolved += 1 if what == "unresolved" else 0
    counts = {"n_hits": n, "n_kept": sum(out), "n_queries": len(seg_off) - 1, "n_narrowed": n_narrowed, "n_unresolved": n_unresolved}
    return out, depth, counts


def truncated(field) -> int:
    """column 12 as the parsers type it: the f64 value truncated toward zero (mod.rs:184)"""
    return int(float(field.decode() if isinstance(field, bytes) else field))


def rewrite_table(src, dst, db_json, use_taxid, milli):
    """Copies the lines of `src` to `dst`, leaving out the top lines of a query that do not start with its covering prefix;
    everything else, empty lines and line ends included, verbatim.  A query is every line with the same first column, wherever
    it stands in the file; a line's lineage is that of the first listing of its column 3 in `db_json`.  Returns the counts
    blu_min_cover_stats gives."""
    tax = tfr.Taxonomy(db_json, use_taxid)
    data = open(src, "rb").read()
    lines, pos = [], 0                       # (raw line, fields or None for an empty line)
    while pos < len(data):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl + 1
        raw = data[pos:end]
        pos = end
        body = raw[:-1] if raw.endswith(b"\n") else raw
        if body.endswith(b"\r"):
            body = body[:-1]
        lines.append((raw, body.split(b"\t") if body else None))
    by_query = {}
    for k, (_, f) in enumerate(lines):
        if f is not None:
            by_query.setdefault(f[0], []).append(k)
    dropped, n_narrowed, n_unresolved = set(), 0, 0
    for ks in by_query.values():
        t = max(truncated(lines[k][1][12]) for k in ks)
        top = [k for k in ks if truncated(lines[k][1][12]) == t]
        lins = []
        for k in top:
            els = tax.elements.get(int(lines[k][1][2]))
            lins.append(None if els is None else tuple(els))           # (a bad lineage reads as no elements: () — unresolved too)
        verdict, _, what = decide(lins, milli)
        dropped.update(k for k, v in zip(top, verdict) if not v)
        n_narrowed += 0 if all(verdict) else 1
        n_unresolved += 1 if what == "unresolved" else 0
    n_in = sum(1 for _, f in lines if f is not None)
    open(dst, "wb").write(b"".join(raw for k, (raw, _) in enumerate(lines) if k not in dropped))
    return {"n_hits": n_in, "n_kept": n_in - len(dropped), "n_queries": len(by_query), "n_narrowed": n_narrowed, "n_unresolved": n_unresolved}


# ---- a database with five ranks, and tables whose top groups hold a majority genus and outliers of another family --------------
FIRST_TAXID, N_TAXIDS = 100, 512
BAD_TAXID, EMPTY_TAXID, LACKING_TAXID = 100 + 37, 100 + 58, 9000


def lineage_of(t, numeric=False):
    """taxon t = 0 .. N_TAXIDS - 1: four species a genus, four genera a family, four families a phylum"""
    if numeric:
        return f"d__2;p__{1000 + t // 64};f__{2000 + t // 16};g__{3000 + t // 4};s__{FIRST_TAXID + t}"
    return f"d__b;p__p{t // 64};f__f{t // 16};g__g{t // 4};s__s{t}"


def write_db(path):
    tx = []
    for t in range(N_TAXIDS):
        taxid = FIRST_TAXID + t
        text, numeric = lineage_of(t), lineage_of(t, True)
        if taxid == BAD_TAXID:                                          # one element of three parts: the whole lineage is refused
            text, numeric = "d__b;p__x__y;s__lost", "d__2;p__1__2;s__0"
        if taxid == EMPTY_TAXID:
            text = numeric = ""
        tx.append({"taxid": taxid, "rank": "species", "numericLineage": numeric, "textLineage": text, "accessions": []})
    open(path, "w").write(json.dumps({"blutilsVersion": "x", "sourceDatabase": "y", "taxonomies": tx}))
    return str(path)


def _usable(t):
    return FIRST_TAXID + t not in (BAD_TAXID, EMPTY_TAXID)


def make_rows(n_q, rng, sample_names=False, lacking=True):
    """BLAST-shaped lines.  A query's top group: 2 .. 9 lines of one genus (its four species, several accessions each) and 0, 1
    or 2 lines of another family — of the same phylum or of another — so that under 80 % some groups keep the genus with the
    outliers dropped, some stand exactly at `need`, and some fall back to the family's or the domain's level and lose nothing;
    a third of the top scores carry a decimal.  Under the top: 0 .. 4 lines of anything.  Every eighth query (lacking) has a
    top line whose taxid the database lacks, or whose lineage is bad or empty (lacking=False: no line of the table is such a
    one).  The lines of a query are shuffled."""
    rows = []
    for q in range(n_q):
        name = f"s{q % 3}.{q}" if sample_names else f"q{q:06d}"
        top = int(rng.integers(200, 3000))
        genus = int(rng.integers(0, N_TAXIDS // 4))
        major = [4 * genus + int(rng.integers(0, 4)) for _ in range(int(rng.integers(2, 10)))]
        major = [t for t in major if _usable(t)] or [4 * genus + 3]
        other_family = (genus // 4 + int(rng.integers(1, N_TAXIDS // 16))) % (N_TAXIDS // 16)
        if rng.random() < 0.5:                                          # the same phylum, another family
            other_family = genus // 16 * 4 + (genus // 4 + int(rng.integers(1, 4))) % 4
        out = [16 * other_family + int(rng.integers(0, 16)) for _ in range(int(rng.choice([0, 1, 1, 2])))]
        out = [t for t in out if _usable(t)]
        mine = [(t, top) for t in major + out]
        if lacking and q % 8 == 5:
            mine.append(((LACKING_TAXID + q, BAD_TAXID, EMPTY_TAXID)[q // 8 % 3] - FIRST_TAXID, top))
        for _ in range(int(rng.integers(0, 5))):
            t = int(rng.integers(0, N_TAXIDS))
            mine.append((t if lacking or _usable(t) else t + 1, top - int(rng.integers(1, 150))))
        lines = []
        for j, (t, b) in enumerate(mine):
            text = f"{b}.{int(rng.integers(0, 10))}" if rng.random() < 0.33 else str(b)
            lines.append(f"{name}\tNR_{t:06d}_{j}.1\t{FIRST_TAXID + t}\t{97 + int(rng.integers(0, 3001)) / 1000:.3f}\t{int(rng.integers(300, 500))}"
                         f"\t1\t0\t1\t400\t1\t400\t1e-{int(rng.integers(50, 150))}\t{text}")
        rows += [lines[i] for i in rng.permutation(len(lines))]
    return rows
