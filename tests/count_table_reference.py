"""Independent restatement of DESIGN.md §22 (abundances from a count table): the parser, the join, the sample table and the
report, each from a parsed document's `results` plus the text of the count table file, in plain dicts.  It does not import
the product: the product (blutils_amd/report.py on the host; csrc/count_table.cpp, csrc/report_kernel.hip, pipeline.cpp and
pipeline_render.cpp on the GPU path) is compared against this."""
import re

_CELL = re.compile(r"([0-9]+)(?:\.0+)?")
LIMIT = 1 << 32


class ParseError(ValueError):
    def __init__(self, line, column, what):
        super().__init__(f"line {line}, column {column}: {what}")
        self.line, self.column = line, column


class JoinError(ValueError):
    def __init__(self, what, names):
        super().__init__(f"{what}: {names}")
        self.what, self.names = what, tuple(names)


def parse(text):
    """-> (sample names in the file's order, [(row name, [count per sample in the file's order])])"""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    samples, rows = None, []
    for number, raw in enumerate(lines, start=1):
        line = raw[:-1] if raw.endswith("\r") else raw
        if line == "":
            continue
        if samples is None and line[0] == "#" and "\t" not in line:
            continue
        cells = line.split("\t")
        if samples is None:
            if len(cells) == 1:
                raise ParseError(number, 2, "no sample")
            for k in range(1, len(cells)):
                if cells[k] == "":
                    raise ParseError(number, k + 1, "empty sample name")
                if cells[k] in cells[1:k]:
                    raise ParseError(number, k + 1, "sample named twice")
            samples = cells[1:]
            continue
        want = len(samples) + 1
        if len(cells) != want:
            # the first missing cell, or the first one too many
            raise ParseError(number, min(len(cells), want) + 1, "wrong number of cells")
        values = []
        for k in range(1, want):
            m = _CELL.fullmatch(cells[k])
            if not m or int(m.group(1)) >= LIMIT:
                raise ParseError(number, k + 1, "not a whole number below 2^32")
            values.append(int(m.group(1)))
        rows.append((cells[0], values))
    if samples is None:
        raise ParseError(len(lines) + 1, 1, "no header")
    return samples, rows


def key(name):
    return name.split(";")[0]


def join(samples, rows, queries):
    """-> ([{sample: count} per query], {sample: count} of the rows no query has, (n_rows, n_samples, n_joined, n_left))"""
    for name, values in rows:
        if sum(values) >= LIMIT:
            raise JoinError("row sum", [name])
    by_key = {}
    for name, values in rows:
        if key(name) in by_key:
            raise JoinError("rows", [by_key[key(name)][0], name])
        by_key[key(name)] = (name, values)
    first = {}
    for q in queries:
        if key(q) in first:
            raise JoinError("queries", [first[key(q)], q])
        first[key(q)] = q
        if key(q) not in by_key:
            raise JoinError("no row", [q])
    per_query = [dict(zip(samples, by_key[key(q)][1])) for q in queries]
    left = dict.fromkeys(samples, 0)
    n_left = 0
    for name, values in rows:
        if key(name) not in first:
            n_left += 1
            for s, v in zip(samples, values):
                left[s] += v
    return per_query, left, (len(rows), len(samples), len(rows) - n_left, n_left)


def _aggregate(results, text):
    samples, rows = parse(text)
    per_query, left, stats = join(samples, rows, [r["query"] for r in results])
    unclassified, unplaced = dict(left), dict.fromkeys(samples, 0)
    direct, cell, listed = {}, {}, set()
    for r, counts in zip(results, per_query):
        taxon = r.get("taxon")
        if taxon is None:
            for s in samples:
                unclassified[s] += counts[s]
        elif taxon.get("taxonomy") in (None, ""):
            for s in samples:
                unplaced[s] += counts[s]
        else:
            p = tuple(taxon["taxonomy"].split(";"))
            direct[p] = direct.get(p, 0) + sum(counts.values())
            for k in range(1, len(p) + 1):
                listed.add(p[:k])
                for s in samples:
                    cell[(p[:k], s)] = cell.get((p[:k], s), 0) + counts[s]
    clade = {p: sum(cell[(p, s)] for s in samples) for p in listed}
    return samples, unclassified, unplaced, direct, cell, clade, stats


def _rows_in_order(clade):
    children = {}
    for p in clade:
        children.setdefault(p[:-1], []).append(p)
    out = []

    def visit(parent):
        for p in sorted(children.get(parent, []), key=lambda p: (-clade[p], p[-1].encode())):
            el = p[-1]
            cut = el.find("__")
            out.append((p, el if cut < 0 else el[:cut], "" if cut < 0 else el[cut + 2:]))
            visit(p)

    visit(())
    return out


def _table(agg):
    samples, unclassified, unplaced, direct, cell, clade, _ = agg
    cols = sorted(samples, key=lambda c: c.encode())
    lines = ["\t".join(["#rank", "identifier", "taxonomy", "total"] + cols)]
    lines.append("\t".join(["-", "unclassified", "", str(sum(unclassified.values()))] + [str(unclassified[c]) for c in cols]))
    if sum(unplaced.values()) > 0:
        lines.append("\t".join(["-", "unplaced", "", str(sum(unplaced.values()))] + [str(unplaced[c]) for c in cols]))
    for p, rank, ident in _rows_in_order(clade):
        lines.append("\t".join([rank, ident, ";".join(p), str(clade[p])] + [str(cell[(p, c)]) for c in cols]))
    return "\n".join(lines) + "\n"


def _report(agg):
    _, unclassified, unplaced, direct, _, clade, _ = agg
    u, n = sum(unclassified.values()), sum(unplaced.values())
    total = u + n + sum(direct.values())

    def pct(x):
        return "%.2f" % (100.0 * x / total if total else 0.0)

    lines = ["#percent\tclade\tdirect\trank\tidentifier\ttaxonomy", f"{pct(u)}\t{u}\t{u}\t-\tunclassified\t"]
    if n > 0:
        lines.append(f"{pct(n)}\t{n}\t{n}\t-\tunplaced\t")
    for p, rank, ident in _rows_in_order(clade):
        lines.append(f"{pct(clade[p])}\t{clade[p]}\t{direct.get(p, 0)}\t{rank}\t{ident}\t{';'.join(p)}")
    return "\n".join(lines) + "\n"


def _stderr_line(stats):
    r, s, j, m = stats
    return f"count table: {r} rows, {s} samples, {j} joined to results, {m} without a result counted as unclassified"


def table(results, text):
    return _table(_aggregate(results, text))


def report(results, text):
    return _report(_aggregate(results, text))


def stats(results, text):
    return _aggregate(results, text)[6]


def stderr_line(results, text):
    return _stderr_line(stats(results, text))


def everything(results, text):
    """(table, report, stats, stderr line) from one pass over the results"""
    agg = _aggregate(results, text)
    return _table(agg), _report(agg), agg[6], _stderr_line(agg[6])
