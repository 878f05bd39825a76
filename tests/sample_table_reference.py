"""Independent restatement of the per-sample table (DESIGN.md §13, §1 of its issue) from a parsed document's `results`, in
plain dicts.  It does not import the product: the product (blutils_amd/report.py on the host, csrc/report_kernel.hip +
pipeline.cpp, pipeline_render.cpp on the GPU path) is compared against this."""
import re

_SAMPLE = re.compile(r"sample=(.+)", re.S)
_SIZE_TAIL = re.compile(r"_size_[0-9]+\Z")
_LABEL = re.compile(r"(.+)\.([0-9]+)\Z", re.S)
_FIELD = re.compile(r"size=([0-9]+)")
_SUFFIX = re.compile(r"_size_([0-9]+)\Z")


class NoSample(ValueError):
    pass


def sample(query):
    for field in query.split(";"):
        m = _SAMPLE.fullmatch(field)
        if m:
            return m.group(1)
    label = _SIZE_TAIL.sub("", query.split(";")[0], count=1)
    m = _LABEL.fullmatch(label)      # greedy: the left part runs to the last '.' followed by digits only
    if m and re.fullmatch(r"[0-9]+", m.group(2)) and "." not in m.group(2):
        return m.group(1)
    raise NoSample(query)


def weight(query, mode):
    if mode == "one":
        return 1
    for field in query.split(";"):
        m = _FIELD.fullmatch(field)
        if m:
            return int(m.group(1))
    m = _SUFFIX.search(query)
    return int(m.group(1)) if m else 1


def table(results, mode="one"):
    cols = set()
    unclassified, unplaced = {}, {}
    direct, cell = {}, {}          # path -> weight ending there; (path, sample) -> clade
    for r in results:
        s = sample(r["query"])
        w = weight(r["query"], mode)
        cols.add(s)
        taxon = r.get("taxon")
        if taxon is None:
            unclassified[s] = unclassified.get(s, 0) + w
        elif taxon.get("taxonomy") in (None, ""):
            unplaced[s] = unplaced.get(s, 0) + w
        else:
            p = tuple(taxon["taxonomy"].split(";"))
            direct[p] = direct.get(p, 0) + w
            for k in range(1, len(p) + 1):
                cell[(p[:k], s)] = cell.get((p[:k], s), 0) + w
    cols = sorted(cols, key=lambda c: c.encode())
    clade = {}
    for p, w in direct.items():
        for k in range(1, len(p) + 1):
            clade[p[:k]] = clade.get(p[:k], 0) + w
    children = {}
    for p in clade:
        children.setdefault(p[:-1], []).append(p)
    lines = ["\t".join(["#rank", "identifier", "taxonomy", "total"] + cols)]

    def fixed(what, per):
        return "\t".join(["-", what, "", str(sum(per.values()))] + [str(per.get(c, 0)) for c in cols])

    lines.append(fixed("unclassified", unclassified))
    if sum(unplaced.values()) > 0:
        lines.append(fixed("unplaced", unplaced))

    def visit(parent):
        for p in sorted(children.get(parent, []), key=lambda p: (-clade[p], p[-1].encode())):
            el = p[-1]
            cut = el.find("__")
            rank, ident = (el, "") if cut < 0 else (el[:cut], el[cut + 2:])
            lines.append("\t".join([rank, ident, ";".join(p), str(clade[p])] + [str(cell.get((p, c), 0)) for c in cols]))
            visit(p)

    visit(())
    return "\n".join(lines) + "\n"
