"""Independent restatement of the taxon abundance report (DESIGN.md §12, §1 of its issue) from a parsed document's
`results`, in plain dicts.  It does not import the product's report code: the product (blutils_amd/report.py on the host,
csrc/report_kernel.hip + pipeline.cpp, pipeline_render.cpp on the GPU path) is compared against this."""
import re

_FIELD = re.compile(r"size=([0-9]+)")
_SUFFIX = re.compile(r"_size_([0-9]+)\Z")


class WeightTooLarge(ValueError):
    pass


def weight(query, mode):
    if mode == "one":
        return 1
    value = None
    for field in query.split(";"):
        m = _FIELD.fullmatch(field)
        if m:
            value = m.group(1)
            break
    if value is None:
        m = _SUFFIX.search(query)
        value = m.group(1) if m else "1"
    if int(value) > 0xFFFFFFFF:
        raise WeightTooLarge(query)
    return int(value)


def report(results, mode="one"):
    unclassified = unplaced = 0
    direct = {}       # path (tuple of element texts) -> summed weight of the queries that end there
    for r in results:
        w = weight(r["query"], mode)
        taxon = r.get("taxon")
        if taxon is None:
            unclassified += w
        elif taxon.get("taxonomy") in (None, ""):
            unplaced += w
        else:
            p = tuple(taxon["taxonomy"].split(";"))
            direct[p] = direct.get(p, 0) + w
    total = unclassified + unplaced + sum(direct.values())
    clade = {}
    for p, w in direct.items():
        for k in range(1, len(p) + 1):
            clade[p[:k]] = clade.get(p[:k], 0) + w
    children = {}
    for p in clade:
        children.setdefault(p[:-1], []).append(p)

    def pct(c):
        return "%.2f" % (100.0 * c / total) if total else "0.00"

    lines = ["#percent\tclade\tdirect\trank\tidentifier\ttaxonomy",
             "\t".join((pct(unclassified), str(unclassified), str(unclassified), "-", "unclassified", ""))]
    if unplaced > 0:
        lines.append("\t".join((pct(unplaced), str(unplaced), str(unplaced), "-", "unplaced", "")))

    def visit(parent):
        kids = sorted(children.get(parent, []), key=lambda p: (-clade[p], p[-1].encode()))
        for p in kids:
            el = p[-1]
            cut = el.find("__")
            rank, ident = (el, "") if cut < 0 else (el[:cut], el[cut + 2:])
            lines.append("\t".join((pct(clade[p]), str(clade[p]), str(direct.get(p, 0)), rank, ident, ";".join(p))))
            visit(p)

    visit(())
    return "\n".join(lines) + "\n"
