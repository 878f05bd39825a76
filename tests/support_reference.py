"""Restatement of the per-query assignment support (include/blu_consensus.h: blu_support) in plain Python:
lineages are walked node by node, in no particular order of the taxonomy rows, so nothing here shares the device pass's
method (one range of sorted positions per query).  Also the renderer of the `--support-table` text.

A hit is MATCHED when its desc row names a taxonomy row whose lineage parsed: not unmatched (-1 / 0xFFFFFFFF), not flagged
`bad`, not empty (an empty lineage string fails parse_taxonomy too).  The ASSIGNED CLADE of a record with status < 2: with
L the highest bit of level_mask, every row whose lineage has more than L levels and whose first L + 1 nodes equal the
first L + 1 nodes of the lineage of the record's reference row; level_mask == 0: every row.  A hit SUPPORTS the
assignment when it is matched and its row is in the clade."""
import numpy as np

SUPPORT_FIELDS = ("n_hits", "n_matched", "n_top", "n_top_support", "n_support", "top_score", "bits", "support_bits")
DTYPE = np.dtype([(f, "<i8") for f in SUPPORT_FIELDS])          # wide on purpose: nothing can wrap here
UNMATCHED = 0xFFFFFFFF
HEADER = "#query\trank\tidentifier\thits\tmatched\ttop_hits\ttop_support\tsupport\tbit_score\tbits\tsupport_bits\tconfidence\n"


def _desc(row):
    row = int(row)
    return -1 if row < 0 or row == UNMATCHED else row


def supporting(seg_off, bitscore, desc_row, lineages, bad, records):
    """(matched, supports): one bool per hit."""
    n = len(bitscore)
    matched, sup = np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        t = _desc(desc_row[i])
        matched[i] = t >= 0 and t < len(lineages) and not (bad is not None and bad[t]) and len(lineages[t]) > 0
    for q in range(len(seg_off) - 1):
        r = records[q]
        if int(r["status"]) >= 2:
            continue
        ref = lineages[_desc(desc_row[int(r["ref_row"])])]
        mask = int(r["level_mask"])
        if mask == 0:
            prefix = []
        else:
            L = mask.bit_length() - 1
            if len(ref) <= L:
                continue                                        # (no row has the reference row's first L + 1 nodes: it has fewer)
            prefix = [int(x) for x in ref[:L + 1]]
        for i in range(int(seg_off[q]), int(seg_off[q + 1])):
            if not matched[i]:
                continue
            lin = lineages[_desc(desc_row[i])]
            ok = len(lin) >= len(prefix)
            for j in range(len(prefix)):
                if not ok:
                    break
                ok = int(lin[j]) == prefix[j]
            sup[i] = ok
    return matched, sup


def support(seg_off, bitscore, desc_row, lineages, bad, records):
    """The eight fields of every query (DTYPE)."""
    matched, sup = supporting(seg_off, bitscore, desc_row, lineages, bad, records)
    out = np.zeros(len(seg_off) - 1, DTYPE)
    for q in range(len(out)):
        a, b = int(seg_off[q]), int(seg_off[q + 1])
        if b <= a:
            continue
        scores = [int(bitscore[i]) for i in range(a, b)]
        top = max(scores)
        o = out[q]
        o["n_hits"] = b - a
        o["n_matched"] = sum(1 for i in range(a, b) if matched[i])
        o["n_top"] = sum(1 for s in scores if s == top)
        o["n_top_support"] = sum(1 for i in range(a, b) if scores[i - a] == top and sup[i])
        o["n_support"] = sum(1 for i in range(a, b) if sup[i])
        o["top_score"] = top
        o["bits"] = sum(scores)
        o["support_bits"] = sum(scores[i - a] for i in range(a, b) if sup[i])
    return out


def lineages_of(lin_off, lin_node):
    return [[int(x) for x in lin_node[int(lin_off[t]):int(lin_off[t + 1])]] for t in range(len(lin_off) - 1)]


def render(results, query_names, fields):
    """The table's text: one line per result of the document, in its order; query_names[q] names the query of fields[q],
    a result whose query is not among them (a header without hits) has every count zero."""
    at = {(n.decode() if isinstance(n, bytes) else n): q for q, n in enumerate(query_names)}
    out = [HEADER]
    for r in results:
        taxon = r.get("taxon")
        if taxon is None:
            rank, ident = "-", "unclassified"
        elif taxon["taxonomy"] == "":
            rank, ident = "-", "unplaced"
        else:
            rank, ident = taxon["taxonomy"].split(";")[-1].split("__", 1)
        q = at.get(r["query"])
        v = [0] * 8 if q is None else [int(fields[q][f]) for f in SUPPORT_FIELDS]
        conf = float(v[4]) / float(v[0]) if v[0] else 0.0
        out.append("\t".join([r["query"], rank, ident] + [str(x) for x in v] + ["%.4f" % conf]) + "\n")
    return "".join(out)
