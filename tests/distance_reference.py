"""Restatement of `build-distances` in plain Python integers: the feature rule on a sample-table text, the
pair integers, and the rendering.  Expected values in tests/test_distance.py and tests/test_gpu_distance.py come from here,
never from the library."""

LETTER = {"undefined": "u", "domain": "d", "kingdom": "k", "phylum": "p", "class": "c", "order": "o", "family": "f", "genus": "g",
          "species": "s"}


class Malformed(Exception):
    """a table the rule refuses; .line is the 1-based line it names (None: the rank)"""

    def __init__(self, line, what):
        self.line = line
        super().__init__(f"line {line}: {what}")


def rank_letter(rank):
    low = rank.strip().lower()
    return LETTER.get(low, low)


def features(text, rank=None, drop_unclassified=False):
    """-> (sample names, [(feature text, [count per sample])]) with the all-zero features left out, n_dropped.  Fixed rows
    first, then the file's order."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    head = lines[0].split("\t") if lines else []
    if head[:4] != ["#rank", "identifier", "taxonomy", "total"] or len(head) < 5:
        raise Malformed(1, "header")
    names = head[4:]
    ns = len(names)
    fixed = {"unclassified": [0] * ns, "unplaced": [0] * ns}
    rows = []                                   # (line, rank, taxonomy, clade cells)
    at = {}
    for no, line in enumerate(lines[1:], 2):
        cells = line.split("\t")
        if len(cells) != ns + 4:
            raise Malformed(no, "cells")
        vals = []
        for c in cells[3:]:
            if not c or any(ch not in "0123456789" for ch in c) or int(c) >= 1 << 64:
                raise Malformed(no, "not a u64")
            vals.append(int(c))
        if vals[0] != sum(vals[1:]):
            raise Malformed(no, "total")
        if cells[0] == "-" and cells[2] == "" and cells[1] in fixed:
            fixed[cells[1]] = vals[1:]
            continue
        if cells[2] in at or not cells[2]:
            raise Malformed(no, "taxonomy")
        at[cells[2]] = len(rows)
        rows.append((no, cells[0], cells[2], vals[1:]))
    parent = []
    for no, _, tax, _ in rows:
        if ";" not in tax:
            parent.append(None)
            continue
        up = tax.rsplit(";", 1)[0]
        if up not in at:
            raise Malformed(no, "parent missing")
        parent.append(at[up])
    direct = [list(r[3]) for r in rows]
    for i, r in enumerate(rows):
        if parent[i] is not None:
            for s in range(ns):
                direct[parent[i]][s] -= r[3][s]
    for i, d in enumerate(direct):
        if any(v < 0 for v in d):
            raise Malformed(rows[i][0], "negative direct count")
    feats = []
    if not drop_unclassified:
        feats += [("unclassified", fixed["unclassified"]), ("unplaced", fixed["unplaced"])]
    if rank is None:
        feats += [(r[2], direct[i]) for i, r in enumerate(rows)]
    else:
        want = rank_letter(rank)
        if not any(r[1] == want for r in rows):
            raise Malformed(None, f"rank {rank}")
        for i, r in enumerate(rows):
            chain, p = [], parent[i]
            while p is not None:
                chain.append(p)
                p = parent[p]
            if any(rows[p][1] == want for p in chain):
                continue
            feats.append((r[2], list(r[3]) if r[1] == want else direct[i]))
    # the invariant: per sample the features add up to unclassified + unplaced + the top-level clade counts
    for s in range(ns):
        expect = sum(r[3][s] for i, r in enumerate(rows) if parent[i] is None)
        if not drop_unclassified:
            expect += fixed["unclassified"][s] + fixed["unplaced"][s]
        assert sum(f[1][s] for f in feats) == expect, (s, expect)
    kept = [f for f in feats if any(f[1])]
    return names, kept, len(feats) - len(kept)


def csr(feats):
    """[(text, cells)] -> row_ptr, sample, count (lists of ints)"""
    row_ptr, sample, count = [0], [], []
    for _, cells in feats:
        for s, v in enumerate(cells):
            if v:
                sample.append(s)
                count.append(v)
        row_ptr.append(len(sample))
    return row_ptr, sample, count


def integers(row_ptr, sample, count, n_samples):
    """the CSR -> total [S], richness [S], min_sum [S][S], shared [S][S] in Python integers"""
    S = n_samples
    total, rich = [0] * S, [0] * S
    min_sum = [[0] * S for _ in range(S)]
    shared = [[0] * S for _ in range(S)]
    for f in range(len(row_ptr) - 1):
        e0, e1 = row_ptr[f], row_ptr[f + 1]
        for i in range(e0, e1):
            a, x = sample[i], count[i]
            total[a] += x
            rich[a] += 1
            ra, sa = min_sum[a], shared[a]
            for j in range(e0, e1):
                y = count[j]
                ra[sample[j]] += x if x < y else y
                sa[sample[j]] += 1
    return total, rich, min_sum, shared


def integers_dense(columns):
    """the same from per-sample {feature: count} dicts (for large sparse cases: the pair loop runs over the smaller dict)"""
    S = len(columns)
    total = [sum(c.values()) for c in columns]
    rich = [len(c) for c in columns]
    min_sum = [[0] * S for _ in range(S)]
    shared = [[0] * S for _ in range(S)]
    for a in range(S):
        for b in range(a, S):
            small, big = (columns[a], columns[b]) if len(columns[a]) <= len(columns[b]) else (columns[b], columns[a])
            m = n = 0
            for f, x in small.items():
                y = big.get(f)
                if y is not None:
                    m += x if x < y else y
                    n += 1
            min_sum[a][b] = min_sum[b][a] = m
            shared[a][b] = shared[b][a] = n
    return total, rich, min_sum, shared


def value(num, den):
    """six decimals, half up, in integers; `nan` for den = 0"""
    if den == 0:
        return "nan"
    q = (num * 10 ** 6 + den // 2) // den
    return f"{q // 10 ** 6}.{q % 10 ** 6:06d}"


def render(metric, names, total, rich, min_sum, shared):
    out = ["".join("\t" + n for n in names) + "\n"]
    for a, name in enumerate(names):
        cells = [name]
        for b in range(len(names)):
            if metric == "bray-curtis":
                n = total[a] + total[b]
                cells.append(value(n - 2 * min_sum[a][b], n))
            elif metric == "jaccard":
                i = shared[a][b]
                u = rich[a] + rich[b] - i
                cells.append(value(u - i, u))
            else:
                raise ValueError(metric)
        out.append("\t".join(cells) + "\n")
    return "".join(out)


def matrix_text(table_text, rank=None, metric="bray-curtis", drop_unclassified=False):
    """the whole chain on a table's text"""
    names, feats, _ = features(table_text, rank, drop_unclassified)
    total, rich, min_sum, shared = integers(*csr(feats), len(names))
    return render(metric, names, total, rich, min_sum, shared)
