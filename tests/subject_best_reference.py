"""Independent statement of the best hit per subject (include/blu_consensus.h: blu_subject_best) in plain Python:
a dict per segment.  Test infrastructure in the manner of tests/score_band_reference.py: shares no code with the product.

The rule under test: a run with --best-hit-per-subject gives what the run without it gives on `rewrite_table`'s copy of the
(filtered) table, from which every line but the best of its (query, subject) pair was deleted.
"""


def keep(seg_off, bitscore, acc_rank):
    """-> (one 0 / 1 verdict per row, n_kept, n_thinned).  Segments as the library reads them: an offset beyond the columns is
    clamped to their length and a decreasing pair is an empty segment; a row that no segment names gets 0.  Of the rows of a
    segment with one acc_rank the first with the highest score is kept."""
    n = len(bitscore)
    out = [0] * n
    n_thinned = 0
    for q in range(len(seg_off) - 1):
        s1 = min(int(seg_off[q + 1]), n)
        s0 = min(int(seg_off[q]), s1)
        best = {}
        for i in range(s0, s1):
            a, b = int(acc_rank[i]), int(bitscore[i])
            if a not in best or b > best[a][0]:              # (strictly better only: the first of equals stays)
                best[a] = (b, i)
        for _, i in best.values():
            out[i] = 1
        n_thinned += 1 if len(best) < s1 - s0 else 0
    return out, sum(out), n_thinned


def compact(seg_off, verdicts, *columns):
    """-> (the new offsets, the columns with the dropped rows left out), for tables whose segments tile the rows"""
    n = len(verdicts)
    before = [0]
    for v in verdicts:
        before.append(before[-1] + (1 if v else 0))
    new_off = [before[min(int(o), n)] for o in seg_off]
    if len(new_off):
        new_off[-1] = before[n]
    return new_off, [[c[i] for i in range(n) if verdicts[i]] for c in columns]


def truncated(field) -> int:
    """column 12 as the parsers type it: the f64 value truncated toward zero (mod.rs:184)"""
    return int(float(field.decode() if isinstance(field, bytes) else field))


def rewrite_table(src, dst, kept=None):
    """Copies the lines of `src` to `dst`, leaving out those that are not kept and, of the lines of one (column 0, column 1) pair,
    all but the first with the highest truncated column 12; everything else, empty lines and line ends included, verbatim.
    kept: one bool per non-empty line (the verdicts of tests/hit_filter_reference.keep or of a taxon filter), None = every
    line.  A query is every line with the same first column, wherever it stands in the file.  Returns (lines in, lines kept,
    queries that lost a line, queries) — the counts blu_subject_best_stats gives."""
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
    if kept is not None:
        verdicts = iter(kept)
        lines = [l for l in lines if l[1] is None or next(verdicts)]
    best = {}
    for k, (_, f) in enumerate(lines):
        if f is not None:
            b = truncated(f[12])
            if (f[0], f[1]) not in best or b > best[(f[0], f[1])][0]:
                best[(f[0], f[1])] = (b, k)
    winners = {k for _, k in best.values()}
    n_in = sum(1 for _, f in lines if f is not None)
    queries = {f[0] for _, f in lines if f is not None}
    thinned = {f[0] for k, (_, f) in enumerate(lines) if f is not None and k not in winners}
    open(dst, "wb").write(b"".join(raw for k, (raw, f) in enumerate(lines) if f is None or k in winners))
    return n_in, len(winners), len(thinned), len(queries)
