"""Independent statement of the bit-score band (include/blu_consensus.h: blu_score_band) in plain Python
integers, which neither overflow nor round.  Test infrastructure in the manner of tests/hit_filter_reference.py: shares no code
with the product.

The rule under test: a run with a band gives what the run without one gives on `rewrite_table`'s copy of the (filtered) table,
in which column 12 of every in-band line is the decimal text of its query's top truncated bit-score.
"""

MILLI_ONE = 100000          # 100 % in thousandths of a percent


def in_band(b, t, m=None, D=None) -> bool:
    """b, t: truncated bit-scores, b a row's and t its query's maximum; m: --top-percent times 1000 (None = not given);
    D: --top-bits (None = not given).  A row at the top is not `in the band`: it has nothing to be raised to."""
    b, t = int(b), int(t)
    if b >= t or (m is None and D is None):
        return False
    if D is not None and not b >= t - int(D):
        return False
    if m is not None and not b * MILLI_ONE >= t * (MILLI_ONE - int(m)):
        return False
    return True


def raise_scores(seg_off, bitscore, m=None, D=None):
    """-> (the raised column as a list of ints, n_raised, n_widened).  Segments as the library reads them: an offset beyond
    the column is clamped to its length and a decreasing pair is an empty segment."""
    out = [int(b) for b in bitscore]
    n = len(out)
    n_raised = n_widened = 0
    for q in range(len(seg_off) - 1):
        s1 = min(int(seg_off[q + 1]), n)
        s0 = min(int(seg_off[q]), s1)
        if s0 == s1:
            continue
        t = max(out[s0:s1])
        up = [i for i in range(s0, s1) if in_band(out[i], t, m, D)]
        for i in up:
            out[i] = t
        n_raised += len(up)
        n_widened += 1 if up else 0
    return out, n_raised, n_widened


def truncated(field) -> int:
    """column 12 as the parsers type it: the f64 value truncated toward zero (mod.rs:184)"""
    return int(float(field.decode() if isinstance(field, bytes) else field))


def rewrite_table(src, dst, m=None, D=None, kept=None):
    """Copies the lines of `src` to `dst`, those that are not kept left out and column 12 of every in-band line replaced by
    the decimal text of its query's top; everything else, line ends included, verbatim.  kept: one bool per non-empty line
    (the verdicts of tests/hit_filter_reference.keep or of a taxon filter), None = every line.  A query is every line with
    the same first column, wherever it stands in the file.  Returns (kept lines, raised lines, queries with a raised line,
    queries) — the counts blu_score_band_stats gives."""
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
        lines.append((raw, body.split(b"\t") if body else None, raw[len(body):]))
    if kept is not None:
        verdicts = iter(kept)
        lines = [l for l in lines if l[1] is None or next(verdicts)]
    top = {}
    for _, f, _ in lines:
        if f is not None:
            b = truncated(f[12])
            top[f[0]] = max(top.get(f[0], b), b)
    out, n_kept, n_raised, widened = [], 0, 0, set()
    for raw, f, eol in lines:
        if f is None:
            out.append(raw)
            continue
        n_kept += 1
        t = top[f[0]]
        if in_band(truncated(f[12]), t, m, D):
            n_raised += 1
            widened.add(f[0])
            raw = b"\t".join(f[:12] + [str(t).encode()] + f[13:]) + eol
        out.append(raw)
    open(dst, "wb").write(b"".join(out))
    return n_kept, n_raised, len(widened), len(top)
