"""Restatement of the alpha-diversity rule in Python integers on top of tests/rarefy_reference.py: the
fixed-point logarithm, the two routes to the subsampled counts x'(j) of a ladder (rarefy at each depth; one entry level per
read), the six integers, the rendering and the ladder of --steps.  Expected values in tests/test_alpha.py and
tests/test_gpu_alpha.py come from here, never from the library."""
import numpy as np

from tests import rarefy_reference as rr

MASK = (1 << 64) - 1
FIELDS = ("n", "observed", "singletons", "doubletons", "sum_sq", "sum_xlog")
HEADER = "#sample\tdepth\treads\tobserved\tsingletons\tdoubletons\tchao1\tsimpson\tshannon\tgoods_coverage\n"


def log2_fixed(x):
    """L(x): log2 x with 24 fractional bits, by squaring"""
    assert x >= 1
    e = x.bit_length() - 1
    m, frac = x << (63 - e), 0
    for i in range(1, 25):
        p = m * m
        hi = p >> 64
        if hi >= 1 << 63:
            m = hi
            frac |= 1 << (24 - i)
        else:
            m = (p >> 63) & MASK
    return (e << 24) | frac


def counts_by_rarefy(counts, depths, st):
    """route 1: x'(j) = §27's kept counts at D_j, one rarefaction per depth.  None for a depth the sample does not reach"""
    return [rr.kept_by_threshold(counts, d, st) for d in depths]


def counts_by_entry_level(counts, depths, st):
    """route 2: e(o) = the first slot whose threshold T(D_j) the key of read o does not pass; x'(j) = the reads with e <= j"""
    counts = [int(c) for c in counts]
    n = sum(counts)
    live = [d for d in depths if d <= n]
    out = [None] * len(depths)
    if not live:
        return out
    k = rr.keys(st, n)
    ordered = np.sort(k)
    thresholds = np.array([ordered[d - 1] for d in live], dtype=np.uint64)
    entry = np.searchsorted(thresholds, k, side="left")                  # the first j with key <= T_j; len(live): none
    owner = np.repeat(np.arange(len(counts)), counts)
    enter = np.zeros((len(counts), len(live) + 1), dtype=np.int64)
    np.add.at(enter, (owner, entry), 1)
    cum = np.cumsum(enter[:, :len(live)], axis=1)
    for j in range(len(live)):
        out[j] = cum[:, j].tolist()
    return out


def integers(xs):
    """the six integers of one list of counts"""
    xs = [int(x) for x in xs]
    return {"n": sum(xs), "observed": sum(1 for x in xs if x > 0), "singletons": xs.count(1), "doubletons": xs.count(2),
            "sum_sq": sum(x * x for x in xs), "sum_xlog": sum(x * log2_fixed(x) for x in xs if x > 0)}


def alpha(row_ptr, sample, count, names, depths=(), seed=0, route=counts_by_entry_level, streams=None):
    """-> {"present": [S][slots], field: [S][slots]}: what blu_sample_alpha returns (absent slots hold 0)"""
    S = len(names)
    cols = rr.columns_of(row_ptr, sample, count, S)
    slots = max(len(depths), 1)
    out = {f: [[0] * slots for _ in range(S)] for f in ("present",) + FIELDS}
    for a in range(S):
        counts = [c for _, c in cols[a]]
        if depths:
            st = rr.stream(seed, names[a]) if streams is None else int(streams[a])
            per_slot = route(counts, list(depths), st)
        else:
            per_slot = [counts]
        for j, xs in enumerate(per_slot):
            if xs is None:
                continue
            got = integers(xs)
            assert got["n"] == (depths[j] if depths else sum(counts))
            out["present"][a][j] = 1
            for f in FIELDS:
                out[f][a][j] = got[f]
    return out


def six(num, den):
    """num / den with six decimals, half up, in integers"""
    q = (num * 1000000 + den // 2) // den
    return f"{q // 1000000}.{q % 1000000:06d}"


def line(name, depth, reads, v):
    n, obs, f1, f2 = v["n"], v["observed"], v["singletons"], v["doubletons"]
    assert v["sum_sq"] <= n * n and f1 <= n and f1 + f2 <= obs
    cells = [name, str(depth), str(reads), str(obs), str(f1), str(f2), six(obs * 2 * (f2 + 1) + f1 * (f1 - 1), 2 * (f2 + 1))]
    if n == 0:
        cells += ["nan", "nan", "nan"]
    else:
        cells += [six(n * n - v["sum_sq"], n * n), six(max(0, n * log2_fixed(n) - v["sum_xlog"]), n << 24), six(n - f1, n)]
    return "\t".join(cells) + "\n"


def render(names, reads, depths, ints):
    """the file from the integers of `alpha`"""
    out = [HEADER]
    for a, name in enumerate(names):
        for j in range(max(len(depths), 1)):
            if ints["present"][a][j]:
                out.append(line(name, depths[j] if depths else reads[a], reads[a], {f: ints[f][a][j] for f in FIELDS}))
    return "".join(out)


def ladder(steps, max_depth):
    """--steps K --max-depth M"""
    return sorted({max(1, k * max_depth // steps) for k in range(1, steps + 1)})


def table_text(names, feats, depths=(), seed=0):
    """distance_reference's (names, [(text, cells)]) -> the alpha file"""
    from tests import distance_reference as ref
    csr = ref.csr(feats)
    reads = [sum(c[s] for _, c in feats) for s in range(len(names))]
    return render(names, reads, list(depths), alpha(*csr, names, list(depths), seed))
