"""Restatement of the rarefaction rule in Python and numpy integers: the stream of a sample, the keys of its
reads, the two routes to the kept counts, the output CSR and the rendering of the rarefied-table file.  Expected values in
tests/test_rarefy.py and tests/test_gpu_rarefy.py come from here, never from the library."""
import numpy as np

MASK = (1 << 64) - 1


def mix64(z):
    """the splitmix64 step on a Python integer"""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix64_np(z):
    """the same on a uint64 array (numpy's unsigned arithmetic wraps)"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fnv1a64(data: bytes):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & MASK
    return h


def stream(seed, name):
    """name: str (its UTF-8 bytes) or bytes"""
    data = name if isinstance(name, bytes) else name.encode("utf-8", "surrogateescape")
    return mix64(mix64(seed & MASK) ^ fnv1a64(data))


def keys(st, n):
    """key(a, i) for i = 0 .. n - 1"""
    return mix64_np(np.arange(n, dtype=np.uint64) + np.uint64(st))


def kept_by_sort(counts, depth, st):
    """route 1: sort all keys of the sample, take the first `depth`, count them per segment.  None: the sample is dropped"""
    counts = [int(c) for c in counts]
    n = sum(counts)
    if n < depth:
        return None
    first = np.argsort(keys(st, n), kind="stable")[:depth]              # (no ties: mix64 is a bijection)
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    return np.bincount(np.searchsorted(ends, first, side="right"), minlength=len(counts)).tolist()


def kept_by_threshold(counts, depth, st):
    """route 2: the depth-th smallest key by np.partition, then key <= T per segment"""
    counts = [int(c) for c in counts]
    n = sum(counts)
    if n < depth:
        return None
    k = keys(st, n)
    t = np.partition(k, depth - 1)[depth - 1]
    below = np.concatenate([[0], np.cumsum(k <= t)])
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    starts = ends - np.asarray(counts, dtype=np.int64)
    return (below[ends] - below[starts]).tolist()


def columns_of(row_ptr, sample, count, n_samples):
    """the CSR -> per sample the list of (feature, count) in feature order"""
    cols = [[] for _ in range(n_samples)]
    for f in range(len(row_ptr) - 1):
        for e in range(int(row_ptr[f]), int(row_ptr[f + 1])):
            cols[int(sample[e])].append((f, int(count[e])))
    return cols


def rarefy(row_ptr, sample, count, names, depth, seed=0, route=kept_by_threshold):
    """-> kept_sample, row_ptr, sample, count (lists of ints): what blu_sample_rarefy returns"""
    S, F = len(names), len(row_ptr) - 1
    cols = columns_of(row_ptr, sample, count, S)
    kept_sample, rows = [], [[] for _ in range(F)]
    for a in range(S):
        got = route([c for _, c in cols[a]], depth, stream(seed, names[a]))
        if got is None:
            continue
        assert sum(got) == depth
        for (f, _), x in zip(cols[a], got):
            if x:
                rows[f].append((len(kept_sample), x))
        kept_sample.append(a)
    out_ptr, out_sample, out_count = [0], [], []
    for r in rows:
        for a, x in r:                                  # (samples ascend: the columns were walked in order)
            out_sample.append(a)
            out_count.append(x)
        out_ptr.append(len(out_sample))
    return kept_sample, out_ptr, out_sample, out_count


def rarefied_features(names, feats, depth, seed=0):
    """distance_reference's (names, [(text, cells)]) rarefied: the kept names and [(text, cells over the kept samples)], every
    feature still there (an emptied one is all zero)"""
    from tests import distance_reference as ref
    kept, rp, sm, ct = rarefy(*ref.csr(feats), names, depth, seed)
    out = []
    for f, (text, _) in enumerate(feats):
        cells = [0] * len(kept)
        for e in range(rp[f], rp[f + 1]):
            cells[sm[e]] = ct[e]
        out.append((text, cells))
    return [names[a] for a in kept], out


def table_text(kept_names, feats):
    """the rarefied-table file: `#feature total <kept samples>`, one line per feature that is still non-zero"""
    out = ["#feature\ttotal" + "".join("\t" + n for n in kept_names) + "\n"]
    for text, cells in feats:
        if any(cells):
            out.append("\t".join([text, str(sum(cells))] + [str(c) for c in cells]) + "\n")
    return "".join(out)
