"""Alpha diversity and rarefaction curves of the samples of a sample table.

    python -m blutils_amd.cli blastn build-diversity TABLE -o OUT [--rank R] [--drop-unclassified]
        [--depths D1,D2,... | --steps K [--max-depth M]] [--seed N] [--device N]

Not in the reference.  TABLE is what `--sample-table` or `build-report --by-sample` wrote.  Three steps, each a call of the
library: the features of the table at one rank as CSR (`distance.features_from_table`, host), the six integers per sample and
depth (`alpha`, counted on the GPU: csrc/alpha_kernel.hip; there is no CPU fallback), and the text (`render`, host, integer
arithmetic).  `build_diversity` chains them in the library (pipeline.alpha_table_file).  Without a ladder every read counts
(one line per sample); with one, a line per sample and depth it reaches, over exactly the reads `build-distances --rarefy D
--seed N` keeps at that depth: the curve is what one picks D from.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

from . import _native as N
from . import distance, pipeline

FIELDS = ("n", "observed", "singletons", "doubletons", "sum_sq", "sum_xlog")


def log2_fixed(x: int) -> int:
    """blu_alpha_log2: log2 x with 24 fractional bits"""
    return int(N.lib().blu_alpha_log2(int(x)))


def alpha(row_ptr, sample, count, names: Sequence[str], depths: Sequence[int] = (), seed: int = 0, device: int = 0,
          n_features: Optional[int] = None, struct_size: Optional[int] = None, streams=None) -> dict:
    """blu_sample_alpha on host CSR arrays -> {"present" [S, slots] uint8, "n", "sum_sq", "sum_xlog" uint64, "observed",
    "singletons", "doubletons" uint32, "t_device_ms"}; slots = len(depths), or 1 without depths (raw: every read counts).  The
    draw of a sample goes by its name and the seed (streams: the u64 per sample instead, for tests)."""
    import numpy as np
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    sample = np.ascontiguousarray(sample, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if streams is None:
        streams = [distance.rarefy_stream(seed, n) for n in names]
    streams = np.ascontiguousarray(streams, dtype=np.uint64)
    ladder = np.ascontiguousarray([int(d) for d in depths], dtype=np.uint64)
    desc = N.AlphaDesc(struct_size=C.sizeof(N.AlphaDesc) if struct_size is None else struct_size, device=int(device),
                       n_features=len(row_ptr) - 1 if n_features is None else int(n_features), n_samples=len(streams),
                       n_depths=len(ladder), row_ptr=row_ptr.ctypes.data, sample=sample.ctypes.data if len(sample) else None,
                       count=count.ctypes.data if len(count) else None, sample_stream=streams.ctypes.data if len(streams) else None,
                       depths=ladder.ctypes.data if len(ladder) else None, stream=None)
    L = N.lib()
    out = N.Alpha()
    rc = L.blu_sample_alpha(C.byref(desc), C.byref(out))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_sample_alpha")
    try:
        s, k = int(out.n_samples), int(out.n_slots)
        got = {f: np.ctypeslib.as_array(getattr(out, f), (s * k,)).copy().reshape(s, k) for f in ("present",) + FIELDS}
        got["t_device_ms"] = float(out.t_device_ms)
        return got
    finally:
        L.blu_alpha_free(C.byref(out))


def render(names: Sequence[str], reads, depths: Sequence[int], integers: dict, out_path: str) -> None:
    """blu_alpha_render: the file from the integers (as `alpha` returns them, or any integer sequences of [S][slots])"""
    import numpy as np
    s, k = len(names), max(len(depths), 1)
    present = np.ascontiguousarray(integers["present"], dtype=np.uint8).reshape(s * k)
    u64 = {f: np.ascontiguousarray(integers[f], dtype=np.uint64).reshape(s * k) for f in ("n", "sum_sq", "sum_xlog")}
    u32 = {f: np.ascontiguousarray(integers[f], dtype=np.uint32).reshape(s * k) for f in ("observed", "singletons", "doubletons")}
    a = N.Alpha(n_samples=s, n_slots=int(integers.get("n_slots", k)), present=present.ctypes.data_as(C.POINTER(C.c_uint8)),
                **{f: v.ctypes.data_as(C.POINTER(C.c_uint64)) for f, v in u64.items()},
                **{f: v.ctypes.data_as(C.POINTER(C.c_uint32)) for f, v in u32.items()})
    reads = (C.c_uint64 * max(s, 1))(*[int(r) for r in reads])
    ladder = (C.c_uint64 * max(len(depths), 1))(*[int(d) for d in depths])
    arr = (C.c_char_p * max(s, 1))(*[n.encode("utf-8", "surrogateescape") for n in names])
    rc = pipeline._bind().blu_alpha_render(arr, reads, ladder, len(depths), C.byref(a), out_path.encode())
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_alpha_render")


def ladder(steps: int, max_depth: int) -> list:
    """--steps K --max-depth M: D_k = max(1, floor(k M / K)) for k = 1 .. K, duplicates removed"""
    steps, max_depth = int(steps), int(max_depth)
    if steps < 1:
        raise ValueError("steps: one or more")
    if max_depth < 1:
        raise ValueError("max_depth: one read or more")
    return sorted({max(1, k * max_depth // steps) for k in range(1, steps + 1)})


def build_diversity(table_path: str, out_path: str, rank: Optional[str] = None, drop_unclassified: bool = False, device: int = 0,
                    depths: Optional[Sequence[int]] = None, steps: Optional[int] = None, max_depth: Optional[int] = None,
                    seed: Optional[int] = None) -> dict:
    """`blastn build-diversity`: the alpha file of table_path to out_path; the counts of the call, "depths" (the ladder used) and
    "partial": (name, total, depths reached) of every sample that misses some."""
    import numpy as np
    if depths is not None and steps is not None:
        raise ValueError("depths and steps: one or the other")
    if max_depth is not None and steps is None:
        raise ValueError("max_depth needs steps")
    if seed is not None and depths is None and steps is None:
        raise ValueError("seed needs depths or steps")
    ft = distance.features_from_table(table_path, rank, drop_unclassified)       # (host; the table is small)
    total = np.zeros(len(ft["samples"]), np.uint64)
    np.add.at(total, ft["sample"], ft["count"])
    if steps is not None:
        top = int(total.max()) if len(total) else 0
        depths = ladder(steps, top if max_depth is None else max_depth) if (top or max_depth is not None) else [1]
    depths = [] if depths is None else [int(d) for d in depths]
    st = pipeline.alpha_table_file(table_path, out_path, rank, drop_unclassified, device, depths, seed or 0)
    st["rank"] = rank
    st["depths"] = depths
    reached = [sum(1 for d in depths if d <= int(t)) for t in total]
    st["partial"] = [(n, int(t), j) for n, t, j in zip(ft["samples"], total, reached) if j < len(depths)]
    return st


def summary(st: dict) -> list:
    """the lines the CLI prints to stderr"""
    return ([f"diversity: {st['n_features']} features at {st['rank'] if st.get('rank') is not None else 'no rank'}, "
             f"{st['n_samples']} samples, {st['n_depths']} depths, {st['n_rows']} rows"]
            + [f"diversity: {n} ({t} reads) reaches {j} of {len(st['depths'])} depths" for n, t, j in st["partial"]])
