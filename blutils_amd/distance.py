"""Bray-Curtis and Jaccard distances between the samples of a sample table.

    python -m blutils_amd.cli blastn build-distances TABLE -o OUT [--rank R] [--metric bray-curtis|jaccard]
        [--drop-unclassified] [--device N] [--rarefy D [--seed N] [--rarefied-table FILE]]

Not in the reference.  TABLE is what `--sample-table` or `build-report --by-sample` wrote.  Three steps, each a call of the
library: the features of the table at one rank as CSR (`features_from_table`, host), the pair integers of the CSR
(`sample_distances`, counted on the GPU: csrc/distance_kernel.hip; there is no CPU fallback), and the text of one metric
(`render`, host, integer arithmetic).  `build_distances` chains them in the library (pipeline.distance_matrix_file).  With `rarefy` a fourth step comes second:
every sample subsampled to one depth without replacement (`rarefy`, selected on the GPU: csrc/rarefy_kernel.hip; DESIGN.md §27;
no CPU fallback either), and the distances are those of the samples that reach the depth.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

from . import _native as N
from . import pipeline

METRICS = tuple(pipeline.DISTANCE_METRIC)


def features_from_table(table_path: str, rank: Optional[str] = None, drop_unclassified: bool = False) -> dict:
    """blu_distance_features_from_table -> {"row_ptr", "sample", "count": numpy arrays (uint64, uint32, uint64), "samples": the
    column names, "features": one text per feature, "n_dropped"}."""
    import numpy as np
    L = pipeline._bind()
    ft = pipeline.DistanceFeatures()
    rc = L.blu_distance_features_from_table(table_path.encode(), None if rank is None else rank.encode(),
                                            pipeline.DISTANCE_DROP_UNCLASSIFIED if drop_unclassified else 0, C.byref(ft))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_distance_features_from_table")
    try:
        nf, ns = int(ft.n_features), int(ft.n_samples)
        row_ptr = np.ctypeslib.as_array(ft.row_ptr, (nf + 1,)).copy()
        nnz = int(row_ptr[nf])
        return {"row_ptr": row_ptr,
                "sample": np.ctypeslib.as_array(ft.sample, (nnz,)).copy() if nnz else np.zeros(0, np.uint32),
                "count": np.ctypeslib.as_array(ft.count, (nnz,)).copy() if nnz else np.zeros(0, np.uint64),
                "samples": [ft.sample_names[s].decode("utf-8", "surrogateescape") for s in range(ns)],
                "features": [ft.feature_text[k].decode("utf-8", "surrogateescape") for k in range(nf)],
                "n_dropped": int(ft.n_dropped)}
    finally:
        L.blu_distance_features_free(C.byref(ft))


def sample_distances(row_ptr, sample, count, n_samples: int, device: int = 0, n_features: Optional[int] = None,
                     struct_size: Optional[int] = None) -> dict:
    """blu_sample_distances on host CSR arrays -> {"total" [S] uint64, "richness" [S] uint32, "min_sum" [S, S] uint64,
    "shared" [S, S] uint32, "t_device_ms"}.  n_features and struct_size default to what the arrays and the struct say."""
    import numpy as np
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    sample = np.ascontiguousarray(sample, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    desc = N.DistanceDesc(struct_size=C.sizeof(N.DistanceDesc) if struct_size is None else struct_size, device=int(device),
                          n_features=len(row_ptr) - 1 if n_features is None else int(n_features), n_samples=int(n_samples),
                          row_ptr=row_ptr.ctypes.data, sample=sample.ctypes.data if len(sample) else None,
                          count=count.ctypes.data if len(count) else None, stream=None)
    L = N.lib()
    out = N.SampleDistance()
    rc = L.blu_sample_distances(C.byref(desc), C.byref(out))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_sample_distances")
    try:
        s = int(out.n_samples)
        return {"total": np.ctypeslib.as_array(out.total, (s,)).copy(), "richness": np.ctypeslib.as_array(out.richness, (s,)).copy(),
                "min_sum": np.ctypeslib.as_array(out.min_sum, (s * s,)).copy().reshape(s, s),
                "shared": np.ctypeslib.as_array(out.shared, (s * s,)).copy().reshape(s, s), "t_device_ms": float(out.t_device_ms)}
    finally:
        L.blu_sample_distance_free(C.byref(out))


def render(metric: str, names: Sequence[str], total, richness, min_sum, shared, out_path: str) -> None:
    """blu_distance_render: the matrix of `metric` from the pair integers (any integer sequences; min_sum and shared [S][S])."""
    import numpy as np
    if metric not in pipeline.DISTANCE_METRIC:
        raise ValueError(f"unknown metric `{metric}`: bray-curtis or jaccard")
    s = len(names)
    total = np.ascontiguousarray(total, dtype=np.uint64).reshape(s)
    richness = np.ascontiguousarray(richness, dtype=np.uint32).reshape(s)
    min_sum = np.ascontiguousarray(min_sum, dtype=np.uint64).reshape(s * s)
    shared = np.ascontiguousarray(shared, dtype=np.uint32).reshape(s * s)
    d = N.SampleDistance(n_samples=s, total=total.ctypes.data_as(C.POINTER(C.c_uint64)),
                         richness=richness.ctypes.data_as(C.POINTER(C.c_uint32)),
                         min_sum=min_sum.ctypes.data_as(C.POINTER(C.c_uint64)), shared=shared.ctypes.data_as(C.POINTER(C.c_uint32)))
    arr = (C.c_char_p * max(s, 1))(*[n.encode("utf-8", "surrogateescape") for n in names])
    rc = pipeline._bind().blu_distance_render(pipeline.DISTANCE_METRIC[metric], arr, C.byref(d), out_path.encode())
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_distance_render")


def rarefy_stream(seed: int, name: str) -> int:
    """blu_rarefy_stream: the stream of the sample `name` under `seed`"""
    b = name.encode("utf-8", "surrogateescape")
    return int(N.lib().blu_rarefy_stream(int(seed) & (2 ** 64 - 1), b, len(b)))


def rarefy(row_ptr, sample, count, names: Sequence[str], depth: int, seed: int = 0, device: int = 0, n_features: Optional[int] = None,
           struct_size: Optional[int] = None, streams=None) -> dict:
    """blu_sample_rarefy on host CSR arrays: every sample of at least `depth` reads subsampled to `depth`, the others dropped ->
    {"kept_sample" [K] uint32, "row_ptr" [F + 1] uint64, "sample" uint32 (0 .. K - 1), "count" uint64, "t_device_ms"}.  The draw
    of a sample goes by its name and the seed (streams: the u64 per sample instead, for tests)."""
    import numpy as np
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    sample = np.ascontiguousarray(sample, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if streams is None:
        streams = [rarefy_stream(seed, n) for n in names]
    streams = np.ascontiguousarray(streams, dtype=np.uint64)
    desc = N.RarefyDesc(struct_size=C.sizeof(N.RarefyDesc) if struct_size is None else struct_size, device=int(device),
                        n_features=len(row_ptr) - 1 if n_features is None else int(n_features), n_samples=len(streams),
                        row_ptr=row_ptr.ctypes.data, sample=sample.ctypes.data if len(sample) else None,
                        count=count.ctypes.data if len(count) else None, sample_stream=streams.ctypes.data if len(streams) else None,
                        depth=int(depth), stream=None)
    L = N.lib()
    out = N.Rarefied()
    rc = L.blu_sample_rarefy(C.byref(desc), C.byref(out))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_sample_rarefy")
    try:
        nf, k = int(out.n_features), int(out.n_kept)
        rp = np.ctypeslib.as_array(out.row_ptr, (nf + 1,)).copy()
        nnz = int(rp[nf])
        return {"kept_sample": np.ctypeslib.as_array(out.kept_sample, (k,)).copy() if k else np.zeros(0, np.uint32), "row_ptr": rp,
                "sample": np.ctypeslib.as_array(out.sample, (nnz,)).copy() if nnz else np.zeros(0, np.uint32),
                "count": np.ctypeslib.as_array(out.count, (nnz,)).copy() if nnz else np.zeros(0, np.uint64),
                "t_device_ms": float(out.t_device_ms)}
    finally:
        L.blu_rarefied_free(C.byref(out))


def build_distances(table_path: str, out_path: str, rank: Optional[str] = None, metric: str = "bray-curtis",
                    drop_unclassified: bool = False, device: int = 0, rarefy: Optional[int] = None, seed: int = 0,
                    rarefied_table: Optional[str] = None) -> dict:
    """`blastn build-distances`: the matrix of `metric` between the samples of table_path, to out_path; the counts of the call.
    rarefy: the depth every sample is subsampled to first (those below it are dropped: "dropped" lists them with their reads)."""
    if rarefy is None:
        if seed or rarefied_table is not None:
            raise ValueError("seed and rarefied_table need rarefy")
        st = pipeline.distance_matrix_file(table_path, out_path, rank, metric, drop_unclassified, device)
        st["rank"] = rank
        return st
    import numpy as np
    st = pipeline.distance_matrix_file_with(table_path, out_path, rank, metric, drop_unclassified, device, rarefy, seed, rarefied_table)
    st["rank"] = rank
    st["seed"] = int(seed)
    ft = features_from_table(table_path, rank, drop_unclassified)       # (host; the table is small)
    total = np.zeros(len(ft["samples"]), np.uint64)
    np.add.at(total, ft["sample"], ft["count"])
    st["dropped"] = [(n, int(t)) for n, t in zip(ft["samples"], total) if int(t) < int(rarefy)]
    return st


def summary(st: dict) -> str:
    """the line the CLI prints to stderr"""
    return (f"distances: {st['n_features']} features at {st['rank'] if st.get('rank') is not None else 'no rank'}, "
            f"{st['n_samples']} samples, {st['n_nonzeros']} non-zeros")


def rarefy_summary(st: dict) -> list:
    """the lines the CLI prints after it when the samples were rarefied"""
    if not st.get("depth"):
        return []
    return ([f"rarefy: depth {st['depth']}, seed {st['seed']}, kept {st['n_samples_kept']} of "
             f"{st['n_samples_kept'] + st['n_samples_dropped']} samples, {st['n_features_emptied']} features emptied"]
            + [f"rarefy: dropped {n} ({t} reads)" for n, t in st["dropped"]])
