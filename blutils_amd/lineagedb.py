"""`build-db lineages`: the taxonomies database (`*.blutils.json`) from a two-column lineage table
`ID<TAB>d__Bacteria; p__Proteobacteria; ...` (SILVA, GTDB, UNITE, Greengenes, any QIIME 2 reference; not in the reference).
The build itself is csrc/lineage_db_gpu.hip behind include/blu_pipeline.h `blu_lineage_db_build`; this module prepares its
arguments and names its outputs as `build-db blu` does (taxdb.output_paths)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

from . import _native as N
from . import blast, taxdb


class LineageDbError(RuntimeError):
    pass


class LineageDbDesc(C.Structure):
    _fields_ = [("table_path", C.c_char_p), ("output_stem", C.c_char_p), ("taxid_map_path", C.c_char_p),
                ("replace_from", C.POINTER(C.c_char_p)), ("replace_to", C.POINTER(C.c_char_p)), ("n_replace", C.c_uint64),
                ("has_replace", C.c_int32), ("device", C.c_int32), ("source_database", C.c_char_p),
                ("blutils_version", C.c_char_p), ("hash_bits", C.c_uint32), ("initial_slots", C.c_uint32)]


STAT_COUNTS = ("lines", "data_lines", "taxonomies", "taxa", "empty", "truncated")
STAT_PLAIN = ("max_depth", "n_levels", "n_dictionary_builds", "input_bytes", "doc_bytes", "tsv_bytes", "map_bytes")
STAT_TIMES = ("upload", "parse", "intern", "group", "render", "write")


class LineageDbStats(C.Structure):
    _fields_ = ([("n_" + k, C.c_uint64) for k in STAT_COUNTS] + [(k, C.c_uint64) for k in STAT_PLAIN]
                + [("t_" + k + "_ms", C.c_double) for k in STAT_TIMES])

    def as_dict(self) -> Dict[str, float]:
        d = {k: int(getattr(self, "n_" + k)) for k in STAT_COUNTS}
        d.update({k: int(getattr(self, k)) for k in STAT_PLAIN})
        d.update({"t_" + k + "_ms": float(getattr(self, "t_" + k + "_ms")) for k in STAT_TIMES})
        return d


def parse_replace_rank(values: Optional[Sequence[str]]) -> Optional[List[Tuple[str, str]]]:
    """-r RANK=NEW as `build-db blu` takes it (exactly one '='), RANK lower-cased: it is matched against lower-cased tokens."""
    try:
        pairs = taxdb.parse_replace_rank(values)
    except taxdb.TaxdbError as e:
        raise LineageDbError(str(e)) from None
    return None if pairs is None else [(a.lower(), b) for a, b in pairs]


def output_paths(output_file_path: str) -> Tuple[str, str]:
    return taxdb.output_paths(output_file_path)


def summary(st: Dict[str, float]) -> str:
    return (f"lineage table: {st['data_lines']} lines, {st['taxonomies']} taxonomies, {st['taxa']} taxa, "
            f"{st['empty']} without a lineage, {st['truncated']} truncated, deepest {st['max_depth']} levels")


def build_ref_db_from_lineage_table(table_path: str, output_file_path: str, taxid_map_path: Optional[str] = None,
                                    replace_rank: Optional[Sequence[Tuple[str, str]]] = None, device: int = 0,
                                    hash_bits: int = 0, initial_slots: int = 0) -> Dict[str, float]:
    """One blu_lineage_db_build call; returns its stats.  hash_bits and initial_slots are the header's two test aids."""
    if not os.path.isfile(table_path):
        raise LineageDbError(f'Invalid lineage table path: "{table_path}"')
    L = N.lib()
    L.blu_lineage_db_build.restype = C.c_int
    L.blu_lineage_db_build.argtypes = [C.POINTER(LineageDbDesc), C.POINTER(LineageDbStats)]
    d = LineageDbDesc()
    keep = []
    d.table_path = table_path.encode()
    d.output_stem = taxdb.output_stem(output_file_path).encode()
    d.taxid_map_path = None if taxid_map_path is None else taxid_map_path.encode()
    if replace_rank is not None:
        fr = (C.c_char_p * max(len(replace_rank), 1))(*[a.encode() for a, _ in replace_rank])
        to = (C.c_char_p * max(len(replace_rank), 1))(*[b.encode() for _, b in replace_rank])
        keep += [fr, to]
        d.replace_from = C.cast(fr, C.POINTER(C.c_char_p))
        d.replace_to = C.cast(to, C.POINTER(C.c_char_p))
        d.n_replace = len(replace_rank)
        d.has_replace = 1
    d.device = device
    d.source_database = table_path.encode()
    d.blutils_version = blast.BLUTILS_VERSION.encode()
    d.hash_bits = hash_bits
    d.initial_slots = initial_slots
    st = LineageDbStats()
    rc = L.blu_lineage_db_build(C.byref(d), C.byref(st))
    if rc != N.BLU_OK:
        raise LineageDbError(f"build-db failed (blu_error {rc}): {N.last_error()}")
    return st.as_dict()
