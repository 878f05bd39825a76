"""`blu build-db blu`: the taxonomies database (`*.blutils.json`) from an NCBI taxdump and a BLAST database's accession list
(core/src/use_cases/build_blutils_db_from_ncbi_files/mod.rs:34-86).  The build itself is csrc/taxdb_gpu.hip behind
include/blu_pipeline.h `blu_taxdb_build`; this module prepares its arguments (the database check, the `blastdbcmd` listing,
the output names) exactly as the reference does."""
from __future__ import annotations

import ctypes as C
import glob
import os
import shutil
import subprocess
import tempfile
from typing import Dict, List, Optional, Sequence, Tuple

from . import _native as N
from . import blast

DUMPS = ("nodes", "names", "taxidlineage", "merged", "delnodes")
BLASTDBCMD_OUTFMT = "%a  %T  %o"           # build_accessions_map.rs:31-38


class TaxdbError(RuntimeError):
    pass


class TaxdbDesc(C.Structure):
    _fields_ = [("nodes_path", C.c_char_p), ("names_path", C.c_char_p), ("lineage_path", C.c_char_p),
                ("merged_path", C.c_char_p), ("delnodes_path", C.c_char_p), ("accessions_path", C.c_char_p),
                ("skip_taxids", C.POINTER(C.c_uint64)), ("n_skip", C.c_uint64), ("has_skip", C.c_int32),
                ("has_replace", C.c_int32), ("replace_from", C.POINTER(C.c_char_p)), ("replace_to", C.POINTER(C.c_char_p)),
                ("n_replace", C.c_uint64), ("drop_non_linnaean", C.c_int32), ("device", C.c_int32),
                ("source_database", C.c_char_p), ("blutils_version", C.c_char_p), ("output_stem", C.c_char_p)]


STAT_COUNTS = ("nodes", "names", "lineage_tokens", "accession_lines", "distinct_taxids", "mapped", "mapped_merged",
               "deleted", "merged_missing", "unknown", "dropped", "unmapped_ancestors", "nonascii_names")
STAT_BYTES = ("input_bytes", "doc_bytes", "tsv_bytes")
STAT_TIMES = ("upload", "parse", "tables", "group", "assemble", "render", "write")


class TaxdbStats(C.Structure):
    _fields_ = ([("n_" + k, C.c_uint64) for k in STAT_COUNTS] + [(k, C.c_uint64) for k in STAT_BYTES]
                + [("t_" + k + "_ms", C.c_double) for k in STAT_TIMES])

    def as_dict(self) -> Dict[str, float]:
        d = {k: int(getattr(self, "n_" + k)) for k in STAT_COUNTS}
        d.update({k: int(getattr(self, k)) for k in STAT_BYTES})
        d.update({"t_" + k + "_ms": float(getattr(self, "t_" + k + "_ms")) for k in STAT_TIMES})
        return d


def parse_replace_rank(values: Optional[Sequence[str]]) -> Optional[List[Tuple[str, str]]]:
    """ports/cli/src/cmds/db_builder/mod.rs:25-33: exactly one '=' per value."""
    if values is None:
        return None
    out = []
    for v in values:
        parts = v.split("=")
        if len(parts) != 2:
            raise TaxdbError(f"Invalid replace rank option: {v!r}")
        out.append((parts[0], parts[1]))
    return out


def output_stem(output_file_path: str) -> str:
    """build_taxonomy_database.rs:240-270: PathBuf::set_extension("json"), then <parent>/<file_stem>."""
    parent, name = os.path.split(output_file_path)
    body = name.lstrip(".")
    if "." in body:
        name = name[:len(name) - len(body)] + body.rsplit(".", 1)[0]
    return os.path.join(parent, name)


def output_paths(output_file_path: str) -> Tuple[str, str]:
    stem = output_stem(output_file_path)
    return stem + ".blutils.json", stem + ".non-mapped.tsv"


def validate_blast_database_with_taxdb(path: str) -> None:
    """shared/validate_blast_database.rs:5-60: a `<stem>*.nsq` must exist (blast.validate_blast_database) and `taxdb.btd`
    must sit beside the first one."""
    blast.validate_blast_database(path)
    stem = os.path.splitext(os.path.basename(path))[0]
    parent = os.path.expanduser(os.path.dirname(path))
    nsq = sorted(glob.glob(os.path.join(parent, stem + "*.nsq")))[0]
    if not os.path.exists(os.path.join(os.path.dirname(nsq), "taxdb.btd")):
        raise TaxdbError(f'Taxdb not found: "{os.path.dirname(nsq)}"')


def blastdbcmd_listing(database: str, out_path: str, executable: str = "blastdbcmd") -> None:
    """build_accessions_map.rs:31-38: `blastdbcmd -entry all -db DB -outfmt "%a  %T  %o"`, stdout to out_path."""
    cmd = [executable, "-entry", "all", "-db", database, "-outfmt", BLASTDBCMD_OUTFMT]
    try:
        with open(out_path, "wb") as f:
            p = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE)
    except OSError as e:
        raise TaxdbError(f"Unexpected error detected on execute blastdbcmd: {e}") from None
    if p.returncode != 0:
        raise TaxdbError(f"blastdbcmd failed ({p.returncode}): {p.stderr.decode('utf-8', 'replace').strip()}")


def build_from_files(dumps: Dict[str, str], accessions_path: str, output_file_path: str, source_database: str,
                     skip_taxids: Optional[Sequence[int]] = None, replace_rank: Optional[Sequence[Tuple[str, str]]] = None,
                     drop_non_linnaean_taxonomies: bool = False, device: int = 0) -> Dict[str, float]:
    """One blu_taxdb_build call; returns its stats."""
    L = N.lib()
    L.blu_taxdb_build.restype = C.c_int
    L.blu_taxdb_build.argtypes = [C.POINTER(TaxdbDesc), C.POINTER(TaxdbStats)]
    d = TaxdbDesc()
    keep = []
    for field, key in (("nodes_path", "nodes"), ("names_path", "names"), ("lineage_path", "taxidlineage"),
                       ("merged_path", "merged"), ("delnodes_path", "delnodes")):
        setattr(d, field, dumps[key].encode())
    d.accessions_path = accessions_path.encode()
    if skip_taxids is not None:
        arr = (C.c_uint64 * max(len(skip_taxids), 1))(*skip_taxids)
        keep.append(arr)
        d.skip_taxids = C.cast(arr, C.POINTER(C.c_uint64))
        d.n_skip = len(skip_taxids)
        d.has_skip = 1
    if replace_rank is not None:
        fr = (C.c_char_p * max(len(replace_rank), 1))(*[a.encode() for a, _ in replace_rank])
        to = (C.c_char_p * max(len(replace_rank), 1))(*[b.encode() for _, b in replace_rank])
        keep += [fr, to]
        d.replace_from = C.cast(fr, C.POINTER(C.c_char_p))
        d.replace_to = C.cast(to, C.POINTER(C.c_char_p))
        d.n_replace = len(replace_rank)
        d.has_replace = 1
    d.drop_non_linnaean = 1 if drop_non_linnaean_taxonomies else 0
    d.device = device
    d.source_database = source_database.encode()
    d.blutils_version = blast.BLUTILS_VERSION.encode()
    d.output_stem = output_stem(output_file_path).encode()
    st = TaxdbStats()
    rc = L.blu_taxdb_build(C.byref(d), C.byref(st))
    if rc != N.BLU_OK:
        raise TaxdbError(f"build-db failed (blu_error {rc}): {N.last_error()}")
    return st.as_dict()


def build_ref_db_from_ncbi_files(blast_database_path: str, taxdump_directory_path: str, output_file_path: str,
                                 skip_taxids: Optional[Sequence[int]] = None,
                                 replace_rank: Optional[Sequence[Tuple[str, str]]] = None,
                                 drop_non_linnaean_taxonomies: bool = False, accessions_file: Optional[str] = None,
                                 blastdbcmd: str = "blastdbcmd", device: int = 0) -> Dict[str, float]:
    """mod.rs:34-86.  accessions_file: the text blastdbcmd would print (then no subprocess and no database check)."""
    tmpdir = None
    try:
        if accessions_file is None:
            validate_blast_database_with_taxdb(blast_database_path)
            # beside the output: the listing of nt is several GB
            tmpdir = tempfile.mkdtemp(prefix=".blu-build-db-", dir=os.path.dirname(os.path.abspath(output_file_path)))
            accessions_file = os.path.join(tmpdir, "accessions.txt")
            blastdbcmd_listing(blast_database_path, accessions_file, blastdbcmd)
        if not os.path.isdir(taxdump_directory_path):
            raise TaxdbError(f'Invalid taxdump directory path: "{taxdump_directory_path}"')
        dumps = {k: os.path.join(taxdump_directory_path, k + ".dmp") for k in DUMPS}
        for key, label in (("names", "names"), ("taxidlineage", "lineages"), ("nodes", "nodes"),
                           ("delnodes", "delnodes"), ("merged", "merged")):          # build_taxonomy_database.rs:64-99
            if not os.path.isfile(dumps[key]):
                raise TaxdbError(f'Invalid {label} path: "{dumps[key]}"')
        return build_from_files(dumps, accessions_file, output_file_path, blast_database_path, skip_taxids, replace_rank,
                                drop_non_linnaean_taxonomies, device)
    finally:
        if tmpdir is not None:
            shutil.rmtree(tmpdir, ignore_errors=True)
