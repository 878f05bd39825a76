"""`blu build-db kraken2` and `blu build-db qiime2`: a BLAST database's sequences exported for Kraken 2 and QIIME 2
(core/src/use_cases/build_kraken_db_from_ncbi_files/, build_qiime_db_from_blutils_db/mod.rs).  The sequence listing is
rewritten by csrc/seqdb_gpu.hip behind include/blu_pipeline.h `blu_seqdb_export`, streamed straight from the `blastdbcmd`
pipe; the QIIME taxonomy TSV is written on the host by `blu_qiime_taxonomy_tsv` (csrc/qiime_tsv.cpp).  This module does
what the reference does around them: the output names, the directory reset, the database check and the child process.

`build-db sintax` and `build-db dada2` are not in the reference: the kraken2 listing rewritten as one FASTA whose headers
carry the lineage of each line's taxid (`blu_seqdb_export_labelled`; DESIGN.md "Labelled FASTA export")."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile
from typing import Dict, Optional

from . import _native as N
from . import blast, taxdb

KRAKEN2, QIIME2, SINTAX, DADA2 = 0, 1, 2, 3
KRAKEN2_OUTFMT = "%a  %T  %s"             # generate_fasta_file.rs:45-52
QIIME2_OUTFMT = "%a  %T  %o  %s"          # build_qiime_db_from_blutils_db/mod.rs:103-110


class SeqdbError(RuntimeError):
    """`stats`: the counts up to the refused line, when blu_seqdb_export raised it (else None)."""
    stats: Optional[Dict[str, float]] = None


class SeqdbDesc(C.Structure):
    _fields_ = [("format", C.c_int32), ("input_fd", C.c_int32), ("input_path", C.c_char_p), ("fna_path", C.c_char_p),
                ("map_path", C.c_char_p), ("chunk_bytes", C.c_uint64), ("device", C.c_int32), ("reserved", C.c_int32)]


STAT_COUNTS = ("n_lines", "input_bytes", "fna_bytes", "map_bytes", "n_chunks", "max_line_bytes", "invalid_utf8_line")
STAT_TIMES = ("t_read_ms", "t_gpu_ms", "t_write_ms", "t_wall_ms")


class SeqdbStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in STAT_COUNTS] + [(k, C.c_double) for k in STAT_TIMES]

    def as_dict(self) -> Dict[str, float]:
        d = {k: int(getattr(self, k)) for k in STAT_COUNTS}
        d.update({k: float(getattr(self, k)) for k in STAT_TIMES})
        return d


class SeqdbLabelDesc(C.Structure):
    """include/blu_pipeline.h: blu_seqdb_label_desc"""
    _fields_ = [("format", C.c_int32), ("input_fd", C.c_int32), ("input_path", C.c_char_p), ("taxonomies_file", C.c_char_p),
                ("use_taxid", C.c_int32), ("device", C.c_int32), ("fna_path", C.c_char_p), ("chunk_bytes", C.c_uint64)]


LABEL_STAT_COUNTS = ("n_lines", "input_bytes", "fna_bytes", "n_chunks", "max_line_bytes", "invalid_utf8_line",
                     "n_unknown_taxid", "n_unlabelled", "n_rows", "label_bytes")
LABEL_STAT_TIMES = STAT_TIMES + ("t_labels_ms",)


class SeqdbLabelStats(C.Structure):
    """include/blu_pipeline.h: blu_seqdb_label_stats"""
    _fields_ = [(k, C.c_uint64) for k in LABEL_STAT_COUNTS] + [(k, C.c_double) for k in LABEL_STAT_TIMES]

    def as_dict(self) -> Dict[str, float]:
        d = {k: int(getattr(self, k)) for k in LABEL_STAT_COUNTS}
        d.update({k: float(getattr(self, k)) for k in LABEL_STAT_TIMES})
        return d


def set_extension(path: str, ext: str) -> str:
    """PathBuf::set_extension (taxdb.output_stem has the rules)"""
    return taxdb.output_stem(path) + "." + ext


def export(fmt: int, fna_path: str, map_path: Optional[str] = None, listing_path: Optional[str] = None,
           input_fd: int = -1, chunk_bytes: int = 0, device: int = 0) -> Dict[str, float]:
    """One blu_seqdb_export call over a listing file or an open descriptor; returns its stats."""
    L = N.lib()
    L.blu_seqdb_export.restype = C.c_int
    L.blu_seqdb_export.argtypes = [C.POINTER(SeqdbDesc), C.POINTER(SeqdbStats)]
    d = SeqdbDesc()
    d.format = fmt
    d.input_fd = input_fd
    d.input_path = listing_path.encode() if listing_path is not None else None
    d.fna_path = fna_path.encode()
    d.map_path = map_path.encode() if map_path is not None else None
    d.chunk_bytes = chunk_bytes
    d.device = device
    st = SeqdbStats()
    rc = L.blu_seqdb_export(C.byref(d), C.byref(st))
    if rc != N.BLU_OK:
        e = SeqdbError(f"build-db failed (blu_error {rc}): {N.last_error()}")
        e.stats = st.as_dict()
        raise e
    return st.as_dict()


def export_labelled(fmt: int, taxonomies_file: str, fna_path: str, use_taxid: bool = False, listing_path: Optional[str] = None,
                    input_fd: int = -1, chunk_bytes: int = 0, device: int = 0) -> Dict[str, float]:
    """One blu_seqdb_export_labelled call (fmt: SINTAX or DADA2) over a listing file or an open descriptor; returns its stats."""
    L = N.lib()
    L.blu_seqdb_export_labelled.restype = C.c_int
    L.blu_seqdb_export_labelled.argtypes = [C.POINTER(SeqdbLabelDesc), C.POINTER(SeqdbLabelStats)]
    d = SeqdbLabelDesc()
    d.format = fmt
    d.input_fd = input_fd
    d.input_path = listing_path.encode() if listing_path is not None else None
    d.taxonomies_file = taxonomies_file.encode()
    d.use_taxid = 1 if use_taxid else 0
    d.device = device
    d.fna_path = fna_path.encode()
    d.chunk_bytes = chunk_bytes
    st = SeqdbLabelStats()
    rc = L.blu_seqdb_export_labelled(C.byref(d), C.byref(st))
    if rc != N.BLU_OK:
        e = SeqdbError(f"build-db failed (blu_error {rc}): {N.last_error()}")
        e.stats = st.as_dict()
        raise e
    return st.as_dict()


def render_labels(fmt: int, taxonomies_file: str, out_path: str, use_taxid: bool = False) -> None:
    """blu_seqdb_render_labels: `TAXID\\tLABEL\\n` per row of the taxonomies file, on the host."""
    L = N.lib()
    L.blu_seqdb_render_labels.restype = C.c_int
    L.blu_seqdb_render_labels.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    rc = L.blu_seqdb_render_labels(taxonomies_file.encode(), 1 if use_taxid else 0, fmt, out_path.encode())
    if rc != N.BLU_OK:
        raise SeqdbError(f"build-db failed (blu_error {rc}): {N.last_error()}")


def export_from_blastdbcmd(fmt: int, database: str, fna_path: str, map_path: Optional[str], executable: str = "blastdbcmd",
                           chunk_bytes: int = 0, device: int = 0, labelled: Optional[dict] = None) -> Dict[str, float]:
    """`blastdbcmd -entry all -db DB -outfmt ...` with its stdout piped into the library.  When the library stops before the
    end of the listing (an invalid-UTF-8 line or an error) the child is killed; otherwise its exit status is checked.
    labelled: the taxonomies_file and use_taxid of export_labelled, for SINTAX and DADA2."""
    cmd = [executable, "-entry", "all", "-db", database, "-outfmt", QIIME2_OUTFMT if fmt == QIIME2 else KRAKEN2_OUTFMT]
    with tempfile.TemporaryFile() as err:
        try:
            p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=err)
        except OSError as e:
            raise SeqdbError(f"Unexpected error detected on execute blastdbcmd: {e}") from None
        stats, failure = None, None
        try:
            if labelled is not None:
                stats = export_labelled(fmt, fna_path=fna_path, listing_path="blastdbcmd output", input_fd=p.stdout.fileno(),
                                        chunk_bytes=chunk_bytes, device=device, **labelled)
            else:
                stats = export(fmt, fna_path, map_path, listing_path="blastdbcmd output", input_fd=p.stdout.fileno(),
                               chunk_bytes=chunk_bytes, device=device)
        except SeqdbError as e:
            failure = e
        finally:
            early = failure is not None or (stats is not None and stats["invalid_utf8_line"] != 0)
            if early and p.poll() is None:
                p.kill()
            p.stdout.close()
            rc = p.wait()
        if failure is not None:
            raise failure
        if not early and rc != 0:
            err.seek(0)
            raise SeqdbError(f"blastdbcmd failed ({rc}): {err.read().decode('utf-8', 'replace').strip()}")
    return stats


def build_kraken_db_from_ncbi_files(blast_database_path: str, output_directory: str, listing_file: Optional[str] = None,
                                    blastdbcmd: str = "blastdbcmd", chunk_bytes: int = 0, device: int = 0) -> Dict[str, float]:
    """build_kraken_db_from_ncbi_files/mod.rs:14-57.  listing_file: the text blastdbcmd would print (then no subprocess and
    no database check)."""
    if os.path.lexists(output_directory):                 # mod.rs:22-30: removed first, whatever it is
        if os.path.isdir(output_directory) and not os.path.islink(output_directory):
            shutil.rmtree(output_directory)
        else:
            os.remove(output_directory)
    os.makedirs(output_directory, exist_ok=True)          # mod.rs:32-34
    fna = os.path.join(output_directory, "library.fna")
    prelim = os.path.join(output_directory, "prelim_map.txt")
    if listing_file is not None:
        return export(KRAKEN2, fna, prelim, listing_path=listing_file, chunk_bytes=chunk_bytes, device=device)
    taxdb.validate_blast_database_with_taxdb(blast_database_path)   # generate_fasta_file.rs:24
    return export_from_blastdbcmd(KRAKEN2, blast_database_path, fna, prelim, blastdbcmd, chunk_bytes, device)


def build_qiime_db_from_blutils_db(taxonomies_database_path: str, output_taxonomies_file: str, blast_database_path: str,
                                   output_sequences_file: str, use_taxid: bool = False, listing_file: Optional[str] = None,
                                   blastdbcmd: str = "blastdbcmd", chunk_bytes: int = 0,
                                   device: int = 0) -> Dict[str, float]:
    """build_qiime_db_from_blutils_db/mod.rs:13-157: the TSV first, then the database check, then the sequences."""
    tsv = set_extension(output_taxonomies_file, "tsv")    # mod.rs:24-28
    if os.path.lexists(tsv):
        os.remove(tsv)
    L = N.lib()
    L.blu_qiime_taxonomy_tsv.restype = C.c_int
    L.blu_qiime_taxonomy_tsv.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    rc = L.blu_qiime_taxonomy_tsv(taxonomies_database_path.encode(), 1 if use_taxid else 0, tsv.encode())
    if rc != N.BLU_OK:
        raise SeqdbError(f"build-db failed (blu_error {rc}): {N.last_error()}")
    if listing_file is None:
        taxdb.validate_blast_database_with_taxdb(blast_database_path)   # mod.rs:92
    fna = set_extension(output_sequences_file, "fna")     # mod.rs:94-98
    if os.path.lexists(fna):
        os.remove(fna)
    if listing_file is not None:
        return export(QIIME2, fna, None, listing_path=listing_file, chunk_bytes=chunk_bytes, device=device)
    return export_from_blastdbcmd(QIIME2, blast_database_path, fna, None, blastdbcmd, chunk_bytes, device)


def _build_labelled_db(fmt: int, taxonomies_database_path: str, blast_database_path: str, output_sequences_file: str,
                       use_taxid: bool, listing_file: Optional[str], blastdbcmd: str, chunk_bytes: int, device: int) -> Dict[str, float]:
    fna = set_extension(output_sequences_file, "fna")
    if os.path.lexists(fna):
        os.remove(fna)
    if listing_file is not None:
        return export_labelled(fmt, taxonomies_database_path, fna, use_taxid, listing_path=listing_file, chunk_bytes=chunk_bytes,
                               device=device)
    taxdb.validate_blast_database_with_taxdb(blast_database_path)
    return export_from_blastdbcmd(fmt, blast_database_path, fna, None, blastdbcmd, chunk_bytes, device,
                                  labelled=dict(taxonomies_file=taxonomies_database_path, use_taxid=use_taxid))


def build_sintax_db_from_blutils_db(taxonomies_database_path: str, blast_database_path: str, output_sequences_file: str,
                                    use_taxid: bool = False, listing_file: Optional[str] = None, blastdbcmd: str = "blastdbcmd",
                                    chunk_bytes: int = 0, device: int = 0) -> Dict[str, float]:
    """Not in the reference.  OUTPUT.fna for `vsearch --sintax` / `usearch -sintax`: `>ACC;tax=d:...,p:...,s:...;` and the
    sequence on one line.  The taxonomies database is a *.blutils.json or a cache-db cache of the same lineage flavour; the
    listing is kraken2's.  listing_file: the text blastdbcmd would print (then no subprocess and no database check)."""
    return _build_labelled_db(SINTAX, taxonomies_database_path, blast_database_path, output_sequences_file, use_taxid, listing_file,
                              blastdbcmd, chunk_bytes, device)


def build_dada2_db_from_blutils_db(taxonomies_database_path: str, blast_database_path: str, output_sequences_file: str,
                                   use_taxid: bool = False, listing_file: Optional[str] = None, blastdbcmd: str = "blastdbcmd",
                                   chunk_bytes: int = 0, device: int = 0) -> Dict[str, float]:
    """Not in the reference.  OUTPUT.fna for DADA2's assignTaxonomy: `>Domain;Phylum;Class;Order;Family;Genus;` (cut at the
    first level the lineage lacks) and the sequence on one line.  Arguments as build_sintax_db_from_blutils_db."""
    return _build_labelled_db(DADA2, taxonomies_database_path, blast_database_path, output_sequences_file, use_taxid, listing_file,
                              blastdbcmd, chunk_bytes, device)
