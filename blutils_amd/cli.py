"""`blu`-compatible driver for the consensus step.

    python -m blutils_amd.cli blastn build-consensus BLAST_OUT -t TAX.json --taxon bacteria --strategy relaxed
        [-c CUTOFFS.yaml] [-u] [--blutils-out-file OUT] [--out-format json|jsonl|yaml]

Same arguments as the reference's `blu blastn build-consensus`
(ports/cli/src/cmds/blast/commands.rs:105-143, cmds/blast/mod.rs:104-146): without --blutils-out-file the
document goes to stdout (compact JSON, as serde_json::to_writer prints it); with it, the extension is forced to
the format's (write_blutils_output.rs:39-52) and JSON is pretty-printed.

    python -m blutils_amd.cli blastn build-tabular [BLU_RESULT|-] [-o OUT] [-i json|jsonl|yaml]

= `blu blastn build-tabular` (commands.rs:145-161, parse_consensus_as_tabular/mod.rs:15).

    python -m blutils_amd.cli blastn build-consensus ... --report FILE [--report-weight one|size]
    python -m blutils_amd.cli blastn run-with-consensus ... --report FILE [--report-weight one|size]
    python -m blutils_amd.cli blastn build-report [BLU_RESULT|-] [-o OUT] [-i json|jsonl|yaml] [--weight one|size]
    python -m blutils_amd.cli blastn build-consensus ... --sample-table FILE [--report-weight one|size]
    python -m blutils_amd.cli blastn run-with-consensus ... --sample-table FILE [--report-weight one|size]
    python -m blutils_amd.cli blastn build-report [BLU_RESULT|-] --by-sample [-o OUT] [-i json|jsonl|yaml] [--weight one|size]

not in the reference: the taxon abundance report — how many queries, or with `size` weighting how many
dereplicated reads (`;size=N` / `_size_N` in the query name), each taxon holds, summed up the lineage.  With --report it is
counted on the GPU from the run's own records and written after the document, which stays what it is without the flag;
build-report makes it on the host from an existing document, including one written by reference blutils
(blutils_amd/report.py, csrc/report_kernel.hip).  --sample-table (and build-report --by-sample) writes the same counts as a
taxon x sample table, one column per sample named in the query names (`;sample=S`, or a `S.<n>` label as
vsearch --relabel writes it); a query that names no sample is an error.

    python -m blutils_amd.cli blastn build-consensus ... [--min-perc-identity P] [--min-align-length L] [--max-e-value E]
        [--min-bit-score B]
    python -m blutils_amd.cli blastn run-with-consensus ... (the same four)

not in the reference: hit filters.  Only the lines of the table that meet every threshold given take part, as
if the others had been deleted from the file first; the GPU parser applies them.  With run-with-consensus the BLAST table is
still written in full (`-p/-q/-e` go to blastn itself); the filter applies to the consensus step.  One line goes to stderr:
`hit filter: kept K of N lines`.

    python -m blutils_amd.cli blastn build-consensus ... --support-table FILE
    python -m blutils_amd.cli blastn run-with-consensus ... --support-table FILE

not in the reference: the per-query support table.  One tab-separated line per result, in the document's
order: the last element of its taxonomy, the number of hits, how many of them name a taxon of the database, the size of the
top bit-score group, and how many hits — of the top group and of all — lie in the clade the result names, with the bit-score
sums and `confidence` = support / hits.  Counted on the GPU from the run's own records and columns (csrc/support_kernel.hip)
and written after the document, the report and the sample table; it combines with those flags and with the hit filters
(the counts are then over the kept lines).  The document stays what it is without the flag.

    python -m blutils_amd.cli blastn build-consensus ... [--exclude-taxon EL]... [--only-taxon EL]...
        [--exclude-taxon-file FILE] [--only-taxon-file FILE]
    python -m blutils_amd.cli blastn run-with-consensus ... (the same four)

not in the reference: taxon filters.  EL is an element as the lineages of the run spell it, `RANK__IDENTIFIER`
(`s__uncultured-bacterium`, `species__x` for `s__x`, `s__1423` under -u); an identifier ending in `*` is a prefix pattern
(`s__uncultured-*`).  A line of the table takes part only if the lineage of its subject holds no --exclude-taxon element and,
when --only-taxon is given, at least one of those; lines whose subject is not in the taxonomies file have no elements.  The
flags repeat; the FILE forms hold one element per line (blank lines and `#` comments skipped).  An element that names no taxon
of the taxonomies file is an error.  The verdict is taken by the parser, on the GPU where it parses, before the hit filters,
and the run gives what it gives on a copy of the table without the dropped lines.  To stderr:
`taxon filter: excluded X, not in --only-taxon Y, of N lines`, then `  EL: count` per exclude element that dropped lines.

    python -m blutils_amd.cli blastn build-consensus ... [--best-hit-per-subject]
    python -m blutils_amd.cli blastn run-with-consensus ... (the same)

not in the reference: the best hit per subject.  BLAST writes one line per HSP, so a subject that aligns to a
query in several places — a genome with seven rRNA operons — occurs several times among the query's hits.  With the flag, of the
lines of one (query, subject accession) pair that the filters above keep, only the best takes part: the highest truncated
bit-score, the first in file order among equals.  The run gives what it gives on a copy of the table without the other lines
— the document, --report, --sample-table and --support-table; one pass over the grouped columns on the GPU
(csrc/subject_kernel.hip) makes it so, before the band below.  What `blastn -max_hsps 1` would have given, without running
BLAST again.  To stderr, after the filter lines: `subject best hit: kept K of N lines, thinned W of Q queries`.

    python -m blutils_amd.cli blastn build-consensus ... [--top-percent P] [--top-bits D]
    python -m blutils_amd.cli blastn run-with-consensus ... (the same two)

not in the reference: the bit-score band.  The reference decides a query by the hits that tie exactly on its top
truncated bit-score; with a band, the hits just under the top count as tied with it, as MEGAN's top-percent or BASTA's band do.
A hit with truncated score b is in the band under the top t when b * 100000 >= t * (100000 - 1000 P) (--top-percent: P a decimal
with at most three decimals, 0 .. 100; read exactly, compared in integers) and b >= t - D (--top-bits: D an integer below 2^32);
with both flags both must hold.  The top is taken over the lines the filters above keep.  The run gives what it gives on a copy
of the table in which column 12 of every in-band line is replaced by its query's top score — the document, --report,
--sample-table and --support-table (whose top_hits is then the band's size, and whose bits / support_bits sum the raised scores);
one pass over the bit-score column on the GPU (csrc/band_kernel.hip) makes it so.  `--top-percent 0` and `--top-bits 0` are the
exact ties: the bytes of the run without the flag.  To stderr, after the filter lines:
`score band: raised R of N lines in W of Q queries`.

    python -m blutils_amd.cli blastn build-consensus ... [--min-cover P]
    python -m blutils_amd.cli blastn run-with-consensus ... (the same)

not in the reference: the minimum cover.  The reference asks every hit of a query's top bit-score group to agree,
so one mislabelled accession among forty tied hits of one species sends the query to the domain — and a band widens the group.
With --min-cover P (a decimal with at most three decimals, above 50 and at most 100; read exactly, compared in integers) the
query is placed at the deepest taxon that still covers P percent of its top hits, as MEGAN's percent-to-cover does: of the n
lines on the top score — the band's lines included — `need` is the smallest integer with need * 100 >= n * P, the covering
lineage prefix is the longest one that at least `need` of them start with, and the top lines that do not start with it do not
take part.  Lines under the top score are never touched; a query with a top line whose taxid is not in the taxonomies file, or
whose lineage is bad or empty, is left as it is.  Applied last, on the table the filters, --best-hit-per-subject and the band
leave: the run gives what it gives on a copy of that table without the dropped lines — the document, --report, --sample-table
and --support-table; one pass over the grouped columns on the GPU (csrc/cover_kernel.hip) makes it so.  `--min-cover 100` drops
nothing: the bytes of the run without the flag.  To stderr, after the band's line:
`min cover: kept K of N lines, narrowed W of Q queries, U left alone`.

    python -m blutils_amd.cli blastn build-consensus ... --count-table FILE (--report FILE | --sample-table FILE)
    python -m blutils_amd.cli blastn run-with-consensus ... (the same)
    python -m blutils_amd.cli blastn build-report [BLU_RESULT|-] [--by-sample] --count-table FILE [-o OUT] [-i json|jsonl|yaml]

not in the reference: abundances from an OTU / ASV count table.  In the usual amplicon workflow only the
representative sequences go through BLAST and their abundances live in a feature x sample table (`vsearch --otutabout`,
`usearch -otutab`, a DADA2 sequence table, `biom convert --to-tsv`): tab-separated, a header whose first cell is ignored and
whose other cells name the samples, then one row per representative with one whole-number cell per sample (`12` or `12.0`, below
2^32); blank lines, and `#` lines without a tab before the header, are skipped.  Rows and queries are joined on their names
up to the first `;`.  --sample-table then has one column per sample of the header (all of them, ascending bytewise) and a query
adds its count in each sample to every taxon of its lineage; --report weighs a query by its row sum.  A row without a result —
a representative BLAST gave no line for — counts as unclassified; a query without a row, two rows or two queries with one key,
a malformed cell (named by line and column) or a row sum of 2^32 or more fail the run before any file is written.  The counts
are summed on the GPU from the run's own records (csrc/report_kernel.hip: count_cells); build-report does the same on the host
from an existing document.  The document and --support-table stay what they are without the flag.  Not together with
`--report-weight size` / `--weight size`.  To stderr, after the selection's lines:
`count table: R rows, S samples, J joined to results, M without a result counted as unclassified`.

    python -m blutils_amd.cli blastn build-consensus ... --blast-outfmt SPEC

not in the reference: tables in any outfmt-6 column order.  build-consensus expects the thirteen columns of the
reference's own blastn call, `6 qseqid saccver staxid pident length mismatch gapopen qstart qend sstart send evalue bitscore`.  A
table written with another list — `6 std staxids`, one that carries `qcovs` or `qlen`, the output of an older pipeline — is read
with --blast-outfmt SPEC, SPEC being the string blastn was given: specifiers separated by blanks, an optional leading `6`, `std`
for BLAST's twelve standard columns, at most 64 columns, none named twice.  The seven fields the run reads are found by name:
the query (`qseqid`, else `qacc`, else `qaccver`), the subject accession (`saccver`, else `sacc`, else `sseqid`), the taxid
(`staxid`, else `staxids`, of which the id before the first `;` counts), `pident`, `length`, `bitscore` and — only needed by
--max-e-value — `evalue`; every other column is skipped.  The run gives what it gives on a copy of the table rewritten to the
reference's columns, under every other flag, and both parsers read the fields in place: no rewritten copy is made.  A line with
fewer fields than SPEC names is an error naming the line.  run-with-consensus writes its own table and has no such flag.

    python -m blutils_amd.cli blastn build-consensus ... --blast-outfmt SPEC --min-query-cover P
        [--query-cover-from auto|qcovhsp|qlen|qcovs]

not in the reference CLI: query coverage, the third threshold of the reference's own blastn call (`-q`, there
`-qcov_hsp_perc`), on a table that already exists.  P is a decimal with at most three decimals, 0 .. 100, read exactly.  A line
takes part only if its coverage is at least P, taken from the columns SPEC names: `qcovhsp` (BLAST's per-HSP integer percent c:
kept when c >= P), else `qstart qend qlen` (kept when (|qend - qstart| + 1) * 100 >= P * qlen, in integers: the exact ratio, not
BLAST's rounded percent, so 79.6 % is below 80 where `qcovhsp` prints 80), else `qcovs` (per subject over all HSPs of the pair:
the coarser figure); --query-cover-from names one of the three instead.  A source whose columns SPEC lacks is an error naming
them, and without --blast-outfmt the flag is refused: the reference's thirteen columns hold no query length.  The coverage
fields are read only under the flag, as integers 0 .. 2^31 - 1 (qlen above 0); one that is not is an error naming the line,
kept or not.  The GPU parser decides it with the other filters — after the taxon verdict, before the e-value — and the run gives
what it gives on a copy of the table without the failing lines.  `--min-query-cover 0` keeps every line.  To stderr, before the
hit filter's line: `query cover: B of N lines under P percent (from SOURCE)`.  run-with-consensus has `-q` for blastn itself
and no such flag.

    python -m blutils_amd.cli blastn build-distances TABLE -o OUT [--rank R] [--metric bray-curtis|jaccard]
        [--drop-unclassified] [--device N] [--rarefy D [--seed N] [--rarefied-table FILE]]
    python -m blutils_amd.cli blastn build-consensus ... --sample-table FILE --distance-matrix OUT [--distance-rank R]
        [--distance-metric M] [--distance-rarefy D [--distance-seed N] [--distance-rarefied-table FILE]]
    python -m blutils_amd.cli blastn run-with-consensus ... (the same three)
    python -m blutils_amd.cli blastn build-report [BLU_RESULT|-] --by-sample -o FILE --distance-matrix OUT (the same two)

not in the reference: distances between the samples of a sample table.  TABLE is what --sample-table or
build-report --by-sample wrote.  Its rows are collapsed at rank R (the table's rank column: `g`, or `genus`): every row of rank
R not under another one is a feature with its clade counts, every row that neither is nor lies under a row of rank R is a feature
with its direct counts (queries that ended above R, branches that skip R), and unclassified and unplaced are one feature each
unless --drop-unclassified leaves them out; without --rank every row is a feature with its direct counts.  OUT is a square
tab-separated matrix with the sample names on both sides, in the table's column order: Bray-Curtis (the default) or Jaccard
distances with six decimals, `nan` between two empty samples.  The sums behind them are integers counted on the GPU
(csrc/distance_kernel.hip) and the rounding is done in integers, half up, so the bytes do not depend on the machine.  A table
whose lines do not add up — a total that is not its cells' sum, children that pass their parent, a missing parent — is an
error naming the line.  The --distance-matrix form runs the same call on the file --sample-table (build-report: -o) just wrote,
after every other output.  To stderr: `distances: F features at R, S samples, Z non-zeros`.

--rarefy D subsamples every sample to D reads first, without replacement: raw counts mostly measure sequencing
depth.  Samples with fewer than D reads are dropped from the matrix, a sample of exactly D reads is kept whole.  The draw is a
rule in integers — read i of a sample is kept when its 64-bit hash, keyed by --seed (default 0) and the sample's NAME, is among
the sample's D smallest — selected on the GPU (csrc/rarefy_kernel.hip), so the same table, depth and seed give the same bytes
on any machine, and re-ordering or leaving out columns does not change the draw of the others.  --rarefied-table FILE also
writes the rarefied features: `#feature total <kept samples>`, one line per feature that is still non-zero.  Two columns of one
name, a D no sample reaches (the message says the largest total) and a sample of 2^32 reads or more are errors.  To stderr,
after the `distances:` line, which then counts the kept samples and the rarefied non-zeros:
`rarefy: depth D, seed N, kept K of S samples, E features emptied`, and `rarefy: dropped SAMPLE (TOTAL reads)` per dropped sample.

    python -m blutils_amd.cli blastn build-diversity TABLE -o OUT [--rank R] [--drop-unclassified]
        [--depths D1,D2,... | --steps K [--max-depth M]] [--seed N] [--device N]
    python -m blutils_amd.cli blastn build-consensus ... --sample-table FILE --alpha-table OUT [--alpha-rank R]
        [--alpha-depths D1,D2,... | --alpha-steps K] [--alpha-seed N]
    python -m blutils_amd.cli blastn run-with-consensus ... (the same five)
    python -m blutils_amd.cli blastn build-report [BLU_RESULT|-] --by-sample -o FILE --alpha-table OUT (the same four)

not in the reference: alpha diversity and rarefaction curves.  OUT is
`#sample depth reads observed singletons doubletons chao1 simpson shannon goods_coverage`, one line per sample; with a ladder
(at most 32 depths: --depths, or --steps K for D_k = max(1, floor(k M / K)), M the largest sample total unless --max-depth says
it), one line per sample and depth the sample reaches, over exactly the reads `build-distances --rarefy D --seed N` keeps at
that depth — the curve is what D is picked from.  The sums are integers counted on the GPU (csrc/alpha_kernel.hip), Shannon's
logarithm included (a fixed-point log2 with 24 fractional bits), and rendered with six decimals half up in integers, so the
bytes do not depend on the machine.  The --alpha-table form runs the same call on the file --sample-table (build-report: -o)
just wrote, after every other output.  To stderr: `diversity: F features at R, S samples, K depths, P rows`, and with a ladder
`diversity: SAMPLE (TOTAL reads) reaches J of K depths` per sample that misses some.

    python -m blutils_amd.cli cache-db TAX.json CACHE [-u]

writes the binary cache of a taxonomies file (not in the reference CLI; pass CACHE as -t afterwards).  
    python -m blutils_amd.cli blastn run-with-consensus [QUERY.fa|-] -d DB -t TAX.json --blast-out-file B --taxon T
        --strategy S [...]

= `blu blastn run-with-consensus` (commands.rs:24-103): `blastn` itself stays an external process (blutils_amd/blast.py).

    python -m blutils_amd.cli build-db blu BLAST_DATABASE_PATH TAXDUMP_DIRECTORY_PATH OUTPUT_FILE_PATH
        [-d] [-s TAXID]... [-r RANK=NEW]... [--accessions-file FILE] [--blastdbcmd EXE] [--device N]

= `blu build-db blu` (ports/cli/src/cmds/db_builder/commands.rs:22-77): the taxonomies database built on the GPU
(blutils_amd/taxdb.py, csrc/taxdb_gpu.hip); `blastdbcmd` stays an external process.

    python -m blutils_amd.cli build-db lineages TABLE OUTPUT_FILE_PATH [--taxid-map FILE] [-r RANK=NEW]... [--device N]

(not in the reference CLI) the taxonomies database from a lineage table `ID<TAB>d__Bacteria; p__Proteobacteria; ...` (SILVA,
GTDB, UNITE, Greengenes, any QIIME 2 reference), interned and rendered on the GPU (blutils_amd/lineagedb.py,
csrc/lineage_db_gpu.hip).  Every distinct path gets a taxid, from 1 in order of first appearance; `--taxid-map FILE` writes
the `ID taxid` lines that `makeblastdb -parse_seqids -taxid_map FILE` takes, so that BLAST prints those ids in `staxid`.  To
stderr: `lineage table: N lines, U taxonomies, T taxa, E without a lineage, C truncated, deepest D levels`.

    python -m blutils_amd.cli build-db kraken2 BLAST_DATABASE_PATH -o OUTPUT_DIRECTORY
        [--listing-file FILE] [--blastdbcmd EXE] [--device N]
    python -m blutils_amd.cli build-db qiime2 TAXONOMIES_DATABASE_PATH OUTPUT_TAXONOMIES_FILE BLAST_DATABASE_PATH
        OUTPUT_SEQUENCES_FILE [-u] [--listing-file FILE] [--blastdbcmd EXE] [--device N]

= `blu build-db kraken2` / `blu build-db qiime2` (commands.rs:11-20): the sequences of `blastdbcmd -entry all` rewritten on
the GPU as they stream from the pipe (blutils_amd/seqdb.py, csrc/seqdb_gpu.hip); the QIIME taxonomy TSV is rendered on the
host from a `*.blutils.json` that `build-db blu` wrote.

    python -m blutils_amd.cli build-db sintax TAXONOMIES_DATABASE_PATH BLAST_DATABASE_PATH OUTPUT_SEQUENCES_FILE
        [-u] [--listing-file FILE] [--blastdbcmd EXE] [--device N]
    python -m blutils_amd.cli build-db dada2 TAXONOMIES_DATABASE_PATH BLAST_DATABASE_PATH OUTPUT_SEQUENCES_FILE
        [-u] [--listing-file FILE] [--blastdbcmd EXE] [--device N]

(not in the reference CLI) one FASTA whose headers carry the lineage, for `vsearch --sintax` (`>ACC;tax=d:...,p:...;`) and
for DADA2's assignTaxonomy (`>Domain;Phylum;...;Genus;`): the kraken2 listing joined on the GPU, taxid by taxid, to the
labels rendered from TAXONOMIES_DATABASE_PATH (a `*.blutils.json` or a `cache-db` cache).  A line whose taxid the
taxonomies file does not hold, or whose lineage gives no label, is left out.  To stderr:
`labelled export: wrote K of N lines, U with a taxid not in the taxonomies file, E without a label`."""
from __future__ import annotations

import argparse
import functools
import os
import sys

from . import _native, blast, distance, diversity, lineagedb, pipeline, report, seqdb, tabular, taxdb


class _BlastnParser(argparse.ArgumentParser):
    """argparse's prefix matching for every flag but the query-cover pair, which is taken only when spelled out: `--min-query-cov`
    stays the unknown flag it was (run-with-consensus calls blastn's own threshold `--query-cov`)."""

    def _get_option_tuples(self, option_string):
        return [t for t in super()._get_option_tuples(option_string) if t[0].dest not in ("min_query_cover", "query_cover_from")]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="blu", description="MI355X-native consensus step of blutils")
    sub = ap.add_subparsers(dest="cmd", required=True)
    blastn = sub.add_parser("blastn").add_subparsers(dest="sub", required=True, parser_class=_BlastnParser)
    bc = blastn.add_parser("build-consensus", help="consensus identities from a BLAST outfmt-6 table")
    bc.add_argument("blast_out")
    bc.add_argument("-t", "--tax-file", required=True)
    bc.add_argument("--blutils-out-file")
    bc.add_argument("--taxon", required=True, choices=["fungi", "bacteria", "eukaryotes", "custom"])
    bc.add_argument("-c", "--custom-taxon-cutoff-file")
    bc.add_argument("--strategy", required=True, choices=["cautious", "relaxed"])
    bc.add_argument("-u", "--use-taxid", action="store_true")
    bc.add_argument("--out-format", default="json", choices=["json", "jsonl", "yaml"])
    bc.add_argument("--device", type=int, default=0, help="HIP device ordinal (not in the reference CLI)")
    bc.add_argument("--blast-outfmt", metavar="SPEC",
                    help="the -outfmt string BLAST_OUT was written with, when it is not the reference's `6 qseqid saccver staxid pident "
                         "length mismatch gapopen qstart qend sstart send evalue bitscore`: e.g. \"6 std staxids\"; the columns are "
                         "found by name, in any order (not in the reference CLI)")
    qcv = bc.add_argument_group("query coverage (not in the reference CLI)",
                                "a line of the table takes part only if its query coverage is at least P; needs --blast-outfmt, "
                                "which names the columns; applied by the parser, on the GPU where it parses")
    qcv.add_argument("--min-query-cover", type=_min_query_cover, metavar="P",
                     help="keep lines whose query coverage is at least P percent; a decimal with at most three decimals, 0 .. 100 "
                          "(not in the reference CLI)")
    qcv.add_argument("--query-cover-from", default="auto", choices=["auto", "qcovhsp", "qlen", "qcovs"],
                     help="where the coverage comes from: the `qcovhsp` column, the exact ratio of `qstart qend qlen`, the `qcovs` "
                          "column, or (auto) the first of these that --blast-outfmt names")
    rw = blastn.add_parser("run-with-consensus", help="blastn fan-out (chunks of 50 queries) + consensus")
    rw.add_argument("query", nargs="?", default="-")
    rw.add_argument("-d", "--database", required=True)
    rw.add_argument("-t", "--tax-file", required=True)
    rw.add_argument("--blast-out-file", required=True)
    rw.add_argument("--blutils-out-file")
    rw.add_argument("--out-format", default="json", choices=["json", "jsonl", "yaml"])
    rw.add_argument("--taxon", required=True, choices=["fungi", "bacteria", "eukaryotes", "custom"])
    rw.add_argument("-c", "--custom-taxon-cutoff-file")
    rw.add_argument("--strategy", required=True, choices=["cautious", "relaxed"])
    rw.add_argument("-u", "--use-taxid", action="store_true")
    rw.add_argument("-f", "--force-overwrite", action="store_true")
    rw.add_argument("-m", "--max-target-seqs", type=int)
    rw.add_argument("-p", "--perc-identity", type=int)
    rw.add_argument("-q", "--query-cov", type=int)
    rw.add_argument("--strand", choices=["both", "plus", "minus"])
    rw.add_argument("-e", "--e-value", type=float)
    rw.add_argument("-w", "--word-size", type=int)
    rw.add_argument("--threads", type=int, default=1, help="the reference's global `--threads` option (default 1)")
    rw.add_argument("--blastn", default="blastn", help="blastn executable (not in the reference CLI)")
    rw.add_argument("--device", type=int, default=0, help="HIP device ordinal (not in the reference CLI)")
    for sp in (bc, rw):
        sp.add_argument("--report", help="also write the taxon abundance report of the results to this file, counted on the "
                                         "GPU (not in the reference CLI)")
        sp.add_argument("--report-weight", default="one", choices=["one", "size"],
                        help="count results (one) or the dereplicated reads in the query names (size); for --report and "
                             "--sample-table")
        sp.add_argument("--sample-table", help="also write the taxon x sample table of the results to this file, counted "
                                               "on the GPU; samples from `;sample=S` or `S.<n>` query names (not in the "
                                               "reference CLI)")
        sp.add_argument("--support-table", help="also write the per-query support table to this file: how many of a query's "
                                                "hits lie in the clade it was assigned to, counted on the GPU (not in the "
                                                "reference CLI)")
        sp.add_argument("--count-table", metavar="FILE",
                        help="a feature x sample count table (OTU / ASV table, tab-separated): --report and --sample-table count "
                             "its abundances, joined to the queries on their names up to the first `;`, instead of what the "
                             "query names say; needs one of the two, not with --report-weight size (not in the reference CLI)")
        flt = sp.add_argument_group("hit filters (not in the reference CLI)",
                                    "a line of the table takes part only if it meets every threshold given; applied by "
                                    "the parser, on the GPU where it parses")
        flt.add_argument("--min-perc-identity", type=_threshold, metavar="P",
                         help="keep lines with perc_identity (column 4) >= P (not in the reference CLI)")
        flt.add_argument("--min-align-length", type=_length, metavar="L",
                         help="keep lines with align_length (column 5) >= L (not in the reference CLI)")
        flt.add_argument("--max-e-value", type=_threshold, metavar="E",
                         help="keep lines with e_value (column 12) <= E (not in the reference CLI)")
        flt.add_argument("--min-bit-score", type=_threshold, metavar="B",
                         help="keep lines with bit_score (column 13) as written >= B (not in the reference CLI)")
        tfl = sp.add_argument_group("taxon filters (not in the reference CLI)",
                                    "a line of the table takes part only if its subject's lineage passes; elements are "
                                    "RANK__IDENTIFIER as the lineages spell them, a trailing * makes a prefix pattern; "
                                    "applied by the parser, on the GPU where it parses")
        tfl.add_argument("--exclude-taxon", action="append", default=[], metavar="EL",
                         help="drop lines whose lineage holds EL; repeatable (not in the reference CLI)")
        tfl.add_argument("--only-taxon", action="append", default=[], metavar="EL",
                         help="keep only lines whose lineage holds one of these; repeatable (not in the reference CLI)")
        tfl.add_argument("--exclude-taxon-file", metavar="FILE",
                         help="--exclude-taxon elements, one per line; blank lines and # comments skipped")
        tfl.add_argument("--only-taxon-file", metavar="FILE",
                         help="--only-taxon elements, one per line; blank lines and # comments skipped")
        sbj = sp.add_argument_group("best hit per subject (not in the reference CLI)",
                                    "one line per (query, subject accession) pair; applied after the filters, on the GPU, "
                                    "before the band")
        sbj.add_argument("--best-hit-per-subject", action="store_true",
                         help="of the lines of one (query, subject accession) pair keep the one with the highest truncated "
                              "bit-score, the first in file order among equals (not in the reference CLI)")
        bnd = sp.add_argument_group("bit-score band (not in the reference CLI)",
                                    "hits inside a band under a query's top bit-score count as tied with it; applied after "
                                    "the filters, on the GPU, before the consensus")
        bnd.add_argument("--top-percent", type=_top_percent, metavar="P",
                         help="hits whose truncated bit-score is within P percent of the query's top count as tied with it; "
                              "a decimal with at most three decimals, 0 .. 100 (not in the reference CLI)")
        bnd.add_argument("--top-bits", type=_top_bits, metavar="D",
                         help="hits whose truncated bit-score is at most D below the query's top count as tied with it; an "
                              "integer, 0 .. 2^32 - 1 (not in the reference CLI)")
        cov = sp.add_argument_group("minimum cover (not in the reference CLI)",
                                    "top hits outside the deepest taxon that still covers P percent of a query's top group do "
                                    "not take part; applied after the band, on the GPU, before the consensus")
        cov.add_argument("--min-cover", type=_min_cover, metavar="P",
                         help="place a query at the deepest taxon that covers at least P percent of its top hits and drop the "
                              "top hits outside it; a decimal with at most three decimals, above 50 and at most 100 (not in the "
                              "reference CLI)")
    br = blastn.add_parser("build-report", help="blutils result document -> taxon abundance report (not in the reference)")
    br.add_argument("blu_result", nargs="?", default="-")
    br.add_argument("-o", "--output-file")
    br.add_argument("-i", "--input-format", default="json", choices=["json", "jsonl", "yaml"])
    br.add_argument("--weight", default="one", choices=["one", "size"])
    br.add_argument("--by-sample", action="store_true",
                    help="write the taxon x sample table instead of the report (not in the reference CLI)")
    br.add_argument("--count-table", metavar="FILE",
                    help="a feature x sample count table: the abundances of the results, joined on their names up to the first "
                         "`;`, instead of what the query names say; not with --weight size (not in the reference CLI)")
    bdi = blastn.add_parser("build-distances", help="sample table -> Bray-Curtis or Jaccard distance matrix between its samples, "
                                                    "counted on the GPU (not in the reference)")
    bdi.add_argument("table", help="a file written by --sample-table or build-report --by-sample")
    bdi.add_argument("-o", "--output-file", required=True)
    bdi.add_argument("--rank", metavar="R", help="collapse the rows at this rank, as the table's rank column spells it (`g`, or "
                                                 "`genus`); default: every row by its direct counts")
    bdi.add_argument("--metric", default="bray-curtis", choices=list(distance.METRICS))
    bdi.add_argument("--drop-unclassified", action="store_true", help="leave the unclassified and unplaced rows out")
    bdi.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    bdi.add_argument("--rarefy", metavar="D", type=_depth, help="subsample every sample to D reads first, without replacement, on "
                                                               "the GPU; samples with fewer are dropped")
    bdi.add_argument("--seed", metavar="N", type=_seed, help="the seed of the draw, 0 .. 2^64 - 1 (default 0); needs --rarefy")
    bdi.add_argument("--rarefied-table", metavar="FILE", help="also write the rarefied features to FILE; needs --rarefy")
    for sp in (bc, rw, br):
        dst = sp.add_argument_group("sample distances (not in the reference CLI)",
                                    "the distance matrix of the sample table just written, as build-distances makes it")
        dst.add_argument("--distance-matrix", metavar="FILE",
                         help="also write the distance matrix between the samples to FILE; needs "
                              + ("--by-sample and -o" if sp is br else "--sample-table"))
        dst.add_argument("--distance-rank", metavar="R", help="build-distances --rank")
        dst.add_argument("--distance-metric", choices=list(distance.METRICS), help="build-distances --metric (default bray-curtis)")
        dst.add_argument("--distance-rarefy", metavar="D", type=_depth, help="build-distances --rarefy")
        dst.add_argument("--distance-seed", metavar="N", type=_seed, help="build-distances --seed; needs --distance-rarefy")
        dst.add_argument("--distance-rarefied-table", metavar="FILE", help="build-distances --rarefied-table; needs --distance-rarefy")
    bdv = blastn.add_parser("build-diversity", help="sample table -> alpha diversity of its samples, raw or along a ladder of "
                                                    "rarefaction depths, counted on the GPU (not in the reference)")
    bdv.add_argument("table", help="a file written by --sample-table or build-report --by-sample")
    bdv.add_argument("-o", "--output-file", required=True)
    bdv.add_argument("--rank", metavar="R", help="collapse the rows at this rank, as build-distances --rank")
    bdv.add_argument("--drop-unclassified", action="store_true", help="leave the unclassified and unplaced rows out")
    bdv.add_argument("--depths", metavar="D1,D2,...", type=_depths, help="the ladder: at most 32 depths, strictly ascending")
    bdv.add_argument("--steps", metavar="K", type=_steps, help="the ladder D_k = max(1, floor(k M / K)), k = 1 .. K, duplicates removed")
    bdv.add_argument("--max-depth", metavar="M", type=_depth, help="the top of --steps' ladder (default: the largest sample total)")
    bdv.add_argument("--seed", metavar="N", type=_seed, help="the seed of the draw, as build-distances --seed; needs a ladder")
    bdv.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    for sp in (bc, rw, br):
        alp = sp.add_argument_group("alpha diversity (not in the reference CLI)",
                                    "the alpha diversity of the sample table just written, as build-diversity makes it")
        alp.add_argument("--alpha-table", metavar="FILE",
                         help="also write the alpha diversity of the samples to FILE; needs "
                              + ("--by-sample and -o" if sp is br else "--sample-table"))
        alp.add_argument("--alpha-rank", metavar="R", help="build-diversity --rank")
        alp.add_argument("--alpha-depths", metavar="D1,D2,...", type=_depths, help="build-diversity --depths")
        alp.add_argument("--alpha-steps", metavar="K", type=_steps, help="build-diversity --steps")
        alp.add_argument("--alpha-seed", metavar="N", type=_seed, help="build-diversity --seed; needs --alpha-depths or --alpha-steps")
    bt = blastn.add_parser("build-tabular", help="blutils result document -> TSV")
    bt.add_argument("blu_result", nargs="?", default="-")
    bt.add_argument("-o", "--output-file")
    bt.add_argument("-i", "--input-format", default="json", choices=["json", "jsonl", "yaml"])
    bd = sub.add_parser("build-db").add_subparsers(dest="sub", required=True)
    db = bd.add_parser("blu", help="the taxonomies database (*.blutils.json) from an NCBI taxdump and a BLAST database")
    db.add_argument("blast_database_path")
    db.add_argument("taxdump_directory_path")
    db.add_argument("output_file_path")
    db.add_argument("-d", "--drop-non-linnaean-taxonomies", action="store_true")
    db.add_argument("-s", "--skip-taxid", type=_u64, action="append")
    db.add_argument("-r", "--replace-rank", action="append")
    db.add_argument("--accessions-file", help="the text `blastdbcmd -entry all -db DB -outfmt \"%%a  %%T  %%o\"` prints; "
                                              "no blastdbcmd run and no database check (not in the reference CLI)")
    db.add_argument("--blastdbcmd", default="blastdbcmd", help="blastdbcmd executable (not in the reference CLI)")
    db.add_argument("--device", type=int, default=0, help="HIP device ordinal (not in the reference CLI)")
    ln = bd.add_parser("lineages", help="the taxonomies database (*.blutils.json) from a lineage table ID<TAB>d__...; p__...; "
                                        "(SILVA, GTDB, UNITE, Greengenes, QIIME 2; not in the reference CLI)")
    ln.add_argument("table", help="two tab-separated columns: ID and lineage; a `Feature ID` header, blank lines and # comments "
                                  "are skipped, a third column is ignored")
    ln.add_argument("output_file_path")
    ln.add_argument("--taxid-map", help="also write `ID taxid` per line, for makeblastdb -parse_seqids -taxid_map")
    ln.add_argument("-r", "--replace-rank", action="append", help="RANK=NEW: levels of rank RANK (lower-cased) get rank NEW")
    ln.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    kr = bd.add_parser("kraken2", help="library.fna and prelim_map.txt for Kraken 2 from a BLAST database",
                       description="OUTPUT_DIRECTORY is removed first, whether it is a directory or a file, and created "
                                   "again, before the database is checked (as the reference does).")
    kr.add_argument("blast_database_path")
    kr.add_argument("-o", "--output-directory", required=True,
                    help="removed if it exists (directory or file), then created; gets library.fna and prelim_map.txt")
    qi = bd.add_parser("qiime2", help="QIIME 2 taxonomy TSV and sequences from a *.blutils.json and a BLAST database")
    qi.add_argument("taxonomies_database_path")
    qi.add_argument("output_taxonomies_file")
    qi.add_argument("blast_database_path")
    qi.add_argument("output_sequences_file")
    qi.add_argument("-u", "--use-taxid", action="store_true")
    sx = bd.add_parser("sintax", help="FASTA with SINTAX headers (>ACC;tax=d:...,p:...;) from a *.blutils.json and a BLAST "
                                      "database (not in the reference CLI)")
    da = bd.add_parser("dada2", help="FASTA with DADA2 assignTaxonomy headers (>Domain;Phylum;...;Genus;) from a "
                                     "*.blutils.json and a BLAST database (not in the reference CLI)")
    for sp in (sx, da):
        sp.add_argument("taxonomies_database_path", help="a *.blutils.json or a cache-db cache of the same lineage flavour")
        sp.add_argument("blast_database_path")
        sp.add_argument("output_sequences_file", help="gets the extension fna; removed first if it exists")
        sp.add_argument("-u", "--use-taxid", action="store_true", help="labels from numericLineage")
    for sp, fmt in ((kr, seqdb.KRAKEN2_OUTFMT), (qi, seqdb.QIIME2_OUTFMT), (sx, seqdb.KRAKEN2_OUTFMT), (da, seqdb.KRAKEN2_OUTFMT)):
        sp.add_argument("--listing-file", help=f"the text `blastdbcmd -entry all -db DB -outfmt \"{fmt}\"` prints; "
                                               "no blastdbcmd run and no database check (not in the reference CLI)"
                                               .replace("%", "%%"))
        sp.add_argument("--blastdbcmd", default="blastdbcmd", help="blastdbcmd executable (not in the reference CLI)")
        sp.add_argument("--device", type=int, default=0, help="HIP device ordinal (not in the reference CLI)")
    cd = sub.add_parser("cache-db", help="binary cache of a *.blutils.json (pass it as --tax-file afterwards)")
    cd.add_argument("tax_file")
    cd.add_argument("cache_file")
    cd.add_argument("-u", "--use-taxid", action="store_true")
    return ap


def _u64(text: str) -> int:
    """clap's u64 value parser"""
    v = int(text)
    if not 0 <= v < (1 << 64):
        raise argparse.ArgumentTypeError(f"invalid u64: {text!r}")
    return v


def _threshold(text: str) -> float:
    """a float threshold of a hit filter: NaN compares false with everything and is refused"""
    v = float(text)
    if v != v:
        raise argparse.ArgumentTypeError("NaN is not a threshold")
    return v


def _length(text: str) -> int:
    """an alignment length: a non-negative integer"""
    v = int(text)
    if v < 0 or v >= (1 << 63):
        raise argparse.ArgumentTypeError(f"invalid length: {text!r}")
    return v


def _top_percent(text: str):
    """--top-percent: a decimal with at most three decimals in 0 .. 100, kept exact (decimal.Decimal)"""
    import decimal
    try:
        pipeline.top_percent_milli(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return decimal.Decimal(text.strip())


def _min_cover(text: str):
    """--min-cover: a decimal with at most three decimals, above 50 and at most 100, kept exact (decimal.Decimal)"""
    import decimal
    try:
        pipeline.min_cover_milli(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return decimal.Decimal(text.strip())


def _min_query_cover(text: str):
    """--min-query-cover: a decimal with at most three decimals in 0 .. 100, kept exact (decimal.Decimal)"""
    import decimal
    try:
        pipeline.min_query_cover_milli(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return decimal.Decimal(text.strip())


def _top_bits(text: str) -> int:
    """--top-bits: an integer in 0 .. 2^32 - 1"""
    try:
        return pipeline.top_bits_value(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _score_band(args):
    """the two flags -> pipeline.ScoreBand, or None when neither was given (today's calls)"""
    b = pipeline.ScoreBand(args.top_percent, args.top_bits)
    return b if b.active() else None


def _hit_filter(args):
    """the four flags -> pipeline.HitFilter, or None when none was given (today's calls)"""
    f = pipeline.HitFilter(args.min_perc_identity, args.min_align_length, args.max_e_value, args.min_bit_score)
    return f if f.active() else None


def _elements_file(path):
    """one element per line; blank lines and `#` comments skipped"""
    try:
        with open(path) as f:
            lines = [l.strip() for l in f]
    except OSError as e:
        raise SystemExit(f"cannot read {path}: {e.strerror}")
    return [l for l in lines if l and not l.startswith("#")]


def _taxon_filter(args):
    """the four flags -> pipeline.TaxonFilter (flag elements first, then the file's), or None when none was given"""
    exclude, only = list(args.exclude_taxon), list(args.only_taxon)
    if args.exclude_taxon_file:
        exclude += _elements_file(args.exclude_taxon_file)
    if args.only_taxon_file:
        only += _elements_file(args.only_taxon_file)
    f = pipeline.TaxonFilter(tuple(exclude), tuple(only))
    return f if f.active() else None


def _say_kept(stats, hit_filter=True) -> None:
    t = stats.get("taxon_filter") if stats else None
    if t:
        print(f"taxon filter: excluded {t['n_excluded']}, not in --only-taxon {t['n_not_only']}, of {t['n_lines']} lines",
              file=sys.stderr)
        for el, count in zip(t["exclude"], t["excluded_by"]):
            if count:
                print(f"  {el}: {count}", file=sys.stderr)
    q = stats.get("query_cover") if stats else None
    if q:
        print(f"query cover: {q['n_below']} of {q['n_lines']} lines under {q['percent']} percent (from {q['source']})", file=sys.stderr)
    if (hit_filter or q) and stats and "n_kept" in stats:
        print(f"hit filter: kept {stats['n_kept']} of {stats['n_lines']} lines", file=sys.stderr)
    s = stats.get("subject_best") if stats else None
    if s:
        print(f"subject best hit: kept {s['n_kept']} of {s['n_hits']} lines, thinned {s['n_thinned']} of {s['n_queries']} queries",
              file=sys.stderr)
    b = stats.get("score_band") if stats else None
    if b:
        print(f"score band: raised {b['n_raised']} of {b['n_hits']} lines in {b['n_widened']} of {b['n_queries']} queries",
              file=sys.stderr)
    c = stats.get("min_cover") if stats else None
    if c:
        print(f"min cover: kept {c['n_kept']} of {c['n_hits']} lines, narrowed {c['n_narrowed']} of {c['n_queries']} queries, "
              f"{c['n_unresolved']} left alone", file=sys.stderr)
    t = stats.get("count_table") if stats else None
    if t:
        print(report.count_table_line(t), file=sys.stderr)


def _check_count_table(args) -> None:
    """--count-table needs a file that uses it, and brings its own counts"""
    if args.count_table is None:
        return
    if args.report is None and args.sample_table is None:
        raise SystemExit("--count-table needs --report or --sample-table")
    if args.report_weight == "size":
        raise SystemExit("--count-table cannot be combined with --report-weight size: the counts are the table's")


def _depth(text: str) -> int:
    """argparse type of --rarefy: a whole number of reads, 1 .. 2^64 - 1"""
    v = int(text)
    if not 1 <= v < 2 ** 64:
        raise argparse.ArgumentTypeError("the depth is a whole number of reads, 1 or more")
    return v


def _seed(text: str) -> int:
    """argparse type of --seed: 0 .. 2^64 - 1"""
    v = int(text)
    if not 0 <= v < 2 ** 64:
        raise argparse.ArgumentTypeError("the seed is a whole number, 0 .. 2^64 - 1")
    return v


def _depths(text: str) -> list:
    """argparse type of --depths: D1,D2,... strictly ascending, 1 .. 32 of them"""
    try:
        v = [_depth(t) for t in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("the depths are whole numbers of reads separated by commas")
    if len(v) > _native.ALPHA_MAX_DEPTHS:
        raise argparse.ArgumentTypeError(f"at most {_native.ALPHA_MAX_DEPTHS} depths")
    if any(a >= b for a, b in zip(v, v[1:])):
        raise argparse.ArgumentTypeError("the depths ascend strictly")
    return v


def _steps(text: str) -> int:
    """argparse type of --steps: 1 .. 32"""
    v = int(text)
    if not 1 <= v <= _native.ALPHA_MAX_DEPTHS:
        raise argparse.ArgumentTypeError(f"the steps are a whole number, 1 .. {_native.ALPHA_MAX_DEPTHS}")
    return v


def _check_alpha_flags(ap, args, table) -> None:
    """--alpha-table needs the table it reads; its companions need it, and the seed needs a ladder"""
    needs = "--by-sample and -o" if args.sub == "build-report" else "--sample-table"
    others = (args.alpha_rank, args.alpha_depths, args.alpha_steps, args.alpha_seed)
    if args.alpha_table is None:
        if any(v is not None for v in others):
            ap.error("--alpha-rank, --alpha-depths, --alpha-steps and --alpha-seed need --alpha-table")
        return
    if table is None:
        ap.error(f"--alpha-table needs {needs}: it reads the table that flag writes")
    if args.alpha_depths is not None and args.alpha_steps is not None:
        ap.error("--alpha-depths and --alpha-steps: one or the other")
    if args.alpha_seed is not None and args.alpha_depths is None and args.alpha_steps is None:
        ap.error("--alpha-seed needs --alpha-depths or --alpha-steps")


def _diversity(table, out, rank, drop, device, depths, steps, max_depth, seed) -> None:
    try:
        st = diversity.build_diversity(table, out, rank, drop, device, depths, steps, max_depth, seed)
    except _native.BluError as e:
        raise SystemExit(str(e))
    print("\n".join(diversity.summary(st)), file=sys.stderr)


def _alpha_table(args, table, device=0) -> None:
    """the alpha diversity of the table just written (after every other output)"""
    if args.alpha_table is not None:
        _diversity(table, args.alpha_table, args.alpha_rank, False, device, args.alpha_depths, args.alpha_steps, None, args.alpha_seed)


def _rarefy_kwargs(depth, seed, table) -> dict:
    """build_distances' keyword arguments of a rarefaction; none without a depth, so that the call is the one it was"""
    return {} if depth is None else {"rarefy": depth, "seed": seed or 0, "rarefied_table": table}


def _check_distance_flags(ap, args, table) -> None:
    """--distance-matrix needs the table it reads; its companions need it, and the rarefaction's need --distance-rarefy"""
    needs = "--by-sample and -o" if args.sub == "build-report" else "--sample-table"
    rarefy = (args.distance_rarefy, args.distance_seed, args.distance_rarefied_table)
    if args.distance_matrix is None:
        if args.distance_rank is not None or args.distance_metric is not None:
            ap.error("--distance-rank and --distance-metric need --distance-matrix")
        if any(v is not None for v in rarefy):
            ap.error("--distance-rarefy, --distance-seed and --distance-rarefied-table need --distance-matrix")
        return
    if table is None:
        ap.error(f"--distance-matrix needs {needs}: it reads the table that flag writes")
    if args.distance_rarefy is None and any(v is not None for v in rarefy):
        ap.error("--distance-seed and --distance-rarefied-table need --distance-rarefy")


def _distance_matrix(args, table, device=0) -> None:
    """the matrix of the table just written (after every other output)"""
    if args.distance_matrix is None:
        return
    try:
        st = distance.build_distances(table, args.distance_matrix, args.distance_rank, args.distance_metric or "bray-curtis",
                                      device=device, **_rarefy_kwargs(args.distance_rarefy, args.distance_seed, args.distance_rarefied_table))
    except _native.BluError as e:
        raise SystemExit(str(e))
    print("\n".join([distance.summary(st)] + distance.rarefy_summary(st)), file=sys.stderr)


def _build_db(args) -> int:
    """ports/cli/src/cmds/db_builder/mod.rs:12-44"""
    try:
        if args.sub == "kraken2":
            seqdb.build_kraken_db_from_ncbi_files(args.blast_database_path, args.output_directory, args.listing_file,
                                                  args.blastdbcmd, device=args.device)
            return 0
        if args.sub == "qiime2":
            seqdb.build_qiime_db_from_blutils_db(args.taxonomies_database_path, args.output_taxonomies_file,
                                                 args.blast_database_path, args.output_sequences_file, args.use_taxid,
                                                 args.listing_file, args.blastdbcmd, device=args.device)
            return 0
        if args.sub in ("sintax", "dada2"):
            build = seqdb.build_sintax_db_from_blutils_db if args.sub == "sintax" else seqdb.build_dada2_db_from_blutils_db
            st = build(args.taxonomies_database_path, args.blast_database_path, args.output_sequences_file, args.use_taxid,
                       args.listing_file, args.blastdbcmd, device=args.device)
            print(f"labelled export: wrote {st['n_lines'] - st['n_unknown_taxid'] - st['n_unlabelled']} of {st['n_lines']} lines, "
                  f"{st['n_unknown_taxid']} with a taxid not in the taxonomies file, {st['n_unlabelled']} without a label",
                  file=sys.stderr)
            return 0
        if args.sub == "lineages":
            st = lineagedb.build_ref_db_from_lineage_table(args.table, args.output_file_path, args.taxid_map,
                                                           lineagedb.parse_replace_rank(args.replace_rank), args.device)
            print(lineagedb.summary(st), file=sys.stderr)
            return 0
        replace = taxdb.parse_replace_rank(args.replace_rank)
        taxdb.build_ref_db_from_ncbi_files(args.blast_database_path, args.taxdump_directory_path, args.output_file_path,
                                           args.skip_taxid, replace, args.drop_non_linnaean_taxonomies,
                                           args.accessions_file, args.blastdbcmd, args.device)
    except (taxdb.TaxdbError, blast.BlastError, seqdb.SeqdbError, lineagedb.LineageDbError) as e:
        raise SystemExit(str(e))
    return 0


def _run_with_consensus(ap, args) -> int:
    """ports/cli/src/cmds/blast/mod.rs:24-102"""
    config = blast.BlastBuilder.default(args.database, args.taxon)
    if args.max_target_seqs is not None:
        config = config.with_max_target_seqs(args.max_target_seqs)
    if args.perc_identity is not None:
        config = config.with_perc_identity(args.perc_identity)
    if args.query_cov is not None:
        config = config.with_query_cov(args.query_cov)
    if args.strand is not None:
        config = config.with_strand(args.strand)
    if args.e_value is not None:
        config = config.with_e_value(args.e_value)
    if args.word_size is not None:
        config = config.with_word_size(args.word_size)
    custom = None
    if args.custom_taxon_cutoff_file:
        custom = pipeline.custom_taxon_from_file(args.custom_taxon_cutoff_file)
    elif args.taxon == "custom":
        raise SystemExit("Custom taxon values are required when the custom taxon option is selected.")
    stats = {}
    hit_filter, taxon_filter = _hit_filter(args), _taxon_filter(args)
    _check_count_table(args)
    _check_distance_flags(ap, args, args.sample_table)
    _check_alpha_flags(ap, args, args.sample_table)
    try:
        blast.run_blast_and_build_consensus(args.query, args.tax_file, args.blast_out_file, args.blutils_out_file, config,
                                            blast.ExecuteBlastnProcRepository(args.blastn), args.force_overwrite,
                                            args.threads, args.strategy, args.use_taxid, args.out_format, custom,
                                            device=args.device, report_path=args.report, report_weight=args.report_weight,
                                            sample_table_path=args.sample_table, hit_filter=hit_filter,
                                            filter_stats=stats, support_table_path=args.support_table,
                                            taxon_filter=taxon_filter, score_band=_score_band(args),
                                            **({"best_hit_per_subject": True} if args.best_hit_per_subject else {}),
                                            **({"min_cover": args.min_cover} if args.min_cover is not None else {}),
                                            **({"count_table": args.count_table} if args.count_table is not None else {}))
    except blast.BlastError as e:
        raise SystemExit(str(e))
    except _native.BluError as e:
        if taxon_filter is None:
            raise
        raise SystemExit(str(e))                                                       # (an unknown element: the library's message)
    _say_kept(stats, hit_filter is not None)
    _distance_matrix(args, args.sample_table, args.device)
    _alpha_table(args, args.sample_table, args.device)
    return 0


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.cmd == "build-db":
        return _build_db(args)
    if args.cmd == "cache-db":
        pipeline.build_db_cache(args.tax_file, args.cache_file, args.use_taxid)
        return 0
    if args.sub == "build-tabular":
        try:
            tabular.parse_consensus_as_tabular(args.blu_result, args.output_file, args.input_format)
        except tabular.TabularError as e:
            raise SystemExit(str(e))
        return 0
    if args.sub == "build-distances":
        if args.rarefy is None and (args.seed is not None or args.rarefied_table is not None):
            ap.error("--seed and --rarefied-table need --rarefy")
        try:
            st = distance.build_distances(args.table, args.output_file, args.rank, args.metric, args.drop_unclassified, args.device,
                                          **_rarefy_kwargs(args.rarefy, args.seed, args.rarefied_table))
        except _native.BluError as e:
            raise SystemExit(str(e))
        print("\n".join([distance.summary(st)] + distance.rarefy_summary(st)), file=sys.stderr)
        return 0
    if args.sub == "build-diversity":
        if args.depths is not None and args.steps is not None:
            ap.error("--depths and --steps: one or the other")
        if args.max_depth is not None and args.steps is None:
            ap.error("--max-depth needs --steps")
        if args.seed is not None and args.depths is None and args.steps is None:
            ap.error("--seed needs a ladder: --depths or --steps")
        _diversity(args.table, args.output_file, args.rank, args.drop_unclassified, args.device, args.depths, args.steps, args.max_depth,
                   args.seed)
        return 0
    if args.sub == "build-report":
        _check_distance_flags(ap, args, args.output_file if args.by_sample else None)
        _check_alpha_flags(ap, args, args.output_file if args.by_sample else None)
        try:
            if args.count_table is not None and args.weight == "size":
                raise SystemExit("--count-table cannot be combined with --weight size: the counts are the table's")
            st = {}
            report.build_report(args.blu_result, args.output_file, args.input_format, args.weight, by_sample=args.by_sample,
                                **({"count_table": args.count_table, "count_stats": st} if args.count_table is not None else {}))
            if st:
                print(report.count_table_line(st), file=sys.stderr)
        except (tabular.TabularError, report.ReportError) as e:
            raise SystemExit(str(e))
        _distance_matrix(args, args.output_file)
        _alpha_table(args, args.output_file)
        return 0
    if args.sub == "run-with-consensus":
        return _run_with_consensus(ap, args)
    custom = None
    if args.custom_taxon_cutoff_file:
        custom = pipeline.custom_taxon_from_file(args.custom_taxon_cutoff_file)        # CustomTaxon::from_file
    elif args.taxon == "custom":
        # cmds/blast/mod.rs:114-117
        raise SystemExit("Custom taxon values are required when the custom taxon option is selected.")
    to_file = args.blutils_out_file is not None
    fmt = args.out_format if (to_file or args.out_format != "json") else "json-compact"
    # (with --report: the same document, plus the report file)
    build = pipeline.build_consensus_identities
    hit_filter = _hit_filter(args)
    extra = {"hit_filter": hit_filter} if hit_filter is not None else {}
    taxon_filter = _taxon_filter(args)
    if taxon_filter is not None:
        extra["taxon_filter"] = taxon_filter
    score_band = _score_band(args)
    if score_band is not None:
        extra["score_band"] = score_band
    if args.best_hit_per_subject:
        extra["best_hit_per_subject"] = True
    if args.min_cover is not None:
        extra["min_cover"] = args.min_cover
    _check_count_table(args)
    _check_distance_flags(ap, args, args.sample_table)
    _check_alpha_flags(ap, args, args.sample_table)
    if args.count_table is not None:
        extra["count_table"] = args.count_table
    if args.blast_outfmt is not None:
        try:
            layout = pipeline.table_layout(args.blast_outfmt)
        except _native.BluError:
            raise SystemExit(f"--blast-outfmt: {_native.last_error()}")
        if layout.e_value == pipeline.TABLE_LAYOUT_NO_COLUMN and args.max_e_value is not None:
            raise SystemExit("--blast-outfmt: --max-e-value needs an `evalue` column and SPEC names none")
        extra["blast_outfmt"] = layout
    if args.min_query_cover is not None:
        if args.blast_outfmt is None:
            raise SystemExit("--min-query-cover needs --blast-outfmt: the reference's thirteen columns hold no query length, so the "
                             "table's columns have to be named (e.g. --blast-outfmt \"6 std staxids qlen\")")
        try:
            pipeline.query_cover_columns(args.blast_outfmt, args.query_cover_from)
        except _native.BluError:
            raise SystemExit(f"--min-query-cover: {_native.last_error()}")
        extra["blast_outfmt"] = args.blast_outfmt
        extra["query_cover"] = pipeline.QueryCover(args.min_query_cover, args.query_cover_from)
    elif args.query_cover_from != "auto":
        raise SystemExit("--query-cover-from needs --min-query-cover")
    if args.support_table is not None:
        build = functools.partial(pipeline.build_consensus_identities_with_tables, report_path=args.report,
                                  sample_table_path=args.sample_table, report_weight=args.report_weight,
                                  support_table_path=args.support_table)
    elif args.sample_table is not None:
        build = functools.partial(pipeline.build_consensus_identities_with_tables, report_path=args.report,
                                  sample_table_path=args.sample_table, report_weight=args.report_weight)
    elif args.report is not None:
        build = functools.partial(pipeline.build_consensus_identities_with_report, report_path=args.report,
                                  report_weight=args.report_weight)
    try:
        if to_file:
            path = os.path.splitext(args.blutils_out_file)[0] + "." + args.out_format      # PathBuf::set_extension
            parent = os.path.dirname(path)
            if parent and not os.path.exists(parent):
                os.makedirs(parent)
            _, stats = build(args.blast_out, args.tax_file, args.taxon, args.strategy, args.use_taxid, custom, headers=None,
                             out_format=fmt, device=args.device, parse=False, out_path=path, **extra)
        else:
            text, stats = build(args.blast_out, args.tax_file, args.taxon, args.strategy, args.use_taxid, custom, headers=None,
                                out_format=fmt, device=args.device, parse=False, **extra)
            sys.stdout.write(text)
    except _native.BluError as e:
        if taxon_filter is None:
            raise
        raise SystemExit(str(e))                                                       # (an unknown element: the library's message)
    _say_kept(stats, hit_filter is not None)
    _distance_matrix(args, args.sample_table, args.device)
    _alpha_table(args, args.sample_table, args.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
