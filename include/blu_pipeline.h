/*
 * blu_pipeline.h — host-side drop-in for blutils' `build_consensus_identities`
 * use-case and the result writer behind `blu blastn build-consensus`.
 *
 * Reference entry points mirrored (same arguments, same meaning):
 *   core/src/use_cases/build_consensus_identities/mod.rs:40-47
 *     build_consensus_identities(blast_output: ParallelBlastOutput{output_file, headers},
 *                                taxonomies_file, taxon, strategy, use_taxid, custom_taxon_values)
 *   core/src/use_cases/write_blutils_output.rs:33-38
 *     write_blutils_output(results, config, blutils_out_file, out_format)
 *
 * What runs where: text ingest (outfmt-6 TSV, blutils DB JSON), lineage
 * interning, the taxid join and the per-query grouping are host C++; the
 * per-query consensus itself is the HIP engine (blu_consensus_run); strings and
 * consensus beans are rebuilt on the host from the 32-byte records.
 */
#ifndef BLU_PIPELINE_H
#define BLU_PIPELINE_H

#include <stddef.h>
#include <stdint.h>

#include "blu_consensus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* write_blutils_output.rs:20-31 OutputFormat */
enum blu_out_format { BLU_OUT_JSON = 0, BLU_OUT_JSONL = 1, BLU_OUT_YAML = 2,
                      BLU_OUT_JSON_COMPACT = 3 /* serde_json::to_writer: what the CLI prints to stdout (:152-163) */ };

typedef struct blu_pipeline_params {
    blu_cutoff_config cutoffs;   /* taxon + Option<CustomTaxon> */
    int32_t strategy;            /* enum blu_strategy */
    int32_t use_taxid;           /* Option<bool>: != 0 -> numericLineage, else textLineage (mod.rs:287-291) */
    int32_t device;              /* HIP device ordinal */
    int32_t out_format;          /* enum blu_out_format */
    int32_t lenient;             /* 0: a query that makes the reference panic fails the call (BLU_ERR_REFERENCE_PANIC),
                                    like the reference aborts; 1: such queries are written with "taxon": null */
    int32_t reserved;
} blu_pipeline_params;

#define BLU_ERR_REFERENCE_PANIC 9 /* a per-query condition on which the reference panics (see blu_status >= 16) */

typedef struct blu_pipeline_stats {
    uint64_t n_hits, n_queries, n_taxids, n_unmatched_rows;
    double t_load_db_s, t_load_hits_s, t_engine_s, t_render_s;
} blu_pipeline_stats;

/* Hit filters (not in the reference): thresholds on four columns of the table, applied by the parser.  A line
 * is kept when every threshold named in `mask` holds, as IEEE comparisons (a NaN fails):
 *   BLU_FILTER_MIN_PERC_IDENTITY  column 3  perc_identity >= min_perc_identity
 *   BLU_FILTER_MIN_ALIGN_LENGTH   column 4  align_length  >= min_align_length
 *   BLU_FILTER_MAX_E_VALUE        column 11 e_value       <= max_e_value
 *   BLU_FILTER_MIN_BIT_SCORE      column 12 bit_score as written (before its truncation) >= min_bit_score
 * The result is what the unfiltered call gives on a copy of the table without the dropped lines: queries numbered by their
 * first kept line, accession ranks over the kept accessions, n_unmatched_rows over kept lines; a query that keeps no line
 * is not in the table.  Every line is validated as without a filter, kept or not.  Column 11 is read — as an f64 column:
 * a field that is no number is BLU_ERR_PARSE naming the line — only under BLU_FILTER_MAX_E_VALUE.  A NULL filter or an
 * empty mask is the unfiltered call. */
#define BLU_FILTER_MIN_PERC_IDENTITY 1u
#define BLU_FILTER_MIN_ALIGN_LENGTH 2u
#define BLU_FILTER_MAX_E_VALUE 4u
#define BLU_FILTER_MIN_BIT_SCORE 8u
typedef struct blu_hit_filter {
    double min_perc_identity;
    int64_t min_align_length;
    double max_e_value;
    double min_bit_score;
    uint32_t mask;                 /* BLU_FILTER_* bits: which of the four are active */
    uint32_t reserved;
} blu_hit_filter;
typedef struct blu_hit_filter_stats {
    uint64_t n_lines;              /* non-empty lines of the table */
    uint64_t n_kept;               /* lines kept by the hit and the taxon filter together (= n_lines without either) */
} blu_hit_filter_stats;

/* Taxon filters (not in the reference): lines are dropped by the lineage of their subject, in the parser, so
 * that hits to uninformative or out-of-scope taxa do not take part.  An element is spelled `RANK__IDENTIFIER` as it appears in
 * the lineage flavour of the run (textLineage, or numericLineage under use_taxid): split at `__` into exactly two non-empty
 * parts; the rank goes through the normalisation lineage ranks go through (lower-cased, `species__x` is `s__x`); an identifier
 * that ends in `*` is a prefix pattern over the identifiers of that rank (`s__uncultured-*`; a lone `*` is every identifier of
 * the rank) and counts as one element.  An element or pattern that names no node of a lineage of the taxonomies file is
 * BLU_ERR_INVALID_ARG naming it; so are more than BLU_TAXON_FILTER_MAX_EXCLUDE exclude elements.
 * The elements of a line are the nodes of the lineage of the taxonomy row its column 3 joins to (the first listing of a taxid
 * listed more than once); a line whose taxid is not in the file, or whose row's lineage is bad or empty, has none.  A line
 * passes when none of its elements is on `exclude` and, if `only` is not empty, at least one is on `only`.  The verdict comes
 * before the thresholds of a blu_hit_filter given alongside and does not depend on them; a line is kept when it passes and
 * every threshold holds, and the result is what the call without filters gives on a copy of the table without the other lines
 * (as under blu_hit_filter, above).  A NULL filter or two empty lists is the call without it. */
#define BLU_TAXON_FILTER_MAX_EXCLUDE 65534u
typedef struct blu_taxon_filter {
    const char* const* exclude; uint64_t n_exclude;
    const char* const* only; uint64_t n_only;
} blu_taxon_filter;
typedef struct blu_taxon_filter_stats {
    uint64_t n_lines;              /* non-empty lines of the table */
    uint64_t n_excluded;           /* lines with an element on the exclude list, whatever the thresholds say */
    uint64_t n_not_only;           /* lines that pass the exclude list and have no element on the only list */
    uint64_t* excluded_by;         /* caller's [n_exclude], or NULL: lines whose first matching exclude element, in list order, is k */
} blu_taxon_filter_stats;

/* Which lines of the table take part, and with which score: the four options of DESIGN.md §14 and §16-§18, each NULL (or with
 * an empty mask / two empty lists) when not asked for.  They apply in this order, and each one's contract is stated on the
 * table the ones before it leave: */
typedef struct blu_hit_selection {
    const blu_hit_filter* hit_filter;       /* 1. with taxon_filter, in the parser: the lines both keep (above) */
    const blu_taxon_filter* taxon_filter;
    const blu_subject_best* subject_best;   /* 2. best hit per subject (include/blu_consensus.h): of the lines of
                                               one (query, subject accession) pair that the filters keep, the one with the highest
                                               truncated bit-score stays, the first in file order among equals; the others are
                                               dropped before the band and the engine run.  The run gives, byte for byte, what the run
                                               without the selection gives on a copy of the (filtered) table without the dropped
                                               lines: the document, the report, the sample table and the support table; the stats'
                                               n_hits and n_unmatched_rows are those of the copy.  Applied once per run on the device
                                               (csrc/subject_kernel.hip): on the columns the GPU ingest left there, or through the
                                               host-pointer route on host columns. */
    const blu_score_band* score_band;       /* 3. bit-score band (include/blu_consensus.h): the rows of a query whose
                                               truncated bit-score lies in the band under the query's top score are given the top
                                               score before the engine runs; the top is taken over the lines that 1 and 2 keep.  The
                                               run gives, byte for byte, what the run without a band gives on a copy of that table in
                                               which column 12 of every in-band line is the decimal text of its query's top score: the
                                               document, the report, the sample table and the support table, whose top_hits is then
                                               the band's size and whose bits / support_bits sum the raised scores.  Applied once per
                                               run on the device (csrc/band_kernel.hip), like 2.  top_percent_milli = 0 and
                                               top_bits = 0 give the bytes of the run without a band. */
} blu_hit_selection;
/* The counts of a selection; an option that was not asked for reports the table as it passed by (nothing dropped, nothing
 * raised), the taxon filter zeros.  Zeroed when the call begins — the caller's taxon_filter.excluded_by array [n_exclude] too, which is the one input
 * here: set the pointer (or NULL) before the call. */
typedef struct blu_hit_selection_stats {
    blu_hit_filter_stats hit_filter;         /* n_kept: lines kept by hit_filter and taxon_filter together */
    blu_taxon_filter_stats taxon_filter;
    blu_subject_best_stats subject_best;
    blu_score_band_stats score_band;
} blu_hit_selection_stats;

/* Weights of the report and the per-sample table: BLU_REPORT_WEIGHT_ONE counts results; BLU_REPORT_WEIGHT_SIZE counts the
 * dereplicated reads in the query name: the first ';'-field `size=<digits>`, else a `_size_<digits>` suffix, else 1 — a size
 * of 2^32 or more is BLU_ERR_INVALID_ARG naming the query. */
enum blu_report_weight { BLU_REPORT_WEIGHT_ONE = 0, BLU_REPORT_WEIGHT_SIZE = 1 };

/* One run of the use-case with everything it can write.  Set struct_size = sizeof(blu_consensus_request) and zero the rest
 * before filling in what is wanted: options are added at the end of the struct, so a caller compiled against an older header
 * keeps working and a size this library does not know is BLU_ERR_INVALID_ARG. */
typedef struct blu_consensus_request {
    uint32_t struct_size;
    uint32_t reserved;
    const char* blast_output_file;     /* ParallelBlastOutput.output_file: the outfmt-6 table */
    const char* const* headers;        /* Option<Vec<String>> of FASTA ids (NULL/0 = None): ids without a hit row become */
    uint64_t n_headers;                /*   NoConsensusFound entries (mod.rs:86-102) */
    const char* taxonomies_file;       /* the `*.blutils.json`, or its binary cache (blu_db_cache_build, below) */
    const blu_pipeline_params* params;
    const char* run_id_text;           /* Some(BlastBuilder) as `config` (run_blast_and_build_consensus/mod.rs:53-67): the config's
                                          run id (36 characters; NULL/"" = a fresh UUID v4 per call), which every result carries
                                          (write_blutils_output.rs:82-104) */
    const char* config_text;           /* the config already serialized for `out_format` at its place in the document (JSON: the
                                          value after "config": — for the pretty form with its inner lines indented by two spaces;
                                          JSONL: the first line; YAML: the block under `config:`), NULL/"" = null.
                                          blutils_amd/blast.py produces it. */
    const char* out_path;              /* the document is written straight there (no copy through the caller: what the CLI does
                                          with --blutils-out-file; an existing file is replaced); NULL: into the outcome's text */
    /* The three tables below are counted on the device from the run's records and written after the document, in this order;
     * the document is, byte for byte, what the request without them gives.  In strict mode a reference panic fails the call
     * before any file is written; so does a query without a sample under sample_table_path. */
    const char* report_path;           /* NULL: no report.  Taxon abundance report, tab-separated:
                                            #percent  clade  direct  rank  identifier  taxonomy        (header)
                                            pct  U  U  -  unclassified  (empty)   always; U = weight of the results with "taxon": null
                                                                                  (headers without hits too)
                                            pct  N  N  -  unplaced  (empty)       when N > 0: results whose taxonomy is ""
                                            one line per path, depth first; siblings by clade descending, then element text
                                            `rank__identifier` ascending (bytewise)
                                          percent = "%.2f" of 100.0 * clade / total (0.00 when total is 0). */
    const char* sample_table_path;     /* NULL: no per-sample table, tab-separated:
                                            #rank  identifier  taxonomy  total  <sample 1>  <sample 2> ...   (header; samples
                                                                                                              ascending bytewise)
                                            -  unclassified  (empty)  U  u1  u2 ...                          always
                                            -  unplaced  (empty)  N  n1  n2 ...                              when N > 0
                                            rank  identifier  taxonomy  clade  <clade in sample 1> ...       one line per path, in
                                                                                                              the report's order
                                          The sample of a query: the first ';'-field `sample=<one or more bytes>`; else, in the
                                          label (the name up to its first ';' with a trailing `_size_<digits>` removed), the part
                                          left of the last '.' when that part is non-empty and the part right of it is ASCII digits
                                          (vsearch --relabel `<sample>.<n>`).  A query (hit or header) with neither is
                                          BLU_ERR_INVALID_ARG naming it. */
    int32_t weight;                    /* enum blu_report_weight, for both files above; read only when one of them is asked for */
    int32_t min_cover_milli;           /* 0: not asked for.  Minimum cover (include/blu_consensus.h: blu_hits_cover_apply),
                                          the percentage times 1000, 50001 .. 100000; any other value is BLU_ERR_INVALID_ARG ("min
                                          cover: ...") before a file is opened.  The FOURTH step of the selection below, after the
                                          band and on the table steps 1 - 3 leave: of the rows on a query's top score — the band's
                                          rows included — those outside the deepest taxon that still covers that share of them are
                                          dropped before the engine runs.  The run gives, byte for byte, what the run with the same
                                          options before it gives on a copy of that table without the dropped lines: the document,
                                          the report, the sample table and the support table; the stats' n_hits and n_unmatched_rows
                                          are those of the copy.  100000 gives the bytes of the run without it.  Applied once per run
                                          on the device (csrc/cover_kernel.hip), like steps 2 and 3; its counts: blu_last_min_cover_stats.
                                          (The field took the place of a reserved word: neither struct here can grow.) */
    const char* support_table_path;    /* NULL: no per-query support table (not in the reference).  The counts come
                                          from the device (blu_consensus_support) — on the records and columns the run left there,
                                          or through the host-pointer route when the columns are on the host — over the lines the
                                          selection leaves, tab-separated:
                                            #query  rank  identifier  hits  matched  top_hits  top_support  support  bit_score  bits
                                            support_bits  confidence
                                          one line per result of the document, in the document's order (headers without hits
                                          included, every count zero).  rank and identifier: the last element of the result's
                                          `taxonomy`, as the report's rows have them; `-` and `unclassified` when `taxon` is null,
                                          `-` and `unplaced` when `taxonomy` is "".  The counts are blu_support's, in decimal;
                                          confidence is "%.4f" of support / hits (0.0000 without hits).  In lenient mode the
                                          queries of a reference panic are `unclassified` lines. */
    blu_hit_selection selection;       /* all NULL: every line takes part */
} blu_consensus_request;

/* What a run gives back.  text: out_path == NULL: a malloc'd buffer with the serialized results (free with blu_free_text),
 * sorted by query (write_blutils_output.rs:111), in `out_format`:
 *   JSON : {"results":[QueryWithConsensus...],"config":null} pretty-printed like serde_json::to_string_pretty
 *   JSON_COMPACT: the same document on one line
 *   JSONL: the config line (`null` without a config_text) then one QueryWithConsensus per line
 *   YAML : block style as serde_yaml 0.9 emits BlutilsOutput (scalar quoting rules of the third-party emitter are
 *          approximated: parity unpinned there)
 * With an out_path, and after a failure, text is NULL and text_len 0.  The whole outcome is zeroed when the call begins,
 * selection.taxon_filter.excluded_by aside (blu_hit_selection_stats, above). */
typedef struct blu_consensus_outcome {
    char* text;
    size_t text_len;
    blu_pipeline_stats stats;
    blu_hit_selection_stats selection;
} blu_consensus_outcome;

int blu_build_consensus(const blu_consensus_request* request, blu_consensus_outcome* outcome);
void blu_free_text(char* text);

/* Options the request above has no room for (its size is pinned).  Set struct_size = sizeof(blu_consensus_extras) and zero the
 * rest: options are added at the end; a size the library does not know is BLU_ERR_INVALID_ARG.
 *
 * count_table_path: a feature x sample count table (vsearch --otutabout, usearch -otutab, biom convert
 * --to-tsv), tab-separated.  Blank lines are skipped; leading lines that start with '#' and hold no tab are comments; the first
 * other line is the header: its first cell is ignored, every further cell a sample name (non-empty, unique, at least one).
 * Every later line: a row name, then one cell per sample — ASCII digits, optionally '.' and only zeros, value < 2^32.  Anything
 * else is BLU_ERR_PARSE naming line and column.  "\r\n" line ends are accepted.  Rows and queries (with hits or header-only)
 * are joined on their names up to the first ';': two rows or two queries with one key, or a query no row has, are
 * BLU_ERR_INVALID_ARG naming them; a row no query has counts as unclassified.  With a table the report weighs a query by its
 * row sum (2^32 or more: BLU_ERR_INVALID_ARG naming the row) and the sample table's columns are all samples of the header
 * (ascending bytewise), a query adding its count in sample s to column s.  It needs report_path or sample_table_path and weight
 * BLU_REPORT_WEIGHT_ONE (else BLU_ERR_INVALID_ARG); the document and the support table are not touched by it.  All refusals
 * come before any file is written. */
typedef struct blu_count_table_stats { uint64_t n_rows, n_samples, n_joined, n_rows_unclassified; } blu_count_table_stats;
typedef struct blu_consensus_extras {
    uint32_t struct_size; uint32_t reserved;    /* options are added at the end; a size the library does not know is INVALID_ARG */
    const char* count_table_path;               /* NULL: none */
    blu_count_table_stats* count_table_stats;   /* caller's, or NULL; zeroed when the call begins */
} blu_consensus_extras;
/* blu_build_consensus(request, outcome) is blu_build_consensus_with(request, NULL, outcome). */
int blu_build_consensus_with(const blu_consensus_request* request, const blu_consensus_extras* extras /* NULL = none */,
                             blu_consensus_outcome* outcome);

/* The column layout of the table (not in the reference), for tables written with another `-outfmt "6 ..."` list
 * than the reference's `6 qseqid saccver staxid pident length mismatch gapopen qstart qend sstart send evalue bitscore`.  Both
 * parsers read the seven role fields through it; the typing rules (Int64 / f64), quote stripping, CR LF, the open last line,
 * blank lines and the left join are those of the reference's columns and apply to whichever field holds the role.  A line with
 * fewer than n_columns fields is BLU_ERR_PARSE naming the line and n_columns; further fields are ignored.  The run gives, byte
 * for byte, what it gives on a copy of the table rewritten to the reference's thirteen columns (the role fields copied as their
 * bytes, a `staxids` field cut at its first ';').  Set struct_size = sizeof(blu_table_layout); a size the library does not know
 * is BLU_ERR_INVALID_ARG, and so are a column count outside 1 .. BLU_TABLE_LAYOUT_MAX_COLUMNS, a role column at or beyond
 * n_columns and two roles in one column. */
#define BLU_TABLE_LAYOUT_MAX_COLUMNS 64u
#define BLU_TABLE_LAYOUT_NO_COLUMN 0xFFFFFFFFu
typedef struct blu_table_layout {
    uint32_t struct_size;
    uint32_t n_columns;            /* fields a line must have, 1 .. BLU_TABLE_LAYOUT_MAX_COLUMNS */
    uint32_t query;                /* 0-based column of each role: qseqid, else qacc, else qaccver */
    uint32_t accession;            /*   saccver, else sacc, else sseqid */
    uint32_t taxid;                /*   staxid, else staxids */
    uint32_t perc_identity;        /*   pident */
    uint32_t align_length;         /*   length */
    uint32_t bit_score;            /*   bitscore */
    uint32_t e_value;              /*   evalue, or BLU_TABLE_LAYOUT_NO_COLUMN: BLU_FILTER_MAX_E_VALUE is then BLU_ERR_INVALID_ARG */
    uint32_t taxid_is_list;        /* 1: the taxid column is `staxids`: the digits before its first ';' are the taxid (read by the
                                      Int64 rules: an empty prefix or `N/A` is BLU_ERR_PARSE); the bytes behind it are not read */
} blu_table_layout;
/* BLAST's own format string -> the layout.  Specifiers are separated by blanks; an optional leading `6` is ignored and any
 * other leading number refused; `std` stands for `qseqid sseqid pident length mismatch gapopen qstart qend sstart send evalue
 * bitscore`; at most BLU_TABLE_LAYOUT_MAX_COLUMNS columns after that expansion; a specifier named twice is refused; any other
 * token of [A-Za-z0-9_]+ is a column nobody reads.  Every role but e_value must be present.  Set out->struct_size before the
 * call.  Each refusal is BLU_ERR_INVALID_ARG with a message that names the offending token. */
int blu_table_layout_parse(const char* spec, blu_table_layout* out);
/* blu_build_consensus_with under a layout (NULL, or the reference's thirteen columns in the reference's order: the call without
 * one — the same parser builds, the same bytes). */
int blu_build_consensus_laid_out(const blu_consensus_request* request, const blu_consensus_extras* extras /* NULL = none */,
                                 const blu_table_layout* layout /* NULL = the reference's columns */, blu_consensus_outcome* outcome);

/* Query coverage (not in the reference, whose `-q` goes to blastn itself): a fifth threshold of the parser's
 * keep word, on columns the thirteen of the reference do not hold, so it needs a layout that names them.  A line is kept iff
 *   BLU_QUERY_COVER_QCOVHSP / _QCOVS  c * 1000 >= min_cover_milli, c the integer of `cover_column` (BLAST's rounded percent: per
 *                                     HSP, or — the coarser figure — per subject over all HSPs of the pair)
 *   BLU_QUERY_COVER_QLEN              (|qend - qstart| + 1) * 100000 >= min_cover_milli * qlen: the exact ratio, not BLAST's
 *                                     rounded percent; a span longer than qlen passes
 * in 64-bit integers (both sides stay below 2^48).  The fields are read only under a cover, by the Int64 rules of `length`; one
 * that does not parse, a value outside 0 .. 2^31 - 1 and qlen = 0 are BLU_ERR_PARSE naming the line, on every line, kept or not.
 * The taxon verdict comes first and is counted as without a cover; a line that fails the cover never has its e-value decided.
 * The run gives, byte for byte, what it gives without the cover on a copy of the table (same layout) from which the failing lines
 * were deleted; min_cover_milli = 0 keeps every line (the fields are still validated).  hit_filter.n_lines / n_kept of the
 * selection's stats then count lines as under a hit filter.  Refused with BLU_ERR_INVALID_ARG before any file is opened: a
 * struct_size the library does not know, a source that is not one of the three resolved ones, min_cover_milli > 100000, a cover
 * without a layout, a column the source reads at or beyond the layout's n_columns, on one of the seven roles, or named twice. */
enum blu_query_cover_source { BLU_QUERY_COVER_AUTO = 0,      /* blu_query_cover_parse only: qcovhsp, else the qlen form, else qcovs */
                              BLU_QUERY_COVER_QCOVHSP = 1, BLU_QUERY_COVER_QLEN = 2, BLU_QUERY_COVER_QCOVS = 3 };
#define BLU_QUERY_COVER_MAX_MILLI 100000u
typedef struct blu_query_cover_stats {
    uint64_t n_lines;              /* non-empty lines of the table */
    uint64_t n_below;              /* of them: coverage below the threshold, whatever the other filters say about the line */
} blu_query_cover_stats;
typedef struct blu_query_cover {
    uint32_t struct_size;
    uint32_t source;               /* enum blu_query_cover_source, resolved */
    uint32_t min_cover_milli;      /* the percentage times 1000, 0 .. BLU_QUERY_COVER_MAX_MILLI */
    uint32_t cover_column;         /* QCOVHSP / QCOVS: the 0-based column; else BLU_TABLE_LAYOUT_NO_COLUMN */
    uint32_t qstart, qend, qlen;   /* QLEN: the three columns; else BLU_TABLE_LAYOUT_NO_COLUMN */
    uint32_t reserved;
    blu_query_cover_stats* stats;  /* caller's, or NULL; zeroed when the call begins */
} blu_query_cover;
/* The format string (blu_table_layout_parse's tokenising and refusals) and a source -> the columns.  BLU_QUERY_COVER_AUTO takes
 * `qcovhsp`, else `qstart qend qlen`, else `qcovs`; an explicit source — or AUTO — whose specifiers the string lacks is
 * BLU_ERR_INVALID_ARG with a message that names the missing ones.  Set out->struct_size before the call; min_cover_milli and
 * stats are left as the caller set them. */
int blu_query_cover_parse(const char* spec, uint32_t source, blu_query_cover* out);
/* blu_build_consensus_laid_out under a cover (NULL: that call). */
int blu_build_consensus_covered(const blu_consensus_request* request, const blu_consensus_extras* extras /* NULL = none */,
                                const blu_table_layout* layout, const blu_query_cover* cover /* NULL = none */,
                                blu_consensus_outcome* outcome);

/* The reference's own three signatures, each the request above with the named fields set and the rest zero
 * (mod.rs:40-47 + write_blutils_output.rs:33-38 with config = None; the same with Some(BlastBuilder); the same to a file).
 * out_len and stats may be NULL. */
int blu_build_consensus_identities(const char* blast_output_file, const char* const* headers, uint64_t n_headers,
                                   const char* taxonomies_file, const blu_pipeline_params* params, char** out_text,
                                   size_t* out_len, blu_pipeline_stats* stats);
int blu_build_consensus_identities_cfg(const char* blast_output_file, const char* const* headers, uint64_t n_headers,
                                       const char* taxonomies_file, const blu_pipeline_params* params,
                                       const char* run_id_text, const char* config_text, char** out_text, size_t* out_len,
                                       blu_pipeline_stats* stats);
int blu_build_consensus_identities_to_file(const char* blast_output_file, const char* const* headers, uint64_t n_headers,
                                           const char* taxonomies_file, const blu_pipeline_params* params,
                                           const char* run_id_text, const char* config_text, const char* out_path,
                                           blu_pipeline_stats* stats);

/* The text-ingest half alone (no GPU): DB JSON + outfmt-6 TSV -> SoA columns, as blu_build_consensus does it.
 * Fills stats (rows, queries, taxids, unmatched rows, load times) and *checksum with an FNV-1a hash over every SoA
 * column, the segment offsets and the query names — identical for any BLU_INGEST_THREADS value.  For tests and for
 * timing the ingest (rows/s) apart from the engine. */
int blu_ingest_only(const char* blast_output_file, const char* taxonomies_file, int use_taxid, blu_pipeline_stats* stats,
                    uint64_t* checksum);
/* The same on HIP device `device` (>= 0): the table is parsed by the GPU ingest (csrc/ingest_gpu.hip) when it is in the
 * plain form BLAST writes, by the CPU otherwise; the columns — and the checksum — are identical either way.
 * BLU_INGEST=cpu|gpu in the environment forces one of the two (gpu also for files under 1 MiB). */
int blu_ingest_only_on(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                       blu_pipeline_stats* stats, uint64_t* checksum);

/* The columns themselves (what blu_ingest_only[_on] hashes), for a caller that wants the SoA table and for tests that
 * compare the parsers column by column with an independent reading of the file.  Every array is malloc'd by the library
 * and released by blu_ingest_columns_free; query_names / accessions are the strings back to back, each NUL-terminated
 * (queries in first-appearance order, accessions in byte order = acc_rank order).  A name that itself holds a NUL byte
 * cannot be told from two names in these tables: n_queries / n_accessions, the byte counts and the checksum of
 * blu_ingest_only still count it as one. */
typedef struct blu_ingest_columns {
    uint64_t n_hits, n_queries, n_accessions;
    uint64_t* seg_off;        /* [n_queries + 1] */
    int32_t* bitscore;        /* [n_hits] truncated toward zero (mod.rs:184) */
    int32_t* align_len;       /* [n_hits] */
    uint32_t* tax_desc_row;   /* [n_hits] row of the taxonomies file (left join, mod.rs:72-76) or BLU_UNMATCHED_TAXID */
    uint32_t* acc_rank;       /* [n_hits] */
    double* pident;           /* [n_hits] */
    char* query_names; uint64_t query_names_bytes;
    char* accessions; uint64_t accessions_bytes;
} blu_ingest_columns;
int blu_ingest_columns_on(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                          blu_ingest_columns* out);
/* The same under a selection (blu_hit_selection, above; NULL = none), on either parser: the columns of the lines the filters
 * keep, thinned to the best hit per subject and with the band applied to the bitscore column, in that order.  stats may be
 * NULL.  A best-hit selection or a band with a non-empty mask needs a device (device >= 0) whichever parser ran.
 * The minimum cover (blu_consensus_request.min_cover_milli) is not part of a blu_hit_selection and this call does not learn it:
 * it needs the taxonomy handle, which the ingest half does not build; blu_hits_cover_keep / blu_hits_cover_apply
 * (include/blu_consensus.h) are the column-level calls. */
int blu_ingest_columns_selected(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                                const blu_hit_selection* selection, blu_ingest_columns* out, blu_hit_selection_stats* stats);
/* The same under a column layout (blu_table_layout, above; NULL = the reference's columns: blu_ingest_columns_selected). */
int blu_ingest_columns_laid_out(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                                const blu_table_layout* layout, const blu_hit_selection* selection, blu_ingest_columns* out,
                                blu_hit_selection_stats* stats);
/* The same under a query cover (blu_query_cover, above; NULL = none: blu_ingest_columns_laid_out). */
int blu_ingest_columns_covered(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                               const blu_table_layout* layout, const blu_query_cover* cover, const blu_hit_selection* selection,
                               blu_ingest_columns* out, blu_hit_selection_stats* stats);
void blu_ingest_columns_free(blu_ingest_columns* cols);

/* Which parser the calling thread's last ingest used: 0 = CPU, 1 = GPU. */
int blu_last_ingest_path(void);
/* The minimum cover's counts of the calling thread's last blu_build_consensus (the outcome has no room for them): zeros when
 * that run had no min_cover_milli or failed.  Returns BLU_OK, BLU_ERR_INVALID_ARG for a NULL `out`. */
int blu_last_min_cover_stats(blu_min_cover_stats* out);

/* Binary cache of the taxonomies file.  The reference re-parses the `*.blutils.json` on every run
 * (mod.rs:246-327, taxonomies_map.rs:6-32) and keeps only {taxid, numericLineage | textLineage}; this writes exactly
 * that — interned lineages of the chosen flavour — as a flat file.  Wherever a `taxonomies_file` is taken
 * (blu_build_consensus, blu_ingest_only) a cache file is recognised by its magic and mapped instead of
 * parsed; results are identical.  A cache built for the other lineage flavour is refused (BLU_ERR_INVALID_ARG), a
 * truncated or altered one fails its checksum (BLU_ERR_PARSE). */
int blu_db_cache_build(const char* taxonomies_file, int use_taxid, const char* cache_file);

/* `blu build-db blu` (core/src/use_cases/build_blutils_db_from_ncbi_files/, build_taxonomy_database.rs:49-498) on the GPU:
 * the NCBI taxdump files and the text `blastdbcmd -entry all -db DB -outfmt "%a  %T  %o"` prints -> <output_stem>.blutils.json
 * (serde_json::to_string_pretty of TaxonomiesMap, taxonomies in ascending taxid) and <output_stem>.non-mapped.tsv (taxid, tab,
 * deleted | merged | unknown; ascending taxid; removed and created again on every call).  DESIGN.md "Taxonomies database
 * builder" has the rules.  Errors name the file and the 1-based line (blu_last_error); there is no CPU path. */
#define BLU_TAXDB_DEFAULT_VERSION "8.3.1"   /* blutilsVersion when blutils_version is NULL (blutils_amd/blast.py BLUTILS_VERSION) */
typedef struct blu_taxdb_desc {
    const char* nodes_path;        /* nodes.dmp */
    const char* names_path;        /* names.dmp */
    const char* lineage_path;      /* taxidlineage.dmp */
    const char* merged_path;       /* merged.dmp */
    const char* delnodes_path;     /* delnodes.dmp */
    const char* accessions_path;   /* the blastdbcmd listing */
    const uint64_t* skip_taxids;   /* -s, in command-line order (written to ignoreTaxids as given) */
    uint64_t n_skip;
    int32_t has_skip;              /* 0: ignoreTaxids is null */
    int32_t has_replace;           /* 0: replaceRank is null */
    const char* const* replace_from;   /* -r FROM=TO pairs, in command-line order (a repeated FROM keeps its last TO) */
    const char* const* replace_to;
    uint64_t n_replace;
    int32_t drop_non_linnaean;     /* -d */
    int32_t device;                /* HIP device ordinal */
    const char* source_database;   /* sourceDatabase, as given */
    const char* blutils_version;   /* NULL = BLU_TAXDB_DEFAULT_VERSION */
    const char* output_stem;       /* <parent>/<stem> after PathBuf::set_extension("json") (rs:240-270) */
} blu_taxdb_desc;

typedef struct blu_taxdb_stats {
    uint64_t n_nodes;              /* nodes.dmp lines read (UTF-8) */
    uint64_t n_names;              /* scientific-name lines of names.dmp */
    uint64_t n_lineage_tokens;     /* ancestor ids in taxidlineage.dmp */
    uint64_t n_accession_lines;
    uint64_t n_distinct_taxids;
    uint64_t n_mapped;             /* entries of a node */
    uint64_t n_mapped_merged;      /* entries through merged.dmp */
    uint64_t n_deleted, n_merged_missing, n_unknown;   /* TSV lines */
    uint64_t n_dropped;            /* leaves dropped by -d */
    uint64_t n_unmapped_ancestors; /* ancestors without a node (the reference's warnings) */
    uint64_t n_nonascii_names;     /* scientific names with bytes >= 0x80 (slug parity unpinned there) */
    uint64_t input_bytes, doc_bytes, tsv_bytes;
    double t_upload_ms, t_parse_ms, t_tables_ms, t_group_ms, t_assemble_ms, t_render_ms, t_write_ms;
} blu_taxdb_stats;

int blu_taxdb_build(const blu_taxdb_desc* desc, blu_taxdb_stats* stats);

/* `build-db lineages` (not in the reference) on the GPU: a two-column lineage table
 * `ID<TAB>d__Bacteria; p__Proteobacteria; ...` (SILVA, GTDB, UNITE, Greengenes, any QIIME 2 reference; what `build-db qiime2`
 * writes) -> <output_stem>.blutils.json, <output_stem>.non-mapped.tsv (`ID<TAB>LINE<TAB>empty-lineage` per data line no level of
 * which survives, in file order; removed and created again on every call) and, with taxid_map_path, the `ID taxid` lines that
 * `makeblastdb -parse_seqids -taxid_map` takes (written as <taxid_map_path>.partial and renamed at the end).  Every distinct
 * normalised path `rank__identifier;...` is one taxon; taxa are numbered from 1 in the order of their first appearance, file
 * top to bottom and levels left to right; the document has one entry per path that a line ends on, in ascending taxid.  Paths
 * are interned exactly: two of them are one taxon only when their bytes are equal, whatever their hashes.  Errors name the
 * table and the 1-based line (blu_last_error) and come before any file is written; there is no CPU path. */
typedef struct blu_lineage_db_desc {
    const char* table_path;        /* the lineage table */
    const char* output_stem;       /* as in blu_taxdb_desc */
    const char* taxid_map_path;    /* NULL: no taxid map */
    const char* const* replace_from;   /* -r FROM=TO pairs in command-line order, FROM lower-cased (a repeated FROM keeps its */
    const char* const* replace_to;     /*   last TO): an exact match on the lower-cased rank token of a level */
    uint64_t n_replace;
    int32_t has_replace;           /* 0: replaceRank is null */
    int32_t device;                /* HIP device ordinal */
    const char* source_database;   /* sourceDatabase, as given */
    const char* blutils_version;   /* NULL = BLU_TAXDB_DEFAULT_VERSION */
    /* two test aids; the files do not depend on either */
    uint32_t hash_bits;            /* 0 = all 64: the path hash is cut to its low hash_bits bits (1 .. 63), so that paths collide */
    uint32_t initial_slots;        /* 0 = sized for the table: slots of the first path dictionary, rounded up to a power of two
                                      (at least 16); a dictionary more than half full is doubled and built again */
} blu_lineage_db_desc;

typedef struct blu_lineage_db_stats {
    uint64_t n_lines;              /* lines of the file */
    uint64_t n_data_lines;         /* of them: not blank, not a comment, not the header */
    uint64_t n_taxonomies;         /* entries of the document */
    uint64_t n_taxa;               /* distinct paths (the largest taxid) */
    uint64_t n_empty;              /* data lines without a surviving level (TSV lines) */
    uint64_t n_truncated;          /* data lines cut at a level whose identifier is empty */
    uint64_t max_depth;            /* levels of the deepest line */
    uint64_t n_levels;             /* surviving levels of all lines (the items interned) */
    uint64_t n_dictionary_builds;  /* 1 + the times the dictionary was doubled */
    uint64_t input_bytes, doc_bytes, tsv_bytes, map_bytes;
    double t_upload_ms, t_parse_ms, t_intern_ms, t_group_ms, t_render_ms, t_write_ms;
} blu_lineage_db_stats;

int blu_lineage_db_build(const blu_lineage_db_desc* desc, blu_lineage_db_stats* stats);

/* `blu build-db kraken2` and the sequence half of `blu build-db qiime2` on the GPU
 * (core/src/use_cases/build_kraken_db_from_ncbi_files/, build_qiime_db_from_blutils_db/mod.rs:90-150): the text
 * `blastdbcmd -entry all -db DB -outfmt "%a  %T  %s"` (kraken2) or `"%a  %T  %o  %s"` (qiime2) prints, streamed in chunks
 * from a file descriptor (the pipe from blastdbcmd) or a path, rewritten on the device and written as it goes.
 *   kraken2: fna_path gets `>kraken:taxid|TAXID|ACC\n` + the sequence upper-cased in 80-column lines + `\n` per line;
 *            map_path gets `TAXID\tkraken:taxid|N|ACC\tN\n` per line (N: the taxid as usize), written only on success.
 *   qiime2:  fna_path gets `>TAXID-OID-ACC\nSEQUENCE\n` per line.
 * Output stops quietly before the first line that is not UTF-8 (the reference's read_line loop ends there); stats
 * `invalid_utf8_line` names it.  A line with too few pieces, a kraken2 taxid that is not a usize or a kraken2 sequence
 * with a byte >= 0x80 is an error (blu_last_error names the input and the 1-based line).  DESIGN.md "Sequence export". */
#define BLU_SEQDB_KRAKEN2 0
#define BLU_SEQDB_QIIME2 1
#define BLU_SEQDB_DEFAULT_CHUNK (1ull << 30)   /* chunk_bytes = 0 */
typedef struct blu_seqdb_desc {
    int32_t format;                /* BLU_SEQDB_KRAKEN2 | BLU_SEQDB_QIIME2 */
    int32_t input_fd;              /* >= 0: read this descriptor (not closed); -1: open input_path */
    const char* input_path;        /* the listing, or a label for input_fd in messages (may be NULL then) */
    const char* fna_path;          /* library.fna (kraken2) / the .fna of qiime2: created or truncated */
    const char* map_path;          /* prelim_map.txt (kraken2; NULL for qiime2) */
    uint64_t chunk_bytes;          /* bytes read per chunk; 0 = BLU_SEQDB_DEFAULT_CHUNK; a longer line grows the chunk */
    int32_t device;                /* HIP device ordinal */
    int32_t reserved;
} blu_seqdb_desc;

typedef struct blu_seqdb_stats {
    uint64_t n_lines;              /* records written */
    uint64_t input_bytes;          /* listing bytes consumed (up to the stop or error line) */
    uint64_t fna_bytes, map_bytes;
    uint64_t n_chunks;
    uint64_t max_line_bytes;       /* longest line seen, newline excluded */
    uint64_t invalid_utf8_line;    /* 1-based line of a quiet stop, 0 = none */
    double t_read_ms, t_gpu_ms, t_write_ms, t_wall_ms;   /* read: time inside read(); gpu: upload + kernels + download;
                                                             write: time inside write(); the three overlap */
} blu_seqdb_stats;

int blu_seqdb_export(const blu_seqdb_desc* desc, blu_seqdb_stats* stats);

/* The taxonomies half of `blu build-db qiime2` (build_qiime_db_from_blutils_db/mod.rs:24-84), on the host: the
 * `*.blutils.json` read as serde reads TaxonomiesMap, then `Feature ID\tTaxon\n` and one `TAXID-OID-ACC\tLINEAGE\n` per
 * accession in document order (numericLineage if use_taxid, else textLineage) to out_path.  A document serde_json would
 * reject is BLU_ERR_PARSE and out_path is then left absent; a binary cache (blu_db_cache_build) is refused. */
int blu_qiime_taxonomy_tsv(const char* json_path, int use_taxid, const char* out_path);

/* `build-db sintax` and `build-db dada2` (neither is in the reference): the kraken2 listing (`"%a  %T  %s"`) rewritten as one
 * FASTA whose header carries the lineage of the line's taxid.  The labels are rendered on the host once per call from the
 * taxonomies file (a `*.blutils.json` or a cache of the same lineage flavour, read by the loader of the consensus use-case)
 * and joined to the lines on the device, by the taxid's value.
 *   sintax: `>ACC;tax=d:bacteria,p:firmicutes,...,s:bacillus-subtilis;\nSEQUENCE\n`
 *   dada2:  `>bacteria;firmicutes;...;bacillus;\nSEQUENCE\n` (domain or kingdom, then phylum to genus, cut at the first gap)
 * The sequence is upper-cased and left on one line.  A line whose taxid has no row in the taxonomies file, or whose row has
 * no label, gives no record and is counted; the refusals and the quiet stop are those of kraken2, and they are decided
 * before the join.  DESIGN.md "Labelled FASTA export" has the label rules. */
#define BLU_SEQDB_SINTAX 2
#define BLU_SEQDB_DADA2 3
typedef struct blu_seqdb_label_desc {
    int32_t format;                /* BLU_SEQDB_SINTAX | BLU_SEQDB_DADA2 */
    int32_t input_fd;              /* >= 0: read this descriptor (not closed); -1: open input_path */
    const char* input_path;        /* the listing, or a label for input_fd in messages (may be NULL then) */
    const char* taxonomies_file;   /* *.blutils.json or its binary cache */
    int32_t use_taxid;             /* labels from numericLineage instead of textLineage */
    int32_t device;                /* HIP device ordinal */
    const char* fna_path;          /* created or truncated */
    uint64_t chunk_bytes;          /* as in blu_seqdb_desc */
} blu_seqdb_label_desc;

typedef struct blu_seqdb_label_stats {
    uint64_t n_lines;              /* listing lines read through (written or skipped), up to the stop or error line */
    uint64_t input_bytes;          /* their bytes */
    uint64_t fna_bytes;
    uint64_t n_chunks;
    uint64_t max_line_bytes;
    uint64_t invalid_utf8_line;    /* 1-based line of a quiet stop, 0 = none */
    uint64_t n_unknown_taxid;      /* of n_lines: skipped, the taxid has no row in the taxonomies file */
    uint64_t n_unlabelled;         /* of n_lines: skipped, the row's label is empty */
    uint64_t n_rows;               /* rows of the taxonomies file */
    uint64_t label_bytes;          /* bytes of all labels */
    double t_read_ms, t_gpu_ms, t_write_ms, t_wall_ms;   /* as in blu_seqdb_stats; wall includes t_labels_ms */
    double t_labels_ms;            /* loading the taxonomies file, rendering the labels, uploading them */
} blu_seqdb_label_stats;

int blu_seqdb_export_labelled(const blu_seqdb_label_desc* desc, blu_seqdb_label_stats* stats);

/* The labels alone, on the host (no device is needed): `TAXID\tLABEL\n` per row of the taxonomies file in file order, rows
 * with an empty label included, to out_path. */
int blu_seqdb_render_labels(const char* taxonomies_file, int use_taxid, int format, const char* out_path);

/* `blastn build-distances` (not in the reference): Bray-Curtis and Jaccard distances between the samples of a
 * sample-table file (`--sample-table`, `build-report --by-sample`), collapsed at one rank.
 *
 * The table: `#rank identifier taxonomy total <sample>...`, then `- unclassified`, optionally `- unplaced`, then one line per path;
 * every cell a u64 clade count.  A row's parent is the row whose taxonomy is its own minus the last `;element`; a row without `;`
 * is top-level.  direct_s(p) = clade_s(p) - the sum of clade_s over p's children.  BLU_ERR_PARSE, naming the 1-based line: a
 * negative direct count (the parent's line), a row whose parent is missing, a line whose cells do not number the header's samples,
 * a cell that is not a u64, a `total` that is not the sum of the line's cells, a taxonomy for the second time.
 * Features at rank R (the spelling of the table's rank column; `genus` is `g`, as for the taxon filters):
 *   (a) every row of rank R without a proper ancestor of rank R, with its clade cells;
 *   (b) every row that neither is nor has an ancestor of rank R, with its direct counts;
 *   (c) unclassified and unplaced, one feature each, unless BLU_DISTANCE_DROP_UNCLASSIFIED is set.
 * rank NULL: (b) for every row.  A feature that is zero in every sample is dropped (counted in n_dropped).  A rank no row
 * carries is BLU_ERR_INVALID_ARG naming it.  Per sample the features add up to unclassified + unplaced + the top-level clade
 * counts (the top-level sum alone under the flag); the call checks it. */
#define BLU_DISTANCE_DROP_UNCLASSIFIED 1u
#define BLU_DISTANCE_BRAY_CURTIS 0
#define BLU_DISTANCE_JACCARD 1
typedef struct blu_distance_features {
    uint64_t n_features;
    uint32_t n_samples;
    uint32_t reserved;
    uint64_t* row_ptr;        /* [n_features + 1] CSR over the features: what blu_distance_desc takes */
    uint32_t* sample;         /* [nnz] column of the table, ascending within a feature */
    uint64_t* count;          /* [nnz] > 0 */
    char** sample_names;      /* [n_samples] in the table's column order */
    char** feature_text;      /* [n_features] the row's taxonomy; `unclassified`, `unplaced`.  Fixed rows first, then file order */
    uint64_t n_dropped;       /* all-zero features left out */
} blu_distance_features;      /* every array malloc'd by the library: blu_distance_features_free */
int blu_distance_features_from_table(const char* table_path, const char* rank /* or NULL */, uint32_t flags, blu_distance_features* out);
void blu_distance_features_free(blu_distance_features* features);

/* The square matrix of one metric as text: a header line with an empty first cell and the names, then per sample its name and
 * one value per sample, tab-separated.
 *   bray-curtis: (N - 2 C) / N, N = total[a] + total[b], C = min_sum[a][b]
 *   jaccard:     (U - I) / U,   I = shared[a][b], U = richness[a] + richness[b] - I
 * with six decimals, rounded half up in integers: (num * 10^6 + den / 2) / den in 128 bits; `nan` where den = 0.
 * `integers` as blu_sample_distances filled it (include/blu_consensus.h); names[integers->n_samples]. */
int blu_distance_render(int metric, const char* const* names, const blu_sample_distance* integers, const char* out_path);

typedef struct blu_distance_stats {
    uint64_t n_features;      /* features kept */
    uint64_t n_samples;
    uint64_t n_nonzeros;
    uint64_t n_dropped;       /* all-zero features left out */
} blu_distance_stats;
/* The three steps chained: the features of table_path at `rank` (NULL: none), blu_sample_distances on `device`, the matrix of
 * `metric` to out_path.  stats may be NULL.  Nothing is written unless every step succeeds. */
int blu_distance_matrix_file(const char* table_path, const char* rank, int metric, uint32_t flags, int device, const char* out_path,
                             blu_distance_stats* stats);

/* The same with every sample rarefied to one depth first (`build-distances --rarefy`): features ->
 * blu_sample_rarefy with sample_stream[a] = blu_rarefy_stream of the seed and column a's name -> blu_sample_distances on the kept
 * samples -> the matrix with the kept names.  options NULL, or depth = 0 without a table path: exactly blu_distance_matrix_file.
 * rarefied_table_path: the rarefied features as text, `#feature<TAB>total<TAB><kept sample names...>`, then one line per feature
 * that is still non-zero, in feature order: its text, the line's sum, one u64 cell per kept sample; lines end in `\n`.
 * BLU_ERR_INVALID_ARG on top of what the steps refuse: a struct_size the library does not know, a table path with depth = 0, two
 * columns of one name (naming both), no sample that reaches `depth` (the message says the largest total).  Nothing is written
 * unless every step succeeds. */
typedef struct blu_distance_options {
    uint32_t struct_size;             /* sizeof(blu_distance_options) */
    uint32_t reserved;
    uint64_t depth;                   /* 0 = no rarefaction */
    uint64_t seed;
    const char* rarefied_table_path;  /* or NULL */
} blu_distance_options;               /* 32 bytes */
typedef struct blu_distance_stats2 {
    uint64_t n_features;              /* features kept; with a depth: those still non-zero after rarefaction */
    uint64_t n_samples;               /* with a depth: the kept samples */
    uint64_t n_nonzeros;              /* with a depth: of the rarefied features */
    uint64_t n_dropped;               /* all-zero features of the table left out */
    uint64_t depth;
    uint64_t n_samples_kept;
    uint64_t n_samples_dropped;
    uint64_t n_features_emptied;      /* features that lost every count */
    uint64_t n_reads_hashed;          /* the reads of the kept samples before rarefaction: what the device pass walks */
} blu_distance_stats2;
int blu_distance_matrix_file_with(const char* table_path, const char* rank, int metric, uint32_t flags, int device, const char* out_path,
                                  const blu_distance_options* options, blu_distance_stats2* stats2);

/* `blastn build-diversity` (not in the reference): alpha diversity of the samples of a sample-table file, raw or
 * along a ladder of rarefaction depths.
 *
 * blu_alpha_render: the integers that include/blu_consensus.h's blu_sample_alpha counts, as text, on the host:
 *   `#sample depth reads observed singletons doubletons chao1 simpson shannon goods_coverage` (tab-separated), then one line per
 *   present (sample, slot), samples in their order, depths ascending.  depth = depths[j] (raw, n_depths = 0: reads[a]); reads =
 *   reads[a] = N_a.  With F1 = singletons, F2 = doubletons and L = blu_alpha_log2:
 *     chao1          = (observed * 2 (F2 + 1) + F1 (F1 - 1)) / (2 (F2 + 1))
 *     simpson        = (n^2 - sum_sq) / n^2
 *     shannon        = max(0, n L(n) - sum_xlog) / (n 2^24)          (bits; the clamp is part of the rule: L is truncated)
 *     goods_coverage = (n - F1) / n
 *   with six decimals, rounded half up in 128-bit integers as blu_distance_render does; `nan` where the denominator is 0.
 *   BLU_ERR_INVALID_ARG for integers that cannot occur: n_slots that is not max(n_depths, 1), n of 2^32 or more, sum_sq > n^2,
 *   F1 > n, F1 + F2 > observed, observed > n. */
int blu_alpha_render(const char* const* names, const uint64_t* reads, const uint64_t* depths, uint32_t n_depths, const blu_alpha* integers,
                     const char* out_path);

typedef struct blu_alpha_options {
    uint32_t struct_size;             /* sizeof(blu_alpha_options) */
    uint32_t n_depths;                /* 0 = raw */
    const uint64_t* depths;           /* [n_depths] */
    uint64_t seed;                    /* not read in raw mode */
} blu_alpha_options;                  /* 24 bytes */
typedef struct blu_alpha_stats {
    uint64_t n_features;              /* features kept */
    uint64_t n_samples;
    uint64_t n_nonzeros;
    uint64_t n_dropped;               /* all-zero features of the table left out */
    uint64_t n_depths;
    uint64_t n_rows;                  /* lines of the file after the header */
    double t_device_ms;
} blu_alpha_stats;
/* The three steps chained: the features of table_path at `rank` (as blu_distance_matrix_file takes them), blu_sample_alpha with
 * sample_stream[a] = blu_rarefy_stream of the seed and column a's name, the text to out_path.  options NULL: raw.
 * BLU_ERR_INVALID_ARG on top of what the steps refuse: a struct_size the library does not know, with a ladder two columns of
 * one name (naming both) and no sample that reaches depths[0] (the message says the largest total).  Nothing is written unless
 * every step succeeds. */
int blu_alpha_table_file(const char* table_path, const char* rank, uint32_t flags, int device, const char* out_path,
                         const blu_alpha_options* options, blu_alpha_stats* stats);

/* CustomTaxon::from_file (domain/dtos/taxon.rs:28-66): .yaml or .json with the eight cutoff fields. */
int blu_custom_taxon_from_file(const char* path, blu_cutoff_config* cfg);

#ifdef __cplusplus
}
#endif
#endif /* BLU_PIPELINE_H */
