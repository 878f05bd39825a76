/*
 * blu_consensus.h — C ABI of the MI355X-native consensus engine.
 *
 * Drop-in boundary for blutils' per-query taxonomic consensus.  The reference
 * (pure Rust, no FFI of its own) exposes this path as
 *
 *   core/src/use_cases/build_consensus_identities/mod.rs:40-47
 *     pub fn build_consensus_identities(blast_output, taxonomies_file, taxon,
 *                                       strategy, use_taxid, custom_taxon_values)
 *   core/src/use_cases/build_consensus_identities/find_single_query_consensus.rs:17-23
 *     fn find_single_query_consensus(query, result: Vec<BlastResultRow>, taxon,
 *                                    strategy, custom_taxon_values)
 *
 * A Rust shim replacing the rayon map at mod.rs:104-128 binds exactly the
 * entry points below (see INTEGRATION.md for the `extern "C"` block).  Plain
 * pointers and sizes only; no exceptions or aborts cross this boundary: every
 * reference panic site becomes a per-query status (blu_status) or a call-level
 * error code (blu_error).
 */
#ifndef BLU_CONSENSUS_H
#define BLU_CONSENSUS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLU_ABI_VERSION 5u
#define BLU_UNMATCHED_TAXID 0xFFFFFFFFu /* hit whose subject_taxid is not in the taxonomy (left join miss, mod.rs:72-76) */
#define BLU_MAX_DEPTH 64u               /* level_mask is 64 bits wide */
#define BLU_ROW_BITS 25u                /* engine row id = sorted position | lineage length << 25: at most 2^25 taxids */
#define BLU_NONE_U8 0xFFu
#define BLU_NONE_U16 0xFFFFu
#define BLU_MAR_NEVER_EQUAL 0xFFFEu     /* Other("k")/Other("u"): a default-letter rank outside the backbone */

/* call-level error codes (return values) */
enum blu_error {
    BLU_OK = 0,
    BLU_ERR_INVALID_ARG = 1,
    BLU_ERR_NO_DEVICE = 2,      /* HIP runtime/device missing: the engine has no CPU fallback */
    BLU_ERR_HIP = 3,
    BLU_ERR_DEPTH = 4,          /* a lineage deeper than BLU_MAX_DEPTH */
    BLU_ERR_CUSTOM_MISSING = 5, /* Taxon::Custom without values (domain/dtos/taxon.rs:117) */
    BLU_ERR_ALLOC = 6,
    BLU_ERR_IO = 7,
    BLU_ERR_PARSE = 8,
    BLU_ERR_INTERNAL = 10       /* a result failed the library's own check (9 is BLU_ERR_REFERENCE_PANIC of blu_pipeline.h) */
};

/* domain/dtos/taxon.rs:68-87 */
enum blu_taxon { BLU_TAXON_FUNGI = 0, BLU_TAXON_BACTERIA = 1, BLU_TAXON_EUKARYOTES = 2, BLU_TAXON_CUSTOM = 3 };
/* domain/dtos/consensus_strategy.rs:4-10 */
enum blu_strategy { BLU_CAUTIOUS = 0, BLU_RELAXED = 1 };

/* Taxon + Option<CustomTaxon> (domain/dtos/taxon.rs:16-25): value order is
 * domain, kingdom, phylum, class, order, family, genus, species. */
typedef struct blu_cutoff_config {
    int32_t taxon;         /* enum blu_taxon */
    int32_t has_custom;    /* Option<CustomTaxon> is Some */
    int16_t custom[8];
    uint8_t custom_has[8]; /* the six middle ranks are Option<i16>; unwrap_or(0) when 0 */
} blu_cutoff_config;

/* Taxonomy table: one row per taxid of the blutils DB (a3), lineage as CSR of
 * interned (rank, identifier) node ids, root -> leaf (a6).  rank_names[] are
 * the rank strings as they appear in lineages ("d", "clade", "species-group"
 * ...); the library applies LinnaeanRank::from_str (linnaean_ranks.rs:52-72).
 * lin_node must be interned on the CANONICAL pair (Display(rank), identifier),
 * the key the reference compares levels on (find_multi_taxa_consensus.rs:150-159). */
typedef struct blu_taxonomy_desc {
    uint64_t n_tax;
    const int64_t* taxid;          /* [n_tax] or NULL */
    const uint64_t* lin_off;       /* [n_tax + 1] */
    const uint32_t* lin_node;      /* [lin_off[n_tax]] */
    const uint16_t* lin_rank;      /* [lin_off[n_tax]] index into rank_names */
    uint32_t n_ranks;
    const char* const* rank_names; /* [n_ranks] */
    const uint8_t* bad;            /* [n_tax] or NULL; 1 = lineage string fails parse_taxonomy (blast_result.rs:109-114) */
} blu_taxonomy_desc;

typedef struct blu_taxonomy blu_taxonomy; /* opaque; owns the device copy */

/* Hit table, SoA, rows grouped by query with in-query FILE ORDER preserved
 * (stable-sort ties depend on it, find_multi_taxa_consensus.rs:39-68).  Only
 * the columns the reference semantics read; e_value and the six
 * coordinate columns are dead inputs and are not part of the layout. */
typedef struct blu_hits {
    const int32_t* bitscore;   /* [n_hits] bit_score truncated toward zero to integer (mod.rs:184) */
    const uint32_t* tax_row;   /* [n_hits] ENGINE row id of subject_taxid (blu_taxonomy_lookup / blu_taxonomy_row_map:
                                  the left join of mod.rs:72-76) or BLU_UNMATCHED_TAXID.  Engine row ids are opaque:
                                  the row's rank in lexicographic lineage order (low BLU_ROW_BITS bits) and its lineage
                                  length (bits above); they are NOT the desc row indices. */
    const double* pident;      /* [n_hits] perc_identity as f64, or NULL when pident_milli is given */
    const int32_t* align_len;  /* [n_hits] */
    const uint32_t* acc_rank;  /* [n_hits] order-preserving rank of subject_accession (bytewise String::cmp) */
    const uint64_t* seg_off;   /* [n_queries + 1] row offsets, seg_off[0] = 0, seg_off[n_queries] = n_hits */
    uint64_t n_hits;           /* < 2^32 - 1 per call (0xFFFFFFFF is the "no row" value of blu_result.ref_row) */
    uint64_t n_queries;
    int32_t on_device;         /* 1: every pointer (and `out`) is a device pointer on the handle's GPU;
                                  0: host pointers, the library stages them over PCIe */
    int32_t reserved;
    const uint32_t* pident_milli; /* [n_hits] or NULL.  Narrow lossless encoding of perc_identity for tables whose
                                  text has at most 3 decimals (BLAST outfmt 6 prints %.3f): k = perc_identity * 1000
                                  as an exact integer.  The engine rebuilds the f64 the reference's parser produces,
                                  the correctly rounded k / 1000, for the few rows that need it.  20 B/hit instead of
                                  24. */
    const uint32_t* packed;    /* [n_hits][4] or NULL (ABI v3).  The four non-bit-score values of a hit side by side,
                                  16 bytes per hit: {tax_row, pident_milli | shape hint << 17, align_len, acc_rank};
                                  tax_row, pident, pident_milli, align_len and acc_rank are then ignored (may be NULL).
                                  Same 20 B/hit as the milli-percent columns, but the engine — which reads those four
                                  values for the top-scoring rows only — finds a row's values in ONE memory line instead
                                  of four.  16-byte aligned.  Built by blu_hits_pack (ABI v4): pident_milli must be below
                                  BLU_PACKED_PIDENT_LIMIT (131.071 %; larger identities go in the column layouts), and
                                  the bits above it carry a hint for the engine — the lineage shape of the hit's taxonomy
                                  row + 1, a function of the joined taxid like the row id itself — which lets it ask for
                                  the per-level tables together with the reference row instead of after it.  A hint of 0
                                  (records put together by hand) or a wrong one costs a memory round trip, never a
                                  result: the engine checks it against the row. */
    const uint32_t* packed64;  /* [n_hits][6] or NULL (ABI v4).  The same for perc_identity values that are not exact
                                  milli-percent: 24 bytes per hit {tax_row, shape hint << 17, align_len, acc_rank,
                                  pident f64 (low word, high word)}, 8-byte aligned; built by blu_hits_pack64.  28 B/hit
                                  with the bit-score column.  Exactly one of pident / pident_milli / packed / packed64
                                  is non-NULL. */
} blu_hits;

#define BLU_PACKED_PIDENT_LIMIT 131071u /* packed layout: pident_milli < this (17 bits, the top value is the engine's "never") */

typedef struct blu_run_params {
    int32_t strategy; /* enum blu_strategy */
    int32_t flags;    /* reserved, 0 */
    void* stream;     /* hipStream_t to launch on (NULL = default stream) */
} blu_run_params;

/* per-query status: 0/1 are the two reference outcomes with a taxon, 2 is
 * NoConsensusFound, >= 16 are the reference's panic sites */
enum blu_status {
    BLU_ST_CONSENSUS_MULTI = 0,   /* find_multi_taxa_consensus outcome */
    BLU_ST_CONSENSUS_SINGLE = 1,  /* single top-score hit (find_single_query_consensus.rs:74-150) */
    BLU_ST_NO_HITS = 2,           /* empty segment: NoConsensusFound (mod.rs:107-113) */
    BLU_ST_ERR_UNMATCHED_TAXID = 16, /* top-group row whose taxid is not in the DB (find_single_query_consensus.rs:58-60) */
    BLU_ST_ERR_BAD_LINEAGE = 17,     /* top-group row whose lineage fails parse_taxonomy (blast_result.rs:109-114) */
    BLU_ST_ERR_ROOT_DISAGREE = 18,   /* disagreement at level 0: `index - 1` underflow (find_multi_taxa_consensus.rs:181) */
    BLU_ST_ERR_SINGLE_BELOW_CUTOFFS = 19, /* single hit below every cutoff (find_single_query_consensus.rs:113-119) */
    BLU_ST_ERR_BAD_PIDENT = 20       /* NaN perc_identity in the top group: comparator/unwrap behaviour not restated */
};

#define BLU_FLAG_MUTATED 0x01u /* TaxonomyBean.mutated (build_blast_consensus_identity.rs:35-37) */
#define BLU_FLAG_AGREE 0x02u   /* every examined level agreed: taxonomy = whole cutoff-filtered reference lineage */

/* One 32-byte record per query.  Strings (taxonomy, consensus beans) are
 * rebuilt on the host from (ref_row, level_mask, bean_index). */
typedef struct blu_result {
    uint8_t status;            /* enum blu_status */
    uint8_t flags;             /* BLU_FLAG_* */
    uint8_t bean_index;        /* index into the reference lineage passed to build_blast_consensus_identity */
    uint8_t max_allowed_level; /* level of the reference lineage whose rank is max_allowed_rank; BLU_NONE_U8 = None */
    uint16_t reached_rank;     /* canonical rank code of the final element (blu_taxonomy_rank_name) */
    uint16_t max_allowed_rank; /* canonical rank code, BLU_MAR_NEVER_EQUAL, or BLU_NONE_U16 */
    uint32_t identifier_node;  /* interned node id of the final element: TaxonomyBean.identifier */
    uint32_t ref_row;          /* absolute hit row of the reference row R: perc_identity, bit_score, lineage */
    uint64_t level_mask;       /* bit j set = level j of R's lineage is in `taxonomy` */
    double ident_used;         /* identity tested against the cutoffs (R's pident, or the group max on disagreement) */
} blu_result;

/* -------------------------------------------------------------------------- */

uint32_t blu_abi_version(void);

/* Copies the last error message of the calling thread into buf (NUL-terminated,
 * truncated to len); returns the message length. */
size_t blu_last_error(char* buf, size_t len);

/* Builds the device-resident taxonomy: lineage rows, rank-sequence shapes and
 * the per-shape f64 cutoff tables (InterpolatedIdentity::interpolate_identities,
 * linnaean_ranks.rs:220-383; Taxon::get_taxon_cutoff, taxon.rs:104-185).
 * device >= 0: HIP device ordinal.  device == -1: host-only handle (cutoff and
 * shape queries work, blu_consensus_run refuses) — used by CPU-side tests.
 * Caller keeps ownership of desc arrays; they may be freed after the call. */
int blu_taxonomy_create(const blu_taxonomy_desc* desc, const blu_cutoff_config* cfg, int device,
                        blu_taxonomy** out);
void blu_taxonomy_destroy(blu_taxonomy* tax);

/* Introspection used by the host-side renderer and by tests. */
uint64_t blu_taxonomy_n_tax(const blu_taxonomy* tax);
uint32_t blu_taxonomy_n_shapes(const blu_taxonomy* tax);
uint32_t blu_taxonomy_n_rank_codes(const blu_taxonomy* tax);
uint32_t blu_taxonomy_max_depth(const blu_taxonomy* tax);
uint64_t blu_taxonomy_device_bytes(const blu_taxonomy* tax);
/* canonical rank code -> Display string (linnaean_ranks.rs:74-89); serde!=0 gives
 * the serde name ("species", raw string for Other; linnaean_ranks.rs:14-29). */
const char* blu_taxonomy_rank_name(const blu_taxonomy* tax, uint32_t rank_code, int serde);
/* cutoffs of one taxonomy row: writes up to cap entries, returns the lineage length
 * (0 for a bad lineage, -1 for an invalid row). is_default[j]=1: level j mapped to a
 * DefaultRank of the backbone.  rank_code[j]: canonical code of level j. */
int32_t blu_taxonomy_row_cutoffs(const blu_taxonomy* tax, uint64_t desc_row, uint32_t cap, double* cutoff,
                                 uint8_t* is_default, uint16_t* rank_code);
/* taxid -> ENGINE row id (BLU_UNMATCHED_TAXID when absent); needs desc.taxid at create.  This is the join of
 * the hit table with the taxonomy (mod.rs:72-76); its output is what blu_hits.tax_row holds.  A taxid the descriptor
 * lists more than once maps to its FIRST row (the reference's left join would multiply the hit rows: the whole-use-case
 * path of blu_pipeline.h does; blutils' own databases have unique taxids). */
int blu_taxonomy_lookup(const blu_taxonomy* tax, const int64_t* taxid, uint64_t n, uint32_t* out_row);
/* desc row index -> engine row id for every row of the table (out_map[n_tax]); inverse in out_inverse[n_tax]
 * (either may be NULL).  For callers that already hold desc row indices. */
int blu_taxonomy_row_map(const blu_taxonomy* tax, uint32_t* out_map, uint32_t* out_inverse);
/* (ABI v5, introspection) Number of leading lineage levels shared by ALL rows at sorted positions lo..hi (the low BLU_ROW_BITS
 * bits of engine row ids; lo <= hi < n_tax) — what the per-level scan of find_multi_taxa_consensus.rs:137-180 finds for a
 * top group spanning those positions, before the clamp to the shortest lineage.  *by_scan: from the adjacent-row prefix
 * lengths, one by one; *by_tables: what the engine's tables give (the wide-node chains for spans of 128 rows and more,
 * the range-minimum tables otherwise and where the chains do not reach; *via = 1 chains, 0 range minimum).  The two
 * must agree; any pointer may be NULL.  Host only, no device needed. */
int blu_taxonomy_shared_levels(const blu_taxonomy* tax, uint32_t lo, uint32_t hi, uint32_t* by_scan, uint32_t* by_tables, int32_t* via);
/* (ABI v5) Frees the device buffers the handle keeps from call to call for the host-pointer path of blu_consensus_run
 * (the staged columns and records of the largest table so far).  The handle stays valid; the next host-pointer call
 * allocates what it needs again.  No run on the handle may be in flight. */
int blu_taxonomy_trim(const blu_taxonomy* tax);

/* (introspection) The device primitives the GPU ingest, the database builders and the report stand on
 * (csrc/dev_prims.hip), callable on their own so that they can be checked against plain references.  Arrays are
 * device pointers on `device` (n_newlines is a host pointer).  Each call synchronises the device on entry and on return, allocates its own scratch,
 * and returns a blu_error code (BLU_ERR_INVALID_ARG for a bad argument, BLU_ERR_ALLOC, BLU_ERR_HIP).
 *
 * Exclusive prefix sum out[i] = in[0] + ... + in[i - 1] (i < n) of n unsigned integers of elem_bytes = 4 or 8 bytes,
 * modulo 2^(8 elem_bytes); in == out is allowed. */
int blu_dev_exclusive_scan(int device, const void* in, void* out, uint64_t n, int elem_bytes);
/* Stable LSD radix sort of n (key, value) pairs in place, 8 bits per pass, ceil(bits / 8) passes (bits 0..32): the
 * pairs end in the order of the low 8 ceil(bits / 8) bits of the key, equal keys in their input order.  Callers pass
 * keys below 2^bits. */
int blu_dev_radix_sort_pairs(int device, uint32_t* keys, uint32_t* vals, uint32_t n, int bits);
/* Line index of text[0, size): *n_newlines = the '\n' bytes in it; line[0] = 0 and line[k + 1] = the offset after
 * newline k.  `text` is 16-byte aligned and readable (padded) for at least 64 bytes past `size`; bytes past `size` are
 * never counted.  The newlines are counted first: if *n_newlines + 1 > cap, or *n_newlines >= 2^32, nothing is written
 * to `line` and the call is BLU_ERR_INVALID_ARG. */
int blu_dev_line_index(int device, const unsigned char* text, uint64_t size, uint64_t* line, uint64_t cap, uint64_t* n_newlines);

/* The hot path: one blu_result per query.  `out` has n_queries records, on the
 * device when hits->on_device, else on the host.  Asynchronous on
 * params->stream when on_device (no host sync inside); synchronous otherwise.
 * Consecutive runs on one handle must be ordered (same stream, or synchronised): the handle's scratch
 * (worklist and its counters) is reused from run to run. */
int blu_consensus_run(const blu_taxonomy* tax, const blu_hits* hits, const blu_run_params* params,
                      blu_result* out);

/* The side records of the packed layouts from the four columns (an ingest-time pass, like the join that produced
 * tax_row): `columns` holds tax_row (engine row ids), align_len, acc_rank and pident_milli or pident, n_hits and
 * on_device (1: device pointers on the handle's GPU, out too; the kernel runs on `stream` and the call returns after
 * it has finished — it reports values the layout cannot hold).  blu_hits_pack writes 4 words per hit and fails with
 * BLU_ERR_INVALID_ARG if a perc_identity is not an exact milli-percent value below BLU_PACKED_PIDENT_LIMIT;
 * blu_hits_pack64 writes 6 words per hit and takes any f64 (or milli-percent column, converted as the engine would). */
int blu_hits_pack(const blu_taxonomy* tax, const blu_hits* columns, uint32_t* packed_out, void* stream);
int blu_hits_pack64(const blu_taxonomy* tax, const blu_hits* columns, uint32_t* packed64_out, void* stream);

/* One host table over several GPUs: `taxes[0..n_tax_handles)` are handles of the SAME taxonomy and cutoff
 * configuration on different devices (the same device twice is allowed).  Queries are cut into contiguous ranges
 * balanced by hit count (blu_shard_ranges), every range runs on its handle from a host thread of its own (staging,
 * kernels and record copy-back overlap across devices), and the records land in `out` in query order with `ref_row`
 * pointing into the whole table.  Host pointers only (hits->on_device must be 0); no collective, nothing shared but
 * the read-only inputs.  Returns the first error of any shard. */
int blu_consensus_run_multi(const blu_taxonomy* const* taxes, uint32_t n_tax_handles, const blu_hits* hits,
                            const blu_run_params* params, blu_result* out);
/* bounds[0..n_shards]: query indices cutting seg_off[0..n_queries] into n_shards contiguous ranges whose hit counts
 * are as equal as the segment boundaries allow (host pointers). */
int blu_shard_ranges(const uint64_t* seg_off, uint64_t n_queries, uint32_t n_shards, uint64_t* bounds);

/* Name of the dominant kernel and its launch geometry for the last run on this
 * thread (for profiles/ bookkeeping). */
int blu_consensus_last_launch(char* kernel_name, size_t len, uint32_t* grid, uint32_t* block);

/* -------------------------------------------------------------------------- */
/* Taxon abundance report (additive, ABI v5).  A query's path is the `taxonomy` the document writes for it: the
 * levels of the lineage of tax_row[ref_row] that level_mask selects.  A path is a node sequence; its prefixes are
 * paths too.  direct = summed weight of the queries whose path is exactly this one, clade = of those that have it as
 * a prefix.  Counted on the device (csrc/report_kernel.hip); DESIGN.md §12. */
#define BLU_REPORT_NO_PARENT 0xFFFFFFFFu

typedef struct blu_report_path {
    uint32_t node;     /* interned node id of the last element (blu_taxonomy_desc.lin_node).  A path may not BEGIN with node id
                          0xFFFFFFFF (elsewhere in a path it is an id like any other): the report and both sample-table calls
                          refuse such a record with BLU_ERR_INVALID_ARG, naming it. */
    uint32_t parent;   /* index of the path one element shorter in blu_report.paths, BLU_REPORT_NO_PARENT for a first element */
    uint64_t direct;
    uint64_t clade;
} blu_report_path;     /* 24 bytes */

typedef struct blu_report {
    uint64_t n_paths;
    blu_report_path* paths;   /* [n_paths], parents before their children (paths[i].parent < i); otherwise in no promised
                                 order.  malloc'd by the library: blu_report_free */
    uint64_t unclassified;    /* weight of the records with status >= 2 (NoConsensusFound, and the panic statuses) */
    uint64_t unplaced;        /* weight of the records with a taxon whose level_mask selects no level (taxonomy "") */
    uint64_t total;           /* unclassified + unplaced + the clades of the first-level paths */
    uint64_t table_slots;     /* size of the device path table of the last attempt */
    uint32_t attempts;        /* 1, or 2 when the first table (sized from 2 n_tax) was too small and was rebuilt from the bound */
    uint32_t reserved;
    double t_device_ms;       /* table clear + count + compaction on the device, by events */
} blu_report;

/* The report of one run's records: `hits` gives the engine row ids (tax_row, or word 0 of the packed / packed64 records),
 * n_hits, n_queries and on_device as for blu_consensus_run (the other columns are not read); results[n_queries] are its
 * records (16-byte aligned); weights[n_queries] per-query weights or NULL (= 1 each), on the same side as the records.
 * Device pointers: waits for `stream` (a hipStream_t, NULL = default) before reading them.  Host pointers: the records, the
 * row of each record and the weights are uploaded.  Synchronous; the paths are on the host on return.  A record with a
 * taxon whose reference row names no taxonomy row is BLU_ERR_INVALID_ARG; there is no CPU fallback. */
int blu_consensus_report(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const uint32_t* weights,
                         void* stream, blu_report* out);
void blu_report_free(blu_report* report);

/* -------------------------------------------------------------------------- */
/* Per-sample taxon abundance table (additive, ABI v5).  The report above split by sample: every query names a sample id
 * (sample_of[q] < n_samples), and a cell (path, sample) holds the summed weight of that sample's queries whose path has
 * `path` as a prefix — a clade count per sample.  Counted on the device in one walk per query (csrc/report_kernel.hip,
 * the report's path table shared); DESIGN.md §13. */
typedef struct blu_sample_cell {
    uint32_t path;     /* index into blu_sample_table.paths */
    uint32_t sample;   /* < n_samples */
    uint64_t clade;    /* > 0 */
} blu_sample_cell;     /* 16 bytes */

typedef struct blu_sample_table {
    uint64_t n_paths;
    blu_report_path* paths;   /* [n_paths] parents before their children, as blu_report.paths; direct and clade are summed
                                 over the samples (the report's numbers) */
    uint64_t n_cells;
    blu_sample_cell* cells;   /* [n_cells] the non-zero cells, sorted by (path, sample) */
    uint32_t n_samples;
    uint32_t reserved;
    uint64_t* unclassified;   /* [n_samples] weight of the records with status >= 2, per sample */
    uint64_t* unplaced;       /* [n_samples] weight of the records with a taxon whose level_mask selects no level */
    uint64_t table_slots;     /* size of the device cell table of the last attempt */
    uint32_t attempts;        /* 1, or 2 when the first tables (sized from an estimate) were rebuilt from the bound */
    uint32_t reserved2;
    double t_device_ms;       /* table clear + count + compaction on the device, by events */
} blu_sample_table;           /* every array malloc'd by the library: blu_sample_table_free */

/* The per-sample table of one run's records: hits, results, weights and stream as for blu_consensus_report;
 * sample_of[n_queries] the sample id of each query, on the same side as the records.  A sample id >= n_samples is
 * BLU_ERR_INVALID_ARG naming the query index; a table that cannot be allocated is BLU_ERR_ALLOC. */
int blu_consensus_sample_table(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const uint32_t* weights,
                               const uint32_t* sample_of, uint32_t n_samples, void* stream, blu_sample_table* out);
void blu_sample_table_free(blu_sample_table* table);

/* The same table when a query's abundances come from a feature x sample count table instead of its name (additive, ABI v5;
 * DESIGN.md §22): query q carries the non-zeros [row_ptr[q], row_ptr[q + 1]) of a CSR matrix, each a sample id and a count,
 * and adds every count to the cells (path, sample) of all prefixes of its path.  The two arrays hold row_ptr[n_queries]
 * entries.  A row may be empty (its paths are still listed), may name a sample twice (the counts add up) and may hold zeros. */
typedef struct blu_count_rows {      /* CSR over the queries; all three on the same side as the records */
    const uint64_t* row_ptr;         /* [n_queries + 1] */
    const uint32_t* sample;          /* [nnz], each < n_samples */
    const uint32_t* count;           /* [nnz]; a zero is allowed and leaves no cell */
} blu_count_rows;
/* hits, results and stream as for blu_consensus_sample_table; fills the same blu_sample_table, freed the same way:
 * paths[i].direct is the summed row sum of the queries that end at the path, clade the sum of the path's cells,
 * unclassified[s] / unplaced[s] the counts in sample s of the records without a taxon / without a selected level.  A sample id
 * >= n_samples, or a row_ptr that decreases or passes row_ptr[n_queries], is BLU_ERR_INVALID_ARG naming the query index (decided
 * on the device, which reads nothing out of range); a host-only taxonomy is BLU_ERR_NO_DEVICE. */
int blu_consensus_sample_table_counts(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const blu_count_rows* rows,
                                      uint32_t n_samples, void* stream, blu_sample_table* out);

/* -------------------------------------------------------------------------- */
/* Per-query assignment support (additive, ABI v5): how well the hits of a query back the taxon its record names.
 * A hit is MATCHED when its row id names a taxonomy row whose lineage parsed (not BLU_UNMATCHED_TAXID, not a `bad` or empty
 * lineage).  The ASSIGNED CLADE of a record with a taxon (status 0 / 1) is every taxonomy row whose lineage has more than L
 * levels and shares its first L + 1 nodes with the lineage of the reference row, L = the highest bit of level_mask (the last
 * level the `taxonomy` string shows; the levels the cutoffs filtered out of the string are compared too); level_mask == 0
 * (taxonomy "") is the empty prefix: every matched hit.  A record with status >= 2 has no clade.  A hit SUPPORTS the
 * assignment when it is matched and its row lies in the clade.  All counts are integers: exact and deterministic.
 * Counted on the device (csrc/support_kernel.hip): the clade is one range of sorted positions, found once per query from
 * the lcp8 / rmq tables, and every hit is one range compare; DESIGN.md §15. */
typedef struct blu_support {
    uint32_t n_hits;           /* rows of the segment */
    uint32_t n_matched;        /* matched rows */
    uint32_t n_top;            /* rows whose bit-score equals the segment's maximum */
    uint32_t n_top_support;    /* of those, the supporting ones */
    uint32_t n_support;        /* supporting rows of the whole segment */
    int32_t top_score;         /* the maximum bit-score (0 for an empty segment) */
    int64_t bits;              /* sum of bit-scores over the segment */
    int64_t support_bits;      /* sum of bit-scores over the supporting rows */
} blu_support;                 /* 40 bytes */

/* The support counts of one run's records: `hits` as for blu_consensus_run, of which seg_off, bitscore, the engine row id of
 * each hit (tax_row, or word 0 of the packed / packed64 records), n_hits, n_queries and on_device are read; results[n_queries]
 * are its records.  Device pointers: results 16-byte aligned, `out` a device pointer too (8-byte aligned); the call waits
 * for `stream` (a hipStream_t, NULL = default) before reading and returns when `out` is complete.  Host pointers: the two
 * columns, the offsets and the records are uploaded and the counts copied back.  For status >= 2, n_top_support, n_support
 * and support_bits are 0 and the rest are still filled; an empty segment gives zeros.  A record with a taxon whose ref_row
 * names no taxonomy row is BLU_ERR_INVALID_ARG naming the query index; a host-only handle is BLU_ERR_NO_DEVICE: there is no
 * CPU fallback. */
int blu_consensus_support(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, void* stream,
                          blu_support* out /* [n_queries] */);

/* -------------------------------------------------------------------------- */
/* Bit-score band (additive, ABI v5; not in the reference).  The consensus of a query is decided by the rows that
 * tie on its top truncated bit-score t; a band lets the rows just under t count as tied.  A row with score b < t is IN THE BAND
 * when every criterion named in `mask` holds, in 64-bit integers (no floating point):
 *   BLU_BAND_TOP_BITS     b >= t - top_bits                                  (top_bits < 2^32)
 *   BLU_BAND_TOP_PERCENT  b * 100000 >= t * (100000 - top_percent_milli)     (top_percent_milli = percent * 1000, <= 100000)
 * (for t < 0 no row meets the percent criterion).  In-band rows get the score t; nothing else changes.  Everything that finds
 * the top group by comparing the column with its maximum — the engine, the top rows, the report, the support counts — then
 * sees the band as the top group.  top_bits = 0 and top_percent_milli = 0 are the exact ties: the column is unchanged.  The
 * pass is idempotent: a raised column raised again is unchanged. */
#define BLU_BAND_TOP_PERCENT 1u
#define BLU_BAND_TOP_BITS    2u
typedef struct blu_score_band { uint32_t top_percent_milli; uint32_t mask; uint64_t top_bits; } blu_score_band;
typedef struct blu_score_band_stats {
    uint64_t n_hits;      /* rows of the column */
    uint64_t n_raised;    /* rows whose score changed */
    uint64_t n_queries;
    uint64_t n_widened;   /* queries with at least one such row */
} blu_score_band_stats;
/* bitscore[n_hits] -> out[n_hits] (out == bitscore: in place; otherwise the two must not overlap) under seg_off[n_queries + 1];
 * stats may be NULL.  Counted on the device (csrc/band_kernel.hip).  on_device = 1: device pointers on `device`; the call waits
 * for `stream` (a hipStream_t, NULL = default), runs on it and returns when `out` and the counts are complete.  OUT OF PLACE
 * WITH AN ACTIVE BAND ONLY THE ROWS THAT A SEGMENT NAMES ARE WRITTEN: where seg_off[0] = 0 and seg_off[n_queries] = n_hits, as in
 * every blu_hits table, that is the whole column; rows outside every segment (n_queries = 0 aside, which copies the column)
 * keep what `out` held.  on_device = 0: the column and the offsets are uploaded, the same kernel runs, the
 * column is copied back — there is no second implementation.  Offsets beyond n_hits are clamped to it and a decreasing pair is
 * an empty segment: a corrupt table reads and writes nothing outside the columns.  A NULL band or an empty mask copies the
 * column.  BLU_ERR_INVALID_ARG: top_percent_milli > 100000, top_bits >= 2^32 (whatever the mask says), unknown mask bits, a
 * NULL array with a non-zero count. */
int blu_hits_score_band(int device, const int32_t* bitscore, const uint64_t* seg_off, uint64_t n_hits, uint64_t n_queries,
                        int on_device, const blu_score_band* band, void* stream, int32_t* out, blu_score_band_stats* stats);

/* -------------------------------------------------------------------------- */
/* Best hit per subject (additive, ABI v5; not in the reference).  BLAST writes one line per HSP, so a subject
 * that aligns to a query in several places occurs several times in the query's segment.  A PAIR is (query, acc_rank): the
 * rows of one segment with one acc_rank, whatever their tax rows.  Of a pair's rows the BEST is kept and the others are
 * dropped: the best has the highest truncated bit-score, and of equal scores it is the first row of the segment.  In one
 * 64-bit value, with i the row's index inside its segment:
 *   pack = (uint64)((uint32)bitscore ^ 0x80000000) << 32 | (0xFFFFFFFF - i)
 * and a row is kept iff no row of its segment has its acc_rank and a larger pack.  Every query keeps at least one row and
 * every pair keeps exactly one; the pass is idempotent. */
#define BLU_SUBJECT_BEST_PER_QUERY 1u
typedef struct blu_subject_best { uint32_t mask; uint32_t reserved; } blu_subject_best;
typedef struct blu_subject_best_stats {
    uint64_t n_hits;      /* rows in */
    uint64_t n_kept;      /* rows kept */
    uint64_t n_queries;
    uint64_t n_thinned;   /* queries that lost at least one row */
} blu_subject_best_stats;
/* The verdicts alone: keep_out[i] = 1 (row i is its pair's best) or 0, one 32-bit word per row, under seg_off[n_queries + 1];
 * stats may be NULL.  Decided on the device (csrc/subject_kernel.hip).  on_device = 1: device pointers on `device`; the call
 * waits for `stream` (a hipStream_t, NULL = default), runs on the default stream and returns when keep_out and the counts are
 * complete.  on_device = 0: the two columns and the offsets are uploaded, the same kernels run, the verdicts are copied back
 * -- there is no second implementation.  Offsets beyond n_hits are clamped to it and a decreasing pair is an empty segment: a
 * corrupt table reads and writes nothing outside the columns; a row that no segment names gets 0.  BLU_ERR_INVALID_ARG, before
 * any device is asked for: a NULL array with a non-zero count, n_hits >= 2^32 or n_queries >= 2^32 (the row index inside a
 * segment and the query in the long path's key are 32 bits; with n_queries < 2^32 no key equals the table's empty key ~0);
 * after the device pass: segments longer than 64 rows that overlap (their rows sum to more than n_hits). */
int blu_hits_subject_keep(int device, const int32_t* bitscore, const uint32_t* acc_rank, const uint64_t* seg_off, uint64_t n_hits,
                          uint64_t n_queries, int on_device, void* stream, uint32_t* keep_out, blu_subject_best_stats* stats);
/* The same pass, then the compaction of the five columns and seg_off IN PLACE: the kept rows move to the front of each column in
 * their order (the placement is an exclusive scan of the verdicts), seg_off[q] becomes the number of kept rows before it.
 * *n_hits_out: the rows left; *n_unmatched_out: how many of them have tax_desc_row == unmatched_marker (either may be NULL).
 * When every row is kept the columns are not touched.  `sel`: NULL or an empty mask leaves the table as it is and asks for no
 * device; unknown mask bits are BLU_ERR_INVALID_ARG.  Device pointers must be 16-byte aligned.  Otherwise as above. */
int blu_hits_subject_best(int device, int32_t* bitscore, int32_t* align_len, uint32_t* tax_desc_row, uint32_t* acc_rank, double* pident,
                          uint64_t* seg_off, uint64_t n_hits, uint64_t n_queries, int on_device, const blu_subject_best* sel, void* stream,
                          uint32_t unmatched_marker, uint64_t* n_hits_out, uint64_t* n_unmatched_out, blu_subject_best_stats* stats);

/* -------------------------------------------------------------------------- */
/* Minimum cover (additive, ABI v5; not in the reference).  The consensus of a query is the strict agreement of the
 * rows that tie on its top truncated bit-score, so one mislabelled accession among forty tied hits of one species has a veto.
 * Under a minimum cover of P percent (min_cover_milli = 1000 P, 50001 .. 100000: 50 < P <= 100, compared in integers) the query is
 * placed at the deepest taxon that still covers P % of its top group, and the top rows outside that taxon are dropped.  For a
 * segment whose top group T (the rows on the segment's maximum score) has n rows:
 *   need = the smallest integer with need * 100000 >= n * min_cover_milli                       (64-bit arithmetic)
 *   c    = the longest sequence of lineage nodes, root first, that at least `need` rows of T start with
 *          (need > n / 2: two such sequences are nested, so the longest is unique; the empty one always qualifies); d* = |c|
 * and a row of T is dropped iff its lineage does not start with c.  Rows under the top score are never touched, and at least
 * `need` >= 1 top rows stay, so the top score stays.  A query is LEFT ALONE — every row kept — when n <= 1, and (counted as
 * n_unresolved) when T holds a row that is BLU_UNMATCHED_TAXID, a row whose lineage is `bad` or empty (length 0 in the engine row
 * id), or a row id that names no taxonomy row (position >= n_tax, length beyond the taxonomy's deepest lineage; under a row_map
 * also a desc row >= n_tax): the engine's verdict on such a query is not this pass's to change.  min_cover_milli = 100000
 * drops nothing (c is the common prefix of T).  On the kept table every row of T starts with c, so a second pass finds a prefix
 * that extends c; it is NOT in general the same one: the group has shrunk, `need` with it, and a deeper taxon may now cover it
 * (10 rows at 60 %: four of species 1;2, two of 1;3, four elsewhere -> c = 1, six rows stay, and of those six 1;2 covers 60 %).
 * The contract is stated for one pass.
 * Decided on the device (csrc/cover_kernel.hip) from the engine row ids and the taxonomy's lcp8 / rmq tables alone: lineage order
 * makes a clade a range of sorted positions, a clade with more than half of T holds T's median row m by position, the levels a
 * row shares with m are a range minimum, and d* is the need-th largest of them. */
typedef struct blu_min_cover_stats {
    uint64_t n_hits;        /* rows in */
    uint64_t n_kept;        /* rows kept */
    uint64_t n_queries;
    uint64_t n_narrowed;    /* queries that lost at least one row */
    uint64_t n_unresolved;  /* queries left alone because of a top row without a usable lineage */
} blu_min_cover_stats;
/* The verdicts alone: keep_out[i] = 1 / 0, one 32-bit word per row, under seg_off[n_queries + 1]; depth_out[q] (may be NULL) = d*,
 * BLU_NONE_U8 for a query left alone (an empty segment too); stats may be NULL.  tax_row[i] is the engine row id of row i, or —
 * when row_map (blu_taxonomy_row_map's forward table, [n_tax]) is given — its desc row, mapped on the device.  The device is the
 * handle's.  on_device = 1: device pointers (row_map too); the call waits for `stream` (a hipStream_t, NULL = default), runs on
 * the default stream and returns when the outputs are complete.  on_device = 0: the columns, the map and the offsets are
 * uploaded, the same kernels run, the verdicts are copied back — there is no second implementation and no CPU fallback: a
 * host-only handle is BLU_ERR_NO_DEVICE.  Offsets beyond n_hits are clamped to it and a decreasing pair is an empty segment: a
 * corrupt table reads nothing outside the columns and the taxonomy's tables; a row that no segment names gets 0.
 * BLU_ERR_INVALID_ARG, before any device is asked for: min_cover_milli outside 50001 .. 100000 ("min cover: ..."), a NULL array
 * with a non-zero count, n_hits >= 2^32 or n_queries >= 2^32. */
int blu_hits_cover_keep(const blu_taxonomy* tax, const int32_t* bitscore, const uint32_t* tax_row, const uint32_t* row_map /* NULL: tax_row holds engine ids */,
                        const uint64_t* seg_off, uint64_t n_hits, uint64_t n_queries, int on_device, uint32_t min_cover_milli, void* stream,
                        uint32_t* keep_out, uint8_t* depth_out, blu_min_cover_stats* stats);
/* The same pass, then the compaction of the five columns and seg_off IN PLACE, as blu_hits_subject_best does it (the same code):
 * the kept rows move to the front of each column in their order, seg_off[q] becomes the number of kept rows before it.
 * *n_hits_out: the rows left; *n_unmatched_out: how many of them have tax_row == unmatched_marker (either may be NULL).  When every
 * row is kept the columns are not touched.  Device pointers must be 16-byte aligned.  Otherwise as above. */
int blu_hits_cover_apply(const blu_taxonomy* tax, int32_t* bitscore, int32_t* align_len, uint32_t* tax_row, uint32_t* acc_rank, double* pident,
                         const uint32_t* row_map, uint64_t* seg_off, uint64_t n_hits, uint64_t n_queries, int on_device,
                         uint32_t min_cover_milli, void* stream, uint32_t unmatched_marker, uint64_t* n_hits_out, uint64_t* n_unmatched_out,
                         blu_min_cover_stats* stats);

/* -------------------------------------------------------------------------- */
/* Pairwise sample distances (additive, ABI v5; not in the reference).  A feature x sample matrix of u64 counts,
 * given as CSR over the features, and for every pair of samples a, b the integers that Bray-Curtis and Jaccard are ratios of:
 *   total[a]      = sum over features f of x[f][a]                      (u64)
 *   richness[a]   = number of features with x[f][a] > 0                 (u32)
 *   min_sum[a][b] = sum over f of min(x[f][a], x[f][b])                 (u64)
 *   shared[a][b]  = number of f with x[f][a] > 0 and x[f][b] > 0        (u32)
 * The matrices are full, row-major [n_samples][n_samples] and symmetric; min_sum[a][a] = total[a], shared[a][a] = richness[a].
 * No floating point takes part: the values are exact and do not depend on the launch geometry.  Counted on the device
 * (csrc/distance_kernel.hip): the CSR is transposed by sample there, and a block that owns sample a stages BLU_DISTANCE_CHUNK
 * features of it in LDS at a time while each of its waves walks the non-zeros of one partner b after the other. */
#define BLU_DISTANCE_MAX_SAMPLES 4096u   /* n_samples above this is refused */
#define BLU_DISTANCE_CHUNK 8192u         /* features staged in LDS at a time (8 bytes each) */
#define BLU_DISTANCE_PARTNERS 64u        /* partners b of one block: 8 waves, 8 partners each */
typedef struct blu_distance_desc {
    uint32_t struct_size;      /* sizeof(blu_distance_desc) */
    int32_t device;            /* HIP device ordinal */
    uint64_t n_features;       /* below 2^31 */
    uint32_t n_samples;        /* 1 .. BLU_DISTANCE_MAX_SAMPLES */
    uint32_t reserved;
    const uint64_t* row_ptr;   /* [n_features + 1] host; non-decreasing, row_ptr[0] = 0, row_ptr[n_features] <= 2^32 - 1024 */
    const uint32_t* sample;    /* [nnz] host; ascending within a feature, each < n_samples */
    const uint64_t* count;     /* [nnz] host; each > 0 */
    void* stream;              /* a hipStream_t the call waits for before it starts (NULL = default); it runs on the default stream */
} blu_distance_desc;           /* 56 bytes */

typedef struct blu_sample_distance {
    uint32_t n_samples;
    uint32_t reserved;
    uint64_t* total;           /* [n_samples] */
    uint32_t* richness;        /* [n_samples] */
    uint64_t* min_sum;         /* [n_samples * n_samples] */
    uint32_t* shared;          /* [n_samples * n_samples] */
    double t_device_ms;        /* transpose + pair kernel on the device, by events */
} blu_sample_distance;         /* every array malloc'd by the library: blu_sample_distance_free */

/* Host arrays in, host arrays out; synchronous.  BLU_ERR_INVALID_ARG, naming the feature, before anything is uploaded or
 * launched: a sample id >= n_samples, a sample that does not ascend within its feature (unsorted or repeated), a zero count, a
 * row_ptr that decreases; and: n_samples of 0 or above BLU_DISTANCE_MAX_SAMPLES, a struct_size the library does not know,
 * n_features >= 2^31, more than 2^32 - 1024 non-zeros, a sample whose counts add up to 2^63 or more (naming the sample).  A device that
 * cannot be used is BLU_ERR_NO_DEVICE: there is no CPU fallback. */
int blu_sample_distances(const blu_distance_desc* desc, blu_sample_distance* out);
void blu_sample_distance_free(blu_sample_distance* out);

/* -------------------------------------------------------------------------- */
/* Rarefaction: every sample subsampled to one depth, without replacement (additive, ABI v5; not in the
 * reference).  The feature CSR of blu_distance_desc in, a CSR over the same features and the kept samples out.  The rule, all in
 * u64 with wrap-around:
 *   mix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *             z ^ (z >> 31)                                    (the splitmix64 step: a bijection)
 *   the reads of sample a are numbered 0 .. N_a - 1 along its non-zeros in feature order: feature f owns
 *   [start_af, start_af + x_fa), start_af = the sum of x_ga over g < f
 *   key(a, i) = mix64(i + sample_stream[a])                    (distinct for distinct i)
 *   N_a < depth: the sample is dropped; else the `depth` reads with the smallest keys are kept, x'_fa = the kept reads among
 *   feature f's ordinals.
 * Kept samples are renumbered 0 .. n_kept - 1 in their order (kept_sample gives the ids they had), zero counts are removed, a
 * feature that lost every count stays as an empty row, and every kept column sums to `depth`: the call checks that on the host
 * and returns BLU_ERR_INTERNAL naming the sample rather than a wrong table.  No sample reaching `depth` is not an error here:
 * n_kept = 0, and no device is asked for.  Selected on the device (csrc/rarefy_kernel.hip): a radix select of the depth-th smallest key over tiles of
 * BLU_RAREFY_TILE reads, then a count per non-zero; integers only, nothing depends on launch geometry or atomic order. */
#define BLU_RAREFY_TILE 65536u                /* reads of one block */
#define BLU_RAREFY_MAX_READS (1ull << 36)     /* the reads of the samples that reach `depth`, together: above is refused */
typedef struct blu_rarefy_desc {
    uint32_t struct_size;          /* sizeof(blu_rarefy_desc) */
    int32_t device;                /* HIP device ordinal */
    uint64_t n_features;           /* as in blu_distance_desc, and so are the next five */
    uint32_t n_samples;
    uint32_t reserved;
    const uint64_t* row_ptr;
    const uint32_t* sample;
    const uint64_t* count;
    const uint64_t* sample_stream; /* [n_samples] host: blu_rarefy_stream(seed, name) of each sample; no two equal */
    uint64_t depth;                /* >= 1 */
    void* stream;                  /* a hipStream_t the call waits for before it starts (NULL = default) */
} blu_rarefy_desc;                 /* 72 bytes */

typedef struct blu_rarefied {
    uint64_t n_features;
    uint32_t n_kept;
    uint32_t reserved;
    uint32_t* kept_sample;         /* [n_kept] ids in the input, ascending */
    uint64_t* row_ptr;             /* [n_features + 1] */
    uint32_t* sample;              /* [row_ptr[n_features]] 0 .. n_kept - 1, ascending within a feature */
    uint64_t* count;               /* [row_ptr[n_features]] > 0 */
    double t_device_ms;            /* transpose, select and count on the device, by events; 0 when nothing was launched */
} blu_rarefied;                    /* every array malloc'd by the library: blu_rarefied_free */

/* mix64(mix64(seed) ^ fnv1a64(name[0, len))): FNV-1a with offset 0xcbf29ce484222325 and prime 0x100000001b3.  The name is hashed,
 * not the column index: re-ordering or subsetting the columns does not change a sample's draw. */
uint64_t blu_rarefy_stream(uint64_t seed, const char* name, uint64_t len);

/* Host arrays in, host arrays out; synchronous.  BLU_ERR_INVALID_ARG before any device is asked for: whatever
 * blu_sample_distances refuses about the CSR, a struct_size the library does not know, depth = 0, a NULL sample_stream, two
 * samples with the same stream (naming both), a sample of 2^32 reads or more (naming it), more than BLU_RAREFY_MAX_READS reads
 * in the samples that reach `depth`.  A device that cannot be used is BLU_ERR_NO_DEVICE: there is no CPU fallback. */
int blu_sample_rarefy(const blu_rarefy_desc* desc, blu_rarefied* out);
void blu_rarefied_free(blu_rarefied* out);

/* -------------------------------------------------------------------------- */
/* Alpha diversity and rarefaction curves (additive, ABI v5; not in the reference).  The feature CSR of
 * blu_distance_desc in; for every sample a and every depth D_j of a strictly ascending ladder (slot j) the integers that
 * observed features, Chao1, Simpson, Shannon and Good's coverage are ratios of, taken over x'_fa(j) = exactly the kept count
 * of blu_sample_rarefy at depth D_j with the same sample_stream: the subsamples of one sample at increasing depths are nested,
 * so one pass over the reads serves every depth.  A slot with D_j > N_a is absent for that sample (present = 0, the integers 0).
 * n_depths = 0 is the raw mode: one slot per sample, x' = x, every read kept.
 *   blu_alpha_log2(x), 1 <= x: log2 x with 24 fractional bits, by squaring, all in u64 with a 128-bit product:
 *     e = bit_length(x) - 1; m = x << (63 - e); frac = 0
 *     for i = 1 .. 24: p = m * m; hi = p >> 64; if hi >= 2^63: m = hi, bit 24 - i of frac is set; else m = (p >> 63) mod 2^64
 *     L = (e << 24) | frac                                   (never above log2 x * 2^24, less than 1 unit below it; L(0) = 0)
 *   n = sum x'  (u64)   observed = #{x' > 0}   singletons = #{x' = 1}   doubletons = #{x' = 2}  (u32)
 *   sum_sq = sum x'^2  (u64)   sum_xlog = sum x' * L(x')  (u64)          (a sample has below 2^32 reads: both fit)
 * Counted on the device (csrc/alpha_kernel.hip): a radix select of all the ladder's thresholds at once, the level at which
 * every read enters over tiles of BLU_ALPHA_TILE reads, then the six sums per (sample, slot); integers only, nothing depends on
 * launch geometry or atomic order.  Before it returns the call checks that every present slot's n is D_j (raw: N_a):
 * BLU_ERR_INTERNAL naming the sample and the depth otherwise. */
#define BLU_ALPHA_MAX_DEPTHS 32u              /* n_depths above this is refused */
#define BLU_ALPHA_TILE 8192u                  /* reads of one block of the level pass: 32 bit maps of it are 32 KB of LDS */
typedef struct blu_alpha_desc {
    uint32_t struct_size;          /* sizeof(blu_alpha_desc) */
    int32_t device;                /* HIP device ordinal */
    uint64_t n_features;           /* as in blu_distance_desc, and so are n_samples, row_ptr, sample and count */
    uint32_t n_samples;
    uint32_t n_depths;             /* 0 (raw) .. BLU_ALPHA_MAX_DEPTHS */
    const uint64_t* row_ptr;
    const uint32_t* sample;
    const uint64_t* count;
    const uint64_t* sample_stream; /* [n_samples] as in blu_rarefy_desc; not read in raw mode */
    const uint64_t* depths;        /* [n_depths] each >= 1, strictly ascending */
    void* stream;                  /* a hipStream_t the call waits for before it starts (NULL = default) */
} blu_alpha_desc;                  /* 72 bytes */

typedef struct blu_alpha {
    uint32_t n_samples;
    uint32_t n_slots;              /* n_depths, or 1 in raw mode */
    uint8_t* present;              /* [n_samples * n_slots], sample-major as the next six: 1 where D_j <= N_a (raw: always) */
    uint64_t* n;
    uint32_t* observed;
    uint32_t* singletons;
    uint32_t* doubletons;
    uint64_t* sum_sq;
    uint64_t* sum_xlog;
    double t_device_ms;            /* transpose, select, levels and sums on the device, by events; 0 when nothing was launched */
} blu_alpha;                       /* every array malloc'd by the library: blu_alpha_free */

uint64_t blu_alpha_log2(uint64_t x);

/* Host arrays in, host arrays out; synchronous.  BLU_ERR_INVALID_ARG before any device is asked for: a struct_size the library
 * does not know, whatever blu_sample_distances refuses about the CSR, n_depths above BLU_ALPHA_MAX_DEPTHS, a depth of 0, depths
 * that do not strictly ascend (naming the position), with a ladder a NULL sample_stream or two samples with the same stream, a
 * sample of 2^32 reads or more (naming it), more than BLU_RAREFY_MAX_READS reads in the samples that reach depths[0].  No sample
 * reaching depths[0] is not an error here: every slot is absent and no device is asked for.  A device that cannot be used is
 * BLU_ERR_NO_DEVICE: there is no CPU fallback. */
int blu_sample_alpha(const blu_alpha_desc* desc, blu_alpha* out);
void blu_alpha_free(blu_alpha* out);

#ifdef __cplusplus
}
#endif
#endif /* BLU_CONSENSUS_H */
