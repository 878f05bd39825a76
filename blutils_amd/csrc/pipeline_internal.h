// What crosses the files of the pipeline's host side (include/blu_pipeline.h):
//   pipeline_taxdb.cpp    the taxonomies file: JSON reader, loader, binary cache, label set
//   pipeline_ingest.cpp   the CPU outfmt-6 parser, the taxon-filter resolver, the ingest entry points
//   pipeline_render.cpp   JSON / JSONL / YAML records and the text of the three tables
//   count_table.cpp       the count table of blu_consensus_extras: its parser and its join with the queries
//   pipeline.cpp          the use-case: one Run from the request to the document
#ifndef BLU_PIPELINE_INTERNAL_H
#define BLU_PIPELINE_INTERNAL_H

#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "blu_internal.h"
#include "blu_pipeline.h"
#include "ingest.h"
#include "ingest_prims.h"

namespace blu {

struct MappedFile {
    const char* data = nullptr;
    size_t size = 0;
    int fd = -1;
    bool open(const char* path) {
        fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0) return false;
        size = (size_t)st.st_size;
        if (size == 0) { data = ""; return true; }
        void* p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) return false;
        data = (const char*)p;
        return true;
    }
    void close() {
        if (data && size) munmap((void*)data, size);
        if (fd >= 0) ::close(fd);
        data = nullptr; size = 0; fd = -1;
    }
    ~MappedFile() { close(); }
};

inline bool write_text_file(const char* path, const std::string& text) {
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return false;
    const bool ok = write_all(fd, text.data(), text.size());
    if (close(fd) != 0 || !ok) { unlink(path); return false; }
    return true;
}

// ---- the taxonomies file as loaded (pipeline_taxdb.cpp) ---------------------------------------------------------------------
struct Db {
    std::vector<int64_t> taxid;
    std::vector<uint64_t> lin_off{0};
    std::vector<uint32_t> lin_node;
    std::vector<uint16_t> lin_rank;          // index into rank_raw
    std::vector<uint8_t> bad;
    std::vector<std::string> rank_raw;       // rank strings as they appear in lineages
    std::vector<std::string> rank_display;   // canonical Display of rank_raw[i]
    std::vector<std::string> node_ident;     // node id -> identifier string
    std::vector<uint16_t> node_rank;         // node id -> index into rank_display (a node is interned on (Display(rank), identifier))
    std::unordered_map<std::string, uint16_t> rank_ids;
    std::unordered_map<std::string, uint32_t> node_ids;   // key: Display(rank) + '\x1f' + identifier
    TaxidMap row_of;                         // taxid -> its (first) row
    // taxids listed more than once -> all their rows in file order.  The reference's polars left join (mod.rs:72-76) emits one
    // joined row per matching taxonomy row, so every hit of such a subject appears once per listing (load_hits does the same).
    std::unordered_map<int64_t, std::vector<uint32_t>> dup_rows;
    void note_row(int64_t taxid, uint32_t row) {
        if (row_of.emplace(taxid, row)) return;
        auto& v = dup_rows[taxid];
        if (v.empty()) v.push_back(row_of.find_or(taxid, 0));
        v.push_back(row);
    }
};
std::string canonical_display(const std::string& raw);
int load_db(const char* path, bool use_taxid, Db& db);

// ---- threads and the stage trace -----------------------------------------------------------------------------------------
inline double thread_cpu_s() { timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

inline unsigned worker_threads() {
    unsigned nthreads = std::thread::hardware_concurrency();
    if (const char* env = getenv("BLU_INGEST_THREADS")) nthreads = (unsigned)atoi(env);
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 32) nthreads = 32;
    return nthreads;
}

template <class F>
void parallel_for(unsigned n, unsigned nthreads, F&& f) {
    if (nthreads <= 1 || n <= 1) { for (unsigned i = 0; i < n; ++i) f(i); return; }
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < n; ++i) pool.emplace_back([&f, i]() { f(i); });
    for (auto& th : pool) th.join();
}

// A tree of merges over n sorted runs: merge(i, step) folds run i + step into run i, for the pairs (i, i + step) of every
// level; the pairs of one level are merged in parallel.
template <class F>
void merge_tree(unsigned n, unsigned nthreads, F&& merge) {
    for (unsigned step = 1; step < n; step *= 2) {
        std::vector<unsigned> heads;
        for (unsigned i = 0; i + step < n; i += 2 * step) heads.push_back(i);
        parallel_for((unsigned)heads.size(), nthreads, [&](unsigned k) { merge(heads[k], step); });
    }
}

// f(k) for k in [0, n), handed out one at a time to `nthreads` workers
// Returns false if a worker ran out of memory (std::bad_alloc from an output buffer): an exception must not leave a
// std::thread — that is std::terminate for the whole host process — so it is caught here and the remaining work dropped.
template <class F>
bool parallel_dynamic(size_t n, unsigned nthreads, F&& f) {
    std::atomic<bool> oom{false};
    auto guarded = [&](size_t k) { try { f(k); } catch (const std::bad_alloc&) { oom = true; } };
    if (nthreads <= 1 || n <= 1) { for (size_t k = 0; k < n && !oom; ++k) guarded(k); return !oom; }
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthreads && t < n; ++t)
        pool.emplace_back([&]() { for (size_t k = next.fetch_add(1); k < n && !oom.load(std::memory_order_relaxed); k = next.fetch_add(1)) guarded(k); });
    for (auto& th : pool) th.join();
    return !oom;
}

// stage trace (BLU_INGEST_TRACE=1): one stderr line per lap; the use-case's, or the CPU ingest's as Trace{"[ingest]", 22}
struct Trace {
    const char* const who = "[pipeline]";
    const int width = 26;
    const bool on = getenv("BLU_INGEST_TRACE") != nullptr;
    double tp = now_s();
    void lap(const char* what) { if (on) { const double t = now_s(); fprintf(stderr, "%s %-*s %.3f s\n", who, width, what, t - tp); tp = t; } }
};

// ---- CPU ingest (pipeline_ingest.cpp) --------------------------------------------------------------------------------------
int taxon_codes(const Db& db, const blu_taxon_filter& f, unsigned nthreads, TaxonCodes& tc);
// lay: the table's column layout, checked by check_table_layout on the way in; null = the reference's columns
// cov: the query cover, checked by check_query_cover on the way in; null = none
int load_hits(const char* path, const Db& db, HitTable& ht, int device = -1, bool host_columns = true, const blu_hit_filter* flt = nullptr,
              TaxonCodes* taxa = nullptr, const blu_table_layout* lay = nullptr, const blu_query_cover* cov = nullptr);
// A caller's layout before any file is opened: BLU_ERR_INVALID_ARG for a size, a count or role columns the library does not
// take, and for an e-value threshold (flt: the active hit filter, or null) over a layout without an e-value column.  *use: the
// layout the parsers are to read through, null when lay is null or names the reference's thirteen columns in their order —
// unless keep_reference: under a query cover the parsers read through the layout whatever it names.
int check_table_layout(const blu_table_layout* lay, const blu_hit_filter* flt, const blu_table_layout** use, bool keep_reference = false);
// A caller's query cover against the caller's layout, before any file is opened: BLU_ERR_INVALID_ARG for a size, a
// source, a threshold or columns the library does not take, and for a cover without a layout.  The caller's stats are zeroed.
int check_query_cover(const blu_query_cover* cov, const blu_table_layout* lay);

// One run's hit selection (include/blu_pipeline.h: blu_hit_selection) as the use-case and the
// ingest-columns call both take it: an option with an empty mask or two empty lists is absent, the taxon lists are resolved
// against the loaded lineages, and the counts are filled where the caller will read them.
struct Selection {
    const blu_hit_selection asked;                // (as the caller gave it; the four below: what of it is active)
    const blu_hit_filter* flt = nullptr;
    const blu_taxon_filter* tflt = nullptr;
    const blu_subject_best* subj = nullptr;
    const blu_score_band* band = nullptr;
    std::unique_ptr<TaxonCodes> taxa;             // (the taxon filter as the parsers read it)
    blu_hit_selection_stats own{};                // (a caller that wants no counts)
    blu_hit_selection_stats* const st;
    const blu_query_cover* cov = nullptr;         // (the query cover beside the request, checked; null = none: DESIGN.md §24)
    int64_t cover_milli = 0;                      // (blu_consensus_request.min_cover_milli; 0 = not asked for: DESIGN.md §20)
    blu_min_cover_stats cover_st{};               // (its counts: blu_last_min_cover_stats)
    bool subject_done = false, band_done = false, cover_done = false;   // (once per run, on the device columns or on the host columns)

    // the caller's counts start at zero, its excluded_by array included, whatever the call then does
    Selection(const blu_hit_selection* sel, blu_hit_selection_stats* stats) : asked(sel ? *sel : blu_hit_selection{}), st(stats ? stats : &own) {
        uint64_t* const by = st->taxon_filter.excluded_by;
        *st = blu_hit_selection_stats{};
        st->taxon_filter.excluded_by = by;
        const blu_taxon_filter* f = asked.taxon_filter;
        if (by && f && f->n_exclude <= BLU_TAXON_FILTER_MAX_EXCLUDE) for (uint64_t k = 0; k < f->n_exclude; ++k) by[k] = 0;
    }
    // before any file is opened: unknown mask bits and band values out of range are refused
    int check() {
        if (asked.hit_filter && (asked.hit_filter->mask & ~15u)) { set_error("hit filter: unknown bits in the mask"); return BLU_ERR_INVALID_ARG; }
        if (int rc = check_score_band(asked.score_band)) return rc;
        if (int rc = check_subject_best(asked.subject_best)) return rc;
        if (cover_milli != 0) if (int rc = check_min_cover(cover_milli)) return rc;
        if (asked.hit_filter && (asked.hit_filter->mask & 15u)) flt = asked.hit_filter;
        if (asked.taxon_filter && (asked.taxon_filter->n_exclude || asked.taxon_filter->n_only)) tflt = asked.taxon_filter;
        if (asked.subject_best && asked.subject_best->mask) subj = asked.subject_best;
        if (asked.score_band && asked.score_band->mask) band = asked.score_band;
        return BLU_OK;
    }
    // a taxon filter: the lists resolved against the lineages -> one code per row
    int resolve(const Db& db, unsigned nthreads) {
        if (!tflt) return BLU_OK;
        taxa = std::make_unique<TaxonCodes>();
        return taxon_codes(db, *tflt, nthreads, *taxa);
    }
    // the parser's counts, and the table as it stands before options 2 and 3
    void loaded(const HitTable& ht) {
        const bool on = flt || taxa || cov;
        st->hit_filter = blu_hit_filter_stats{on ? ht.n_lines : ht.n_hits, on ? ht.n_kept : ht.n_hits};
        if (cov && cov->stats) *cov->stats = blu_query_cover_stats{ht.n_lines, ht.n_below};
        if (taxa) {
            st->taxon_filter.n_lines = ht.n_lines; st->taxon_filter.n_excluded = taxa->n_excluded; st->taxon_filter.n_not_only = taxa->n_not_only;
            if (st->taxon_filter.excluded_by) for (uint32_t k = 0; k < taxa->n_exclude; ++k) st->taxon_filter.excluded_by[k] = taxa->excluded_by[k];
        }
        st->subject_best = blu_subject_best_stats{ht.n_hits, ht.n_hits, ht.n_queries, 0};
        st->score_band = blu_score_band_stats{ht.n_hits, 0, ht.n_queries, 0};
    }
    // Options 2 and 3 and the minimum cover on the columns the GPU ingest left on the device, each once per run, compacted or
    // raised where the engine will read them — a download after a failed device run then brings the table as they left it.
    // The best hit per subject comes before the band (§17), the cover (§20) after the band, whose rows are part
    // of the top group it reads.  The table's counts follow the kept rows.
    int on_device_columns(HitTable& ht, Trace& tr, const blu_taxonomy* tax, const uint32_t* fwd, uint64_t n_tax) {
        DeviceHits& dev = *ht.dev;
        if (subj) {
            uint64_t unmatched = ht.unmatched;
            if (int rc = subject_best_hits(dev, &st->subject_best, &unmatched)) return rc;
            ht.n_hits = dev.n_hits; ht.unmatched = unmatched;
            st->score_band.n_hits = ht.n_hits;
            subject_done = true;
            tr.lap("subject best hit (device)");
        }
        if (band) {
            if (int rc = blu_hits_score_band(dev.device, dev.bitscore, (const uint64_t*)dev.seg_off, dev.n_hits, dev.n_queries, 1, band, nullptr,
                                             dev.bitscore, &st->score_band)) return rc;
            band_done = true;
            tr.lap("score band (device)");
        }
        if (cover_milli && dev.n_hits) {
            uint64_t unmatched = ht.unmatched;
            if (int rc = cover_hits(tax, dev, fwd, n_tax, (uint32_t)cover_milli, &cover_st, &unmatched)) return rc;
            ht.n_hits = dev.n_hits; ht.unmatched = unmatched;
            cover_done = true;
            tr.lap("min cover (device)");
        }
        return BLU_OK;
    }
    // Options 2 and 3 and the minimum cover on host columns, through the host-pointer route of their kernels: whatever of the
    // three has not been applied on the device columns.  The table's counts follow the kept rows.  tax, fwd: the taxonomy handle
    // and its forward row map, which the cover needs (the ingest-columns call has neither, and no cover).
    int on_host_columns(int device, HitTable& ht, Trace* tr = nullptr, const blu_taxonomy* tax = nullptr, const uint32_t* fwd = nullptr) {
        auto shrink = [&ht](uint64_t n_out, uint64_t unmatched) {   // the rows a pass kept: the front of each column
            ht.bitscore.resize(n_out); ht.align_len.resize(n_out); ht.tax_desc_row.resize(n_out); ht.acc_rank.resize(n_out); ht.pident.resize(n_out);
            ht.n_hits = n_out; ht.unmatched = unmatched;
        };
        if (subj && !subject_done && ht.n_hits) {
            uint64_t n_out = ht.n_hits, unmatched = ht.unmatched;
            int rc = blu_hits_subject_best(device, ht.bitscore.data(), ht.align_len.data(), ht.tax_desc_row.data(), ht.acc_rank.data(),
                                           ht.pident.data(), ht.seg_off.data(), ht.n_hits, ht.n_queries, 0, subj, nullptr, BLU_UNMATCHED_TAXID,
                                           &n_out, &unmatched, &st->subject_best);
            if (rc != BLU_OK) return rc;
            shrink(n_out, unmatched);
            subject_done = true;
            st->score_band.n_hits = n_out;
            if (tr) tr->lap("subject best hit (host columns)");
        }
        if (band && !band_done && ht.n_hits) {
            int rc = blu_hits_score_band(device, ht.bitscore.data(), ht.seg_off.data(), ht.n_hits, ht.n_queries, 0, band, nullptr,
                                         ht.bitscore.data(), &st->score_band);
            if (rc != BLU_OK) return rc;
            band_done = true;
            if (tr) tr->lap("score band (host columns)");
        }
        if (cover_milli && !cover_done && tax && ht.n_hits) {
            uint64_t n_out = ht.n_hits, unmatched = ht.unmatched;
            int rc = blu_hits_cover_apply(tax, ht.bitscore.data(), ht.align_len.data(), ht.tax_desc_row.data(), ht.acc_rank.data(), ht.pident.data(),
                                          fwd, ht.seg_off.data(), ht.n_hits, ht.n_queries, 0, (uint32_t)cover_milli, nullptr, BLU_UNMATCHED_TAXID,
                                          &n_out, &unmatched, &cover_st);
            if (rc != BLU_OK) return rc;
            shrink(n_out, unmatched);
            cover_done = true;
            if (tr) tr->lap("min cover (host columns)");
        }
        return BLU_OK;
    }
};

// ---- rendering (pipeline_render.cpp) ---------------------------------------------------------------------------------------
// Output buffer of the JSON writer: the std::string calls the writers use (append / push_back / +=), inlined — a
// record is ~70 short appends, and the out-of-line call per append was a third of the rendering time.
struct Out {
    char* base = nullptr;
    size_t len = 0, cap = 0;
    Out() = default;
    Out(const Out&) = delete;
    Out& operator=(const Out&) = delete;
    Out(Out&& o) noexcept : base(o.base), len(o.len), cap(o.cap) { o.base = nullptr; o.len = o.cap = 0; }
    Out& operator=(Out&& o) noexcept { if (this != &o) { free(base); base = o.base; len = o.len; cap = o.cap; o.base = nullptr; o.len = o.cap = 0; } return *this; }
    ~Out() { free(base); }
    void reserve(size_t n) {
        if (n <= cap) return;
        char* nb = (char*)realloc(base, n);
        if (!nb) throw std::bad_alloc();
        base = nb; cap = n;
    }
    __attribute__((noinline)) void grow(size_t n) { reserve(std::max(cap * 2, len + n + 4096)); }
    __attribute__((always_inline)) inline void need(size_t n) { if (__builtin_expect(len + n > cap, 0)) grow(n); }
    __attribute__((always_inline)) inline void append(const char* p, size_t n) { need(n); memcpy(base + len, p, n); len += n; }
    __attribute__((always_inline)) inline void append(size_t n, char c) { need(n); memset(base + len, c, n); len += n; }
    __attribute__((always_inline)) inline void push_back(char c) { need(1); base[len++] = c; }
    __attribute__((always_inline)) inline Out& operator+=(const char* z) { append(z, __builtin_strlen(z)); return *this; }
    Out& operator+=(const std::string& z) { append(z.data(), z.size()); return *this; }
    void assign(const std::string& z) { len = 0; append(z.data(), z.size()); }
    const char* data() const { return base; }
    size_t size() const { return len; }
    void clear() { len = 0; }
};

// The serialized document as the pieces the workers rendered, in order: they are copied (or written) in parallel
// straight from the worker buffers, never concatenated.
struct Document {
    std::vector<Out> pieces;
    bool written = false;      // the pieces went to the output file while they were rendered (and were freed)
    bool has_report = false;   // report: the taxon report's text, written by the caller once the document is out
    std::string report;
    bool has_table = false;    // table: the per-sample table's text, written after the report
    std::string table;
    bool has_support = false;  // support: the per-query support table's text, written last
    std::string support;
    // piece k starts at byte at[k] of the document; at.back(): its size
    std::vector<size_t> offsets() const {
        std::vector<size_t> at(pieces.size() + 1, 0);
        for (size_t k = 0; k < pieces.size(); ++k) at[k + 1] = at[k] + pieces[k].size();
        return at;
    }
};

// ---- the count table (count_table.cpp) ----------------------------------------------------------------------------
// The file as parsed: the samples in column order of the sample table (ascending bytewise), the rows in file order as CSR over
// those sample ids, zeros left out.
struct CountTable {
    std::vector<std::string> samples;
    std::vector<std::string> row_names;
    std::vector<uint64_t> row_ptr{0};
    std::vector<uint32_t> sample, count;
    std::vector<uint64_t> row_sum;
};
// The rows as the run's queries carry them (blu_count_rows over the queries with hits), each query's row sum (the report's
// weight), and what counts as unclassified per sample: the rows of headers without hits and the rows no query has.
struct CountJoin {
    std::vector<uint64_t> row_ptr{0};
    std::vector<uint32_t> sample, count;
    std::vector<uint32_t> weight;
    std::vector<uint64_t> unclassified;
    uint64_t unclassified_total = 0;
};
// BLU_ERR_IO / BLU_ERR_PARSE (naming line and column)
int parse_count_table(const char* path, CountTable& t);
// joined on the names up to their first ';'; BLU_ERR_INVALID_ARG for a row sum of 2^32 or more, two rows or two queries with one
// key, and a query (with hits, or `extra`: header-only) no row has
int join_count_table(const CountTable& t, const std::vector<std::string>& query_names, const std::vector<std::string>& extra,
                     CountJoin& j, blu_count_table_stats* st);

// ---- the use-case (pipeline.cpp) -----------------------------------------------------------------------------------------------
struct Item { const std::string* name; int64_t q; };   // one result of the document; q < 0: a header without hits

// One call of the use-case: the request, and what its steps hand from one to the next.  It owns what goes to the graveyard
// thread at the end (bury), and whatever of it is left when a step fails.
struct Run {
    const blu_consensus_request& rq;
    const blu_consensus_extras* const ex;          // (NULL: none)
    const blu_table_layout* lay;                   // (the table's column layout; NULL once start() has checked it: the reference's columns)
    const blu_query_cover* const cov;              // (the query cover; NULL: none)
    const blu_pipeline_params* const params;
    Selection sel;
    blu_pipeline_stats st{};
    Trace tr;
    const unsigned nthreads = worker_threads();
    double t0 = 0;                                 // (start of the stage st is timing)
    std::thread warm_up;                           // (HIP start-up beside the reading of the taxonomy file)
    std::unique_ptr<Db> db = std::make_unique<Db>();               // (on the heap, as the hit table: handed to the graveyard)
    std::unique_ptr<HitTable> ht = std::make_unique<HitTable>();
    blu_taxonomy* tax = nullptr;
    std::vector<uint32_t> fwd;                     // blu_taxonomy_row_map's forward table
    Column<blu_result> recs;                       // (not zero-filled: the engine writes every record; the fresh pages are touched by
    TopTable top;                                  //  the threads that copy the records back)
    bool on_device = false, done_on_device = false;   // the engine is to read the device columns; it did
    DeviceRecords kept;                            // (the device records, for the tables)
    std::vector<uint32_t> eng_rows;                // (the host path's engine row ids, for the tables)
    std::vector<std::string> extra;                // headers without hits (mod.rs:86-102)
    std::vector<Item> items;                       // results + extra, sorted by query (write_blutils_output.rs:111)
    std::unique_ptr<CountTable> counts;            // (the count table, when the extras name one, and its join with the queries)
    CountJoin joined;

    Run(const blu_consensus_request& request, const blu_consensus_extras* extras, const blu_table_layout* layout, const blu_query_cover* cover,
        blu_consensus_outcome* outcome)
        : rq(request), ex(extras), lay(layout), cov(cover), params(request.params), sel(&request.selection, &outcome->selection) {}
    ~Run() { if (warm_up.joinable()) warm_up.join(); if (tax) blu_taxonomy_destroy(tax); }
    // the steps of build_document, in order; each returns an error code
    int start();
    int taxonomy_beside_ingest();
    int select_on_device();
    int engine();
    int engine_on_host_columns();
    int order();
    int count_table();
    int tables(Document* document);
    int render(Document* document);
    void bury();
};

void top_rows_from_columns(const HitTable& ht, const Column<blu_result>& recs, unsigned nthreads, TopTable& top);
std::string uuid_v4();
const char* status_site(uint8_t st);
bool size_weight(std::string_view name, uint32_t* w);
bool sample_of(std::string_view name, std::string_view* out);
std::string render_report(const Db& db, const blu_report& rep);
std::string render_sample_table(const Db& db, const blu_sample_table& tab, const std::vector<std::string_view>& names);
// one line per item from the counts of its query (sup[q]; zeros for a header without hits)
std::string render_support(const Run& r, const std::vector<blu_support>& sup);
// The document's records.  YAML is one text; JSON / JSON-compact / JSONL are a head, the items [i0, i1) appended to a
// worker's buffer block by block, and a tail.  run_id_json: the run id as a JSON string.
std::string render_yaml(const Run& r, const std::string& run_id, const std::string& cfg);
void render_head(int32_t format, const std::string& cfg, Out& head);
void render_block(const Run& r, const std::string& run_id_json, size_t i0, size_t i1, Out& po);
void render_tail(int32_t format, const std::string& cfg, bool any_items, Out& tail);

}  // namespace blu
#endif
