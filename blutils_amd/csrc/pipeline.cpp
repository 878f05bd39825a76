// Host-side drop-in for `build_consensus_identities` + the result writer (include/blu_pipeline.h): the use-case.  The
// taxonomies file, the CPU ingest and the rendering are files of their own (pipeline_internal.h).  Reference files followed:
//   core/src/use_cases/build_consensus_identities/mod.rs:40-129   orchestration, headers without hits
//   use_cases/write_blutils_output.rs:57-63,82-85,111   the output file replaced, the run id, sort by query
#include <condition_variable>
#include <mutex>

#include "pipeline_internal.h"

namespace blu {
namespace {

// The memory of a finished use-case call (the hit table's strings, the records, the top rows, the taxonomy DB: 30 ms of
// free() and munmap() for a 2 M-query table) is given back by a thread of its own instead of on the caller's path.  At most
// one such thread exists: the next call that has something to release joins it first, and so does the unloading of the
// library.
struct Graveyard {
    std::mutex mu;
    std::thread t;
    void bury(std::thread&& next) { std::lock_guard<std::mutex> lk(mu); if (t.joinable()) t.join(); t = std::move(next); }
    void drain() { std::lock_guard<std::mutex> lk(mu); if (t.joinable()) t.join(); }
    ~Graveyard() { if (t.joinable()) t.join(); }
};
Graveyard g_graveyard;

thread_local double g_t_body_end = 0;   // stage trace: when build_document's last statement ran (what follows is its tear-down)
// the minimum cover's counts (blu_last_min_cover_stats): of the run under way, and of the last run once it has succeeded
thread_local blu_min_cover_stats g_cover_pending{}, g_last_min_cover{};

// ---- the three tables: the weights and sample ids from the names, the device pass over the run's records (in place on the
// device path; uploaded by the kernels' host-pointer route on the host path), the text ------------------------------------------
// Under `size` weighting: w for the queries and extra_w for the headers without hits (weight one: w empty, extra_w all 1).
int size_weights(const Run& r, std::vector<uint32_t>& w, std::vector<uint32_t>& extra_w) {
    extra_w.assign(r.extra.size(), 1);
    if (r.counts) { w = r.joined.weight; return BLU_OK; }   // (a count table: the row sums; what is unclassified beside the records: build_report)
    if (r.rq.weight != BLU_REPORT_WEIGHT_SIZE) return BLU_OK;
    w.resize(r.recs.size());
    for (size_t k = 0; k < w.size() + extra_w.size(); ++k) {
        const std::string& name = k < w.size() ? r.ht->query_names[k] : r.extra[k - w.size()];
        if (!size_weight(name, k < w.size() ? &w[k] : &extra_w[k - w.size()])) { set_error("query `%s`: its size is 2^32 or more", name.c_str()); return BLU_ERR_INVALID_ARG; }
    }
    return BLU_OK;
}

// the run's records and engine rows as the report kernels read them: on the device, or for the host-pointer route
ReportInput device_records(const Run& r, const uint32_t* d_w) { return ReportInput{r.kept.recs, r.recs.size(), r.kept.rows, r.ht->n_hits, r.kept.row_stride, false, d_w}; }
blu_hits host_rows(const Run& r) {
    blu_hits h{};
    h.tax_row = r.eng_rows.data(); h.n_hits = r.eng_rows.size(); h.n_queries = r.recs.size(); h.on_device = 0;
    return h;
}

// The report (blu_consensus_request.report_path): the header-only queries count as unclassified.
int build_report(const Run& r, std::string& text) {
    const uint64_t nq = r.recs.size();
    std::vector<uint32_t> w, extra_w;
    if (int rc = size_weights(r, w, extra_w)) return rc;
    blu_report rep{};
    struct Free { blu_report& r; ~Free() { blu_report_free(&r); } } free_rep{rep};
    int rc;
    if (r.done_on_device && nq) {
        HipPolicy pol{"report", BLU_ERR_ALLOC};
        DeviceArena mem(pol);
        uint32_t* d_w = nullptr;
        if (!w.empty()) HIP_CHECK(pol, mem.upload(&d_w, w.data(), nq, "weights"));
        rc = report_device(r.tax, device_records(r, d_w), &rep);
    } else {
        const blu_hits h = host_rows(r);
        rc = blu_consensus_report(r.tax, &h, r.recs.data(), w.empty() ? nullptr : w.data(), nullptr, &rep);
    }
    if (rc != BLU_OK) return rc;
    if (r.counts) { rep.unclassified += r.joined.unclassified_total; rep.total += r.joined.unclassified_total; }
    else for (uint32_t x : extra_w) { rep.unclassified += x; rep.total += x; }
    text = render_report(*r.db, rep);
    return BLU_OK;
}

// The per-sample table with a count table: the columns are the table's samples, a query adds the counts of its
// row, and the rows of header-only queries and of no query at all count as unclassified.
int build_count_sample_table(const Run& r, std::string& text) {
    const uint64_t nq = r.recs.size();
    const CountJoin& j = r.joined;
    const uint32_t ns = (uint32_t)r.counts->samples.size();
    blu_sample_table tab{};
    struct Free { blu_sample_table& t; ~Free() { blu_sample_table_free(&t); } } free_tab{tab};
    int rc;
    if (r.done_on_device && nq) {
        HipPolicy pol{"count table", BLU_ERR_ALLOC};
        DeviceArena mem(pol);
        uint64_t* d_ptr = nullptr;
        uint32_t *d_s = nullptr, *d_c = nullptr;
        HIP_CHECK(pol, mem.upload(&d_ptr, j.row_ptr.data(), j.row_ptr.size(), "row offsets"));
        HIP_CHECK(pol, mem.upload(&d_s, j.sample.data(), j.sample.size(), "sample ids"));
        HIP_CHECK(pol, mem.upload(&d_c, j.count.data(), j.count.size(), "counts"));
        rc = sample_table_counts_device(r.tax, device_records(r, nullptr), CountRows{d_ptr, d_s, d_c, j.sample.size()}, ns, &tab);
    } else {
        const blu_hits h = host_rows(r);
        const blu_count_rows rows{j.row_ptr.data(), j.sample.data(), j.count.data()};
        rc = blu_consensus_sample_table_counts(r.tax, &h, r.recs.data(), &rows, ns, nullptr, &tab);
    }
    if (rc != BLU_OK) return rc;
    for (uint32_t s = 0; s < ns; ++s) tab.unclassified[s] += j.unclassified[s];
    std::vector<std::string_view> names(r.counts->samples.begin(), r.counts->samples.end());
    text = render_sample_table(*r.db, tab, names);
    return BLU_OK;
}

// The per-sample table (blu_consensus_request.sample_table_path): the samples from the query names and the header-only names
// (ids in ascending byte order = column order); the header-only queries count as unclassified in their sample.
int build_sample_table(const Run& r, std::string& text) {
    if (r.counts) return build_count_sample_table(r, text);
    const std::vector<std::string>& extra = r.extra;
    const uint64_t nq = r.recs.size();
    std::vector<uint32_t> sid(nq + extra.size());
    std::vector<std::string_view> names;          // in order of first appearance, then sorted
    {
        std::unordered_map<std::string_view, uint32_t> seen;
        std::string_view last;
        uint32_t last_id = 0;
        for (uint64_t k = 0; k < sid.size(); ++k) {
            const std::string& name = k < nq ? r.ht->query_names[k] : extra[k - nq];
            std::string_view smp;
            if (!sample_of(name, &smp)) {
                set_error("query `%s` names no sample: neither a `sample=` field nor a `<sample>.<digits>` label", name.c_str());
                return BLU_ERR_INVALID_ARG;
            }
            // (a pooled file is per-sample files back to back: the previous query's sample first)
            if (names.empty() || smp != last) {
                auto it = seen.emplace(smp, (uint32_t)names.size());
                if (it.second) names.push_back(smp);
                last = smp;
                last_id = it.first->second;
            }
            sid[k] = last_id;
        }
        std::vector<uint32_t> order(names.size()), rank(names.size());
        for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
        std::vector<std::string_view> sorted(names.size());
        for (uint32_t k = 0; k < order.size(); ++k) { rank[order[k]] = k; sorted[k] = names[order[k]]; }
        names.swap(sorted);
        for (uint32_t& x : sid) x = rank[x];
    }
    const uint32_t ns = (uint32_t)names.size();
    std::vector<uint32_t> w, extra_w;
    if (int rc = size_weights(r, w, extra_w)) return rc;
    blu_sample_table tab{};
    struct Free { blu_sample_table& t; ~Free() { blu_sample_table_free(&t); } } free_tab{tab};
    int rc;
    if (r.done_on_device && nq) {
        HipPolicy pol{"sample table", BLU_ERR_ALLOC};
        DeviceArena mem(pol);
        uint32_t *d_w = nullptr, *d_s = nullptr;
        if (!w.empty()) HIP_CHECK(pol, mem.upload(&d_w, w.data(), nq, "weights"));
        HIP_CHECK(pol, mem.upload(&d_s, sid.data(), nq, "sample ids"));
        rc = sample_table_device(r.tax, device_records(r, d_w), d_s, ns, &tab);
    } else {
        const blu_hits h = host_rows(r);
        rc = blu_consensus_sample_table(r.tax, &h, r.recs.data(), w.empty() ? nullptr : w.data(), sid.data(), ns, nullptr, &tab);
    }
    if (rc != BLU_OK) return rc;
    for (size_t k = 0; k < extra.size(); ++k) tab.unclassified[sid[nq + k]] += extra_w[k];
    text = render_sample_table(*r.db, tab, names);
    return BLU_OK;
}

// The support table (blu_consensus_request.support_table_path): the counts of every query, then one line per
// result in the document's order.
int build_support(const Run& r, std::string& text) {
    const HitTable& ht = *r.ht;
    const uint64_t nq = r.recs.size();
    std::vector<blu_support> sup(nq);
    if (r.done_on_device && nq) {
        HipPolicy pol{"support", BLU_ERR_ALLOC};
        DeviceArena mem(pol);
        blu_support* d_sup = nullptr;
        HIP_CHECK(pol, mem.alloc(&d_sup, nq * sizeof(blu_support), "counts"));
        SupportInput in{r.kept.recs, nq, (const uint64_t*)ht.dev->seg_off, ht.dev->bitscore, r.kept.rows, r.kept.row_stride, ht.n_hits};
        if (int rc = support_device(r.tax, in, d_sup)) return rc;
        HIP_CHECK(pol, hipMemcpy(sup.data(), d_sup, nq * sizeof(blu_support), hipMemcpyDeviceToHost));
    } else if (nq) {
        blu_hits h = host_rows(r);
        h.bitscore = ht.bitscore.data();
        h.seg_off = ht.seg_off.data();
        if (int rc = blu_consensus_support(r.tax, &h, r.recs.data(), nullptr, sup.data())) return rc;
    }
    text = render_support(r, sup);
    return BLU_OK;
}

// The output file's writer: a thread that sends the finished pieces out in order while the later ones are being rendered,
// and hands their buffers back to the renderers.  However the owner leaves — an exception of its own included — the writer
// is released (every piece counts as ready, nothing more is written) and joined: a joinable std::thread must not be
// destroyed, and the writer must not wait for pieces that never come.
class PieceWriter {
    std::vector<Out>& pieces;
    int fd = -1;
    std::thread old_file;       // releases the replaced file's pages off the caller's path
    std::thread writer;
    std::vector<uint8_t> ready;
    std::vector<Out> pool;      // buffers the writer is done with, taken again by the renderers (guarded by mu)
    std::mutex mu;
    std::condition_variable cv;
    bool write_ok = true;

public:
    double t_write = 0;         // inside write(), in all (read after finish())
    explicit PieceWriter(std::vector<Out>& p) : pieces(p), ready(p.size(), 0) {}
    ~PieceWriter() {
        if (writer.joinable()) {
            { std::lock_guard<std::mutex> lk(mu); write_ok = false; std::fill(ready.begin(), ready.end(), (uint8_t)1); }
            cv.notify_all();
            writer.join();
        }
        if (fd >= 0) close(fd);
        if (old_file.joinable()) old_file.join();
    }
    bool is_open() const { return fd >= 0; }
    // write_blutils_output.rs:58-63: an existing file is removed, then a new one created.  (Truncating it in place instead
    // makes ext4 allocate and flush the new blocks inside close().)  The old inode is held open across the unlink, so that
    // dropping its pages happens in close(old) on a thread of its own.  Only a regular file is replaced that way: a FIFO would
    // block in open(O_RDONLY), and a device node (/dev/stdout, /dev/null) must be written to, not deleted.
    int open(const char* out_path) {
        struct stat sb;
        if (stat(out_path, &sb) == 0 && S_ISREG(sb.st_mode)) {
            const int old = ::open(out_path, O_RDONLY | O_NONBLOCK);
            if (old >= 0) {
                if (unlink(out_path) != 0) { close(old); set_error("cannot replace %s", out_path); return BLU_ERR_IO; }
                old_file = std::thread([old]() { close(old); });
            }
        }
        fd = ::open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) { set_error("cannot write %s", out_path); return BLU_ERR_IO; }
        writer = std::thread([this]() {
            for (size_t k = 0; k < pieces.size(); ++k) {
                { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return ready[k] != 0; }); }
                const double ts = now_s();
                if (write_ok && !write_all(fd, pieces[k].data(), pieces[k].size())) write_ok = false;
                t_write += now_s() - ts;
                pieces[k].clear();
                std::lock_guard<std::mutex> lk(mu);
                pool.push_back(std::move(pieces[k]));
            }
        });
        return BLU_OK;
    }
    void publish(size_t k) { { std::lock_guard<std::mutex> lk(mu); ready[k] = 1; } cv.notify_all(); }
    // a buffer the writer has handed back, or an empty one
    Out spare() {
        Out o;
        if (fd >= 0) { std::lock_guard<std::mutex> lk(mu); if (!pool.empty()) { o = std::move(pool.back()); pool.pop_back(); } }
        return o;
    }
    // once every piece is published: false when a write or the close failed
    bool finish(Trace& tr) {
        writer.join();
        tr.lap("wait for the writer");
        const bool closed = close(fd) == 0;
        fd = -1;
        return closed && write_ok;
    }
};

// stable sort by name: sorted runs per worker, then a tree of stable merges
void sort_items(std::vector<Item>& items, unsigned nthreads) {
    auto less = [](const Item& a, const Item& b) { return *a.name < *b.name; };
    const unsigned nt = items.size() < 65536 ? 1 : nthreads;
    const size_t n = items.size();
    // BLAST writes its queries in the order of the FASTA file, which is often sorted already: checked first (in slices)
    std::atomic<bool> sorted{true};
    parallel_for(nt, nt, [&](unsigned t) {
        const size_t i0 = n * t / nt, i1 = std::min(n, n * (t + 1) / nt + 1);
        if (i1 > i0 && !std::is_sorted(items.begin() + i0, items.begin() + i1, less)) sorted = false;
    });
    if (sorted) return;
    if (nt == 1) { std::stable_sort(items.begin(), items.end(), less); return; }
    parallel_for(nt, nt, [&](unsigned t) { std::stable_sort(items.begin() + n * t / nt, items.begin() + n * (t + 1) / nt, less); });
    merge_tree(nt, nt, [&](unsigned t, unsigned w) {
        std::inplace_merge(items.begin() + n * t / nt, items.begin() + n * (t + w) / nt, items.begin() + n * std::min(t + 2 * w, nt) / nt, less);
    });
}

}  // namespace

// ---- the steps of one run ----------------------------------------------------------------------------------------------------
int Run::start() {
    if (!rq.blast_output_file || !rq.taxonomies_file || !params) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    sel.cover_milli = rq.min_cover_milli;
    if (int rc = sel.check()) return rc;
    if (int rc = check_query_cover(cov, lay)) return rc;
    if (int rc = check_table_layout(lay, sel.flt, &lay, cov != nullptr)) return rc;
    sel.cov = cov;
    if ((rq.report_path || rq.sample_table_path) && rq.weight != BLU_REPORT_WEIGHT_ONE && rq.weight != BLU_REPORT_WEIGHT_SIZE) {
        set_error("report: a path and weight BLU_REPORT_WEIGHT_ONE or BLU_REPORT_WEIGHT_SIZE are needed");
        return BLU_ERR_INVALID_ARG;
    }
    if (ex && ex->count_table_path) {
        if (!rq.report_path && !rq.sample_table_path) { set_error("count table: neither a report nor a sample table is asked for"); return BLU_ERR_INVALID_ARG; }
        if (rq.weight != BLU_REPORT_WEIGHT_ONE) { set_error("count table: the weight must be BLU_REPORT_WEIGHT_ONE (the counts are the table's)"); return BLU_ERR_INVALID_ARG; }
    }
    g_graveyard.drain();   // (a previous call's memory — device memory too — is back before this one sizes itself against what is free)
    t0 = now_s();
    // (HIP start-up beside the reading of the taxonomy file; BLU_INGEST=cpu callers with no device never get here with one)
    if (params->device >= 0) warm_up = std::thread([dev = params->device]() { warm_up_device(dev); });
    if (int rc = load_db(rq.taxonomies_file, params->use_taxid != 0, *db)) return rc;     // mod.rs:64
    if (int rc = sel.resolve(*db, nthreads)) return rc;
    st.t_load_db_s = now_s() - t0;
    tr.lap("load db");
    return BLU_OK;
}

// the taxonomy table (sorted lineages, cutoff tables, upload) is built by a second thread while the hits are ingested
int Run::taxonomy_beside_ingest() {
    std::vector<const char*> names;
    for (auto& s : db->rank_raw) names.push_back(s.c_str());
    blu_taxonomy_desc desc{};
    desc.n_tax = db->taxid.size(); desc.taxid = db->taxid.data(); desc.bad = db->bad.data();
    desc.lin_off = db->lin_off.data(); desc.lin_node = db->lin_node.data(); desc.lin_rank = db->lin_rank.data();
    desc.n_ranks = (uint32_t)names.size(); desc.rank_names = names.data();
    fwd.assign(std::max<size_t>(db->taxid.size(), 1), 0);
    int tax_rc = BLU_OK;
    std::string tax_err;
    double t_tax = 0;
    auto create = [&]() {
        tax_rc = blu_taxonomy_create(&desc, &params->cutoffs, params->device, &tax);
        if (tax_rc == BLU_OK) blu_taxonomy_row_map(tax, fwd.data(), nullptr);
        else { char b[1024]; blu_last_error(b, sizeof b); tax_err = b; }
    };
    std::thread tax_thread([&]() { const double ts = now_s(); create(); t_tax = now_s() - ts; });
    struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join_tax{tax_thread};
    t0 = now_s();
    if (int rc = load_hits(rq.blast_output_file, *db, *ht, params->device, /*host_columns=*/false, sel.flt, sel.taxa.get(), lay, cov)) return rc;   // mod.rs:54, 72-82
    sel.loaded(*ht);
    st.t_load_hits_s = now_s() - t0;
    tr.lap("load hits");
    st.n_hits = ht->n_hits; st.n_queries = ht->n_queries; st.n_taxids = db->taxid.size(); st.n_unmatched_rows = ht->unmatched;

    t0 = now_s();
    tax_thread.join();
    if (tax_rc == BLU_ERR_HIP || tax_rc == BLU_ERR_ALLOC) {
        // the table was built while the ingest held its work buffers (sized from a snapshot of the free memory that did not
        // know about it): on a nearly full card that can fail where the sequential order would not have — once more, now
        // that the ingest has handed its buffers back
        if (tr.on) fprintf(stderr, "[pipeline] taxonomy create failed beside the ingest (%s): once more\n", tax_err.c_str());
        create();
    }
    if (tax_rc != BLU_OK) { set_error("%s", tax_err.c_str()); return tax_rc; }
    if (tr.on) fprintf(stderr, "[pipeline] (taxonomy create, 2nd thread %.3f s)\n", t_tax);
    tr.lap("wait for the taxonomy");
    return BLU_OK;
}

// the hit selection on the columns the GPU ingest left on the device, when the engine is to read them there
int Run::select_on_device() {
    recs.resize(ht->n_queries);
    // (BLU_PIPELINE_HOST_COLUMNS=1, tests: take the host-column route although the device path would work)
    const bool force_host = getenv("BLU_PIPELINE_HOST_COLUMNS") != nullptr;
    if (force_host && ht->dev) if (int rc = download_columns(*ht)) return rc;
    on_device = ht->dev && !recs.empty() && !force_host;
    return on_device ? sel.on_device_columns(*ht, tr, tax, fwd.data(), db->taxid.size()) : BLU_OK;
}

int Run::engine() {
    if (on_device) {
        // the GPU ingest left the grouped columns on the device: the engine reads them in place and only the records and
        // the top-score rows come back (if that fails — e.g. no room for the work buffers — the columns are downloaded and
        // go through the staging path below)
        done_on_device = device_run_consensus(tax, *ht->dev, fwd.data(), db->taxid.size(), params->strategy, recs.data(), &top, &kept) == BLU_OK;   // mod.rs:104-128
        if (!done_on_device) if (int rc = download_columns(*ht)) return rc;
    }
    // (the device columns and the engine's work buffers stay with the hit table: they are freed off the caller's path at the end)
    if (!done_on_device) {
        ht->dev.reset();
        if (int rc = engine_on_host_columns()) return rc;
    }
    if (sel.subject_done || sel.cover_done) { st.n_hits = ht->n_hits; st.n_unmatched_rows = ht->unmatched; }
    if (sel.cover_milli && !sel.cover_done) sel.cover_st = blu_min_cover_stats{ht->n_hits, ht->n_hits, ht->n_queries, 0, 0};   // (an empty table)
    g_cover_pending = sel.cover_st;
    st.t_engine_s = now_s() - t0;
    tr.lap("engine + top rows");
    return BLU_OK;
}

// the host columns (the CPU ingest, or a download): what is left of the selection, the engine's staging path, the top rows
int Run::engine_on_host_columns() {
    HitTable& ht = *this->ht;
    if (int rc = sel.on_host_columns(params->device, ht, &tr, tax, fwd.data())) return rc;
    eng_rows.resize(ht.tax_desc_row.size());
    for (size_t i = 0; i < eng_rows.size(); ++i)
        eng_rows[i] = ht.tax_desc_row[i] == BLU_UNMATCHED_TAXID ? BLU_UNMATCHED_TAXID : fwd[ht.tax_desc_row[i]];
    if (!recs.empty()) {
            blu_hits h{};
            h.bitscore = ht.bitscore.data(); h.tax_row = eng_rows.data();
            // 20 B/hit layout when every perc_identity is exactly k/1000 (BLAST prints <= 3 decimals): verified per value,
            // so the engine's fl(k / 1000.0) is bit-identical to the parsed f64; otherwise the f64 column goes over.
            std::vector<uint32_t> milli(ht.pident.size());
            bool exact = true;
            for (size_t i = 0; i < milli.size() && exact; ++i) {
                const double p = ht.pident[i];
                if (!(p >= 0.0 && p < 4.0e6)) { exact = false; break; }
                const uint32_t k = (uint32_t)(p * 1000.0 + 0.5);
                const double back = (double)k / 1000.0;
                exact = memcmp(&back, &p, 8) == 0;
                milli[i] = k;
            }
            if (exact) h.pident_milli = milli.data(); else h.pident = ht.pident.data();
            h.align_len = ht.align_len.data(); h.acc_rank = ht.acc_rank.data(); h.seg_off = ht.seg_off.data();
            h.n_hits = ht.bitscore.size(); h.n_queries = ht.n_queries; h.on_device = 0;
            blu_run_params rp{params->strategy, 0, nullptr};
        if (int rc = blu_consensus_run(tax, &h, &rp, recs.data())) return rc;             // mod.rs:104-128
    }
    top_rows_from_columns(ht, recs, nthreads, top);
    return BLU_OK;
}

// results + headers without hits (mod.rs:86-102), sorted by query (write_blutils_output.rs:111)
int Run::order() {
    t0 = now_s();
    ht->wait_strings();
    if (!ht->strings_ok) { set_error("out of memory while building the query / accession strings"); return BLU_ERR_ALLOC; }
    tr.lap("wait for the strings");
    const std::vector<std::string>& names = ht->query_names;
    items.reserve(names.size());
    for (size_t q = 0; q < names.size(); ++q) items.push_back({&names[q], (int64_t)q});
    if (rq.headers) {
        std::unordered_map<std::string, uint32_t> have;
        for (size_t q = 0; q < names.size(); ++q) have.emplace(names[q], (uint32_t)q);
        extra.reserve(rq.n_headers);
        for (uint64_t i = 0; i < rq.n_headers; ++i)
            if (!have.count(rq.headers[i])) extra.emplace_back(rq.headers[i]);
        for (auto& s : extra) items.push_back({&s, -1});
    }
    sort_items(items, nthreads);
    tr.lap("sort by query");
    for (const Item& it : items) {
        if (it.q < 0) continue;
        const uint8_t s = recs[(size_t)it.q].status;
        if (s >= 16 && !params->lenient) {
            set_error("query `%s`: %s", it.name->c_str(), status_site(s));
            return BLU_ERR_REFERENCE_PANIC;
        }
    }
    return BLU_OK;
}

// the count table, when the extras name one: parsed and joined with the results' names before any table is built
int Run::count_table() {
    if (!ex || !ex->count_table_path) return BLU_OK;
    counts = std::make_unique<CountTable>();
    if (int rc = parse_count_table(ex->count_table_path, *counts)) return rc;
    if (int rc = join_count_table(*counts, ht->query_names, extra, joined, ex->count_table_stats)) return rc;
    tr.lap("count table");
    return BLU_OK;
}

// the tables that were asked for, from the records while they (on the device path: and the engine rows) are still on the device
int Run::tables(Document* d) {
    if (rq.report_path) {
        if (int rc = build_report(*this, d->report)) return rc;
        d->has_report = true;
        tr.lap("report");
    }
    if (rq.sample_table_path) {
        if (int rc = build_sample_table(*this, d->table)) return rc;
        d->has_table = true;
        tr.lap("sample table");
    }
    if (rq.support_table_path) {
        if (int rc = build_support(*this, d->support)) return rc;
        d->has_support = true;
        tr.lap("support table");
    }
    return BLU_OK;
}

// rq.out_path != nullptr: the document is written there (an existing file is replaced, write_blutils_output.rs:57-63) by a
// writer thread that follows the renderers piece by piece; otherwise the pieces are left in `document` (YAML: always).
int Run::render(Document* document) {
    const int32_t format = params->out_format;
    // write_blutils_output.rs:82-85: the config's run id, or a fresh one
    const std::string run_id = (rq.run_id_text && *rq.run_id_text) ? std::string(rq.run_id_text) : uuid_v4();
    const std::string cfg = (rq.config_text && *rq.config_text) ? std::string(rq.config_text) : std::string();
    std::vector<Out>& pieces = document->pieces;
    pieces.clear();
    if (format == BLU_OUT_YAML) {
        pieces.emplace_back();
        pieces.back().assign(render_yaml(*this, run_id, cfg));
        st.t_render_s = now_s() - t0;
        return BLU_OK;
    }
    // records are independent: blocks of the sorted list are rendered by worker threads, one piece per block, between a head
    // and a tail
    const size_t block = 4096, n_blocks = (items.size() + block - 1) / block;
    pieces.resize(n_blocks + 2);
    render_head(format, cfg, pieces.front());
    std::string run_id_json;
    json_str(run_id_json, run_id);
    PieceWriter out(pieces);
    if (rq.out_path) if (int rc = out.open(rq.out_path)) return rc;
    out.publish(0);
    std::atomic<uint64_t> cpu_us{0};
    std::atomic<bool> render_oom{false};   // a worker ran out of memory: its piece and all later ones are published empty (the writer must not wait for them)
    parallel_dynamic(n_blocks, items.size() < 4096 ? 1 : nthreads, [&](size_t bk) {
        if (render_oom.load(std::memory_order_relaxed)) { out.publish(bk + 1); return; }
        try {
            const double tc = thread_cpu_s();
            Out po = out.spare();
            render_block(*this, run_id_json, bk * block, std::min(items.size(), (bk + 1) * block), po);
            pieces[bk + 1] = std::move(po);
            cpu_us += (uint64_t)((thread_cpu_s() - tc) * 1e6);
        } catch (const std::bad_alloc&) { render_oom = true; }
        out.publish(bk + 1);
    });
    render_tail(format, cfg, !items.empty(), pieces.back());
    out.publish(pieces.size() - 1);
    if (tr.on) fprintf(stderr, "[pipeline] (render workers: %.3f s of CPU time in all)\n", (double)cpu_us.load() * 1e-6);
    tr.lap("render");
    if (out.is_open()) {
        const bool ok = out.finish(tr);
        if (render_oom) { set_error("out of memory while rendering the results"); return BLU_ERR_ALLOC; }
        if (!ok) { set_error("cannot write %s", rq.out_path); return BLU_ERR_IO; }
        document->written = true;
        if (tr.on) fprintf(stderr, "[pipeline] (writer thread: %.3f s inside write())\n", out.t_write);
        tr.lap("close file");
    }
    if (render_oom) { set_error("out of memory while rendering the results"); return BLU_ERR_ALLOC; }
    st.t_render_s = now_s() - t0;
    return BLU_OK;
}

// the big objects and the taxonomy handle (whose 2 GB of packed staging take 25 ms to hipFree) go to the graveyard thread;
// if it cannot be started they die here, as they would have anyway
void Run::bury() {
    blu_taxonomy* const tax_to_free = tax;
    tax = nullptr;
    try {
        g_graveyard.bury(std::thread([tax_to_free, db = std::move(db), ht = std::move(ht), recs = std::move(recs), top = std::move(top),
                                      items = std::move(items)]() mutable { blu_taxonomy_destroy(tax_to_free); }));
    } catch (...) { blu_taxonomy_destroy(tax_to_free); }
    tr.lap("hand the memory to its thread");
}

namespace {

int build_document(const blu_consensus_request& rq, const blu_consensus_extras* ex, const blu_table_layout* lay, const blu_query_cover* cov,
                   Document* document, blu_consensus_outcome* outcome) {
    Run r(rq, ex, lay, cov, outcome);
    if (int rc = r.start()) return rc;
    if (int rc = r.taxonomy_beside_ingest()) return rc;
    if (int rc = r.select_on_device()) return rc;
    if (int rc = r.engine()) return rc;
    if (int rc = r.order()) return rc;
    if (int rc = r.count_table()) return rc;
    if (int rc = r.tables(document)) return rc;
    if (int rc = r.render(document)) return rc;
    outcome->stats = r.st;
    r.bury();
    g_t_body_end = now_s();
    return BLU_OK;
}

// the report, then the per-sample table, then the support table, after the document
int put_tables(const Document& d, const blu_consensus_request& rq) {
    if (d.has_report && !write_text_file(rq.report_path, d.report)) { set_error("cannot write %s", rq.report_path); return BLU_ERR_IO; }
    if (d.has_table && !write_text_file(rq.sample_table_path, d.table)) { set_error("cannot write %s", rq.sample_table_path); return BLU_ERR_IO; }
    if (d.has_support && !write_text_file(rq.support_table_path, d.support)) { set_error("cannot write %s", rq.support_table_path); return BLU_ERR_IO; }
    return BLU_OK;
}

// rq.out_path == NULL: the pieces joined into one malloc'd text
int consensus_to_text(const blu_consensus_request& rq, const blu_consensus_extras* ex, const blu_table_layout* lay, const blu_query_cover* cov,
                      blu_consensus_outcome* outcome) {
    Document d;
    int rc = build_document(rq, ex, lay, cov, &d, outcome);
    if (rc != BLU_OK) return rc;
    if ((rc = put_tables(d, rq)) != BLU_OK) return rc;
    const std::vector<size_t> at = d.offsets();
    const size_t total = at.back();
    char* buf = (char*)malloc(total + 1);
    if (!buf) { set_error("out of memory"); return BLU_ERR_ALLOC; }
    parallel_dynamic(d.pieces.size(), total < (1u << 24) ? 1 : worker_threads(),
                     [&](size_t k) { memcpy(buf + at[k], d.pieces[k].data(), d.pieces[k].size()); });
    buf[total] = 0;
    outcome->text = buf;
    outcome->text_len = total;
    return BLU_OK;
}

// (the report and table files, when asked for, are written once the document is out)
int consensus_to_file(const blu_consensus_request& rq, const blu_consensus_extras* ex, const blu_table_layout* lay, const blu_query_cover* cov,
                      blu_consensus_outcome* outcome) {
    const char* const out_path = rq.out_path;
    Document d;
    int rc = build_document(rq, ex, lay, cov, &d, outcome);
    if (rc != BLU_OK) return rc;
    if (getenv("BLU_INGEST_TRACE")) fprintf(stderr, "[pipeline] %-26s %.3f s\n", "tear-down (tables, strings)", now_s() - g_t_body_end);
    if (d.written) return put_tables(d, rq);
    // (YAML: one piece, written here) write_blutils_output.rs:57-63: an existing file is replaced
    Trace tr;
    const int fd = open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { set_error("cannot write %s", out_path); return BLU_ERR_IO; }
    const std::vector<size_t> at = d.offsets();
    std::atomic<bool> ok{true};
    parallel_dynamic(d.pieces.size(), at.back() < (1u << 24) ? 1 : std::min(worker_threads(), 16u), [&](size_t k) {
        const char* p = d.pieces[k].data();
        size_t left = d.pieces[k].size(), off = at[k];
        while (left && ok.load(std::memory_order_relaxed)) {
            const ssize_t w = pwrite(fd, p, left, (off_t)off);
            if (w < 0) { if (errno == EINTR) continue; ok = false; break; }
            p += w; left -= (size_t)w; off += (size_t)w;
        }
    });
    if (close(fd) != 0 || !ok) { set_error("cannot write %s", out_path); return BLU_ERR_IO; }
    tr.lap("write file");
    return put_tables(d, rq);
}

}  // namespace
}  // namespace blu

using namespace blu;

extern "C" {

int blu_build_consensus(const blu_consensus_request* request, blu_consensus_outcome* outcome) {
    return blu_build_consensus_with(request, nullptr, outcome);
}

int blu_build_consensus_with(const blu_consensus_request* request, const blu_consensus_extras* extras, blu_consensus_outcome* outcome) {
    return blu_build_consensus_laid_out(request, extras, nullptr, outcome);
}

int blu_build_consensus_laid_out(const blu_consensus_request* request, const blu_consensus_extras* extras, const blu_table_layout* layout,
                                 blu_consensus_outcome* outcome) {
    return blu_build_consensus_covered(request, extras, layout, nullptr, outcome);
}

int blu_build_consensus_covered(const blu_consensus_request* request, const blu_consensus_extras* extras, const blu_table_layout* layout,
                                const blu_query_cover* cover, blu_consensus_outcome* outcome) {
    g_cover_pending = g_last_min_cover = blu_min_cover_stats{};
    if (!request || !outcome) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    if (extras) {
        if (extras->struct_size != sizeof(blu_consensus_extras)) {
            set_error("blu_build_consensus_with: struct_size %u is not a blu_consensus_extras this library knows (%zu bytes)", extras->struct_size,
                      sizeof(blu_consensus_extras));
            return BLU_ERR_INVALID_ARG;
        }
        if (extras->count_table_stats) *extras->count_table_stats = blu_count_table_stats{};
    }
    if (request->struct_size != sizeof(blu_consensus_request)) {
        set_error("blu_build_consensus: struct_size %u is not a blu_consensus_request this library knows (%zu bytes)", request->struct_size,
                  sizeof(blu_consensus_request));
        return BLU_ERR_INVALID_ARG;
    }
    outcome->text = nullptr; outcome->text_len = 0; outcome->stats = blu_pipeline_stats{};   // (outcome->selection: by Selection)
    try {
        const int rc = request->out_path ? consensus_to_file(*request, extras, layout, cover, outcome) : consensus_to_text(*request, extras, layout, cover, outcome);
        if (rc == BLU_OK) g_last_min_cover = g_cover_pending;
        return rc;
    }
    catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }   // (no exception crosses the C ABI)
}

// the reference's three signatures: the fields they name, everything else absent
static int build_as_the_reference(const char* blast_output_file, const char* const* headers, uint64_t n_headers, const char* taxonomies_file,
                                  const blu_pipeline_params* params, const char* run_id_text, const char* config_text, const char* out_path,
                                  char** out_text, size_t* out_len, blu_pipeline_stats* stats) {
    if (!out_path && !out_text) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    blu_consensus_request rq{};
    rq.struct_size = sizeof rq;
    rq.blast_output_file = blast_output_file; rq.headers = headers; rq.n_headers = n_headers; rq.taxonomies_file = taxonomies_file;
    rq.params = params; rq.run_id_text = run_id_text; rq.config_text = config_text; rq.out_path = out_path;
    blu_consensus_outcome oc{};
    const int rc = blu_build_consensus(&rq, &oc);
    if (out_text) *out_text = oc.text;
    if (out_len) *out_len = oc.text_len;
    if (stats && rc == BLU_OK) *stats = oc.stats;
    return rc;
}

int blu_build_consensus_identities(const char* blast_output_file, const char* const* headers, uint64_t n_headers,
                                   const char* taxonomies_file, const blu_pipeline_params* params, char** out_text,
                                   size_t* out_len, blu_pipeline_stats* stats) {
    return build_as_the_reference(blast_output_file, headers, n_headers, taxonomies_file, params, nullptr, nullptr, nullptr, out_text, out_len, stats);
}

int blu_build_consensus_identities_cfg(const char* blast_output_file, const char* const* headers, uint64_t n_headers,
                                       const char* taxonomies_file, const blu_pipeline_params* params,
                                       const char* run_id_text, const char* config_text, char** out_text, size_t* out_len,
                                       blu_pipeline_stats* stats) {
    return build_as_the_reference(blast_output_file, headers, n_headers, taxonomies_file, params, run_id_text, config_text, nullptr, out_text, out_len, stats);
}

int blu_build_consensus_identities_to_file(const char* blast_output_file, const char* const* headers, uint64_t n_headers,
                                           const char* taxonomies_file, const blu_pipeline_params* params,
                                           const char* run_id_text, const char* config_text, const char* out_path,
                                           blu_pipeline_stats* stats) {
    if (!out_path) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    return build_as_the_reference(blast_output_file, headers, n_headers, taxonomies_file, params, run_id_text, config_text, out_path, nullptr, nullptr, stats);
}

void blu_free_text(char* text) { free(text); }

int blu_last_min_cover_stats(blu_min_cover_stats* out) {
    if (!out) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    *out = g_last_min_cover;
    return BLU_OK;
}

}  // extern "C"
